"""ucf_fit_create_network on the GPU against the oracle (fixtures: tools/gen_fit_network_fixture.py).

The network: piezometer A (5 times, below the screen, the largest radius of its group), piezometer B (70 times, above the
screen: two blocks, the second padded), screened well C (9 times, three depths, observed as their screen average and once at
its middle depth alone) and well D that no observation names; observations in a shuffled order.  Deck neuman74_partpen, free
= Kr, Sy -- the shared launch sequence, blocks = (plan, well) tiles -- and deck c1_theis, free = Kr, Ss -- plan by plan and
well by well.

Every bound is derived as in tests/test_gpu_fit.py: per value b = max(1e-10, 10 x the oracle's distance from its binary128
build) x max(|ref|, 1e-3); a screen-averaged observation gets the weights of the average applied to the b of its depths;
sums are held to (n + 4) u sum|terms|; parameters to the first-order displacement of a least-squares minimiser under data
errors bounded by b."""
import ctypes as C
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_fit import NAN_R, NAN_T, U, check_sums, gate, recomputed

pytestmark = pytest.mark.gpu

PROBLEMS = ["neuman74", "theis"]
LM = dict(max_iter=60, dlog=1.0e-3, lambda0=1.0e-2, lambda_up=10.0, lambda_down=0.1, tol_step=1.0e-8, tol_phi=1.0e-9)


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def wells_of(fx):
    out, at = [], 0
    for r, n in zip(fx["well_r"], fx["well_nz"]):
        out.append((float(r), fx["well_z"][at:at + n].copy()))
        at += n
    return out


def average(v):
    """the rule of ucf_screen_average along the last axis (any weights >= 0: it maps bounds to the bound of the average)"""
    n = v.shape[-1]
    if n == 1:
        return v[..., 0]
    s = v[..., 1]
    for j in range(2, n):
        s = s + v[..., j]
    return ((v[..., 0] + 2.0 * s) + v[..., n - 1]) / (2 * n)


def per_observation(fx, values):
    """[..., entries] of the fixture's value list -> [..., nobs]: what each observation reads, averaged where it is a screen"""
    return np.stack([average(values[..., a:a + n]) for a, n in zip(fx["e_first"], fx["e_count"])], axis=-1)


_cache = {}


def problem(ufit, key):
    """(fixture, deck parameters, network Fit with unit weights, reference per observation, bound per observation)"""
    if key not in _cache:
        fx = np.load(os.path.join(GOLD, f"fit_network_{key}.npz"))
        _, _, P = load_deck(str(fx["deck"]))
        f = ufit.Fit.network(P, [str(n) for n in fx["free"]], wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"])
        ref = per_observation(fx, fx["ref"])
        bound = per_observation(fx, gate(fx["ref"], fx["noise"]))
        _cache[key] = (fx, P, f, ref, bound)
    return _cache[key]


def evaluated(ufit, key):
    if (key, "eval") not in _cache:
        fx, _, f, _, _ = problem(ufit, key)
        _cache[(key, "eval")] = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), jacobian=True, sim_all=True)
    return _cache[(key, "eval")]


@pytest.mark.parametrize("key", PROBLEMS)
def test_values_against_the_oracle(ufit, key):
    """every row of sim_all -- base and perturbed plans, point observations and screen averages, in the caller's order --
    within b of the oracle at the same parameters"""
    fx, _, _, ref, bound = problem(ufit, key)
    out = evaluated(ufit, key)
    assert np.isfinite(fx["ref"]).all()
    err = np.abs(out["sim_all"] - ref)
    print(f"[fit network {key}] worst |sim - oracle| / b = {float((err / bound).max()):.3f} "
          f"(screens: {float((err / bound)[..., fx['e_count'] > 1].max()):.3f})")
    assert (out["nbad"] == 0).all()
    assert (err <= bound).all(), (key, float((err / bound).max()))


def test_screen_average_is_the_stated_arithmetic(ufit):
    """A second fit observes the three depths of C as three point observations per time; it names the same (well, time)
    points, so both fits launch identical blocks and the h behind them is identical, bit for bit (asserted).  The averaged
    observation of the first fit is ucf_screen_average of that dimensionless h, times Hc of the plan -- bit for bit.

    The comparison is made on the h read back from the device (ucf_fit_debug_h) because that is what the kernel averages:
    sim_all / Hc is NOT h bit for bit (h x Hc / Hc rounds twice), so ucf_screen_average of the second fit's sim_all / Hc rows
    is held to the first fit only within (n + 2) u sum|terms| -- n - 1 additions, the doubling and the division are exact or
    one rounding each, plus the two roundings of x Hc / Hc per term."""
    from unconfined_amd import lib as ucflib
    fx, P, f1, _, _ = problem(ufit, "neuman74")
    lib = ucflib.load()
    screens = np.flatnonzero(fx["iz"] == -1)
    n = 3
    points = np.flatnonzero(fx["iz"] >= 0)
    t2 = np.concatenate([fx["t"][points], np.repeat(fx["t"][screens], n)])
    w2 = np.concatenate([fx["well"][points], np.repeat(fx["well"][screens], n)]).astype(np.int32)
    iz2 = np.concatenate([fx["iz"][points], np.tile(np.arange(n), len(screens))]).astype(np.int32)
    f2 = ufit.Fit.network(P, [str(x) for x in fx["free"]], wells_of(fx), t2, w2, iz2, np.ones(len(t2)))
    assert f2.eval_counts() == f1.eval_counts()
    dlog = float(fx["eval_dlog"])
    a = f1.evaluate(fx["eval_theta"], dlog, sim_all=True)["sim_all"]
    b = f2.evaluate(fx["eval_theta"], dlog, sim_all=True)["sim_all"]
    nplans = a.shape[0] * a.shape[1]
    a, b = a.reshape(nplans, -1), b.reshape(nplans, -1)
    rows = []
    for th in fx["eval_theta"]:
        rows.append(th)
        for j in range(len(th)):
            for fac in (np.exp(dlog), np.exp(-dlog)):
                x = np.array(th); x[j] = x[j] * fac
                rows.append(x)
    worst = 0.0
    for k in range(nplans):
        D = ucflib.UcfDerived()
        ucflib.check(lib.ucf_nondimensionalise(C.byref(ufit.perturb(P, [str(x) for x in fx["free"]], rows[k])), C.byref(D)))
        for q, i in enumerate(screens):
            h1 = f1.debug_h(k, i)
            at = len(points) + q * n
            h2 = np.array([f2.debug_h(k, at + j)[0] for j in range(n)])
            assert h1.tobytes() == h2.tobytes(), (k, i, h1, h2)
            avg = np.zeros(1)
            ucflib.check(lib.ucf_screen_average(1, n, np.ascontiguousarray(h1), avg))
            assert (avg * D.Hc).tobytes() == a[k, i:i + 1].tobytes(), (k, i, avg * D.Hc, a[k, i])
            assert (h2 * D.Hc).tobytes() == b[k, at:at + n].tobytes()
            # the weaker statement on sim_all alone
            v = np.ascontiguousarray(b[k, at:at + n] / D.Hc)
            ucflib.check(lib.ucf_screen_average(1, n, v, avg))
            terms = (abs(v[0]) + 2 * np.abs(v[1:n - 1]).sum() + abs(v[n - 1])) / (2 * n) * D.Hc
            worst = max(worst, abs(avg[0] * D.Hc - a[k, i]) / ((n + 2) * U * terms))
            assert abs(avg[0] * D.Hc - a[k, i]) <= (n + 2) * U * terms
    print(f"[fit network] screen average from sim_all / Hc: worst error / bound = {worst:.3f}")
    f2.close()


def test_reduction_is_the_arithmetic_it_claims(ufit):
    """as the test of that name for ucf_fit_create: J within 2 ulp, every sum within (nobs + 4) u sum|terms| of the
    np.longdouble value recomputed from sim_all, weights that are not 1; the same call twice gives identical bits"""
    fx, P, _, _, _ = problem(ufit, "neuman74")
    n = len(fx["obs"])
    w = 1.0 + 0.5 * np.sin(np.arange(n))
    f = ufit.Fit.network(P, [str(x) for x in fx["free"]], wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"], weight=w)
    dlog = float(fx["eval_dlog"])
    a = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    b = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["nbad"] == 0).all() and np.isfinite(a["sim_all"]).all()
    for s in range(len(fx["eval_theta"])):
        sim = a["sim_all"][s]
        ref = recomputed(sim, fx["obs"], w, dlog)
        for j in range(f.npar):
            big = np.maximum(np.abs(sim[1 + 2 * j]), np.abs(sim[2 + 2 * j])) / (2 * dlog)
            assert (np.abs(a["J"][s][:, j].astype(np.longdouble) - ref["J"][:, j]) <= 2 * np.spacing(big)).all(), (s, j)
        check_sums(a, s, ref, n)
    f.close()


def test_against_the_dense_path(ufit):
    """ucf_fit_create on the same points with the union of all depths of the network (a screen average becomes one point
    observation per depth, averaged here): within 2 b per observation -- not bit for bit, the shared launch picks its
    instantiation from the union of the blocks -- while the network form launches fewer (point, depth) evaluations"""
    fx, P, f, _, bound = problem(ufit, "neuman74")
    z0 = np.concatenate([[0], np.cumsum(fx["well_nz"])])
    t, r, iz = [], [], []
    for i in range(len(fx["t"])):
        w = fx["well"][i]
        depths = range(fx["well_nz"][w]) if fx["iz"][i] < 0 else [fx["iz"][i]]
        for j in depths:
            t.append(fx["t"][i]); r.append(fx["well_r"][w]); iz.append(z0[w] + j)
    dense = ufit.Fit(P, [str(x) for x in fx["free"]], t, r, fx["well_z"], np.array(iz, np.int32), np.ones(len(t)))
    sim = dense.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), sim_all=True)["sim_all"]
    first = np.concatenate([[0], np.cumsum(np.where(fx["iz"] < 0, fx["well_nz"][fx["well"]], 1))])
    sim = np.stack([average(sim[..., first[i]:first[i + 1]]) for i in range(len(fx["t"]))], axis=-1)
    net = evaluated(ufit, "neuman74")["sim_all"]
    err = np.abs(net - sim)
    print(f"[fit network] network against dense: worst |difference| / 2b = {float((err / (2 * bound)).max()):.3f}")
    assert (err <= 2 * bound).all(), float((err / (2 * bound)).max())
    launched, all_depths = f.eval_counts()
    assert (launched, all_depths) == ufit.network_eval_counts(wells_of(fx), fx["t"], fx["well"])
    assert launched < all_depths
    d_launched, d_dense = dense.eval_counts()
    assert d_launched == d_dense == len(t) * len(fx["well_z"])
    dense.close()


@pytest.mark.parametrize("key", PROBLEMS)
def test_lm_recovers_theta_star(ufit, key):
    """two starts in one lm call on the oracle's noise-free observations at theta_star: both converge, phi <= sum b^2 (the
    device at theta_star itself cannot exceed that and the minimiser lies below), |ln theta_hat - ln theta_star| within
    2 sum_i |(A^-1 J')_ji| b_i, the first-order displacement of the minimiser under data errors bounded by b"""
    from unconfined_amd import abi
    fx, _, f, _, bound = problem(ufit, key)
    b = bound[0, 0]                     # set 0, row 0 of the fixture is theta_star itself
    assert np.array_equal(fx["eval_theta"][0], fx["theta_star"])
    res = f.lm(fx["starts"], **LM)
    print(f"[fit network {key}] iterations {res['iters'].tolist()}, phi / sum b^2 = {(res['phi'] / np.sum(b * b)).max():.3e}")
    assert (res["status"] == abi.FIT_CONVERGED).all(), res["status"]
    assert (res["phi"] <= np.sum(b * b)).all(), (res["phi"], float(np.sum(b * b)))
    for s in range(len(fx["starts"])):
        out = f.evaluate(res["theta"][s], LM["dlog"], jacobian=True)
        lim = 2.0 * np.abs(np.linalg.solve(out["A"][0], out["J"][0].T)) @ b
        err = np.abs(np.log(res["theta"][s]) - np.log(fx["theta_star"]))
        assert (err <= lim).all(), (key, s, err, lim)
        assert np.isfinite(res["cov"][s]).all() and (np.diag(res["cov"][s]) > 0).all()


def test_nonfinite_observation_is_left_out_and_counted(ufit, oracle):
    """one more piezometer at the point where the oracle gives NaN (tests/test_gpu_fit.py): nbad = 1, the sums are those of
    the network without it, nothing faults"""
    fx, P, _, ref, bound = problem(ufit, "neuman74")
    D = oracle.nondim(P)
    zD = np.array([145.7]) / D.Lc
    ho, _ = oracle.batch(P, np.array([NAN_T / D.Tc]), np.array([NAN_R / D.Lc]), np.array([1], np.int32), zD, oracle.zlay(D, zD))
    assert np.isnan(ho[0, 0]), ho                      # the oracle alone
    n = len(fx["obs"])
    wells = wells_of(fx) + [(NAN_R, [145.7])]
    t, well = np.append(fx["t"], NAN_T), np.append(fx["well"], len(wells) - 1)
    iz, obs = np.append(fx["iz"], 0), np.append(fx["obs"], 1.0)
    f = ufit.Fit.network(P, [str(x) for x in fx["free"]], wells, t, well, iz, obs)
    dlog = float(fx["eval_dlog"])
    out = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    assert (out["nbad"] == 1).all(), out["nbad"]
    assert not np.isfinite(out["sim_all"][:, 0, n]).any()
    assert np.isfinite(out["phi"]).all() and np.isfinite(out["g"]).all() and np.isfinite(out["A"]).all()
    keep = np.arange(n + 1) < n
    for s in range(len(fx["eval_theta"])):
        check_sums(out, s, recomputed(out["sim_all"][s], obs, np.ones(n + 1), dlog, keep), n + 1)
        # ... and the other observations are the network without it
        assert (np.abs(out["sim_all"][s][:, :n] - ref[s]) <= bound[s]).all()
    f.close()


@pytest.mark.parametrize("key", PROBLEMS)
def test_repeated_evaluations_do_not_allocate(ufit, key):
    fx, P, _, _, _ = problem(ufit, key)
    f = ufit.Fit.network(P, [str(x) for x in fx["free"]], wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"])
    counts = []
    for i in range(10):
        f.evaluate(fx["eval_theta"] * (1.0 + 0.01 * i), 1e-3)
        counts.append(f.alloc_count())
    assert counts[0] > 0
    assert counts[1] == counts[9], counts
    f.close()
