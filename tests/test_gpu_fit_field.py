"""ucf_fit_create_field on the GPU against the oracle (fixtures: tools/gen_fit_field_fixture.py).

The field: pumping wells P0 (origin, q = 1, t0 = 0), P1 (q = 0.6, t0 = 20) and the constant-head image of P0 (q = -1);
observation wells A (one depth, 66 times: two blocks towards P0 and the image, fewer times towards P1), B (three depths,
screen average at 6 times and once its middle depth alone), C (4 times, all before P1 starts) and D that no observation
names; observations in a shuffled order.  Deck neuman74_partpen, free = Kr, Sy -- the shared launch sequence -- and deck
c1_theis, free = Kr, Ss -- plan by plan and virtual well by virtual well.

No tolerance is new.  Per stored value b = gate() of tests/test_gpu_fit.py; a screen-averaged term gets the weights of the
average applied to the b of its depths (tests/test_gpu_fit_network.py); an observation is a sum over pumping wells of q_j
x term, so its bound is sum_j |q_j| b_j.  Sums are held to (n + 4) u sum|terms|, parameters to the first-order displacement
of a least-squares minimiser under data errors bounded by b.  Everything else here is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_fit import NAN_R, NAN_T, U, check_sums, gate, recomputed
from test_gpu_fit_network import LM, average, wells_of

pytestmark = pytest.mark.gpu

PROBLEMS = ["neuman74", "theis"]


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def obs_wells_of(fx):
    out, at = [], 0
    for x, y, n in zip(fx["well_x"], fx["well_y"], fx["well_nz"]):
        out.append((float(x), float(y), fx["well_z"][at:at + n].copy()))
        at += n
    return out


def per_term(fx, values):
    """[..., entries] of the fixture's value list -> [..., nterm]: what each term reads, averaged where it is a screen"""
    return np.stack([average(values[..., a:a + n]) for a, n in zip(fx["e_first"], fx["e_count"])], axis=-1)


def superposed(fx, terms, q):
    """[..., nterm] -> [..., nobs]: acc = 0; acc = acc + q * term over the terms of each observation, in their order"""
    out = np.zeros(terms.shape[:-1] + (len(fx["t"]),))
    for i in range(len(fx["t"])):
        for k in range(fx["term_first"][i], fx["term_first"][i + 1]):
            out[..., i] = out[..., i] + q[fx["term_pump"][k]] * terms[..., k]
    return out


_cache = {}


def problem(ufit, key):
    """(fixture, deck parameters, field Fit with unit weights, reference per observation, bound per observation)"""
    if key not in _cache:
        fx = np.load(os.path.join(GOLD, f"fit_field_{key}.npz"))
        _, _, P = load_deck(str(fx["deck"]))
        f = ufit.Fit.field(P, [str(n) for n in fx["free"]], fx["pump"], obs_wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"])
        q = fx["pump"][:, 2]
        ref = superposed(fx, per_term(fx, fx["ref"]), q)
        bound = superposed(fx, per_term(fx, gate(fx["ref"], fx["noise"])), np.abs(q))
        _cache[key] = (fx, P, f, ref, bound)
    return _cache[key]


def evaluated(ufit, key):
    if (key, "eval") not in _cache:
        fx, _, f, _, _ = problem(ufit, key)
        _cache[(key, "eval")] = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), jacobian=True, sim_all=True)
    return _cache[(key, "eval")]


def plan_rows(fx):
    """the parameter sets of the plans of one evaluate of the fixture's sets, in plan order"""
    dlog, out = float(fx["eval_dlog"]), []
    for th in fx["eval_theta"]:
        out.append(np.array(th))
        for j in range(len(th)):
            for fac in (np.exp(dlog), np.exp(-dlog)):
                x = np.array(th); x[j] = x[j] * fac
                out.append(x)
    return out


@pytest.mark.parametrize("key", PROBLEMS)
def test_values_against_the_oracle(ufit, key):
    """every row of sim_all -- base and perturbed plans, one, two and three terms, point observations and screen averages,
    in the caller's order -- within sum_j |q_j| b_j of the oracle's superposition at the same parameters"""
    fx, _, f, ref, bound = problem(ufit, key)
    out = evaluated(ufit, key)
    assert np.isfinite(fx["ref"]).all() and np.isfinite(fx["noise"]).all()
    err = np.abs(out["sim_all"] - ref)
    nterm = np.diff(fx["term_first"])
    print(f"[fit field {key}] worst |sim - oracle| / bound = {float((err / bound).max()):.3f} "
          f"(three terms: {float((err / bound)[..., nterm == 3].max()):.3f}, screens: {float((err / bound)[..., fx['iz'] < 0].max()):.3f})")
    assert (out["nbad"] == 0).all()
    assert (err <= bound).all(), (key, float((err / bound).max()))
    # what the fit launches is the network of its virtual wells
    virt_nz = np.ascontiguousarray(fx["well_nz"][fx["virt_well"]], np.int32)
    a, b = C.c_longlong(), C.c_longlong()
    assert f._lib.ucf_fit_network_eval_counts(len(virt_nz), virt_nz, len(fx["term_t"]), fx["term_t"], fx["term_virt"], C.byref(a), C.byref(b)) == 0
    assert f.eval_counts() == (a.value, b.value)


@pytest.mark.parametrize("key", PROBLEMS)
def test_one_well_at_the_origin_is_the_network_fit_bit_for_bit(ufit, key):
    """one pumping well at the origin with q = 1 and t0 = 0, the network fixture's wells at (r, 0): sqrt(r r) = r, t - 0 = t and
    0 + 1 v = v, so points, blocks and split vector are those of Fit.network and every output has the same bytes"""
    fx = np.load(os.path.join(GOLD, f"fit_network_{key}.npz"))
    _, _, P = load_deck(str(fx["deck"]))
    free = [str(n) for n in fx["free"]]
    w = 1.0 + 0.5 * np.cos(np.arange(len(fx["t"])))
    net = ufit.Fit.network(P, free, wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"], weight=w)
    fld = ufit.Fit.field(P, free, [(0.0, 0.0, 1.0, 0.0)], [(r, 0.0, z) for r, z in wells_of(fx)], fx["t"], fx["well"], fx["iz"], fx["obs"],
                         weight=w)
    assert fld.eval_counts() == net.eval_counts()
    a = net.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), jacobian=True, sim_all=True)
    b = fld.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), jacobian=True, sim_all=True)
    assert np.isfinite(a["sim_all"]).all() and (a["sim_all"] != 0).any()
    for k in ("phi", "g", "A", "J", "sim_all", "nbad"):
        assert a[k].tobytes() == b[k].tobytes(), k
    net.close(); fld.close()


def test_exact_cancellation(ufit):
    """wells at (-d, 0) and (+d, 0) with q = +1 and -1 and one start, observation well on the y axis: both lie at the same
    distance, the fit has ONE virtual well, and every simulated value is (0 + v) + (-v) = +0.0 -- in every row, so J is 0"""
    _, _, P = load_deck("neuman74_partpen")
    wells = [(-30.0, 0.0, 1.0, 2.0), (30.0, 0.0, -1.0, 2.0)]
    t = np.array([1.0, 2.0, 5.0, 50.0, 500.0, 50.0])           # before the start, at the start (no term), after it
    iz = np.array([0, 1, -1, 0, 2, -1], np.int32)
    f = ufit.Fit.field(P, ["Kr", "Sy"], wells, [(0.0, 40.0, [105.0, 123.0, 141.0])], t, np.zeros(6, np.int32), iz, np.full(6, 0.25))
    assert f.eval_counts() == (64 * 3, 3 * 3)                   # one block of one virtual well; 3 distinct times x 3 depths
    th = np.array([[P.Kr, P.Sy], [1.3 * P.Kr, 0.9 * P.Sy]])
    out = f.evaluate(th, 1e-3, jacobian=True, sim_all=True)
    assert np.isfinite(f.debug_h(0, 0)).all() and f.debug_h(0, 0)[0] != 0.0       # the terms themselves are not 0
    assert out["sim_all"].tobytes() == np.zeros((2, 5, 6)).tobytes()              # +0.0, sign included
    assert (out["J"] == 0.0).all() and (out["nbad"] == 0).all()
    assert (out["g"] == 0.0).all() and (out["A"] == 0.0).all()
    assert out["phi"].tolist() == [6 * 0.0625, 6 * 0.0625]
    f.close()


def test_the_sum_is_the_stated_arithmetic(ufit):
    """each term's dimensionless h read back from the device (ucf_fit_debug_h takes a term index), the recurrence of
    include/ucf.h redone in numpy one rounded operation at a time -- screen average, q x v, the running sum, x Hc -- and
    compared with sim_all byte for byte: observations with one pumping well skipped and screen-averaged ones included"""
    from unconfined_amd import lib as ucflib
    fx, P, f, _, _ = problem(ufit, "neuman74")
    lib = ucflib.load()
    out = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), sim_all=True)      # debug_h reads the LAST evaluation
    sim = out["sim_all"].reshape(-1, len(fx["t"]))
    q = fx["pump"][:, 2]
    first = fx["term_first"]
    nterm = np.diff(first)
    assert (nterm[fx["iz"] < 0] == 2).any() and (nterm[fx["iz"] < 0] == 3).any() and (nterm[fx["iz"] >= 0] == 2).any()
    for k, th in enumerate(plan_rows(fx)):
        D = ucflib.UcfDerived()
        ucflib.check(lib.ucf_nondimensionalise(C.byref(ufit.perturb(P, [str(x) for x in fx["free"]], th)), C.byref(D)))
        Hc = np.float64(D.Hc)
        for i in range(len(fx["t"])):
            acc = np.float64(0.0)
            for m in range(first[i], first[i + 1]):
                v = f.debug_h(k, m)
                assert len(v) == fx["e_count"][m]
                n = len(v)
                if n > 1:
                    s = v[1]
                    for j in range(2, n):
                        s = s + v[j]
                    v = ((v[0] + np.float64(2.0) * s) + v[n - 1]) / np.float64(2 * n)
                else:
                    v = v[0]
                acc = acc + q[fx["term_pump"][m]] * v
            want = np.array([acc * Hc])
            assert want.tobytes() == sim[k, i:i + 1].tobytes(), (k, i, want, sim[k, i])


def test_against_the_forward_map(ufit):
    """P0 and its NO-FLOW image, both from t = 0: the field has one group and its split vector is taken over the same times
    as the fit's, so ucf_field_drawdown in the fast flavour at the observation wells and the distinct observation times is
    the same model evaluated through the grid path.  Row 0 of sim_all agrees with it within twice the bound of the values
    test for these two wells (b of the P0 term + b of the image term: same distances and times as in the fixture)"""
    from unconfined_amd import engine as eng
    from unconfined_amd.field import WellField
    fx, P, _, _, _ = problem(ufit, "neuman74")
    assert np.array_equal(fx["eval_theta"][0], fx["theta_star"])
    wells = fx["pump"][[0, 2]].copy()
    wells[1, 2] = 1.0
    assert (wells[:, 3] == 0.0).all()
    f = ufit.Fit.field(P, [str(n) for n in fx["free"]], wells, obs_wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"])
    sim = f.evaluate(fx["theta_star"], float(fx["eval_dlog"]), sim_all=True)["sim_all"][0, 0]
    times = np.unique(fx["t"])
    plan = eng.Plan(P, mode="fast")
    field = WellField(wells, np.stack([fx["well_x"], fx["well_y"]], axis=1), times)
    assert field.group_count() == 1
    s, _ = field.drawdown(plan, fx["well_z"])
    z0 = np.concatenate([[0], np.cumsum(fx["well_nz"])])
    b = per_term(fx, gate(fx["ref"][0, 0], fx["noise"][0, 0]))
    worst = 0.0
    for i in range(len(fx["t"])):
        w, k = fx["well"][i], int(np.searchsorted(times, fx["t"][i]))
        col = s[k, w, z0[w]:z0[w + 1]]
        fwd = average(col) if fx["iz"][i] < 0 else col[fx["iz"][i]]
        terms = np.arange(fx["term_first"][i], fx["term_first"][i + 1])
        lim = 2.0 * sum(b[m] for m in terms if fx["term_pump"][m] in (0, 2))
        worst = max(worst, abs(sim[i] - fwd) / lim)
        assert abs(sim[i] - fwd) <= lim, (i, sim[i], fwd, lim)
    print(f"[fit field] against ucf_field_drawdown: worst |difference| / 2b = {worst:.3f}")
    f.close()


def test_sums_and_determinism(ufit):
    """weights that are not 1: every sum within (nobs + 4) u sum|terms| of the np.longdouble value recomputed from sim_all, J
    within 2 ulp; the same call twice gives identical bits and allocates nothing the second time"""
    fx, P, _, _, _ = problem(ufit, "neuman74")
    n = len(fx["obs"])
    w = 1.0 + 0.5 * np.sin(np.arange(n))
    f = ufit.Fit.field(P, [str(x) for x in fx["free"]], fx["pump"], obs_wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"], weight=w)
    dlog = float(fx["eval_dlog"])
    a = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    count = f.alloc_count()
    b = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    assert count > 0 and f.alloc_count() == count
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


def test_a_nonfinite_term_is_counted_and_left_out(ufit, oracle):
    """one more observation well whose term towards P0 lies where the oracle gives NaN (tests/test_gpu_fit.py): nothing is
    scrubbed, the sum is not finite, nbad counts exactly that observation and the sums are those of the others"""
    fx, P, _, ref, bound = problem(ufit, "neuman74")
    D = oracle.nondim(P)
    zD = np.array([145.7]) / D.Lc
    ho, _ = oracle.batch(P, np.array([NAN_T / D.Tc]), np.array([NAN_R / D.Lc]), np.array([1], np.int32), zD, oracle.zlay(D, zD))
    assert np.isnan(ho[0, 0]), ho                      # the oracle alone
    n = len(fx["obs"])
    obs_wells = obs_wells_of(fx) + [(NAN_R, 0.0, [145.7])]
    t, well = np.append(fx["t"], NAN_T), np.append(fx["well"], len(obs_wells) - 1)
    iz, obs = np.append(fx["iz"], 0), np.append(fx["obs"], 1.0)
    f = ufit.Fit.field(P, [str(x) for x in fx["free"]], fx["pump"], obs_wells, t, well, iz, obs)
    dlog = float(fx["eval_dlog"])
    out = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    assert (out["nbad"] == 1).all(), out["nbad"]
    assert not np.isfinite(out["sim_all"][:, 0, n]).any()
    assert np.isfinite(out["sim_all"][:, :, :n]).all()
    assert np.isfinite(out["phi"]).all() and np.isfinite(out["g"]).all() and np.isfinite(out["A"]).all()
    keep = np.arange(n + 1) < n
    for s in range(len(fx["eval_theta"])):
        check_sums(out, s, recomputed(out["sim_all"][s], obs, np.ones(n + 1), dlog, keep), n + 1)
    # measured, not gated: the new earliest time moves every plan's split vector, the other observations move with it
    print(f"[fit field] others against the oracle of the field without it: worst / bound = "
          f"{float((np.abs(out['sim_all'][:, :, :n] - ref) / bound).max()):.3f}")
    f.close()


def test_lm_recovers_theta_star(ufit):
    """two starts in one lm call on the oracle's noise-free superposition at theta_star: both converge, |ln theta_hat - ln
    theta_star| within 2 sum_i |(A^-1 J')_ji| b_i, the first-order displacement of the minimiser under data errors bounded by
    b (derived in tests/test_gpu_fit_network.py).  cov = phi / (nobs - npar) A^-1 comes column by column from Cholesky solves
    of a symmetric matrix: finite, and symmetric to the backward error of such a solve, 8 u cond(A) max|cov|"""
    from unconfined_amd import abi
    fx, _, f, _, bound = problem(ufit, "neuman74")
    b = bound[0, 0]                     # set 0, row 0 of the fixture is theta_star itself
    assert np.array_equal(fx["eval_theta"][0], fx["theta_star"])
    res = f.lm(fx["starts"], **LM)
    print(f"[fit field] iterations {res['iters'].tolist()}, phi / sum b^2 = {(res['phi'] / np.sum(b * b)).max():.3e}")
    assert (res["status"] == abi.FIT_CONVERGED).all(), res["status"]
    for s in range(len(fx["starts"])):
        out = f.evaluate(res["theta"][s], LM["dlog"], jacobian=True)
        lim = 2.0 * np.abs(np.linalg.solve(out["A"][0], out["J"][0].T)) @ b
        err = np.abs(np.log(res["theta"][s]) - np.log(fx["theta_star"]))
        print(f"[fit field] start {s}: |ln theta_hat - ln theta_star| / bound = {(err / lim).tolist()}")
        assert (err <= lim).all(), (s, err, lim)
        cov = res["cov"][s]
        assert np.isfinite(cov).all() and (np.diag(cov) > 0).all()
        assert (np.abs(cov - cov.T) <= 8 * U * np.linalg.cond(out["A"][0]) * np.abs(cov).max()).all(), cov
