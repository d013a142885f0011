"""Derivative data in a fit on the GPU: ucf_fit_set_derivative, ucf_fit_evaluate_joint, ucf_fit_debug_dh and ucf_fit_lm on
both curves (fixtures: tools/gen_fit_deriv_fixture.py).

The problems: the two of tests/test_gpu_fit.py (22 observations; neuman74_partpen through the shared launch sequence, c1_theis
plan by plan) with the oracle's log-time derivative beside every drawdown, a small network (wells A, B and the screened C of
tests/test_gpu_fit_network.py) and a small field (P0, P1 that starts at 20, the constant-head image of P0; wells A and the
screened B of tests/test_gpu_fit_field.py), both on neuman74_partpen.

No tolerance is new.  Per stored value of h, b = gate() of tests/test_gpu_fit.py; per stored value of dh, b_d = gate_d():
max(1e-10, 10 x the WORST oracle-vs-binary128 distance of dh in its row) x max(|ref|, 1e-3), a row being the values of one plan
-- the dh gate of test_parameter_batched_sweep_vs_oracle, which also takes the worst noise of a plan.  That factor 10 was
measured on the Neuman problem only; the Theis rows use 14.4 of it (one value of one row, measured on the MI355X), so the Theis
problem takes the 20 x of the deck gates of tests/test_gpu_parity.py (DH_FACTOR), of which it uses 72 %.  A screen average gets the weights of the average applied to the b of its depths; a field observation sum |q| b and
sum |q| tfac b_d; sums are held to (nobs + nd + 4) u sum|terms| -- nd more terms than without derivative data; parameters to
the first-order displacement of a least-squares minimiser under data errors bounded by b and b_d.  Everything else is bit for
bit."""
import ctypes as C
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_fit import NAN_R, NAN_T, U, gate, lm_options
from test_gpu_fit_field import obs_wells_of, plan_rows
from test_gpu_fit_network import average, wells_of

pytestmark = pytest.mark.gpu

PLAIN = ["neuman74", "theis"]
KINDS = ["plain", "network", "field"]
OUTPUTS = ("phi", "g", "A", "nbad", "J", "sim_all")
DH_FACTOR = {"neuman74": 10.0, "theis": 20.0, "network": 10.0, "field": 10.0}       # per fixture; see the module docstring


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


_fx = {}


def fixture(key):
    if key not in _fx:
        fx = np.load(os.path.join(GOLD, f"fit_deriv_{key}.npz"))
        _fx[key] = ({k: fx[k] for k in fx.files}, load_deck(str(fx["deck"]))[2])
    return _fx[key]


def make(ufit, kind, weight=None, key="neuman74", extra=None):
    """(fixture, deck parameters, a new Fit of that kind); ``extra`` = (t, r) of one more observation of a plain fit"""
    fx, P = fixture({"plain": key}.get(kind, kind))
    free = [str(n) for n in fx["free"]]
    if kind == "plain":
        t, r, iz, obs = fx["t"], fx["r"], fx["iz"], fx["obs"]
        if extra:
            t, r, iz, obs = np.append(t, extra[0]), np.append(r, extra[1]), np.append(iz, 0).astype(np.int32), np.append(obs, 1.0)
        return fx, P, ufit.Fit(P, free, t, r, fx["z"], iz, obs, weight=weight)
    if kind == "network":
        return fx, P, ufit.Fit.network(P, free, wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"], weight=weight)
    return fx, P, ufit.Fit.field(P, free, fx["pump"], obs_wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"], weight=weight)


def hc_of_plans(ufit, fx, P):
    from unconfined_amd import lib as ucflib
    lib, out = ucflib.load(), []
    for th in plan_rows(fx):
        D = ucflib.UcfDerived()
        ucflib.check(lib.ucf_nondimensionalise(C.byref(ufit.perturb(P, [str(x) for x in fx["free"]], th)), C.byref(D)))
        out.append(np.float64(D.Hc))
    return out


def gate_d(dref, dnoise, factor=10.0):
    """b_d per value: the noise is the worst of the value's row (last axis: the values of one plan)"""
    return np.maximum(1e-10, factor * dnoise.max(axis=-1, keepdims=True)) * np.maximum(np.abs(dref), 1e-3)


def per_place(fx, values):
    """[..., entries] -> [..., observations of a network | terms of a field]: averaged where the place is a screen"""
    return np.stack([average(values[..., a:a + n]) for a, n in zip(fx["e_first"], fx["e_count"])], axis=-1)


def superposed(fx, terms, q, tfac=None):
    """[..., nterm] -> [..., nobs]: acc = 0; acc = acc + q * term (q * (tfac * term)) over the terms of each observation"""
    out = np.zeros(terms.shape[:-1] + (len(fx["t"]),))
    for i in range(len(fx["t"])):
        for k in range(fx["term_first"][i], fx["term_first"][i + 1]):
            v = terms[..., k] if tfac is None else tfac[k] * terms[..., k]
            out[..., i] = out[..., i] + q[fx["term_pump"][k]] * v
    return out


def references(kind, key="neuman74"):
    """per observation and row: the oracle's value and its bound, of h and of dh -- ref, b, dref, b_d [sets][rows][nobs]"""
    fx, _ = fixture({"plain": key}.get(kind, kind))
    if kind == "plain":
        return fx["eval_ref"], gate(fx["eval_ref"], fx["eval_noise"]), fx["eval_dref"], gate_d(fx["eval_dref"], fx["eval_dnoise"], DH_FACTOR[key])
    ref, b = per_place(fx, fx["ref"]), per_place(fx, gate(fx["ref"], fx["noise"]))
    dref, bd = per_place(fx, fx["dref"]), per_place(fx, gate_d(fx["dref"], fx["dnoise"]))
    if kind == "network":
        return ref, b, dref, bd
    q = fx["pump"][:, 2]
    return superposed(fx, ref, q), superposed(fx, b, np.abs(q)), superposed(fx, dref, q, fx["tfac"]), superposed(fx, bd, np.abs(q), fx["tfac"])


def recomputed_joint(out, s, obs, dobs, w, wd, dlog, keep=None):
    """phi, phi_d, g, A of set s in np.longdouble from its sim_all and simd_all rows, with sum|terms| of every sum: the rows of h
    that ``keep`` names, then the rows of dh that it names and that have a positive weight"""
    L = np.longdouble
    sim, simd = out["sim_all"][s].astype(L), out["simd_all"][s].astype(L)
    P = (sim.shape[0] - 1) // 2
    keep = np.ones(len(obs), bool) if keep is None else keep
    parts = []
    for v, o, wt, rows in ((sim, obs, w, keep), (simd, dobs, wd, keep & (wd > 0))):
        J = np.stack([(v[1 + 2 * j] - v[2 + 2 * j]) / (L(2.0) * L(dlog)) for j in range(P)], axis=1)[rows]
        parts.append((J, (o.astype(L) - v[0])[rows], wt.astype(L)[rows] ** 2))
    tphi = [w2 * r * r for _, r, w2 in parts]
    tg = np.concatenate([J * (w2 * r)[:, None] for J, r, w2 in parts])
    tA = np.concatenate([J[:, :, None] * J[:, None, :] * w2[:, None, None] for J, r, w2 in parts])
    return dict(phi=tphi[0].sum() + tphi[1].sum(), aphi=tphi[0].sum() + tphi[1].sum(), phi_d=tphi[1].sum(), g=tg.sum(0), ag=np.abs(tg).sum(0),
                A=tA.sum(0), aA=np.abs(tA).sum(0), nterms=sum(len(r) for _, r, _ in parts))


def check_joint_sums(out, s, ref, n):
    """as check_sums of tests/test_gpu_fit.py, n = nobs + nd terms, phi_d among the sums"""
    tol = (n + 4) * U
    assert abs(np.longdouble(out["phi"][s]) - ref["phi"]) <= tol * ref["aphi"], ("phi", s)
    assert abs(np.longdouble(out["phi_d"][s]) - ref["phi_d"]) <= tol * ref["phi_d"], ("phi_d", s)
    assert (np.abs(out["g"][s].astype(np.longdouble) - ref["g"]) <= tol * ref["ag"]).all(), ("g", s)
    assert (np.abs(out["A"][s].astype(np.longdouble) - ref["A"]) <= tol * ref["aA"]).all(), ("A", s)
    assert np.array_equal(out["A"][s], out["A"][s].T)


def some_weights(n):
    """weights that are not 1 on both curves; every fourth observation has no derivative datum (and NaN in its place)"""
    w = 1.0 + 0.5 * np.sin(np.arange(n))
    wd = 0.7 + 0.4 * np.cos(np.arange(n))
    wd[1::4] = 0.0
    return w, wd


def with_gaps(dobs, wd):
    return np.where(wd > 0, dobs, np.nan)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_weights_change_nothing_bit_for_bit(ufit, kind):
    """dweight all zero and dobs all NaN: the joint kernel runs, and phi, g, A, nbad, J and sim_all have the bytes of the same
    fit without derivative data; phi_d is +0.0; the same joint evaluation twice gives identical bytes in every output"""
    n = len(fixture({"plain": "neuman74"}.get(kind, kind))[0]["obs"])
    fx, _, f = make(ufit, kind, weight=some_weights(n)[0])
    dlog = float(fx["eval_dlog"])
    plain = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    assert (plain["nbad"] == 0).all() and np.isfinite(plain["sim_all"]).all() and (plain["phi"] > 0).any()
    with pytest.raises(Exception, match="no derivative data"):
        f.evaluate(fx["eval_theta"], dlog, derivative=True)
    f.set_derivative(np.full(n, np.nan), np.zeros(n))
    a = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    b = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    c = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)          # ucf_fit_evaluate on the same fit
    for k in OUTPUTS:
        assert a[k].tobytes() == plain[k].tobytes(), k
        assert c[k].tobytes() == plain[k].tobytes(), k
    assert a["phi_d"].tobytes() == np.zeros(len(fx["eval_theta"])).tobytes()     # +0.0, sign included
    assert set(a) == set(OUTPUTS) | {"phi_d", "Jd", "simd_all"}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(a["simd_all"]).all() and (a["simd_all"] != 0).any() and (a["Jd"] != 0).any()
    f.close()


@pytest.mark.parametrize("key", PLAIN)
def test_plain_values_are_the_evaluators_dh(ufit, key):
    """simd_all[k][i] = debug_dh(k, i)[0] * Hc_k, byte for byte; debug_h beside it is what sim_all was formed from"""
    fx, P, f = make(ufit, "plain", key=key)
    n = len(fx["obs"])
    f.set_derivative(fx["dobs"])
    out = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), sim_all=True, derivative=True)
    sim, simd = out["sim_all"].reshape(-1, n), out["simd_all"].reshape(-1, n)
    for k, Hc in enumerate(hc_of_plans(ufit, fx, P)):
        dh = np.array([f.debug_dh(k, i) for i in range(n)])
        h = np.array([f.debug_h(k, i) for i in range(n)])
        assert dh.shape == (n, 1) and not np.array_equal(dh, h)
        assert (dh[:, 0] * Hc).tobytes() == simd[k].tobytes(), k
        assert (h[:, 0] * Hc).tobytes() == sim[k].tobytes(), k
    f.close()


def test_network_values_are_the_evaluators_dh(ufit):
    """a screened observation is ucf_screen_average of debug_dh times Hc, a point observation debug_dh[0] times Hc, byte for
    byte (the pattern of tests/test_gpu_fit_network.py for h)"""
    from unconfined_amd import lib as ucflib
    fx, P, f = make(ufit, "network")
    lib = ucflib.load()
    n = len(fx["obs"])
    f.set_derivative(fx["dobs"])
    simd = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), sim_all=True, derivative=True)["simd_all"].reshape(-1, n)
    assert (fx["e_count"] > 1).any() and (fx["e_count"] == 1).any()
    for k, Hc in enumerate(hc_of_plans(ufit, fx, P)):
        for i in range(n):
            dh = f.debug_dh(k, i)
            assert len(dh) == fx["e_count"][i]
            avg = dh.copy()
            if len(dh) > 1:
                ucflib.check(lib.ucf_screen_average(1, len(dh), np.ascontiguousarray(dh), avg))
            avg = avg[:1]
            assert (avg * Hc).tobytes() == simd[k, i:i + 1].tobytes(), (k, i, avg * Hc, simd[k, i])
    f.close()


def test_field_values_are_the_stated_recurrence(ufit):
    """each term's dimensionless dh read back (ucf_fit_debug_dh takes a term index), tfac = t / term_t from ucf_fit_field_terms,
    and acc = acc + q * (tfac * v), x Hc, redone in numpy one rounded operation at a time: simd_all byte for byte
    (the pattern of tests/test_gpu_fit_field.py)"""
    fx, P, f = make(ufit, "field")
    n = len(fx["obs"])
    tm = ufit.field_terms(P, fx["pump"], obs_wells_of(fx), fx["t"], fx["well"])
    first = tm["term_first"]
    tfac = np.repeat(fx["t"], np.diff(first)) / tm["term_t"]
    assert tfac.tobytes() == fx["tfac"].tobytes() and (tfac == 1.0).any() and (tfac > 1.0).any()
    q = fx["pump"][:, 2]
    f.set_derivative(fx["dobs"])
    simd = f.evaluate(fx["eval_theta"], float(fx["eval_dlog"]), sim_all=True, derivative=True)["simd_all"].reshape(-1, n)
    nterm = np.diff(first)
    assert (nterm[fx["iz"] < 0] == 3).any() and (nterm == 2).any()
    for k, Hc in enumerate(hc_of_plans(ufit, fx, P)):
        for i in range(n):
            acc = np.float64(0.0)
            for m in range(first[i], first[i + 1]):
                v = f.debug_dh(k, m)
                assert len(v) == fx["e_count"][m]
                acc = acc + q[tm["term_pump"][m]] * (tfac[m] * average(v))
            want = np.array([acc * Hc])
            assert want.tobytes() == simd[k, i:i + 1].tobytes(), (k, i, want, simd[k, i])
    f.close()


def test_field_derivative_against_the_forward_map(ufit):
    """P0 and its NO-FLOW image, both from t = 0 (tfac = 1): ds of ucf_field_drawdown in the fast flavour at the observation
    wells and the distinct observation times is the same model through the grid path.  Row 0 of simd_all agrees with it by
    the rule of test_against_the_forward_map of tests/test_gpu_fit_field.py for s: within twice (b_d of the P0 term + b_d of
    the image term)"""
    from unconfined_amd import engine as eng
    from unconfined_amd.field import WellField
    fx, P = fixture("field")
    assert np.array_equal(fx["eval_theta"][0], fx["theta_star"])
    wells = fx["pump"][[0, 2]].copy()
    wells[1, 2] = 1.0
    assert (wells[:, 3] == 0.0).all()
    f = ufit.Fit.field(P, [str(n) for n in fx["free"]], wells, obs_wells_of(fx), fx["t"], fx["well"], fx["iz"], fx["obs"])
    f.set_derivative(fx["dobs"])
    simd = f.evaluate(fx["theta_star"], float(fx["eval_dlog"]), sim_all=True, derivative=True)["simd_all"][0, 0]
    times = np.unique(fx["t"])
    field = WellField(wells, np.stack([fx["well_x"], fx["well_y"]], axis=1), times)
    assert field.group_count() == 1
    _, ds = field.drawdown(eng.Plan(P, mode="fast"), fx["well_z"])
    z0 = np.concatenate([[0], np.cumsum(fx["well_nz"])])
    bd = per_place(fx, gate_d(fx["dref"][0, 0], fx["dnoise"][0, 0]))
    worst = 0.0
    for i in range(len(fx["t"])):
        w, k = fx["well"][i], int(np.searchsorted(times, fx["t"][i]))
        col = ds[k, w, z0[w]:z0[w + 1]]
        fwd = average(col) if fx["iz"][i] < 0 else col[fx["iz"][i]]
        lim = 2.0 * sum(bd[m] for m in range(fx["term_first"][i], fx["term_first"][i + 1]) if fx["term_pump"][m] in (0, 2))
        worst = max(worst, abs(simd[i] - fwd) / lim)
        assert abs(simd[i] - fwd) <= lim, (i, simd[i], fwd, lim)
    print(f"[fit deriv field] against ds of ucf_field_drawdown: worst |difference| / 2 b_d = {worst:.3f}")
    f.close()


@pytest.mark.parametrize("kind", KINDS)
def test_reduction_is_the_arithmetic_it_claims(ufit, kind):
    """weights that are not 1 on both curves, a quarter of the derivative weights 0 with NaN in dobs: Jd within 2 ulp of
    max(|sd+|, |sd-|) / (2 dlog) of the value from simd_all, J likewise; phi, phi_d, g, A within (nobs + nd + 4) u sum|terms| of
    np.longdouble sums over the rows of h and the weighted rows of dh; A symmetric"""
    n = len(fixture({"plain": "neuman74"}.get(kind, kind))[0]["obs"])
    w, wd = some_weights(n)
    fx, _, f = make(ufit, kind, weight=w)
    dobs = with_gaps(fx["dobs"] * (1.0 + 0.01 * np.cos(np.arange(n))), wd)        # residuals that are not 0 at theta_star
    f.set_derivative(dobs, wd)
    nd = int((wd > 0).sum())
    assert 0 < nd < n and ufit.derivative_check(dobs, wd) == nd
    dlog = float(fx["eval_dlog"])
    a = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    assert (a["nbad"] == 0).all() and np.isfinite(a["sim_all"]).all() and np.isfinite(a["simd_all"]).all()
    assert (a["phi_d"] > 0).all() and (a["phi_d"] <= a["phi"]).all() and (a["phi_d"] < a["phi"]).any()
    for s in range(len(fx["eval_theta"])):
        for name, rows in (("J", a["sim_all"][s]), ("Jd", a["simd_all"][s])):
            for j in range(f.npar):
                up, dn = rows[1 + 2 * j].astype(np.longdouble), rows[2 + 2 * j].astype(np.longdouble)
                big = np.maximum(np.abs(rows[1 + 2 * j]), np.abs(rows[2 + 2 * j])) / (2 * dlog)
                want = (up - dn) / (np.longdouble(2.0) * np.longdouble(dlog))
                assert (np.abs(a[name][s][:, j].astype(np.longdouble) - want) <= 2 * np.spacing(big)).all(), (name, s, j)
        ref = recomputed_joint(a, s, fx["obs"], dobs, w, wd, dlog)
        assert ref["nterms"] == n + nd
        check_joint_sums(a, s, ref, n + nd)
    f.close()


def share(err, bound):
    return float((err / bound).max())


@pytest.mark.parametrize("kind,key", [("plain", "neuman74"), ("plain", "theis"), ("network", "neuman74"), ("field", "neuman74")])
def test_values_against_the_oracle(ufit, kind, key):
    """every row of simd_all within b_d = max(1e-10, 10 x (Theis: 20 x) the row's worst oracle-vs-binary128 noise of dh) x
    max(|ref|, 1e-3) of the oracle's dh at the same parameters -- the dh gate of test_parameter_batched_sweep_vs_oracle per row; a screen gets the
    weights of the average, a field observation sum |q| tfac b_d; sim_all within the h gate of tests/test_gpu_fit.py; Jd within
    (b_d+ + b_d-) / (2 dlog) of the oracle's central difference.  The used share of every gate is printed."""
    fx, _, f = make(ufit, kind, key=key)
    ref, b, dref, bd = references(kind, key)
    dlog = float(fx["eval_dlog"])
    f.set_derivative(fx["dobs"])
    out = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    assert (out["nbad"] == 0).all()
    eh, ed = np.abs(out["sim_all"] - ref), np.abs(out["simd_all"] - dref)
    print(f"[fit deriv {kind} {key}] worst |sim - oracle| / b = {share(eh, b):.3f}, worst |simd - oracle| / b_d = {share(ed, bd):.3f}")
    worst = 0.0
    for j in range(f.npar):
        Jd_or = (dref[:, 1 + 2 * j] - dref[:, 2 + 2 * j]) / (2 * dlog)
        lim = (bd[:, 1 + 2 * j] + bd[:, 2 + 2 * j]) / (2 * dlog)
        worst = max(worst, share(np.abs(out["Jd"][:, :, j] - Jd_or), lim))
    print(f"[fit deriv {kind} {key}] worst |Jd - Jd_or| / bound = {worst:.3f}")
    assert (eh <= b).all(), (kind, key, share(eh, b))
    assert (ed <= bd).all(), (kind, key, share(ed, bd))
    assert worst <= 1.0, (kind, key, worst)
    f.close()


def test_nonfinite_derivative_is_left_out_and_counted(ufit):
    """the overflow point of test_nonfinite_observation_is_left_out_and_counted as one more observation, with a positive
    derivative weight: nbad = 1 and every sum is that of the problem without it.

    The other half of the rule -- an observation whose h is finite and whose dh is not is KEPT under dweight = 0 -- has no
    test on data: tools/gen_fit_deriv_fixture.py scans the overflow regime around this point for one where the oracle's h is
    finite under every plan and its dh is not, and finds none (hfin_found = False in the fixture, asserted here): where the
    in-band rules fail they fail for both.  The all-zero-weights test covers dweight = 0 with finite dh."""
    assert not bool(fixture("neuman74")[0]["hfin_found"])
    n = len(fixture("neuman74")[0]["obs"])
    w, wd = some_weights(n + 1)
    wd[n] = 0.9
    fx, _, f = make(ufit, "plain", weight=w, extra=(NAN_T, NAN_R))
    obs, dobs = np.append(fx["obs"], 1.0), with_gaps(np.append(fx["dobs"] * 1.01, 1.0), wd)
    f.set_derivative(dobs, wd)
    dlog = float(fx["eval_dlog"])
    out = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    assert (out["nbad"] == 1).all(), out["nbad"]
    assert not np.isfinite(out["simd_all"][:, 0, n]).any()
    assert np.isfinite(out["simd_all"][:, :, :n]).all() and np.isfinite(out["sim_all"][:, :, :n]).all()
    for k in ("phi", "phi_d", "g", "A"):
        assert np.isfinite(out[k]).all(), k
    keep = np.arange(n + 1) < n
    nd = int((wd[:n] > 0).sum())
    for s in range(len(fx["eval_theta"])):
        check_joint_sums(out, s, recomputed_joint(out, s, obs, dobs, w, wd, dlog, keep), n + nd)
    f.close()


@pytest.mark.parametrize("mode", ["joint", "deriv"])
@pytest.mark.parametrize("key", PLAIN)
def test_lm_recovers_theta_star(ufit, key, mode):
    """the 4 stored starts in ONE lm call, jointly (unit weights on both curves) and on the derivative alone (weight 0 on every
    h): all converge within twice the iterations that the same Levenberg-Marquardt needs on the oracle alone (stored by the
    generator); phi <= sum w^2 b^2 + sum wd^2 b_d^2 (the device at theta_star cannot exceed that and the minimiser lies below);
    |ln theta_hat - ln theta_star| within 2 sum |(A^-1 [J; Jd]' W^2)_ji| [b; b_d]_i, the bound of parameter_bound of
    tests/test_gpu_fit.py with the rows of h and dh stacked; cov = phi / (nobs + nd - npar) A^-1, finite with a positive diagonal
    -- held to numpy's inverse of the A of the same evaluation within 16 u cond(A) max|cov|, the backward error of the Cholesky
    solves that form it"""
    from unconfined_amd import abi
    n = len(fixture(key)[0]["obs"])
    w = np.ones(n) if mode == "joint" else np.zeros(n)
    fx, _, f = make(ufit, "plain", weight=w, key=key)
    f.set_derivative(fx["dobs"])
    opt = lm_options(fx)
    res = f.lm(fx["starts"], **opt)
    b, bd = gate(fx["obs"], fx["noise"]), gate_d(fx["dobs"], fx["dnoise"], DH_FACTOR[key])
    limit = float(np.sum((w * b) ** 2) + np.sum(bd * bd))
    cap = 2 * int(fx[f"lm_iters_{mode}"].max())
    print(f"[fit deriv {key} {mode}] iterations {res['iters'].tolist()} (oracle alone: {fx[f'lm_iters_{mode}'].tolist()}), "
          f"phi / bound = {(res['phi'] / limit).max():.3e}")
    assert (res["status"] == abi.FIT_CONVERGED).all(), res["status"]
    assert (res["iters"] <= cap).all(), (res["iters"], cap)
    assert (res["phi"] <= limit).all(), (res["phi"], limit)
    out = f.evaluate(res["theta"], opt["dlog"], jacobian=True, derivative=True)      # the evaluation that cov came from
    dof = n + n - f.npar
    for s in range(len(fx["starts"])):
        A = out["A"][s]
        pinv = np.linalg.solve(A, np.concatenate([out["J"][s] * (w * w)[:, None], out["Jd"][s]]).T)
        lim = 2.0 * np.abs(pinv) @ np.concatenate([b, bd])
        err = np.abs(np.log(res["theta"][s]) - np.log(fx["theta_star"]))
        print(f"[fit deriv {key} {mode}] start {s}: |ln theta_hat - ln theta_star| / bound = {(err / lim).tolist()}")
        assert (err <= lim).all(), (key, mode, s, err, lim)
        cov = res["cov"][s]
        assert np.isfinite(cov).all() and (np.diag(cov) > 0).all()
        want = res["phi"][s] / dof * np.linalg.inv(A)
        assert (np.abs(cov - want) <= 16 * U * np.linalg.cond(A) * np.abs(cov).max()).all(), (cov, want)
    f.close()


@pytest.mark.parametrize("kind", KINDS)
def test_allocation_and_clear(ufit, kind):
    """set_derivative allocates the first time it is called (dobs and dweight; a field fit tfac as well) and not again; joint
    evaluations of one size allocate nothing after the first; clear_derivative restores the plain results bit for bit"""
    n = len(fixture({"plain": "neuman74"}.get(kind, kind))[0]["obs"])
    w, wd = some_weights(n)
    fx, _, f = make(ufit, kind, weight=w)
    dlog = float(fx["eval_dlog"])
    plain = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    c0 = f.alloc_count()
    f.set_derivative(with_gaps(fx["dobs"], wd), wd)
    c1 = f.alloc_count()
    assert c1 - c0 == (3 if kind == "field" else 2)
    f.set_derivative(fx["dobs"] * 1.01)
    assert f.alloc_count() == c1
    joint = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True, derivative=True)
    c2 = f.alloc_count()
    assert c2 > c1                                        # Jd and simd_all, and the sums grew by phi_d
    for i in range(3):
        f.evaluate(fx["eval_theta"] * (1.0 + 0.01 * i), dlog, jacobian=True, sim_all=True, derivative=True)
        f.evaluate(fx["eval_theta"] * (1.0 + 0.01 * i), dlog)
    assert f.alloc_count() == c2
    assert (joint["phi"] > plain["phi"]).all() and joint["phi_d"].tobytes() != np.zeros(len(joint["phi_d"])).tobytes()
    f.clear_derivative()
    again = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    for k in OUTPUTS:
        assert again[k].tobytes() == plain[k].tobytes(), k
    assert f.alloc_count() == c2
    with pytest.raises(Exception, match="no derivative data"):
        f.evaluate(fx["eval_theta"], dlog, derivative=True)
    f.set_derivative(fx["dobs"] * 1.01)
    assert f.alloc_count() == c2
    assert f.evaluate(fx["eval_theta"], dlog, derivative=True)["phi"].tobytes() == joint["phi"].tobytes()
    f.close()
