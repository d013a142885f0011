"""Robust losses in a fit on the GPU: ucf_fit_set_loss, ucf_fit_loss_report and the entries that honour the loss
(ucf_fit_evaluate, ucf_fit_evaluate_joint, ucf_fit_objective, ucf_fit_lm), on the problems and fixtures of tests/test_gpu_fit.py
(fit_synthetic_neuman74, fit_synthetic_theis) and the network fixture of tests/test_gpu_fit_deriv.py.  The arithmetic is the text
of include/ucf.h at ucf_fit_set_loss, restated by tests/fit_loss_restate.py; the kernel at its edges is
tests/test_gpu_fit_loss_edges.py.

1. evaluate against the restatement: phi, g, A (phi_d) of a call under each loss are recomputed from the sim_all (simd_all) of the
   same call, bit for bit; the same for phi, phi_w, ndown, b (bd) of loss_report, from the sim of objective.  c is taken from the
   residuals themselves (the robust scale of those of the sets away from theta_star) and both sides of it are shown to be populated.
2. Huber with c = 1e300 has the bytes of least squares in evaluate, objective and lm; set_loss('l2') after robust calls gives the
   bytes of a fresh fit; repeated calls do not allocate.
3. recovery.  The fixtures are noise-free: the device meets the oracle's observations within the gate b_i = max(1e-10, 10 noise)
   max(|obs_i|, 1e-3), 1e-10 relative.  ndown counts EVERY term with b < 1.0, and under Tukey b = (1 - (x / c)^2)^2 is 1.0 only
   where (x / c)^2 < 2^-54, |x| < 7.4e-9 c.  For "ndown = number planted" to hold, Tukey's c has to lie more than eight decades
   above the clean residuals, and the gross errors above that.  So, with unit weights (a weighted residual is a drawdown):
   gross errors of +-GROSS x max b at PLANTED (2 of 22 observations, 9 %: one early at the middle radius, one late at the far
   one), Huber with c = C_HUBER x max b from the stored starts, Tukey with c = C_TUKEY x max b (a fixed multiple of the
   fixture's gate) from Huber's result with tol_phi = 0 (the outliers' constant share 2 c^2 / 3 of Tukey's phi would end the
   iteration on a relative decrease before the clean residuals reach their floor).  tools/fit_robust_oracle.py runs this
   sequence with the oracle as the forward model on the CPU; with these constants it works there from every stored start of
   theis and from the starts of neuman74 used here (the iteration counts and errors it printed are in its log, not asserted).
4. a fit with derivative data: an outlier only in dobs is flagged in bd and not in b."""
import numpy as np
import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
from test_gpu_fit import fixture, gate, lm_options
from golden_util import load_deck

pytestmark = pytest.mark.gpu

PLANTED = np.array([5, 16])
SIGN = np.array([1.0, -1.0])
C_HUBER, C_TUKEY, GROSS = 2.5e8, 4.0e9, 1.0e10
STARTS = {"theis": list(range(16)), "neuman74": [0, 5]}


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def plain_fit(ufit, key, obs=None, weight=None, keep=None):
    fx = fixture(key)
    P = load_deck(str(fx["deck"]))[2]
    k = slice(None) if keep is None else keep
    f = ufit.Fit(P, [str(n) for n in fx["free"]], fx["t"][k], fx["r"][k], fx["z"], fx["iz"][k], (fx["obs"] if obs is None else obs)[k],
                 weight=None if weight is None else weight[k])
    return fx, f


def restated(sim, simd, npar, obs, w, dobs, wd, two_dlog, kind, c):
    """the restatement on the rows of a call: one slot per observation, Hc = 1, so that s[k] is the value itself"""
    nplans, nobs = sim.shape
    inp = dict(source=fr.SLOTS, npar=npar, nsets=nplans // (1 + 2 * npar), nobs=nobs, two_dlog=two_dlog, h=sim.ravel(), Hc=np.ones(nplans),
               obs=obs, w=w, slot=np.arange(nobs, dtype=np.int32), plan_stride=nobs, dh=None, dobs=None, wd=None)
    if simd is not None:
        inp.update(dh=simd.ravel(), dobs=dobs, wd=wd)
    return fl.restate(inp, kind, c)


def check_against_restatement(f, theta, dlog, obs, w, dobs, wd, kind, c, what):
    deriv = dobs is not None
    npar, n = f.npar, len(obs)
    f.set_loss(kind, c)
    out = f.evaluate(theta, dlog, jacobian=True, sim_all=True, derivative=deriv)
    nsets = len(out["phi"])
    want = restated(out["sim_all"].reshape(-1, n), out["simd_all"].reshape(-1, n) if deriv else None, npar, obs, w, dobs, wd, 2.0 * dlog, kind, c)
    inside = float((np.abs(want["x"][want["counted"]]) < c).mean())
    assert 0.1 <= inside <= 0.9, what + ("share of residuals inside c", inside)         # a condition on the inputs
    assert (out["nbad"] == 0).all() and (want["nbad"] == 0).all(), what
    assert want["sums"][:, 0].tobytes() == out["phi"].tobytes(), what + ("phi",)
    assert np.ascontiguousarray(want["sums"][:, 1:1 + npar]).tobytes() == out["g"].tobytes(), what + ("g",)
    iu = np.triu_indices(npar)
    na = npar * (npar + 1) // 2
    for s in range(nsets):
        assert want["sums"][s, 1 + npar:1 + npar + na].tobytes() == out["A"][s][iu].tobytes(), what + ("A", s)
        assert np.array_equal(out["A"][s], out["A"][s].T)
    assert want["J"].tobytes() == out["J"].tobytes(), what + ("J",)
    if deriv:
        assert want["sums"][:, -2].tobytes() == out["phi_d"].tobytes(), what + ("phi_d",)
    # the report: base plans only; its residuals are those of objective(sim=True) under the same loss
    obj = f.objective(theta, sim=True)
    rep = f.loss_report(theta, factors=True)
    want = restated(obj["sim"], obj["simd"] if deriv else None, 0, obs, w, dobs, wd, 2.0 * dlog, kind, c)
    assert want["sums"][:, 0].tobytes() == rep["phi"].tobytes() == obj["phi"].tobytes(), what + ("report phi",)
    assert want["sums"][:, -1].tobytes() == rep["phi_w"].tobytes(), what + ("report phi_w",)
    assert (rep["ndown"] == want["ndown"]).all() and (rep["ndown"][1:] > 0).all() and (rep["nbad"] == 0).all(), what + (rep["ndown"], want["ndown"])
    assert rep["b"].tobytes() == want["b"].tobytes(), what + ("b",)
    if deriv:
        assert want["sums"][:, 1].tobytes() == obj["phi_d"].tobytes(), what + ("objective phi_d",)
        nan = np.isnan(want["bd"])
        assert (np.isnan(rep["bd"]) == nan).all() and rep["bd"][~nan].tobytes() == want["bd"][~nan].tobytes(), what + ("bd",)
        assert (nan == (wd == 0.0)).all()
    f.clear_loss()


@pytest.mark.parametrize("kind", ["huber", "tukey"])
def test_evaluate_and_report_are_the_restatement(ufit, kind):
    """neuman74 (slots, NPAR = 4, weights that are not 1) and the network fixture with derivative data (network source, screens,
    gaps in the derivative weights): c = the robust scale of the weighted residuals of the sets after the first, which is theta_star"""
    fx, _ = plain_fit(ufit, "neuman74")
    n = len(fx["obs"])
    w = (1.0 + 0.5 * np.sin(np.arange(n))) / gate(fx["obs"], fx["noise"]).max()
    _, f = plain_fit(ufit, "neuman74", weight=w)
    dlog = float(fx["eval_dlogs"][0])
    sim = f.objective(fx["eval_theta"], sim=True)["sim"]
    c = ufit.robust_scale((w * (fx["obs"] - sim[1:])).ravel())
    check_against_restatement(f, fx["eval_theta"], dlog, fx["obs"], w, None, None, fl.KINDS[kind], c, (kind, "neuman74"))
    f.close()
    from test_gpu_fit_deriv import make
    nx, _, net = make(ufit, "network")
    n = len(nx["obs"])
    wd = np.where(np.arange(n) % 5 == 3, 0.0, 1.0 + 0.25 * np.cos(np.arange(n)))
    dobs = np.where(wd > 0.0, nx["dobs"], np.nan)
    net.set_derivative(dobs, wd)
    dlog = float(nx["eval_dlog"])
    obj = net.objective(nx["eval_theta"], sim=True)
    c = ufit.robust_scale(np.concatenate([(nx["obs"] - obj["sim"][1:]).ravel(), (wd * (dobs - obj["simd"][1:]))[:, wd > 0.0].ravel()]))
    check_against_restatement(net, nx["eval_theta"], dlog, nx["obs"], np.ones(n), dobs, wd, fl.KINDS[kind], c, (kind, "network"))
    net.close()


@pytest.mark.parametrize("key", ["theis", "neuman74"])
def test_huber_beyond_every_residual_has_the_bytes_of_least_squares(ufit, key):
    fx, plain = plain_fit(ufit, key)
    _, f = plain_fit(ufit, key)
    dlog = float(fx["eval_dlogs"][0])
    o = lm_options(fx)
    starts = fx["starts"][:4]
    want = dict(ev=plain.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True), ob=plain.objective(fx["eval_theta"], sim=True),
                lm=plain.lm(starts, **o))

    def same(got, names, what):
        for part in names:
            for k in names[part]:
                assert got[part][k].tobytes() == want[part][k].tobytes(), (key, what, part, k)
    names = dict(ev=("phi", "g", "A", "nbad", "J", "sim_all"), ob=("phi", "nbad", "sim"), lm=("theta", "phi", "iters", "status"))
    f.set_loss("huber", 1.0e300)
    assert f.get_loss() == (fl.HUBER, 1.0e300)
    got = dict(ev=f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True), ob=f.objective(fx["eval_theta"], sim=True), lm=f.lm(starts, **o))
    same(got, names, "huber 1e300")
    rep = f.loss_report(fx["eval_theta"], factors=True)
    assert rep["phi"].tobytes() == rep["phi_w"].tobytes() == want["ob"]["phi"].tobytes() and (rep["ndown"] == 0).all() and (rep["b"] == 1.0).all()
    # a loss for one call of lm: the fit's own is put back
    one = f.lm(starts, loss=("tukey", 3.0), **o)
    assert f.get_loss() == (fl.HUBER, 1.0e300) and one["phi"].tobytes() != want["lm"]["phi"].tobytes()
    # robust calls, then least squares again: the bytes of a fresh fit, from every entry; the report of a least-squares fit
    f.set_loss("tukey", 0.5 * float(np.abs(fx["obs"]).max()))
    f.evaluate(fx["eval_theta"], dlog)
    f.objective(fx["eval_theta"])
    f.set_loss("l2")
    assert f.get_loss() == (fl.L2, 0.0)
    got = dict(ev=f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True), ob=f.objective(fx["eval_theta"], sim=True), lm=f.lm(starts, **o))
    same(got, names, "l2 again")
    assert got["lm"]["cov"].tobytes() == want["lm"]["cov"].tobytes()
    rep = f.loss_report(fx["eval_theta"], factors=True)
    assert rep["phi"].tobytes() == rep["phi_w"].tobytes() == want["ob"]["phi"].tobytes() and (rep["ndown"] == 0).all() and (rep["b"] == 1.0).all()
    # bd on a fit without derivative data is refused
    theta1, bd = np.ascontiguousarray(fx["eval_theta"][:1]), np.zeros(len(fx["obs"]))
    assert f._lib.ucf_fit_loss_report(f._h, 1, theta1.ctypes.data, None, None, None, None, None, bd.ctypes.data) == -11
    assert b"derivative" in f._lib.ucf_last_error()
    # repeated calls of the same size allocate nothing, under a loss as without
    f.set_loss("huber", 1.0e300)
    counts = []
    for i in range(4):
        f.evaluate(fx["eval_theta"] * (1.0 + 0.01 * i), dlog)
        f.objective(fx["eval_theta"] * (1.0 + 0.01 * i))
        f.loss_report(fx["eval_theta"] * (1.0 + 0.01 * i), factors=True)
        counts.append(f.alloc_count())
    assert counts[1] == counts[3], counts
    f.close()
    plain.close()


def clean_parameter_bound(f, b, w, theta_hat, dlog):
    """parameter_bound of tests/test_gpu_fit.py for a fit with weights: 2 sum_i |(A^-1 J' W^2)_ji| b_i at theta_hat.  With weight 0
    at the planted observations they add nothing: the bound is that of the clean observations alone."""
    out = f.evaluate(theta_hat, dlog, jacobian=True)
    pinv = np.linalg.solve(out["A"][0], (out["J"][0] * (w * w)[:, None]).T)
    return 2.0 * np.abs(pinv) @ b


@pytest.mark.parametrize("key", ["theis", "neuman74"])
def test_recovery_from_gross_errors(ufit, key):
    """module docstring, 3.  Asserted per start: every clean |wr| at Huber's result lies below Tukey's c (the precondition, loud); at
    Tukey's result {b == 0} is exactly the planted set and ndown its size; |ln theta - ln theta_star| within the bound of the
    clean observations; the least-squares fit of the contaminated data outside it; cov finite with a positive diagonal"""
    from unconfined_amd import abi
    fx = fixture(key)
    n = len(fx["obs"])
    b = gate(fx["obs"], fx["noise"])
    cH, cT, gross = C_HUBER * b.max(), C_TUKEY * b.max(), GROSS * b.max()
    obs = fx["obs"].copy()
    obs[PLANTED] += SIGN * gross
    clean = np.ones(n, bool)
    clean[PLANTED] = False
    assert len(PLANTED) <= 0.1 * n and len(set(fx["r"][PLANTED])) == 2
    _, f = plain_fit(ufit, key, obs=obs)
    _, f0 = plain_fit(ufit, key, weight=clean.astype(float))          # the plain fit whose planted observations have weight 0
    o = lm_options(fx)
    starts = fx["starts"][STARTS[key]]
    l2 = f.lm(starts, **o)
    hub = f.lm(starts, loss=("huber", cH), **o)
    r = obs - f.objective(hub["theta"], sim=True)["sim"]
    print(f"[fit loss {key}] Huber c = {cH:.3e}: status {hub['status'].tolist()} iters {hub['iters'].tolist()}, clean |r| <= {np.abs(r[:, clean]).max():.3e}, "
          f"planted |r| >= {np.abs(r[:, ~clean]).min():.3e}; Tukey c = {cT:.3e}")
    assert (np.abs(r[:, clean]) < cT).all(), ("precondition: a clean residual at Huber's result beyond Tukey's c", float(np.abs(r[:, clean]).max()), cT)
    tuk = f.lm(hub["theta"], loss=("tukey", cT), **{**o, "tol_phi": 0.0})
    f.set_loss("tukey", cT)
    rep = f.loss_report(tuk["theta"], factors=True)
    err_t = np.abs(np.log(tuk["theta"] / fx["theta_star"]))
    err_2 = np.abs(np.log(l2["theta"] / fx["theta_star"]))
    print(f"[fit loss {key}] Tukey: status {tuk['status'].tolist()} iters {tuk['iters'].tolist()} ndown {rep['ndown'].tolist()}; worst |ln theta / theta_star| "
          f"Tukey {err_t.max():.3e}, Huber {np.abs(np.log(hub['theta'] / fx['theta_star'])).max():.3e}, least squares {err_2.max():.3e}")
    for s in range(len(starts)):
        assert np.array_equal(np.flatnonzero(rep["b"][s] == 0.0), PLANTED), (key, s, np.flatnonzero(rep["b"][s] == 0.0))
        assert rep["ndown"][s] == len(PLANTED) and rep["nbad"][s] == 0, (key, s, rep["ndown"][s], np.flatnonzero(rep["b"][s] < 1.0))
        lim = clean_parameter_bound(f0, b, clean.astype(float), tuk["theta"][s], o["dlog"])
        print(f"[fit loss {key}] start {STARTS[key][s]}: worst Tukey error / bound = {(err_t[s] / lim).max():.3f}, least squares error / bound = {(err_2[s] / lim).max():.3e}")
        assert (err_t[s] <= lim).all(), (key, s, err_t[s], lim)
        assert (err_2[s] > lim).any(), (key, s, err_2[s], lim)
        assert np.isfinite(tuk["cov"][s]).all() and (np.diag(tuk["cov"][s]) > 0).all(), (key, s)
        assert tuk["status"][s] in (abi.FIT_CONVERGED, abi.FIT_MAX_ITER)
    f.close()
    f0.close()


def test_an_outlier_in_the_derivative_alone_is_flagged_in_bd(ufit):
    """the theis fixture with derivative data at theta_star, where every residual lies at the gate: one dobs moved by half the
    largest |dobs|; Tukey with a tenth of that as c.  bd == 0 there and nowhere else, b > 0 everywhere, ndown counts it; under
    Huber with the same c it is the one term with a factor below 1"""
    from test_gpu_fit_deriv import make
    fx, _, f = make(ufit, "plain", key="theis")
    n = len(fx["obs"])
    k = 7
    move = 0.5 * float(np.abs(fx["dobs"]).max())
    dobs = fx["dobs"].copy()
    dobs[k] += move
    f.set_derivative(dobs)
    c = 0.1 * move
    obj = f.objective(fx["theta_star"], sim=True)
    rs, rd = fx["obs"] - obj["sim"][0], dobs - obj["simd"][0]
    others = np.arange(n) != k
    assert (np.abs(rs) < 1e-6 * c).all() and (np.abs(rd[others]) < 1e-6 * c).all() and abs(rd[k]) > c, (np.abs(rs).max(), np.abs(rd[others]).max(), rd[k], c)
    f.set_loss("tukey", c)
    rep = f.loss_report(fx["theta_star"], factors=True)
    assert np.array_equal(np.flatnonzero(rep["bd"][0] == 0.0), [k]) and (rep["b"][0] > 0.0).all() and (rep["bd"][0][others] > 0.0).all()
    assert rep["ndown"][0] >= 1 and rep["nbad"][0] == 0
    f.set_loss("huber", c)
    rep = f.loss_report(fx["theta_star"], factors=True)
    assert np.array_equal(np.flatnonzero(rep["bd"][0] < 1.0), [k]) and (rep["b"][0] == 1.0).all() and rep["ndown"][0] == 1
    assert rep["bd"][0][k] == c / abs(rd[k])
    f.close()
