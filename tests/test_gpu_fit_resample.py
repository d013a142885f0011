"""Resampled fits on the GPU: ucf_fit_set_resample and the entries that read the multiplicities (ucf_fit_evaluate_resampled,
ucf_fit_objective_resampled, ucf_fit_lm_resampled, Fit.bootstrap), on the Theis fixture of tests/test_gpu_fit.py (a slots fit, three
observation wells) and the network fixture of tests/test_gpu_fit_deriv.py (a screened well, derivative data).  The arithmetic is the
text of include/ucf.h at ucf_fit_set_resample, restated by tests/fit_resample_restate.py; the kernel at its edges is
tests/test_gpu_fit_resample_edges.py.

1. evaluate_resampled (objective_resampled) is the restatement applied to the sim_all / simd_all (sim / simd) of a plain evaluate
   (objective) at the same theta, bit for bit, under least squares and under Huber.
2. sharing: 64 replicates reduced at ONE evaluated theta (set_of = 0) have the bytes of 64 copies of theta with identity set_of.
3. lm_resampled with rep = -1 has the bytes of lm in theta, phi, iters, status and cov; evaluate, objective, lm and loss_report with
   multiplicities attached have the bytes they have without.
4. subset equivalence: a 0/1 jackknife replicate against a fit made of the kept observations alone, at the same theta.  The lanes
   differ, so the sums are reordered: |delta| <= 2 n 2^-53 sum |terms| per sum, n the number of residual terms, the sum formed here
   from the J and sim that the subset fit returns.  phi_out meets the same bound against the weighted squared residuals of the
   deleted observations.
5. jackknife LM: lm_resampled over leave-one-well-out replicates against lm on the subset fits from the same theta0.  The fixture
   is noise-free, so every subset has the same minimiser; observations are therefore multiplied by 1 + 0.03 sin(1 + 2.7 i) (a
   fixed pattern, 3 % at most) to give each well its own pull.  The gate is measured on existing code only: d0 = max |delta ln
   theta| between two subset-fit runs from theta0 and theta0 (1 + 1e-3); a replicate must agree with its subset fit within 4
   max(d0, tol_step), and different replicates must differ from each other by more than that.  d0, the gate and the observed values
   are printed here and recorded by tools/bench_fit_resample.py in profiles/fit_resample.json.
6. a repeated call allocates nothing (ucf_fit_alloc_count); the refusals that need a fit leave it as it was."""
import numpy as np
import pytest

import fit_reduce_restate as fr
import fit_resample_restate as frs
from golden_util import load_deck
from test_gpu_fit import fixture, lm_options

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def theis(ufit, keep=None, obs=None):
    fx = fixture("theis")
    P = load_deck(str(fx["deck"]))[2]
    k = slice(None) if keep is None else keep
    well = np.searchsorted(np.unique(fx["r"]), fx["r"]).astype(np.int32)         # three radii: three wells
    f = ufit.Fit(P, [str(n) for n in fx["free"]], fx["t"][k], fx["r"][k], fx["z"], fx["iz"][k], (fx["obs"] if obs is None else obs)[k])
    return fx, well, f


def network(ufit, keep=None):
    from test_gpu_fit_deriv import fixture as dfixture, wells_of
    fx, P = dfixture("network")
    k = slice(None) if keep is None else keep
    n = len(fx["obs"])
    wd = np.where(np.arange(n) % 5 == 3, 0.0, 1.0 + 0.25 * np.cos(np.arange(n)))
    dobs = np.where(wd > 0.0, fx["dobs"], np.nan)
    f = ufit.Fit.network(P, [str(s) for s in fx["free"]], wells_of(fx), fx["t"][k], fx["well"][k], fx["iz"][k], fx["obs"][k])
    f.set_derivative(dobs[k], wd[k])
    return fx, fx["well"].astype(np.int32), f, dobs, wd


def restated(sim, simd, npar, obs, w, dobs, wd, two_dlog, kind, c, mult, set_of, rep):
    """the restatement on the rows of a call: one slot per observation, Hc = 1, so that s[k] is the value itself"""
    nplans, nobs = sim.shape
    inp = dict(source=fr.SLOTS, npar=npar, nsets=nplans // (1 + 2 * npar), nobs=nobs, two_dlog=two_dlog, h=sim.ravel(), Hc=np.ones(nplans),
               obs=obs, w=w, slot=np.arange(nobs, dtype=np.int32), plan_stride=nobs, dh=None, dobs=None, wd=None)
    if simd is not None:
        inp.update(dh=simd.ravel(), dobs=dobs, wd=wd)
    return frs.restate(inp, kind, c, mult, set_of, rep)


def check_against_restatement(ufit, f, theta, dlog, obs, dobs, wd, what):
    deriv = dobs is not None
    npar, n = f.npar, len(obs)
    w = np.ones(n)
    mult = frs.gpu_mult(n)
    f.set_resample(mult)
    iu = np.triu_indices(npar)
    na = npar * (npar + 1) // 2
    sim0 = f.objective(theta, sim=True)
    res = np.concatenate([(obs - sim0["sim"][1:]).ravel()] + ([(wd * (dobs - sim0["simd"][1:]))[:, wd > 0.0].ravel()] if deriv else []))
    for kind, c in (("l2", 0.0), ("huber", ufit.robust_scale(res))):
        f.set_loss(kind, c)
        plain = f.evaluate(theta, dlog, sim_all=True, derivative=deriv)
        got = f.evaluate_resampled(theta, dlog, set_of=frs.SET_OF, rep=frs.REP)
        want = restated(plain["sim_all"].reshape(-1, n), plain["simd_all"].reshape(-1, n) if deriv else None, npar, obs, w, dobs, wd,
                        2.0 * dlog, frs.KINDS[kind], c, mult, frs.SET_OF, frs.REP)
        tag = what + (kind,)
        assert want["sums"][:, 0].tobytes() == got["phi"].tobytes(), tag + ("phi",)
        assert np.ascontiguousarray(want["sums"][:, 1:1 + npar]).tobytes() == got["g"].tobytes(), tag + ("g",)
        for r in range(len(frs.REP)):
            assert want["sums"][r, 1 + npar:1 + npar + na].tobytes() == got["A"][r][iu].tobytes(), tag + ("A", r)
            assert np.array_equal(got["A"][r], got["A"][r].T)
        assert want["sums"][:, -2].tobytes() == got["phi_w"].tobytes() and want["sums"][:, -1].tobytes() == got["phi_out"].tobytes(), tag
        assert (want["nbad"] == got["nbad"]).all() and (want["counts"] == got["counts"]).all(), tag + (got["counts"],)
        assert (got["nbad"] == 0).all() and got["counts"][4, 0] == 0 and got["counts"][4, 2] == n and got["phi"][4] == 0.0, tag
        assert got["phi_out"][4] > 0.0 and (got["counts"][2:, 2] > 0).all() and (got["counts"][:2, 2] == 0).all(), tag
        if deriv:
            assert want["sums"][:, -3].tobytes() == got["phi_d"].tobytes(), tag + ("phi_d",)
            assert got["counts"][0, 1] == int((wd > 0).sum())
        if kind == "huber":
            assert 0 < got["counts"][0, 3] < got["counts"][0, 0] + got["counts"][0, 1], tag + ("both sides of c", got["counts"][0])
        # the base plans alone
        ob = f.objective(theta, sim=True)
        got = f.objective_resampled(theta, set_of=frs.SET_OF, rep=frs.REP)
        want = restated(ob["sim"], ob["simd"] if deriv else None, 0, obs, w, dobs, wd, 2.0 * dlog, frs.KINDS[kind], c, mult, frs.SET_OF, frs.REP)
        assert want["sums"][:, 0].tobytes() == got["phi"].tobytes() and want["sums"][:, -2].tobytes() == got["phi_w"].tobytes(), tag + ("objective",)
        assert want["sums"][:, -1].tobytes() == got["phi_out"].tobytes() and (want["counts"] == got["counts"]).all(), tag + ("objective",)
        if deriv:
            assert want["sums"][:, 1].tobytes() == got["phi_d"].tobytes(), tag + ("objective phi_d",)
    f.clear_loss()


def test_evaluate_resampled_is_the_restatement(ufit):
    fx, _, f = theis(ufit)
    check_against_restatement(ufit, f, fx["eval_theta"][:2], float(fx["eval_dlogs"][0]), fx["obs"], None, None, ("theis",))
    f.close()
    nx, _, net, dobs, wd = network(ufit)
    check_against_restatement(ufit, net, nx["eval_theta"], float(nx["eval_dlog"]), nx["obs"], dobs, wd, ("network",))
    net.close()


def test_replicates_share_one_evaluation(ufit):
    fx, well, f = theis(ufit)
    nrep = 64
    mult = ufit.resample_blocks(f.nobs, nrep, block=well, seed=11)
    assert len({m.tobytes() for m in mult}) > 5
    f.set_resample(mult)
    theta, dlog = fx["eval_theta"][1], float(fx["eval_dlogs"][0])
    rep = np.arange(nrep, dtype=np.int32)
    shared = f.evaluate_resampled(theta, dlog, set_of=np.zeros(nrep, np.int32), rep=rep)
    copies = f.evaluate_resampled(np.tile(theta, (nrep, 1)), dlog, set_of=None, rep=rep)
    for k in shared:
        assert shared[k].tobytes() == copies[k].tobytes(), k
    assert len(set(shared["phi"].tolist())) > 5
    a = f.objective_resampled(theta, set_of=np.zeros(nrep, np.int32), rep=rep)
    b = f.objective_resampled(np.tile(theta, (nrep, 1)), rep=rep)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["phi"].tobytes() == shared["phi"].tobytes() and a["phi_out"].tobytes() == shared["phi_out"].tobytes()
    f.close()


@pytest.mark.parametrize("loss", [None, ("tukey", 3.0)])
def test_unit_multiplicities_are_the_plain_entries_and_existing_entries_ignore_mult(ufit, loss):
    fx, well, f = theis(ufit)
    if loss:
        f.set_loss(*loss)
    dlog, o, starts = float(fx["eval_dlogs"][0]), lm_options(fx), fx["starts"][:4]
    before = dict(ev=f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True), ob=f.objective(fx["eval_theta"], sim=True),
                  lm=f.lm(starts, **o), rep=f.loss_report(fx["eval_theta"], factors=True))
    # no multiplicities attached: rep NULL and rep = -1
    for rep in (None, np.full(len(starts), -1, np.int32)):
        got = f.lm_resampled(starts, rep=rep, **o)
        for k in ("theta", "phi", "iters", "status", "cov"):
            assert got[k].tobytes() == before["lm"][k].tobytes(), (loss, k)
        assert (got["phi_out"] == 0.0).all() and (got["counts"][:, 0] == f.nobs).all() and (got["counts"][:, 1:3] == 0).all()
    f.set_resample(ufit.resample_jackknife(f.nobs, well))
    after = dict(ev=f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True), ob=f.objective(fx["eval_theta"], sim=True),
                 lm=f.lm(starts, **o), rep=f.loss_report(fx["eval_theta"], factors=True))
    for part in before:
        for k in before[part]:
            assert before[part][k].tobytes() == after[part][k].tobytes(), (loss, part, k)
    got = f.lm_resampled(starts, rep=np.full(len(starts), -1, np.int32), **o)
    for k in ("theta", "phi", "iters", "status", "cov"):
        assert got[k].tobytes() == before["lm"][k].tobytes(), (loss, k, "attached")
    ev = f.evaluate_resampled(fx["eval_theta"], dlog)
    for k in ("phi", "g", "A", "nbad"):
        assert ev[k].tobytes() == before["ev"][k].tobytes(), (loss, k)
    assert ev["phi_w"].tobytes() == before["rep"]["phi_w"].tobytes() and (ev["counts"][:, 3] == before["rep"]["ndown"]).all()
    f.close()


def abs_terms(out, obs, w, dobs=None, wd=None):
    """(sum |terms| of phi, g [npar], A [npar][npar], number of terms) of set 0 from the J and sim (Jd and simd) of an evaluate"""
    wr = w * (obs - out["sim_all"][0, 0])
    wj = w[:, None] * out["J"][0]
    phi, g, A, n = (wr * wr).sum(), np.abs(wj * wr[:, None]).sum(axis=0), np.abs(wj[:, :, None] * wj[:, None, :]).sum(axis=0), len(obs)
    if dobs is not None:
        m = wd > 0.0
        wrd = wd[m] * (dobs[m] - out["simd_all"][0, 0][m])
        wjd = wd[m, None] * out["Jd"][0][m]
        phi, g, A, n = phi + (wrd * wrd).sum(), g + np.abs(wjd * wrd[:, None]).sum(axis=0), A + np.abs(wjd[:, :, None] * wjd[:, None, :]).sum(axis=0), n + int(m.sum())
    return phi, g, A, n


@pytest.mark.parametrize("which", ["theis", "network"])
def test_a_jackknife_replicate_is_the_fit_of_the_kept_observations(ufit, which):
    if which == "theis":
        fx, well, f = theis(ufit)
        obs, dobs, wd = fx["obs"], None, None
        theta, dlog = fx["eval_theta"][1], float(fx["eval_dlogs"][0])
        sub = lambda keep: theis(ufit, keep=keep)[2]
    else:
        fx, well, f, dobs, wd = network(ufit)
        obs = fx["obs"]
        theta, dlog = fx["eval_theta"][1], float(fx["eval_dlog"])
        sub = lambda keep: network(ufit, keep=keep)[2]
    deriv = dobs is not None
    n = f.nobs
    mult = ufit.resample_jackknife(n, well)
    f.set_resample(mult)
    nb = len(mult)
    got = f.evaluate_resampled(theta, dlog, set_of=np.zeros(nb, np.int32), rep=np.arange(nb, dtype=np.int32))
    full = f.evaluate(theta, dlog, jacobian=True, sim_all=True, derivative=deriv)
    worst = 0.0
    for b in range(nb):
        keep = well != b
        g = sub(keep)
        out = g.evaluate(theta, dlog, jacobian=True, sim_all=True, derivative=deriv)
        g.close()
        aphi, ag, aA, nt = abs_terms(out, obs[keep], np.ones(int(keep.sum())), None if not deriv else dobs[keep], None if not deriv else wd[keep])
        lim = 2.0 * nt * U
        assert got["counts"][b, 0] == int(keep.sum()) and got["counts"][b, 2] == int((~keep).sum()) and got["nbad"][b] == 0, (which, b, got["counts"][b])
        assert abs(got["phi"][b] - out["phi"][0]) <= lim * aphi, (which, b, "phi", got["phi"][b], out["phi"][0], lim * aphi)
        assert abs(got["phi_w"][b] - out["phi"][0]) <= lim * aphi, (which, b, "phi_w")
        assert (np.abs(got["g"][b] - out["g"][0]) <= lim * ag).all(), (which, b, "g", got["g"][b] - out["g"][0], lim * ag)
        assert (np.abs(got["A"][b] - out["A"][0]) <= lim * aA).all(), (which, b, "A", got["A"][b] - out["A"][0], lim * aA)
        worst = max(worst, abs(got["phi"][b] - out["phi"][0]) / (lim * aphi), float((np.abs(got["g"][b] - out["g"][0]) / (lim * ag)).max()),
                    float((np.abs(got["A"][b] - out["A"][0]) / (lim * aA)).max()))
        if deriv:
            assert got["counts"][b, 1] == int((wd[keep] > 0).sum())
            assert abs(got["phi_d"][b] - out["phi_d"][0]) <= lim * aphi, (which, b, "phi_d")
        # the held-out sum against the deleted observations' weighted squared residuals, from the full fit's own sim
        r2 = (obs[~keep] - full["sim_all"][0, 0][~keep]) ** 2
        if deriv:
            m = ~keep & (wd > 0.0)
            r2 = np.concatenate([r2, (wd[m] * (dobs[m] - full["simd_all"][0, 0][m])) ** 2])
        assert abs(got["phi_out"][b] - r2.sum()) <= 2.0 * len(r2) * U * r2.sum(), (which, b, "phi_out", got["phi_out"][b], r2.sum())
    print(f"[fit resample {which}] subset equivalence: worst |delta| / bound = {worst:.3f}")
    f.close()


def jackknife_lm(ufit, printer=print):
    """module docstring, 5.  Returns the figures; asserts nothing"""
    fx, well, _ = theis(ufit)
    _.close()
    n = len(fx["obs"])
    obs = fx["obs"] * (1.0 + 0.03 * np.sin(1.0 + 2.7 * np.arange(n)))
    _, _, f = theis(ufit, obs=obs)
    o = lm_options(fx)
    theta0 = fx["starts"][0]
    mult = ufit.resample_jackknife(n, well)
    nb = len(mult)
    f.set_resample(mult)
    got = f.lm_resampled(np.tile(theta0, (nb, 1)), rep=np.arange(nb), **o)
    subs, d0 = [], 0.0
    for b in range(nb):
        g = theis(ufit, keep=well != b, obs=obs)[2]
        res = g.lm(np.stack([theta0, theta0 * (1.0 + 1.0e-3)]), **o)
        g.close()
        subs.append(res)
        d0 = max(d0, float(np.abs(np.log(res["theta"][0] / res["theta"][1])).max()))
    f.close()
    gate = 4.0 * max(d0, o["tol_step"])
    agree = [float(np.abs(np.log(got["theta"][b] / subs[b]["theta"][0])).max()) for b in range(nb)]
    apart = [float(np.abs(np.log(got["theta"][a] / got["theta"][b])).max()) for a in range(nb) for b in range(a + 1, nb)]
    out = dict(d0=d0, tol_step=float(o["tol_step"]), gate=gate, replicate_vs_subset=agree, between_replicates=apart,
               status=got["status"].tolist(), iters=got["iters"].tolist(), subset_status=[s["status"].tolist() for s in subs],
               phi=got["phi"].tolist(), subset_phi=[float(s["phi"][0]) for s in subs], phi_out=got["phi_out"].tolist(),
               counts=got["counts"].tolist())
    printer(f"[fit resample] jackknife LM: d0 = {d0:.3e}, gate = {gate:.3e}, replicate vs subset {agree}, between replicates {apart}, "
            f"status {out['status']} iters {out['iters']}")
    return out, got


def test_jackknife_lm_is_lm_on_the_kept_observations(ufit):
    from unconfined_amd import abi
    out, got = jackknife_lm(ufit)
    assert all(s in (abi.FIT_CONVERGED, abi.FIT_MAX_ITER) for s in out["status"]), out["status"]
    assert max(out["replicate_vs_subset"]) <= out["gate"], out
    assert min(out["between_replicates"]) > out["gate"], out
    for b in range(len(out["status"])):
        assert np.isfinite(got["cov"][b]).all() and (np.diag(got["cov"][b]) > 0).all() and got["phi_out"][b] > 0.0
        assert got["counts"][b][0] + got["counts"][b][2] == 22 and got["counts"][b][2] > 0


def test_repeated_calls_allocate_nothing_and_refusals_leave_the_fit_alone(ufit):
    fx, well, f = theis(ufit)
    dlog, theta = float(fx["eval_dlogs"][0]), fx["eval_theta"]
    so, UcfError = f._lib, __import__("unconfined_amd.lib", fromlist=["UcfError"]).UcfError

    def bad(call, word):
        with pytest.raises(UcfError) as err:
            call()
        assert err.value.status == -11 and word in err.value.message, err.value.message
    # no multiplicities attached: only -1 may be named
    bad(lambda: f.evaluate_resampled(theta, dlog, rep=[-1, 0, -1]), "no multiplicities")
    bad(lambda: f.lm_resampled(theta, rep=[0, -1, -1]), "no multiplicities")
    bad(lambda: f.set_resample(np.ones((65537, f.nobs), np.uint16)), "nrep=65537")
    assert so.ucf_fit_set_resample(f._h, 0, np.ones(f.nobs, np.uint16).ctypes.data) == -11
    mult = ufit.resample_blocks(f.nobs, 8, block=well, seed=2)
    f.set_resample(mult)
    n0 = f.alloc_count()
    bad(lambda: f.evaluate_resampled(theta, dlog, set_of=[0, 3], rep=[0, 0]), "set_of[1]")
    bad(lambda: f.evaluate_resampled(theta, dlog, set_of=[0, -1], rep=[0, 0]), "set_of[1]")
    bad(lambda: f.evaluate_resampled(theta, dlog, set_of=[0, 1], rep=[0, 8]), "rep[1]")
    bad(lambda: f.objective_resampled(theta, set_of=[0, 1], rep=[-2, 0]), "rep[0]")
    bad(lambda: f.objective_resampled(theta, rep=[0, 1, 2, 3]), "exceeds nsets")
    bad(lambda: f.lm_resampled(theta, rep=[0, 1, 8]), "rep[2]")
    x = np.zeros(3)
    assert so.ucf_fit_evaluate_resampled(f._h, 3, np.ascontiguousarray(theta).ctypes.data, dlog, 0, *([None] * 10)) == -11         # nred = 0
    assert so.ucf_fit_evaluate_resampled(f._h, 3, np.ascontiguousarray(theta).ctypes.data, dlog, 3, None, None, None, None, None, None,
                                         x.ctypes.data, None, None, None) == -11 and b"derivative" in so.ucf_last_error()
    assert f.alloc_count() == n0
    counts = []
    for i in range(4):
        th = theta * (1.0 + 0.01 * i)
        f.evaluate_resampled(th, dlog, set_of=[0, 1, 2, 0, 1], rep=[0, 1, 2, 3, -1])
        f.objective_resampled(th, set_of=[0, 1, 2, 0, 1], rep=[0, 1, 2, 3, -1])
        f.set_resample(mult)                                                     # the same size again: the buffer stays
        counts.append(f.alloc_count())
    assert counts[1] == counts[3], counts
    f.set_resample(None)
    bad(lambda: f.objective_resampled(theta, rep=[0, 0, 0]), "no multiplicities")
    assert (f.objective_resampled(theta)["counts"][:, 0] == f.nobs).all() and f.alloc_count() == counts[3]
    f.close()


def test_bootstrap_gives_an_ensemble(ufit):
    """the convenience: the one-step bootstrap is one evaluation; its thetas scatter about theta_hat and their covariance is
    symmetric and positive definite; a repeated call gives the same bytes; a refit of the first replicates uses the same draws and
    ends in a usable state (how far it lands from its one-step estimate is printed, not asserted: it is second order in the noise)"""
    fx, well, _ = theis(ufit)
    _.close()
    n = len(fx["obs"])
    obs = fx["obs"] * (1.0 + 0.03 * np.sin(1.0 + 2.7 * np.arange(n)))
    _, _, f = theis(ufit, obs=obs)
    o = lm_options(fx)
    hat = f.lm(fx["starts"][:1], **o)["theta"][0]
    one = f.bootstrap(hat, 256, seed=5)
    assert one["thetas"].shape == (256, 2) and one["used"].sum() >= 250 and one["nused"] == int(one["used"].sum())
    assert np.array_equal(one["cov"], one["cov"].T) and (np.diag(one["cov"]) > 0).all() and np.linalg.eigvalsh(one["cov"]).min() > 0
    assert (np.abs(one["mean"] - np.log(hat)) < 3.0 * np.sqrt(np.diag(one["cov"]))).all()
    again = f.bootstrap(hat, 256, seed=5)
    assert again["thetas"].tobytes() == one["thetas"].tobytes() and again["cov"].tobytes() == one["cov"].tobytes()
    re = f.bootstrap(hat, 8, seed=5, refit=True, **{k: v for k, v in o.items() if k != "dlog"})
    assert re["used"].all() and (re["mult"] == one["mult"][:8]).all()
    sd = np.sqrt(np.diag(one["cov"]))
    print(f"[fit resample] bootstrap: sd(ln theta) = {sd}, worst |refit - one step| / sd = {np.abs(np.log(re['thetas'] / one['thetas'][:8]) / sd).max():.3f}")
    f.close()
