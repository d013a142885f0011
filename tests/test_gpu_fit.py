"""ucf_fit_evaluate / ucf_fit_lm on the GPU against the oracle (fixtures: tools/gen_fit_fixture.py).

The problems: deck neuman74_partpen with the observation layout of test_parameter_batched_sweep_vs_oracle (22 times
1e-1 ... 1e4, radii 30 / 85.1 / 300, z = [145.7, 100.0], iz alternating), free = Kr, kappa, Ss, Sy -- the shared launch
sequence -- and deck c1_theis, free = Kr, Ss -- the plan-by-plan path.  The synthetic observations are the ORACLE's values
at the deck's parameters theta_star.

Every bound is derived: b_i = max(1e-10, 10 x the oracle's distance from its binary128 build at that observation) x
max(|ref_i|, 1e-3) is the gate of test_parameter_batched_sweep_vs_oracle taken per observation; sums are held to the
classical (n + 4) u sum|terms|; parameters to the first-order displacement of a least-squares minimiser under data errors
bounded by b.

Problem moench8 is there for the largest instantiation of the fit reduction (NPAR = 8 = UCF_FIT_MAX_PAR, reached by a real call):
deck c3_moench with a fourth Moench alpha, which the oracle and ucf_fit_perturb accept, free = Kr, kappa, Ss, Sy and the four
alphas, 12 observations, two parameter sets, one step.  Its values and Jacobian are held to the oracle by the same gate; its
sums are the documented arithmetic bit for bit (tests/fit_reduce_restate.py); eight log-parameters with four Moench alphas among
them are not claimed to be identifiable, so of ucf_fit_lm only the contract is asserted."""
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPT_NAMES = ("max_iter", "dlog", "lambda0", "lambda_up", "lambda_down", "tol_step", "tol_phi")
PROBLEMS = ["neuman74", "theis"]
EVAL_PROBLEMS = PROBLEMS + ["moench8"]              # moench8 has no lm part: NPAR = 8, values, Jacobian and sums only
# overflow regime of the neuman74_partpen deck (rD = 0.01, tD = 1e-4): the Laplace-space samples are NaN, the in-band rules
# scrub them and the result is NaN.  (The points of test_in_band_rule_counters_match_the_oracle, rD = 0.02 ... 0.7, fire the
# Wynn rules but every RESULT there is finite, in the oracle too: the NaN point is taken one step further into the same regime.)
NAN_T, NAN_R = 3.1e-4, 1.6


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def fixture(key):
    return np.load(os.path.join(GOLD, f"fit_synthetic_{key}.npz"))


def gate(ref, noise):
    return np.maximum(1e-10, 10.0 * noise) * np.maximum(np.abs(ref), 1e-3)


_cache = {}


def problem(ufit, key):
    """(fixture, deck parameters, Fit with unit weights)"""
    if key not in _cache:
        fx = fixture(key)
        dk, _, P = load_deck(str(fx["deck"]))
        if "moench_alpha" in fx.files:
            from unconfined_amd.abi import params_from_deck
            P = params_from_deck(dk.replace(MoenchM=len(fx["moench_alpha"]), MoenchAlpha=fx["moench_alpha"].tolist()))
        f = ufit.Fit(P, [str(n) for n in fx["free"]], fx["t"], fx["r"], fx["z"], fx["iz"], fx["obs"])
        _cache[key] = (fx, P, f)
    return _cache[key]


def evaluated(ufit, key, d):
    """one ucf_fit_evaluate of the fixture's three parameter sets at its d-th step"""
    if (key, d) not in _cache:
        fx, _, f = problem(ufit, key)
        _cache[(key, d)] = f.evaluate(fx["eval_theta"], float(fx["eval_dlogs"][d]), jacobian=True, sim_all=True)
    return _cache[(key, d)]


def recomputed(sim, obs, w, dlog, keep=None):
    """r, phi, g, A, J of one parameter set in np.longdouble from its sim_all rows; also sum|terms| of every sum"""
    L = np.longdouble
    s = sim.astype(L)
    P = (s.shape[0] - 1) // 2
    J = np.stack([(s[1 + 2 * j] - s[2 + 2 * j]) / (L(2.0) * L(dlog)) for j in range(P)], axis=1)
    r = obs.astype(L) - s[0]
    w2 = w.astype(L) ** 2
    if keep is not None:
        J, r, w2 = J[keep], r[keep], w2[keep]
    tphi = w2 * r * r
    tg = J * (w2 * r)[:, None]
    tA = J[:, :, None] * J[:, None, :] * w2[:, None, None]
    return dict(J=J, phi=tphi.sum(), g=tg.sum(0), A=tA.sum(0), aphi=np.abs(tphi).sum(), ag=np.abs(tg).sum(0), aA=np.abs(tA).sum(0))


def check_sums(out, s, ref, n):
    tol = (n + 4) * U
    assert abs(np.longdouble(out["phi"][s]) - ref["phi"]) <= tol * ref["aphi"], ("phi", s)
    assert (np.abs(out["g"][s].astype(np.longdouble) - ref["g"]) <= tol * ref["ag"]).all(), ("g", s)
    assert (np.abs(out["A"][s].astype(np.longdouble) - ref["A"]) <= tol * ref["aA"]).all(), ("A", s)
    assert np.array_equal(out["A"][s], out["A"][s].T)


def test_reduction_is_the_arithmetic_it_claims(ufit):
    """from the sim_all of ONE evaluate call (3 sets): J within 2 ulp of max(|sim+|, |sim-|) / (2 dlog), every sum within
    (nobs + 4) u sum|terms| of the np.longdouble value -- the classical bound for a sum of nobs terms whose terms carry a few
    roundings of their own; the same call twice gives identical bits"""
    fx, P, _ = problem(ufit, "neuman74")
    n = len(fx["obs"])
    w = 1.0 + 0.5 * np.sin(np.arange(n))             # weights that are not 1: W^2 must appear where it belongs
    f = ufit.Fit(P, [str(x) for x in fx["free"]], fx["t"], fx["r"], fx["z"], fx["iz"], fx["obs"], weight=w)
    dlog = 1e-3
    a = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    b = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["nbad"] == 0).all() and np.isfinite(a["sim_all"]).all()
    for s in range(3):
        sim = a["sim_all"][s]
        ref = recomputed(sim, fx["obs"], w, dlog)
        for j in range(f.npar):
            big = np.maximum(np.abs(sim[1 + 2 * j]), np.abs(sim[2 + 2 * j])) / (2 * dlog)
            assert (np.abs(a["J"][s][:, j].astype(np.longdouble) - ref["J"][:, j]) <= 2 * np.spacing(big)).all(), (s, j)
        check_sums(a, s, ref, n)
    f.close()


@pytest.mark.parametrize("key", EVAL_PROBLEMS)
def test_values_against_the_oracle(ufit, key):
    """every row of sim_all -- base and perturbed plans, both steps -- within b of the oracle at the same parameters"""
    fx, _, _ = problem(ufit, key)
    for d in range(len(fx["eval_dlogs"])):
        out = evaluated(ufit, key, d)
        ref, bound = fx["eval_ref"][d], gate(fx["eval_ref"][d], fx["eval_noise"][d])
        err = np.abs(out["sim_all"] - ref)
        print(f"[fit {key}] dlog={fx['eval_dlogs'][d]:g}: worst |sim - oracle| / b = {float((err / bound).max()):.3f}")
        assert (out["nbad"] == 0).all()
        assert (err <= bound).all(), (key, d, float((err / bound).max()))


@pytest.mark.parametrize("key", EVAL_PROBLEMS)
def test_jacobian_against_the_oracle(ufit, key):
    """the oracle's central difference with the same dlog: |J_dev - J_or| <= (b+ + b-) / (2 dlog) element by element (the
    truncation error is common to both sides and cancels)"""
    fx, _, f = problem(ufit, key)
    for d, dlog in enumerate(fx["eval_dlogs"]):
        out = evaluated(ufit, key, d)
        ref, bound = fx["eval_ref"][d], gate(fx["eval_ref"][d], fx["eval_noise"][d])
        for j in range(f.npar):
            J_or = (ref[:, 1 + 2 * j] - ref[:, 2 + 2 * j]) / (2 * dlog)
            lim = (bound[:, 1 + 2 * j] + bound[:, 2 + 2 * j]) / (2 * dlog)
            err = np.abs(out["J"][:, :, j] - J_or)
            print(f"[fit {key}] dlog={dlog:g} parameter {j}: worst |J - J_or| / bound = {float((err / lim).max()):.3f}")
            assert (err <= lim).all(), (key, dlog, j, float((err / lim).max()))


def test_sums_of_the_largest_npar_are_the_documented_arithmetic(ufit):
    """moench8, NPAR = 8: the call's own sim_all fed through the restatement of tests/fit_reduce_restate.py as h (one slot per
    observation, Hc = 1, so s[k] is the value itself) gives the bits of the call's phi, g, A and J"""
    import fit_reduce_restate as fr
    fx, _, f = problem(ufit, "moench8")
    assert f.npar == 8 and fx["eval_ref"].shape[2] == 17
    out = evaluated(ufit, "moench8", 0)
    nsets, nplan, nobs = out["sim_all"].shape
    inp = dict(source=fr.SLOTS, npar=8, nsets=nsets, nobs=nobs, two_dlog=2.0 * float(fx["eval_dlogs"][0]), h=out["sim_all"].ravel(), dh=None,
               Hc=np.ones(nsets * nplan), obs=fx["obs"], w=np.ones(nobs), slot=np.arange(nobs, dtype=np.int32), plan_stride=nobs)
    want = fr.restate(inp)
    assert (out["nbad"] == 0).all() and (want["nbad"] == 0).all()
    assert want["sim"].tobytes() == out["sim_all"].tobytes() and want["J"].tobytes() == out["J"].tobytes()
    assert want["sums"][:, 0].tobytes() == out["phi"].tobytes() and want["sums"][:, 1:9].tobytes() == out["g"].tobytes()
    iu = np.triu_indices(8)
    for s in range(nsets):
        assert want["sums"][s, 9:].tobytes() == out["A"][s][iu].tobytes(), s
        assert np.array_equal(out["A"][s], out["A"][s].T)
    # the same data through the hook: the instantiation <8, slots, no derivative data> once more
    got = fr.debug_fit_reduce(inp)
    for k in ("sums", "nbad", "J", "sim"):
        assert got[k].tobytes() == want[k].tobytes(), k


def test_lm_contract_at_the_largest_npar(ufit):
    """moench8: two starts off theta_star (parameter j moved by 25 % up or 20 % down in turn), max_iter = 2.  The trial points run the
    NPAR = 0 kernel, the steps ucf_fit_solve_step at npar = 8.  Only the contract: a status of the enum, no more than max_iter
    iterations, and a phi that is not above the phi of its start (from an evaluate there)"""
    from unconfined_amd import abi
    fx, _, f = problem(ufit, "moench8")
    up = np.where(np.arange(8) % 2 == 0, 1.25, 0.8)
    starts = np.stack([fx["theta_star"] * up, fx["theta_star"] / up])
    dlog = float(fx["eval_dlogs"][0])
    phi0 = f.evaluate(starts, dlog, jacobian=True)["phi"]         # the evaluation that ucf_fit_lm begins with
    res = f.lm(starts, max_iter=2, dlog=dlog)
    print(f"[fit moench8] lm: status {res['status'].tolist()} iters {res['iters'].tolist()} phi {res['phi'].tolist()} from {phi0.tolist()}")
    assert np.isfinite(phi0).all()
    assert set(res["status"].tolist()) <= {abi.FIT_CONVERGED, abi.FIT_MAX_ITER, abi.FIT_SINGULAR, abi.FIT_NONFINITE_START}
    assert (res["iters"] <= 2).all() and (res["iters"] >= 0).all()
    assert (res["phi"] <= phi0).all(), (res["phi"], phi0)


def lm_options(fx):
    o = dict(zip(OPT_NAMES, fx["lm_options"]))
    o["max_iter"] = int(o["max_iter"])
    return o


def lm_batch(ufit, key):
    if (key, "lm") not in _cache:
        fx, _, f = problem(ufit, key)
        _cache[(key, "lm")] = f.lm(fx["starts"], **lm_options(fx))
    return _cache[(key, "lm")]


def parameter_bound(f, fx, theta_hat):
    """2 sum_i |(A^-1 J' W^2)_ji| b_i at theta_hat (unit weights): the first-order displacement of the minimiser under data errors
    bounded by b; the factor 2 covers J being taken at theta_hat and being a finite difference"""
    b = gate(fx["obs"], fx["noise"])
    out = f.evaluate(theta_hat, float(fx["lm_options"][1]), jacobian=True)
    J = out["J"][0]
    pinv = np.linalg.solve(out["A"][0], J.T)
    return 2.0 * np.abs(pinv) @ b


@pytest.mark.parametrize("key", PROBLEMS)
def test_lm_recovers_theta_star(ufit, key):
    """16 starts (theta_star times factors from [0.3, 3], stored) in ONE lm call: all converge, within twice the iterations the
    same Levenberg-Marquardt needs on the oracle alone (a measurement, stored by the generator); phi <= sum w^2 b^2 (the device
    at theta_star itself cannot exceed that and the minimiser lies below); |ln theta_hat - ln theta_star| within the first-order
    bound"""
    from unconfined_amd import abi
    fx, _, f = problem(ufit, key)
    res = lm_batch(ufit, key)
    b = gate(fx["obs"], fx["noise"])
    cap = 2 * int(fx["lm_worst_iters"])
    print(f"[fit {key}] iterations {res['iters'].tolist()} (oracle alone: {fx['lm_iters'].tolist()}), phi / sum b^2 = "
          f"{(res['phi'] / np.sum(b * b)).max():.3e}")
    assert (res["status"] == abi.FIT_CONVERGED).all(), res["status"]
    assert (res["iters"] <= cap).all(), (res["iters"], cap)
    assert (res["phi"] <= np.sum(b * b)).all(), (res["phi"], float(np.sum(b * b)))
    for s in range(len(fx["starts"])):
        lim = parameter_bound(f, fx, res["theta"][s])
        err = np.abs(np.log(res["theta"][s]) - np.log(fx["theta_star"]))
        assert (err <= lim).all(), (key, s, err, lim)
        assert np.isfinite(res["cov"][s]).all() and (np.diag(res["cov"][s]) > 0).all()


def test_a_start_alone_and_in_the_batch_agree(ufit):
    """not bit for bit (the shared launch picks its instantiation from the union of the plans) but within the parameter bound"""
    from unconfined_amd import abi
    fx, _, f = problem(ufit, "neuman74")
    res = lm_batch(ufit, "neuman74")
    for s in (3, 11):
        one = f.lm(fx["starts"][s], **lm_options(fx))
        assert one["status"][0] == abi.FIT_CONVERGED
        lim = parameter_bound(f, fx, res["theta"][s])
        assert (np.abs(np.log(one["theta"][0]) - np.log(res["theta"][s])) <= lim).all(), (s, one["theta"], res["theta"][s], lim)


def test_nonfinite_observation_is_left_out_and_counted(ufit, oracle):
    """one more observation where the oracle gives NaN: nbad = 1, the sums are those of the problem without it, nothing faults"""
    fx, P, _ = problem(ufit, "neuman74")
    D = oracle.nondim(P)
    zD = fx["z"] / D.Lc
    ho, _ = oracle.batch(P, np.array([NAN_T / D.Tc]), np.array([NAN_R / D.Lc]), np.array([1], np.int32), zD, oracle.zlay(D, zD))
    assert np.isnan(ho[0, 0]), ho                      # the oracle alone
    n = len(fx["obs"])
    t, r = np.append(fx["t"], NAN_T), np.append(fx["r"], NAN_R)
    iz, obs = np.append(fx["iz"], 0).astype(np.int32), np.append(fx["obs"], 1.0)
    f = ufit.Fit(P, [str(x) for x in fx["free"]], t, r, fx["z"], iz, obs)
    dlog = float(fx["eval_dlogs"][0])
    out = f.evaluate(fx["eval_theta"], dlog, jacobian=True, sim_all=True)
    assert (out["nbad"] == 1).all(), out["nbad"]
    assert not np.isfinite(out["sim_all"][:, 0, n]).any()
    assert np.isfinite(out["phi"]).all() and np.isfinite(out["g"]).all() and np.isfinite(out["A"]).all()
    keep = np.arange(n + 1) < n
    bound = gate(fx["eval_ref"][0], fx["eval_noise"][0])
    for s in range(3):
        check_sums(out, s, recomputed(out["sim_all"][s], obs, np.ones(n + 1), dlog, keep), n + 1)
        # ... and the other observations are the problem without it
        assert (np.abs(out["sim_all"][s][:, :n] - fx["eval_ref"][0][s]) <= bound[s]).all()
    # a start there is refused with its own status, a trial step there is a rejected step
    from unconfined_amd import abi
    res = f.lm(fx["theta_star"] * 1.1, cov=False, **lm_options(fx))
    assert res["status"][0] == abi.FIT_NONFINITE_START and res["iters"][0] == 0
    f.close()


@pytest.mark.parametrize("key", PROBLEMS)
def test_repeated_evaluations_do_not_allocate(ufit, key):
    fx, P, _ = problem(ufit, key)
    f = ufit.Fit(P, [str(x) for x in fx["free"]], fx["t"], fx["r"], fx["z"], fx["iz"], fx["obs"])
    theta = fx["eval_theta"]
    counts = []
    for i in range(10):
        f.evaluate(theta * (1.0 + 0.01 * i), 1e-3)
        counts.append(f.alloc_count())
    assert counts[0] > 0
    assert counts[1] == counts[9], counts
    f.close()
