"""Writes the fixtures of tests/test_gpu_fit.py: tests/golden/fit_synthetic_<problem>.npz.  CPU only (the oracle and its
binary128 build, tests/oracle_lib.py); a few minutes (moench8: just under four on eight cores, nearly all of it the 34 binary128 evaluations of its 12 points).

    python tools/gen_fit_fixture.py [neuman74 | theis | moench8]

Per problem (deck, free parameters, observation layout):
  obs          the ORACLE's dimensional drawdown at the deck's own parameters theta_star: the synthetic observations;
  noise        per observation |oracle - binary128| / max(|binary128|, 1e-3): the oracle's own error there;
  eval_*       three parameter sets and two steps dlog: the oracle's values (and their noise) of the base plan and of every
               plan with one parameter moved by e^{+-dlog}, rows as in sim_all of ucf_fit_evaluate;
  starts       16 starting points, theta_star times factors drawn once, log-uniformly, from [0.3, 3];
  lm_*         Levenberg-Marquardt as ucf_fit_lm runs it, here in numpy ON THE ORACLE ALONE from those starts: all must
               converge (asserted), cond(A) at theta_star must be < 1e8 (asserted); the worst iteration count is stored and
               the GPU test allows twice that.  A problem with lm=False has no starts and no lm_*: moench8 -- deck c3_moench with
               a fourth Moench alpha (moench_alpha in the fixture; the oracle and ucf_fit_perturb accept it), free = Kr, kappa,
               Ss, Sy and the four alphas: 8 = UCF_FIT_MAX_PAR free parameters, 12 observations, two sets, one step -- is there
               for the largest instantiation of the fit reduction; eight log-parameters with four Moench alphas among them
               are not claimed to be identifiable, and nothing asserts that a fit of them converges.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_deck          # noqa: E402
from unconfined_amd.abi import params_from_deck   # noqa: E402
from oracle_lib import Oracle              # noqa: E402
from unconfined_amd import fit as ufit     # noqa: E402  (ucf_fit_perturb, ucf_fit_solve_step: host arithmetic, no GPU)

PROBLEMS = {
    # the observation layout of tests/test_gpu_contract.py::test_parameter_batched_sweep_vs_oracle
    "neuman74": dict(deck="neuman74_partpen", free=["Kr", "kappa", "Ss", "Sy"], radii=(30.0, 85.1, 300.0), z=[145.7, 100.0], seed=74),
    # Theis has no shared launch: the plan-by-plan path of the parameter batch
    "theis": dict(deck="c1_theis", free=["Kr", "Ss"], radii=(0.5, 2.0, 8.0), z=[5.0, 2.0], seed=1),
    # the largest number of free parameters: the radii and depths of neuman74, 12 times, a fourth Moench alpha
    "moench8": dict(deck="c3_moench", moench_alpha=[0.000278, 0.0168, 0.416, 2.0], free=["Kr", "kappa", "Ss", "Sy"] + [f"MoenchAlpha[{i}]" for i in range(4)],
                    radii=(30.0, 85.1, 300.0), z=[145.7, 100.0], seed=3, nt=12, lm=False, eval_dlogs=[1.0e-3],
                    eval_factors=[[1.0] * 8, [1.3, 0.8, 1.2, 0.9, 1.1, 0.85, 1.25, 0.9]]),
}
LM = dict(max_iter=60, dlog=1.0e-3, lambda0=1.0e-2, lambda_up=10.0, lambda_down=0.1, tol_step=1.0e-8, tol_phi=1.0e-9)
EVAL_FACTORS = np.array([[1.0, 1.0, 1.0, 1.0], [1.3, 0.8, 1.2, 0.9], [0.7, 1.5, 0.8, 1.4]])
EVAL_DLOGS = np.array([1.0e-3, 1.0e-2])


def layout(radii, nt=22):
    r = np.full(nt, radii[1]); r[::3] = radii[0]; r[1::5] = radii[2]
    iz = (np.arange(nt) % 2).astype(np.int32)
    return 10.0 ** np.linspace(-1, 4, nt), r, iz


def theta_of(P, free):
    return np.array([P.MoenchAlpha[int(n[len("MoenchAlpha["):-1])] if n.startswith("MoenchAlpha[") else getattr(P, n) for n in free])


class Problem:
    def __init__(self, key):
        pr = PROBLEMS[key]
        self.dk, _, self.P0 = load_deck(pr["deck"])
        if "moench_alpha" in pr:
            self.dk = self.dk.replace(MoenchM=len(pr["moench_alpha"]), MoenchAlpha=list(pr["moench_alpha"]))
            self.P0 = params_from_deck(self.dk)
        self.free = pr["free"]
        self.t, self.r, self.iz = layout(pr["radii"], pr.get("nt", 22))
        self.z = np.array(pr["z"])
        self.theta_star = theta_of(self.P0, self.free)
        self.O, self.Q = Oracle(), Oracle(quad=True)

    def sim(self, theta, oracle=None, threads=0):
        """dimensional drawdown of every observation at the parameters theta"""
        O = oracle or self.O
        P = ufit.perturb(self.P0, self.free, theta)
        D = self.O.nondim(P)
        tD, rD, zD = self.t / D.Tc, self.r / D.Lc, self.z / D.Lc
        sv = self.O.split_vector(list(self.dk.j0s), tD)
        zl = self.O.zlay(D, zD)
        h, _ = O.batch(P, tD, rD, sv, zD, zl, threads)
        return h[np.arange(len(self.t)), self.iz] * D.Hc

    def rows(self, theta, dlog):
        """the parameter sets of one ucf_fit_evaluate set: base, then parameter j up, parameter j down"""
        out = [np.array(theta, float)]
        for j in range(len(theta)):
            for f in (np.exp(dlog), np.exp(-dlog)):
                th = np.array(theta, float); th[j] = th[j] * f
                out.append(th)
        return out

    def with_noise(self, theta):
        ref = self.sim(theta)
        truth = self.sim(theta, self.Q, threads=16)
        return ref, np.abs(ref - truth) / np.maximum(np.abs(truth), 1e-3)

    def normal(self, theta, obs, dlog):
        s = [self.sim(th, threads=8) for th in self.rows(theta, dlog)]
        J = np.stack([(s[1 + 2 * j] - s[2 + 2 * j]) / (2 * dlog) for j in range(len(theta))], axis=1)
        res = obs - s[0]
        return float(res @ res), J.T @ res, J.T @ J, J

    def lm(self, theta0, obs, o):
        """ucf_fit_lm for one start (unit weights); returns theta, phi, iterations, converged"""
        x = np.log(theta0); lam = o["lambda0"]; it = 0
        phi, g, A, _ = self.normal(np.exp(x), obs, o["dlog"])
        while True:
            step = ufit.solve_step(A, g, lam)
            trial = self.sim(np.exp(x + step), threads=8)
            ph = float((obs - trial) @ (obs - trial))
            it += 1
            done = np.max(np.abs(step)) <= o["tol_step"]
            if np.isfinite(ph) and ph <= phi:
                if phi - ph <= o["tol_phi"] * phi:
                    done = True
                x = x + step; lam *= o["lambda_down"]
                if not done and it < o["max_iter"]:
                    phi, g, A, _ = self.normal(np.exp(x), obs, o["dlog"])
                phi = ph
            else:
                lam *= o["lambda_up"]
            if done:
                return np.exp(x), phi, it, True
            if it >= o["max_iter"]:
                return np.exp(x), phi, it, False


def generate(key):
    pb = Problem(key)
    P = len(pb.free)
    pr = PROBLEMS[key]
    factors, dlogs = np.array(pr.get("eval_factors", EVAL_FACTORS))[:, :P], np.array(pr.get("eval_dlogs", EVAL_DLOGS))
    out = dict(t=pb.t, r=pb.r, z=pb.z, iz=pb.iz, free=np.array(pb.free), theta_star=pb.theta_star, deck=np.array(PROBLEMS[key]["deck"]))
    out["obs"], out["noise"] = pb.with_noise(pb.theta_star)
    assert np.isfinite(out["obs"]).all()
    print(key, "observations:", out["obs"][:4], "... worst noise", out["noise"].max())
    # evaluation sets
    thetas = pb.theta_star * factors
    ref = np.zeros((len(dlogs), len(thetas), 1 + 2 * P, len(pb.t))); noise = np.zeros_like(ref)
    for s, th in enumerate(thetas):
        base = pb.with_noise(th)
        for d, dlog in enumerate(dlogs):
            for k, row in enumerate(pb.rows(th, dlog)):
                ref[d, s, k], noise[d, s, k] = base if k == 0 else pb.with_noise(row)
        print(key, "evaluation set", s, "worst noise", noise[:, s].max())
    out.update(eval_theta=thetas, eval_dlogs=dlogs, eval_ref=ref, eval_noise=noise)
    path = os.path.join(ROOT, "tests", "golden", f"fit_synthetic_{key}.npz")
    if "moench_alpha" in pr:
        out["moench_alpha"] = np.array(pr["moench_alpha"])
    if not pr.get("lm", True):
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes; no lm part")
        return
    # conditioning at theta_star
    _, _, A, _ = pb.normal(pb.theta_star, out["obs"], LM["dlog"])
    cond = float(np.linalg.cond(A))
    assert cond < 1e8, cond
    # starts, and the same Levenberg-Marquardt on the oracle alone
    rng = np.random.default_rng(PROBLEMS[key]["seed"])
    factors = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (16, P)))
    starts = pb.theta_star * factors
    iters = []
    for s in range(16):
        th, phi, it, ok = pb.lm(starts[s], out["obs"], LM)
        print(key, "start", s, "iters", it, "phi", phi, "ln(theta/theta_star)", np.log(th / pb.theta_star), flush=True)
        assert ok, (key, s, "the oracle alone does not converge from this start: change the start")
        iters.append(it)
    out.update(starts=starts, cond_A=np.array(cond), lm_iters=np.array(iters), lm_worst_iters=np.array(max(iters)),
               lm_options=np.array([LM[k] for k in ("max_iter", "dlog", "lambda0", "lambda_up", "lambda_down", "tol_step", "tol_phi")]))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; cond(A) =", cond, "worst iterations", max(iters))


if __name__ == "__main__":
    for key in (sys.argv[1:] or list(PROBLEMS)):
        generate(key)
