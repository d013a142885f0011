"""The recovery sequence of tests/test_gpu_fit_loss.py with the ORACLE as the forward model: CPU only (tests/oracle_lib.py, the
problems and fixtures of tools/gen_fit_fixture.py), numpy Levenberg-Marquardt as ucf_fit_lm runs it, the loss through
ucf_fit_loss_terms.  This is where the constants of that test were chosen and shown to work before any GPU run.

    python tools/fit_robust_oracle.py theis            # all 16 stored starts, a minute
    python tools/fit_robust_oracle.py neuman74 0 5     # the starts named, a few minutes each

Sequence (unit weights, so a weighted residual is a drawdown in metres): plant gross errors at PLANTED; Huber with c = C_HUBER x
the largest gate from the stored starts; Tukey with c = C_TUKEY x the largest gate from Huber's result, with tol_phi = 0 (the
outliers' constant share 2 c^2 / 3 of Tukey's phi would otherwise end the iteration on a relative decrease before the clean
residuals have reached their floor).  Printed per start: the
largest clean |r| at Huber's result against Tukey's c (the precondition), the factors at Tukey's result, |ln theta - ln theta_star|
of the plain, Huber and Tukey fits."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_fit_fixture import LM, Problem     # noqa: E402
from unconfined_amd import fit as ufit      # noqa: E402

PLANTED = np.array([5, 16])                 # of 22: radii[1] early, radii[2] late
SIGN = np.array([1.0, -1.0])
C_HUBER, C_TUKEY, GROSS = 2.5e8, 4.0e9, 1.0e10          # multiples of the largest gate max(1e-10, 10 noise) max(|obs|, 1e-3)


def gate(ref, noise):
    return np.maximum(1e-10, 10.0 * noise) * np.maximum(np.abs(ref), 1e-3)


def normal(pb, theta, obs, dlog, kind, c):
    s = [pb.sim(th, threads=8) for th in pb.rows(theta, dlog)]
    J = np.stack([(s[1 + 2 * j] - s[2 + 2 * j]) / (2 * dlog) for j in range(len(theta))], axis=1)
    x = obs - s[0]
    rho, b = ufit.loss_terms(kind, c, x)
    return float(rho.sum()), (J * b[:, None]).T @ x, (J * b[:, None]).T @ J


def lm(pb, theta0, obs, o, kind, c):
    x = np.log(theta0); lam = o["lambda0"]; it = 0
    phi, g, A = normal(pb, np.exp(x), obs, o["dlog"], kind, c)
    while True:
        try:
            step = ufit.solve_step(A, g, lam)
        except Exception:
            return np.exp(x), phi, it, False
        ph = float(ufit.loss_terms(kind, c, obs - pb.sim(np.exp(x + step), threads=8))[0].sum())
        it += 1
        done = np.max(np.abs(step)) <= o["tol_step"]
        if np.isfinite(ph) and ph <= phi:
            if phi - ph <= o["tol_phi"] * phi:
                done = True
            x = x + step; lam *= o["lambda_down"]
            if not done and it < o["max_iter"]:
                _, g, A = normal(pb, np.exp(x), obs, o["dlog"], kind, c)
            phi = ph
        else:
            lam *= o["lambda_up"]
        if done or it >= o["max_iter"]:
            return np.exp(x), phi, it, done


def main(key, which):
    pb = Problem(key)
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"fit_synthetic_{key}.npz"))
    b = gate(fx["obs"], fx["noise"])
    cH, cT, gross = C_HUBER * b.max(), C_TUKEY * b.max(), GROSS * b.max()
    obs = fx["obs"].copy()
    obs[PLANTED] += SIGN * gross
    clean = np.ones(len(obs), bool); clean[PLANTED] = False
    print(f"{key}: largest gate {b.max():.3e}, Huber c {cH:.3e}, Tukey c {cT:.3e}, planted {SIGN * gross} at {PLANTED}", flush=True)
    for s in (which or range(len(fx["starts"]))):
        l2, _, it0, ok0 = lm(pb, fx["starts"][s], obs, LM, "l2", 0.0)
        hub, _, it1, ok1 = lm(pb, fx["starts"][s], obs, LM, "huber", cH)
        r = obs - pb.sim(hub, threads=8)
        tuk, _, it2, ok2 = lm(pb, hub, obs, {**LM, "tol_phi": 0.0}, "tukey", cT)
        rT = obs - pb.sim(tuk, threads=8)
        bT = ufit.loss_terms("tukey", cT, rT)[1]
        err = lambda th: np.abs(np.log(th / fx["theta_star"])).max()
        print(f"start {s}: iters {it0} {it1} {it2} converged {ok0} {ok1} {ok2}; at Huber's result clean |r| <= {np.abs(r[clean]).max():.3e} (c_T {cT:.3e}), "
              f"planted |r| >= {np.abs(r[~clean]).min():.3e}; at Tukey's result b == 0 at {np.flatnonzero(bT == 0.0)}, b < 1 at {int((bT < 1.0).sum())}, "
              f"clean |r| <= {np.abs(rT[clean]).max():.3e}; |ln theta/theta_star| plain {err(l2):.3e} Huber {err(hub):.3e} Tukey {err(tuk):.3e}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "theis", [int(a) for a in sys.argv[2:]])
