"""Measurement behind profiles/fit_eval.json (recorded, not gated): one ucf_fit_evaluate of 64 parameter sets x 4 free
parameters (576 plans x 22 observations) against the same 576 plans through ucf_drawdown_multi plus the reduction in numpy,
alternated in one process; 3 warm-ups, median of 10.

    python tools/bench_fit_eval.py OUT.json            # the timing
    python tools/bench_fit_eval.py --once              # one evaluate, for a kernel trace of its own
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import GOLD, load_deck                 # noqa: E402
from unconfined_amd import engine, fit as ufit          # noqa: E402

NSETS, DLOG = 64, 1e-3


def main():
    fx = np.load(os.path.join(GOLD, "fit_synthetic_neuman74.npz"))
    _, _, P = load_deck(str(fx["deck"]))
    free = [str(n) for n in fx["free"]]
    npar, nobs = len(free), len(fx["obs"])
    rng = np.random.default_rng(5)
    theta = fx["theta_star"] * np.exp(rng.uniform(np.log(0.5), np.log(2.0), (NSETS, npar)))
    f = ufit.Fit(P, free, fx["t"], fx["r"], fx["z"], fx["iz"], fx["obs"])
    if "--once" in sys.argv:
        f.evaluate(theta, DLOG)
        f.evaluate(theta, DLOG)
        return
    # the same plans for the host path
    sets = []
    for th in theta:
        sets.append(th)
        for j in range(npar):
            for s in (DLOG, -DLOG):
                v = th.copy(); v[j] *= np.exp(s)
                sets.append(v)
    plans = [engine.Plan(ufit.perturb(P, free, th), mode="fast") for th in sets]
    iz, obs = fx["iz"], fx["obs"]

    def host_path():
        for pl, th in zip(plans, sets):
            pl.update(ufit.perturb(P, free, th))
        h, _ = engine.drawdown_multi(plans, fx["t"], fx["r"], fx["z"])
        sim = h[:, np.arange(nobs), iz].reshape(NSETS, 1 + 2 * npar, nobs)
        r = obs - sim[:, 0]
        J = (sim[:, 1::2] - sim[:, 2::2]) / (2 * DLOG)                   # [set][par][obs]
        return (r * r).sum(1), np.einsum("spi,si->sp", J, r), np.einsum("spi,sqi->spq", J, J)

    def fit_path():
        o = f.evaluate(theta, DLOG)
        return o["phi"], o["g"], o["A"]

    for _ in range(3):
        a, b = fit_path(), host_path()
    agree = max(float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))) for x, y in zip(a[:1], b[:1]))
    tf, th_ = [], []
    for _ in range(10):
        t0 = time.perf_counter(); fit_path(); t1 = time.perf_counter(); host_path(); t2 = time.perf_counter()
        tf.append(t1 - t0); th_.append(t2 - t1)
    rep = {"build_id": engine.build_id(), "what": "one ucf_fit_evaluate (64 sets x 4 parameters = 576 plans x 22 observations x 2 depths, "
           "deck neuman74_partpen) vs ucf_plan_update + ucf_drawdown_multi of the same 576 plans + the reduction in numpy; alternated in "
           "one process, 3 warm-ups, median of 10 wall-clock times [ms]; recorded, not gated",
           "fit_evaluate_ms": {"median": 1e3 * float(np.median(tf)), "min": 1e3 * min(tf), "max": 1e3 * max(tf)},
           "drawdown_multi_numpy_ms": {"median": 1e3 * float(np.median(th_)), "min": 1e3 * min(th_), "max": 1e3 * max(th_)},
           "ratio_fit_over_host": float(np.median(tf) / np.median(th_)), "phi_rel_difference_between_paths": agree}
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fit_eval.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
