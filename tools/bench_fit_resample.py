"""Measurement behind profiles/fit_resample.json (recorded with the build id, not gated: nobody has measured any of this before).

1. "almost free": a one-step bootstrap of 1024 replicates at one theta -- ONE ucf_fit_evaluate_resampled with set_of = 0, 1024
   reductions of the one evaluation -- against one ucf_fit_evaluate at the same theta, which is what the parent commit offers for
   a single replicate.  Workload: the network of tools/bench_fit_network.py (20 wells x 60 times, deck neuman74_partpen, 4
   parameters = 9 plans), blocks = wells.  Also the whole Fit.bootstrap (draws, upload, evaluation, 1024 host solves, covariance).
2. the reduction launch alone, RESAMPLE against ROBUST at equal nsets: 64 sets under Huber, through ucf_fit_evaluate and through
   ucf_fit_evaluate_resampled with the identity set_of and 64 bootstrap replicates; the kernel's own time comes from rocprofv3
   --kernel-trace --stats runs of --once (each a run of its own, no counters), merged with --trace.
3. the figures of the jackknife LM test (tests/test_gpu_fit_resample.py, docstring 5): d0, the gate and what was observed.

    python tools/bench_fit_resample.py OUT.json            # 1 and 3, and the wall clock of 2
    python tools/bench_fit_resample.py --once robust|resample        # one warm-up + one evaluation of 64 sets, for a kernel trace
    python tools/bench_fit_resample.py OUT.json --trace robust=DIR --trace resample=DIR
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from unconfined_amd import engine, fit as ufit                          # noqa: E402
from bench_fit_network import DLOG, FREE, arg, network                  # noqa: E402
from bench_fit_robust import reduce_rows, stats                         # noqa: E402
from golden_util import load_deck                                       # noqa: E402

NREP, NSETS, REPS, C_HUBER = 1024, 64, 5, 0.5


def problem():
    _, _, P = load_deck("neuman74_partpen")
    wells, t, well, iz = network()
    theta_star = np.array([getattr(P, n) for n in FREE])
    thetas = theta_star * np.exp(np.random.default_rng(5).uniform(np.log(0.7), np.log(1.4), (NSETS, len(FREE))))
    return ufit.Fit.network(P, FREE, wells, t, well, iz, np.ones(len(t))), theta_star, thetas, well


def clock(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "fit_resample.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        for i, a in enumerate(sys.argv):
            if a == "--trace":
                which, d = sys.argv[i + 1].split("=", 1)
                rep.setdefault("reduce_kernel", {})[which] = reduce_rows(d)
        rep["reduce_kernel_what"] = ("fit_reduce_kernel rows of rocprofv3 --kernel-trace --stats of `--once <mode>`, each a run of its own without "
                                     "counters: one warm-up and one evaluation of 64 sets x 9 plans under Huber, so 2 calls of 64 workgroups; "
                                     "average_ms is the kernel's own time per launch")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    f, theta, thetas, well = problem()
    f.set_loss("huber", C_HUBER)
    mult64 = ufit.resample_blocks(f.nobs, NSETS, block=well, seed=1)
    rep64 = np.arange(NSETS, dtype=np.int32)
    once = arg("--once", "")
    if once:
        f.set_resample(mult64)
        for _ in range(2):
            if once == "resample":
                f.evaluate_resampled(thetas, DLOG, rep=rep64)
            else:
                f.evaluate(thetas, DLOG)
        return
    # 2. wall clock at equal nsets (the evaluators dominate both)
    f.set_resample(mult64)
    modes = {"robust": lambda: f.evaluate(thetas, DLOG), "resample": lambda: f.evaluate_resampled(thetas, DLOG, rep=rep64)}
    for call in modes.values():
        call(); call()
    at64 = {k: [] for k in modes}
    for _ in range(REPS):
        for k, call in modes.items():
            at64[k].append(clock(call))
    # 1. one theta: one evaluate against 1024 reductions of one evaluation
    f.clear_loss()
    mult = ufit.resample_blocks(f.nobs, NREP, block=well, seed=1)
    f.set_resample(mult)
    zero, rep = np.zeros(NREP, np.int32), np.arange(NREP, dtype=np.int32)
    one = {"evaluate": lambda: f.evaluate(theta, DLOG), "evaluate_resampled_1024": lambda: f.evaluate_resampled(theta, DLOG, set_of=zero, rep=rep),
           "bootstrap_1024": lambda: f.bootstrap(theta, NREP, block=well, seed=1)}
    for call in one.values():
        call(); call()
    t1 = {k: [] for k in one}
    for _ in range(REPS):
        for k, call in one.items():
            t1[k].append(clock(call))
    bs = f.bootstrap(theta, NREP, block=well, seed=1)
    f.close()
    from test_gpu_fit_resample import jackknife_lm
    jk, _ = jackknife_lm(ufit, printer=lambda s: None)
    res = {"build_id": engine.build_id(),
           "what": f"the network of tools/bench_fit_network.py (20 wells x 60 times, deck neuman74_partpen, 4 parameters), unit weights and "
                   f"observations of 1 m, blocks = wells; two warm-ups, then {REPS} rounds with the calls in turn, wall clock [ms]; recorded, not gated",
           "one_theta_ms": {k: stats(v) for k, v in t1.items()},
           "one_theta_what": "evaluate: one ucf_fit_evaluate at theta (9 plans, one reduction: the parent's path for ONE replicate); "
                             "evaluate_resampled_1024: the same 9 plans once, then one launch of 1024 reductions; bootstrap_1024: Fit.bootstrap "
                             "(draws, upload of 1024 x 1200 multiplicities, that call, 1024 host solves, the covariance)",
           "one_step_over_evaluate": float(np.median(t1["evaluate_resampled_1024"]) / np.median(t1["evaluate"])),
           "bootstrap_used": int(bs["nused"]),
           "sets64_huber_ms": {k: stats(v) for k, v in at64.items()},
           "sets64_what": f"{NSETS} sets x 9 plans under Huber (c = {C_HUBER}): ucf_fit_evaluate (ROBUST instantiation, 64 workgroups) against "
                          "ucf_fit_evaluate_resampled with the identity set_of and 64 bootstrap replicates (RESAMPLE instantiation, 64 workgroups)",
           "jackknife_lm": jk,
           "jackknife_lm_what": "tests/test_gpu_fit_resample.py, docstring 5: d0 = max |delta ln theta| between two subset-fit runs from theta0 and "
                                "theta0 (1 + 1e-3); gate = 4 max(d0, tol_step); replicate_vs_subset must lie within it, between_replicates beyond it"}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
