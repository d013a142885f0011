"""Measurement behind profiles/fit_robust.json (recorded, not gated): one ucf_fit_evaluate of the network workload of
tools/bench_fit_network.py (20 wells x 60 times, deck neuman74_partpen, 64 sets x 4 parameters = 576 plans) under least squares,
Huber and Tukey.  The loss lives in the reduction kernel alone, so the evaluators dominate and the three totals are expected to be
indistinguishable; nothing here promises a ratio.

    python tools/bench_fit_robust.py OUT.json [--sets N] [--tree DIR]
          # per loss two warm-ups, then 5 evaluations, the losses in turn; wall clock around evaluate, median of 5.
          # --tree DIR: a built checkout of the PARENT commit; its least-squares time is measured in a child process before
          # and after, in the same run: the yardstick for "least squares did not get slower"
    python tools/bench_fit_robust.py --l2-only [--sets N]       # what the child runs: prints its 5 times as JSON (no loss API used)
    python tools/bench_fit_robust.py --once l2|huber|tukey      # one warm-up + one evaluate, for a kernel trace
    python tools/bench_fit_robust.py OUT.json --trace l2=DIR --trace huber=DIR --trace tukey=DIR
          # add the fit_reduce_kernel rows of rocprofv3 --kernel-trace --stats runs of --once, each a run of its own
"""
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("UCF_BENCH_TREE") or os.path.dirname(HERE)          # the tree whose package is measured
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
sys.path.insert(0, HERE)

from unconfined_amd import engine, fit as ufit                          # noqa: E402  (first: the package of ROOT, whatever is imported below)
from bench_fit_network import DLOG, FREE, arg, network                  # noqa: E402
from golden_util import load_deck                                       # noqa: E402

C = {"l2": 0.0, "huber": 0.5, "tukey": 0.8}          # metres: the observations are 1 m, the residuals of the 64 sets lie on both sides
REPS = 5


def problem(nsets):
    _, _, P = load_deck("neuman74_partpen")
    wells, t, well, iz = network()
    theta_star = np.array([getattr(P, n) for n in FREE])
    theta = theta_star * np.exp(np.random.default_rng(5).uniform(np.log(0.7), np.log(1.4), (nsets, len(FREE))))
    # observations of 1 m with unit weights, as tools/bench_fit_network.py has them
    return ufit.Fit.network(P, FREE, wells, t, well, iz, np.ones(len(t))), theta


def timed(f, theta):
    t0 = time.perf_counter()
    o = f.evaluate(theta, DLOG)
    return time.perf_counter() - t0, o


def reduce_rows(d):
    """the rows of fit_reduce_kernel in the kernel_stats.csv files under d, the instantiation kept in the name"""
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                m = re.search(r"fit_reduce_kernel<[^>]*>", r["Name"])
                if m:
                    rows.append({"name": m.group(0).replace("(anonymous namespace)::", ""), "calls": int(r["Calls"]),
                                 "total_ms": float(r["TotalDurationNs"]) / 1e6, "average_ms": float(r["AverageNs"]) / 1e6, "percent": float(r["Percentage"])})
    return rows


def stats(ts):
    return {"median": 1e3 * float(np.median(ts)), "min": 1e3 * min(ts), "max": 1e3 * max(ts), "all": [1e3 * x for x in ts]}


def child_l2(tree, nsets):
    env = dict(os.environ, UCF_BENCH_TREE=os.path.abspath(tree))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--l2-only", "--sets", str(nsets)], env=env, capture_output=True, text=True, timeout=600)
    if res.returncode:
        raise RuntimeError(res.stderr[-2000:])
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(os.path.dirname(HERE), "profiles", "fit_robust.json"))
    nsets = arg("--sets", 64)
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        for i, a in enumerate(sys.argv):
            if a == "--trace":
                which, d = sys.argv[i + 1].split("=", 1)
                rep.setdefault("reduce_kernel", {})[which] = reduce_rows(d)
        rep["reduce_kernel_what"] = ("fit_reduce_kernel rows of rocprofv3 --kernel-trace --stats of `--once <loss>`, each a run of its own without "
                                     "counters: one warm-up and one evaluate, so 2 calls; average_ms is the kernel's own time per launch")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    if "--l2-only" in sys.argv:
        f, theta = problem(nsets)
        timed(f, theta); timed(f, theta)
        print(json.dumps({"build_id": engine.build_id(), "times": [timed(f, theta)[0] for _ in range(REPS)]}))
        return
    once = arg("--once", "")
    f, theta = problem(nsets)
    if once:
        f.set_loss(once, C[once])
        f.evaluate(theta, DLOG)
        f.evaluate(theta, DLOG)
        return
    tree = arg("--tree", "")
    parent = [child_l2(tree, nsets)] if tree else []
    times, down = {}, {}
    for k in C:
        f.set_loss(k, C[k])
        timed(f, theta); timed(f, theta)
        rep = f.loss_report(theta)
        down[k] = float(rep["ndown"].sum()) / float(len(theta) * f.nobs - rep["nbad"].sum())
    for k in C:
        times[k] = []
    for _ in range(REPS):
        for k in C:
            f.set_loss(k, C[k])
            times[k].append(timed(f, theta)[0])
    if tree:
        parent.append(child_l2(tree, nsets))
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_fit_evaluate, {nsets} sets x 4 parameters = {nsets * 9} plans, the network of tools/bench_fit_network.py (20 wells x 60 "
                   f"times, deck neuman74_partpen), unit weights and observations of 1 m; per loss two warm-ups, then {REPS} evaluations with the "
                   "losses in turn, wall clock [ms] around evaluate; recorded, not gated.  The evaluators dominate: the loss is a few operations "
                   "per residual in the reduction kernel",
           "c": C, "share_of_factors_below_1": down, "evaluate_ms": {k: stats(v) for k, v in times.items()}}
    if tree:
        rep["parent_l2_ms"] = {"what": "least squares of the parent commit's build on the same workload, in a child process before and after the loop "
                                       "above: two warm-ups, then 5 evaluations each",
                               "build_id": parent[0]["build_id"], "before": stats(parent[0]["times"]), "after": stats(parent[1]["times"])}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
