"""Measurement behind profiles/fit_network.json (recorded, not gated): ucf_fit_evaluate of an observation network made by
ucf_fit_create_network against the dense form -- ucf_fit_create with the union of all depths of the network -- on the same
(well, time) points.

The problem is made up here, in the shape of a real pumping test (about twenty piezometers and observation wells): 20 wells
with 60 times each, 16 piezometers at distinct depths and 4 screened wells of 5 depths (36 depths in all), deck
neuman74_partpen (model 5, partially penetrating), free = Kr, kappa, Ss, Sy, 64 parameter sets = 576 plans.  The dense
form has no screen average: it observes the middle depth of a screened well, which leaves its evaluator work, every depth
at every point, what it is.

    python tools/bench_fit_network.py OUT.json [--sets N] [--pairs N]     # alternating pairs, wall clock around evaluate
    python tools/bench_fit_network.py --once network|dense [--sets N]     # one warm-up + one evaluate, for a kernel trace
    python tools/bench_fit_network.py OUT.json --trace network=DIR --trace dense=DIR
                                                   # add the per-kernel rows of rocprofv3 --kernel-trace --stats runs of --once
"""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_deck                       # noqa: E402
from unconfined_amd import engine, fit as ufit          # noqa: E402

DLOG = 1e-3
FREE = ["Kr", "kappa", "Ss", "Sy"]
NT = 60


def network():
    """wells [(r, z)], and per observation t, well, iz (-1: screen average)"""
    rng = np.random.default_rng(20)
    radii = np.sort(10.0 ** rng.uniform(np.log10(5.0), np.log10(400.0), 20))
    wells, t, well, iz = [], [], [], []
    piezo_z = np.linspace(8.0, 155.0, 16)
    for w in range(20):
        if w % 5 == 4:                                   # 4 screened wells, 5 depths across 30 m
            top = 70.0 + 15.0 * (w // 5)
            z = np.linspace(top, top + 30.0, 5)
        else:
            z = piezo_z[w - w // 5: w - w // 5 + 1]
        wells.append((float(radii[w]), z))
        tw = 10.0 ** np.linspace(-1.0, 4.0, NT) * (1.0 + 0.01 * w)      # every well logged on its own clock
        t.append(tw); well.append(np.full(NT, w)); iz.append(np.full(NT, -1 if len(z) > 1 else 0))
    return wells, np.concatenate(t), np.concatenate(well).astype(np.int32), np.concatenate(iz).astype(np.int32)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def kernel_rows(d):
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                rows.append({"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                             "average_ms": float(r["AverageNs"]) / 1e6, "percent": float(r["Percentage"])})
    return rows


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "fit_network.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        for i, a in enumerate(sys.argv):
            if a == "--trace":
                which, d = sys.argv[i + 1].split("=", 1)
                rep.setdefault("kernel_trace", {})[which] = kernel_rows(d)
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once network` / `--once dense`, runs of their own without "
                                    "counters: one warm-up and one evaluate each, so calls and totals are for two evaluations")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    nsets, pairs = arg("--sets", 64), arg("--pairs", 5)
    _, _, P = load_deck("neuman74_partpen")
    wells, t, well, iz = network()
    theta_star = np.array([getattr(P, n) for n in FREE])
    theta = theta_star * np.exp(np.random.default_rng(5).uniform(np.log(0.7), np.log(1.4), (nsets, len(FREE))))
    z_all = np.concatenate([z for _, z in wells])
    z0 = np.concatenate([[0], np.cumsum([len(z) for _, z in wells])])
    obs = np.ones(len(t))
    once = arg("--once", "")

    def make_network():
        return ufit.Fit.network(P, FREE, wells, t, well, iz, obs)

    def make_dense():
        mid = np.array([z0[w] + len(wells[w][1]) // 2 for w in well], np.int32)
        return ufit.Fit(P, FREE, t, np.array([wells[w][0] for w in well]), z_all, mid, obs)

    if once:
        f = make_network() if once == "network" else make_dense()
        f.evaluate(theta, DLOG)
        f.evaluate(theta, DLOG)
        return
    fn, fd = make_network(), make_dense()
    counts = {"network": fn.eval_counts(), "dense": fd.eval_counts()}

    def timed(f):                                        # evaluate ends with its streams drained and the sums on the host
        t0 = time.perf_counter()
        o = f.evaluate(theta, DLOG)
        return time.perf_counter() - t0, o

    (_, a), (_, b) = timed(fn), timed(fd)                # warm-up, discarded
    timed(fn); timed(fd)
    tn, td = [], []
    for _ in range(pairs):
        tn.append(timed(fn)[0]); td.append(timed(fd)[0])
    launched, dense = counts["network"]
    ratio = float(np.median(tn) / np.median(td))
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_fit_evaluate, {nsets} sets x 4 parameters = {nsets * 9} plans, deck neuman74_partpen, 20 wells x {NT} times "
                   "(16 piezometers, 4 screened wells of 5 depths): network form (ucf_fit_create_network) vs dense form (ucf_fit_create, all "
                   f"36 depths at every point); two warm-ups each, then {pairs} alternating pairs, wall clock [ms] around evaluate; recorded, "
                   "not gated",
           "network_ms": {"median": 1e3 * float(np.median(tn)), "min": 1e3 * min(tn), "max": 1e3 * max(tn), "all": [1e3 * x for x in tn]},
           "dense_ms": {"median": 1e3 * float(np.median(td)), "min": 1e3 * min(td), "max": 1e3 * max(td), "all": [1e3 * x for x in td]},
           "eval_counts": {"network": {"launched": counts["network"][0], "dense": counts["network"][1]},
                           "dense": {"launched": counts["dense"][0], "dense": counts["dense"][1]}},
           "time_ratio_network_over_dense": ratio, "count_ratio_launched_over_dense": launched / dense,
           "time_ratio_over_count_ratio": ratio / (launched / dense),
           "nbad": {"network": int(a["nbad"].sum()), "dense": int(b["nbad"].sum())}}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
