"""Measurement behind profiles/field_forecast.json (recorded, not gated): one ucf_field_forecast of the map of
tools/bench_field.py -- 64 x 64 locations, 8 wells, 32 times, 2 depths, deck neuman74_partpen (model 5, partially
penetrating), fast flavour -- with four free parameters (Kr, kappa, Ss, Sy), against what it replaces: nine times
ucf_plan_update + ucf_field_drawdown over the same nine parameter sets, every map copied to the host.  Both forms end in a
synchronise inside the library; the host clock runs around the calls.

    python tools/bench_field_forecast.py OUT.json [--calls N]    # two warm-ups each, then N (5) alternating repetitions
    python tools/bench_field_forecast.py --once                  # one warm-up + one forecast, for a kernel trace
    python tools/bench_field_forecast.py OUT.json --trace DIR    # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
"""
import csv
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from golden_util import load_deck                                # noqa: E402
from bench_field import Z, problem                               # noqa: E402
from unconfined_amd import WellField, engine, forecast_sets      # noqa: E402

FREE = ["Kr", "kappa", "Ss", "Sy"]
DLOG = 1e-3
COV = np.diag([0.0025, 0.0036, 0.0016, 0.0049])


def kernel_name(n):
    """`void (anonymous namespace)::field_forecast_kernel<4>(long long, ...)` -> `field_forecast_kernel<4>`"""
    n = n.replace("(anonymous namespace)::", "")
    return (n[5:] if n.startswith("void ") else n).split("(")[0]


def kernel_rows(d):
    """per-kernel rows of a rocprofv3 --kernel-trace --stats output directory (its *kernel_stats.csv, or the `kernels` view of
    the database that newer versions write instead), as tools/bench_field.py reads them but with the kernels of an anonymous
    namespace named"""
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                rows.append({"name": kernel_name(r["Name"]), "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                             "average_ms": float(r["AverageNs"]) / 1e6, "percent": float(r["Percentage"])})
    if not rows:
        for path in sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True)):
            got = list(sqlite3.connect(path).execute("select name, count(*), sum(duration) from kernels group by name order by 3 desc"))
            total = sum(g[2] for g in got)
            rows += [{"name": kernel_name(n), "calls": k, "total_ms": ns / 1e6, "average_ms": ns / 1e6 / k, "percent": 100.0 * ns / total}
                     for n, k, ns in got]
    return rows


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_forecast.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rep["kernel_trace"] = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one "
                                    "call, so calls and totals are for two ucf_field_forecast; field_forecast_kernel is the combination "
                                    "(two launches per call)")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    sets = forecast_sets(P, FREE, theta, DLOG)
    plan = engine.Plan(P, mode="fast")              # the caller's plan of the forecast
    loop_plan = engine.Plan(P, mode="fast")         # the plan that the hand-written loop refreshes
    wells, loc, times = problem()
    field, loop_field = WellField(wells, loc, times), WellField(wells, loc, times)

    def forecast():
        t0 = time.perf_counter()
        field.forecast(plan, FREE, theta, Z, cov=COV, dlog=DLOG)
        return time.perf_counter() - t0

    def by_hand():
        t0 = time.perf_counter()
        for Pk in sets:
            loop_plan.update(Pk)
            loop_field.drawdown(loop_plan, Z)
        return time.perf_counter() - t0

    forecast()
    if "--once" in sys.argv:
        forecast()
        return
    forecast(); by_hand(); by_hand()
    tf, th = [], []
    for _ in range(calls):
        tf.append(forecast()); th.append(by_hand())
    nout, npar = len(loc) * len(times) * len(Z), len(FREE)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_forecast ({npar} free parameters: s, ds, sens, dsens, se, dse) of {len(loc)} locations x {len(times)} times x "
                   f"{len(Z)} depths, {len(wells)} wells, deck neuman74_partpen, fast flavour, against {len(sets)} x (ucf_plan_update + "
                   f"ucf_field_drawdown) in the same process; two warm-ups each, then {calls} alternating repetitions, wall clock [ms]; "
                   f"recorded, not gated",
           "outputs": nout, "parameter_sets": len(sets),
           "forecast_ms": ms(tf), "field_calls_by_hand_ms": ms(th),
           "forecast_over_by_hand": float(np.median(tf)) / float(np.median(th)),
           # from the shapes: the forecast returns s, ds, se, dse [nout] and sens, dsens [npar][nout]; by hand every set returns s, ds
           "bytes_to_host_forecast": 8 * nout * (4 + 2 * npar), "bytes_to_host_by_hand": 8 * nout * 2 * len(sets),
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
