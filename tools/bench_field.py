"""Measurement behind profiles/field.json (recorded, not gated): one ucf_field_drawdown of a drawdown map -- 64 x 64 locations,
8 wells (4 real ones in two start-time groups and their images in a constant-head boundary), 32 times, 2 depths, deck
neuman74_partpen (model 5, partially penetrating), fast flavour -- and, for scale, ucf_drawdown_grid called once per group
with the arrays of ucf_field_group: the same launches without the superposition, their h and dh copied to the host.

    python tools/bench_field.py OUT.json [--calls N]       # wall clock around the calls, alternating
    python tools/bench_field.py --once                     # one warm-up + one call, for a kernel trace
    python tools/bench_field.py OUT.json --trace DIR       # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
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
from unconfined_amd import WellField, engine, images    # noqa: E402

Z = np.array([145.7, 100.0])


def problem():
    real = [(0.0, 0.0, 1.0, 0.0), (120.0, 40.0, 0.7, 0.0), (-60.0, 150.0, 0.5, 30.0), (80.0, -110.0, 0.9, 30.0)]
    wells = images(real, (1.0, 0.0, 400.0), "constant_head")
    gx, gy = np.meshgrid(np.linspace(-291.0, 389.0, 64), np.linspace(-303.0, 297.0, 64), indexing="ij")      # no node within rw of a well
    times = 10.0 ** np.linspace(0.0, 4.0, 32)
    return wells, np.stack([gx.ravel(), gy.ravel()], axis=1), times


def kernel_rows(d):
    """per-kernel rows of a rocprofv3 --kernel-trace --stats output directory: its *kernel_stats.csv, or the `kernels` view of
    the database that newer versions write instead"""
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                rows.append({"name": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                             "average_ms": float(r["AverageNs"]) / 1e6, "percent": float(r["Percentage"])})
    if not rows:
        import sqlite3
        for path in sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True)):
            con = sqlite3.connect(path)
            got = list(con.execute("select name, count(*), sum(duration) from kernels group by name order by 3 desc"))
            total = sum(g[2] for g in got)
            rows += [{"name": n.split("(")[0] if not n.startswith("(") else n[:n.index("(", 1)], "calls": k, "total_ms": ns / 1e6,
                      "average_ms": ns / 1e6 / k, "percent": 100.0 * ns / total} for n, k, ns in got]
    return rows


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rep["kernel_trace"] = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one "
                                    "call, so calls and totals are for two ucf_field_drawdown; field_superpose_kernel is the superposition")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    field = WellField(wells, loc, times)
    groups = field.groups(plan)
    zD = Z / plan.derived.Lc
    zl = plan.zlay(zD)

    def whole():
        t0 = time.perf_counter()
        field.drawdown(plan, Z)
        return time.perf_counter() - t0

    def grids():
        t0 = time.perf_counter()
        for g in groups:
            plan.drawdown_grid(g["tD"], g["sv"], g["rD"], zD, zl)
        return time.perf_counter() - t0

    whole()
    if "--once" in sys.argv:
        whole()
        return
    grids()
    tw, tg = [], []
    for _ in range(calls):
        tw.append(whole()); tg.append(grids())
    points = int(sum(len(g["tD"]) * len(g["rD"]) for g in groups))
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_drawdown of {len(loc)} locations x {len(times)} times x {len(Z)} depths, {len(wells)} wells in "
                   f"{len(groups)} groups, deck neuman74_partpen, fast flavour, against ucf_drawdown_grid once per group with the same "
                   f"arrays; one warm-up each, then {calls} alternating calls, wall clock [ms]; recorded, not gated",
           "groups": [{"nt": len(g["tD"]), "nr": len(g["rD"])} for g in groups], "grid_points": points,
           "outputs": len(loc) * len(times) * len(Z),
           "field_ms": ms(tw), "grid_calls_alone_ms": ms(tg),
           "grid_points_per_s_in_the_field_call": points / float(np.median(tw)),
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
