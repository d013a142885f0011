"""Measurement behind profiles/field_yield.json (recorded, not gated): the map of tools/bench_field.py -- 64 x 64 locations, 8
wells, 32 times, 2 depths -- deck neuman74_partpen, fast flavour, four free parameters, 64 members from ensemble_draw, through
ucf_field_yield with 4 controls (two wells each), 1024 rate patterns and a limit on every output of the last time (8 192
constrained outputs), beside one ucf_field_ensemble of the same members, in one process, alternating.  Expected: a yield call
costs what the ensemble costs plus the two new kernels -- 64 launches of field_response_kernel in place of
field_superpose_kernel and one launch of field_yield_kernel<4> (64 x 1024 x 8192 divisions).  Both calls end in a synchronise
inside the library; the host clock runs around the calls.

    python tools/bench_field_yield.py OUT.json [--calls N]   # one warm-up each, then N (2) alternating repetitions
    python tools/bench_field_yield.py --once                 # one warm-up and one yield call, for a kernel trace
    python tools/bench_field_yield.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from golden_util import load_deck                                # noqa: E402
from bench_field import Z, problem                               # noqa: E402
from bench_field_forecast import COV, FREE, kernel_rows          # noqa: E402
from unconfined_amd import WellField, engine, ensemble_draw      # noqa: E402

NENS, SEED, NCTL, NPAT, SMAX = 64, 1, 4, 1024, 4.0
LEVELS = (0.05, 0.5, 0.95)
SCALES = (1.0, 2.0)
LIMIT = 0.2                                                      # a drawdown limit of tools/bench_field_ensemble.py


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_yield.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rows = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace"] = rows
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one call, so "
                                    f"calls and totals are for two ucf_field_yield; field_response_kernel runs once per member ({NENS} per call), "
                                    f"field_yield_kernel<{NCTL}> once per call")
        for key, name in (("field_response_kernel_average_ms", "field_response_kernel"), ("field_yield_kernel_average_ms", "field_yield_kernel")):
            mine = [r for r in rows if r["name"].startswith(name)]
            rep[key] = mine[0]["average_ms"] if mine else None
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 2
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = ensemble_draw(theta, COV, NENS, seed=SEED)
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    controls = np.arange(len(wells)) % NCTL
    patterns = np.random.default_rng(SEED).uniform(0.0, 1.0, (NPAT, NCTL))
    limit = np.full((len(times), len(loc), len(Z)), np.inf)
    limit[-1] = LIMIT
    field, ens_field = WellField(wells, loc, times), WellField(wells, loc, times)
    last = {}

    def ensemble():
        t0 = time.perf_counter()
        ens_field.ensemble(plan, FREE, thetas, Z, quantiles=LEVELS, limits=(LIMIT,))
        return time.perf_counter() - t0

    def sustainable():
        t0 = time.perf_counter()
        last["yield"] = field.sustainable_yield(plan, FREE, thetas, Z, controls, patterns, limit, SMAX, q=LEVELS, levels=SCALES)
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        for _ in range(2):
            print(f"yield {1e3 * sustainable():.0f} ms", flush=True)
        return
    print(f"warm-up: ensemble {1e3 * ensemble():.0f} ms, yield {1e3 * sustainable():.0f} ms", flush=True)
    t = {"ensemble": [], "yield": []}
    for _ in range(calls):
        t["ensemble"].append(ensemble())
        t["yield"].append(sustainable())
        print(f"ensemble {1e3 * t['ensemble'][-1]:.0f} ms, yield {1e3 * t['yield'][-1]:.0f} ms", flush=True)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    res = last["yield"]
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_yield ({len(FREE)} free parameters, {NENS} members of ensemble_draw seed {SEED}, {NCTL} controls, {NPAT} patterns, "
                   f"limit {LIMIT} on every output of the last time, smax {SMAX}; every output) against ucf_field_ensemble (mean, sd, min, max, quant, "
                   f"nfin of s and ds, pexc) of the same members: {len(loc)} locations x {len(times)} times x {len(Z)} depths, {len(wells)} wells, deck "
                   f"neuman74_partpen, fast flavour; one process, one warm-up of each call, then {calls} alternating repetitions, wall clock [ms]; "
                   "recorded, not gated",
           "expectation": "one yield call = one ensemble plus the response kernel per member and one ratio-test launch",
           "outputs": len(loc) * len(times) * len(Z), "constrained_outputs": int(len(res["con"])), "members": NENS, "patterns": NPAT,
           "divisions": NENS * NPAT * int(len(res["con"])),
           "ensemble_ms": ms(t["ensemble"]), "yield_ms": ms(t["yield"]),
           "yield_over_ensemble": float(np.median(t["yield"]) / np.median(t["ensemble"])),
           "nbad": res["nbad"], "share_of_feasible_member_patterns": float(np.nanmean(res["pfeas"])),
           "median_yield_of_the_first_patterns": [float(v) for v in res["quant"][1][:4]],
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
