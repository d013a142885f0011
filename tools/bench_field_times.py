"""Measurement behind profiles/field_times.json (recorded, not gated): the map of tools/bench_field.py -- 64 x 64 locations, 8
wells, 32 times, 2 depths -- deck neuman74_partpen, fast flavour, four free parameters, 64 members from ensemble_draw, through
ucf_field_ensemble_times with 4 limits (two first up-crossings, two recovery times; ln t as the abscissa, three quantile levels,
one horizon), beside one ucf_field_ensemble of the same members, in one process, alternating.  Expected: a times call costs what
the ensemble costs plus one launch of field_times_kernel, which reads members x limits x times x sites doubles once (64 x 4 x 32
x 8192 x 8 bytes = 0.54 GB: a fraction of a millisecond at the HBM rate where nothing stays in a cache), and a reduction over
4 x 8192 outputs in place of two over 262 144.  Both calls end in a synchronise inside the library; the host clock runs around
the calls.

    python tools/bench_field_times.py OUT.json [--calls N]   # two warm-ups each, then N (5) alternating repetitions; medians
    python tools/bench_field_times.py --once                 # one warm-up and one times call, for a kernel trace
    python tools/bench_field_times.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
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

NENS, SEED, WARMUPS = 64, 1, 2
LEVELS = (0.05, 0.5, 0.95)
LIMITS = (0.1, 0.2, 0.1, 0.2)                                    # 0.2 is the drawdown limit of tools/bench_field_ensemble.py
KINDS = ("first_above", "first_above", "last_above", "last_above")
HORIZON = 365.0


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_times.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rows = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace"] = rows
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one call, so "
                                    "calls and totals are for two ucf_field_ensemble_times; field_times_kernel runs once per call")
        mine = [r for r in rows if r["name"].startswith("field_times_kernel")]
        rep["field_times_kernel_average_ms"] = mine[0]["average_ms"] if mine else None
        if mine:
            rep["field_times_kernel_GB_per_s_of_the_series_read_once"] = rep["series_bytes_read_once_per_limit"] / (mine[0]["average_ms"] * 1e-3) / 1e9
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = ensemble_draw(theta, COV, NENS, seed=SEED)
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    field, ens_field = WellField(wells, loc, times), WellField(wells, loc, times)
    last = {}

    def ensemble():
        t0 = time.perf_counter()
        ens_field.ensemble(plan, FREE, thetas, Z, quantiles=LEVELS, limits=(LIMITS[1],))
        return time.perf_counter() - t0

    def to_limit():
        t0 = time.perf_counter()
        last["times"] = field.time_to_limit(plan, FREE, thetas, Z, LIMITS, kinds=KINDS, q=LEVELS, horizons=(HORIZON,), abscissa="lnt")
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        for _ in range(2):
            print(f"times {1e3 * to_limit():.0f} ms", flush=True)
        return
    for _ in range(WARMUPS):
        print(f"warm-up: ensemble {1e3 * ensemble():.0f} ms, times {1e3 * to_limit():.0f} ms", flush=True)
    t = {"ensemble": [], "times": []}
    for _ in range(calls):
        t["ensemble"].append(ensemble())
        t["times"].append(to_limit())
        print(f"ensemble {1e3 * t['ensemble'][-1]:.0f} ms, times {1e3 * t['times'][-1]:.0f} ms", flush=True)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    res = last["times"]
    nsite = len(loc) * len(Z)
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_ensemble_times ({len(FREE)} free parameters, {NENS} members of ensemble_draw seed {SEED}, limits {LIMITS} as {KINDS}, "
                   f"ln t as the abscissa, levels {LEVELS}, horizon {HORIZON}; mean, sd, min, max, quant, nfin, plater) against ucf_field_ensemble (mean, "
                   f"sd, min, max, quant, nfin of s and ds, pexc) of the same members: {len(loc)} locations x {len(times)} times x {len(Z)} depths, "
                   f"{len(wells)} wells, deck neuman74_partpen, fast flavour; one process, {WARMUPS} warm-ups of each call, then {calls} alternating "
                   "repetitions, wall clock [ms], medians; recorded, not gated",
           "expectation": "one times call = one ensemble plus one launch of field_times_kernel, with a smaller reduction",
           "outputs_of_the_map": len(loc) * len(times) * len(Z), "outputs_of_the_times": len(LIMITS) * nsite, "members": NENS, "limits": len(LIMITS),
           "series_bytes_read_once_per_limit": 8 * NENS * len(LIMITS) * len(times) * nsite,
           "ensemble_ms": ms(t["ensemble"]), "times_ms": ms(t["times"]),
           "times_over_ensemble": float(np.median(t["times"]) / np.median(t["ensemble"])),
           "nbad": res.nbad,
           "share_of_sites_where_a_member_is_censored": [float(np.mean(res.max[l] > times[-1])) for l in range(len(LIMITS))],
           "median_time_at_the_first_sites": [[float(v) for v in res.quant[1][l].ravel()[:4]] for l in range(len(LIMITS))],
           "share_later_than_the_horizon_mean_over_sites": [float(np.mean(res.later[0][l])) for l in range(len(LIMITS))],
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
