"""Measurement behind profiles/field_worth.json (recorded, not gated): the map of tools/bench_field.py -- 64 x 64 locations, 8
wells, 32 times, 2 depths = 262 144 outputs, 8 192 candidate wells -- deck neuman74_partpen, fast flavour, four free parameters,
three targets, four picks, through ucf_field_worth, beside one ucf_field_forecast with all outputs on the same inputs, in one
process, alternating.  Expected: a worth call costs one forecast plus a negligible amount -- the evaluation of the nine
parameter sets is the same, and four launches of field_worth_kernel<4> on 8 192 candidates with eight small gathers stand
against the forecast's two combination launches and the maps it copies back.  Both calls end in a synchronise inside the
library; the host clock runs around the calls.

    python tools/bench_field_worth.py OUT.json [--calls N]   # two warm-ups each, then N (3) alternating repetitions
    python tools/bench_field_worth.py --once                 # one warm-up and one worth call, for a kernel trace
    python tools/bench_field_worth.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
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
from bench_field_forecast import COV, DLOG, FREE, kernel_rows    # noqa: E402
from unconfined_amd import WellField, engine                     # noqa: E402

SIGMA_S, SIGMA_D, PICKS = 0.01, 0.05, 4
# the drawdown at the last time in two corners of the map and its derivative in the middle of the time axis near the centre
TARGETS = [("s", 31, 0, 0), ("s", 31, 64 * 64 - 1, 1), ("ds", 16, 32 * 64 + 32, 0)]


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_worth.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rows = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace"] = rows
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one call, so "
                                    f"calls and totals are for two ucf_field_worth of {PICKS} picks each; field_worth_kernel<4> runs once per pick, "
                                    "field_gather_kernel twice for the targets and twice per pick")
        mine = [r for r in rows if r["name"].startswith("field_worth_kernel")]
        rep["field_worth_kernel_average_ms"] = mine[0]["average_ms"] if mine else None
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 3
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    field = WellField(wells, loc, times)
    last = {}

    def forecast():
        t0 = time.perf_counter()
        field.forecast(plan, FREE, theta, Z, cov=COV, dlog=DLOG)
        return time.perf_counter() - t0

    def worth():
        t0 = time.perf_counter()
        last["worth"] = field.worth(plan, FREE, theta, COV, Z, TARGETS, SIGMA_S, sigma_d=SIGMA_D, picks=PICKS, dlog=DLOG)
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        for _ in range(2):
            print(f"worth {1e3 * worth():.0f} ms", flush=True)
        return
    for _ in range(2):
        print(f"warm-up: forecast {1e3 * forecast():.0f} ms, worth {1e3 * worth():.0f} ms", flush=True)
    t = {"forecast": [], "worth": []}
    for _ in range(calls):
        t["forecast"].append(forecast())
        t["worth"].append(worth())
        print(f"forecast {1e3 * t['forecast'][-1]:.0f} ms, worth {1e3 * t['worth'][-1]:.0f} ms", flush=True)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    res = last["worth"]
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_worth ({len(FREE)} free parameters, {len(TARGETS)} targets, {PICKS} picks, sigma_s = {SIGMA_S}, sigma_d = {SIGMA_D}, every "
                   f"output) against ucf_field_forecast (s, ds, sens, dsens, se, dse) on the same inputs: {len(loc)} locations x {len(times)} times x "
                   f"{len(Z)} depths, {len(wells)} wells, deck neuman74_partpen, fast flavour; one process, two warm-ups of each call, then {calls} "
                   "alternating repetitions, wall clock [ms]; recorded, not gated",
           "expectation": "one worth call = one forecast plus a negligible amount: the nine parameter sets are evaluated by the same launch sequence",
           "outputs": len(loc) * len(times) * len(Z), "candidates": len(loc) * len(Z),
           "forecast_ms": ms(t["forecast"]), "worth_ms": ms(t["worth"]),
           "worth_over_forecast": float(np.median(t["worth"]) / np.median(t["forecast"])),
           "picks": res["pick"], "prior": res["prior"].tolist(), "largest_reduction_per_round": [float(np.nanmax(r)) for r in res["reduction"]],
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
