"""Measurement behind profiles/field_sobol.json (recorded, not gated): the map of tools/bench_field.py -- 64 x 64 locations, 8
wells, 32 times, 2 depths -- deck neuman74_partpen, fast flavour, the four free parameters and COV of
tools/bench_field_forecast.py, a Saltelli design of nbase = 8 (sobol_design, only the diagonal of COV), 48 members, through
ucf_field_sobol (every statistic of s and of ds) beside one ucf_field_ensemble of the same 48 members on a second field, in one
process, alternating.  Expected: a ratio near 1 -- the members dominate; the reduction reads the slots of a map twice, 2 x 6 x 8 x
nout x 8 bytes, a fraction of a millisecond at the HBM rate.  Both calls end in a synchronise inside the library; the host clock
runs around the calls.

    python tools/bench_field_sobol.py OUT.json [--calls N]   # one warm-up each, then N (3) alternating repetitions; medians
    python tools/bench_field_sobol.py --once                 # one warm-up and one Sobol call, for a kernel trace
    python tools/bench_field_sobol.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
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
from unconfined_amd import WellField, engine, sobol_design       # noqa: E402

NBASE, SEED, WARMUPS = 8, 1, 1
LEVELS = (0.05, 0.5, 0.95)


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_sobol.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rows = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace"] = rows
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one call, so "
                                    "calls and totals are for two ucf_field_sobol; field_sobol_kernel runs twice per call, on s and on ds")
        mine = [r for r in rows if "field_sobol_kernel" in r["name"]]
        rep["field_sobol_kernel_average_ms"] = mine[0]["average_ms"] if mine else None
        if mine:
            rep["field_sobol_kernel_GB_per_s_of_the_slots_read_twice"] = rep["slot_bytes_read_twice_per_map"] / (mine[0]["average_ms"] * 1e-3) / 1e9
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 3
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = sobol_design(theta, COV, NBASE, seed=SEED)
    nmem = len(thetas)
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    field, ens_field = WellField(wells, loc, times), WellField(wells, loc, times)
    last = {}

    def ensemble():
        t0 = time.perf_counter()
        ens_field.ensemble(plan, FREE, thetas, Z, quantiles=LEVELS)
        return time.perf_counter() - t0

    def sobol():
        t0 = time.perf_counter()
        last["sobol"] = field.sobol(plan, FREE, thetas, Z)
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        for _ in range(2):
            print(f"sobol {1e3 * sobol():.0f} ms", flush=True)
        return
    for _ in range(WARMUPS):
        print(f"warm-up: ensemble {1e3 * ensemble():.0f} ms, sobol {1e3 * sobol():.0f} ms", flush=True)
    t = {"ensemble": [], "sobol": []}
    for _ in range(calls):
        t["ensemble"].append(ensemble())
        t["sobol"].append(sobol())
        print(f"ensemble {1e3 * t['ensemble'][-1]:.0f} ms, sobol {1e3 * t['sobol'][-1]:.0f} ms", flush=True)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    res = last["sobol"]
    nout = len(loc) * len(times) * len(Z)
    ok = res.var > 0.0
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_sobol ({len(FREE)} free parameters {FREE}, a design of nbase = {NBASE} from sobol_design seed {SEED}: {nmem} members; S, ST, "
                   f"seS, seST, mean, var, nrow of s and of ds) against ucf_field_ensemble (mean, sd, min, max, quant at {LEVELS}, nfin of s and ds) of "
                   f"the same {nmem} members on a second field: {len(loc)} locations x {len(times)} times x {len(Z)} depths, {len(wells)} wells, deck "
                   f"neuman74_partpen, fast flavour; one process, {WARMUPS} warm-up of each call, then {calls} alternating repetitions, wall clock [ms], "
                   "medians (a call takes about 20 s: the whole run stays within a few minutes); recorded, not gated",
           "expectation": "a ratio near 1: the members dominate, the reduction is two launches of field_sobol_kernel",
           "outputs_of_the_map": nout, "members": nmem, "nbase": NBASE,
           "slot_bytes_read_twice_per_map": 2 * (len(FREE) + 2) * NBASE * nout * 8,
           "ensemble_ms": ms(t["ensemble"]), "sobol_ms": ms(t["sobol"]),
           "sobol_over_ensemble": float(np.median(t["sobol"]) / np.median(t["ensemble"])),
           "nbad": res.nbad.tolist(),
           "share_of_outputs_with_positive_variance": float(np.mean(ok)),
           "median_over_outputs_of_S": [float(np.median(res.S[j][ok])) for j in range(len(FREE))],
           "median_over_outputs_of_ST": [float(np.median(res.ST[j][ok])) for j in range(len(FREE))],
           "median_over_outputs_of_seS": [float(np.median(res.se_S[j][ok])) for j in range(len(FREE))],
           "median_over_outputs_of_seST": [float(np.median(res.se_ST[j][ok])) for j in range(len(FREE))],
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
