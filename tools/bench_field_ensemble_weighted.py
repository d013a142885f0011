"""Measurement behind profiles/field_ensemble_weighted.json (recorded, not gated): the map of tools/bench_field_ensemble.py -- 64 x
64 locations, 8 wells, 32 times, 2 depths = 262 144 outputs, deck neuman74_partpen, fast flavour, four free parameters, 64 members
of ensemble_draw, three quantile levels, two limits -- through ucf_field_ensemble_weighted, in one process, alternating:
  a) all weights 1 against the unweighted ucf_field_ensemble of the same build.  Expected: equal to within the spread, since
     the evaluation of the members is 99.99 % of the time and the reduction kernels are the only difference;
  b) every second member at weight 0.  Expected: half the time of (a): a member of weight 0 is not evaluated.
Both calls end in a synchronise inside the library; the host clock runs around the calls.

    python tools/bench_field_ensemble_weighted.py OUT.json [--calls N]   # two warm-ups each, then N (5) alternating repetitions
    python tools/bench_field_ensemble_weighted.py --once                 # one unweighted and one weighted call, for a kernel trace
    python tools/bench_field_ensemble_weighted.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
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
from bench_field_ensemble import LEVELS, LIMITS, NENS, SEED      # noqa: E402
from bench_field_forecast import COV, FREE, kernel_rows          # noqa: E402
from unconfined_amd import WellField, engine, ensemble_draw      # noqa: E402


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_ensemble_weighted.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rep["kernel_trace"] = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one ucf_field_ensemble and one "
                                    "ucf_field_ensemble_weighted with unit weights, 64 members each; the four reduction kernels are "
                                    "field_ensemble_moments_kernel, field_ensemble_quantile_kernel<64>, field_ensemble_wmoments_kernel and "
                                    "field_ensemble_wquantile_kernel<64> (two launches each)")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = ensemble_draw(theta, COV, NENS, seed=SEED)
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    field = WellField(wells, loc, times)
    ones = np.ones(NENS)
    half = np.where(np.arange(NENS) % 2 == 0, 1.0, 0.0)
    launched = {}

    def run(name, weights):
        t0 = time.perf_counter()
        res = field.ensemble(plan, FREE, thetas, Z, quantiles=LEVELS, limits=LIMITS, weights=weights)
        dt = time.perf_counter() - t0
        launched[name] = res.get("nlaunched", NENS)
        print(f"{name:10s} {1e3 * dt:.0f} ms", flush=True)
        return dt

    variants = (("unweighted", None), ("unit", ones), ("half", half))
    if "--once" in sys.argv:
        run("unweighted", None); run("unit", ones)
        return
    for _ in range(2):
        for name, w in variants:
            run(name, w)
    t = {name: [] for name, _ in variants}
    for _ in range(calls):
        for name, w in variants:
            t[name].append(run(name, w))
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    med = {k: float(np.median(v)) for k, v in t.items()}
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_ensemble_weighted against ucf_field_ensemble of the same build ({len(FREE)} free parameters, {NENS} members of "
                   f"ensemble_draw seed {SEED}, {len(LEVELS)} quantile levels, {len(LIMITS)} limits) of {len(loc)} locations x {len(times)} times x "
                   f"{len(Z)} depths, {len(wells)} wells, deck neuman74_partpen, fast flavour; one process, two warm-ups of each form, then "
                   f"{calls} alternating repetitions, wall clock [ms]; recorded, not gated",
           "expectation": "unit weights = unweighted to within the spread (the members' evaluation is 99.99 % of the time); every second member at "
                          "weight 0 = half of that (a member of weight 0 is not evaluated)",
           "outputs": len(loc) * len(times) * len(Z), "members": NENS, "members_launched": launched,
           "unweighted_ms": ms(t["unweighted"]), "weighted_unit_ms": ms(t["unit"]), "weighted_half_zero_ms": ms(t["half"]),
           "unit_over_unweighted": med["unit"] / med["unweighted"], "half_zero_over_unit": med["half"] / med["unit"],
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
