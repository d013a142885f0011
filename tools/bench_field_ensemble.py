"""Measurement behind profiles/field_ensemble.json (recorded, not gated): one ucf_field_ensemble of the map of
tools/bench_field.py -- 64 x 64 locations, 8 wells, 32 times, 2 depths, deck neuman74_partpen (model 5, partially
penetrating), fast flavour -- with four free parameters (Kr, kappa, Ss, Sy), 64 members from ensemble_draw, three quantile
levels and two drawdown limits, against what it replaces: 64 times ucf_plan_update + ucf_field_drawdown over the same members,
every map copied to the host (the statistics are then still to be formed there).  Both forms end in a synchronise inside the
library; the host clock runs around the calls.

    python tools/bench_field_ensemble.py OUT.json [--calls N]    # two warm-ups each, then N (5) alternating repetitions
    python tools/bench_field_ensemble.py --once                  # one warm-up + one ensemble, for a kernel trace
    python tools/bench_field_ensemble.py OUT.json --trace DIR    # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
"""
import ctypes as C
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
from unconfined_amd import lib as ucflib                         # noqa: E402
from unconfined_amd.fit import par_id                            # noqa: E402

NENS, SEED = 64, 1
LEVELS = (0.05, 0.5, 0.95)
LIMITS = (0.05, 0.2)


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_ensemble.json"))
    if "--trace" in sys.argv:
        rep = json.load(open(out))
        rep["kernel_trace"] = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one "
                                    "call, so calls and totals are for two ucf_field_ensemble; field_ensemble_moments_kernel and "
                                    "field_ensemble_quantile_kernel<64> are the reduction (two launches each per call)")
        json.dump(rep, open(out, "w"), indent=1, sort_keys=True)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = ensemble_draw(theta, COV, NENS, seed=SEED)
    so = ucflib.load()
    ids = np.ascontiguousarray([par_id(n) for n in FREE], dtype=np.int32)
    members = []
    for th in thetas:
        Pm = type(P)()
        ucflib.check(so.ucf_fit_perturb(C.byref(P), len(ids), ids, np.ascontiguousarray(th), C.byref(Pm)))
        members.append(Pm)
    plan = engine.Plan(P, mode="fast")              # the caller's plan of the ensemble
    loop_plan = engine.Plan(P, mode="fast")         # the plan that the hand-written loop refreshes
    wells, loc, times = problem()
    field, loop_field = WellField(wells, loc, times), WellField(wells, loc, times)

    def ensemble():
        t0 = time.perf_counter()
        field.ensemble(plan, FREE, thetas, Z, quantiles=LEVELS, limits=LIMITS)
        dt = time.perf_counter() - t0
        print(f"ensemble {1e3 * dt:.0f} ms", flush=True)
        return dt

    def by_hand():
        t0 = time.perf_counter()
        for Pm in members:
            loop_plan.update(Pm)
            loop_field.drawdown(loop_plan, Z)
        dt = time.perf_counter() - t0
        print(f"by hand  {1e3 * dt:.0f} ms", flush=True)
        return dt

    ensemble()
    if "--once" in sys.argv:
        ensemble()
        return
    ensemble(); by_hand(); by_hand()
    te, th = [], []
    for _ in range(calls):
        te.append(ensemble()); th.append(by_hand())
    nout, nq, nlim = len(loc) * len(times) * len(Z), len(LEVELS), len(LIMITS)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_field_ensemble ({len(FREE)} free parameters, {NENS} members of ensemble_draw seed {SEED}, {nq} quantile levels, {nlim} "
                   f"limits; mean, sd, min, max, quant, nfin of s and of ds, pexc) of {len(loc)} locations x {len(times)} times x {len(Z)} depths, "
                   f"{len(wells)} wells, deck neuman74_partpen, fast flavour, against {NENS} x (ucf_plan_update + ucf_field_drawdown) in the "
                   f"same process; two warm-ups each, then {calls} alternating repetitions, wall clock [ms]; recorded, not gated",
           "outputs": nout, "members": NENS,
           "ensemble_ms": ms(te), "field_calls_by_hand_ms": ms(th),
           "ensemble_over_by_hand": float(np.median(te)) / float(np.median(th)),
           # from the shapes: per map mean, sd, min, max [nout] and quant [nq][nout] in doubles and nfin in int32, pexc [nlim][nout];
           # by hand every member returns s, ds
           "bytes_to_host_ensemble": 2 * nout * (8 * (4 + nq) + 4) + 8 * nout * nlim, "bytes_to_host_by_hand": 8 * nout * 2 * NENS,
           "device_allocations_of_the_field": field.alloc_count()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
