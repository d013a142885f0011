"""Measurement behind profiles/field_allocate.json (recorded, not gated): the map and the members of tools/bench_field_yield.py --
64 x 64 locations, 8 wells, 32 times, 2 depths, deck neuman74_partpen, fast flavour, four free parameters, 64 members from
ensemble_draw, 4 controls (two wells each), a limit on every output of the last time (8 192 constrained outputs) -- through
ucf_field_allocate with 2 objectives and the reliability stage, beside one ucf_field_yield of the same members with its 1024
patterns, in one process, alternating.  Expected: an allocate call costs what a yield call costs plus field_allocate_kernel<4>,
which rereads a member's R once per iteration (and, here, minus the 1024-pattern ratio test of the yield call, plus a 128-pattern
one).  Both calls end in a synchronise inside the library; the host clock runs around the calls.

    python tools/bench_field_allocate.py OUT.json [--calls N]   # 2 warm-ups each, then N (5) alternating repetitions, medians
    python tools/bench_field_allocate.py --once                 # one warm-up and one allocate call, for a kernel trace
    python tools/bench_field_allocate.py OUT.json --trace DIR   # add the per-kernel rows of a rocprofv3 --kernel-trace --stats run of --once
    python tools/bench_field_allocate.py OUT.json --certificate # add the worst error ratio of tests/test_field_allocate_host.py (no GPU)
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

from unconfined_amd import lib as ucflib                         # noqa: E402

NOBJ, MAXIT, XMAX, WARMUPS = 2, 64, 4.0, 2


def load_report(out):
    return json.load(open(out)) if os.path.exists(out) else {}


def dump_report(rep, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1, sort_keys=True)


def certificate(out):
    """the exact certificate of tests/test_field_allocate_host.py: the error of x against the exact vertex over LAPACK's"""
    import test_field_allocate_host as T
    so = ucflib.load()
    per = {}
    for nctl in range(1, 9):
        ratios = T.certificate_ratios(so, nctl)
        some = [r for r in ratios if r is not None]
        per[str(nctl)] = {"cases": len(ratios), "both_exact": len(ratios) - len(some), "worst_ratio": max(some) if some else 0.0}
    rep = load_report(out)
    rep["certificate"] = {"what": f"nctl 1..8, ncon {T.CERT_NCON}, {len(T.CERT_SEEDS)} seeds each: every reported working set proven optimal in exact "
                                  "rational arithmetic; ratio = error of x against the exact vertex over the error of numpy.linalg.solve on the "
                                  f"same system, margin {T.MARGIN}",
                          "per_nctl": per, "worst_ratio": max(v["worst_ratio"] for v in per.values()), "margin": T.MARGIN}
    dump_report(rep, out)
    print(json.dumps(rep["certificate"]))


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "field_allocate.json"))
    if "--certificate" in sys.argv:
        return certificate(out)
    from golden_util import load_deck
    from bench_field import Z, problem
    from bench_field_forecast import COV, FREE, kernel_rows
    from bench_field_yield import LEVELS, LIMIT, NCTL, NENS, NPAT, SCALES, SEED, SMAX
    from unconfined_amd import WellField, engine, ensemble_draw
    if "--trace" in sys.argv:
        rep = load_report(out)
        rows = kernel_rows(sys.argv[sys.argv.index("--trace") + 1])
        rep["kernel_trace"] = rows
        rep["kernel_trace_what"] = ("rocprofv3 --kernel-trace --stats of `--once`, a run of its own without counters: one warm-up and one call, so "
                                    f"calls and totals are for two ucf_field_allocate; field_response_kernel runs once per member ({NENS} per call), "
                                    f"field_allocate_kernel<{NCTL}> and field_yield_kernel<{NCTL}> (the reliability stage) once per call")
        for key, name in (("field_allocate_kernel_average_ms", "field_allocate_kernel"), ("field_yield_kernel_average_ms", "field_yield_kernel"),
                          ("field_response_kernel_average_ms", "field_response_kernel")):
            mine = [r for r in rows if r["name"].startswith(name)]
            rep[key] = mine[0]["average_ms"] if mine else None
        dump_report(rep, out)
        return
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 5
    _, _, P = load_deck("neuman74_partpen")
    theta = np.array([getattr(P, n) for n in FREE])
    thetas = ensemble_draw(theta, COV, NENS, seed=SEED)
    plan = engine.Plan(P, mode="fast")
    wells, loc, times = problem()
    controls = np.arange(len(wells)) % NCTL
    patterns = np.random.default_rng(SEED).uniform(0.0, 1.0, (NPAT, NCTL))
    objectives = np.ones((NOBJ, NCTL))
    objectives[1] = np.linspace(1.0, 0.25, NCTL)
    limit = np.full((len(times), len(loc), len(Z)), np.inf)
    limit[-1] = LIMIT
    field, yield_field = WellField(wells, loc, times), WellField(wells, loc, times)
    last = {}

    def sustainable():
        t0 = time.perf_counter()
        yield_field.sustainable_yield(plan, FREE, thetas, Z, controls, patterns, limit, SMAX, q=LEVELS, levels=SCALES)
        return time.perf_counter() - t0

    def allocate():
        t0 = time.perf_counter()
        last["res"] = field.optimal_rates(plan, FREE, thetas, Z, controls, objectives, XMAX, limit, q=LEVELS, maxit=MAXIT)
        return time.perf_counter() - t0

    if "--once" in sys.argv:
        for _ in range(2):
            print(f"allocate {1e3 * allocate():.0f} ms", flush=True)
        return
    for _ in range(WARMUPS):
        print(f"warm-up: yield {1e3 * sustainable():.0f} ms, allocate {1e3 * allocate():.0f} ms", flush=True)
    t = {"yield": [], "allocate": []}
    for _ in range(calls):
        t["yield"].append(sustainable())
        t["allocate"].append(allocate())
        print(f"yield {1e3 * t['yield'][-1]:.0f} ms, allocate {1e3 * t['allocate'][-1]:.0f} ms", flush=True)
    ms = lambda v: {"median": 1e3 * float(np.median(v)), "min": 1e3 * min(v), "max": 1e3 * max(v), "all": [1e3 * x for x in v]}
    res = last["res"]
    iters, counts = np.unique(res.iters, return_counts=True)
    rep = load_report(out)
    rep.update({
        "build_id": engine.build_id(),
        "what": f"ucf_field_allocate ({len(FREE)} free parameters, {NENS} members of ensemble_draw seed {SEED}, {NCTL} controls, {NOBJ} objectives, xmax "
                f"{XMAX}, maxit {MAXIT}, limit {LIMIT} on every output of the last time, the reliability stage at q = {list(LEVELS)}; every output) "
                f"against ucf_field_yield ({NPAT} patterns, smax {SMAX}, every statistic) of the same members: {len(loc)} locations x {len(times)} "
                f"times x {len(Z)} depths, {len(wells)} wells, deck neuman74_partpen, fast flavour; one process, {WARMUPS} warm-ups of each call, then "
                f"{calls} alternating repetitions, wall clock [ms], medians; recorded, not gated",
        "expectation": "one allocate call = one yield call plus a kernel that rereads a member's R once per iteration",
        "constrained_outputs": int(len(res.con)), "members": NENS, "objectives": NOBJ,
        "yield_ms": ms(t["yield"]), "allocate_ms": ms(t["allocate"]),
        "allocate_over_yield": float(np.median(t["allocate"]) / np.median(t["yield"])),
        "iters_histogram": {str(int(i)): int(c) for i, c in zip(iters, counts)},
        "status_histogram": {str(int(s)): int(c) for s, c in zip(*np.unique(res.status, return_counts=True))},
        "nbad": res.nbad, "g_of_the_first_members": [[float(v) for v in row] for row in res.g[:4]],
        "gquant": [[float(v) for v in row] for row in res.gquant], "best": res.best.tolist(),
        "value_of_best": [[float(res.value[iq, p]) if p >= 0 else None for p in row] for iq, row in enumerate(res.best)],
        "device_allocations_of_the_field": field.alloc_count()})
    dump_report(rep, out)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
