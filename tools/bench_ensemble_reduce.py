"""Measurement behind profiles/ensemble_reduce_refactor.json: the ensemble reduction kernels of this build against the
library built from the parent commit (loaded through UCF_LIB_PATH), on synthetic data through the two debug hooks.

    python tools/bench_ensemble_reduce.py --once NENS NOUT
        one process: ucf_debug_ensemble and ucf_debug_ensemble_weighted on a seeded [NENS][NOUT], three levels and two limits
        (those of tools/bench_field_ensemble.py), every statistic asked for; one warm-up call and one measured call of each, so a
        kernel trace of the process holds two dispatches per kernel
    python tools/bench_ensemble_reduce.py --collect DIR OUT.json PARENT_COMMIT
        DIR holds one `rocprofv3 --kernel-trace --stats` directory per process, named {parent,new}_{NENS}x{NOUT}_{run}, and
        {parent,new}.build_id; tools/ensemble_reduce_ab.sh makes them, parent and new alternating.  Writes both series, medians,
        the parent's spread and the rule: median(new) <= median(parent) + (max - min of the parent's runs)
"""
import ctypes as C
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = (0.05, 0.5, 0.95)
LIMITS = (0.05, 0.2)
KERNELS = ("field_ensemble_moments_kernel", "field_ensemble_wmoments_kernel", "field_ensemble_quantile_kernel", "field_ensemble_wquantile_kernel")


def once(nens, nout):
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    rng = np.random.default_rng(nens)
    a = rng.standard_normal((nens, nout)) * 0.1 + 0.1
    w = np.ascontiguousarray(rng.uniform(0.1, 1.0, nens))
    q, lim = np.array(LEVELS), np.array(LIMITS)
    out = {k: np.empty((len(q), nout) if k == "quant" else nout, np.int32 if k == "nfin" else np.float64)
           for k in ("mean", "sd", "min", "max", "quant", "nfin")}
    m = abi.UcfEnsembleMaps()
    for k, v in out.items():
        setattr(m, k, v.ctypes.data)
    pexc, nbad = np.empty((len(lim), nout)), np.zeros(1, np.int64)
    for _ in range(2):
        ucflib.check(so.ucf_debug_ensemble(nens, nout, a.ctypes.data, len(q), q.ctypes.data, len(lim), lim.ctypes.data, C.byref(m),
                                           pexc.ctypes.data, nbad.ctypes.data))
        ucflib.check(so.ucf_debug_ensemble_weighted(nens, nout, a.ctypes.data, w.ctypes.data, len(q), q.ctypes.data, len(lim), lim.ctypes.data,
                                                    C.byref(m), pexc.ctypes.data, nbad.ctypes.data))
    print(f"nens={nens} nout={nout} build {so.ucf_build_id().decode()} median of the weighted median map {np.median(out['quant'][1]):.6f}", flush=True)


def collect(d, out, parent_commit):
    from bench_field_forecast import kernel_rows
    runs = {}
    for path in sorted(glob.glob(os.path.join(d, "*_*x*_*"))):
        m = re.fullmatch(r"(parent|new)_(\d+x\d+)_(\d+)", os.path.basename(path))
        if m and os.path.isdir(path):
            for r in kernel_rows(path):
                if r["name"].split("<")[0] in KERNELS:
                    assert r["calls"] == 2, (path, r)
                    runs.setdefault((m.group(2), r["name"]), {}).setdefault(m.group(1), []).append(round(1e3 * r["total_ms"], 3))
    rep = {"what": "total time of the ensemble reduction kernel rows of `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) over one "
                   "process of `tools/bench_ensemble_reduce.py --once NENS NOUT` (one warm-up and one call of each debug hook), in microseconds "
                   "for both dispatches together; the library built from the parent commit and from this one, alternated parent / new in one "
                   "session on one MI355X, three runs each, per shape NENSxNOUT.  Check: median of the new build <= median of the parent + the "
                   "parent's own spread (max - min of its three runs).",
           "parent_commit": parent_commit,
           "parent_build_id": open(os.path.join(d, "parent.build_id")).read().strip(),
           "new_build_id": open(os.path.join(d, "new.build_id")).read().strip()}
    for (shape, name), s in sorted(runs.items()):
        p, n = s["parent"], s["new"]
        spread = round(max(p) - min(p), 3)
        rep.setdefault(shape, {})[name] = {"dispatches_per_run": 2, "parent_total_us": p, "new_total_us": n, "parent_median_us": float(np.median(p)),
                                           "new_median_us": float(np.median(n)), "parent_spread_us": spread,
                                           "met": bool(np.median(n) <= np.median(p) + spread)}
    with open(out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps(rep))


if __name__ == "__main__":
    if sys.argv[1] == "--once":
        once(int(sys.argv[2]), int(sys.argv[3]))
    else:
        collect(*sys.argv[2:5])
