#!/usr/bin/env python3
"""tests/golden/finish_loads_parent.npz: h and dh of the calls of tests/test_gpu_finish_loads.py from the library that is
loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).  The `guard` call runs the first grid of
GUARD_GRIDS on which that library counts all-zero series, early exits or truncated series in the epsilon tables; the file
names the grid and keeps the counts.
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_finish_loads_fixture.py <parent commit id> [out.npz]"""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_finish_loads as T

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
with tempfile.TemporaryDirectory() as d:
    guard_grid = None
    for g in range(len(T.GUARD_GRIDS)):
        counts = T.run_calls(d, g, ["guard"])["guard"][4]
        print("guard grid", g, dict(zip(T.GUARD_COUNTERS, counts.tolist())))
        if counts.sum() > 0:
            guard_grid = g
            break
    assert guard_grid is not None, "no grid of GUARD_GRIDS needs the guarded epsilon table: add another"
    res = T.run_calls(d, guard_grid)
ids = {r[3] for r in res.values()}
assert len(ids) == 1
arrays = {"parent_commit": np.array(commit), "parent_build_id": np.array(ids.pop()),
          "guard_grid": np.array(guard_grid), "guard_stats": res["guard"][4]}
assert int(arrays["guard_stats"].sum()) > 0
for tag, (h, dh, kernels, _, _) in res.items():
    fk = T.finish_kernels(kernels)
    print(tag, h.shape, "finite", int(np.isfinite(h).sum()), "of", h.size, fk)
    assert fk, (tag, kernels)
    arrays[tag + "_h"] = h
    arrays[tag + "_dh"] = dh
np.savez_compressed(out, **arrays)
print("wrote", out, os.path.getsize(out), "bytes; build", str(arrays["parent_build_id"]))
