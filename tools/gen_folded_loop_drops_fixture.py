#!/usr/bin/env python3
"""tests/golden/folded_loop_drops_parent.npz: h and dh of the calls of tests/test_gpu_folded_loop_drops.py from the
library that is loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_folded_loop_drops_fixture.py <parent commit id> [out.npz]"""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_folded_loop_drops as T

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
with tempfile.TemporaryDirectory() as d:
    res = T.run_calls(d)
ids = {r[3] for r in res.values()}
assert len(ids) == 1
arrays = {"parent_commit": np.array(commit), "parent_build_id": np.array(ids.pop())}
for tag, (h, dh, kernels, _) in res.items():
    assert any(T.KERNEL.search(k) for k in kernels), (tag, kernels)
    arrays[tag + "_h"] = h
    arrays[tag + "_dh"] = dh
np.savez_compressed(out, **arrays)
print("wrote", out, os.path.getsize(out), "bytes; build", str(arrays["parent_build_id"]))
