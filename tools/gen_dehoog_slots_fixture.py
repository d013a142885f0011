#!/usr/bin/env python3
"""tests/golden/dehoog_slots_parent.npz: h and dh of the calls of tests/test_gpu_dehoog_slots.py from the library that is
loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_dehoog_slots_fixture.py <parent commit id> [out.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_dehoog_slots as T
from unconfined_amd import engine

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
cases = T.build_cases()
res = T.run_cases(cases)
names = [c[0] for c in cases] + [g[0] for g in T.GRIDS]
off = np.concatenate([[0], np.cumsum([len(res[n][0]) for n in names])]).astype(np.int64)
np.savez_compressed(out, parent_commit=np.array(commit), parent_build_id=np.array(engine.build_id()),
                    inputs_sha256=np.array(T.inputs_digest(cases)), tags=np.array(names), offsets=off,
                    h=np.concatenate([res[n][0] for n in names]), dh=np.concatenate([res[n][1] for n in names]))
print("wrote", out, os.path.getsize(out), "bytes;", len(names), "calls,", int(off[-1]), "values; build", engine.build_id())
