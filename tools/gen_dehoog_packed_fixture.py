#!/usr/bin/env python3
"""tests/golden/dehoog_packed_parent.npz: h and dh of the calls of tests/test_gpu_dehoog_packed.py from the library that is
loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_dehoog_packed_fixture.py <parent commit id> [out.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_dehoog_packed as T
from unconfined_amd import engine

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
cases = T.build_cases()
res = T.run_cases(cases)
off = np.concatenate([[0], np.cumsum([len(c[2]) for c in cases])]).astype(np.int64)
np.savez_compressed(out, parent_commit=np.array(commit), parent_build_id=np.array(engine.build_id()),
                    inputs_sha256=np.array(T.inputs_digest(cases)), tags=np.array([c[0] for c in cases]), offsets=off,
                    h=np.concatenate([res[c[0]][0] for c in cases]), dh=np.concatenate([res[c[0]][1] for c in cases]))
print("wrote", out, os.path.getsize(out), "bytes;", len(cases), "calls,", int(off[-1]), "vectors; build", engine.build_id())
