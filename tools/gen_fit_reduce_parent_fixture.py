#!/usr/bin/env python3
"""tests/golden/fit_reduce_parent.npz: the inputs and results of the calls of tests/test_gpu_fit_reduce_parent.py from the
library that is loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).  Only unconfined_amd.fit is
called, so the same script runs on either build.
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_fit_reduce_parent_fixture.py <parent commit id> [out.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_fit_reduce_parent as T
from unconfined_amd import engine, fit

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
data = dict(parent_commit=np.array(commit), parent_build_id=np.array(engine.build_id()))
for kind in T.KINDS:
    t, place, iz = T.layout(kind)
    obs, dobs = T.parent_observations(fit, kind)
    assert np.isfinite(obs).all() and np.isfinite(dobs).all(), kind
    res = T.run_calls(fit, kind, t, place, iz, obs, dobs)
    again = T.run_calls(fit, kind, t, place, iz, obs, dobs)
    assert all(np.asarray(res[k]).tobytes() == np.asarray(again[k]).tobytes() for k in res), (kind, "the library does not repeat itself")
    data.update({f"{kind}_in_{k}": v for k, v in zip(("t", "place", "iz", "obs", "dobs"), (t, place, iz, obs, dobs))})
    data.update({f"{kind}_out_{k}": v for k, v in res.items()})
    print(kind, len(res), "results; phi", res[f"p{len(T.geometry(kind)['free'])}_joint_phi"], "lm iters", res["lm_joint_iters"], flush=True)
np.savez_compressed(out, **data)
print("wrote", out, os.path.getsize(out), "bytes; build", engine.build_id())
