#!/usr/bin/env python3
"""tests/golden/launch_names_parent.json: the kernel names, in launch order, of the cases of tests/test_gpu_launch_plan.py from
the library that is loaded (UCF_LIB_PATH = the build of the commit to compare with; needs a GPU).  One fresh child process per
environment setting, as in the test.  The names are stored once and the lists as indices into them.
usage: UCF_LIB_PATH=/path/to/parent/libucf.so tools/gen_launch_names_fixture.py <parent commit id> [out.json]"""
import json, os, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_launch_plan as T

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
assert len(commit) == 40, "full commit id"
names, settings = [], {}
with tempfile.TemporaryDirectory() as tmp:
    for s in T.SETTINGS:
        cases = T.run_setting(s, tmp)
        for lst in cases.values():
            names += [n for n in lst if n not in names]
        settings[s] = {c: [names.index(n) for n in lst] for c, lst in cases.items()}
        print(repr(s), len(cases), "cases,", sum(len(v) for v in cases.values()), "launches", flush=True)
with open(out, "w") as f:
    json.dump({"parent_commit": commit, "names": names, "settings": settings}, f, separators=(",", ":"))
    f.write("\n")
print("wrote", out, os.path.getsize(out), "bytes;", len(names), "distinct names")
