"""The folded water-table kernel with one depth per launch, bit for bit against the library it was restructured from.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (the lane = time grid of a fully penetrating well: what
bench.py times) lost the part of its abscissa loop that is not arithmetic -- arms issued with an empty EXEC mask, join copies,
a flag's round trip through a VGPR, fmin's canonicalisation, lapTime(p) held in registers -- and not one floating-point
operation: its h and dh must be the SAME BITS as before.  tests/golden/folded_loop_parent.npz holds what the parent build
(commit and build id inside the file) gave on an MI355X for the calls below; tools/gen_folded_loop_fixture.py wrote it.

Calls (CALLS): the C2 deck (beta = 0) at zD = 0.6, 0 and 1 and the same deck with Malama's beta = 0.5 at zD = 0.6 (the
closure's other shape of denominator), each 128 times x 8 radii
(lane = time needs 64 times; rD = 0.02 leaves the fast evaluators inside an item: hand-over to point_kernel; the large radii
put whole waves on the exponential form, the middle ones waves with lanes on both forms), and the first call once more with
every work item cut into 8 parts.  Every call must have run the folded one-depth kernel (ucf_plan_kernel_times)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "folded_loop_parent.npz")
# FAMILY 2, lane = time, any wave budget, one plan, FOLD, no depth above the screen, NZC = 1
KERNEL = re.compile(r"integrate_kernel<2, 1, \d+, false, true, false, 1, (true|false), false>")
DECK = "c2_neuman74_fullpen"
CALLS = (("c2_z06", 0.0, 0.6, {}),            # tag, Malama beta, zD, cut
         ("c2_z0", 0.0, 0.0, {}),
         ("c2_z1", 0.0, 1.0, {}),
         ("c2_beta_z06", 0.5, 0.6, {}),
         ("c2_z06_parts", 0.0, 0.6, {"UCF_NSPLIT": "8"}))
KNOBS = ("UCF_NSPLIT", "UCF_TAIL_LSPLIT", "UCF_TAIL_ITEMS", "UCF_PERSIST")

_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
dk, ts, P = load_deck(sys.argv[2])
dk.beta = float(sys.argv[5])
P = params_from_deck(dk)
pl = engine.Plan(P, mode="fast")
pl.set_timing(True)
zD = np.array([float(sys.argv[3])])
tD = np.logspace(-1, 4, 128)
rD = np.array([0.02, 0.11, 0.4, 0.7, 1.5, 3.0, 9.0, 30.0])
h, dh = pl.drawdown_grid(tD, pl.split_vector(tD), rD, zD, pl.zlay(zD))
names = [k[0] for k in pl.kernel_times()]
pl.close()
np.savez(sys.argv[4], h=h, dh=dh, kernels=np.array(names), build_id=np.array(engine.build_id()))
"""


def run_calls(outdir):
    """{tag: (h, dh, kernel names, build id)}: every call of CALLS in a process of its own (the cut is read once per process)"""
    res = {}
    for tag, beta, zD, env in CALLS:
        out = os.path.join(str(outdir), tag + ".npz")
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env)
        subprocess.run([sys.executable, "-c", _CALL_SCRIPT, ROOT, DECK, repr(zD), out, repr(beta)], check=True, env=e, timeout=600)
        with np.load(out) as d:
            res[tag] = (d["h"], d["dh"], [str(k) for k in d["kernels"]], str(d["build_id"]))
    return res


def test_folded_one_depth_kernel_keeps_every_bit(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    got = run_calls(tmp_path)
    for tag, (h, dh, kernels, _) in got.items():
        assert any(KERNEL.search(k) for k in kernels), (tag, kernels)
        for name, a in (("h", h), ("dh", dh)):
            ref = want[f"{tag}_{name}"]
            assert a.shape == ref.shape == (128, 8, 1) and a.dtype == ref.dtype == np.float64
            diff = np.flatnonzero(a.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
            assert diff.size == 0, (tag, name, diff.size, diff[:8], a.ravel()[diff[:8]], ref.ravel()[diff[:8]])
    # (the fixture itself: cutting the items did not change a bit in the parent build either)
    assert np.array_equal(want["c2_z06_h"].view(np.uint64), want["c2_z06_parts_h"].view(np.uint64))
