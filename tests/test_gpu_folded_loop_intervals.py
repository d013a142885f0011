"""The folded water-table kernel with one depth per launch: whole J0 intervals decided once, bit for bit against the parent.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (the lane = time grid of a fully penetrating well: what
bench.py times) evaluates eta at the two ends of every J0 interval before the interval's first Gauss-Lobatto node
(zpair_interval_class, ucf_fastpath.h).  Re eta grows with the abscissa and |Im eta| falls, so the two ends settle for all
nodes of the interval and every lane: the range tests, the form of the closure (cosh/sinh below Re eta = maxexp,
exponential above) and whether every sin/cos argument is below UCF_SC_SMALL.  A proven interval runs a loop that holds the
one arm of its class and no test; any other runs the loop with the UCF_PH_* bits as before.  Not one floating-point operation
that reaches a result moved: h and dh must be the SAME BITS as before.  tests/golden/folded_loop_intervals_parent.npz holds
what the parent build (commit and build id inside the file) gave on an MI355X for the calls below;
tools/gen_folded_loop_intervals_fixture.py wrote it.

Calls (CALLS): the C2 deck (beta = 0) at the bench's depth zD = 0.9106, at the interior depth 0.4, at 0 and at 1, the same
deck with Malama's beta = 0.5 at zD = 0.9106, 1 and 0; zD = 0.9106 and (beta = 0.5) zD = 0.4 once more with every work item
cut into 8 parts (UCF_NSPLIT=8: a part starts at an interval boundary with cleared bits).  Each 256 times (lane = time needs
64) in four groups of 64, half a decade each, from tD = 10^-2, 1, 10^2 and 10^4 -- a wave is 64 consecutive times -- x 8 radii
rD = 0.02 ... 30.  At rD = 0.02 Re eta passes fast_eta_max inside the third J0 interval and at rD = 0.07 inside the last:
both are unproven intervals that follow proven ones, and the item is handed over to point_kernel from there; the large
radii stay on the cosh/sinh form.  Every call runs all 2M + 1 = 53 Laplace indices, index 0 (Im eta = 0 exactly) among them.
Every call must have run the folded one-depth kernel (ucf_plan_kernel_times).

Where the Gauss-Lobatto (wave, abscissa) pairs of these grids lie by the class of their interval, from the CPU restatement of
the classifier (tools/folded_loop_phase_shares.py intervals: binary64, the oracle's J0 zeros and de Hoog p-values; 4 waves x
8 radii x 53 Laplace indices = 1 696 items of 10 intervals of 48 nodes, 814 080 pairs per call):

    depth        cosh/sinh: table / short    exponential: table / short    unproven (the loop with the bits)
    zD = 1           18.7 % /  9.1 %              0.0 % / 57.8 %                 14.4 %
    zD = 0.9106      18.7 % /  9.1 %             31.3 % / 26.5 %                 14.4 %
    zD = 0.4         18.7 % /  9.1 %             35.5 % / 22.3 %                 14.4 %
    zD = 0           18.7 % /  9.1 %             37.0 % / 20.8 %                 14.4 %

(beta does not enter eta.)  Along an item, share of the 1 696 items: an unproven interval that straddles maxexp between a
cosh/sinh and an exponential one 16.4 %; table -> short at an interval boundary on the cosh/sinh form 4.9 %, on the
exponential form 4.5 % at zD = 0.9106 (6.0 % at 0.4, 7.0 % at 0, none at 1, where the exponential form's argument is 0 and
every such interval is short); an unproven last interval after proven ones 25.0 % (the two small radii)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "folded_loop_intervals_parent.npz")
# FAMILY 2, lane = time, any wave budget, one plan, FOLD, no depth above the screen, NZC = 1
KERNEL = re.compile(r"integrate_kernel<2, 1, \d+, false, true, false, 1, (true|false), false>")
DECK = "c2_neuman74_fullpen"
ZBENCH = 0.9106
CALLS = (("z091", 0.0, ZBENCH, {}),            # tag, Malama beta, zD, cut
         ("z04", 0.0, 0.4, {}),
         ("z0", 0.0, 0.0, {}),
         ("z1", 0.0, 1.0, {}),
         ("beta_z091", 0.5, ZBENCH, {}),
         ("beta_z1", 0.5, 1.0, {}),
         ("beta_z0", 0.5, 0.0, {}),
         ("z091_parts", 0.0, ZBENCH, {"UCF_NSPLIT": "8"}),
         ("beta_z04_parts", 0.5, 0.4, {"UCF_NSPLIT": "8"}))
KNOBS = ("UCF_NSPLIT", "UCF_TAIL_LSPLIT", "UCF_TAIL_ITEMS", "UCF_PERSIST")
TD_CLUSTERS = (-2.0, 0.0, 2.0, 4.0)       # four waves of 64 times, half a decade each, from 10^c
NT = 64 * len(TD_CLUSTERS)
RD = (0.02, 0.07, 0.2, 0.6, 1.5, 4.0, 10.0, 30.0)

_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
import test_gpu_folded_loop_intervals as T
dk, ts, P = load_deck(sys.argv[2])
dk.beta = float(sys.argv[5])
P = params_from_deck(dk)
pl = engine.Plan(P, mode="fast")
pl.set_timing(True)
zD = np.array([float(sys.argv[3])])
tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in T.TD_CLUSTERS])
rD = np.array(T.RD)
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


def test_folded_one_depth_kernel_interval_loops_keep_every_bit(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    got = run_calls(tmp_path)
    assert set(got) == {c[0] for c in CALLS}
    for tag, (h, dh, kernels, _) in got.items():
        assert any(KERNEL.search(k) for k in kernels), (tag, kernels)
        for name, a in (("h", h), ("dh", dh)):
            ref = want[f"{tag}_{name}"]
            assert a.shape == ref.shape == (NT, len(RD), 1) and a.dtype == ref.dtype == np.float64
            diff = np.flatnonzero(a.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
            print(f"{tag} {name}: {diff.size} of {a.size} values differ in a bit")
            assert diff.size == 0, (tag, name, diff.size, diff[:8], a.ravel()[diff[:8]], ref.ravel()[diff[:8]])
    # (the fixture itself: cutting the items did not change a bit in the parent build either)
    assert np.array_equal(want["z091_h"].view(np.uint64), want["z091_parts_h"].view(np.uint64))
