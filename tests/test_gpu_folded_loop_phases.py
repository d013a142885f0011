"""The folded water-table kernel with one depth per launch: the phases of its abscissa loop, bit for bit against the parent.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (the lane = time grid of a fully penetrating well: what
bench.py times) carries what a wave has established for the rest of its part of a work item across the abscissae
(UCF_PH_*, ucf_fastpath.h): range tests that can only turn one way are not issued again, and a wave whose sin/cos arguments
have all fallen below UCF_SC_SMALL = 0.012 takes them from sincos_small_, which is sincos_tab_ at table entry 0 without the
table.  Not one floating-point operation that reaches a result moved: h and dh must be the SAME BITS as before.
tests/golden/folded_loop_phases_parent.npz holds what the parent build (commit and build id inside the file) gave on an
MI355X for the calls below; tools/gen_folded_loop_phases_fixture.py wrote it.

Calls (CALLS): the C2 deck (beta = 0) at the bench's depth zD = 0.9106, at 0.6, 0 and 1, and the same deck with Malama's
beta = 0.5 at zD = 0.9106 and 0; zD = 0.9106 and (beta = 0.5) zD = 0.6 once more with every work item cut into 8 parts
(UCF_NSPLIT=8: every part starts from cleared flags in the middle of an item).  Each 256 times (lane = time needs 64) in
four groups of 64, half a decade each, from tD = 10^-2.5, 10^-0.5, 10^1.5 and 10^3.5 -- a wave is 64 consecutive times, and
only times close together (the bench has 114 per decade) let a whole wave reach the small-argument phase; the early groups
have large Im p and reach it late or never -- x 8 radii rD = 0.02 ... 30 (rD = 0.02 leaves the fast evaluators inside an
item: hand-over to point_kernel; the large radii stay on the cosh/sinh form).  Every call runs all 2M + 1 = 53 Laplace
indices, index 0 (Im eta = 0 exactly) among them.  Every call must have run the folded one-depth kernel
(ucf_plan_kernel_times).

Where the (wave, abscissa) pairs of these grids lie, from a binary64 CPU evaluation of eta (tools/folded_loop_phase_shares.py:
the oracle's J0 zeros, tanh-sinh and Gauss-Lobatto nodes and de Hoog p-values; 4 waves x 8 radii x 53 Laplace indices = 1 696
items of 543 abscissae, 920 928 pairs per call).  "short" = the wave is on sincos_small_ there: every lane's argument (cosh/sinh
form: Im eta; exponential form: Im eta (1 - zD)) was below 0.012 at an abscissa where the kernel may set the bit (any
tanh-sinh node, the last Gauss-Lobatto node of a J0 interval), and from then on:

    depth        cosh/sinh: table / short    both forms    exponential: table / short    beyond the fast range
    zD = 0.9106      18.0 % /  6.2 %            6.5 %           34.2 % / 21.9 %                13.3 %
    zD = 0.6         18.0 % /  6.2 %            6.5 %           37.5 % / 18.5 %                13.3 %
    zD = 0           18.0 % /  6.2 %            6.5 %           39.8 % / 16.2 %                13.3 %
    zD = 1           18.0 % /  6.2 %            6.5 %            2.3 % / 53.7 %                13.3 %

(beta does not enter eta.)  Transitions along an item, share of the 1 696 items at zD = 0.9106: cosh/sinh -> exponential
44.6 %, table -> short on the cosh/sinh form 23.4 %, on the exponential form 14.3 %; 2.4 % are on the short form from their
first abscissa (Laplace index 0 and the latest times; 26.9 % at zD = 1, where the exponential form's argument is 0)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "folded_loop_phases_parent.npz")
# FAMILY 2, lane = time, any wave budget, one plan, FOLD, no depth above the screen, NZC = 1
KERNEL = re.compile(r"integrate_kernel<2, 1, \d+, false, true, false, 1, (true|false), false>")
DECK = "c2_neuman74_fullpen"
ZBENCH = 0.9106
CALLS = (("z091", 0.0, ZBENCH, {}),            # tag, Malama beta, zD, cut
         ("z06", 0.0, 0.6, {}),
         ("z0", 0.0, 0.0, {}),
         ("z1", 0.0, 1.0, {}),
         ("beta_z091", 0.5, ZBENCH, {}),
         ("beta_z0", 0.5, 0.0, {}),
         ("z091_parts", 0.0, ZBENCH, {"UCF_NSPLIT": "8"}),
         ("beta_z06_parts", 0.5, 0.6, {"UCF_NSPLIT": "8"}))
KNOBS = ("UCF_NSPLIT", "UCF_TAIL_LSPLIT", "UCF_TAIL_ITEMS", "UCF_PERSIST")
TD_CLUSTERS = (-2.5, -0.5, 1.5, 3.5)      # four waves of 64 times, half a decade each, from 10^c
NT = 64 * len(TD_CLUSTERS)
RD = (0.02, 0.05, 0.11, 0.4, 1.5, 3.0, 9.0, 30.0)

_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
import test_gpu_folded_loop_phases as T
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


def test_folded_one_depth_kernel_phases_keep_every_bit(tmp_path):
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
