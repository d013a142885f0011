"""The folded water-table kernel with one depth per launch: quadrature units settled by bounds, bit for bit against the parent.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (the lane = time grid of a fully penetrating well: what
bench.py times) decides for every quadrature unit which loop it may run.  Three things changed around its loops (the ZPAIR
branch of integrate_kernel, zpair_unit_bounds in ucf_fastpath.h), none of them a floating-point operation that reaches a result:
  * the ends of the J0 intervals are read from a table that abscissa_kernel writes behind the abscissa rows (the same
    correctly rounded quotients the kernel formed for itself);
  * a unit is first tried with bounds on eta that need no eta (zpair_unit_bounds); only a unit they leave open pays for the
    two evaluations of the exact classifier, and a part that is in range to its end needs no test at all after its first
    unit proven exponential and short;
  * the tanh-sinh part is classified in runs of nodes like the J0 intervals, and a proven run takes a loop without tests.
h and dh must be the SAME BITS as before.  tests/golden/folded_loop_units_parent.npz holds what the parent build (commit and
build id inside the file) gave on an MI355X for the calls below; tools/gen_folded_loop_units_fixture.py wrote it.

Calls (CALLS): as tests/test_gpu_folded_loop_intervals.py has them -- the C2 deck (beta = 0) at the bench's depth
zD = 0.9106, at 0.4, 0 and 1, Malama's beta = 0.5 at zD = 0.9106, 1 and 0, and zD = 0.9106 and (beta = 0.5) zD = 0.4 once more
with every work item cut into 8 parts (a part starts at an interval boundary with cleared bits and its own table index) --
each 256 times x 8 radii rD = 0.02 ... 30, all 53 Laplace indices.  The times are four waves of 64, half a decade each, from
tD = 10^-4, 10^-1, 10 and 10^6.  What the tanh-sinh runs of these waves are (CPU model, tools/folded_loop_phase_shares.py):
  * tD from 10^-4: the low Laplace indices are on the exponential form from the first node, sin/cos from the table, decided
    by the bounds; from index 22 on Re eta is past fast_eta_max at the first node and point_kernel takes the whole item; at
    rD = 0.02 index 21 passes it at node 34 -- a hand-over from inside the second tanh-sinh run, at the abscissa itself -- and
    the indices below it in the first, second or later J0 intervals;
  * tD from 10^-1: runs the bounds leave open and the exact classifier proves (exponential, table), and runs that straddle
    maxexp and keep the loop with the tests;
  * tD from 10: cosh/sinh with the table at rD >= 0.6, exponential at the two small radii, a straddling run at rD = 0.2;
  * tD from 10^6: cosh/sinh short, decided by the bounds or, where they leave it open, by the exact classifier.
The two smallest radii pass fast_eta_max inside a late J0 interval: an unproven interval after proven ones, and after units
that needed no test at all.  Every call must have run the folded one-depth kernel (ucf_plan_kernel_times).
(43 of the 64 times of the first wave -- the earliest -- give NaN at every radius, in the parent build as now: the
reference's own overflow at such times, which point_kernel reproduces.  They are held to their bits like every other value,
and the 21 finite times of that wave went through the same wave-uniform branches.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "folded_loop_units_parent.npz")
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
TD_CLUSTERS = (-4.0, -1.0, 1.0, 6.0)      # four waves of 64 times, half a decade each, from 10^c
NT = 64 * len(TD_CLUSTERS)
RD = (0.02, 0.07, 0.2, 0.6, 1.5, 4.0, 10.0, 30.0)

# every call of CALLS in ONE child process (the cut is read once per process: a call with a cut gets a process of its own)
_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
import test_gpu_folded_loop_units as T
tags = sys.argv[3].split(",")
out = {"build_id": np.array(engine.build_id())}
tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in T.TD_CLUSTERS])
rD = np.array(T.RD)
for tag, beta, zD0, _ in T.CALLS:
    if tag not in tags:
        continue
    dk, ts, P = load_deck(T.DECK)
    dk.beta = beta
    P = params_from_deck(dk)
    pl = engine.Plan(P, mode="fast")
    pl.set_timing(True)
    zD = np.array([zD0])
    h, dh = pl.drawdown_grid(tD, pl.split_vector(tD), rD, zD, pl.zlay(zD))
    out[tag + "_kernels"] = np.array([k[0] for k in pl.kernel_times()])
    pl.close()
    out[tag + "_h"], out[tag + "_dh"] = h, dh
np.savez(sys.argv[2], **out)
"""


def run_calls(outdir):
    """{tag: (h, dh, kernel names, build id)}: the calls of CALLS, one child process per cut"""
    res = {}
    cuts = []
    for c in CALLS:
        if c[3] not in cuts:
            cuts.append(c[3])
    for i, env in enumerate(cuts):
        tags = [c[0] for c in CALLS if c[3] == env]
        out = os.path.join(str(outdir), f"cut{i}.npz")
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env)
        subprocess.run([sys.executable, "-c", _CALL_SCRIPT, ROOT, out, ",".join(tags)], check=True, env=e, timeout=600)
        with np.load(out) as d:
            for tag in tags:
                res[tag] = (d[tag + "_h"], d[tag + "_dh"], [str(k) for k in d[tag + "_kernels"]], str(d["build_id"]))
    return res


def test_folded_one_depth_kernel_units_settled_by_bounds_keep_every_bit(tmp_path):
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
