"""The folded water-table kernel with one depth per launch: what a proven class already rules out is not issued, bit for bit.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (the lane = time grid of a fully penetrating well: what
bench.py times).  Three things left its loops, none of them a floating-point operation that reaches a result:
  * the proven cosh/sinh loops do not clamp Re eta at maxexp (v_min_f64): every lane of such a unit is below it;
  * a proven cosh/sinh J0 interval of a part that has UCF_PH_SH ("Re eta zD >= 0.35 in every lane from here on": set by the
    units' classifiers from the lower end of a unit, by bounds or from eta there; ucf_fastpath.h) runs a loop whose sinh(eta)
    and sinh(eta zD) take the difference form without testing for the series;
  * the weights of the tanh-sinh level update come by scalar load.
h and dh must be the SAME BITS as before.  tests/golden/folded_loop_drops_parent.npz holds what the parent build (commit and
build id inside the file) gave on an MI355X for the calls below; tools/gen_folded_loop_drops_fixture.py wrote it.

Calls (CALLS): the C2 deck, 256 times (four waves of 64, half a decade each) x 8 radii, all 53 Laplace indices, every work
item cut into 8 parts unless said otherwise (a part starts at an interval boundary with cleared bits: the tanh-sinh nodes |
intervals 0-1 | 2 | 3 | 4-5 | 6 | 7-8 | 9).  What they exercise, from the CPU model (tools/folded_loop_phase_shares.py sh;
counts of parts, one part = one wave's share of one item; tests/test_folded_loop_sh_bound.py asserts that they occur):
  * z091_far, z1_far, z04_far, beta_z04_far (tD from 10^2, 10^4, 10^6, 10^8; rD = 3 ... 30: 95 % of the Gauss-Lobatto pairs are
    proven cosh/sinh, 91 / 92 / 75 / 75 % of those run with the bit): Re eta zD crosses 0.35 INSIDE a J0 interval, so that a
    later interval of the same part sets the bit and the part runs both loops (954 / 1113 / 636 parts); BETWEEN THE LANES of a
    wave at a unit's lower end (some past the limit, some not: the wave waits for the last; 327 / 326 / 773 units); AT A
    PART BOUNDARY (the first unit of a part sets it, the part before ended without it: 742 / 583 / 1060 parts); and NEVER in a
    part (2438 / 2226 / 4611 parts, among them the first two intervals at rD = 30 at the late times: a < 0.29 there and
    Re eta stays near a / sqrt(kappa));
  * z0_far (zD = 0): no part ever sets the bit, every cosh/sinh interval runs the plain loop;
  * beta_z091_wide, z04_wide (tD from 10^-4, 10^-1, 10, 10^6; rD = 0.02 ... 30: the grids of the older tests, 19 % of the
    pairs proven cosh/sinh): the bit beside exponential and unproven units, hand-overs to point_kernel and the NaN of the
    overflow regime at the earliest times;
  * z091_far_whole, beta_z1_wide_whole (items not cut): a TANH-SINH RUN sets the bit (265 / 491 items) for the intervals
    behind it; in every item of the first the bit is set inside the one part (1696 items).
Every call must have run the folded one-depth kernel (ucf_plan_kernel_times)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "folded_loop_drops_parent.npz")
# FAMILY 2, lane = time, any wave budget, one plan, FOLD, no depth above the screen, NZC = 1
KERNEL = re.compile(r"integrate_kernel<2, 1, \d+, false, true, false, 1, (true|false), false>")
DECK = "c2_neuman74_fullpen"
ZBENCH = 0.9106
CUT = {"UCF_NSPLIT": "8"}
RD_WIDE = (0.02, 0.07, 0.2, 0.6, 1.5, 4.0, 10.0, 30.0)
RD_FAR = (3.0, 5.0, 8.0, 12.0, 16.0, 20.0, 25.0, 30.0)
LATE = (2.0, 4.0, 6.0, 8.0)            # four waves of 64 times, half a decade each, from 10^c
WIDE = (-4.0, -1.0, 1.0, 6.0)
# tag, Malama beta, zD, cut, time clusters, radii
CALLS = (("z091_far", 0.0, ZBENCH, CUT, LATE, RD_FAR),
         ("z04_far", 0.0, 0.4, CUT, LATE, RD_FAR),
         ("z0_far", 0.0, 0.0, CUT, LATE, RD_FAR),
         ("z1_far", 0.0, 1.0, CUT, LATE, RD_FAR),
         ("beta_z04_far", 0.5, 0.4, CUT, LATE, RD_FAR),
         ("beta_z091_wide", 0.5, ZBENCH, CUT, WIDE, RD_WIDE),
         ("z04_wide", 0.0, 0.4, CUT, WIDE, RD_WIDE),
         ("z091_far_whole", 0.0, ZBENCH, {}, LATE, RD_FAR),
         ("beta_z1_wide_whole", 0.5, 1.0, {}, WIDE, RD_WIDE))
KNOBS = ("UCF_NSPLIT", "UCF_TAIL_LSPLIT", "UCF_TAIL_ITEMS", "UCF_PERSIST")
NT = 256

# every call of CALLS in ONE child process per cut (the cut is read once per process)
_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
import test_gpu_folded_loop_drops as T
tags = sys.argv[3].split(",")
out = {"build_id": np.array(engine.build_id())}
for tag, beta, zD0, _, clusters, radii in T.CALLS:
    if tag not in tags:
        continue
    tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in clusters])
    rD = np.array(radii)
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


def test_folded_one_depth_kernel_without_clamp_series_test_and_vector_weight_loads_keeps_every_bit(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    got = run_calls(tmp_path)
    assert set(got) == {c[0] for c in CALLS}
    for tag, (h, dh, kernels, _) in got.items():
        assert any(KERNEL.search(k) for k in kernels), (tag, kernels)
        nr = len(next(c for c in CALLS if c[0] == tag)[5])
        for name, a in (("h", h), ("dh", dh)):
            ref = want[f"{tag}_{name}"]
            assert a.shape == ref.shape == (NT, nr, 1) and a.dtype == ref.dtype == np.float64
            diff = np.flatnonzero(a.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
            print(f"{tag} {name}: {diff.size} of {a.size} values differ in a bit; {int(np.isfinite(a).sum())} finite")
            assert diff.size == 0, (tag, name, diff.size, diff[:8], a.ravel()[diff[:8]], ref.ravel()[diff[:8]])
    # (the fixture itself: cutting the items did not change a bit in the parent build either)
    assert np.array_equal(want["z091_far_h"].view(np.uint64), want["z091_far_whole_h"].view(np.uint64))
