"""Every loop class of the folded one-depth water-table kernel, held to the oracle away from the C2 deck's kappa.

integrate_kernel<2, 1, W, false, FOLD = true, false, NZC = 1, ...> (what bench.py times) picks, per wave and quadrature unit, one
of seven loops (UCF_IV_UNPROVEN, CS_TAB, CS_SHORT, EX_TAB, EX_SHORT and the two _SH twins) from limits that are functions of
kappa, of the depth and of the Laplace parameters.  The parent-fixture tests (tests/test_gpu_folded_loop_*.py) hold its bits at
kappa = 0.4 only.  Here the configurations of tests/folded_configs.py (kappa 0.03, 0.4, 4; zD 0 ... 1; Malama's beta and
Moench's boundary; other numerics) run on one grid of 256 times x 5 radii, one depth; tests/test_midstages_folded.py shows
without a GPU which loops the picks' waves run.  Per configuration, fast flavour:

  * stages: tmp, glarea and totlap of every pick of tests/golden/midstages_folded_<tag>.npz under the rule of
    tests/test_gpu_stages_families.py (_judge, with its K, F, spread and refq: no bar of this file's own), from the launch that
    ran the folded one-depth kernel (ucf_plan_kernel_times) and whose h, dh are those of drawdown_grid bit for bit;
  * the same bits however the items are cut: h and dh of child processes with UCF_NSPLIT unset, 1 and 8 (read once per process;
    ucf_env.h declares it bit-neutral) are identical, NaNs included.  Parts clear the UCF_PH_* bits, so the same nodes run in a
    proven or _SH loop in one run and in a plain loop in another: the dropped clamp, range tests and series test reach no result;
  * end to end on all 1280 points against the binary64 oracle: the same NaN pattern (but for the allowance of the overflow
    regime that tools/fuzz_flavours.py documents: nan_patterns_agree), and at the picks h under gate (1) of
    tests/test_gpu_parity.py (gate1_bounds) against binary128.

What this file does NOT see: a limit that is wrong by a factor but lands on another VALID form.  UCF_ZB_SH without its kappa
(tried once in a scratch build) passes every case here: at kappa = 4 the difference form of sinh then runs from Re eta zD =
0.175 on, where it is good to 6e-16 -- far below K F -- and the wrong limit is applied alike however the items are cut.  That is
caught on the CPU: tests/test_folded_loop_classifiers_configs.py proves the limits sound node by node at every configuration
and takes them from the kernel's own zpair_bound_limit, bit for bit.

The faithful flavour has no classifier and runs once per kappa as the control: if it fails too, the fixture or the decoding is
wrong, not the loops.  The share of the rule every configuration / flavour / stage used goes to stages_folded.json in the log
folder of the tools (tools_out/ or $UCF_TOOLS_OUT; tools/collect_profiles.py copies it to profiles/)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import folded_configs as FC
import test_gpu_stages as base
import test_midstages_folded as fixtures
from golden_util import rel_err
from test_gpu_folded_loop_drops import KERNEL, KNOBS
from test_gpu_parity import gate1_bounds
from test_gpu_stages_families import ARBITRATION, F, K, STAGES, _judge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CONTROLS = ("k003_z04", "k04_z04", "k4_z04")              # faithful: one configuration per kappa
CASES = [(t, "fast") for t in FC.TAGS] + [(t, "faithful") for t in CONTROLS]
CUTS = (None, "1", "8")                                  # UCF_NSPLIT
REPORT = {}
_ORACLE = {}
_BUILD = {}


@pytest.fixture(scope="module")
def engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine as e
    _BUILD["id"] = e.build_id()
    return e


def _grid(plan, tag):
    tD, rD = FC.times(), FC.radii()
    zD = np.array([FC.config(tag)[2]])
    return tD, plan.split_vector(tD), rD, zD, plan.zlay(zD)


@pytest.mark.parametrize("tag,mode", CASES)
def test_stages_at_the_picks(engine, oracle, monkeypatch, tag, mode):
    monkeypatch.setattr(base, "REPORT", {})              # _check_point keeps ITS report for ITS decks
    z = fixtures.load(tag)
    dk, P, _ = FC.deck_of(tag)
    j0z = oracle.j0_zeros(oracle.nondim(P).nj0z)
    plan = engine.Plan(P, mode=mode)
    tD, sv, rD, zD, zl = _grid(plan, tag)
    assert np.array_equal(z["times"], tD) and np.array_equal(z["radii"], rD)
    picks = [(int(it), int(ir)) for it, ir in z["picks"]]
    args = [j0z[sv[it] - 1] / rD[ir] for it, ir in picks]
    plan.set_timing(True)
    st = plan.debug_stages(tD, sv, rD, zD, zl, grid=True)
    kernels = [n for n, ms, cnt in plan.kernel_times()]
    hg, dg = plan.drawdown_grid(tD, sv, rD, zD, zl)
    kernels_grid = [n for n, ms, cnt in plan.kernel_times()]
    plan.set_timing(False)
    plan.close()
    rep = REPORT.setdefault(tag, {}).setdefault(mode, {"kernels": kernels})
    assert st["layout"] == 1 and st["has_state"]
    if mode == "fast":
        assert any(KERNEL.search(k) for k in kernels), (tag, kernels)
        assert any(KERNEL.search(k) for k in kernels_grid), (tag, kernels_grid)
    else:
        assert any("integrate_generic_kernel<2, 1" in k for k in kernels), (tag, kernels)
    assert hg.shape == (len(tD), len(rD), 1)
    assert st["h"].reshape(hg.shape).tobytes() == hg.tobytes() and st["dh"].reshape(dg.shape).tobytes() == dg.tobytes()
    failures = []
    _judge(tag, mode, 1, z, st, [(k, it * len(rD) + ir) for k, (it, ir) in enumerate(picks)], args, rep, failures)
    judged = rep["L1"]["stages"]
    assert set(judged) == set(STAGES) and all(not judged[s]["not_judged"] and judged[s]["rule_pick"] >= 0 for s in STAGES)
    assert not failures, failures


# every configuration in ONE child process per cut (the cut is read once per process)
_CALL_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import folded_configs as FC
from unconfined_amd import engine
out = {}
for tag in FC.TAGS:
    dk, P, z0 = FC.deck_of(tag)
    pl = engine.Plan(P, mode="fast")
    pl.set_timing(True)
    tD, zD = FC.times(), np.array([z0])
    h, dh = pl.drawdown_grid(tD, pl.split_vector(tD), FC.radii(), zD, pl.zlay(zD))
    out[tag + "_kernels"] = np.array([k[0] for k in pl.kernel_times()])
    pl.close()
    out[tag + "_h"], out[tag + "_dh"] = h, dh
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def cut_runs(engine, tmp_path_factory):
    """{cut: npz} of the fast flavour's h, dh at every configuration"""
    outdir = tmp_path_factory.mktemp("folded_cuts")
    res = {}
    for cut in CUTS:
        out = os.path.join(str(outdir), f"nsplit_{cut}.npz")
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        if cut is not None:
            e["UCF_NSPLIT"] = cut
        subprocess.run([sys.executable, "-c", _CALL_SCRIPT, ROOT, out], check=True, env=e, timeout=600)
        res[cut] = dict(np.load(out))
    return res


@pytest.mark.parametrize("tag", FC.TAGS)
def test_same_bits_however_the_items_are_cut(cut_runs, tag):
    whole = cut_runs[None]
    for cut in CUTS:
        kernels = [str(k) for k in cut_runs[cut][tag + "_kernels"]]
        assert any(KERNEL.search(k) for k in kernels), (tag, cut, kernels)
        for name in ("h", "dh"):
            a, ref = cut_runs[cut][f"{tag}_{name}"], whole[f"{tag}_{name}"]
            assert a.shape == ref.shape == (256, len(FC.RD), 1) and a.dtype == ref.dtype == np.float64
            diff = np.flatnonzero(a.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
            print(f"{tag} UCF_NSPLIT={cut} {name}: {diff.size} of {a.size} values differ in a bit; {int(np.isfinite(a).sum())} finite")
            assert diff.size == 0, (tag, cut, name, diff.size, diff[:8], a.ravel()[diff[:8]], ref.ravel()[diff[:8]])


@pytest.mark.parametrize("tag,mode", CASES)
def test_end_to_end_against_the_oracle(engine, oracle, oracle_quad, cut_runs, tag, mode):
    from fuzz_flavours import nan_patterns_agree
    z = fixtures.load(tag)
    dk, P, _ = FC.deck_of(tag)
    D = oracle.nondim(P)
    plan = engine.Plan(P, mode=mode)
    tD, sv, rD, zD, zl = _grid(plan, tag)
    h, dh = plan.drawdown_grid(tD, sv, rD, zD, zl)
    plan.close()
    if mode == "fast":      # what the child processes gave is what this process gives
        assert h.tobytes() == cut_runs[None][tag + "_h"].tobytes() and dh.tobytes() == cut_runs[None][tag + "_dh"].tobytes()
    nt, nr = len(tD), len(rD)
    if tag not in _ORACLE:      # (computed once per configuration, shared by the flavours, never changed)
        ho, dho = oracle.batch(P, np.repeat(tD, nr), np.tile(rD, nt), np.repeat(sv, nr), zD, zl)
        hq, dhq = oracle_quad.batch(P, tD[z["picks"][:, 0]], rD[z["picks"][:, 1]], sv[z["picks"][:, 0]], zD, zl, threads=8)
        _ORACLE[tag] = (ho.reshape(h.shape), dho.reshape(dh.shape), hq)
    ho, dho, hq = _ORACLE[tag]
    for name, got, ref in (("h", h, ho), ("dh", dh, dho)):
        ndiff = int(np.sum(np.isnan(got) != np.isnan(ref)))
        print(f"{tag} {mode} {name}: {int(np.isnan(ref).sum())} NaN in the oracle's {ref.size} values, pattern differs at {ndiff}")
        assert nan_patterns_agree(ndiff, got.size, float(dk.kappa)), (tag, mode, name, ndiff)
    # gate (1) of tests/test_gpu_parity.py at the picks: as close to binary128 as the binary64 oracle is
    it, ir = z["picks"][:, 0], z["picks"][:, 1]
    floor = 1e-3 / (1.0 if dk.dimless else D.Hc)
    eg, er = rel_err(h[it, ir, :], hq, floor), rel_err(ho[it, ir, :], hq, floor)
    bound_max, bound_med = gate1_bounds(mode, False, er)
    rep = REPORT.setdefault(tag, {}).setdefault(mode, {})
    rep["gate1_h"] = {"max": float(eg.max() / bound_max), "median": float(np.median(eg) / bound_med), "err": float(eg.max()), "ref_err": float(er.max())}
    print(f"{tag} {mode} h at the picks: err {eg.max():.2e} (oracle {er.max():.2e}), median {np.median(eg):.2e} (oracle {np.median(er):.2e})")
    assert eg.max() <= bound_max, (tag, mode, float(eg.max()), float(er.max()))
    assert np.median(eg) <= bound_med, (tag, mode, float(np.median(eg)), float(np.median(er)))


def test_zz_every_configuration_ran_and_report():
    """(last in this file) the shares of the rule go next to the parity report"""
    if not REPORT:
        pytest.skip("no stage test ran")
    out = os.path.join(ROOT, os.environ.get("UCF_TOOLS_OUT", "tools_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "stages_folded.json"), "w") as f:
        json.dump({"what": "tests/test_gpu_stages_folded.py: per configuration of tests/folded_configs.py / flavour / stage the worst share of the "
                           "rule of tests/test_gpu_stages_families.py over the picks of tests/golden/midstages_folded_<tag>.npz (1.0 = "
                           "exhausted): vs_oracle = e_ref / (K max(F, spread)), vs_binary128 = e_q / (K max(F, refq)), rule = the smaller of the "
                           "two; gate1_h: the share of gate (1) of tests/test_gpu_parity.py that h at the picks used",
                   "K": K, "F": F, "arbitration": ARBITRATION, "build_id": _BUILD.get("id"),
                   "configurations": {t: {"overrides": c[1], "zD": c[2]} for t, c in ((c[0], c) for c in FC.CONFIGS)},
                   "shares": REPORT}, f, indent=1, sort_keys=True)
    ran = {(t, m) for t, by_mode in REPORT.items() for m, rep in by_mode.items() if "L1" in rep}
    if len(ran) == len(CASES):
        assert all(any(KERNEL.search(k) for k in REPORT[t]["fast"]["kernels"]) for t in FC.TAGS)
