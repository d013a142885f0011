"""Every evaluator family between "sample" and "h, dh", held to the reference's own rounding noise.

tests/test_gpu_stages.py reads the level sums tmp, the Gauss-Lobatto areas glarea and the accelerated transform totlap out of
the production launch sequence (ucf_debug_stages) for five decks of families 2 and 4, with absolute bars of 2e-13 ... 1e-10.
This file does the same for 18 decks of all six families (family_of: 0 Theis, 1 Hantush, 5 Hantush with wellbore storage,
2 water table, 3 Mishra-Neuman in Malama's form, 4 Mishra-Neuman by finite differences), both flavours, the three lane
layouts, against tests/golden/midstages_fam_<deck>.npz (oracle/gen_midstages_families.py) -- and with NO absolute bar.

The rule, per pick, stage and layout (constants in tests/test_midstages_families.py, which checks the fixtures without a GPU):
e_ref = device against the binary64 oracle, e_q = device against binary128, both in the measure of _vec_err; F = 1e-15;
spread = what one ulp in tD or rD changes in the oracle's own vector; refq = the oracle's distance from binary128;
K = 8 / 16 (faithful / fast) for tmp and glarea, 16 / 32 for totlap.  A pick passes if

    e_ref <= K max(F, spread)        the device is another binary64 realisation of the same algorithm: it may differ from
                                     the oracle by what one ulp in an input already changes, times K; or
    e_q <= K max(F, refq)            (only where refq <= 4 max(F, spread), i.e. binary64 and binary128 ran the same path) the
                                     device is as close to exact arithmetic as the reference is.  This admits the
                                     cancellation-free forms of the fast flavour, which are more accurate than the oracle.

Nothing here is fitted to what the device gives: K is the factor test_gpu_stages.BARS already grants, F its floor, spread
and refq come from the reference alone.  The report (stages_families.json in the log folder of the tools, tools_out/ or
$UCF_TOOLS_OUT; tools/collect_profiles.py copies it to profiles/) gives the share of the rule each deck / flavour / layout /
stage used; 1.0 = exhausted."""
import json
import os
import re

import numpy as np
import pytest

import test_gpu_stages as base
import test_midstages_families as rule
from test_gpu_stages import _check_point, _cplx, _vec_err  # noqa: F401  (the measure and the decoding of `state`)
from test_midstages_families import ARBITRATION, DECKS, F, K, STAGES  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["faithful", "fast"]
REPORT = {}
NO_BARS = {s: (float("inf"), 0.0) for s in STAGES}       # _check_point decodes and measures; the rule is applied here
TRANSFORM = re.compile(r"(integrate_kernel|integrate_generic_kernel|point_kernel)<(\d+), (\d+)")


@pytest.fixture(scope="module")
def engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine as e
    return e


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    return rule.families_of(str(tmp_path_factory.mktemp("family_of")), DECKS)


class _View:
    """a deck's file under the key names _check_point reads (<deck>_<pick>_<stage>)"""

    def __init__(self, name, z):
        self.prefix, self.z = name + "_", z

    def __getitem__(self, key):
        assert key.startswith(self.prefix)
        return self.z[key[len(self.prefix):]]


def _judge(name, mode, layout, z, st, points, args, rep, failures):
    """the rule on the picks `points` = [(pick number, point index in st)] of one call"""
    view = _View(name, z)
    ent = rep.setdefault(f"L{layout}", {"has_state": bool(st["has_state"]), "stages": {}})
    for k, q in points:
        out = _check_point(name, mode, layout, k, st, q, args[k], view, NO_BARS)
        for s, (e_ref, e_q, ref_q) in out.items():
            n, rq = rule.noise(z, k, s), max(F, rule.refq(z, k, s))
            assert ref_q == rule.refq(z, k, s)
            kk = K[mode][s]
            arb = rule.arbitrated(z, name, k, s)
            judged = k not in rule.excluded(name, s)
            share_ref, share_q = e_ref / (kk * n), e_q / (kk * rq)
            share = min(share_ref, share_q) if arb else share_ref
            print(f"{name} {mode} L{layout} pick {k} {s}: e_ref {e_ref:.2e} e_q {e_q:.2e} spread {n:.2e} refq {rq:.2e} "
                  f"share {share:.3f}{'' if arb else ' (not arbitrated)'}{'' if judged else ' (not judged)'}")
            r = ent["stages"].setdefault(s, {"vs_oracle": 0.0, "vs_oracle_pick": -1, "vs_binary128": 0.0, "vs_binary128_pick": -1,
                                             "rule": 0.0, "rule_pick": -1, "not_judged": []})
            if not judged:
                r["not_judged"].append({"pick": k, "e_ref": e_ref, "e_q": e_q})
                continue
            if not share_ref <= r["vs_oracle"]:
                r["vs_oracle"], r["vs_oracle_pick"] = share_ref, k
            if arb and not share_q <= r["vs_binary128"]:
                r["vs_binary128"], r["vs_binary128_pick"] = share_q, k
            if not share <= r["rule"]:
                r["rule"], r["rule_pick"] = share, k
            if not share <= 1.0:
                failures.append((name, mode, f"L{layout}", k, s, dict(e_ref=e_ref, e_q=e_q, spread=n, refq=rq, K=kk, arbitrated=arb)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", DECKS)
def test_stages_of_every_family(engine, oracle, families, monkeypatch, name, mode):
    """the 128 x 2 grid (LAYOUT 1), the 256-point list in order of radius (LAYOUT 3, or 0 where the launch keeps no state)
    and the picks alone (LAYOUT 0)"""
    monkeypatch.setattr(base, "REPORT", {})              # _check_point keeps ITS report for ITS decks
    z = rule.load(name)
    dk, (P, D, j0z, tD, sv, rD, zD, zl) = rule.gen.context(oracle, name)
    picks = [(int(it), int(ir)) for it, ir in z["picks"]]
    args = [j0z[sv[it] - 1] / rD[ir] for it, ir in picks]
    fam = families[name]
    rep = REPORT.setdefault(name, {}).setdefault(mode, {"family": fam})
    failures = []
    plan = engine.Plan(P, mode=mode)
    nt, nr = len(tD), len(rD)

    # LAYOUT 1: the grid entry, and the instantiation that ran
    plan.set_timing(True)
    st = plan.debug_stages(tD, sv, rD, zD, zl, grid=True)
    hg, dg = plan.drawdown_grid(tD, sv, rD, zD, zl)
    rep["kernels"] = [n for n, ms, cnt in plan.kernel_times()]
    plan.set_timing(False)
    assert st["layout"] == 1
    assert np.array_equal(st["h"].reshape(hg.shape), hg, equal_nan=True) and np.array_equal(st["dh"].reshape(dg.shape), dg, equal_nan=True)
    found = [TRANSFORM.search(n) for n in rep["kernels"]]
    found = [m for m in found if m]
    assert found, rep["kernels"]
    kind, kfam, klay = found[0].group(1), int(found[0].group(2)), int(found[0].group(3))
    rep["transform_kernel"] = [n for n in rep["kernels"] if TRANSFORM.search(n)][0]
    assert (kfam, klay) == (fam, 1), rep["kernels"]
    if mode == "fast":
        # every family has its fast evaluators in integrate_kernel, and that launch keeps its state
        assert kind == "integrate_kernel" and st["has_state"], rep["kernels"]
    else:
        # the reference-order evaluators: integrate_generic_kernel, or inside point_kernel (no state) where the Thomas buffer of
        # the finite differences is too large for the split (split_kind, ucf_launch_plan.h)
        assert kind == ("integrate_generic_kernel" if st["has_state"] else "point_kernel"), rep["kernels"]
        assert st["has_state"] or fam == 4
    _judge(name, mode, 1, z, st, [(k, it * nr + ir) for k, (it, ir) in enumerate(picks)], args, rep, failures)

    # LAYOUT 3: a list of 256 points, ordered by radius (point = ir * nt + it)
    tl = np.tile(tD, nr); rl = np.repeat(rD, nt); sl = np.tile(sv, nr)
    st = plan.debug_stages(tl, sl, rl, zD, zl, grid=False)
    assert st["layout"] == (3 if st["has_state"] else 0)
    _judge(name, mode, st["layout"] if st["has_state"] else "0_list", z, st, [(k, ir * nt + it) for k, (it, ir) in enumerate(picks)], args, rep, failures)

    # LAYOUT 0: the picks on their own
    order = sorted(range(len(picks)), key=lambda i: rD[picks[i][1]])
    t5 = np.array([tD[picks[i][0]] for i in order]); r5 = np.array([rD[picks[i][1]] for i in order])
    s5 = np.array([sv[picks[i][0]] for i in order], np.int32)
    st0 = plan.debug_stages(t5, s5, r5, zD, zl, grid=False)
    assert st0["layout"] == 0
    _judge(name, mode, 0, z, st0, [(i, q) for q, i in enumerate(order)], args, rep, failures)
    assert not failures, failures


def test_zz_all_six_families_ran_in_both_flavours_and_report(families):
    """(last in this file) over all decks the fast flavour ran integrate_kernel of all six families, the faithful flavour its
    reference-order kernel of all six; the shares of the rule go next to the parity report"""
    if not REPORT:
        pytest.skip("no stage test ran")
    ran = {m: {} for m in MODES}
    for name, by_mode in REPORT.items():
        for mode, rep in by_mode.items():
            if "transform_kernel" in rep:
                m = TRANSFORM.search(rep["transform_kernel"])
                ran[mode].setdefault(int(m.group(2)), set()).add(m.group(1))
    out = os.path.join(ROOT, os.environ.get("UCF_TOOLS_OUT", "tools_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "stages_families.json"), "w") as f:
        json.dump({"what": "per deck / flavour / lane layout / stage the worst share of the rule of tests/test_gpu_stages_families.py over the "
                           "picks (1.0 = exhausted): vs_oracle = e_ref / (K max(F, spread)), vs_binary128 = e_q / (K max(F, refq)) over the "
                           "arbitrated picks, rule = the smaller of the two that apply to a pick; has_state false: the launch keeps no "
                           "level sums or areas, only totlap is checked; L0_list: the 256-point list where it runs lane layout 0",
                   "K": K, "F": F, "arbitration": ARBITRATION,
                   "kernels_that_ran": {m: {str(f): sorted(v) for f, v in sorted(ran[m].items())} for m in MODES},
                   "decks": REPORT}, f, indent=1, sort_keys=True)
    if set(REPORT) == set(DECKS) and all(set(v) == set(MODES) for v in REPORT.values()):
        assert {f for f, kinds in ran["fast"].items() if "integrate_kernel" in kinds} == {0, 1, 2, 3, 4, 5}, ran
        assert {f for f, kinds in ran["faithful"].items() if kinds & {"integrate_generic_kernel", "point_kernel"}} == {0, 1, 2, 3, 4, 5}, ran
        assert all("integrate_generic_kernel" in ran["faithful"][f] for f in (0, 1, 2, 3, 5)), ran
