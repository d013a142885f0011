"""The stage fixtures of the folded one-depth water-table kernel (tests/golden/midstages_folded_<tag>.npz,
oracle/gen_midstages_folded.py; one per configuration of tests/folded_configs.py), looked at WITHOUT a GPU.

The conditions the generator asserts before it writes a file are asserted again from the files (gen.check): six picks or
more, each within the information caps of tests/test_midstages_families.py (its constants, imported), each arbitrated by
binary128 under that file's rule, none excluded from judgement; the recorded loops of every pick's wave are what the CPU model
of the classifiers (tools/folded_loop_phase_shares.py) gives today, for items whole and cut into eight parts; and the waves of
the picks together reach every loop of the kernel that the configuration can reach -- seven, six at zD = 1 (no exponential
unit keeps the table sin/cos there), five at zD = 0 (no UCF_PH_SH), four at kappa = 0.03 and zD = 1 on this grid
(gen.GRID_NEVER) -- and, where zD > 0, a unit decided by the bounds, a unit left to the exact classifier, a tanh-sinh run that
sets UCF_PH_SH and a part of eight whose first unit sets it.  The oracle built here still gives the files' bits."""
import os
import sys

import numpy as np
import pytest

import folded_configs as FC
import test_midstages_families as rule
from test_midstages_families import STAGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_midstages_folded as gen  # noqa: E402


def load(tag):
    return np.load(gen.path_of(tag))


def test_there_is_one_file_per_configuration_and_no_other():
    on_disk = sorted(f[len("midstages_folded_"):-4] for f in os.listdir(os.path.dirname(gen.path_of("x"))) if f.startswith("midstages_folded_"))
    assert on_disk == sorted(FC.TAGS)
    kappas = {c[1]["kappa"] for c in FC.CONFIGS}
    assert kappas == {0.03, 0.4, 4.0}
    assert {(c[1]["kappa"], c[2]) for c in FC.CONFIGS if set(c[1]) == {"kappa"}} == {(k, z) for k in kappas for z in (0.4, 1.0)}
    assert any(c[2] == 0.0 for c in FC.CONFIGS)
    assert {c[1]["kappa"] for c in FC.CONFIGS if c[1].get("model") == 4 and c[1].get("beta") == 2.0} == {0.03, 4.0}


@pytest.mark.parametrize("tag", FC.TAGS)
def test_file_meets_the_generators_conditions(tag):
    z = load(tag)
    zD = FC.config(tag)[2]
    npk = len(z["picks"])
    want = {"picks", "radii", "times", "refq", "spread", "loops"} | {f"{k}_{s}{q}" for k in range(npk) for s in STAGES for q in ("", "_q")}
    assert set(z.files) == want, tag
    assert os.path.getsize(gen.path_of(tag)) < gen.MAX_BYTES
    got = gen.check(rule, tag, z)
    loops = {l for l in got if l in FC.LOOPS}
    print(tag, "picks", [tuple(p) for p in z["picks"]], "reach", sorted(got))
    assert loops == set(FC.reachable_loops(zD)) - set(gen.GRID_NEVER.get(tag, ())), (tag, sorted(loops))
    if zD > 0.0:
        assert set(gen.FLAGS) <= got, (tag, sorted(got))
        assert {"cs_tab_sh", "cs_short_sh"} <= loops
    else:
        assert not any(l.endswith("_sh") for l in loops)
    # readable from the file alone: the codes of `loops` name them
    in_file = {FC.LOOPS[i] for i in np.unique(z["loops"])}
    assert in_file == loops, (tag, sorted(in_file))
    # the rule of tests/test_midstages_families.py sees every pick as judged and arbitrated
    assert all(rule.excluded(tag, s) == [] and rule.arbitrated(z, tag, k, s) for k in range(npk) for s in STAGES)
    assert all(rule.noise(z, k, s) <= rule.CAPS[s] and rule.refq(z, k, s) <= rule.ARBITRATION * rule.noise(z, k, s)
               for k in range(npk) for s in STAGES)


def test_only_the_listed_configurations_miss_a_loop_their_depth_could_reach():
    assert set(gen.GRID_NEVER) == {"k003_z1"}
    S = gen.model("k003_z1")
    # the reason: the lowest J0 interval of the grid starts past the abscissa from which Re eta zD >= 0.35 whatever p is
    assert S.j0z[0] / max(FC.RD) > S.SINH_SERIES * np.sqrt(S.kappa) / 1.0 * (1.0 + 2.0 ** -19)
    for tag in FC.TAGS:
        if tag not in gen.GRID_NEVER and FC.config(tag)[2] > 0.0:
            S, zD = gen.model(tag), FC.config(tag)[2]
            assert S.j0z[int(S.P.j0s[0]) - 1] / max(FC.RD) < S.SINH_SERIES * np.sqrt(S.kappa) / zD, tag


def test_the_oracle_built_here_gives_the_files_bits(oracle, oracle_quad):
    """the first pick of every configuration in binary64 (vectors bit for bit, spread the same number), one in binary128"""
    for tag in FC.TAGS:
        z = load(tag)
        dk, ctx = gen.context(oracle, tag)
        it, ir = z["picks"][0]
        st, sq, rq, spread = gen.one_pick(oracle, oracle_quad if tag == FC.TAGS[0] else None, ctx, int(it), int(ir))
        for s in STAGES:
            assert st[s].tobytes() == z[f"0_{s}"].tobytes(), (tag, s)
            if sq is not None:
                assert sq[s].tobytes() == z[f"0_{s}_q"].tobytes(), (tag, s)
        assert np.array_equal(spread, z["spread"][0]), tag
        if rq is not None:
            assert np.array_equal(rq, z["refq"][0])
