"""The stage fixtures of every evaluator family (tests/golden/midstages_fam_<deck>.npz, oracle/gen_midstages_families.py),
looked at WITHOUT a GPU: do they carry information at the rounding level, is the binary128 value usable, do the decks reach
all six families, and does the oracle built here still give these bits.

Per deck the file holds six picks (time index, radius index) of the 128 x 2 grid of oracle/gen_midstages.py and per pick the
vectors tmp, glarea, totlap of the binary64 oracle, the same of its binary128 build (*_q) and, per stage, two scalars in the
measure of test_gpu_stages._vec_err (max norm over the Laplace samples, relative to the vector's largest modulus):

    refq      distance of the binary64 oracle from binary128
    spread    change of the binary64 oracle's own vector when tD or rD moves by one ulp (four draws)

tests/test_gpu_stages_families.py holds the device to K max(F, spread) against the oracle, or to K max(F, refq) against
binary128 where the pick is arbitrated; the rule and its constants live HERE so that they can be read without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLD, load_deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_midstages_families as gen  # noqa: E402

DECKS = gen.DECKS
STAGES = gen.STAGES
F = 1e-15                                   # the floor test_gpu_stages.py already puts under the oracle's own distance
CAPS = {"tmp": 1e-12, "glarea": 1e-12, "totlap": 1e-11}       # a pick carries information while max(F, spread) <= cap
ARBITRATION = 4.0                           # refq <= 4 n: binary64 and binary128 ran the same path, their distance is noise
# the factor that test_gpu_stages.BARS grants on the oracle's own distance from binary128
K = {"faithful": {"tmp": 8.0, "glarea": 8.0, "totlap": 16.0}, "fast": {"tmp": 16.0, "glarea": 16.0, "totlap": 32.0}}
FD_DECKS = ("c5_mishra_fd64", "mishra_fd30")

# picks above the caps, (deck, stage) -> pick numbers: none.  (The generator avoids the larger radius at early times, where
# h ~ 0 and the totlap spread is 1e-11 ... 3e-9 in every family, and takes time index 118 instead of 126 for c5.)
EXCLUDED = {}
# picks whose binary128 value took another branch of an in-band rule (the Wynn-epsilon truncation or the early exit) than the
# binary64 oracle, or whose four draws happen to lie closer together than binary128 is: refq > 4 max(F, spread).  They are
# judged against the oracle alone.  (deck, stage) -> {pick number: (refq, spread)} as the generator printed them
NOT_ARBITRATED = {
    ("hantush_fullpen", "totlap"): {1: (5.5e-13, 4.6e-15)},
    ("hantush_lay1", "totlap"): {0: (4.8e-09, 1.6e-15)},
    ("hstorage_partpen_lay1", "totlap"): {0: (5.8e-06, 3.0e-15)},
    ("hstorage_partpen_lay2", "totlap"): {0: (7.0e-07, 1.5e-14)},
    ("malama_k10", "totlap"): {2: (7.4e-15, 1.4e-15), 4: (1.1e-14, 2.6e-15)},
    ("mishra_malama", "totlap"): {4: (6.5e-15, 1.0e-15)},
}


def load(name):
    return np.load(gen.path_of(name))


def noise(z, k, stage):
    """n = max(F, spread) of pick k"""
    return max(F, float(z["spread"][k][STAGES.index(stage)]))


def refq(z, k, stage):
    return float(z["refq"][k][STAGES.index(stage)])


def excluded(name, stage):
    return sorted(EXCLUDED.get((name, stage), ()))


def arbitrated(z, name, k, stage):
    return k not in NOT_ARBITRATED.get((name, stage), {})


@pytest.fixture(scope="module")
def files():
    return {name: load(name) for name in DECKS}


def test_files_hold_what_the_generator_writes_and_nothing_else(files):
    cap = os.path.getsize(os.path.join(GOLD, "midstages.npz"))
    total = 0
    for name, z in files.items():
        npk = len(z["picks"])
        want = {"picks", "radii", "nt", "refq", "spread"} | {f"{k}_{s}{q}" for k in range(npk) for s in STAGES for q in ("", "_q")}
        assert set(z.files) == want, name
        assert z["refq"].shape == z["spread"].shape == (npk, 3)
        assert int(z["nt"][0]) == gen.NT and tuple(z["radii"]) == gen.RADII
        assert [tuple(p) for p in z["picks"]] == gen.DECK_PICKS.get(name, gen.PICKS)
        # the radii alternate, the times ascend and span the grid
        assert [int(p[1]) for p in z["picks"]] == [k % 2 for k in range(npk)]
        its = [int(p[0]) for p in z["picks"]]
        assert its == sorted(its) and its[0] < gen.NT // 8 and its[-1] >= gen.NT - gen.NT // 8
        for k in range(npk):
            for s in STAGES:
                assert z[f"{k}_{s}"].shape == z[f"{k}_{s}_q"].shape and np.isfinite(z[f"{k}_{s}"]).all() and np.isfinite(z[f"{k}_{s}_q"]).all()
                # the scalars are those of the vectors beside them
                assert refq(z, k, s) == gen.vec_err(gen.cplx(z[f"{k}_{s}"]), gen.cplx(z[f"{k}_{s}_q"])), (name, k, s)
        size = os.path.getsize(gen.path_of(name))
        assert size <= cap, (name, size)
        total += size
    assert total <= 2.5 * 2 ** 20, total
    on_disk = sorted(f[len("midstages_fam_"):-4] for f in os.listdir(GOLD) if f.startswith("midstages_fam_"))
    assert on_disk == sorted(DECKS)


def test_every_deck_carries_information_at_the_rounding_level(files):
    """2a: at least six picks per deck and stage whose own noise n = max(F, spread) is within the cap; the others by name"""
    for name, z in files.items():
        npk = len(z["picks"])
        for s in STAGES:
            above = [k for k in range(npk) if not noise(z, k, s) <= CAPS[s]]
            assert above == excluded(name, s), (name, s, above, [noise(z, k, s) for k in above])
            assert len(above) <= (3 if (s == "tmp" and name in FD_DECKS) else 2), (name, s)
            assert npk - len(above) >= 6, (name, s)
    assert all(name in DECKS and s in STAGES for name, s in EXCLUDED)


def test_picks_not_arbitrated_by_binary128_are_the_listed_ones(files):
    """2b: refq <= 4 n, or the pick is listed with its numbers"""
    found = {}
    for name, z in files.items():
        for s in STAGES:
            for k in range(len(z["picks"])):
                if not refq(z, k, s) <= ARBITRATION * noise(z, k, s):
                    found.setdefault((name, s), {})[k] = (refq(z, k, s), float(z["spread"][k][STAGES.index(s)]))
    assert {key: sorted(v) for key, v in found.items()} == {key: sorted(v) for key, v in NOT_ARBITRATED.items()}, found
    for key, picks in NOT_ARBITRATED.items():
        for k, (rq, sp) in picks.items():
            assert abs(found[key][k][0] - rq) <= 0.06 * rq and abs(found[key][k][1] - sp) <= 0.06 * sp, (key, k, found[key][k])
    # tmp and glarea run no in-band rule: every pick of theirs is arbitrated
    assert all(s == "totlap" for _, s in NOT_ARBITRATED)


FAMILY_PROGRAM = r"""
#include "ucf_launch_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv)
{
    for (int i = 1; i + 1 < argc; i += 2) {
        ucf_dev_params dp;
        memset(&dp, 0, sizeof(dp));
        dp.model = atoi(argv[i]); dp.MNtype = atoi(argv[i + 1]);
        printf("%d\n", family_of(dp));
    }
    return 0;
}
"""


def families_of(tmp_dir, names):
    """family_of (ucf_launch_plan.h) of the decks' model and MNtype, from a stand-alone program: {deck: family}"""
    src = os.path.join(tmp_dir, "family_of.cpp")
    exe = os.path.join(tmp_dir, "family_of")
    with open(src, "w") as f:
        f.write(FAMILY_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "unconfined_amd", "csrc"), src, "-o", exe], check=True)
    args = []
    for name in names:
        dk, ts, P = load_deck(name)
        args += [str(dk.model), str(dk.MNtype)]
    out = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.split()
    return {name: int(v) for name, v in zip(names, out)}


def test_the_decks_reach_all_six_families(tmp_path):
    fam = families_of(str(tmp_path), DECKS)
    assert set(fam.values()) == {0, 1, 2, 3, 4, 5}
    for f, decks in gen.FAMILY_DECKS.items():
        assert decks and all(fam[d] == f for d in decks), (f, [fam[d] for d in decks])


def test_the_oracle_built_here_gives_the_files_bits(files, oracle, oracle_quad):
    """2d: the first pick of every deck in binary64 (vectors bit for bit, spread the same number), one pick of c1_theis in
    binary128"""
    for name, z in files.items():
        dk, ctx = gen.context(oracle, name)
        it, ir = z["picks"][0]
        st, sq, rq, spread = gen.one_pick(oracle, oracle_quad if name == "c1_theis" else None, ctx, int(it), int(ir))
        for s in STAGES:
            assert st[s].tobytes() == z[f"0_{s}"].tobytes(), (name, s)
            if sq is not None:
                assert sq[s].tobytes() == z[f"0_{s}_q"].tobytes(), (name, s)
        assert np.array_equal(spread, z["spread"][0]), name
        if rq is not None:
            assert np.array_equal(rq, z["refq"][0])
