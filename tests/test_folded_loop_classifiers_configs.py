"""The loop classifiers of the folded one-depth water-table kernel at every configuration of tests/folded_configs.py, on the CPU.

tests/test_folded_loop_{bound_classifier,interval_classifier,sh_bound}.py check the model of the classifiers
(tools/folded_loop_phase_shares.py) node by node at the C2 deck's kappa = 0.4.  Every limit of the classifiers is a function
of kappa, of the depth and of the Laplace parameters, so the same checks -- the check_grid functions of those three files,
unchanged -- run here with a Model per configuration (kappa 0.03 ... 4, zD 0 ... 1, Malama's and Moench's boundary, other
numerics) on the grid that the stage fixtures and tests/test_gpu_stages_folded.py use (256 times x 5 radii):

  * bounds: for every unit the bounds decide, eta recomputed at every node violates nothing that was decided;
  * exact classifier: the same for every J0 interval it proves;
  * UCF_PH_SH: wherever the bit is set, Re eta zD at every later node of the item is >= 0.35 (1 + 2^-21).

A pass that decides nothing is ruled out per configuration: each of the five classes occurs (at zD = 1 the four that can:
folded_configs.reachable_loops), the bounds decide each of the proven classes somewhere and leave something to the exact
classifier, and for zD > 0 the bit is set by the bounds somewhere and left unset on a cosh/sinh unit somewhere (zD = 0: never
set).  No GPU."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import folded_configs as FC
import test_folded_loop_bound_classifier as TB
import test_folded_loop_interval_classifier as TI
import test_folded_loop_sh_bound as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@functools.lru_cache(maxsize=None)
def model(tag):
    import folded_loop_phase_shares as S
    _, over, zD = FC.config(tag)
    m = S.Model(deck=FC.DECK, **over)
    assert m.P.kappa == over["kappa"] and m.kappa == over["kappa"]
    return m


@pytest.mark.parametrize("tag", FC.TAGS)
def test_no_node_of_a_unit_the_bounds_decide_violates_what_was_decided(tag):
    S, zD = model(tag), FC.config(tag)[2]
    seen = TB.new_counts(S)
    TB.check_grid(S, FC.times(), FC.radii(), (zD,), seen)
    print(tag, {k: {c: n for c, n in v.items() if n} for k, v in seen.items()})
    iv = seen["interval"]
    assert sum(iv.values()) == 4 * len(FC.RD) * S.nacc * (2 * S.M + 1), iv
    proven = [c for c in FC.reachable_classes(zD) if c != "unproven"]
    assert all(iv[c] > 0 for c in proven) and iv["undecided"] > 0, (tag, iv)
    assert all(seen[kind][c] == 0 for kind in TB.KINDS for c in S.CLASSES[:4] if c not in proven), (tag, seen)
    for kind in TB.KINDS:
        assert sum(seen[kind][c] for c in S.CLASSES[:4]) > 0, (tag, kind, seen[kind])


@pytest.mark.parametrize("tag", FC.TAGS)
def test_no_node_of_an_interval_the_exact_classifier_proves_violates_what_was_proven(tag):
    S, zD = model(tag), FC.config(tag)[2]
    seen = dict.fromkeys(S.CLASSES, 0)
    TI.check_grid(S, FC.times(), FC.radii(), zD, seen)
    print(tag, seen)
    assert sum(seen.values()) == 4 * len(FC.RD) * S.nacc * (2 * S.M + 1), seen
    assert all((seen[c] > 0) == (c in FC.reachable_classes(zD)) for c in S.CLASSES), (tag, seen)


@pytest.mark.parametrize("tag", FC.TAGS)
def test_where_the_bit_is_set_no_later_node_is_below_the_series_limit(tag):
    S, zD = model(tag), FC.config(tag)[2]
    seen = TS.new_counts()
    worst = TS.check_grid(S, FC.times(), FC.radii(), (zD,), seen)
    print(tag, seen, f"; smallest Re eta zD behind a set bit: {worst:.9f}")
    cs = sum(seen[k]["cs"] for k in seen)
    assert cs > 0, (tag, seen)
    if zD == 0.0:
        assert all(seen[k]["bound"] == 0 and seen[k]["eta"] == 0 for k in seen) and worst == np.inf, (tag, seen)
        return
    assert worst >= S.SINH_SERIES * (1.0 + TS.MARGIN)
    # set by the bounds in both kinds of unit, and cosh/sinh units that stay without it.  (Of the J0 intervals only where the
    # grid has one: at kappa = 0.03 and zD = 1 the lowest interval end, j0z[0] / 30 = 0.080, is already past
    # 0.35 sqrt(kappa) / zD = 0.061, and every cosh/sinh interval sets the bit; the tanh-sinh runs below it do not.)
    for kind in ("ts", "interval"):
        assert seen[kind]["bound"] > 0, (tag, kind, seen[kind])
    assert seen["ts"]["cs"] > seen["ts"]["eta"], (tag, seen)
    lowest = S.j0z[int(S.P.j0s[0]) - 1] / max(FC.RD)
    if lowest < S.SINH_SERIES * np.sqrt(S.kappa) / zD:
        assert seen["interval"]["cs"] > seen["interval"]["eta"], (tag, seen)


def test_the_models_differ_where_the_configurations_do():
    """the limits follow the configuration's kappa and depth (a Model that read the C2 deck's would pass the rest)"""
    import folded_loop_phase_shares as S
    for tag, over, zD in FC.CONFIGS:
        m = model(tag)
        Z = m.bound_limits(zD)
        k = over["kappa"]
        assert Z["cs"] == k * (m.maxexp * m.maxexp) / (1.0 + 2.0 ** -19) and Z["ys"] == 4.0 * k * (S.SMALL * S.SMALL)
        lim, s = 0.99 * 700.0, (0.35 / zD if zD > 0.0 else np.inf)
        assert Z["range"] == k * (lim * lim) and Z["im"] == k * (1.0e6 * 1.0e6)
        assert m.sh_limit(zD) == k * (s * s) / (1.0 - 2.0 ** -19)
        assert (m.M, m.nacc, m.ngl) == (over.get("M", 26), over.get("nacc", 10), over.get("ord", 50) - 2)
    assert S.DEFAULT.kappa == 0.4 and S.P.kappa == 0.4


LIMITS_PROGRAM = r"""
#include "ucf_launch_plan.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv)
{
    for (int i = 1; i + 3 < argc; i += 4) {
        ucf_dev_params dp;
        memset(&dp, 0, sizeof(dp));
        dp.kappa = strtod(argv[i], nullptr); dp.zD[0] = strtod(argv[i + 1], nullptr);
        dp.fast_eta_max = strtod(argv[i + 2], nullptr); dp.fast_im_max = strtod(argv[i + 3], nullptr);
        dp.maxexp = -log(DBL_EPSILON) / 3.0;      // ucf_plan.cpp
        for (int w = 0; w < UCF_ZB_COUNT; w++) printf("%a ", zpair_bound_limit(dp, w));
        printf("%a %a\n", (double)UCF_ZB_SC_SMALL, (double)UCF_ZB_SINH_SERIES);
    }
    return 0;
}
"""


def test_the_models_limits_are_those_of_the_kernels_own_function(tmp_path):
    """zpair_bound_limit (ucf_launch_plan.h: constexpr, host and device; abscissa_kernel writes its values into the table the
    kernel reads) from a stand-alone program, against the model's bound_limits and sh_limit at every configuration, bit for
    bit: what the soundness checks above prove of the model holds of the limits the device is given"""
    import folded_loop_phase_shares as S
    src, exe = os.path.join(str(tmp_path), "limits.cpp"), os.path.join(str(tmp_path), "limits")
    with open(src, "w") as f:
        f.write(LIMITS_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "unconfined_amd", "csrc"), src, "-o", exe],
                   check=True)
    cases = [(model(tag), zD) for tag, _, zD in FC.CONFIGS] + [(S.DEFAULT, 0.9106), (S.DEFAULT, 0.5)]
    args = [x for m, zD in cases for x in (float(m.kappa).hex(), float(zD).hex(), float(m.fast_eta_max).hex(), float(m.fast_im_max).hex())]
    rows = subprocess.run([exe, *args], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(rows) == len(cases)
    names = ("range", "im", "cs", "ex", "ys", "yl")              # UCF_ZB_RANGE ... UCF_ZB_YL, then UCF_ZB_SH
    for (m, zD), row in zip(cases, rows):
        got = [float.fromhex(x) for x in row.split()]
        Z = m.bound_limits(zD)
        assert [Z[n] for n in names] == got[:6], (m.kappa, zD, Z, got)
        assert m.sh_limit(zD) == got[6], (m.kappa, zD, m.sh_limit(zD), got[6])
        assert got[7] == 0.0 and got[8:] == [S.SMALL, S.SINH_SERIES], got
        assert m.maxexp == -np.log(np.finfo(float).eps) / 3.0
