"""UCF_PH_SH of the folded one-depth water-table kernel ("Re eta zD >= 0.35 in every lane from here on": ucf_fastpath.h; the
limit of its bound: zpair_bound_limit, ucf_launch_plan.h) against the model of tools/folded_loop_phase_shares.py, on the CPU.

prim_from_e takes sinh(x) from its series below x = 0.35 and from e^x / 2 - e^-x / 2 above, per lane, for the two primitives of
the cosh/sinh form (eta and eta zD).  A unit proven on that form sets the bit from its lower end lob -- zpair_unit_bounds from
kappa (Re eta)^2 >= Re p + lob^2 against kappa (0.35 / zD)^2 / (1 - 2^-19), zpair_interval_class from Re eta at lob where the
bounds did not decide the unit -- and a proven cosh/sinh J0 interval of a part that has the bit runs a loop without the test.
Re eta grows with the abscissa, every node of a unit lies at or above its lower end and every later unit above that.  Here
both tests are restated in binary64 (sh_bound_v, sh_exact_v) and applied to every unit the kernel classifies as cosh/sinh --
J0 intervals and the two tanh-sinh runs -- on the sweep that bench.py times (every 8th radius, every Laplace index) and on the
grids of tests/test_gpu_folded_loop_drops.py.  Wherever either sets the bit, eta is recomputed at every node from the unit's
first to the item's last, in every lane: no Re eta zD may be below 0.35, and none within 2^-21 of it (the margin of the
classifiers is 2^-20; the computed eta follows the true one to a few ulp).  The share of the sweep's proven cosh/sinh
Gauss-Lobatto pairs that run with the bit is printed and must be at least one half: below that the loops would not be worth
their place in the instruction cache.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MARGIN = 2.0 ** -21


def check_grid(S, tD, radii, depths, seen):
    """every cosh/sinh unit of the grid at every depth; seen counts the units by who set the bit"""
    kappa = S.P.kappa
    CS = (S.CLASSES.index("cs_tab"), S.CLASSES.index("cs_short"))
    worst = np.inf
    for s, p in S.waves(tD):                                      # p[lane][m]
        for rD in radii:
            a = S.row(rD, s)
            re = np.sqrt((p[:, :, None] + a[None, None, :] ** 2) / kappa).real.min(0)      # [m][abscissa], the slowest lane
            re_from = np.minimum.accumulate(re[:, ::-1], axis=1)[:, ::-1]                  # ... from an abscissa to the item's end
            for zD in depths:
                for kind, b, e, cls, sets, have, ip, lob, hib in S.sh_walk(p, a, s, rD, zD):
                    assert lob <= a[b:e].min(), (kind, s, rD, b)
                    is_cs = (cls == CS[0]) | (cls == CS[1])
                    by_bound, by_eta = is_cs & S.sh_bound_v(p, lob, zD), is_cs & S.sh_exact_v(p, lob, zD)
                    seen[kind]["cs"] += int(is_cs.sum())
                    seen[kind]["bound"] += int(by_bound.sum())
                    seen[kind]["eta"] += int(by_eta.sum())
                    seen[kind]["eta_only"] += int((by_eta & ~by_bound).sum())
                    assert np.all(sets <= (by_bound | by_eta)), (kind, s, rD, b, zD)
                    sel = by_bound | by_eta
                    if sel.any():
                        x = re_from[sel, b] * zD
                        worst = min(worst, float(x.min()))
                        assert np.all(x >= S.SINH_SERIES * (1.0 + MARGIN)), (kind, s, rD, b, zD, float(x.min()))
    return worst


def new_counts():
    return {k: dict(cs=0, bound=0, eta=0, eta_only=0) for k in ("ts", "interval")}


def test_where_the_bit_is_set_no_later_node_is_below_the_series_limit_on_the_bench_sweep():
    import folded_loop_phase_shares as S
    tD, radii, zD = S.bench_grid()
    seen = new_counts()
    worst = check_grid(S, tD, radii, (zD,), seen)
    print("bench sweep:", seen, f"; smallest Re eta zD behind a set bit: {worst:.9f}")
    for kind in ("ts", "interval"):
        assert seen[kind]["bound"] > 0 and seen[kind]["eta"] >= seen[kind]["bound"], (kind, seen[kind])
    cnt, ev = S.sh_shares(tD, radii, zD)
    cs = cnt["cs_sh"] + cnt["cs_plain"]
    share = cnt["cs_sh"] / cs
    print(f"proven cosh/sinh Gauss-Lobatto pairs of the sweep: {cs}, with UCF_PH_SH {100.0 * share:.2f} %; {ev}")
    assert share >= 0.5, (cnt, ev)


def test_where_the_bit_is_set_no_later_node_is_below_the_series_limit_on_the_test_grids():
    import folded_loop_phase_shares as S
    import test_gpu_folded_loop_drops as T
    seen = new_counts()
    worst = np.inf
    for clusters, radii in sorted({(c[4], c[5]) for c in T.CALLS}):
        tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in clusters])
        depths = sorted({c[2] for c in T.CALLS if (c[4], c[5]) == (clusters, radii)})
        worst = min(worst, check_grid(S, tD, np.array(radii), depths, seen))
    print("test grids:", seen, f"; smallest Re eta zD behind a set bit: {worst:.9f}")
    assert {c[2] for c in T.CALLS} == {0.0, 0.4, T.ZBENCH, 1.0}
    for kind in ("ts", "interval"):
        # set by the bounds, set by eta where the bounds were too weak, and cosh/sinh units that stay without it
        assert seen[kind]["bound"] > 0 and seen[kind]["eta_only"] > 0 and seen[kind]["cs"] > seen[kind]["eta"], (kind, seen[kind])


def test_the_cases_the_gpu_grids_are_there_for_occur_in_them():
    import folded_loop_phase_shares as S
    import test_gpu_folded_loop_drops as T
    for tag, beta, zD, cut, clusters, radii in T.CALLS:
        tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in clusters])
        cnt, ev = S.sh_shares(tD, np.array(radii), zD, int(cut.get("UCF_NSPLIT", 1)))
        print(tag, cnt, ev)
        if zD == 0.0:
            assert cnt["cs_sh"] == 0 and ev["never"] == ev["parts"] and cnt["cs_plain"] > 0, (tag, cnt, ev)
            continue
        # loops with and without the bit both run; the limit is crossed inside a unit and between the lanes of a wave
        assert cnt["cs_sh"] > 0 and cnt["cs_plain"] > 0 and ev["inside"] > 0, (tag, cnt, ev)
        if cut:
            assert ev["never"] > 0 and ev["first_of_part_after_none"] > 0, (tag, ev)      # ... and at a part boundary
        else:
            assert ev["ts_sets"] > 0, (tag, ev)                       # a tanh-sinh run sets it for the intervals behind it
        if clusters == T.LATE:
            assert ev["lanes_split"] > 0, (tag, ev)


def test_a_nan_a_depth_of_zero_or_a_value_inside_the_margin_sets_nothing():
    import folded_loop_phase_shares as S
    k = S.P.kappa
    p = np.full(64, 1e-9 + 0.0j)
    a0 = S.SINH_SERIES / 0.5 * np.sqrt(k)                       # Re eta zD = 0.35 about there, at zD = 0.5
    for test in (S.sh_bound_v, S.sh_exact_v):
        assert bool(test(p, 1.1 * a0, 0.5))
        assert not bool(test(p, 0.9 * a0, 0.5))
        assert not bool(test(p, a0 * (1.0 + 2.0 ** -22), 0.5))      # inside the 2^-20 margin
        assert bool(test(p, a0 * (1.0 + 2.0 ** -18), 0.5))
        assert not bool(test(p, 1e6, 0.0))                          # zD = 0: sinh(eta zD) = 0 is the series' business for good
        q = p.copy(); q[5] = complex(np.nan, 0.0)
        assert not bool(test(q, 1.1 * a0, 0.5))
        q = p.copy(); q[5] = 1e-9 - (1.1 * a0) ** 2 + 0.0j          # one lane short of the limit
        assert not bool(test(q, 1.1 * a0, 0.5))
    assert S.sh_limit(0.0) == np.inf and S.sh_limit(1.0) == k * (0.35 * 0.35) / (1.0 - 2.0 ** -19)
