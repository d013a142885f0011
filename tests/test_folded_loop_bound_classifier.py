"""The bound classifier of the folded one-depth water-table kernel (zpair_unit_bounds, ucf_fastpath.h; its limits:
zpair_bound_limit, ucf_launch_plan.h) against the model of tools/folded_loop_phase_shares.py, on the CPU.

Before the kernel pays for eta at the two ends of a quadrature unit (zpair_interval_class), it tries bounds that need no eta:
for Re p > 0, (Re p + a^2) / kappa <= (Re eta)^2 <= (Re p + a^2 + |Im p| / 2) / kappa and (Im eta)^2 <= (Im p)^2 /
(4 kappa (Re p + a^2)), all monotone in the abscissa a, so that the two ends of a unit bound every node in it.  bound_class_v()
of the tool restates the device code in binary64 with its limits and margins.  Here the units are the ones the kernel
classifies -- whole J0 intervals and the tanh-sinh part in 1, 2 or 4 runs of nodes -- and the 12-node runs of Gauss-Lobatto
nodes, over the sweep that bench.py times (every 8th radius, every Laplace index: 271 360 intervals) and over the grids of
tests/test_gpu_folded_loop_intervals.py and tests/test_gpu_folded_loop_units.py at zD = 0, 0.4, 0.9106 and 1.  For every unit
the bounds decide, eta is recomputed at every node, and no node may violate what was decided -- by the exact limits the
kernel's evaluators have, not the classifier's margins.  The bounds must also decide at least 85 % of the sweep's J0
intervals (the model gives 89.7 %): a classifier that decides nothing would pass the first check.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KINDS = ("interval", "ts1", "ts2", "ts4", "gl12")


def units_of(S, a, s, rD):
    """(kind, first node, end node, lob, hib) of every unit of the row `a` of radius rD and split index s"""
    N, nacc, ngl = S.N, S.nacc, S.ngl
    out = []
    for jj in range(nacc):
        b = N + jj * ngl
        out.append(("interval", b, b + ngl, S.j0z[s + jj - 1] / rD, S.j0z[s + jj] / rD))
        for r0 in range(0, ngl, 12):                              # (the nodes of an interval descend)
            e = min(r0 + 12, ngl)
            out.append(("gl12", b + r0, b + e, a[b + e - 1], a[b + r0]))
    for runs in (1, 2, 4):
        for b, e in S.ts_runs(runs):
            out.append((f"ts{runs}", b, e, 0.0 if b == 0 else a[b], a[e - 1]))
    return out


def check_grid(S, tD, radii, depths, seen):
    """every unit of the grid at every depth; seen[kind][class or 'undecided'] counts them"""
    kappa = S.P.kappa
    limits = {zD: S.bound_limits(zD) for zD in depths}
    for s, p in S.waves(tD):                                      # p[lane][m]
        for rD in radii:
            a = S.row(rD, s)
            eta = np.sqrt((p[:, :, None] + a[None, None, :] ** 2) / kappa)      # [lane][m][abscissa]
            q_pos = np.all(p.real[:, :, None] + a[None, None, :] ** 2 > 0.0, axis=0)      # [m][abscissa]
            re_max, re_min = eta.real.max(0), eta.real.min(0)
            im_max, im_min = np.abs(eta.imag).max(0), eta.imag.min(0)
            for kind, b, e, lob, hib in units_of(S, a, s, rD):
                assert lob <= a[b:e].min() and a[b:e].max() <= hib, (kind, s, rD, b)
                for zD in depths:
                    cls = S.bound_class_v(p, lob, hib, zD, lim=limits[zD])      # [m]
                    seen[kind]["undecided"] += int((cls == S.UNDECIDED).sum())
                    for k in np.unique(cls[cls != S.UNDECIDED]):
                        name, sel = S.CLASSES[k], cls == k
                        seen[kind][name] += int(sel.sum())
                        where = (kind, name, s, rD, b, zD)
                        assert np.all(q_pos[sel, b:e]), where
                        assert np.all(re_max[sel, b:e] <= S.FAST_ETA_MAX) and np.all(im_max[sel, b:e] < S.FAST_IM_MAX), where
                        assert np.all(im_min[sel, b:e] >= 0.0), where                # (sincos_small_ wants +0 or above)
                        if name.startswith("cs"):
                            assert np.all(re_max[sel, b:e] < S.maxexp), where
                            arg = im_max[sel, b:e]
                        else:
                            assert np.all(re_min[sel, b:e] >= S.maxexp), where
                            arg = im_max[sel, b:e] * (1.0 - zD)
                        if name.endswith("short"):
                            assert np.all(arg < S.SMALL), where


def new_counts(S):
    return {k: dict.fromkeys(S.CLASSES[:4] + ("undecided",), 0) for k in KINDS}


def test_no_node_of_a_unit_the_bounds_decide_violates_what_was_decided_on_the_bench_sweep():
    import folded_loop_phase_shares as S
    tD, radii, zD = S.bench_grid()
    seen = new_counts(S)
    check_grid(S, tD, radii, (zD,), seen)
    iv = seen["interval"]
    assert sum(iv.values()) == 271360, iv
    decided = sum(v for k, v in iv.items() if k != "undecided")
    print("bench sweep:", {k: {c: n for c, n in v.items() if n} for k, v in seen.items()})
    print(f"J0 intervals decided by the bounds alone: {100.0 * decided / sum(iv.values()):.2f} %")
    assert decided >= 0.85 * sum(iv.values()), iv
    # the sweep exercises every class, in the intervals and in the tanh-sinh runs
    for kind in ("interval", "ts2", "ts4"):
        assert all(seen[kind][c] > 0 for c in S.CLASSES[:4]), (kind, seen[kind])


def test_no_node_of_a_unit_the_bounds_decide_violates_what_was_decided_on_the_test_grids():
    import folded_loop_phase_shares as S
    import test_gpu_folded_loop_intervals as TI
    import test_gpu_folded_loop_units as TU
    depths = (0.0, 0.4, TI.ZBENCH, 1.0)
    assert {c[2] for c in TI.CALLS} == set(depths) == {c[2] for c in TU.CALLS}
    seen = new_counts(S)
    for T in (TI, TU):
        tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in T.TD_CLUSTERS])
        check_grid(S, tD, np.array(T.RD), depths, seen)
    print("test grids:", {k: {c: n for c, n in v.items() if n} for k, v in seen.items()})
    for kind in ("interval", "ts2"):
        assert all(seen[kind][c] > 0 for c in S.CLASSES[:4]) and seen[kind]["undecided"] > 0, (kind, seen[kind])


def test_a_nan_or_a_value_at_a_limit_decides_nothing():
    import folded_loop_phase_shares as S
    p = np.full(64, 0.5 + 0.0j)
    assert S.bound_class(p, 1.0, 2.0, 0.5) == "cs_short"
    q = p.copy(); q[7] = complex(np.nan, 0.0)
    assert S.bound_class(q, 1.0, 2.0, 0.5) is None
    q = p.copy(); q[7] = complex(0.5, np.nan)
    assert S.bound_class(q, 1.0, 2.0, 0.5) is None
    q = p.copy(); q[7] = -1.0                                   # Re p <= 0
    assert S.bound_class(q, 0.5, 2.0, 0.5) is None
    k = S.P.kappa
    tiny = p * 0 + 1e-9
    a_max = S.maxexp * np.sqrt(k)                               # Re eta = maxexp about there: the unit straddles it
    assert S.bound_class(tiny, 0.9 * a_max, 1.1 * a_max, 0.5) is None
    assert S.bound_class(tiny, 0.8 * a_max, 0.9 * a_max, 0.5) == "cs_short"
    assert S.bound_class(tiny, 1.1 * a_max, 1.2 * a_max, 0.5) == "ex_short"
    assert S.bound_class(tiny, 0.8 * a_max, a_max * (1.0 - 2.0 ** -22), 0.5) is None      # inside the 2^-20 margin
    assert S.bound_class(tiny, a_max * (1.0 + 2.0 ** -22), 1.2 * a_max, 0.5) is None
    a_out = S.FAST_ETA_MAX * np.sqrt(k)
    assert S.bound_class(p, 0.9 * a_out, 0.995 * a_out, 0.5) is None                     # inside the 1 % margin
    assert S.bound_class(p, 0.9 * a_out, 0.98 * a_out, 0.5) == "ex_short"
    # an argument of sin/cos that the bounds neither prove short nor refute: |Im eta| within its bounds' slack of the limit
    im = 2.0 * k * S.SMALL * np.sqrt((1.0 + 1.0) / k) * (1.0 + 1e-3)     # |Im eta| ~ SMALL (1 + 1e-3) at a = 1, Re p = 1
    mid = np.full(64, complex(1.0, im))
    assert S.bound_class(mid, 1.0, 1.5, 0.5) in (None, "cs_tab")
    assert S.bound_class(np.full(64, complex(1.0, 3.0 * im)), 1.0, 1.5, 0.5) == "cs_tab"
    # the fast evaluators switched off (a limit <= 0): nothing is decided
    assert int(S.bound_class_v(p, 1.0, 2.0, 0.5, lim=S.bound_limits(0.5, fast_eta_max=-1.0))) == S.UNDECIDED
