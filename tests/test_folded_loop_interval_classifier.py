"""The interval classifier of the folded one-depth water-table kernel (zpair_interval_class, ucf_fastpath.h) against the
model of tools/folded_loop_phase_shares.py, on the CPU.

The kernel decides once per J0 interval, from eta at the interval's two ends, what holds at all of its Gauss-Lobatto nodes
in every lane: the fast evaluators' range, the form of the closure (cosh/sinh below Re eta = maxexp, exponential above), and
whether every sin/cos argument of that form is below UCF_SC_SMALL.  interval_class() of the tool restates the classifier in
binary64 with its margins.  Here, for the p-values and interval boundaries of the sweep that bench.py times (every 8th
radius, every Laplace index), eta is recomputed at every node of every interval the classifier proves, and no node may
violate what was proven -- by the exact limits the kernel's evaluators have, not the classifier's margins.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def check_grid(S, tD, radii, zD, seen):
    """every J0 interval of the grid at the depth zD; seen[class] counts them (S: the tool's module or a Model of it)"""
    kappa, M, nacc, ngl = S.P.kappa, S.M, S.nacc, S.ngl
    for s, p in S.waves(tD):
        for rD in radii:
            a = S.row(rD, s)[S.N:].reshape(nacc, ngl)
            for jj in range(nacc):
                lob, hib = S.j0z[s + jj - 1] / rD, S.j0z[s + jj] / rD
                assert lob < a[jj].min() and a[jj].max() < hib
                for m in range(2 * M + 1):
                    pm = p[:, m]
                    cls = S.interval_class(pm, lob, hib, zD)
                    seen[cls] += 1
                    if cls == "unproven":
                        continue
                    eta = np.sqrt((pm[:, None] + a[jj][None, :] ** 2) / kappa)      # [lane][node]
                    where = (cls, s, rD, jj, m)
                    assert np.all(pm.real[:, None] + a[jj][None, :] ** 2 > 0.0), where
                    assert np.all(eta.real <= S.FAST_ETA_MAX) and np.all(np.abs(eta.imag) < S.FAST_IM_MAX), where
                    assert np.all(eta.imag >= 0.0), where                            # (sincos_small_ wants +0 or above)
                    if cls.startswith("cs"):
                        assert np.all(eta.real < S.maxexp), where
                        arg = np.abs(eta.imag)
                    else:
                        assert np.all(eta.real >= S.maxexp), where
                        arg = np.abs(eta.imag) * (1.0 - zD)
                    if cls.endswith("short"):
                        assert np.all(arg < S.SMALL), where


def test_no_node_of_a_proven_interval_violates_what_was_proven():
    import folded_loop_phase_shares as S
    tD, radii, zD = S.bench_grid()
    seen = dict.fromkeys(S.CLASSES, 0)
    check_grid(S, tD, radii, zD, seen)
    # the sweep exercises every class, and the classifier proves most of it (the premise of the interval loops)
    assert all(seen[c] > 0 for c in S.CLASSES), seen
    assert sum(seen[c] for c in S.CLASSES if c != "unproven") >= 0.8 * sum(seen.values()), seen


def test_a_nan_or_a_value_at_a_limit_proves_nothing():
    import folded_loop_phase_shares as S
    p = np.full(64, 0.5 + 0.0j)
    assert S.interval_class(p, 1.0, 2.0, 0.5) != "unproven"
    q = p.copy(); q[7] = complex(np.nan, 0.0)
    assert S.interval_class(q, 1.0, 2.0, 0.5) == "unproven"
    q = p.copy(); q[7] = -1.0                                   # Re p <= 0
    assert S.interval_class(q, 0.5, 2.0, 0.5) == "unproven"
    k = S.P.kappa
    a_max = S.maxexp * np.sqrt(k)                               # Re eta = maxexp about there: the interval straddles it
    assert S.interval_class(p * 0 + 1e-9, 0.9 * a_max, 1.1 * a_max, 0.5) == "unproven"
    assert S.interval_class(p * 0 + 1e-9, 0.8 * a_max, 0.9 * a_max, 0.5).startswith("cs")
    assert S.interval_class(p * 0 + 1e-9, 1.1 * a_max, 1.2 * a_max, 0.5).startswith("ex")
    a_out = S.FAST_ETA_MAX * np.sqrt(k)
    assert S.interval_class(p, 0.9 * a_out, 0.995 * a_out, 0.5) == "unproven"      # inside the 1 % margin
