#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- mid-pipeline stage vectors for EVERY evaluator family (family_of, ucf_launch_plan.h), with the
reference's own rounding noise beside them.  gen_midstages.py covers the water-table and finite-difference families
(2 and 4) with five points per deck; this generator takes the same 128 x 2 grid (grid() is imported from there) and writes,
per deck and pick,

    tmp, glarea, totlap           the binary64 oracle's loop body (ucfo_point; driver.f90:135-216)
    tmp_q, glarea_q, totlap_q     the binary128 build of the same code
    refq   [npicks, 3]            distance of the binary64 vectors from the binary128 ones        (tmp, glarea, totlap)
    spread [npicks, 3]            the largest change of the binary64 vectors when tD or rD moves by one ulp: four draws
                                  (tD up, tD down, rD up, rD down).  It needs the reference only, and it measures what
                                  another binary64 realisation of the same algorithm may differ by

both in the measure of tests/test_gpu_stages.py::_vec_err (max norm over the Laplace samples, relative to the vector's
largest modulus).  One file per deck: tests/golden/midstages_fam_<deck>.npz.

    python oracle/gen_midstages_families.py [deck ...]        (no argument: every deck)

Decks by family.  tests/test_midstages_families.py holds every one of them to the information caps (spread <= 1e-12 for
tmp and glarea, <= 1e-11 for totlap, at six picks or more).  Left out on purpose:
    hantush_lay3      a depth above the screen top: pure cancellation, the binary64 and binary128 glarea differ by factors
                      of 1e19 -- no information at stage level ("where the reference itself is noise")
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_midstages import NT, RADII, grid  # noqa: E402
from golden_util import GOLD  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

FAMILY_DECKS = {
    0: ["c1_theis", "theis_sched3"],                                         # (a schedule: the laptime multiplier)
    1: ["hantush_lay1", "hantush_lay2", "hantush_fullpen"],
    5: ["hstorage_partpen_lay1", "hstorage_partpen_lay2", "hstorage_fullpen_lay1"],
    3: ["mishra_malama"],
    4: ["c5_mishra_fd64", "mishra_fd30"],                                    # (two orders of the finite differences)
    2: ["c2_neuman74_fullpen", "neuman74_partpen", "c3_moench", "c4_malama_partpen", "malama_fullpen", "malama_k10", "neuman_sched2"],
}
DECKS = [d for f in (0, 1, 5, 3, 4, 2) for d in FAMILY_DECKS[f]]
STAGES = ("tmp", "glarea", "totlap")
# (time index, radius index): the radii alternate, the times span the grid.  Six picks, not eight: eight of them make
# 3.3 MB of fixtures over the 18 decks.  All six lie within the caps for every deck: the larger radius at time indices
# below about 30 (h ~ 0: totlap spread 1e-11 ... 3e-9 in every family) is avoided
PICKS = [(4, 0), (37, 1), (62, 0), (87, 1), (110, 0), (126, 1)]
# decks whose default picks would leave fewer than six within the caps take others (the reason beside each)
DECK_PICKS = {
    # (126, 1): tmp spread 1.8e-12 (1.5e-12 from binary128) -- the Thomas recursion of order 64 amplifies at late times
    "c5_mishra_fd64": PICKS[:5] + [(118, 1)],
}


def cplx(a):
    return a[..., 0] + 1j * a[..., 1]


def vec_err(got, ref):
    """tests/test_gpu_stages.py::_vec_err"""
    scale = np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-300)
    return float((np.abs(got - ref) / scale).max())


def one_pick(O, Q, ctx, it, ir):
    """(binary64 stages, binary128 stages, refq[3], spread[3]) of one pick; Q None: no binary128 evaluation"""
    P, D, j0z, tD, sv, rD, zD, zl = ctx
    t, r = float(tD[it]), float(rD[ir])
    _, _, st = O.point(P, D, j0z, t, r, sv[it], zD, zl, stages=True)
    spread = np.zeros(3)
    for tt, rr in ((np.nextafter(t, np.inf), r), (np.nextafter(t, 0.0), r), (t, np.nextafter(r, np.inf)), (t, np.nextafter(r, 0.0))):
        _, _, s2 = O.point(P, D, j0z, tt, rr, sv[it], zD, zl, stages=True)
        spread = np.maximum(spread, [vec_err(cplx(s2[k]), cplx(st[k])) for k in STAGES])
    if Q is None:
        return st, None, None, spread
    _, _, sq = Q.point(P, D, j0z, t, r, sv[it], zD, zl, stages=True)
    refq = np.array([vec_err(cplx(st[k]), cplx(sq[k])) for k in STAGES])
    return st, sq, refq, spread


def context(O, name):
    dk, P, D, tD, sv, rD, zD, zl = grid(O, name)
    return dk, (P, D, O.j0_zeros(D.nj0z), tD, sv, rD, zD, zl)


def path_of(name):
    return os.path.join(GOLD, f"midstages_fam_{name}.npz")


def main(names):
    O, Q = Oracle(), Oracle(quad=True)
    for name in names:
        dk, ctx = context(O, name)
        picks = DECK_PICKS.get(name, PICKS)
        out = {"picks": np.array(picks, np.int32), "radii": np.array(RADII), "nt": np.array([NT]),
               "refq": np.zeros((len(picks), 3)), "spread": np.zeros((len(picks), 3))}
        for k, (it, ir) in enumerate(picks):
            st, sq, refq, spread = one_pick(O, Q, ctx, it, ir)
            for key in STAGES:
                out[f"{k}_{key}"] = st[key]
                out[f"{k}_{key}_q"] = sq[key]
            out["refq"][k], out["spread"][k] = refq, spread
            print(name, "model", dk.model, "pick", k, (it, ir), "refq tmp %.1e gl %.1e tl %.1e" % tuple(refq),
                  "| spread tmp %.1e gl %.1e tl %.1e" % tuple(spread), flush=True)
        np.savez_compressed(path_of(name), **out)
        print(name, os.path.getsize(path_of(name)), "bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or DECKS)
