#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- whole points with more Laplace samples than a wave has lanes (M > 31), for
tests/test_gpu_dehoog_big.py.  Per deck and M the 12 points of a 6 x 2 grid (6 times 10 ** linspace(-1, 3, 6), radii rD 0.1
and 3.0) at the deck's own depths cut to two (one for a piezometer deck), from this repository's oracle alone:

    tD [6], rD [2], sv [6], zD [nz], zl [nz]      the inputs, as the tests pass them on (the same for every M)
    ref_h_M<M>, ref_dh_M<M>     [12, nz]          ucfo_batch in binary64, point = it * 2 + ir
    noise_h_M<M>, noise_dh_M<M> [12, nz]          |binary64 - binary128| / max(|binary128|, 1e-3)
    spread_h_M<M>, spread_dh_M<M> [12, nz]        what one ulp in tD or rD changes in the binary64 values (spread())

Two times of the six are others for one deck each (REPLACED, with the reason).

One file per deck: tests/golden/dehoog_big_<deck>.npz.  A point in binary128 with 129 samples takes seconds, which is why the
values are kept in a file; tests/test_gpu_dehoog_big.py checks without a GPU that the inputs follow from the deck bit for bit
and that the binary64 oracle built there gives ref_* again.

    python oracle/gen_dehoog_big.py [deck ...]        (no argument: every deck)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from golden_util import GOLD, load_deck  # noqa: E402
from oracle_lib import Oracle  # noqa: E402
from unconfined_amd.abi import params_from_deck  # noqa: E402

DECKS = ("c2_neuman74_fullpen", "neuman74_partpen", "hantush_lay1", "c3_moench")
MS = (32, 64)                   # 65 samples: two register sets per lane; 129: four
NT, RADII, NZ = 6, (0.1, 3.0), 2
# deck -> {time index: exponent taken instead of linspace(-1, 3, 6)[index]}.  At the time it replaces the binary64 oracle is not
# sharp enough for the gate max(1e-10, 10 noise): ONE ulp in tD moves its own dh with 129 samples by more than that (relative
# to max(|dh|, 1e-3)), although it happens to lie within 1e-12 of binary128 at the very point -- no other binary64 evaluation
# can be asked to come closer to it than it comes to itself.  These jumps sit at single bit patterns of tD: neighbours a few
# per cent away are sharp (spread_* below, which tests/test_gpu_dehoog_big.py holds to the gate without a GPU)
REPLACED = {
    "c2_neuman74_fullpen": {5: 2.8},      # 10^3, rD 0.1, M 64: dh moves by 3.2e-10 under tD - 1 ulp, 3.2 times the gate
    "c3_moench": {3: 1.3},                # 10^1.4, rD 0.1, second depth, M 64: dh moves by 2.8 times the gate
}


def path_of(name):
    return os.path.join(GOLD, f"dehoog_big_{name}.npz")


def inputs(O, name):
    """(deck, tD [6], rD [2], sv [6], zD, zl): none of them depends on M"""
    dk, ts, P = load_deck(name)
    D = O.nondim(P)
    e = O.linspace(-1.0, 3.0, NT)
    for i, v in REPLACED.get(name, {}).items():
        e[i] = v
    tD = 10.0 ** e
    sv = O.split_vector(list(dk.j0s), tD)
    zz = O.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd)
    zD = np.ascontiguousarray((zz / D.Lc)[:NZ])
    return dk, tD, np.array(RADII), sv, zD, O.zlay(D, zD)


def points(tD, rD, sv):
    """the grid as a list, point = it * nr + ir"""
    return np.repeat(tD, len(rD)), np.tile(rD, len(tD)), np.repeat(sv, len(rD)).astype(np.int32)


def params(dk, M):
    return params_from_deck(dk.replace(M=M))


def reference(O, dk, M, tD, rD, sv, zD, zl):
    tl, rl, sl = points(tD, rD, sv)
    return O.batch(params(dk, M), tl, rl, sl, zD, zl)


def spread(O, dk, M, tD, rD, sv, zD, zl):
    """the largest change of the binary64 oracle's own h and dh when every tD or every rD moves by one ulp (four draws: up and
    down), relative to max(|value|, 1e-3)"""
    tl, rl, sl = points(tD, rD, sv)
    P = params(dk, M)
    h0, d0 = O.batch(P, tl, rl, sl, zD, zl)
    sh, sd = np.zeros_like(h0), np.zeros_like(d0)
    for to in (np.inf, -np.inf):
        for t2, r2 in ((np.nextafter(tl, to), rl), (tl, np.nextafter(rl, to))):
            h, d = O.batch(P, t2, r2, sl, zD, zl)
            sh, sd = np.maximum(sh, np.abs(h - h0)), np.maximum(sd, np.abs(d - d0))
    return sh / np.maximum(np.abs(h0), 1e-3), sd / np.maximum(np.abs(d0), 1e-3)


def main(names):
    O, Q = Oracle(), Oracle(quad=True)
    for name in names:
        dk, tD, rD, sv, zD, zl = inputs(O, name)
        out = {"tD": tD, "rD": rD, "sv": sv, "zD": zD, "zl": zl}
        for M in MS:
            h, dh = reference(O, dk, M, tD, rD, sv, zD, zl)
            hq, dq = reference(Q, dk, M, tD, rD, sv, zD, zl)
            with np.errstate(invalid="ignore"):
                nh = np.abs(h - hq) / np.maximum(np.abs(hq), 1e-3)
                nd = np.abs(dh - dq) / np.maximum(np.abs(dq), 1e-3)
            out[f"ref_h_M{M}"], out[f"ref_dh_M{M}"], out[f"noise_h_M{M}"], out[f"noise_dh_M{M}"] = h, dh, nh, nd
            sh, sd = spread(O, dk, M, tD, rD, sv, zD, zl)
            out[f"spread_h_M{M}"], out[f"spread_dh_M{M}"] = sh, sd
            print(name, "M", M, "worst spread / max(1e-10, 10 noise): h %.2f dh %.2f" %
                  ((sh / np.maximum(1e-10, 10 * nh)).max(), (sd / np.maximum(1e-10, 10 * nd)).max()), flush=True)
            print(name, "M", M, "finite", int(np.isfinite(h).sum()), "of", h.size, "worst noise h %.1e dh %.1e" % (np.nanmax(nh), np.nanmax(nd)), flush=True)
        np.savez_compressed(path_of(name), **out)
        print(name, os.path.getsize(path_of(name)), "bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or DECKS)
