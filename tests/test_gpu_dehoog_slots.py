"""dehoog_tiles_kernel<TU, false> (fast flavour) after its non-arithmetic instructions were taken out, bit for bit against
the parent.

What changed (ucf_device.h: dehoog_qd_tile_slots, dehoog_cf_slot): the one-lane shifts write registers of their own, the
steps of the solo, the pair and the quad phase of the rhombus run two to a loop turn (values change places, no copies), the
coefficients are stored unnegated and negated where the continued fraction reads them, the validity of a lane comes from a
scalar mask, q(i,1) is one division, and the A and the B recurrence of a vector run on a lane each.  Per lane not one
floating-point operation on a value that reaches a result changed, so h and dh must be the SAME BITS as before:
tests/golden/dehoog_slots_parent.npz holds what the parent build (commit and build id inside the file) gave on an MI355X,
tools/gen_dehoog_slots_fixture.py wrote it.

tests/test_gpu_dehoog_packed.py holds the kernel at M in 26 31 16 15 8 7 3.  This file adds what those calls leave out
(inputs: that test's construction, single IEEE operations only; the fixture keeps their SHA-256):

  through ucf_debug_dehoog_tiles, M in 1 2 9 17 24 30 -- steps in groups of 64 / 32 / 16 lanes:
      M = 1   0 / 0 / 0 + the last step     (no quotient at all)
      M = 2   0 / 0 / 1                     M = 17   1 / 8 / 7
      M = 9   0 / 1 / 7                     M = 24   8 / 8 / 7
                                            M = 30  14 / 8 / 7
    so every loop of paired steps meets an even count, an odd one, one and none.
    fill_M{M}_nt{n}      n in 1 2 3 4 5 7 times (empty groups, odd quads, a partial last tile)
    zero_M{M}_p{k}       4 times, the vector of time k all zeros: each place of the two quads
    nan_M{M}_p{k}        4 times, a NaN in one sample of vector k (sample 1 / M / 2M / 0, real or imaginary part)
    dip_M{M}_{i}{j}      4 times, vector i with sample M x 1e-155, vector j with sample 2M x 1e-155 (every ordered pair): q and
                         e of those vectors leave the range of the unscaled quotient, so one group of a packed pass takes
                         the scaled one while its neighbours do not
    alone_M{M}_{kind}{k} one time: every vector of the dip tiles and the plain ones on their own
  through Plan.drawdown_grid, fast flavour:
    grid_c2              the C2 deck, 7 times x 3 radii (a partial last tile, several radii)
    grid_c3              c3_moench, 6 times x 2 radii, nz = 2 (the kernel's depth loop and its barriers)

Two properties need no fixture: a vector's h and dh in a tile are the bits it gives alone, and the first n times of a
longer call are the bits of the shorter call."""
import hashlib
import os

import numpy as np
import pytest

from golden_util import load_deck
from test_gpu_dehoog_packed import ALPHA, TOL, vectors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dehoog_slots_parent.npz")
MS = (1, 2, 9, 17, 24, 30)
FILLS = (1, 2, 3, 4, 5, 7)
PAIRS = tuple((i, j) for i in range(4) for j in range(4) if i != j)
GRIDS = (("grid_c2", "c2_neuman74_fullpen", (1.0e-2, 0.3, 1.0, 7.0, 1.0e2, 1.0e3, 1.0e4), (0.1, 0.53, 3.0)),
         ("grid_c3", "c3_moench", (1.0e-1, 1.0, 5.0, 1.0e2, 2.0e3, 1.0e4), (0.2, 1.7)))


def steps_by_width(M):
    """quotient steps (r < M) that run in groups of 64, 32 and 16 lanes (dehoog_qd_tile)"""
    r32, r16 = max(M - 15, 1), max(M - 7, 1)
    return r32 - 1, r16 - r32, M - r16


def dip_tiles(M, fp):
    for i, j in PAIRS:
        f = fp[:4].copy()
        f[i, M] = f[i, M] * 1e-155
        f[j, 2 * M] = f[j, 2 * M] * 1e-155
        yield i, j, f


def build_cases():
    """[(tag, M, t, fp)] in a fixed order"""
    cases = []
    for M in MS:
        t, fp = vectors(M)
        for n in FILLS:
            cases.append((f"fill_M{M}_nt{n}", M, t[:n].copy(), fp[:n].copy()))
        for k in range(4):
            f = fp[:4].copy()
            f[k] = 0.0
            cases.append((f"zero_M{M}_p{k}", M, t[:4].copy(), f))
        for k in range(4):
            f = fp[:4].copy()
            f[k, (1, M, 2 * M, 0)[k], k & 1] = np.nan
            cases.append((f"nan_M{M}_p{k}", M, t[:4].copy(), f))
        for i, j, f in dip_tiles(M, fp):
            cases.append((f"dip_M{M}_{i}{j}", M, t[:4].copy(), f))
            for k in (i, j):
                tag = f"alone_M{M}_dip{'ab'[k == j]}{k}"
                if all(c[0] != tag for c in cases):
                    cases.append((tag, M, t[k:k + 1].copy(), f[k:k + 1].copy()))
        for k in range(4):
            cases.append((f"alone_M{M}_plain{k}", M, t[k:k + 1].copy(), fp[k:k + 1].copy()))
    return cases


def grid_inputs():
    """[(tag, deck, tD, rD)]"""
    return [(tag, deck, np.array(tD), np.array(rD)) for tag, deck, tD, rD in GRIDS]


def inputs_digest(cases):
    s = hashlib.sha256()
    for tag, M, t, fp in cases:
        s.update(tag.encode()); s.update(t.tobytes()); s.update(fp.tobytes())
    for tag, deck, tD, rD in grid_inputs():
        s.update(tag.encode()); s.update(deck.encode()); s.update(tD.tobytes()); s.update(rD.tobytes())
    return s.hexdigest()


def run_cases(cases):
    """{tag: (h, dh)} from the library that is loaded, the grids flattened"""
    from unconfined_amd import engine
    got = {tag: engine.debug_dehoog_tiles(M, ALPHA, TOL, t, fp, "fast") for tag, M, t, fp in cases}
    for tag, deck, tD, rD in grid_inputs():
        dk, _, P = load_deck(deck)
        plan = engine.Plan(P, mode="fast")
        zD = engine.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd) / plan.derived.Lc
        h, dh = plan.drawdown_grid(tD, plan.split_vector(tD), rD, zD, plan.zlay(zD))
        plan.close()
        assert h.shape == (len(tD), len(rD), len(zD))
        got[tag] = (h.ravel().copy(), dh.ravel().copy(), len(zD))
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def results():
    cases = build_cases()
    return cases, run_cases(cases)


def test_cases_cover_every_parity_of_the_paired_loops(results):
    cases, got = results
    tags = [c[0] for c in cases]
    assert len(set(tags)) == len(tags)
    assert [steps_by_width(M) for M in MS] == [(0, 0, 0), (0, 0, 1), (0, 1, 7), (1, 8, 7), (8, 8, 7), (14, 8, 7)]
    for M in MS:
        for n in FILLS:
            assert got[f"fill_M{M}_nt{n}"][0].shape == (n,)
        assert sum(t.startswith(f"dip_M{M}_") for t in tags) == 12
        assert sum(t.startswith(f"zero_M{M}_") for t in tags) == 4 and sum(t.startswith(f"nan_M{M}_") for t in tags) == 4
        for k in range(4):
            for kind in ("dipa", "dipb", "plain"):
                assert f"alone_M{M}_{kind}{k}" in got
    assert got["grid_c2"][2] == 1 and got["grid_c3"][2] == 2       # depths: C3 runs the kernel's depth loop


def test_every_bit_of_the_parent(results):
    cases, got = results
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    names = [c[0] for c in cases] + [g[0] for g in GRIDS]
    assert [str(s) for s in want["tags"]] == names
    assert str(want["inputs_sha256"]) == inputs_digest(cases), "this machine built other input bits than the fixture's"
    off = want["offsets"]
    bad = []
    for k, tag in enumerate(names):
        for name, a in zip(("h", "dh"), got[tag][:2]):
            ref = want[name][off[k]:off[k + 1]]
            assert a.shape == ref.shape and a.dtype == ref.dtype == np.float64, tag
            diff = np.flatnonzero(_bits(a) != _bits(ref))
            if diff.size:
                bad.append((tag, name, diff.tolist(), a[diff].tolist(), ref[diff].tolist()))
    print(f"{len(bad)} of {2 * len(names)} vectors of results differ from the parent in a bit")
    assert not bad, bad[:6]
    # the fixture's content: a zero vector gives exactly 0, the others do not; a NaN sample leaves the neighbours finite
    for M in MS:
        for k in range(4):
            h, dh = got[f"zero_M{M}_p{k}"]
            assert h[k] == 0.0 and dh[k] == 0.0 and np.all(np.delete(h, k) != 0.0) and np.all(np.isfinite(np.delete(h, k)))
            assert np.all(np.isfinite(np.delete(got[f"nan_M{M}_p{k}"][0], k)))
    for tag in ("grid_c2", "grid_c3"):
        assert np.all(np.isfinite(got[tag][0])) and np.all(np.isfinite(got[tag][1])) and np.any(got[tag][0] != 0.0)


def test_a_vector_does_not_see_its_neighbours(results):
    """independent of the parent: in a tile with vectors that take the scaled quotient every vector gives the bits it gives
    alone, and a longer call repeats the shorter one"""
    cases, got = results
    for M in MS:
        for i, j in PAIRS:
            h, dh = got[f"dip_M{M}_{i}{j}"]
            for k in range(4):
                who = "dipa" if k == i else "dipb" if k == j else "plain"
                h1, dh1 = got[f"alone_M{M}_{who}{k}"]
                assert _bits(h)[k] == _bits(h1)[0] and _bits(dh)[k] == _bits(dh1)[0], (M, i, j, k, h[k], h1[0], dh[k], dh1[0])
        full = got[f"fill_M{M}_nt7"]
        for n in FILLS:
            part = got[f"fill_M{M}_nt{n}"]
            assert np.array_equal(_bits(part[0]), _bits(full[0])[:n]) and np.array_equal(_bits(part[1]), _bits(full[1])[:n]), (M, n)
        for k in range(4):
            assert _bits(got[f"alone_M{M}_plain{k}"][0])[0] == _bits(full[0])[k]
