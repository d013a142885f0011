"""The packed quotient-difference rhombus of dehoog_tiles_kernel (fast flavour), bit for bit against the parent.

dehoog_tiles_kernel<TU, false> inverts a tile of 4 times = 8 vectors (h and dh of each time) per wave.  The parent ran the
M steps of each vector's rhombus one vector per wave pass; the packed code lets a vector live in the narrowest group of
lanes (64, 32 or 16) that holds its 2(M - r) + 1 live entries at step r and runs two or four vectors in one pass.  Per
lane not one operation changed, so h and dh must be the SAME BITS as before: tests/golden/dehoog_packed_parent.npz holds
what the parent build (commit and build id inside the file) gave on an MI355X for the calls below through
ucf_debug_dehoog_tiles, which launches the kernel itself; tools/gen_dehoog_packed_fixture.py wrote it.

Inputs: seeded synthetic vectors F(p_m) = sum_k a_k / (p_m + b_k), p_m = c / T + i pi m / T, T = 2 t, three real poles per
vector: smooth, decaying, complex.  They are made of single IEEE operations on binary64 arrays (no library function), so
that every machine builds the same bits; the fixture keeps their SHA-256 and the test checks it first.

Cases (every one in the fast flavour):
  fill_M{M}_nt{n}      M in 26 31 16 15 8 7 3 (np = 63 fills the wave; 16 / 15 and 8 / 7 straddle the switch to half- and
                       quarter-wave groups; 3 is packed from the first step) x n in 1 2 3 4 5 7 times (empty groups, odd
                       quads, a partial last tile): the first n of the 7 vectors of that M
  zero_M{M}_p{k}       4 times, the vector of time k all zeros (k = 0..3); 7 times with time 5 zero (p5)
  nan_M{M}_p{k}        4 times, the vector of time k with a NaN in one sample (sample 1 / M / 2M / 0, real or imaginary part)
  scale_M{M}_{i}{j}    4 times, vector i scaled by 1e160 and vector j by 1e-160, every ordered pair i != j
  dip_M{M}_{i}{j}      4 times, vector i with sample M scaled by 1e-155 and vector j with sample 2M scaled by 1e-155
  alone_M{M}_{kind}{k} one time: every vector of the scale and dip tiles on its own

Why the dip cases: q(i,1) = f(i+1) / f(i) does not see a factor common to the whole vector, so a scaled vector runs the
same rhombus as the plain one and never leaves the unscaled quotient of qd_quotient.  One sample 1e155 times smaller than
its neighbours gives q = O(1e155) and e beyond the 1e150 guard: that vector, and only that one, takes cdiv.  Sample 2M sits
on the right edge of the rhombus at every step, so the guard fires in the solo, the paired and the four-fold steps.

Beside the fixture two properties are asserted that do not depend on the parent: a vector's h and dh in a scale or dip
tile are the bits it gives alone, and the first times of a fill case are the bits of the shorter fill cases."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dehoog_packed_parent.npz")
MS = (26, 31, 16, 15, 8, 7, 3)
FILLS = (1, 2, 3, 4, 5, 7)
ALPHA, TOL = 1e-8, 1e-9
NVEC = 7
PAIRS = tuple((i, j) for i in range(4) for j in range(4) if i != j)


def vectors(M):
    """t [NVEC], fp [NVEC, 2M+1, 2]: single IEEE operations only"""
    rng = np.random.Generator(np.random.PCG64(1000 + M))
    u = rng.integers(1, 1 << 20, size=(NVEC, 7)).astype(np.float64) / float(1 << 20)       # exact dyadic rationals in (0, 1)
    t = 0.25 + 8.0 * u[:, 0]
    T = 2.0 * t
    m = np.arange(2 * M + 1, dtype=np.float64)
    x0 = 10.36 / T
    y = (np.pi * m)[None, :] / T[:, None]
    re = np.zeros((NVEC, 2 * M + 1))
    im = np.zeros((NVEC, 2 * M + 1))
    for k in range(3):
        a = 0.5 + u[:, 1 + 2 * k]
        b = 0.125 + 4.0 * u[:, 2 + 2 * k]
        x = (x0 + b)[:, None] + 0.0 * y
        d = x * x + y * y
        re = re + a[:, None] * (x / d)
        im = im - a[:, None] * (y / d)
    return t, np.ascontiguousarray(np.stack([re, im], axis=2))


def build_cases():
    """[(tag, M, t, fp)] in a fixed order"""
    cases = []
    for M in MS:
        t, fp = vectors(M)
        for n in FILLS:
            cases.append((f"fill_M{M}_nt{n}", M, t[:n].copy(), fp[:n].copy()))
        for k in (0, 1, 2, 3, 5):
            n = 7 if k == 5 else 4
            f = fp[:n].copy()
            f[k] = 0.0
            cases.append((f"zero_M{M}_p{k}", M, t[:n].copy(), f))
        for k in range(4):
            f = fp[:4].copy()
            f[k, (1, M, 2 * M, 0)[k], k & 1] = np.nan
            cases.append((f"nan_M{M}_p{k}", M, t[:4].copy(), f))
        for kind, i, j, f in special_tiles(M, fp):
            cases.append((f"{kind}_M{M}_{i}{j}", M, t[:4].copy(), f))
            for k in (i, j):
                tag = f"alone_M{M}_{kind}{'ab'[k == j]}{k}"
                if all(c[0] != tag for c in cases):
                    cases.append((tag, M, t[k:k + 1].copy(), f[k:k + 1].copy()))
        for k in range(4):
            cases.append((f"alone_M{M}_plain{k}", M, t[k:k + 1].copy(), fp[k:k + 1].copy()))
    return cases


def special_tiles(M, fp):
    for i, j in PAIRS:
        f = fp[:4].copy()
        f[i] = f[i] * 1e160
        f[j] = f[j] * 1e-160
        yield "scale", i, j, f
    for i, j in PAIRS:
        f = fp[:4].copy()
        f[i, M] = f[i, M] * 1e-155
        f[j, 2 * M] = f[j, 2 * M] * 1e-155
        yield "dip", i, j, f


def inputs_digest(cases):
    s = hashlib.sha256()
    for tag, M, t, fp in cases:
        s.update(tag.encode()); s.update(t.tobytes()); s.update(fp.tobytes())
    return s.hexdigest()


def run_cases(cases):
    """{tag: (h, dh)} from the library that is loaded"""
    from unconfined_amd import engine
    return {tag: engine.debug_dehoog_tiles(M, ALPHA, TOL, t, fp, "fast") for tag, M, t, fp in cases}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def results():
    cases = build_cases()
    return cases, run_cases(cases)


def test_cases_are_the_ones_the_issue_lists(results):
    cases, got = results
    tags = [c[0] for c in cases]
    assert len(set(tags)) == len(tags) == len(got)
    for M in MS:
        for n in FILLS:
            assert got[f"fill_M{M}_nt{n}"][0].shape == (n,)
        assert sum(t.startswith(f"scale_M{M}_") for t in tags) == 12 and sum(t.startswith(f"dip_M{M}_") for t in tags) == 12
        assert sum(t.startswith(f"zero_M{M}_") for t in tags) == 5 and sum(t.startswith(f"nan_M{M}_") for t in tags) == 4
        for k in range(4):
            for kind in ("scalea", "scaleb", "dipa", "dipb", "plain"):
                assert f"alone_M{M}_{kind}{k}" in got


def test_packed_rhombus_keeps_every_bit_of_the_parent(results):
    cases, got = results
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    assert [str(s) for s in want["tags"]] == [c[0] for c in cases]
    assert str(want["inputs_sha256"]) == inputs_digest(cases), "this machine built other input bits than the fixture's"
    off = want["offsets"]
    bad = []
    for k, (tag, M, t, fp) in enumerate(cases):
        for name, a in zip(("h", "dh"), got[tag]):
            ref = want[name][off[k]:off[k + 1]]
            assert a.shape == ref.shape == t.shape and a.dtype == ref.dtype == np.float64
            diff = np.flatnonzero(_bits(a) != _bits(ref))
            if diff.size:
                bad.append((tag, name, diff.tolist(), a[diff].tolist(), ref[diff].tolist()))
    print(f"{len(bad)} of {2 * len(cases)} vectors of results differ from the parent in a bit")
    assert not bad, bad[:6]
    # the fixture's content: a zero vector gives exactly 0, the others do not; NaN samples and dips leave the neighbours finite
    for M in MS:
        for k in (0, 1, 2, 3, 5):
            h, dh = got[f"zero_M{M}_p{k}"]
            assert h[k] == 0.0 and dh[k] == 0.0 and np.all(np.delete(h, k) != 0.0) and np.all(np.isfinite(np.delete(h, k)))
        for k in range(4):
            assert np.all(np.isfinite(np.delete(got[f"nan_M{M}_p{k}"][0], k)))


def test_a_vector_does_not_see_its_neighbours(results):
    """independent of the parent: packed with scaled vectors or with vectors that take cdiv, every vector gives the bits it
    gives alone, and a longer call repeats the shorter one"""
    cases, got = results
    for M in MS:
        for kind in ("scale", "dip"):
            for i, j in PAIRS:
                h, dh = got[f"{kind}_M{M}_{i}{j}"]
                for k in range(4):
                    who = f"{kind}a" if k == i else f"{kind}b" if k == j else "plain"
                    h1, dh1 = got[f"alone_M{M}_{who}{k}"]
                    assert _bits(h)[k] == _bits(h1)[0] and _bits(dh)[k] == _bits(dh1)[0], (M, kind, i, j, k, h[k], h1[0], dh[k], dh1[0])
        full = got[f"fill_M{M}_nt7"]
        for n in FILLS:
            part = got[f"fill_M{M}_nt{n}"]
            assert np.array_equal(_bits(part[0]), _bits(full[0])[:n]) and np.array_equal(_bits(part[1]), _bits(full[1])[:n]), (M, n)
        for k in range(4):
            assert _bits(got[f"alone_M{M}_plain{k}"][0])[0] == _bits(full[0])[k]
