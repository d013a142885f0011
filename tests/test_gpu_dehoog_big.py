"""The de Hoog inversion with more Laplace samples than a wave has lanes (M > 31, 2M+1 > 64), held to the oracle.

Such a plan runs code that no plan with M <= 31 reaches: dehoog_sets<2> / dehoog_sets<4> (element i = lane + 64 g in register
set g, lane 63 of a set taking its neighbour from lane 0 of the next: shift_down_sets), dehoog_big (h, and dh through p F(p)),
dehoog_tiles_kernel<1, true> after every grid, the chunked transform (lane layout 2: work item = point x 64-sample chunk) and
dehoog_points_kernel after every point list, and the faithful dehoog_kernel behind ucf_dehoog.

1. The kernels on synthetic transforms, through ucf_debug_dehoog_tiles and ucf_dehoog.  Seven seeded vectors per M -- sums of
   three real poles made of single IEEE operations, at the p the kernel assumes (oracle.pvalues(2 t, M, alpha, tol)) -- for
   M = 32 33 40 63 (two register sets; 65 samples: element 64 alone in set 1; 127: the largest odd fill), 64 65 95 96 127 (four
   sets; 129 / 193: elements 128 / 192 alone in sets 2 / 3; 255: the maximum), in fills of 1 2 3 4 5 7 vectors (a tile of four,
   a ragged last tile, several workgroups), both flavours.  Reference per vector and channel: d = oracle.dehoog in binary64,
   q = the same in binary128; for dh both on the samples times p (the product in numpy complex128), times t.  The bar is the
   rule of tests/test_gpu_stages_families.py with its constants imported (F, ARBITRATION, K of the totlap stage):

       err_d <= K max(F, spread)                                     or
       refq <= 4 max(F, spread)  and  err_q <= K max(F, refq)

   err_d, err_q = the device's distances from d and q, refq = |d - q|, spread = the largest change of d under eight seeded
   perturbations of every sample component by -1, 0 or +1 ulp; all relative to max(|q|, 1e-3).  Every vector of every case is
   judged.  The faithful flavour's h has the bits of ucf_dehoog on the same vector.  Edges (tiles of four, M = 32 64 96 127): a
   zero vector gives exactly 0 and leaves its neighbours alone; a NaN in one sample on either side of every set boundary and
   on the right edge of the rhombus does what it does in the oracle, which scrubs it to 0 and leaves it out of the largest
   modulus: as the last sample (never a divisor) it gives a finite value, held to the rule; anywhere else the zero divides its
   right neighbour and binary64 and binary128 both end in NaN, and so must the device, with the neighbours in the tile keeping
   their bits; vectors scaled by 1e160 and 1e-160 are held to the oracle on the scaled input, relative to |q| with no floor.
   Without a reference: a vector in a tile gives the bits it gives alone, a shorter fill is the head of the longer one, a
   repeated call gives the same bytes.  (What the values can and cannot see: once the continued fraction has converged its
   last coefficients carry no weight, so a wrong neighbour in the last few elements -- the set boundary at M = 32 ... 40 --
   moves h and dh by less than one ulp in a sample does, here and in any transform this smooth; from M = 63 on the boundaries
   lie inside the rhombus and a wrong neighbour moves the values by up to 25 times the rule.  At M = 32 it is the NaN at
   sample 63 that tells: the device must end in NaN as the oracle does.)  Fixtures of stages_generic.npz that test_gpu_stages.py::test_dehoog_tiled_kernel
   skips for 2M+1 > 64 are held to that test's own bars (the file holds none today: its largest M is 26).

2. Whole calls with M = 32 and 64 (two and four register sets) on four decks, both flavours: the 12 points of a 6 x 2 grid
   (6 times 10 ** linspace(-1, 3, 6), rD 0.1 and 3.0) through the grid entry, as a list of 12 points and as a list of 384
   points (the 12 repeated cyclically), against tests/golden/dehoog_big_<deck>.npz (oracle/gen_dehoog_big.py: ucfo_batch in
   binary64, and its distance from binary128 as noise) under gate() of tests/test_gpu_fit.py; every repeat of a point has the
   bits of its first occurrence.  The grid entry gets the 6 times repeated cyclically to 46 (eleven tiles of four and a
   ragged one of two): a grid of 6 times runs the chunked layout like a list, lane = time needs 33 times or more at M = 32 and
   44 or more at M = 64 (grid_lane_time).  Two of the times are others for one deck each: there one ulp in tD moves the binary64 oracle's own dh at
   M = 64 by three times what the gate allows the device (gen.REPLACED; the faithful flavour missed the gate at the first of
   them by 3.9, in all three entries alike, where the oracle's own neighbour misses it by 3.2).  test_fixture_* check the
   files without a GPU, and that the reference is sharp enough for its gate everywhere.

   Which kernels ran: a child process with UCF_TRACE_LAUNCHES=1 names them.  The grid entry ends in
   dehoog_tiles_kernel<1, true>.  Both lists run the chunked transform (template argument LAYOUT = 2), whose only launcher,
   launch_points_chunked, launches dehoog_points_kernel right after it (that launch carries no name in the trace).  NO size of
   a point list reaches dehoog_tiles_kernel<3, true>: launch_points_any (ucf_drawdown.cpp) takes the lane = point layout only
   for plans with 2M+1 <= 64, and launch_points_lanes refuses the others, so that instantiation is never launched; the test
   asserts what a long list does run.

   ucf_debug_stages refuses lane layout 2 ("no stage hook for the chunked layout"), so the transform of the short list is not
   looked at apart from the inversion here.

The share of the rule (1) and of the gate (2) that every M / flavour / channel used goes to dehoog_big.json in the log folder
of the tools (tools_out/ or $UCF_TOOLS_OUT; tools/collect_profiles.py copies it to profiles/); 1.0 = exhausted."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLD
from test_gpu_fit import gate
from test_midstages_families import ARBITRATION, F, K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_dehoog_big as gen  # noqa: E402

gpu = pytest.mark.gpu

MODES = ("faithful", "fast")
MS = (32, 33, 40, 63, 64, 65, 95, 96, 127)
EDGE_MS = (32, 64, 96, 127)
FILLS = (1, 2, 3, 4, 5, 7)
NVEC = 7
ALPHA, TOL = 1e-8, 1e-9
NDRAWS, SPREAD_SEED = 8, 20261021
FLOOR = 1e-3
REPORT = {"hook": {}, "edges": {}, "whole": {}, "skipped_fixtures": {}}


def _cplx(a):
    return a[..., 0] + 1j * a[..., 1]


def _pairs(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- 1. inputs and reference
def vectors(oracle, M):
    """t [NVEC], fp [NVEC, 2M+1, 2], p [NVEC, 2M+1] complex: F(p) = sum of three real poles a / (p + b) at the kernel's own
    p = sigma + i pi m / (2 t), from single IEEE operations on binary64 arrays"""
    rng = np.random.Generator(np.random.PCG64(1000 + M))
    u = rng.integers(1, 1 << 20, size=(NVEC, 7)).astype(np.float64) / float(1 << 20)       # exact dyadic rationals in (0, 1)
    t = 0.25 + 8.0 * u[:, 0]
    pv = np.stack([oracle.pvalues(2.0 * tt, M, ALPHA, TOL) for tt in t])                   # [NVEC, np, 2]
    re = np.zeros((NVEC, 2 * M + 1))
    im = np.zeros((NVEC, 2 * M + 1))
    y = pv[:, :, 1]
    for k in range(3):
        a = 0.5 + u[:, 1 + 2 * k]
        b = 0.125 + 4.0 * u[:, 2 + 2 * k]
        x = pv[:, :, 0] + b[:, None]
        d = x * x + y * y
        re = re + a[:, None] * (x / d)
        im = im - a[:, None] * (y / d)
    return t, np.ascontiguousarray(np.stack([re, im], axis=2)), _cplx(pv)


def _channel(lib, M, t, f, p, ch):
    """the oracle `lib` on one vector f [np, 2]: h, or dh = t x the inversion of p F(p)"""
    t = float(t)
    with np.errstate(all="ignore"):
        if ch == "h":
            return lib.dehoog(M, ALPHA, TOL, t, 2.0 * t, f)
        return lib.dehoog(M, ALPHA, TOL, t, 2.0 * t, _pairs(_cplx(f) * p)) * t


def _draws(f, key):
    """NDRAWS copies of f with every component moved by -1, 0 or +1 ulp, seeded by `key`"""
    rng = np.random.default_rng([SPREAD_SEED, *key])
    for _ in range(NDRAWS):
        s = rng.integers(-1, 2, size=f.shape)
        yield np.where(s > 0, np.nextafter(f, np.inf), np.where(s < 0, np.nextafter(f, -np.inf), f))


_REF = {}


def reference(oracle, oracle_quad, M, t, f, p, key):
    """{"h" | "dh": (d, q, spread)} of one vector: spread is absolute here, judge() makes it relative"""
    if key not in _REF:
        out = {}
        pert = list(_draws(f, key))
        for ch in ("h", "dh"):
            d = _channel(oracle, M, t, f, p, ch)
            q = _channel(oracle_quad, M, t, f, p, ch)
            spread = max(abs(_channel(oracle, M, t, g, p, ch) - d) for g in pert)
            out[ch] = (d, q, spread)
        _REF[key] = out
    return _REF[key]


def judge(dev, ref, mode, floor=FLOOR):
    """(passes, share of the rule used, figures) of one device value against (d, q, spread)"""
    d, q, spread = ref
    kk = K[mode]["totlap"]
    scale = max(abs(q), floor)
    err_d, err_q, refq = abs(dev - d) / scale, abs(dev - q) / scale, abs(d - q) / scale
    n = max(F, spread / scale)
    share = err_d / (kk * n)
    if refq <= ARBITRATION * n:
        share = min(share, err_q / (kk * max(F, refq)))
    ok = bool(np.isfinite(dev) and np.isfinite(d) and np.isfinite(q) and share <= 1.0)
    return ok, float(share), dict(dev=float(dev), d=float(d), q=float(q), err_d=float(err_d), err_q=float(err_q),
                                  spread=float(spread / scale), refq=float(refq), K=kk)


def _note(section, key, ch, share, figs):
    ent = REPORT[section].setdefault(key, {}).setdefault(ch, {"rule": 0.0, "worst": None})
    if not share <= ent["rule"]:
        ent["rule"], ent["worst"] = share, figs


@pytest.fixture(scope="module")
def engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine as e
    return e


@pytest.fixture(scope="module")
def inputs(oracle):
    return {M: vectors(oracle, M) for M in MS}


@pytest.fixture(scope="module")
def hook(engine, inputs):
    """{(M, mode, tag): (h, dh)} of every fill and of every vector alone, one launch each"""
    got = {}
    for M in MS:
        t, fp, p = inputs[M]
        for mode in MODES:
            for n in FILLS:
                got[M, mode, f"fill{n}"] = engine.debug_dehoog_tiles(M, ALPHA, TOL, t[:n], fp[:n], mode)
            got[M, mode, "again"] = engine.debug_dehoog_tiles(M, ALPHA, TOL, t, fp, mode)
            for k in range(NVEC):
                got[M, mode, f"alone{k}"] = engine.debug_dehoog_tiles(M, ALPHA, TOL, t[k:k + 1], fp[k:k + 1], mode)
    return got


# ---------------------------------------------------------------------------------------------- 1. the kernels
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", MS)
def test_every_vector_of_every_fill_against_the_oracle(hook, inputs, oracle, oracle_quad, M, mode):
    t, fp, p = inputs[M]
    failures = []
    for n in FILLS:
        res = hook[M, mode, f"fill{n}"]
        assert res[0].shape == res[1].shape == (n,)
        for k in range(n):
            ref = reference(oracle, oracle_quad, M, t[k], fp[k], p[k], (M, k))
            for ch, a in zip(("h", "dh"), res):
                ok, share, figs = judge(a[k], ref[ch], mode)
                print(f"M {M} {mode} fill {n} vector {k} {ch}: share {share:.3f} err_d {figs['err_d']:.2e} err_q {figs['err_q']:.2e} "
                      f"spread {figs['spread']:.2e} refq {figs['refq']:.2e}")
                _note("hook", f"M{M}/{mode}", ch, share, dict(figs, fill=n, vector=k))
                if not ok:
                    failures.append((n, k, ch, share, figs))
    assert not failures, failures[:4]


@gpu
@pytest.mark.parametrize("M", MS)
def test_faithful_h_has_the_bits_of_ucf_dehoog(engine, hook, inputs, M):
    """dehoog_big repeats the arithmetic of the faithful dehoog_kernel (dehoog_sets<2> / <4> in both)"""
    t, fp, p = inputs[M]
    hw = engine.dehoog(M, ALPHA, TOL, t, 2.0 * t, fp)
    h = hook[M, "faithful", "fill7"][0]
    assert np.array_equal(_bits(h), _bits(hw)), (M, h, hw)
    one = np.array([engine.dehoog(M, ALPHA, TOL, t[k], 2.0 * t[k], fp[k][None])[0] for k in (0, NVEC - 1)])
    assert np.array_equal(_bits(one), _bits(hw[[0, NVEC - 1]]))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", MS)
def test_a_vector_does_not_see_its_neighbours_or_the_fill(hook, M, mode):
    full = hook[M, mode, "fill7"]
    for n in FILLS:
        part = hook[M, mode, f"fill{n}"]
        for a, b in zip(part, full):
            assert np.array_equal(_bits(a), _bits(b)[:n]), (M, mode, n)
    for k in range(NVEC):
        for a, b in zip(hook[M, mode, f"alone{k}"], full):
            assert _bits(a)[0] == _bits(b)[k], (M, mode, k, a[0], b[k])
    for a, b in zip(hook[M, mode, "again"], full):
        assert a.tobytes() == b.tobytes(), (M, mode)
    assert np.isfinite(full[0]).all() and np.isfinite(full[1]).all() and (full[0] != 0.0).all() and (full[1] != 0.0).all()


def nan_places(M):
    """[(sample index, 0 real | 1 imaginary)]: both sides of every set boundary that exists, and the right edge of the rhombus"""
    idx = [i for i in (0, 63, 64, 127, 128, 191, 192) if i <= 2 * M]
    idx += [i for i in (2 * M - 1, 2 * M) if i not in idx]
    return [(i, j & 1) for j, i in enumerate(idx)]


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", EDGE_MS)
def test_edges_in_tiles_of_four(engine, hook, inputs, oracle, oracle_quad, M, mode):
    t, fp, p = inputs[M]
    alone = [tuple(a[0] for a in hook[M, mode, f"alone{k}"]) for k in range(4)]
    failures = []

    def neighbours_keep_their_bits(res, but, what):
        for k in range(4):
            if k not in but:
                assert _bits(res[0])[k] == _bits(alone[k][0])[0] and _bits(res[1])[k] == _bits(alone[k][1])[0], (M, mode, what, k)
                assert np.isfinite(res[0][k]) and res[0][k] != 0.0 and np.isfinite(res[1][k]) and res[1][k] != 0.0

    nan_results = []

    def held(res, k, f, key, what, floor, nan_ok=False):
        ref = reference(oracle, oracle_quad, M, t[k], f[k], p[k], key)
        for ch, a in zip(("h", "dh"), res):
            if np.isnan(ref[ch][0]) and np.isnan(ref[ch][1]):
                # a sample scrubbed to 0 divides its right neighbour (q = f(i+1) / f(i)): NaN in binary64 and binary128 alike
                assert nan_ok and np.isnan(a[k]), (M, mode, what, k, ch, a[k])
                nan_results.append(what)
                continue
            ok, share, figs = judge(a[k], ref[ch], mode, floor)
            print(f"M {M} {mode} {what} vector {k} {ch}: share {share:.3f} dev {figs['dev']:.6e} d {figs['d']:.6e} err_d {figs['err_d']:.2e} "
                  f"err_q {figs['err_q']:.2e} spread {figs['spread']:.2e} refq {figs['refq']:.2e}")
            _note("edges", f"M{M}/{mode}/{what.split('_')[0]}", ch, share, dict(figs, case=what, vector=k))
            if not ok:
                failures.append((what, k, ch, share, figs))

    # one vector all zeros: exactly 0.0 in both channels
    for k in range(4):
        f = fp[:4].copy()
        f[k] = 0.0
        res = engine.debug_dehoog_tiles(M, ALPHA, TOL, t[:4], f, mode)
        assert res[0][k] == 0.0 and res[1][k] == 0.0, (M, mode, k, res)
        neighbours_keep_their_bits(res, (k,), f"zero{k}")
    # one NaN sample: scrubbed to 0 and left out of the largest modulus, as the oracle does
    for j, (i, part) in enumerate(nan_places(M)):
        k = j % 4
        f = fp[:4].copy()
        f[k, i, part] = np.nan
        res = engine.debug_dehoog_tiles(M, ALPHA, TOL, t[:4], f, mode)
        neighbours_keep_their_bits(res, (k,), f"nan{i}")
        held(res, k, f, (M, k, 1000 + i, part), f"nan_sample{i}_{'ri'[part]}", FLOOR, nan_ok=i != 2 * M)
    # (the last sample is never a divisor: that case, element 64 / 128 / 192 alone in its set for M = 32 / 64 / 96, is finite
    #  and went through the rule; every other place gives NaN in both channels)
    assert len(nan_results) == 2 * (len(nan_places(M)) - 1), nan_results
    # scaled vectors: relative to |q|, no floor
    for i, j in ((0, 1), (3, 2)):
        f = fp[:4].copy()
        f[i] = f[i] * 1e160
        f[j] = f[j] * 1e-160
        res = engine.debug_dehoog_tiles(M, ALPHA, TOL, t[:4], f, mode)
        neighbours_keep_their_bits(res, (i, j), f"scale{i}{j}")
        held(res, i, f, (M, i, 2000), f"scale_up_v{i}", 0.0)
        held(res, j, f, (M, j, 3000), f"scale_down_v{j}", 0.0)
    assert not failures, failures[:4]


SKIPPED_BARS = (("faithful", 1e-13), ("fast", 5e-12))          # those of test_gpu_stages.py::test_dehoog_tiled_kernel


def skipped_fixtures():
    """the de Hoog fixtures of stages_generic.npz with T = 2 t and 2M+1 > 64: [(i, M, alpha, tol, t, fp, ref)]"""
    z = np.load(os.path.join(GOLD, "stages_generic.npz"))
    out = []
    for i in range(int(z["counts"][2])):
        M, alpha, tol, t, tee = z[f"dehoog_par_{i}"]
        if abs(tee - 2.0 * t) <= 1e-15 * tee and 2 * int(M) + 1 > 64:
            out.append((i, int(M), float(alpha), float(tol), float(t), z[f"dehoog_fp_{i}"], float(z[f"dehoog_out_{i}"][0])))
    return out


@gpu
def test_fixtures_that_the_stage_test_skips(engine):
    """the reference's own de Hoog fixtures with 2M+1 > 64, under the bars the stage test holds the others to"""
    fx = skipped_fixtures()
    for i, M, alpha, tol, t, fp, ref in fx:
        for mode, bar in SKIPPED_BARS:
            h, dh = engine.debug_dehoog_tiles(M, alpha, tol, [t], fp[None], mode)
            err = None
            if np.isnan(ref):
                assert np.isnan(h[0]), (i, mode, h[0])
            elif ref == 0.0:
                assert h[0] == 0.0, (i, mode, h[0])
            else:
                err = abs(h[0] - ref) / abs(ref)
                print(f"fixture {i} M {M} {mode}: h {h[0]:.17g} ref {ref:.17g} err {err:.2e} bar {bar:.0e}")
                assert err <= bar, (i, M, mode, h[0], ref, err)
            REPORT["skipped_fixtures"][f"{i}/M{M}/{mode}"] = {"err": err, "bar": bar}
    REPORT["skipped_fixtures"]["count"] = len(fx)


# ---------------------------------------------------------------------------------------------- 2. whole calls
ENTRIES = ("grid46x2", "list12", "list384")
# the grid entry takes lane = time, and with it dehoog_tiles_kernel<1, true>, only where the times fill their waves better than
# the samples fill theirs (grid_lane_time, ucf_drawdown.cpp): nt / 64 > 65 / 128 for M = 32 and > 129 / 192 for M = 64, that is
# 33 and 44 times or more.  A 6 x 2 grid runs the chunked layout like a list.  So the six times are repeated cyclically to 46:
# eleven tiles of four and a ragged one of two
NGRID, NLONG = 46, 384
TRANSFORM = re.compile(r"(integrate_kernel|integrate_generic_kernel|point_kernel)<(\d+), (\d+)")


def run_entries(plan, tD, rD, sv, zD, zl):
    """{entry: (h, dh) [points, nz]} of the 12 points, repeated cyclically, through the three entries (point = it * 2 + ir)"""
    tl, rl, sl = gen.points(tD, rD, sv)
    idx = np.arange(NLONG) % len(tl)
    it = np.arange(NGRID) % len(tD)
    out = {}
    h, dh = plan.drawdown_grid(tD[it], sv[it], rD, zD, zl)
    out["grid46x2"] = (h.reshape(NGRID * len(rD), -1), dh.reshape(NGRID * len(rD), -1))
    out["list12"] = plan.drawdown(tl, rl, sl, zD, zl)
    out["list384"] = plan.drawdown(tl[idx], rl[idx], sl[idx], zD, zl)
    return out


def fixture_of(name):
    return np.load(gen.path_of(name))


def test_fixture_inputs_follow_from_the_deck_bit_for_bit(oracle):
    for name in gen.DECKS:
        z = fixture_of(name)
        dk, tD, rD, sv, zD, zl = gen.inputs(oracle, name)
        nz = 1 if dk.piezometer else min(gen.NZ, dk.zOrd)
        kinds = ("ref_h", "ref_dh", "noise_h", "noise_dh", "spread_h", "spread_dh")
        assert set(z.files) == {"tD", "rD", "sv", "zD", "zl"} | {f"{key}_M{M}" for key in kinds for M in gen.MS}, name
        for key, a in (("tD", tD), ("rD", rD), ("sv", sv), ("zD", zD), ("zl", zl)):
            assert z[key].dtype == a.dtype and z[key].tobytes() == a.tobytes(), (name, key)
        assert len(tD) == gen.NT == 6 and tuple(rD) == (0.1, 3.0) and len(zD) == nz
        # 10 ** linspace(-1, 3, 6) but for the replaced times, which stay inside the span and in order
        usual = 10.0 ** oracle.linspace(-1.0, 3.0, 6)
        other = sorted(gen.REPLACED.get(name, {}))
        assert len(other) <= 1 and np.array_equal(np.delete(tD, other), np.delete(usual, other)) and (np.diff(tD) > 0).all()
        assert len(set(zip(*gen.points(tD, rD, sv)[:2]))) == 12
        for M in gen.MS:
            assert 2 * gen.params(dk, M).M + 1 > 64
            for key in kinds:
                assert z[f"{key}_M{M}"].shape == (12, nz) and z[f"{key}_M{M}"].dtype == np.float64
                # finite everywhere: no point has to be left out
                assert np.isfinite(z[f"{key}_M{M}"]).all(), (name, M, key)
            for ch in ("h", "dh"):
                # the reference is sharp enough for its gate: one ulp in an input moves it by less than the gate allows the device
                # (both relative to max(|ref|, 1e-3)), and the gate is far below the O(1) of an indexing error
                rel_gate = gate(z[f"ref_{ch}_M{M}"], z[f"noise_{ch}_M{M}"]) / np.maximum(np.abs(z[f"ref_{ch}_M{M}"]), 1e-3)
                assert (z[f"spread_{ch}_M{M}"] <= rel_gate).all(), (name, M, ch, float((z[f"spread_{ch}_M{M}"] / rel_gate).max()))
                assert rel_gate.max() <= 1e-7, (name, M, ch)
        assert os.path.getsize(gen.path_of(name)) <= 8192, name
    assert sorted(gen.REPLACED) == ["c2_neuman74_fullpen", "c3_moench"]


def test_fixture_reference_is_what_the_oracle_built_here_gives(oracle):
    for name in gen.DECKS:
        z = fixture_of(name)
        dk = gen.inputs(oracle, name)[0]
        for M in gen.MS:
            h, dh = gen.reference(oracle, dk, M, z["tD"], z["rD"], z["sv"], z["zD"], z["zl"])
            assert h.tobytes() == z[f"ref_h_M{M}"].tobytes() and dh.tobytes() == z[f"ref_dh_M{M}"].tobytes(), (name, M)
        if name in gen.REPLACED:                # (and the spread, where a time was chosen by it)
            M = gen.MS[-1]
            sh, sd = gen.spread(oracle, dk, M, z["tD"], z["rD"], z["sv"], z["zD"], z["zl"])
            assert sh.tobytes() == z[f"spread_h_M{M}"].tobytes() and sd.tobytes() == z[f"spread_dh_M{M}"].tobytes(), name


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M", gen.MS)
@pytest.mark.parametrize("name", gen.DECKS)
def test_whole_calls_against_the_oracle(engine, oracle, name, M, mode):
    z = fixture_of(name)
    dk = gen.inputs(oracle, name)[0]
    plan = engine.Plan(gen.params(dk, M), mode=mode)
    assert plan.derived.np == 2 * M + 1
    got = run_entries(plan, z["tD"], z["rD"], z["sv"], z["zD"], z["zl"])
    plan.close()
    failures = []
    for entry in ENTRIES:
        h, dh = got[entry]
        assert len(h) == len(dh) == {"grid46x2": 2 * NGRID, "list12": 12, "list384": NLONG}[entry]
        for a in (h, dh):                                   # every repeat of a point has the bits of its first occurrence
            assert np.array_equal(_bits(a), _bits(a[np.arange(len(a)) % 12])), (name, M, mode, entry, "repeats")
        for ch, a in (("h", h[:12]), ("dh", dh[:12])):
            ref, noise = z[f"ref_{ch}_M{M}"], z[f"noise_{ch}_M{M}"]
            assert a.shape == ref.shape
            fin = np.isfinite(ref)
            assert not np.isfinite(a[~fin]).any(), (name, M, mode, entry, ch)      # (the fixtures are finite everywhere)
            with np.errstate(invalid="ignore"):
                share = np.abs(a - ref) / gate(ref, noise)
            share = np.where(np.isnan(share) | ~fin, np.where(fin, np.inf, 0.0), share)
            w = np.unravel_index(int(np.argmax(share)), share.shape)
            worst = float(share[w])
            print(f"{name} M {M} {mode} {entry} {ch}: worst err / gate {worst:.3e} at point {w[0]} depth {w[1]}: device {a[w]:.17g} "
                  f"oracle {ref[w]:.17g} noise {noise[w]:.2e}")
            REPORT["whole"].setdefault(f"{name}/M{M}/{mode}", {}).setdefault(entry, {})[ch] = worst
            if not worst <= 1.0:
                failures.append((entry, ch, worst, w, float(a[w]), float(ref[w]), float(noise[w])))
    assert not failures, failures


CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, os.path.join(root, "oracle"))
import gen_dehoog_big as gen
from golden_util import load_deck
from unconfined_amd import engine
for name in gen.DECKS:
    z = np.load(gen.path_of(name))
    dk = load_deck(name)[0]
    tl, rl, sl = gen.points(z["tD"], z["rD"], z["sv"])
    idx = np.arange(int(sys.argv[3])) % len(tl)
    it = np.arange(int(sys.argv[2])) % len(z["tD"])
    for M in gen.MS:
        for mode in ("faithful", "fast"):
            plan = engine.Plan(gen.params(dk, M), mode=mode)
            def case(entry):
                sys.stderr.write("[case] %s/M%d/%s/%s\n" % (name, M, mode, entry)); sys.stderr.flush()
            case("grid46x2"); plan.drawdown_grid(z["tD"][it], z["sv"][it], z["rD"], z["zD"], z["zl"])
            case("list12"); plan.drawdown(tl, rl, sl, z["zD"], z["zl"])
            case("list384"); plan.drawdown(tl[idx], rl[idx], sl[idx], z["zD"], z["zl"])
            plan.close()
sys.stderr.write("[case] end\n")
"""


@gpu
def test_the_kernels_these_calls_launch(tmp_path):
    script = os.path.join(str(tmp_path), "dehoog_big_child.py")
    with open(script, "w") as f:
        f.write(CHILD)
    r = subprocess.run([sys.executable, script, ROOT, str(NGRID), str(NLONG)], env=dict(os.environ, UCF_TRACE_LAUNCHES="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    cases, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:]
            assert cur not in cases, cur
            cases[cur] = []
            continue
        m = re.search(r"next: (.*)$", line)
        if m and line.startswith("[ucf] stream"):
            assert line.startswith("[ucf] stream clean;"), line
            cases[cur].append(m.group(1))
    assert cases.pop("end") == []
    assert len(cases) == len(gen.DECKS) * len(gen.MS) * len(MODES) * len(ENTRIES)
    REPORT["kernels"] = {c: sorted(set(v)) for c, v in cases.items()}
    for c, names in cases.items():
        ns = "ucf_fast" if "/fast/" in c else "ucf_faithful"
        layouts = {int(m.group(3)) for m in map(TRANSFORM.search, names) if m}
        # (the abscissa table is the faithful kernel's in both flavours; the transform and the inversion are the flavour's own)
        assert names and all(n.startswith(ns + "::") for n in names if TRANSFORM.search(n) or "dehoog" in n), (c, names)
        if c.endswith("grid46x2"):
            assert names[-1] == ns + "::dehoog_tiles_kernel<1, true>" and layouts == {1}, (c, names)
        else:
            # the chunked transform; launch_points_chunked, its only launcher, runs dehoog_points_kernel next (not named in the trace)
            assert layouts == {2} and not any("dehoog_tiles_kernel" in n for n in names), (c, names)


@gpu
def test_zz_report():
    """(last in this file) the shares go next to the parity report"""
    if not (REPORT["hook"] or REPORT["whole"]):
        pytest.skip("no GPU test of this file ran")
    out = os.path.join(ROOT, os.environ.get("UCF_TOOLS_OUT", "tools_out"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "dehoog_big.json"), "w") as f:
        json.dump({"what": "tests/test_gpu_dehoog_big.py.  hook / edges: per M, flavour and channel the worst share of the rule over all vectors "
                           "of all cases (1.0 = exhausted): err_d / (K max(F, spread)), or, where refq <= ARBITRATION max(F, spread), the smaller "
                           "of that and err_q / (K max(F, refq)); `worst` holds that vector's figures.  whole: per deck, M, flavour and entry the "
                           "worst |device - binary64 oracle| / gate(ref, noise) over the 12 points and the depths.  skipped_fixtures: the "
                           "de Hoog fixtures of stages_generic.npz with 2M+1 > 64 against the bars of test_dehoog_tiled_kernel.  kernels: what "
                           "UCF_TRACE_LAUNCHES named per entry",
                   "K": {m: K[m]["totlap"] for m in MODES}, "F": F, "arbitration": ARBITRATION, "draws": NDRAWS, **REPORT}, f, indent=1, sort_keys=True)
