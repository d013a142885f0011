#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- mid-pipeline stage vectors for the folded one-depth water-table kernel at the configurations of
tests/folded_configs.py (kappa 0.03 ... 4, depths 0 ... 1, Malama's and Moench's boundary, other numerics), with the
reference's own rounding noise beside them, in the format of oracle/gen_midstages_families.py (one_pick is imported from
there): per configuration tests/golden/midstages_folded_<tag>.npz with

    picks [npicks, 2]                       (time index, radius index) into `times` (256) and `radii` (5)
    <k>_{tmp,glarea,totlap}, <k>_..._q      the binary64 oracle's stage vectors of pick k and those of its binary128 build
    refq, spread [npicks, 3]                the oracle's distance from binary128; what one ulp in tD or rD changes in it
    loops [2, npicks, nacc, 2M+1] int8      which loop of the kernel the pick's wave runs for each J0 interval and Laplace index,
                                            items whole (0) and cut into 8 parts (1): index into folded_configs.LOOPS

    python oracle/gen_midstages_folded.py [tag ...]        (no argument: every configuration)

The picks are PROPOSED from the CPU model of the kernel's classifiers (tools/folded_loop_phase_shares.py: sh_walk), not by
hand: a pick stands for its wave (the 64 times of its half decade, its radius, every Laplace index), and the waves are chosen
greedily so that their quadrature units together reach everything required() lists -- every loop the grid reaches at this
configuration, a unit the bounds decide, one they leave to the exact classifier, a tanh-sinh run that sets UCF_PH_SH and a part
(of 8) whose first unit sets it -- and then filled up to six.  Within a wave the lane is free: a candidate whose own noise is
outside the information caps of tests/test_midstages_families.py, or that binary128 does not arbitrate (refq > 4 max(F,
spread)), or that is not finite (rD = 0.05 at kappa <= 0.4: the late intervals' areas overflow), is REPLACED by another lane of the wave, and
a wave without a usable lane by another wave; nothing is listed as excluded.  check() asserts all of it before a file is
written, and tests/test_midstages_folded.py asserts it again from the files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import folded_configs as FC  # noqa: E402
from gen_midstages_families import STAGES, cplx, one_pick, vec_err  # noqa: E402,F401
from golden_util import GOLD  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

MIN_PICKS, MAX_PICKS, MAX_BYTES = 6, 8, 200 * 1000
LANES = (32, 12, 52, 22, 42, 4, 60)           # the lanes of a wave in the order they are tried
FLAGS = ("by_bounds", "by_exact", "ts_sets_sh", "part_first_sets_sh")
_MODELS = {}


def path_of(tag):
    return os.path.join(GOLD, f"midstages_folded_{tag}.npz")


def model(tag):
    """the CPU model of the classifiers at the configuration"""
    import folded_loop_phase_shares as S
    if tag not in _MODELS:
        _MODELS[tag] = S.Model(deck=FC.DECK, **FC.config(tag)[1])
    return _MODELS[tag]


def context(O, tag):
    """the arguments of one_pick: (P, D, j0z, tD, sv, rD, zD, zl)"""
    dk, P, zD = FC.deck_of(tag)
    D = O.nondim(P)
    tD = FC.times()
    z = np.array([zD])
    return dk, (P, D, O.j0_zeros(D.nj0z), tD, O.split_vector(list(dk.j0s), tD), FC.radii(), z, O.zlay(D, z))


def wave_reach(tag):
    """per wave (wave index = time index // 64, radius index): (loops [2][nacc][2M+1] int8 for items whole and cut into 8, the
    set of FLAGS that its units show), from the model's sh_walk"""
    S = model(tag)
    zD = FC.config(tag)[2]
    tD, rD = FC.times(), FC.radii()
    sv = S.split_vector(tD)
    assert len(np.unique(sv)) == 1 and len(tD) == 256         # one split index: wave w is the times [64 w, 64 w + 64)
    cs = (S.CLASSES.index("cs_tab"), S.CLASSES.index("cs_short"))
    out = {}
    for w, (s, p) in enumerate(S.waves(tD)):
        for ir, r in enumerate(rD):
            a = S.row(r, s)
            loops = np.zeros((2, S.nacc, 2 * S.M + 1), np.int8)
            flags = set()
            for c, nsplit in enumerate((1, 8)):
                first_of_part = {}
                for kind, b, e, cls, sets, have, ip, lob, hib in S.sh_walk(p, a, s, r, zD, nsplit):
                    bc = S.bound_class_v(p, lob, hib, zD)
                    if (bc != S.UNDECIDED).any():
                        flags.add("by_bounds")
                    if ((bc == S.UNDECIDED) & (cls != S.CLASSES.index("unproven"))).any():
                        flags.add("by_exact")
                    if nsplit == 1 and kind == "ts" and sets.any():
                        flags.add("ts_sets_sh")
                    if nsplit == 8 and ip not in first_of_part:
                        first_of_part[ip] = True
                        if ip > 0 and sets.any():                 # (part 0 starts with the tanh-sinh nodes)
                            flags.add("part_first_sets_sh")
                    if kind == "interval":
                        jj = (b - S.N) // S.ngl
                        sh = ((cls == cs[0]) | (cls == cs[1])) & have
                        loops[c, jj] = np.where(sh, len(S.CLASSES) + (cls == cs[1]), cls)
            out[(w, ir)] = (loops, flags)
    return out


def items_of(loops, flags):
    return {FC.LOOPS[i] for i in np.unique(loops)} | set(flags)


def required(tag, reach):
    """what the picks' waves must reach together: every loop that a wave of the grid reaches at this configuration (all that
    the depth can reach, but for the reasons GRID_NEVER gives), and for zD > 0 the four FLAGS"""
    zD = FC.config(tag)[2]
    on_grid = set().union(*(items_of(l, ()) for l, f in reach.values()))
    assert on_grid == set(FC.reachable_loops(zD)) - set(GRID_NEVER.get(tag, ())), (tag, sorted(on_grid))
    return on_grid | (set(FLAGS) if zD > 0.0 else set())


# loops that a depth could reach but no wave of the grid does.  kappa = 0.03 at zD = 1: Re eta zD >= a / sqrt(kappa) is past
# 0.35 from a = 0.061 on, the lowest J0 interval of the grid starts at j0z[0] / 30 = 0.080, so every cosh/sinh interval sets
# UCF_PH_SH itself and none runs the loop that keeps the series test (the tanh-sinh runs below it do go without the bit)
GRID_NEVER = {"k003_z1": ("cs_tab", "cs_short")}


def propose(tag, reach, bad):
    """waves (wave index, radius index), greedily: the fewest that reach everything required, then up to MIN_PICKS spread
    over the waves and radii; `bad`: waves without a usable lane"""
    need = required(tag, reach)
    cand = {k: items_of(*v) for k, v in reach.items() if k not in bad}
    chosen = []
    while need:
        k = max(sorted(cand), key=lambda k: len(cand[k] & need))
        assert cand[k] & need, (tag, "not reachable by the usable waves", sorted(need))
        chosen.append(k)
        need -= cand.pop(k)
    while len(chosen) < MIN_PICKS:
        k = min(sorted(cand), key=lambda k: (sum(c[0] == k[0] for c in chosen) + sum(c[1] == k[1] for c in chosen), -len(cand[k])))
        chosen.append(k)
        cand.pop(k)
    assert len(chosen) <= MAX_PICKS, (tag, chosen)
    return sorted(chosen)


def usable(rule, st, sq, refq, spread):
    """within the information caps, arbitrated by binary128, finite (tests/test_midstages_families.py: CAPS, F, ARBITRATION)"""
    for i, s in enumerate(STAGES):
        n = max(rule.F, float(spread[i]))
        if not (np.isfinite(st[s]).all() and np.isfinite(sq[s]).all() and n <= rule.CAPS[s] and refq[i] <= rule.ARBITRATION * n):
            return False
    return True


def check(rule, tag, z):
    """the conditions on a file (a dict or an open npz); returns what the picks' waves reach"""
    zD = FC.config(tag)[2]
    S = model(tag)
    picks = [(int(it), int(ir)) for it, ir in z["picks"]]
    npk = len(picks)
    assert MIN_PICKS <= npk <= MAX_PICKS and len(set((it // 64, ir) for it, ir in picks)) == npk, (tag, picks)
    assert z["refq"].shape == z["spread"].shape == (npk, 3)
    assert np.array_equal(z["times"], FC.times()) and np.array_equal(z["radii"], FC.radii())
    for k in range(npk):
        for i, s in enumerate(STAGES):
            v, q = z[f"{k}_{s}"], z[f"{k}_{s}_q"]
            assert v.shape == q.shape and np.isfinite(v).all() and np.isfinite(q).all(), (tag, k, s)
            n = max(rule.F, float(z["spread"][k][i]))
            assert n <= rule.CAPS[s], (tag, k, s, n)                                        # carries information
            assert float(z["refq"][k][i]) <= rule.ARBITRATION * n, (tag, k, s)              # arbitrated
            assert float(z["refq"][k][i]) == vec_err(cplx(v), cplx(q)), (tag, k, s)
    reach = wave_reach(tag)
    assert z["loops"].shape == (2, npk, S.nacc, 2 * S.M + 1) and z["loops"].dtype == np.int8
    got = set()
    for k, (it, ir) in enumerate(picks):
        loops, flags = reach[(it // 64, ir)]
        assert np.array_equal(z["loops"][:, k], loops), (tag, k)
        got |= items_of(loops, flags)
    need = required(tag, reach)
    assert need <= got, (tag, sorted(need - got))
    return got


def generate(O, Q, rule, tag):
    dk, ctx = context(O, tag)
    reach = wave_reach(tag)
    bad, cache = set(), {}

    def pick_in(w, ir):
        """the first usable lane of the wave, or None"""
        lost = 0
        for lane in LANES:
            p = (64 * w + lane, ir)
            if p not in cache:
                cache[p] = one_pick(O, Q, ctx, *p)
                st, sq, refq, spread = cache[p]
                print(tag, "candidate", p, "refq tmp %.1e gl %.1e tl %.1e" % tuple(refq), "| spread tmp %.1e gl %.1e tl %.1e" % tuple(spread),
                      "" if usable(rule, *cache[p]) else "-> replaced", flush=True)
            if usable(rule, *cache[p]):
                return p
            lost += not np.isfinite(cache[p][3]).all()
            if lost == 3:                                       # three lanes are not finite: the overflow regime
                break
        print(tag, "wave", (w, ir), "has no usable lane", flush=True)
        return None

    while True:
        waves = propose(tag, reach, bad)
        picks = [pick_in(w, ir) for w, ir in waves]
        if None not in picks:
            break
        bad.update(wv for wv, p in zip(waves, picks) if p is None)
    out = {"picks": np.array(picks, np.int32), "radii": FC.radii(), "times": FC.times(),
           "refq": np.zeros((len(picks), 3)), "spread": np.zeros((len(picks), 3)),
           "loops": np.stack([reach[(it // 64, ir)][0] for it, ir in picks], axis=1)}
    for k, p in enumerate(picks):
        st, sq, refq, spread = cache[p]
        for key in STAGES:
            out[f"{k}_{key}"], out[f"{k}_{key}_q"] = st[key], sq[key]
        out["refq"][k], out["spread"][k] = refq, spread
    got = check(rule, tag, out)
    np.savez_compressed(path_of(tag), **out)
    size = os.path.getsize(path_of(tag))
    print(tag, "model", dk.model, "picks", picks, "reach", sorted(got), size, "bytes", flush=True)
    assert size < MAX_BYTES, (tag, size)


def main(tags):
    import test_midstages_families as rule
    O, Q = Oracle(), Oracle(quad=True)
    for tag in tags:
        generate(O, Q, rule, tag)


if __name__ == "__main__":
    main(sys.argv[1:] or FC.TAGS)
