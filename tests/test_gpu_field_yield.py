"""ucf_field_yield on the GPU: field_yield_kernel through ucf_debug_field_yield on synthetic response slots, and the whole call
on the fixtures of tests/test_gpu_field_forecast.py (4 wells, 5 locations, 6 times, 2 depths; decks neuman74_partpen and
c1_theis; both flavours; 3 members: the first three parameter sets of the forecast), against the numpy restatement of
include/ucf.h (tests/field_yield_restate.py).

Bounds.  The kernels hold +, -, * and / only, each rounded on its own: y, fe, hi, lo, bind, dead, nbad, the response slots and
every statistic are compared bit for bit (NaN positions equal, zeros by value: the sign of a zero is not part of the contract).
The one exception is the one of the ensemble reduction itself (tests/test_gpu_field_ensemble.py): sd ends in a square root, which
numpy may round 1 ulp apart; sd is held to 1 ulp of the restatement AND bit for bit to ucf_debug_ensemble on the returned y.
Physical closure: a second field pumps y x_c q_j; its drawdown at an output is the same terms q_j h summed in another order
(all wells in the caller's order instead of slot by slot) with the rounded rate products (y x_c) q_j in place of y (x_c r_c):
two summation orders of nwell terms and two roundings per product, 4 (nwell + 2) u (|b| + y sum_c |x_c r_c|)."""
import ctypes as C
import os

import numpy as np
import pytest

import field_yield_restate as Y
from ensemble_weighted_restate import quantise, restate_weighted
from golden_util import GOLD, load_deck
from test_gpu_field_ensemble import check_statistics, debug_ensemble, restate, same_bits

pytestmark = pytest.mark.gpu

DECKS = ["neuman74_partpen", "c1_theis"]
MODES = ["faithful", "fast"]
U = 2.0 ** -53
SENTINEL = -999999.9
TILE = 8
SMAX = 3.0
SPECIALS = ("sentinel", "tie", "dead", "negative_hi", "lo_above_hi", "zero_pattern", "unbound")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def addr(a):
    return a.ctypes.data if a is not None else None


def debug(R, x, lim, con, smax):
    """one launch of field_yield_kernel through the library's launcher on caller data"""
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    assert abi.UCF_YIELD_PAT_TILE == TILE
    so = ucflib.load()
    R, x, lim = (np.ascontiguousarray(a, dtype=float) for a in (R, x, lim))
    con = np.ascontiguousarray(con, dtype=np.int32)
    nens, nslot, ncon = R.shape
    npat, nctl = x.shape
    assert nslot == nctl + 1 and lim.shape == con.shape == (ncon,)
    out = {k: np.zeros((nens, npat)) for k in ("y", "fe", "hi", "lo")}
    out.update({k: np.zeros((nens, npat), np.int32) for k in ("bind", "dead")})
    nbad = C.c_longlong(-1)
    ucflib.check(so.ucf_debug_field_yield(nctl, nens, ncon, npat, addr(R), addr(x), addr(lim), addr(con), float(smax),
                                          *(addr(out[k]) for k in ("y", "fe", "hi", "lo", "bind", "dead")), C.addressof(nbad)))
    out["nbad"] = int(nbad.value)
    return out


def same_values(got, want, what):
    """NaN positions equal, everything else equal by value: bit for bit but for the sign of a zero"""
    for key in ("y", "fe", "hi", "lo"):
        g, w = got[key], want[key]
        assert g.shape == w.shape and (np.isnan(g) == np.isnan(w)).all(), (what, key, "NaN pattern")
        ok = np.isnan(w) | (g == w)
        assert ok.all(), (what, key, int((~ok).sum()), g[~ok][:3], w[~ok][:3])
    for key in ("bind", "dead"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (what, key)
    assert got["nbad"] == want["nbad"], (what, got["nbad"], want["nbad"])


def synthetic(nctl, ncon, npat, nens, seed):
    """response slots with every member valid, patterns and limits, and the names of the special cases that the sizes have room
    for.  Usual outputs have room > 0 and responses of both signs.  The chosen (member, output) pairs:
      sentinel     member 0, slot 0, output 3 (output 0 where ncon == 1 and there are three members): finite, it takes part
      tie          outputs 5 and ncon - 1 of every member: the same slot values and limit, the tightest of the map
      special      output 20 of the last member: r = (1, 0, ..), room = -0.3: dead under a pattern with x_0 == 0, a negative hi
                   under x_0 > 0, a raised lo under x_0 < 0 and lo > hi under x_0 = -0.01.  Its negative candidate would bind
                   before the tie wherever x_0 > 0, and with one member and one control that is every pattern in which the tie
                   can bind: so the special output is planted at npat = 7 and 17 and the tie is asked for at npat = 9
    and the patterns (npat >= 7): 0 has x_0 = 0.7, 1 has x_0 = -0.01, 2 is all zeros, 3 has x_0 = 0, 4 is +-1e-7: no candidate
    reaches smax, 5 is all ones: the tie binds."""
    rng = np.random.default_rng(seed)
    R = np.zeros((nens, nctl + 1, ncon))
    R[:, :nctl] = rng.uniform(0.1, 1.0, (nens, nctl, ncon)) * rng.choice([-1.0, 1.0], (nens, nctl, ncon), p=[0.2, 0.8])
    R[:, nctl] = rng.uniform(0.0, 0.5, (nens, ncon))
    lim = 1.0 + rng.uniform(0.0, 1.0, ncon)
    x = rng.uniform(-1.0, 2.0, (npat, nctl))
    con = np.cumsum(rng.integers(1, 4, ncon)).astype(np.int32) - 1
    present = set()
    last = nens - 1
    if ncon >= 70:
        R[0, 0, 3] = SENTINEL
        R[:, :nctl, 5], R[:, nctl, 5], lim[5] = 0.9, 0.25, 0.3125
        R[:, :, ncon - 1], lim[ncon - 1] = R[:, :, 5], lim[5]
        present.add("sentinel")
        if npat == TILE + 1:
            present.add("tie")
        elif npat >= 7:
            R[last, :nctl, 20], R[last, 0, 20], R[last, nctl, 20] = 0.0, 1.0, lim[20] + 0.3
            present |= {"dead", "negative_hi", "lo_above_hi"}
    elif nens == 3:
        R[0, 0, 0] = SENTINEL
        present.add("sentinel")
    if npat >= 7:
        x[0, 0], x[1, 0], x[2], x[3, 0] = 0.7, -0.01, 0.0, 0.0
        x[4] = 1e-7 * np.where(np.arange(nctl) % 2 == 0, -1.0, 1.0)
        x[5] = 1.0
        present |= {"zero_pattern", "unbound"}
    return R, x, lim, con, present


def occurs(name, R, x, lim, con, want):
    """whether the special case shows in the restatement's output"""
    nctl, ncon, last = x.shape[1], R.shape[2], len(R) - 1
    if name == "sentinel":
        m0 = np.isfinite(R[0]).all() and (R[0] == SENTINEL).any()
        return bool(m0 and np.isfinite(want["hi"][0]).all())
    if name == "tie":                                   # the lower of the two outputs binds, with the bits of the upper one's candidate
        hit = np.argwhere(want["bind"] == con[5])
        for m, p in hit:
            D = np.float64(0.0)
            for c in range(nctl):
                D = D + x[p, c] * R[m, c, ncon - 1]
            if (lim[ncon - 1] - R[m, nctl, ncon - 1]) / D == want["hi"][m, p]:
                return True
        return False
    if name == "dead":
        return bool(want["dead"][last, 3] == 1 and want["y"][last, 3] == 0.0 and want["fe"][last, 3] == 0.0)
    if name == "negative_hi":
        return bool(want["hi"][last, 0] < 0.0 and want["fe"][last, 0] == 0.0 and want["bind"][last, 0] == con[20])
    if name == "lo_above_hi":
        return bool(want["dead"][last, 1] == 0 and want["hi"][last, 1] >= 0.0 and want["lo"][last, 1] > want["hi"][last, 1] and want["fe"][last, 1] == 0.0)
    if name == "zero_pattern":
        m = 0 if last > 0 else last
        return bool((x[2] == 0.0).all() and want["bind"][m, 2] == -1 and want["hi"][m, 2] == SMAX)
    if name == "unbound":
        return bool((x[4] != 0.0).all() and (want["bind"][:, 4] == -1).all() and (want["hi"][:, 4] == SMAX).all())
    raise KeyError(name)


@pytest.mark.parametrize("nens", [1, 3])
@pytest.mark.parametrize("nctl", range(1, 9))
def test_kernel_is_the_stated_arithmetic(eng, nctl, nens):
    """ncon under a wave, over a wave, over the 256-thread stride and several strides; npat 1, one below the pattern tile, one
    above it and two tiles + 1.  Per size one launch with every member valid and one with members made invalid by a NaN, a +inf
    or a -inf, each in another slot and at another output (two of the three per size, in turn; the member between them stays
    valid)."""
    seen = set()
    poisons = [(np.nan, 0, lambda n: n - 1), (np.inf, nctl, lambda n: n // 2), (-np.inf, nctl - 1, lambda n: 0)]
    feasible = 0
    for a, ncon in enumerate((1, 70, 257, 1030)):
        for b, npat in enumerate((1, TILE - 1, TILE + 1, 2 * TILE + 1)):
            R, x, lim, con, present = synthetic(nctl, ncon, npat, nens, 10000 * nctl + 100 * ncon + 10 * npat + nens)
            want = Y.ratio_test(R, x, lim, con, SMAX)
            assert want["nbad"] == 0
            for name in present:
                assert occurs(name, R, x, lim, con, want), (name, ncon, npat)
            seen |= present
            feasible += int((want["fe"] == 1.0).sum())
            same_values(debug(R, x, lim, con, SMAX), want, ("valid", ncon, npat))
            # members that are not valid
            Rb = R.copy()
            k = 4 * a + b
            for member, (value, slot, at) in zip((0, 2) if nens == 3 else (0,), (poisons[k % 3], poisons[(k + 1) % 3])):
                Rb[member, slot, at(ncon)] = value
            wantb = Y.ratio_test(Rb, x, lim, con, SMAX)
            assert wantb["nbad"] == (2 if nens == 3 else 1) and np.isnan(wantb["y"][0]).all() and (wantb["bind"][0] == -1).all()
            if nens == 3:
                assert np.array_equal(wantb["hi"][1], want["hi"][1])
            same_values(debug(Rb, x, lim, con, SMAX), wantb, ("invalid", ncon, npat))
    assert seen == set(SPECIALS), set(SPECIALS) - seen
    assert feasible > 0


# ---- the whole call on the fixtures

_cache = {}
X1 = np.array([[1.0], [0.5], [2.0]])
CTL2 = np.array([0, 1, -1, 0], np.int32)
X2 = np.array([[1.0, 1.0], [0.5, 2.0], [2.0, 0.5], [0.0, 1.0], [1.0, 0.0], [-1.0, 1.0], [0.0, 0.0], [1e-9, 1e-9], [1.0, -1.0]])
QS = (0.0, 0.05, 0.5, 1.0)
LEVELS = (0.5, 1.0)
SMAX2 = 10.0


def case(eng, deck, mode):
    """one ensemble call over the three members, then the yield calls of every test below, each once"""
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField, forecast_sets
        fx = np.load(os.path.join(GOLD, f"field_forecast_{deck}.npz"))
        _, _, P = load_deck(deck)
        free = [str(n) for n in fx["free"]]
        sets = forecast_sets(P, free, fx["theta"], float(fx["dlog"]))[:3]
        thetas = np.array([[getattr(Pk, name) for name in free] for Pk in sets])
        plan = eng.Plan(P, mode=mode)
        wells, loc, times, z = fx["wells"], fx["locations"], fx["times"], fx["z"]
        other = WellField(wells, loc, times)
        ens = other.ensemble(plan, free, thetas, z, quantiles=None, derivative=False, all_maps=True, with_stats=True)
        wens = other.ensemble(plan, free, thetas, z, quantiles=None, derivative=False, with_stats=True, weights=[1.0, 0.0, 0.5])
        other.close()
        # limits on both depths of every location at the last two times and on three earlier outputs: half again the largest
        # drawdown of the members there, so that the rates as given are admissible and the scale 1.5 is about the end
        s = ens["s_all"]
        limit = np.full(s.shape[1:], np.inf)
        top = np.abs(s).max(axis=0)
        limit[-2:] = 1.5 * top[-2:] + 1e-3 * top.max()
        for k, i, iz in ((0, 1, 0), (2, 4, 1), (3, 0, 0)):
            limit[k, i, iz] = 1.5 * top[k, i, iz] + 1e-3 * top.max()
        field = WellField(wells, loc, times)
        kw = dict(limit=limit, smax=SMAX2, q=QS, levels=LEVELS, with_stats=True)
        one = field.sustainable_yield(plan, free, thetas, z, np.zeros(4, np.int32), X1, **kw)
        two = field.sustainable_yield(plan, free, thetas, z, CTL2, X2, **kw)
        n = field.alloc_count()
        again = field.sustainable_yield(plan, free, thetas, z, CTL2, X2, **kw)
        n_again = field.alloc_count()
        weighted = field.sustainable_yield(plan, free, thetas, z, CTL2, X2, weights=[1.0, 0.0, 0.5], **kw)
        equal = field.sustainable_yield(plan, free, thetas, z, CTL2, X2, weights=[2.0, 2.0, 2.0], **kw)
        _cache[(deck, mode)] = dict(fx=fx, free=free, sets=sets, thetas=thetas, plan=plan, ens=ens, wens=wens, limit=limit, field=field, one=one, two=two,
                                    again=again, n=n, n_again=n_again, weighted=weighted, equal=equal)
    return _cache[(deck, mode)]


def check_call(out, x, limit, smax, u=None):
    """y .. dead and every statistic of a call against the restatement applied to the returned response slots"""
    con, lim_con = Y.constrained(limit)
    assert out["con"].dtype == np.int32 and np.array_equal(out["con"], con)
    want = Y.ratio_test(out["resp"], x, lim_con, con, smax)
    # a member that is not launched is not counted in nbad; fe is no output of the call: pfeas below is its reduction
    got = dict(out, fe=want["fe"], nbad=out["nbad"] + (0 if u is None else int((u == 0).sum())))
    same_values(got, want, "call")
    stat = restate(out["y"], QS, LEVELS) if u is None else restate_weighted(out["y"], u, QS, LEVELS)
    off = check_statistics(out, stat)
    same_bits(out["pexc"], stat["pexc"], "pexc")
    fes = restate(want["fe"], (), (0.5,)) if u is None else restate_weighted(want["fe"], u, (), (0.5,))
    same_bits(out["pfeas"], fes["pexc"][0], "pfeas")
    if u is None:
        # sd bit for bit: the reduction kernels alone on the returned y
        alone = debug_ensemble(out["y"], levels=QS, limits=LEVELS)
        for key in ("mean", "sd", "min", "max", "quant", "nfin", "pexc"):
            same_bits(out[key], alone[key], "alone " + key)
    return want, off


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_one_control_is_the_ensemble_map(eng, deck, mode):
    c = case(eng, deck, mode)
    out, ens = c["one"], c["ens"]
    con = out["con"]
    assert len(con) == 23 and out["resp"].shape == (3, 2, 23)
    for m in range(3):
        assert out["resp"][m, 0].tobytes() == ens["s_all"][m].ravel()[con].tobytes(), m
        assert (out["resp"][m, 1] == 0.0).all()                # no well is fixed
    assert out["stats"] == ens["stats"]
    want, _ = check_call(out, X1, c["limit"], SMAX2)
    # the limits are 1.5 times the largest member's drawdown and more: the rates as given are admissible, 1.5 times them too
    assert (out["y"][:, 0] >= 1.5).all() and (out["pfeas"] == 1.0).all() and (out["bind"] >= 0).all() and out["nbad"] == 0
    # half the rates admit twice the scale: the candidates are room / (0.5 r) against room / r
    assert np.allclose(out["y"][:, 1], np.minimum(2.0 * out["y"][:, 0], SMAX2), rtol=4 * U)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_two_controls_and_a_fixed_well(eng, deck, mode):
    c = case(eng, deck, mode)
    out = c["two"]
    want, off = check_call(out, X2, c["limit"], SMAX2)
    print(f"[yield {deck} {mode}] y of [1, 1]: {out['y'][:, 0]}, feasible {int(want['fe'].sum())} of {want['fe'].size}, "
          f"sd values 1 ulp from numpy's square root: {off} of {out['sd'].size}")
    assert out["stats"] == c["ens"]["stats"] and out["nbad"] == 0
    assert (out["resp"][:, 2] != 0.0).any()                     # the fixed well pumps
    assert (out["bind"][:, 6] == -1).all() and (out["bind"][:, 7] == -1).all()      # all zeros; rates too small to reach smax
    assert (want["fe"][:, 0] == 1.0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_physical_closure(eng, deck, mode):
    """a second field that pumps y x_c q_j meets the limit at `bind` under the binding member and exceeds it nowhere"""
    from unconfined_amd import WellField
    c = case(eng, deck, mode)
    out, fx, limit = c["two"], c["fx"], c["limit"]
    wells, con = fx["wells"], out["con"]
    nwell, checked = len(wells), 0
    for m in range(3):
        plan_m = eng.Plan(c["sets"][m], mode=mode)
        for p in (0, 1, 2):                                     # the patterns without a zero: a well needs a rate
            y, e = out["y"][m, p], out["bind"][m, p]
            if not (y > 0.0 and e >= 0):
                continue
            w2 = wells.copy()
            for j in range(nwell):
                if CTL2[j] >= 0:
                    w2[j, 2] = (y * X2[p, CTL2[j]]) * wells[j, 2]
            second = WellField(w2, fx["locations"], fx["times"])
            s2 = second.drawdown(plan_m, fx["z"])[0].ravel()
            second.close()
            R = out["resp"][m]
            bound = 4 * (nwell + 2) * U * (np.abs(R[2]) + y * (np.abs(X2[p, 0] * R[0]) + np.abs(X2[p, 1] * R[1])))
            over = s2[con] - limit.ravel()[con]
            i = int(np.flatnonzero(con == e)[0])
            print(f"[yield closure {deck} {mode}] member {m} pattern {p}: y = {y:.6f}, at bind |s - limit| = {abs(over[i]):.3e}, "
                  f"{abs(over[i]) / bound[i]:.3f} of the bound; largest excess elsewhere {float((over / bound).max()):.3f} of its bound")
            assert abs(over[i]) <= bound[i], (m, p, over[i], bound[i])
            assert (over <= bound).all(), (m, p)
            checked += 1
        plan_m.close()
    assert checked >= 3


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_a_member_of_weight_zero_is_not_launched(eng, deck, mode):
    c = case(eng, deck, mode)
    out, two = c["weighted"], c["two"]
    u, ess = quantise([1.0, 0.0, 0.5])
    assert out["u"].tobytes() == u.tobytes() and out["ess"] == ess and out["nlaunched"] == 2
    assert out["stats"] == c["wens"]["stats"]                   # what the weighted ensemble call launches for the same weights
    for key in ("resp", "y", "hi", "lo"):
        assert np.isnan(out[key][1]).all(), key
        assert out[key][0].tobytes() == two[key][0].tobytes() and out[key][2].tobytes() == two[key][2].tobytes(), key
    assert (out["bind"][1] == -1).all() and (out["dead"][1] == 0).all() and out["nbad"] == 0
    check_call(out, X2, c["limit"], SMAX2, u=u)
    assert (out["nfin"] == 2).all()
    # equal weights: the statistics of the unweighted call, bit for bit (the quantile is the inverse distribution function)
    eq = c["equal"]
    assert eq["nlaunched"] == 3 and (eq["u"] == 2 ** 32).all()
    for key in ("y", "hi", "lo", "bind", "dead", "resp", "mean", "sd", "min", "max", "nfin", "pexc", "pfeas"):
        assert eq[key].tobytes() == two[key].tobytes(), key
    check_call(eq, X2, c["limit"], SMAX2, u=eq["u"])


@pytest.mark.parametrize("deck,mode", [("neuman74_partpen", "fast"), ("c1_theis", "faithful")])
def test_repetition(eng, deck, mode):
    c = case(eng, deck, mode)
    assert c["n"] > 0 and c["n_again"] == c["n"]
    for key, v in c["two"].items():
        if isinstance(v, np.ndarray):
            assert c["again"][key].tobytes() == v.tobytes(), key
        else:
            assert c["again"][key] == v, key
