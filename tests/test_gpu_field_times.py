"""ucf_field_ensemble_times on the GPU.

The kernel alone, through ucf_debug_field_times on synthetic series: bit for bit (tobytes, NaN included: the statement names
the NaN) the arithmetic that include/ucf.h states, restated in numpy (tests/field_times_restate.py, itself held to hand-made
columns by tests/test_field_times_host.py).

End to end on the fixtures of tests/test_gpu_field.py (4 wells in 2 start-time groups, 5 locations, 6 times, 2 depths, both
flavours) with three members -- the deck's own values and two sets moved by +-0.2 in ln Kr and -+0.2 in ln Ss: T.all is the
restatement applied to the member maps of ucf_field_ensemble on a fresh field, every statistic and plater is what
ucf_debug_ensemble (with weights ucf_debug_ensemble_weighted) makes of T.all, all bit for bit.

Against the oracle nothing is chosen.  tests/test_gpu_field.py holds every output of the field to |s - s_ref| <= bound_s, the
|q|-weighted sum of the gates of its terms; `gate` and that sum are restated here.  The first up-crossing is antitone in the
series: raising every value can only move it earlier.  So with T_lo the restatement on s_ref + bound_s and T_hi the one on
s_ref - bound_s every device T lies in [T_lo, T_hi] -- PROVIDED that the rounding of the interpolation itself cannot matter,
which the condition |s_ref[k] - L| > 4 bound_s[k] at every time of every site secures: then s, s_ref + bound_s and s_ref - bound_s
cross in the same interval, with L - v0 and v - v0 both above 3 bound_s >= 3e-10 |s_ref| (the gate's floor), ten thousand times
the 5 u = 5.6e-16 relative that the five roundings of the statement can move T by, while the envelope is 2 bound_s / (v - v0) of
the interval wide.  The condition is asserted, for all 10 sites of every deck; the limits were chosen on the fixtures' reference
values so that it holds."""
import os

import numpy as np
import pytest

import field_times_restate as R
from golden_util import GOLD, load_deck
from test_gpu_field_ensemble import debug_ensemble, same_bits
from test_gpu_field_ensemble_weighted import debug_weighted

pytestmark = pytest.mark.gpu

DECKS = ["neuman74_partpen", "c2_neuman74_fullpen", "c1_theis"]
MODES = ["faithful", "fast"]
ORACLE_LIMITS = {"c1_theis": (8.99, 18.29, 28.62), "c2_neuman74_fullpen": (0.053, 0.174, 0.49), "neuman74_partpen": (0.073, 0.213, 0.533)}
FREE = ["Kr", "Ss"]
LEVELS = (0.05, 0.5, 0.95)
SENTINEL = -999999.9
FIRST, LAST = R.FIRST_ABOVE, R.LAST_ABOVE
STAT_KEYS = ("mean", "sd", "min", "max", "quant", "nfin")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


# ---- the kernel alone

def debug_times(a, tau, tau_never, limit, kind):
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    nens, nt, nsite = a.shape
    tau, limit = np.ascontiguousarray(tau, dtype=np.float64), np.ascontiguousarray(limit, dtype=np.float64)
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    T = np.full((nens, len(limit), nsite), -7.0)
    ucflib.check(so.ucf_debug_field_times(nens, nt, nsite, a.ctypes.data, tau.ctypes.data, float(tau_never), len(limit), limit.ctypes.data,
                                          kind.ctypes.data, T.ctypes.data))
    return T


NKINDS = 13


def series(nens, nt, nsite, seed):
    """a [nens][nt][nsite] about the limit 1, the column of site e of kind (e + seed) % 13, the positions random per member: plain;
    above at k = 0; never above; v == 1 exactly and nowhere above; v0 == 1 below the crossing (f = 0); a plateau above; rise, fall,
    rise; still above at nt - 1; NaN before the crossing; NaN after the crossing; +-inf; zeros of both signs (with a few +-1);
    the Wynn sentinel among the values.  A kind that needs more times than there are keeps what fits."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(nens, nt, nsite)) + 0.6
    for m in range(nens):
        for e in range(nsite):
            kind, c = (e + seed) % NKINDS, a[m, :, e]
            k = int(rng.integers(nt))
            if kind == 1:
                c[0] = 2.5
            elif kind == 2:
                c[:] = np.minimum(c, 0.9)
            elif kind == 3:
                c[:] = np.minimum(c, 0.9)
                c[k] = 1.0
            elif kind == 4:
                c[:] = 0.5
                c[max(k - 1, 0)] = 1.0
                if k >= 1:
                    c[k] = 2.0
            elif kind == 5:
                c[:] = 0.5
                c[1:max(nt - 1, 1)] = 2.0
            elif kind == 6:
                c[:] = np.where(np.arange(nt) % 2 == 1, 2.0 + 0.25 * np.arange(nt), -0.5)
                if nt % 2 == 0:
                    c[nt - 1] = 0.25
            elif kind == 7:
                c[nt - 1] = 2.0
            elif kind == 8:
                c[:] = 0.5
                c[0] = np.nan
                c[nt - 1] = 2.0 if nt > 1 else np.nan
            elif kind == 9:
                c[:] = 0.5
                if nt >= 3:
                    c[1], c[2 + int(rng.integers(nt - 2))] = 2.0, np.nan
                elif nt == 2:
                    c[0], c[1] = 2.0, np.nan
            elif kind == 10:
                c[k] = np.inf if rng.random() < 0.5 else -np.inf
            elif kind == 11:
                c[:] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), nt)
            elif kind == 12:
                c[k] = SENTINEL
    return a


LIMITS16 = np.array([1.0, 1.0, 0.0, -0.0, 2.0, 2.0, SENTINEL, SENTINEL, 0.5, 0.9, 2.5, -0.5, 0.25, 3.0, 0.6, 0.6])
KINDS16 = np.array([FIRST, LAST, FIRST, LAST, LAST, FIRST, FIRST, LAST, LAST, FIRST, LAST, FIRST, LAST, FIRST, FIRST, LAST], np.int32)


@pytest.mark.parametrize("nlim", [1, 16])
@pytest.mark.parametrize("nt", [1, 2, 7])
@pytest.mark.parametrize("nens", [1, 3])
def test_the_kernel_is_the_restatement(eng, nens, nt, nlim):
    """a partial wave, exactly one, one lane more, a second workgroup (nsite = 257); one time (no interpolation at all), two, and
    enough for every kind of column; one limit and the most there may be, the two kinds mixed"""
    tau = np.cumsum(np.array([0.5, 1.5, 5.0, 143.0, 850.0, 2000.0, 4000.0]))[:nt]
    never = 2.0 * tau[-1]
    seen = dict(nan=0, never=0, first=0, inner=0)
    for i, nsite in enumerate((1, 63, 64, 65, 257)):
        seed = 100 * nens + 10 * nt + nlim + i
        a = series(nens, nt, nsite, seed)
        if nlim == 1:
            limit, kind = LIMITS16[:1], np.array([(FIRST, LAST)[i % 2]], np.int32)
        else:
            limit, kind = LIMITS16.copy(), KINDS16
            limit[14:] = a[0, nt // 2, nsite // 2] if np.isfinite(a[0, nt // 2, nsite // 2]) else 0.6      # the bits of a value that occurs
        got = debug_times(a, tau, never, limit, kind)
        want = R.times(a, tau, never, limit, kind)
        assert got.shape == want.shape == (nens, nlim, nsite)
        assert got.tobytes() == want.tobytes(), (nens, nt, nsite, nlim, np.argwhere(got.view(np.int64) != want.view(np.int64))[:5].tolist())
        seen["nan"] += int(np.isnan(got).sum())
        seen["never"] += int((got == never).sum())
        seen["first"] += int((got == tau[0]).sum())
        seen["inner"] += int(((got > tau[0]) & (got < tau[-1])).sum())
        # a call repeated gives the same bytes
        assert debug_times(a, tau, never, limit, kind).tobytes() == got.tobytes()
    assert seen["nan"] and seen["never"] and seen["first"] and (nt == 1 or seen["inner"]), seen


def test_the_kernel_on_the_hand_made_columns(eng):
    """the columns of tests/test_field_times_host.py with their written-out values, on the device"""
    from test_field_times_host import COLUMNS, NEVER, TAU
    a = np.array([c[0] for c in COLUMNS.values()]).T[None]
    got = debug_times(a, TAU, NEVER, [1.0, 1.0, 0.0, 0.0], [FIRST, LAST, FIRST, LAST])[0]
    want = np.array([c[1:] for c in COLUMNS.values()]).T
    assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (got.tolist(), want.tolist())


# ---- end to end

_cache = {}


def case(eng, deck, mode):
    """(fixture, parameters, plan, the three members, their maps from ucf_field_ensemble on a fresh field) -- once per deck and flavour"""
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField
        fx = np.load(os.path.join(GOLD, f"field_{deck}.npz"))
        _, _, P = load_deck(deck)
        plan = eng.Plan(P, mode=mode)
        up, down = np.exp(0.2), np.exp(-0.2)
        thetas = np.array([[P.Kr, P.Ss], [P.Kr * up, P.Ss * down], [P.Kr * down, P.Ss * up]])
        fresh = WellField(fx["wells"], fx["locations"], fx["times"])
        ens = fresh.ensemble(plan, FREE, thetas, fx["z"], quantiles=None, derivative=False, all_maps=True)
        fresh.close()
        _cache[(deck, mode)] = dict(fx=fx, P=P, plan=plan, thetas=thetas, s_all=ens["s_all"])
    return _cache[(deck, mode)]


def e2e_limits(deck):
    """the limits of the oracle test twice, as first up-crossings and as recovery times"""
    return np.array(ORACLE_LIMITS[deck] * 2), np.array([FIRST] * 3 + [LAST] * 3, np.int32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_end_to_end_is_the_restatement_and_the_existing_reduction(eng, deck, mode):
    from unconfined_amd import WellField
    c = case(eng, deck, mode)
    fx, t = c["fx"], c["fx"]["times"]
    limit, kind = e2e_limits(deck)
    never = 2.0 * t[-1]
    horizons = np.array([100.0, t[-1]])
    nens, shape = len(c["thetas"]), (len(limit), len(fx["locations"]), len(fx["z"]))
    assert c["s_all"].shape == (3, 6, 5, 2) and np.isfinite(c["s_all"]).all()
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    res = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, kinds=kind, q=LEVELS, horizons=horizons, all_times=True)
    want = R.times(c["s_all"], t, never, limit, kind)
    assert res.all.shape == want.shape == (nens,) + shape
    assert res.all.tobytes() == want.tobytes(), (deck, mode, float(np.nanmax(np.abs(res.all - want))))
    assert res.never == never and not res.log_moments and res.nbad == 0 and (res.nfin == nens).all()
    # first crossings are decided within the map; these wells never stop and the drawdown only rises, so it is above a limit to
    # the end (never) or not at all (the first time): test_recovery_after_the_pumps_stop has recovery times within the map
    assert ((res.all[:, :3] > t[0]) & (res.all[:, :3] < t[-1])).any() and np.isin(res.all[:, 3:], (never, t[0])).all()
    assert ((res.all[:, :3] == never) == (res.all[:, 3:] == t[0])).all()
    ref = debug_ensemble(res.all.reshape(nens, -1), LEVELS, horizons)
    for key in STAT_KEYS:
        same_bits(getattr(res, key).reshape(ref[key].shape), ref[key], key)
    same_bits(res.later.reshape(ref["pexc"].shape), ref["pexc"], "plater")
    assert ref["nbad"] == 0
    # the chance of never crossing within the map is plater at the last time
    assert (res.later[1] == (res.all > t[-1]).sum(axis=0) / float(nens)).all()

    # the members count by their weight; the one of weight 0 is not launched
    w = np.array([1.0, 0.0, 0.25])
    rw = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, kinds=kind, q=LEVELS, horizons=horizons, all_times=True, weights=w)
    assert rw.nlaunched == 2 and rw.u.tolist() == [2 ** 32, 0, 2 ** 30]
    assert np.isnan(rw.all[1]).all() and rw.all[[0, 2]].tobytes() == res.all[[0, 2]].tobytes()
    refw = debug_weighted(rw.all.reshape(nens, -1), w, LEVELS, horizons)
    for key in STAT_KEYS:
        same_bits(getattr(rw, key).reshape(refw[key].shape), refw[key], key)
    same_bits(rw.later.reshape(refw["pexc"].shape), refw["pexc"], "weighted plater")
    assert rw.nbad == refw["nbad"] == 0 and (rw.nfin == 2).all()

    # ln t as the abscissa: the restatement on ln t, exponentiated -- min, max, quant and all are times, mean and sd stay in ln t
    rl = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, kinds=kind, q=LEVELS, all_times=True, abscissa="lnt")
    wl = R.times(c["s_all"], np.log(t), float(np.log(never)), limit, kind)
    back = lambda v: np.where(v == float(np.log(never)), never, np.exp(v))       # a censored value comes back as `never` itself
    assert rl.all.tobytes() == back(wl).tobytes() and rl.log_moments and rl.later is None and (rl.all == never).any()
    refl = debug_ensemble(wl.reshape(nens, -1), LEVELS, ())
    same_bits(rl.mean.reshape(-1), refl["mean"], "mean of ln t")
    same_bits(rl.sd.reshape(-1), refl["sd"], "sd of ln t")
    for key in ("min", "max", "quant"):
        same_bits(getattr(rl, key).reshape(refl[key].shape), back(refl[key]), key + " in lnt")
    field.close()


@pytest.mark.parametrize("deck", DECKS)
def test_recovery_after_the_pumps_stop(eng, deck):
    """a well that pumps from 0 and an injection of the same rate at the same place from t = 5 on -- the pump stops --: the drawdown
    rises, then falls, and LAST_ABOVE interpolates within the map.  The reference is ucf_field_ensemble on a fresh field."""
    from unconfined_amd import WellField
    c = case(eng, deck, "fast")
    fx, t = c["fx"], c["fx"]["times"]
    wells = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, -1.0, 5.0]])
    fresh = WellField(wells, fx["locations"], t)
    s_all = fresh.ensemble(c["plan"], FREE, c["thetas"], fx["z"], quantiles=None, derivative=False, all_maps=True)["s_all"]
    fresh.close()
    assert np.isfinite(s_all).all() and (s_all[:, 2] > s_all[:, 5]).all()           # higher at t = 7 than at the end
    limit = np.quantile(s_all[0], [0.25, 0.5, 0.75, 0.25, 0.5, 0.75])
    kind = np.array([LAST] * 3 + [FIRST] * 3, np.int32)
    never = 2.0 * t[-1]
    field = WellField(wells, fx["locations"], t)
    res = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, kinds=kind, q=LEVELS, horizons=[150.0], all_times=True)
    want = R.times(s_all, t, never, limit, kind)
    assert res.all.tobytes() == want.tobytes(), (deck, float(np.nanmax(np.abs(res.all - want))))
    inner = (res.all > t[0]) & (res.all < t[-1])
    print(f"[field times recovery {deck}] recovery times within the map: {int(inner[:, :3].sum())} of {inner[:, :3].size}, "
          f"first crossings within it: {int(inner[:, 3:].sum())} of {inner[:, 3:].size}")
    assert inner[:, :3].any() and inner[:, 3:].any()
    # where both are decided the drawdown recovers below a limit after it has first passed it
    both = inner[:, :3] & inner[:, 3:]
    assert (res.all[:, :3][both] > res.all[:, 3:][both]).all()
    ref = debug_ensemble(res.all.reshape(len(s_all), -1), LEVELS, [150.0])
    for key in STAT_KEYS:
        same_bits(getattr(res, key).reshape(ref[key].shape), ref[key], key)
    same_bits(res.later.reshape(ref["pexc"].shape), ref["pexc"], "plater")
    field.close()


# ---- against the oracle

def gate(ref, noise):
    """the bound on a launched value of tests/test_gpu_field.py, restated"""
    return np.maximum(1e-10, 10.0 * noise) * np.maximum(np.abs(ref), 1e-3)


def abs_superpose(wells, groups, b, nt, nloc, nz):
    """sum_j |q_j| b_j over the terms of an output, in the order of field_superpose_kernel (tests/test_gpu_field.py: `superpose`
    with the rates' magnitudes, tfac = 1 and no scale), restated; b[g]: [nt_g][nr_g][nz]"""
    out = np.zeros((nt, nloc, nz))
    owner = [next(g for g, grp in enumerate(groups) if grp["col"][0, j] >= 0) for j in range(len(wells))]
    for k in range(nt):
        for i in range(nloc):
            for iz in range(nz):
                acc = np.float64(0.0)
                for j in range(len(wells)):
                    grp = groups[owner[j]]
                    if k < grp["k0"]:
                        continue
                    acc = acc + np.abs(wells[j, 2]) * b[owner[j]][k - grp["k0"], grp["col"][i, j], iz]
                out[k, i, iz] = acc
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_against_the_oracle(eng, deck, mode):
    from unconfined_amd import WellField
    c = case(eng, deck, mode)
    fx, t = c["fx"], c["fx"]["times"]
    nt, nloc, nz = len(t), len(fx["locations"]), len(fx["z"])
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    groups = field.groups(c["plan"])
    bound_s = abs_superpose(fx["wells"], groups, [gate(fx[f"g{g}_ref_h"], fx[f"g{g}_noise_h"]) for g in range(len(groups))], nt, nloc, nz)
    s_ref = fx["s_ref"]
    assert (bound_s > 0.0).all() and bound_s.shape == s_ref.shape
    limit = np.array(ORACLE_LIMITS[deck])
    kind = np.full(len(limit), FIRST, np.int32)
    never = 2.0 * t[-1]
    # the condition: no value of the reference within 4 bounds of a limit, at any time of any site
    for L in limit:
        margin = np.abs(s_ref - L) / bound_s
        assert (margin > 4.0).all(), (deck, L, float(margin.min()))
    T_lo = R.times((s_ref + bound_s)[None], t, never, limit, kind)[0]
    T_hi = R.times((s_ref - bound_s)[None], t, never, limit, kind)[0]
    assert (T_lo <= T_hi).all() and np.isfinite(T_hi).all()
    width = float(((T_hi - T_lo) / T_hi).max())
    assert width <= 6e-9, width
    res = field.time_to_limit(c["plan"], FREE, c["thetas"][:1], fx["z"], limit, kinds=kind, all_times=True)
    T = res.all[0]
    pos = np.where(T_hi > T_lo, (T - T_lo) / np.where(T_hi > T_lo, T_hi - T_lo, 1.0), 0.5)
    print(f"[field times {deck} {mode}] envelope at most {width:.2e} of T wide; T at {float(pos.min()):.3f} .. {float(pos.max()):.3f} of it; "
          f"{int((T == never).sum())} of {T.size} censored, {int((T == t[0]).sum())} above from the first time")
    assert res.nbad == 0 and T.shape == T_lo.shape == (len(limit), nloc, nz)
    assert ((T_lo <= T) & (T <= T_hi)).all(), (deck, mode, float(pos.min()), float(pos.max()))
    # one member: the statistics are that member
    assert res.min.tobytes() == res.max.tobytes() == res.mean.tobytes() == T.tobytes() and np.isnan(res.sd).all()
    field.close()


# ---- repetition

def test_repetition(eng):
    """a second identical call gives the same bytes and allocates nothing; ucf_field_ensemble before and after gives the same bytes"""
    from unconfined_amd import WellField
    deck = DECKS[1]
    c = case(eng, deck, "fast")
    fx = c["fx"]
    limit, kind = e2e_limits(deck)
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    ens_kw = dict(quantiles=LEVELS, limits=limit[:2], all_maps=True)
    tim_kw = dict(kinds=kind, q=LEVELS, horizons=[100.0], all_times=True, weights=[1.0, 0.5, 0.25])
    e1 = field.ensemble(c["plan"], FREE, c["thetas"], fx["z"], **ens_kw)
    a = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, **tim_kw)
    n = field.alloc_count()
    b = field.time_to_limit(c["plan"], FREE, c["thetas"], fx["z"], limit, **tim_kw)
    assert n > 0 and field.alloc_count() == n
    for key in STAT_KEYS + ("all", "later", "u"):
        assert getattr(a, key).tobytes() == getattr(b, key).tobytes(), key
    assert (a.nbad, a.ess, a.nlaunched) == (b.nbad, b.ess, b.nlaunched) == (0, a.ess, 3)
    e2 = field.ensemble(c["plan"], FREE, c["thetas"], fx["z"], **ens_kw)
    assert sorted(e1) == sorted(e2)
    for key in e1:
        assert e1[key].tobytes() == e2[key].tobytes(), key
    assert e1["s_all"].tobytes() == c["s_all"].tobytes()
    # a smaller call after a larger one allocates nothing either
    field.time_to_limit(c["plan"], FREE, c["thetas"][:2], fx["z"], limit[:1], kinds=kind[:1])
    assert field.alloc_count() == n
    field.close()
