"""ucf_field_ensemble on the GPU.  The members are the parameter sets of the forecast fixtures (tests/test_gpu_field_forecast.py:
4 wells in 2 start-time groups, 5 locations, 6 times, 2 depths = 60 outputs; nine sets for neuman74_partpen, five for c1_theis),
so every slot has three independent references that already exist: ucf_field_forecast's slots, ucf_field_drawdown on a fresh
field and plan, and the oracle values of the fixture.

Bounds.  Slots: bit for bit.  Statistics: bit for bit against the arithmetic that include/ucf.h states, restated in numpy one
rounded operation at a time (`restate`); sd within 1 ulp of numpy's square root; the payload of a NaN is not compared.  quant is
also held to np.quantile(method="linear") within 4 ulp of the larger neighbouring order statistic: both interpolate between the
same two values and differ only in how they round.  Against the oracle nothing is chosen: each slot lies within the fixture's
bound[m] of the oracle's value (tests/test_gpu_field_forecast.py asserts that), hence |mean - mean(ref)| <= mean(bound) by the
triangle inequality, and an order statistic of values each moved by at most b = max_m bound[m] moves by at most b -- so do min,
max and the interpolated quantiles, which are convex combinations of two order statistics.
The kernels' edges are tested through ucf_debug_ensemble on synthetic data, without evaluations."""
import ctypes as C
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_field_forecast import DECKS, MODES, case
from test_gpu_fit import NAN_R, NAN_T

pytestmark = pytest.mark.gpu

LEVELS = (0.0, 0.05, 0.5, 1.0)
STATS = ("mean", "sd", "min", "max", "quant", "nfin")
SENTINEL = -999999.9


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def restate(a, levels, limits):
    """the arithmetic of field_ensemble_moments_kernel and field_ensemble_quantile_kernel as include/ucf.h states it, on
    a [nens][...]: dict of nfin, mean, sd (numpy's square root), min, max, quant [nq][...], pexc [nlim][...], nbad"""
    nens, shape = len(a), a.shape[1:]
    v = a.reshape(nens, -1)
    fin = np.isfinite(v)
    n = fin.sum(axis=0)
    dn = n.astype(np.float64)
    nan = np.full(v.shape[1], np.nan)
    with np.errstate(all="ignore"):
        acc, lo, hi = np.zeros(v.shape[1]), nan.copy(), nan.copy()
        for m in range(nens):
            acc = np.where(fin[m], acc + v[m], acc)
            lo = np.where(fin[m] & ~(v[m] >= lo), v[m], lo)
            hi = np.where(fin[m] & ~(v[m] < hi), v[m], hi)
        mean = acc / dn
        ss = np.zeros(v.shape[1])
        for m in range(nens):
            d = v[m] - mean
            ss = np.where(fin[m], ss + d * d, ss)
        sd = np.where(n < 2, np.nan, np.sqrt(ss / (dn - 1.0)))
        pexc = np.stack([(fin & (v > np.float64(lim))).sum(axis=0).astype(np.float64) / dn for lim in limits]) if len(limits) else np.zeros((0, v.shape[1]))
        # ascending, ties in member order (a stable sort: -0.0 and +0.0 are equal); members that are not finite go last and are never read
        xs = np.sort(np.where(fin, v, np.inf), axis=0, kind="stable")
        quant = []
        for p in levels:
            pos = np.float64(p) * (dn - 1.0)
            fl = np.floor(pos)
            k = np.clip(fl.astype(np.int64), 0, max(nens - 1, 0))
            last = k >= n - 1
            x0 = np.take_along_axis(xs, np.where(last, np.maximum(n - 1, 0), k)[None], axis=0)[0]
            x1 = np.take_along_axis(xs, np.minimum(k + 1, nens - 1)[None], axis=0)[0]
            g = pos - fl
            quant.append(np.where(n == 0, np.nan, np.where(last, x0, x0 + g * (x1 - x0))))
    out = dict(nfin=n.astype(np.int32).reshape(shape), mean=mean.reshape(shape), sd=sd.reshape(shape), min=lo.reshape(shape), max=hi.reshape(shape),
               pexc=pexc.reshape((len(limits),) + shape), nbad=int((n < nens).sum()))
    out["quant"] = np.stack(quant).reshape((len(levels),) + shape) if len(levels) else np.zeros((0,) + shape)
    return out


def same_bits(got, want, what):
    """byte for byte, except that any NaN stands for any NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind != "f":
        assert got.tobytes() == want.tobytes(), what
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaN pattern")
    assert got[~nan].tobytes() == want[~nan].tobytes(), (what, int((got[~nan] != want[~nan]).sum()), np.signbit(got[~nan]).sum(), np.signbit(want[~nan]).sum())


def check_statistics(got, want, pre=""):
    """got: the maps of a call (keys with prefix `pre`), want: restate(); returns the number of sd values 1 ulp from numpy's"""
    for key in ("mean", "min", "max", "nfin", "quant"):
        if pre + key in got:
            same_bits(got[pre + key], want[key], pre + key)
    if pre + "sd" not in got:
        return 0
    sd, ref = got[pre + "sd"], want["sd"]
    fin = np.isfinite(ref)
    assert (np.isnan(sd) == np.isnan(ref)).all() and (np.isfinite(sd) == fin).all(), pre + "sd"
    assert (np.abs(sd[fin] - ref[fin]) <= np.spacing(ref[fin])).all(), pre + "sd"
    return int((sd[fin] != ref[fin]).sum())


_cache = {}


def ens_case(eng, deck, mode):
    """the forecast case of tests/test_gpu_field_forecast.py (shared with that module) and one ensemble call over its sets"""
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField
        c = case(eng, deck, mode)
        fx, free = c["fx"], c["free"]
        # the members: theta as the sets of the forecast hold it, read, not recomputed
        thetas = np.array([[getattr(Pk, name) for name in free] for Pk in c["sets"]])
        ref = c["out"]["s_all"]
        # limits: the bits of one member's value at one output (the strict >), a value between the members, one above all
        limits = np.array([ref[0].ravel()[7], ref[len(ref) - 1].ravel()[41], 0.5 * (ref.min() + ref.max()), 2.0 * np.abs(ref).max()])
        other = WellField(fx["wells"], fx["locations"], fx["times"])
        before = other.drawdown(c["plan"], fx["z"])
        field = WellField(fx["wells"], fx["locations"], fx["times"])
        out = field.ensemble(c["plan"], free, thetas, fx["z"], quantiles=LEVELS, limits=limits, all_maps=True, with_stats=True)
        after = other.drawdown(c["plan"], fx["z"])
        other.close()
        _cache[(deck, mode)] = dict(c=c, thetas=thetas, limits=limits, field=field, out=out, before=before, after=after)
    return _cache[(deck, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_every_slot_is_the_existing_entry(eng, deck, mode):
    e = ens_case(eng, deck, mode)
    c, out = e["c"], e["out"]
    assert len(e["thetas"]) == len(c["sets"]) == len(out["s_all"]) == (9 if deck == DECKS[0] else 5) and out["s_all"][0].size == 60
    # the slots of ucf_field_forecast over the same sets ...
    assert out["s_all"].tobytes() == c["out"]["s_all"].tobytes() and out["ds_all"].tobytes() == c["out"]["ds_all"].tobytes()
    # ... ucf_field_drawdown on a fresh field and a fresh plan of every member ...
    for m, ref in enumerate(c["alone"]):
        assert out["s_all"][m].tobytes() == ref["s"].tobytes(), m
        assert out["ds_all"][m].tobytes() == ref["ds"].tobytes(), m
    assert out["s_all"][1].tobytes() != out["s_all"][2].tobytes()
    # ... the counters their sum
    assert out["stats"] == {key: sum(ref["stats"][key] for ref in c["alone"]) for key in out["stats"]}
    # the caller's plan maps the same bits before and after
    assert e["before"][0].tobytes() == e["after"][0].tobytes() == out["s_all"][0].tobytes()
    assert e["before"][1].tobytes() == e["after"][1].tobytes() == out["ds_all"][0].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_the_statistics_are_the_stated_arithmetic(eng, deck, mode):
    e = ens_case(eng, deck, mode)
    out, nens = e["out"], len(e["thetas"])
    off = 0
    for i, (pre, maps) in enumerate((("", "s_all"), ("d", "ds_all"))):
        want = restate(out[maps], LEVELS, e["limits"] if pre == "" else ())
        off += check_statistics(out, want, pre)
        assert out["nbad"][i] == want["nbad"] == 0 and (out[pre + "nfin"] == nens).all()
        # the textbook definition: within 4 ulp of the larger of the two order statistics it interpolates between
        xs = np.sort(out[maps], axis=0)
        for j, p in enumerate(LEVELS):
            k = int(np.floor(p * (nens - 1)))
            nb = np.maximum(np.abs(xs[k]), np.abs(xs[min(k + 1, nens - 1)]))
            err = np.abs(out[pre + "quant"][j] - np.quantile(out[maps], p, axis=0, method="linear"))
            assert (err <= 4.0 * np.spacing(nb)).all(), (pre, p, float((err / np.spacing(nb)).max()))
        # levels 0 and 1 are the extremes (no zero among these values: bit for bit)
        assert out[pre + "quant"][0].tobytes() == out[pre + "min"].tobytes() and out[pre + "quant"][3].tobytes() == out[pre + "max"].tobytes()
    print(f"[ensemble {deck} {mode}] sd / dsd values 1 ulp from numpy's square root: {off} of {2 * out['sd'].size}")
    same_bits(out["pexc"], restate(out["s_all"], (), e["limits"])["pexc"], "pexc")
    # the strict comparison: the member whose bits are the limit does not exceed it
    s = out["s_all"].reshape(nens, -1)
    for l, (m, at) in enumerate(((0, 7), (nens - 1, 41))):
        assert e["limits"][l].tobytes() == s[m, at].tobytes()
        assert out["pexc"][l].ravel()[at] == float((s[:, at] > s[m, at]).sum()) / nens < float((s[:, at] >= s[m, at]).sum()) / nens
    assert (out["pexc"][3] == 0.0).all() and (out["sd"] > 0.0).all() and (out["min"] < out["max"]).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_against_the_oracle(eng, deck, mode):
    e = ens_case(eng, deck, mode)
    out, fx = e["out"], e["c"]["fx"]
    for pre, ref_key, bound_key in (("", "s_all_ref", "bound_s"), ("d", "ds_all_ref", "bound_ds")):
        ref, bound = fx[ref_key], fx[bound_key]
        assert len(ref) == len(e["thetas"]) and (bound > 0.0).all()
        want = restate(ref, LEVELS, ())
        err = np.abs(out[pre + "mean"] - ref.mean(axis=0))
        lim = bound.mean(axis=0)
        print(f"[ensemble {deck} {mode}] {pre}mean: worst |mean - mean(ref)| / mean(bound) = {float((err / lim).max()):.3f}")
        assert (err <= lim).all(), (deck, mode, pre + "mean", float((err / lim).max()))
        b = bound.max(axis=0)
        for key in ("min", "max", "quant"):
            err = np.abs(out[pre + key] - want[key])
            print(f"[ensemble {deck} {mode}] {pre}{key}: worst |{key} - {key}(ref)| / max bound = {float((err / b).max()):.3f}")
            assert (err <= b).all(), (deck, mode, pre + key, float((err / b).max()))


# ---- the kernels at their edges, through ucf_debug_ensemble

def debug_ensemble(a, levels=(), limits=(), want=STATS, pexc=True):
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    nens, nout = a.shape
    q, lim = np.ascontiguousarray(levels, dtype=np.float64), np.ascontiguousarray(limits, dtype=np.float64)
    out = {k: np.full((len(q), nout) if k == "quant" else nout, -7, np.int32 if k == "nfin" else np.float64) for k in want}
    m = abi.UcfEnsembleMaps()
    for k in want:
        setattr(m, k, out[k].ctypes.data)
    if pexc and len(lim):
        out["pexc"] = np.full((len(lim), nout), -7.0)
    nbad = np.full(1, -7, np.int64)
    ucflib.check(so.ucf_debug_ensemble(nens, nout, a.ctypes.data, len(q), q.ctypes.data if len(q) else None, len(lim),
                                       lim.ctypes.data if len(lim) else None, C.byref(m), out["pexc"].ctypes.data if "pexc" in out else None,
                                       nbad.ctypes.data))
    out["nbad"] = int(nbad[0])
    return out


def synthetic(nens, nout, seed):
    """columns of every kind, by e % 12: plain; all NaN (n = 0); one finite member; two; NaN and +-Inf mixed in; all members
    equal; ties; +0.0 and -0.0 mixed (with a few +-1); the Wynn sentinel among the values; plain with one +Inf; descending
    integers; plain.  nout = 1 gets the kind seed % 12."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(nens, nout)) * 3.0
    for e in range(nout):
        kind = (e + (seed if nout == 1 else 0)) % 12
        colv = a[:, e]
        if kind == 1:
            colv[:] = np.nan
        elif kind in (2, 3):
            keep = rng.choice(nens, size=min(kind - 1, nens), replace=False)
            v = colv[keep].copy()
            colv[:] = np.nan
            colv[keep] = v
        elif kind == 4:
            colv[rng.random(nens) < 0.3] = np.nan
            colv[rng.random(nens) < 0.1] = np.inf
            colv[rng.random(nens) < 0.1] = -np.inf
        elif kind == 5:
            colv[:] = 2.0
        elif kind == 6:
            colv[:] = rng.integers(-2, 3, nens).astype(float)
        elif kind == 7:
            colv[:] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), nens)
        elif kind == 8:
            colv[rng.random(nens) < 0.25] = SENTINEL
        elif kind == 9:
            colv[rng.integers(nens)] = np.inf
        elif kind == 10:
            colv[:] = np.arange(nens, 0, -1.0)
    return a


@pytest.mark.parametrize("nens", [1, 2, 63, 64, 65, 256, 257, 512, 1024])
def test_kernel_edges(eng, nens):
    """every tile width (64 / 32 / 16 outputs for nens <= 256 / 512 / 1024) on both sides of each switch, member counts that are
    no multiple of the four a thread ranks at a time, one output, partial and several workgroups.  Levels whose pos is integral:
    0, 1, 0.5 for odd nens, 0.25 and 0.75 for nens = 65, 257; 1/3 is no binary fraction.  nens = 64 and 1024 run the full 16
    levels and 16 limits.  Limits with the bits of values that occur: 2.0, the zeros, the sentinel."""
    full = nens in (64, 1024)
    levels = np.linspace(0.0, 1.0, 16) if full else np.array([0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 1.0])
    limits = np.concatenate([[2.0, 0.0, -0.0, SENTINEL, -1.0, 1e300], np.linspace(-4.0, 4.0, 10)]) if full else np.array([2.0, 0.0, SENTINEL, -1.5])
    off = total = 0
    for nout in (1, 255, 256, 257, 540):
        a = synthetic(nens, nout, 1000 * nens + nout)
        got = debug_ensemble(a, levels, limits)
        want = restate(a, levels, limits)
        off += check_statistics(got, want)
        total += int(np.isfinite(want["sd"]).sum())
        same_bits(got["pexc"], want["pexc"], "pexc")
        assert got["nbad"] == want["nbad"] == int((np.isfinite(a).sum(axis=0) < nens).sum()), (nens, nout)
        if nout >= 12:
            assert (got["nfin"][1::12] == 0).all() and np.isnan(got["mean"][1::12]).all() and np.isnan(got["quant"][:, 1::12]).all()
            assert (got["nfin"][2::12] == 1).all() and np.isnan(got["sd"][2::12]).all() and not np.isnan(got["mean"][2::12]).any()
        # level 1 is max, bit for bit (x_{n-1} as it stands); level 0 is min in value: x_0 + 0 * (x_1 - x_0) turns a -0.0 into +0.0
        same_bits(got["quant"][-1], got["max"], "quant[-1] = max")
        nan = np.isnan(got["min"])
        assert (np.isnan(got["quant"][0]) == nan).all() and (got["quant"][0][~nan] == got["min"][~nan]).all()
    print(f"[ensemble edges nens={nens}] sd values 1 ulp from numpy's square root: {off} of {total}")
    # asking for less changes nothing of what is asked for
    only = debug_ensemble(a, levels, (), want=("quant",))
    assert sorted(only) == ["nbad", "quant"] and only["nbad"] == got["nbad"]
    same_bits(only["quant"], got["quant"], "quant alone")
    only = debug_ensemble(a, (), limits, want=("mean", "nfin"))
    same_bits(only["mean"], got["mean"], "mean alone")
    same_bits(only["pexc"], got["pexc"], "pexc without levels")
    assert only["nfin"].tobytes() == got["nfin"].tobytes()


# ---- real calls again

def test_members_that_are_not_finite_in_a_real_call(eng):
    """one well at the origin; location 0 at distance NAN_R, first time NAN_T (tests/test_gpu_field_forecast.py): the drawdown
    there at z = 145.7 is NaN under every set of the forecast, so no member is finite: nfin = 0, every statistic NaN, counted in
    nbad.  Every other output is the same call without that location."""
    from unconfined_amd import WellField, forecast_sets
    _, _, P = load_deck("neuman74_partpen")
    free = ["Kr", "kappa", "Ss", "Sy"]
    thetas = np.array([[getattr(Pk, n) for n in free] for Pk in forecast_sets(P, free, [P.Kr, P.kappa, P.Ss, P.Sy], 1e-3)])
    z, times = np.array([145.7, 100.0]), np.array([NAN_T, 1.0, 100.0])
    plan = eng.Plan(P, mode="fast")
    well = [(0.0, 0.0, 1.0, 0.0)]
    both = WellField(well, [(NAN_R, 0.0), (0.0, 85.1)], times)
    rest = WellField(well, [(0.0, 85.1)], times)
    kw = dict(quantiles=LEVELS, limits=[0.0, 0.01], all_maps=True)
    out, ref = both.ensemble(plan, free, thetas, z, **kw), rest.ensemble(plan, free, thetas, z, **kw)
    assert not np.isfinite(out["s_all"][:, 0, 0, 0]).any()
    assert out["nfin"][0, 0, 0] == 0
    for key in ("mean", "sd", "min", "max"):
        assert np.isnan(out[key][0, 0, 0]), key
    assert np.isnan(out["quant"][:, 0, 0, 0]).all() and np.isnan(out["pexc"][:, 0, 0, 0]).all()
    for i, pre in enumerate(("", "d")):
        assert out["nbad"][i] == (out[pre + "nfin"] < len(thetas)).sum() >= (1 if pre == "" else 0)
        check_statistics(out, restate(out[pre + "s_all"], LEVELS, ()), pre)
        assert ref["nbad"][i] == (out[pre + "nfin"][:, 1:, :] < len(thetas)).sum()
    same_bits(out["pexc"], restate(out["s_all"], (), kw["limits"])["pexc"], "pexc")
    # the later times are finite everywhere
    assert (out["nfin"][1:] == len(thetas)).all() and np.isfinite(out["mean"][1:]).all()
    for key in [p + k for p in ("", "d") for k in STATS + ("s_all",)] + ["pexc"]:
        axis = out[key].ndim - 2                       # [..., nt, nloc, nz]
        same_bits(np.take(out[key], [1], axis=axis), ref[key], key)
    both.close(); rest.close(); plan.close()


def test_a_refused_member_is_named_before_any_launch(eng):
    """a location inside a well bore: what ucf_field_group refuses, found in the checks of member 0, which is named with its
    parameter values; nothing was allocated or launched"""
    from unconfined_amd import WellField
    from unconfined_amd import lib as ucflib
    _, _, P = load_deck("c1_theis")
    plan = eng.Plan(P, mode="fast")
    field = WellField([(0.0, 0.0, 1.0, 0.0)], [(10.0, 0.0), (0.5 * P.rw, 0.0)], [1.0, 10.0])
    thetas = np.array([[P.Kr, P.Ss], [1.1 * P.Kr, 0.9 * P.Ss]])
    with pytest.raises(ucflib.UcfError) as err:
        field.ensemble(plan, ["Kr", "Ss"], thetas, [0.5 * P.b])
    msg = err.value.message
    assert err.value.status == -11 and "member 0 (Kr=" in msg and ", Ss=" in msg and "location 1" in msg and "inside its bore" in msg, msg
    assert field.alloc_count() == 0
    field.close(); plan.close()


def test_repetition(eng):
    """a second call allocates nothing and gives the same bytes; fewer members afterwards allocate nothing; without the
    derivative's maps the drawdown's are unchanged"""
    from unconfined_amd import WellField, ensemble_draw
    fx = np.load(os.path.join(GOLD, "field_forecast_neuman74_partpen.npz"))
    _, _, P = load_deck("neuman74_partpen")
    free, z = [str(n) for n in fx["free"]], fx["z"]
    thetas = ensemble_draw(fx["theta"], fx["cov"], 12, seed=5)
    plan = eng.Plan(P, mode="fast")
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    kw = dict(quantiles=(0.05, 0.5, 0.95), limits=[0.02], all_maps=True)
    a = field.ensemble(plan, free, thetas, z, **kw)
    n = field.alloc_count()
    b = field.ensemble(plan, free, thetas, z, **kw)
    assert n > 0 and field.alloc_count() == n
    assert sorted(a) == sorted(b) and "stats" not in a
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["nbad"].tolist() == [0, 0] and (a["s_all"][0] != a["s_all"][1]).any()
    check_statistics(a, restate(a["s_all"], kw["quantiles"], kw["limits"]))
    check_statistics(a, restate(a["ds_all"], kw["quantiles"], ()), "d")
    # fewer members: their maps are the first rows of the larger call, nothing is allocated
    c = field.ensemble(plan, free, thetas[:5], z, **kw)
    assert field.alloc_count() == n
    assert c["s_all"].tobytes() == a["s_all"][:5].tobytes() and c["ds_all"].tobytes() == a["ds_all"][:5].tobytes()
    check_statistics(c, restate(c["s_all"], kw["quantiles"], kw["limits"]))
    # a NULL ds: the s outputs are what they were
    d = field.ensemble(plan, free, thetas, z, derivative=False, **kw)
    assert field.alloc_count() == n
    assert sorted(d) == sorted(k for k in a if not k.startswith("d"))
    for key in d:
        assert d[key].tobytes() == a[key].tobytes() or key == "nbad", key
    assert d["nbad"][0] == a["nbad"][0]
    field.close(); plan.close()
