"""ucf_field_ensemble_weighted on the GPU.

The kernels alone, through ucf_debug_ensemble_weighted on synthetic data: nfin, mean, min, max, quant, pexc and nbad bit for bit
against the arithmetic that include/ucf.h states, restated in numpy (tests/ensemble_weighted_restate.py, itself held to numpy's
weighted inverted_cdf by tests/test_ensemble_weights_host.py); sd within 1 ulp of numpy's square root; the payload of a NaN is
not compared.  With equal weights every statistic but quant has the bits of the unweighted kernels (ucf_debug_ensemble).

End to end on the forecast fixtures that tests/test_gpu_field_ensemble.py uses (60 outputs, 9 / 5 members, both flavours): a
launched slot is the slot of the unweighted call bit for bit, a member of weight 0 is not launched.  Against the oracle nothing
is chosen: each slot lies within the fixture's bound[m] of the oracle's value, hence |mean - weighted mean(ref)| <= sum_m u_m
bound_m / U by the triangle inequality; min and max move by at most b = max_m bound_m; and the weighted inverse distribution
function selects the SAME member from the device's values as from the reference's wherever the reference value of the selected
member lies farther than 2 b from every other member's, because the sets of members below and above it are then the same -- so
there the quantile moves by at most b too.  Cells where the reference does not separate the members that far are skipped; they
are counted, and at most 10 % of the (level, output) pairs may be (the fixtures have none)."""
import ctypes as C

import numpy as np
import pytest

from ensemble_weighted_restate import order_statistic, quantise, restate_weighted
from test_gpu_field_ensemble import LEVELS, SENTINEL, STATS, check_statistics, debug_ensemble, ens_case, same_bits, synthetic
from test_gpu_field_forecast import DECKS, MODES

pytestmark = pytest.mark.gpu

NENS = [1, 2, 3, 4, 5, 63, 64, 65, 256, 257, 512, 513, 1024]
E2E_LEVELS = LEVELS + (0.25, 0.75)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def tile(nens):
    return 64 if nens <= 256 else 32 if nens <= 512 else 16


def debug_weighted(a, w, levels=(), limits=(), want=STATS, pexc=True):
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    a, w = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    nens, nout = a.shape
    q, lim = np.ascontiguousarray(levels, dtype=np.float64), np.ascontiguousarray(limits, dtype=np.float64)
    out = {k: np.full((len(q), nout) if k == "quant" else nout, -7, np.int32 if k == "nfin" else np.float64) for k in want}
    m = abi.UcfEnsembleMaps()
    for k in want:
        setattr(m, k, out[k].ctypes.data)
    if pexc and len(lim):
        out["pexc"] = np.full((len(lim), nout), -7.0)
    nbad = np.full(1, -7, np.int64)
    ucflib.check(so.ucf_debug_ensemble_weighted(nens, nout, a.ctypes.data, w.ctypes.data, len(q), q.ctypes.data if len(q) else None, len(lim),
                                                lim.ctypes.data if len(lim) else None, C.byref(m), out["pexc"].ctypes.data if "pexc" in out else None,
                                                nbad.ctypes.data))
    out["nbad"] = int(nbad[0])
    return out


def weights_of(nens, seed, dyadic):
    """random weights over several decades with zeros and weights too small to count among them, or (dyadic) weights from
    {0, 1/4, 1/2, 1}: then 0.25 U, 0.5 U and 0.75 U are exact and land on interval ends"""
    rng = np.random.default_rng(seed)
    if dyadic:
        w = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), nens)
    else:
        w = rng.random(nens) * 10.0 ** rng.uniform(-6, 0, nens)
        w[rng.random(nens) < 0.2] = 0.0
        w[rng.random(nens) < 0.1] = 1e-13                   # below 2^-33 of the largest: u = 0
        w[rng.random(nens) < 0.2] = 0.125                   # equal weights among the others
    w[rng.integers(nens)] = 1.0
    return w * 3.7


def wsynthetic(nens, nout, w, seed):
    """values over several decades and columns of every kind, by e % 12: plain; every member NaN; exactly one member in F; two; the
    only finite members have u = 0; +-Inf mixed in; the Wynn sentinel among the values; ties between members of different
    weight; +0.0 and -0.0 mixed (a tie of zeros); NaN mixed in; all members equal; plain.  nout = 1 gets the kind seed % 12."""
    rng = np.random.default_rng(seed)
    u, _ = quantise(w)
    a = rng.normal(size=(nens, nout)) * 10.0 ** rng.uniform(-5, 5, (nens, nout))
    live = np.flatnonzero(u > 0)
    for e in range(nout):
        kind = (e + (seed if nout == 1 else 0)) % 12
        c = a[:, e]
        if kind == 1:
            c[:] = np.nan
        elif kind in (2, 3):
            keep = rng.choice(live, size=min(kind - 1, len(live)), replace=False)
            v = c[keep].copy()
            c[:] = np.nan
            c[rng.random(nens) < 0.3] = np.inf
            c[keep] = v
        elif kind == 4:
            c[u > 0] = np.nan
        elif kind == 5:
            c[rng.random(nens) < 0.15] = np.inf
            c[rng.random(nens) < 0.15] = -np.inf
        elif kind == 6:
            c[rng.random(nens) < 0.25] = SENTINEL
        elif kind == 7:
            c[:] = rng.integers(-2, 3, nens).astype(float)
        elif kind == 8:
            c[:] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), nens)
        elif kind == 9:
            c[rng.random(nens) < 0.3] = np.nan
        elif kind == 10:
            c[:] = 2.0
    return a, u


@pytest.mark.parametrize("nens", NENS)
def test_kernel_edges(eng, nens):
    """every tile width (64 / 32 / 16 outputs for nens <= 256 / 512 / 1024) on both sides of each switch, the remainders 0..3 of
    the four members a thread owns per pass and a second pass of the member loop, a partial tile, a partial 256-thread block and
    a second block.  Limits with the bits of values that occur (the strict >): 2.0, the zeros, the sentinel, one member's value."""
    T = tile(nens)
    levels = np.array([0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 1.0])
    off = total = 0
    for i, nout in enumerate((1, T - 1, T, T + 1, 255, 256, 257)):
        seed = 1000 * nens + nout
        w = weights_of(nens, seed, dyadic=bool(i & 1))
        a, u = wsynthetic(nens, nout, w, seed)
        live = np.isfinite(a) & (u > 0)[:, None]
        limits = np.array([2.0, 0.0, SENTINEL, -1.5, a[live][0] if live.any() else 1.0])
        got = debug_weighted(a, w, levels, limits)
        want = restate_weighted(a, u, levels, limits)
        off += check_statistics(got, want)
        total += int(np.isfinite(want["sd"]).sum())
        same_bits(got["pexc"], want["pexc"], "pexc")
        assert got["nbad"] == want["nbad"] == int((live.sum(axis=0) < (u > 0).sum()).sum()), (nens, nout)
        if nout >= 12:
            for kind in (1, 4):                          # no member in F: every member NaN, or the finite ones have u = 0
                assert (got["nfin"][kind::12] == 0).all() and np.isnan(got["mean"][kind::12]).all() and np.isnan(got["quant"][:, kind::12]).all()
                assert np.isnan(got["pexc"][:, kind::12]).all() and np.isnan(got["min"][kind::12]).all()
            assert (got["nfin"][2::12] == 1).all() and np.isnan(got["sd"][2::12]).all() and not np.isnan(got["mean"][2::12]).any()
            assert (got["quant"][:, 2::12] == got["min"][2::12]).all() and (got["min"][2::12] == got["max"][2::12]).all()
        # level 0 is min and level 1 is max in value (a tie of zeros may return the other zero: the stable order decides)
        nan = np.isnan(got["min"])
        assert (np.isnan(got["quant"][[0, -1]]) == nan).all()
        assert (got["quant"][0][~nan] == got["min"][~nan]).all() and (got["quant"][-1][~nan] == got["max"][~nan]).all()
        # a call repeated gives the same bytes
        again = debug_weighted(a, w, levels, limits)
        for key in got:
            assert np.asarray(got[key]).tobytes() == np.asarray(again[key]).tobytes(), key
    print(f"[weighted ensemble edges nens={nens}] sd values 1 ulp from numpy's square root: {off} of {total}")
    # asking for less changes nothing of what is asked for
    only = debug_weighted(a, w, levels, (), want=("quant",))
    assert sorted(only) == ["nbad", "quant"] and only["nbad"] == got["nbad"]
    same_bits(only["quant"], got["quant"], "quant alone")
    only = debug_weighted(a, w, (), limits, want=("mean", "nfin"))
    same_bits(only["mean"], got["mean"], "mean alone")
    same_bits(only["pexc"], got["pexc"], "pexc without levels")


@pytest.mark.parametrize("nens", NENS)
def test_equal_weights_are_the_unweighted_kernels(eng, nens):
    """all weights equal: every u is 2^32, and mean, sd, min, max, nfin, pexc and nbad come out bit for bit as ucf_debug_ensemble
    gives them on the same data; quant is the order statistic of index ceil(p n) - 1 (0 at p = 0) of the stable sort"""
    T = tile(nens)
    levels = np.array([0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.75, 1.0])
    limits = np.array([2.0, 0.0, -0.0, SENTINEL, -1.5])
    for nout in (1, T + 1, 257):
        a = synthetic(nens, nout, 2000 * nens + nout)
        got = debug_weighted(a, np.full(nens, 0.3), levels, limits)
        ref = debug_ensemble(a, levels, limits)
        for key in ("mean", "sd", "min", "max", "nfin", "pexc"):
            same_bits(got[key], ref[key], key)
        assert got["nbad"] == ref["nbad"]
        same_bits(got["quant"], order_statistic(a, levels), "quant")


def test_levels_on_interval_ends(eng):
    """weights 1, 1, 2 on ascending values: U = 2^33 and the intervals end at 2^31, 2^32, 2^33, so p = 0.25 and p = 0.5 sit on an
    end and belong to the member below it; the next double above belongs to the member above"""
    up = lambda p: np.nextafter(p, 1.0)
    levels = np.array([0.0, 0.25, up(0.25), 0.5, up(0.5), 1.0])
    a = np.array([[1.0, 30.0, -0.0], [2.0, 10.0, 0.0], [3.0, 20.0, 5.0]])
    w = np.array([1.0, 1.0, 2.0])
    got = debug_weighted(a, w, levels, ())
    assert got["quant"][:, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 3.0, 3.0]
    # column 1 in value order: member 1 (u 2^31), member 2 (2^32), member 0 (2^31): the ends are 2^31 and 3 2^31
    assert got["quant"][:, 1].tolist() == [10.0, 10.0, 20.0, 20.0, 20.0, 30.0]
    # column 2: a tie of zeros keeps its member order, -0.0 first
    assert np.signbit(got["quant"][0, 2]) and got["quant"][1, 2] == 0.0 and np.signbit(got["quant"][1, 2])
    assert not np.signbit(got["quant"][2, 2]) and got["quant"][3, 2] == 0.0 and got["quant"][4, 2] == 5.0
    same_bits(got["quant"], restate_weighted(a, quantise(w)[0], levels, ())["quant"], "quant")


# ---- end to end

_cache = {}


def e2e_weights(nens):
    """two members get u = 0: member 0, so that the scratch plan starts at a later member, by a weight of 0, and member
    nens - 2 by a weight below 2^-33 of the largest"""
    w = 0.9 ** np.arange(nens)
    w[0], w[nens - 2] = 0.0, 1e-13
    return w


def weighted_case(eng, deck, mode):
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField
        e = ens_case(eng, deck, mode)
        fx = e["c"]["fx"]
        field = WellField(fx["wells"], fx["locations"], fx["times"])
        w = e2e_weights(len(e["thetas"]))
        kw = dict(quantiles=E2E_LEVELS, limits=e["limits"], all_maps=True, with_stats=True)
        out = field.ensemble(e["c"]["plan"], e["c"]["free"], e["thetas"], fx["z"], weights=w, **kw)
        _cache[(deck, mode)] = dict(e=e, field=field, w=w, kw=kw, out=out)
    return _cache[(deck, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_a_member_of_weight_zero_is_not_launched(eng, deck, mode):
    wc = weighted_case(eng, deck, mode)
    e, out, w = wc["e"], wc["out"], wc["w"]
    nens = len(w)
    u, ess = quantise(w)
    assert out["u"].tobytes() == u.tobytes() and out["ess"] == ess and (u == 0).sum() == 2 and out["nlaunched"] == nens - 2
    for m in range(nens):
        for key in ("s_all", "ds_all"):
            if u[m] == 0:
                assert np.isnan(out[key][m]).all(), (key, m)
            else:
                assert out[key][m].tobytes() == e["out"][key][m].tobytes(), (key, m)
    alone = e["c"]["alone"]
    assert out["stats"] == {key: sum(alone[m]["stats"][key] for m in range(nens) if u[m] > 0) for key in out["stats"]}
    # the statistics are the stated arithmetic on the returned slots
    off = 0
    for i, (pre, maps) in enumerate((("", "s_all"), ("d", "ds_all"))):
        want = restate_weighted(out[maps], u, E2E_LEVELS, e["limits"] if pre == "" else ())
        off += check_statistics(out, want, pre)
        assert out["nbad"][i] == want["nbad"] == 0 and (out[pre + "nfin"] == nens - 2).all()
        assert (out[pre + "min"] <= out[pre + "quant"][2]).all() and (out[pre + "quant"][2] <= out[pre + "max"]).all()
        if pre == "":
            same_bits(out["pexc"], want["pexc"], "pexc")
    print(f"[weighted ensemble {deck} {mode}] sd / dsd values 1 ulp from numpy's square root: {off} of {2 * out['sd'].size}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_unit_weights_are_the_unweighted_call(eng, deck, mode):
    wc = weighted_case(eng, deck, mode)
    e = wc["e"]
    nens = len(wc["w"])
    n0 = wc["field"].alloc_count()
    kw = dict(wc["kw"], quantiles=LEVELS)
    out = wc["field"].ensemble(e["c"]["plan"], e["c"]["free"], e["thetas"], e["c"]["fx"]["z"], weights=np.ones(nens), **kw)
    assert wc["field"].alloc_count() == n0                                          # the buffers of the weighted call before it serve
    assert out["nlaunched"] == nens and out["ess"] == float(nens) and (out["u"] == 2 ** 32).all()
    for key in e["out"]:
        if key in ("quant", "dquant"):
            same_bits(out[key], order_statistic(out["s_all" if key == "quant" else "ds_all"], LEVELS), key)
        elif key == "stats":
            assert out[key] == e["out"][key]
        else:
            assert out[key].tobytes() == e["out"][key].tobytes(), key


def selected_and_separated(ref, u, p, b):
    """per output of ref [nens][nout]: the value that the weighted inverse distribution function selects at level p, and whether
    it lies farther than 2 b from the value of every other member with u > 0"""
    live = np.flatnonzero(u > 0)
    x, ui = ref[live], np.array([int(v) for v in u[live]], dtype=np.int64)
    order = np.argsort(x, axis=0, kind="stable")
    xs, us = np.take_along_axis(x, order, axis=0), ui[order]
    cum = np.cumsum(us, axis=0)
    tgt = np.float64(p) * np.float64(cum[-1])
    k = (cum.astype(np.float64) < tgt).sum(axis=0)
    val = np.take_along_axis(xs, k[None], axis=0)[0]
    gap = np.abs(xs - val)
    gap[k, np.arange(xs.shape[1])] = np.inf
    return val, gap.min(axis=0) > 2.0 * b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_against_the_oracle(eng, deck, mode):
    wc = weighted_case(eng, deck, mode)
    out, fx = wc["out"], wc["e"]["c"]["fx"]
    u, _ = quantise(wc["w"])
    du = u.astype(np.float64)
    live = u > 0
    skipped = cells = 0
    for pre, ref_key, bound_key in (("", "s_all_ref", "bound_s"), ("d", "ds_all_ref", "bound_ds")):
        ref, bound = fx[ref_key], fx[bound_key]
        shape = ref.shape[1:]
        assert len(ref) == len(u) and (bound > 0.0).all()
        wmean = np.tensordot(du, ref, axes=1) / du.sum()
        lim = np.tensordot(du, bound, axes=1) / du.sum()
        err = np.abs(out[pre + "mean"] - wmean)
        print(f"[weighted ensemble {deck} {mode}] {pre}mean: worst |mean - weighted mean(ref)| / bound = {float((err / lim).max()):.3f}")
        assert (err <= lim).all(), (deck, mode, pre + "mean", float((err / lim).max()))
        b = bound[live].max(axis=0)
        for key, want in (("min", ref[live].min(axis=0)), ("max", ref[live].max(axis=0))):
            err = np.abs(out[pre + key] - want)
            print(f"[weighted ensemble {deck} {mode}] {pre}{key}: worst |{key} - {key}(ref)| / max bound = {float((err / b).max()):.3f}")
            assert (err <= b).all(), (deck, mode, pre + key, float((err / b).max()))
        for j, p in enumerate(E2E_LEVELS):
            val, ok = selected_and_separated(ref.reshape(len(u), -1), u, p, b.ravel())
            err = np.abs(out[pre + "quant"][j].ravel() - val)
            assert (err[ok] <= b.ravel()[ok]).all(), (deck, mode, pre + "quant", p, float((err / b.ravel())[ok].max()))
            skipped += int((~ok).sum())
            cells += ok.size
        assert shape == out[pre + "mean"].shape
    print(f"[weighted ensemble {deck} {mode}] quantile cells skipped for want of separation in the reference: {skipped} of {cells}")
    assert skipped <= 0.1 * cells


def test_repetition(eng):
    """a second call allocates nothing and gives the same bytes; the weights are a buffer of the field, allocated once"""
    wc = weighted_case(eng, DECKS[1], "fast")
    e, field = wc["e"], wc["field"]
    args = (e["c"]["plan"], e["c"]["free"], e["thetas"], e["c"]["fx"]["z"])
    a = field.ensemble(*args, weights=wc["w"], **wc["kw"])
    n = field.alloc_count()
    b = field.ensemble(*args, weights=wc["w"], **wc["kw"])
    assert n > 0 and field.alloc_count() == n
    for key in a:
        if key in ("stats", "ess", "nlaunched"):
            assert a[key] == b[key] == wc["out"][key], key
        else:
            assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])) and a[key][~np.isnan(a[key])].tobytes() == b[key][~np.isnan(b[key])].tobytes(), key
    # a fresh field: the unweighted call allocates one buffer fewer than the weighted one (u)
    from unconfined_amd import WellField
    fx = e["c"]["fx"]
    f1, f2 = (WellField(fx["wells"], fx["locations"], fx["times"]) for _ in range(2))
    f1.ensemble(*args, **wc["kw"])
    f2.ensemble(*args, weights=np.ones(len(wc["w"])), **wc["kw"])
    assert f2.alloc_count() == f1.alloc_count() + 1
    f1.close(); f2.close()
