"""ucf_field_sobol on the GPU.

The kernel alone, through ucf_debug_sobol on synthetic member maps: bit for bit (tobytes, NaN included: the statement names the
NaN) the arithmetic that include/ucf.h states, restated in numpy (tests/field_sobol_restate.py, itself held to hand-made columns,
to exact rational arithmetic and to the Ishigami function by tests/test_field_sobol_host.py), for every instantiation NPAR =
1 .. 8, the smallest and the largest nbase, and nout below, at and across the boundaries of a wave and of a workgroup.

End to end on the fixtures of tests/test_gpu_field.py (4 wells in 2 start-time groups, 5 locations, 6 times, 2 depths, both
flavours) with the design sobol_design(theta, diag(0.04, 0.04), 3, seed=1) of Kr and Ss, 12 members: `all` is, bit for bit,
the `all` of ucf_field_ensemble on a fresh field with the same thetas -- tests/test_gpu_field_ensemble.py holds those bits to
ucf_field_drawdown and tests/test_gpu_field.py holds that to the oracle, so nothing further is chosen here -- and every
statistic and nbad is what ucf_debug_sobol makes of `all`, bit for bit, for s and for ds."""
import ctypes as C
import os

import numpy as np
import pytest

import field_sobol_restate as R
from golden_util import GOLD, load_deck
from test_gpu_field import MODES, eng  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DECKS = ["c1_theis", "neuman74_partpen"]
FREE = ["Kr", "Ss"]
SENTINEL = -999999.9
KEYS = ("S", "ST", "seS", "seST", "mean", "var", "nrow")


# ---- the kernel alone

def debug_sobol(a, npar, nbase, want=KEYS):
    """ucf_debug_sobol on a [(npar + 2) nbase][nout]: the maps in `want` (the others are not asked for) and nbad"""
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[0] == (npar + 2) * nbase
    nout = a.shape[1]
    out = {k: np.full((npar, nout) if k in KEYS[:4] else (nout,), -7, np.int32 if k == "nrow" else np.float64) for k in want}
    maps = abi.UcfSobolMaps(*(out[k].ctypes.data if k in out else None for k in ("S", "ST", "seS", "seST", "mean", "var", None, "nrow")))
    nbad = np.full(1, -1, np.int64)
    ucflib.check(so.ucf_debug_sobol(npar, nbase, nout, a.ctypes.data, C.byref(maps), nbad.ctypes.data))
    out["nbad"] = int(nbad[0])
    return out


NKINDS = 11


def columns(npar, nbase, nout, seed):
    """a [(npar + 2) nbase][nout], the column of output e of kind (e + seed) % 11, the positions random: plain; NaN in A only; in B
    only; in one AB block only; +-inf; every row incomplete; exactly one complete row; a constant column; a dead parameter (its AB
    block has the bits of A); zeros of both signs (with a few +-1); the Wynn sentinel among the values"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(npar + 2, nbase, nout)) + 0.6
    for e in range(nout):
        kind, c = (e + seed) % NKINDS, a[:, :, e]
        r, j = int(rng.integers(nbase)), int(rng.integers(npar))
        if kind == 1:
            c[0, r] = np.nan
        elif kind == 2:
            c[1, r] = np.nan
        elif kind == 3:
            c[2 + j, r] = np.nan
        elif kind == 4:
            c[int(rng.integers(npar + 2)), r] = np.inf if rng.random() < 0.5 else -np.inf
        elif kind == 5:
            c[rng.integers(npar + 2, size=nbase), np.arange(nbase)] = np.nan
        elif kind == 6:
            c[rng.integers(npar + 2, size=nbase), np.arange(nbase)] = np.nan
            c[:, r] = rng.normal(size=npar + 2)
        elif kind == 7:
            c[:] = 1.25
        elif kind == 8:
            c[2 + j] = c[0]
        elif kind == 9:
            c[:] = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), c.shape)
        elif kind == 10:
            c[int(rng.integers(npar + 2)), r] = SENTINEL
    return a.reshape((npar + 2) * nbase, nout)


def where_differs(got, want):
    bits = np.int32 if got.dtype == np.int32 else np.int64
    return np.argwhere(got.view(bits) != want.view(bits))[:5].tolist()


@pytest.mark.parametrize("npar,nbase,nout", [(1, 2, 1), (2, 3, 65), (3, 5, 257), (4, 130, 1000), (5, 2, 64), (6, 7, 255), (7, 3, 513), (8, 1024, 64)])
def test_the_kernel_is_the_restatement(eng, npar, nbase, nout):  # noqa: F811
    a = columns(npar, nbase, nout, seed=100 * npar + nbase)
    want = R.sobol(a, npar, nbase)
    got = debug_sobol(a, npar, nbase)
    for key in KEYS:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        assert got[key].tobytes() == want[key].tobytes(), (key, npar, nbase, nout, where_differs(got[key], want[key]))
    assert got["nbad"] == want["nbad"] == int((want["nrow"] < nbase).sum())
    if nout >= NKINDS:
        # every kind of column is there, and does what it is there for
        assert want["nbad"] > 0 and (want["nrow"] == nbase).any() and np.isnan(want["S"]).any() and np.isfinite(want["seS"]).any()
        assert (want["nrow"] == 0).any() and (want["nrow"] == 1).any()
        assert ((want["ST"] == 0.0) & (want["seST"] == 0.0) & (want["S"] == 0.0)).any(), "no dead parameter"
    # only S is asked for: the same bits, and nothing else is touched
    only = debug_sobol(a, npar, nbase, want=("S",))
    assert sorted(only) == ["S", "nbad"] and only["S"].tobytes() == got["S"].tobytes() and only["nbad"] == got["nbad"]
    # a call repeated gives the same bytes
    again = debug_sobol(a, npar, nbase)
    assert all(again[key].tobytes() == got[key].tobytes() for key in KEYS) and again["nbad"] == got["nbad"]


def test_the_kernel_on_the_hand_made_columns(eng):  # noqa: F811
    """the columns of tests/test_field_sobol_host.py with their written-out values, on the device"""
    from test_field_sobol_host import CASES, CLAMPED, WITH_SENTINEL, check_case, column
    for name, npar, nbase, rows, want in CASES:
        got = debug_sobol(column(rows), npar, nbase)
        check_case(name, got, want, npar)
        assert got["nbad"] == int(want["nrow"] < nbase), name
    # the two columns that are not exact: the bits of the restatement, which the host test holds to rational arithmetic
    for rows, nbase in ((CLAMPED, 3), (WITH_SENTINEL, 2)):
        got, want = debug_sobol(column(rows), 1, nbase), R.sobol(column(rows), 1, nbase)
        for key in KEYS:
            assert got[key].tobytes() == want[key].tobytes(), (key, got[key].tolist(), want[key].tolist())
    clamped = debug_sobol(column(CLAMPED), 1, 3)
    assert clamped["seST"][0, 0] == 0.0 and not np.signbit(clamped["seST"][0, 0])


# ---- end to end

_cache = {}


def sobol_case(eng, deck, mode, free=FREE):  # noqa: F811
    """(fixture, plan, the design, the member maps of ucf_field_ensemble on a fresh field) -- once per deck, flavour and free set"""
    key = (deck, mode, tuple(free))
    if key not in _cache:
        from unconfined_amd import WellField, sobol_design
        fx = np.load(os.path.join(GOLD, f"field_{deck}.npz"))
        _, _, P = load_deck(deck)
        plan = eng.Plan(P, mode=mode)
        theta = np.array([getattr(P, name) for name in free])
        thetas = sobol_design(theta, np.diag([0.04] * len(free)), 3, seed=1)
        fresh = WellField(fx["wells"], fx["locations"], fx["times"])
        ens = fresh.ensemble(plan, free, thetas, fx["z"], quantiles=None, all_maps=True)
        fresh.close()
        _cache[key] = dict(fx=fx, P=P, plan=plan, thetas=thetas, s_all=ens["s_all"], ds_all=ens["ds_all"])
    return _cache[key]


def check_against_debug(res, npar, nbase):
    """every statistic and nbad of both maps is ucf_debug_sobol of `all`, bit for bit"""
    for i, pre in enumerate(("", "d")):
        ref = debug_sobol(getattr(res, pre + "all").reshape((npar + 2) * nbase, -1), npar, nbase)
        for attr, key in (("S", "S"), ("ST", "ST"), ("se_S", "seS"), ("se_ST", "seST"), ("mean", "mean"), ("var", "var"), ("nrow", "nrow")):
            got = getattr(res, pre + attr)
            assert got.dtype == ref[key].dtype and got.reshape(ref[key].shape).tobytes() == ref[key].tobytes(), pre + attr
        assert int(res.nbad[i]) == ref["nbad"], pre


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_end_to_end_is_the_ensemble_and_the_kernel(eng, deck, mode):  # noqa: F811
    from unconfined_amd import WellField
    c = sobol_case(eng, deck, mode)
    fx = c["fx"]
    assert c["thetas"].shape == (12, 2) and c["s_all"].shape == (12, 6, 5, 2)
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    res = field.sobol(c["plan"], FREE, c["thetas"], fx["z"], members=True, with_stats=True)
    assert res.all.tobytes() == c["s_all"].tobytes() and res.dall.tobytes() == c["ds_all"].tobytes()
    check_against_debug(res, 2, 3)
    assert (res.nrow == 3).all() and (res.dnrow == 3).all() and res.nbad.tolist() == [0, 0]
    assert res.S.shape == (2, 6, 5, 2) and np.isfinite(res.S).all() and np.isfinite(res.se_ST).all() and (res.var > 0.0).all()
    assert (res.ST >= 0.0).all() and (res.se_S >= 0.0).all() and (res.se_ST >= 0.0).all() and set(res.stats) >= {"nan_scrubbed"}
    print(f"[field sobol {deck} {mode}] S of Kr {float(res.S[0].min()):.3f} .. {float(res.S[0].max()):.3f}, of Ss {float(res.S[1].min()):.3f} .. "
          f"{float(res.S[1].max()):.3f}; ST of Kr {float(res.ST[0].min()):.3f} .. {float(res.ST[0].max()):.3f}, of Ss {float(res.ST[1].min()):.3f} .. "
          f"{float(res.ST[1].max()):.3f}")
    # without the derivative and without the members: the same bits of what is asked for
    small = field.sobol(c["plan"], FREE, c["thetas"], fx["z"], derivative=False)
    assert small.dS is None and small.all is None
    for attr in ("S", "ST", "se_S", "se_ST", "mean", "var", "nrow"):
        assert getattr(small, attr).tobytes() == getattr(res, attr).tobytes(), attr
    field.close()


NOT_READ_BY_THEIS = ("Sy", "kappa", "ac", "ak", "usL")


def test_no_free_parameter_of_the_theis_deck_is_dead(eng):  # noqa: F811
    """A third free parameter that leaves every member map bitwise unchanged would have ST and seST of exactly +0.0.  The Theis
    deck has none: every parameter that its model does not read is refused by name, as a free parameter, before any launch
    (ucf_fit_perturb), and Kr and Ss both move every map.  The dead parameter is therefore held at the level of the kernel
    (test_the_kernel_is_the_restatement, the hand-made columns); here the refusals, and that both live parameters are alive."""
    from unconfined_amd import WellField, sobol_design
    from unconfined_amd.lib import UcfError
    c = sobol_case(eng, "c1_theis", "fast")
    fx, P = c["fx"], c["P"]
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    for name in NOT_READ_BY_THEIS:
        free = FREE + [name]
        theta = np.array([getattr(P, n) if getattr(P, n) > 0.0 else 1.0 for n in free])
        thetas = sobol_design(theta, np.diag([0.04] * 3), 3, seed=1)
        with pytest.raises(UcfError) as e:
            field.sobol(c["plan"], free, thetas, fx["z"], members=True)
        assert f"({name}) is not read by model" in e.value.message, (name, e.value.message)
    assert field.alloc_count() == 0
    field.close()
    # no AB block of the two-parameter design has the bits of A, in s or in ds
    for maps in (c["s_all"], c["ds_all"]):
        assert all(maps[(2 + j) * 3:(3 + j) * 3].tobytes() != maps[:3].tobytes() for j in range(2))


# ---- repetition

def test_repetition(eng):  # noqa: F811
    """a second identical call gives the same bytes and allocates nothing; a later ucf_field_ensemble on the same field still
    matches its own fresh-field result"""
    from unconfined_amd import WellField
    c = sobol_case(eng, "neuman74_partpen", "fast")
    fx = c["fx"]
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    a = field.sobol(c["plan"], FREE, c["thetas"], fx["z"], members=True)
    n = field.alloc_count()
    b = field.sobol(c["plan"], FREE, c["thetas"], fx["z"], members=True)
    assert n > 0 and field.alloc_count() == n
    for pre in ("", "d"):
        for attr in ("S", "ST", "se_S", "se_ST", "mean", "var", "nrow", "all"):
            assert getattr(a, pre + attr).tobytes() == getattr(b, pre + attr).tobytes(), pre + attr
    assert a.nbad.tolist() == b.nbad.tolist() == [0, 0]
    ens = field.ensemble(c["plan"], FREE, c["thetas"][:5], fx["z"], quantiles=(0.05, 0.5, 0.95), all_maps=True)
    fresh = WellField(fx["wells"], fx["locations"], fx["times"])
    ref = fresh.ensemble(c["plan"], FREE, c["thetas"][:5], fx["z"], quantiles=(0.05, 0.5, 0.95), all_maps=True)
    fresh.close()
    assert sorted(ens) == sorted(ref)
    for key in ens:
        assert ens[key].tobytes() == ref[key].tobytes(), key
    assert ens["s_all"].tobytes() == c["s_all"][:5].tobytes()
    # a smaller call after a larger one allocates nothing either
    n = field.alloc_count()
    field.sobol(c["plan"], FREE, c["thetas"], fx["z"], derivative=False)
    assert field.alloc_count() == n
    field.close()
