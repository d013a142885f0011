"""The host half of the weighted ensembles (include/ucf.h): ucf_ensemble_quantise and ucf_ensemble_likelihood_weights against the
rules the header states, every refusal with its offender named, the argument checks of ucf_field_ensemble_weighted,
ucf_debug_ensemble_weighted and ucf_fit_objective that need no GPU, and the restatement that the GPU tests hold the kernels to
(tests/ensemble_weighted_restate.py): with equal weights it is the unweighted restatement bit for bit, and its quantiles are
numpy's weighted inverted_cdf exactly -- the integer weights as doubles make numpy's cumulative sums exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ensemble_weighted_restate import order_statistic, quantise, restate_weighted
from test_field_ensemble_host import LOCATIONS, TIMES, WELLS, addr, create
from test_gpu_field_ensemble import SENTINEL, restate, same_bits
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
ENTRIES = ("ucf_ensemble_quantise", "ucf_ensemble_likelihood_weights", "ucf_field_ensemble_weighted", "ucf_debug_ensemble_weighted",
           "ucf_fit_objective")
NENS = (1, 2, 3, 5, 17, 64, 257, 1024)


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def test_header_and_exports(so):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucf.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s


# ---- ucf_ensemble_quantise

def lib_quantise(so, w, nens=None, null=(), want_ess=True):
    w = np.ascontiguousarray(w, dtype=np.float64)
    nens = len(w) if nens is None else nens
    u = np.full(max(len(w), 1), 7, np.uint64)
    ess = C.c_double(-7.0)
    rc = so.ucf_ensemble_quantise(nens, None if "weight" in null else addr(w), None if "u" in null else addr(u),
                                  C.addressof(ess) if want_ess else None)
    return rc, u[:len(w)], ess.value, (so.ucf_last_error() or b"").decode()


def test_quantise_is_the_stated_rule(so):
    rng = np.random.default_rng(11)
    for nens in NENS:
        for kind in range(4):
            w = rng.random(nens) * 10.0 ** rng.uniform(-12, 3, nens)
            if kind == 1:
                w[rng.random(nens) < 0.4] = 0.0
                w[rng.integers(nens)] = 3.5
            elif kind == 2:
                w[:] = 0.37
            elif kind == 3:
                w = w * 1e-300                              # tiny weights: only ratios count
            rc, u, ess, msg = lib_quantise(so, w)
            assert rc == 0, msg
            want_u, want_ess = quantise(w)
            assert u.tobytes() == want_u.tobytes(), (nens, kind)
            assert ess == want_ess, (nens, kind, ess, want_ess)
            assert int(u.max()) == 2 ** 32 and 1.0 <= ess <= nens
            if kind == 2:
                # equal weights: all 2^32, and ess is nens exactly
                assert (u == 2 ** 32).all() and ess == float(nens)
    # ess may be NULL
    rc, u, ess, msg = lib_quantise(so, [1.0, 0.5], want_ess=False)
    assert rc == 0 and u.tolist() == [2 ** 32, 2 ** 31] and ess == -7.0


def test_quantise_rounds_to_nearest_and_drops_what_is_below_half_a_unit(so):
    # r 2^32 + 0.5 floored: 2^-33 of the largest is the first weight that survives (0.5 + 0.5 = 1); a weight below it by more
    # than the rounding of that sum is 0
    w = np.array([1.0, 2.0 ** -33, 2.0 ** -33 * (1.0 - 2.0 ** -20), 2.0 ** -34, 0.0, 1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, 1.0 - 2.0 ** -34])
    rc, u, ess, msg = lib_quantise(so, w)
    assert rc == 0, msg
    assert u.tolist() == [2 ** 32, 1, 0, 0, 0, 2, 3, 2 ** 32]
    assert u.tobytes() == quantise(w)[0].tobytes()
    # scaled by a factor that keeps every product and quotient exact: the same integers
    for f in (3.0, 2.0 ** -900, 2.0 ** 900):
        assert lib_quantise(so, w * f)[1].tobytes() == u.tobytes(), f


def test_quantise_refusals_name_the_member(so):
    cases = [
        (dict(w=[1.0], nens=0), "nens=0"), (dict(w=[1.0], nens=-2), "nens=-2"), (dict(w=np.ones(4), nens=abi.UCF_ENSEMBLE_MAX + 1), "nens=1025"),
        (dict(w=[1.0, 2.0], null=("weight",)), "NULL weight"), (dict(w=[1.0, 2.0], null=("u",)), "NULL u"),
        (dict(w=[1.0, -0.5, 2.0]), "member 1: weight=-0.5"), (dict(w=[1.0, 2.0, np.nan]), "member 2: weight=nan"),
        (dict(w=[np.inf, 2.0]), "member 0: weight=inf"), (dict(w=[1.0, -np.inf]), "member 1: weight=-inf"),
        (dict(w=[0.0, 0.0, 0.0]), "all 3 weights are 0"), (dict(w=[-0.0]), "all 1 weights are 0"),
    ]
    for kw, offender in cases:
        rc, _, _, msg = lib_quantise(so, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    assert lib_quantise(so, np.ones(abi.UCF_ENSEMBLE_MAX))[0] == 0


# ---- ucf_ensemble_likelihood_weights

def lib_weights(so, phi, nbad=None, s2=1.0, nens=None, null=()):
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    nb = None if nbad is None else np.ascontiguousarray(nbad, dtype=np.int32)
    nens = len(phi) if nens is None else nens
    w = np.full(max(len(phi), 1), -7.0)
    best, nadm = C.c_int(-7), C.c_int(-7)
    rc = so.ucf_ensemble_likelihood_weights(nens, None if "phi" in null else addr(phi), addr(nb), s2, None if "weight" in null else addr(w),
                                            None if "best" in null else C.addressof(best), None if "nadmissible" in null else C.addressof(nadm))
    return rc, w[:len(phi)], best.value, nadm.value, (so.ucf_last_error() or b"").decode()


def test_likelihood_weights_are_the_stated_expression(so):
    rng = np.random.default_rng(5)
    for nens in NENS:
        for s2 in (1.0, 0.37, 250.0):
            phi = 3.0 + rng.random(nens) * 10.0 ** rng.uniform(-3, 3, nens)
            nbad = (rng.random(nens) < 0.2).astype(np.int32) * rng.integers(1, 5, nens).astype(np.int32)
            phi[rng.random(nens) < 0.1] = np.nan
            phi[rng.random(nens) < 0.1] = np.inf
            adm = np.isfinite(phi) & (nbad == 0)
            if not adm.any():
                phi[0], nbad[0], adm[0] = 4.0, 0, True
            rc, w, best, nadm, msg = lib_weights(so, phi, nbad, s2)
            assert rc == 0, msg
            want_best = int(np.flatnonzero(adm)[np.argmin(phi[adm])])
            assert best == want_best and nadm == int(adm.sum())
            with np.errstate(all="ignore"):
                want = np.where(adm, np.exp(np.float64(-0.5) * ((phi - phi[best]) / np.float64(s2))), 0.0)
            # another libm may round exp differently: 1e-15 relative, as tests/test_field_ensemble_host.py allows its exp
            assert (w[~adm] == 0.0).all() and w[best] == 1.0 and not np.signbit(w).any()
            assert (np.abs(w - want) <= 1e-15 * want).all(), (nens, s2, float(np.abs(w / want - 1)[adm].max()))
            print(f"[likelihood weights] nens={nens} s2={s2}: {int((w != want).sum())} of {nens} differ from numpy's exp")
            # without nbad only the first test applies
            rc, w2, best2, nadm2, _ = lib_weights(so, phi, None, s2)
            fin = np.isfinite(phi)
            assert rc == 0 and nadm2 == int(fin.sum()) and best2 == int(np.flatnonzero(fin)[np.argmin(phi[fin])]) and (w2[~fin] == 0).all()


def test_likelihood_weights_ties_and_outputs(so):
    # ties in phi take the lowest index; a lower phi with nbad > 0 is not the best
    rc, w, best, nadm, msg = lib_weights(so, [5.0, 2.0, 2.0, 1.0, 2.0], [0, 0, 0, 3, 0])
    assert rc == 0 and best == 1 and nadm == 4 and w[1:].tolist() == [1.0, 1.0, 0.0, 1.0] and abs(w[0] / np.exp(-1.5) - 1.0) <= 1e-15, (w, msg)
    # a member far away underflows to 0 without harm; best and nadmissible may be NULL
    rc, w, best, nadm, _ = lib_weights(so, [1.0, 1e9], null=("best", "nadmissible"))
    assert rc == 0 and w.tolist() == [1.0, 0.0] and best == nadm == -7
    # -inf is not finite: not admissible
    rc, w, best, _, _ = lib_weights(so, [-np.inf, 3.0])
    assert rc == 0 and best == 1 and w.tolist() == [0.0, 1.0]


def test_likelihood_weights_refusals(so):
    cases = [
        (dict(phi=[1.0], nens=0), "nens=0"), (dict(phi=np.ones(3), nens=1025), "nens=1025"),
        (dict(phi=[1.0], null=("phi",)), "NULL phi"), (dict(phi=[1.0], null=("weight",)), "NULL weight"),
        (dict(phi=[1.0], s2=0.0), "s2=0"), (dict(phi=[1.0], s2=-1.0), "s2=-1"), (dict(phi=[1.0], s2=np.nan), "s2=nan"), (dict(phi=[1.0], s2=np.inf), "s2=inf"),
        (dict(phi=[np.nan, np.inf]), "no admissible member"), (dict(phi=[1.0, 2.0], nbad=[1, 2]), "no admissible member"),
        (dict(phi=[np.nan, 2.0], nbad=[0, 1]), "no admissible member"),
    ]
    for kw, offender in cases:
        rc, _, _, _, msg = lib_weights(so, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)


def test_python_front_end():
    from unconfined_amd import likelihood_weights, quantise_weights
    out = likelihood_weights([4.0, 2.0, np.nan, 2.5], nbad=[0, 0, 0, 1], s2=0.5)
    assert out["best"] == 1 and out["nadmissible"] == 2 and out["weight"][1:].tolist() == [1.0, 0.0, 0.0]
    assert abs(out["weight"][0] / np.exp(-2.0) - 1.0) <= 1e-15
    u, ess = quantise_weights(out["weight"])
    assert u.dtype == np.uint64 and u.tobytes() == quantise(out["weight"])[0].tobytes() and ess == quantise(out["weight"])[1]
    with pytest.raises(ucflib.UcfError) as e:
        quantise_weights([0.0, 0.0])
    assert e.value.status == BAD and "all 2 weights are 0" in e.value.message
    with pytest.raises(ValueError):
        likelihood_weights([1.0, 2.0], nbad=[0])


# ---- the restatement itself

def columns(nens, nout, seed):
    """random values over several decades, and by e % 6: plain; NaN mixed in; +-Inf mixed in; every member NaN; ties; the zeros"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(nens, nout)) * 10.0 ** rng.uniform(-6, 6, (nens, nout))
    for e in range(nout):
        c = a[:, e]
        if e % 6 == 1:
            c[rng.random(nens) < 0.3] = np.nan
        elif e % 6 == 2:
            c[rng.random(nens) < 0.2] = np.inf
            c[rng.random(nens) < 0.2] = -np.inf
        elif e % 6 == 3:
            c[:] = np.nan
        elif e % 6 == 4:
            c[:] = rng.integers(-2, 3, nens).astype(float)
        elif e % 6 == 5:
            c[:] = rng.choice(np.array([0.0, -0.0, 1.0, SENTINEL]), nens)
    return a


@pytest.mark.parametrize("nens", NENS)
def test_equal_weights_are_the_unweighted_arithmetic(nens):
    a = columns(nens, 24, 100 + nens)
    levels, limits = (0.0, 0.05, 0.5, 0.95, 1.0), (0.0, 1.0, SENTINEL, -0.3)
    u, ess = quantise(np.full(nens, 0.125))
    assert (u == 2 ** 32).all() and ess == nens
    got, want = restate_weighted(a, u, levels, limits), restate(a, levels, limits)
    for key in ("mean", "sd", "min", "max", "nfin", "pexc"):
        same_bits(got[key], want[key], key)
    assert got["nbad"] == want["nbad"]
    same_bits(got["quant"], order_statistic(a, levels), "quant")


@pytest.mark.parametrize("nens", NENS)
def test_quantiles_are_numpys_weighted_inverted_cdf(nens):
    rng = np.random.default_rng(200 + nens)
    a = columns(nens, 24, 300 + nens)
    levels = (0.0, 0.05, 0.25, 1.0 / 3.0, 0.5, 0.95, 1.0)
    for kind in range(3):
        w = rng.random(nens) * 10.0 ** rng.uniform(-4, 0, nens)
        if kind == 1:
            w[rng.random(nens) < 0.4] = 0.0                # members that are not in the ensemble
            w[rng.integers(nens)] = 1.0
        elif kind == 2:
            w = rng.choice(np.array([0.25, 0.5, 1.0]), nens)        # equal weights among the members: cumulative sums that tie
            w[rng.integers(nens)] = 1.0
        u, _ = quantise(w)
        got = restate_weighted(a, u, levels, ())
        v = a.reshape(nens, -1)
        for e in range(v.shape[1]):
            keep = np.isfinite(v[:, e]) & (u > 0)
            assert got["nfin"].ravel()[e] == keep.sum()
            if not keep.any():
                assert np.isnan(got["quant"][:, e]).all()
                continue
            want = np.quantile(v[keep, e], levels, weights=u[keep].astype(np.float64), method="inverted_cdf")
            assert (got["quant"][:, e] == want).all(), (nens, kind, e, got["quant"][:, e], want)
            # a weighted mean that any textbook gives, to a few roundings
            ref = np.average(v[keep, e], weights=u[keep].astype(np.float64))
            assert abs(got["mean"].ravel()[e] - ref) <= 4.0 * nens * np.spacing(np.abs(v[keep, e]).max())


def test_a_level_on_an_interval_end_takes_the_member_below():
    # weights 1, 1, 2 on the values 3, 1, 2: in ascending order u = 2^31, 2^32, 2^31, the intervals end at 2^31, 3 2^31 and U = 2^33,
    # so p = 0.25 and p = 0.75 sit on an end and belong to the member below it
    a = np.array([[3.0], [1.0], [2.0]])
    u, _ = quantise([1.0, 1.0, 2.0])
    assert u.tolist() == [2 ** 31, 2 ** 31, 2 ** 32]
    got = restate_weighted(a, u, (0.0, 0.25, np.nextafter(0.25, 1.0), 0.5, 0.75, np.nextafter(0.75, 1.0), 1.0), ())
    assert got["quant"][:, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 2.0, 3.0, 3.0]


# ---- argument checks of the GPU entries that need no GPU

def weighted(so, h, plan=None, npar=2, ids=(0, 2), nens=3, thetas=None, weight=(1.0, 0.5, 0.25), nz=2, z=(145.7, 100.0), q=(0.05, 0.5, 0.95),
             limit=(0.5,), null=()):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32),
                thetas=np.ascontiguousarray(np.ones((max(nens, 1), max(npar, 1))) if thetas is None else thetas, dtype=float),
                weight=np.ascontiguousarray(weight, dtype=float), z=np.ascontiguousarray(z, dtype=float), q=np.ascontiguousarray(q, dtype=float),
                limit=np.ascontiguousarray(limit, dtype=float))
    nq, nlim = len(arrs["q"]), len(arrs["limit"])
    for k in null:
        arrs[k] = None
    nout = 60
    m = abi.UcfEnsembleMaps()
    mean, quant = np.zeros(nout), np.zeros(nout * max(nq, 1))
    m.mean, m.quant = mean.ctypes.data, quant.ctypes.data if nq else None
    pe, nbad = np.zeros(nout * max(nlim, 1)), np.zeros(2, np.int64)
    u, ess, nl = np.full(max(nens, 1), 7, np.uint64), C.c_double(-7.0), C.c_int(-7)
    rc = so.ucf_field_ensemble_weighted(h, plan, npar, addr(arrs["ids"]), nens, addr(arrs["thetas"]), addr(arrs["weight"]), nz, addr(arrs["z"]), nq,
                                        addr(arrs["q"]), nlim, addr(arrs["limit"]), C.byref(m), None, addr(pe) if nlim else None, addr(nbad), None,
                                        addr(u), C.addressof(ess), C.addressof(nl))
    return rc, (so.ucf_last_error() or b"").decode(), u, ess.value, nl.value


def test_weighted_call_checks_before_it_asks_for_a_device(so):
    import torch
    h = create(so, WELLS, LOCATIONS, TIMES)
    th = np.array([[1.0, 1e-4], [1.1, 1e-4], [1.2, 2e-4]])
    cases = [
        # the checks of ucf_field_ensemble, in its order ...
        (dict(nz=0), "nz"), (dict(null=("z",)), "NULL z"), (dict(null=("ids",)), "NULL ids"), (dict(null=("thetas",)), "NULL thetas"),
        (dict(npar=0, ids=(0,)), "npar=0"), (dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"),
        (dict(thetas=[[1.0, 1e-4], [1.1, 0.0], [1.2, 2e-4]]), "member 1: Ss=0"), (dict(q=(0.5, 1.5)), "q[1]"), (dict(limit=(np.nan,)), "limit[0]"),
        # ... then those of ucf_ensemble_quantise
        (dict(null=("weight",)), "NULL weight"), (dict(weight=(1.0, -1.0, 0.5)), "member 1: weight=-1"), (dict(weight=(1.0, 1.0, np.nan)), "member 2: weight=nan"),
        (dict(weight=(0.0, 0.0, 0.0)), "all 3 weights are 0"),
        # a bad theta is named before a bad weight
        (dict(thetas=[[1.0, 1e-4], [1.1, 1e-4], [-1.2, 2e-4]], weight=(-1.0, 1.0, 1.0)), "member 2: Kr=-1.2"),
    ]
    for kw, offender in cases:
        a = dict(thetas=th)
        a.update(kw)
        rc, msg, _, _, _ = weighted(so, h, **a)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg, _, _, _ = weighted(so, None, thetas=th)
    assert rc == BAD and "field" in msg
    # every argument in order: the weights are quantised, then a plan cannot exist without a device
    rc, msg, u, ess, nl = weighted(so, h, thetas=th, weight=(0.5, 2.0, 1e-12))
    assert u.tolist() == [2 ** 30, 2 ** 32, 0] and nl == 2 and ess == quantise([0.5, 2.0, 1e-12])[1]
    if torch.cuda.is_available():
        assert rc == BAD and "plan" in msg, msg
    else:
        assert rc == NO_DEVICE and "no CPU fallback" in msg, msg
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    a = np.arange(12.0)
    q, lim, wt = np.array([0.5]), np.array([3.0]), np.array([1.0, 2.0, 0.0])
    m = abi.UcfEnsembleMaps()
    quant = np.zeros(4)
    m.quant = quant.ctypes.data
    pexc, nbad = np.zeros(4), np.zeros(1, np.int64)
    call = lambda nens=3, nout=4, a=a, wt=wt, nq=1, q=q, nlim=1, lim=lim: (
        so.ucf_debug_ensemble_weighted(nens, nout, addr(a), addr(wt), nq, addr(q), nlim, addr(lim), C.byref(m), addr(pexc), addr(nbad)),
        (so.ucf_last_error() or b"").decode())
    for kw, offender in ((dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"), (dict(nq=0), "quant is asked for with nq=0"),
                         (dict(nlim=0), "pexc is asked for with nlim=0"), (dict(q=np.array([1.5])), "q[0]"), (dict(a=None), "NULL a"), (dict(nout=0), "nout=0"),
                         (dict(wt=None), "NULL weight"), (dict(wt=np.array([1.0, np.inf, 1.0])), "member 1: weight=inf"),
                         (dict(wt=np.zeros(3)), "all 3 weights are 0")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)


def test_objective_refuses_a_null_fit(so):
    phi, nbad = np.zeros(2), np.zeros(2, np.int32)
    rc = so.ucf_fit_objective(None, 2, addr(np.ones((2, 2))), addr(phi), addr(nbad), None, None, None)
    assert rc == BAD and b"NULL" in so.ucf_last_error()
