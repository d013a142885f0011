"""The host half of ucf_field_ensemble_times (include/ucf.h): every refusal of ucf_field_ensemble_times and ucf_debug_field_times
with its offender named and without a device, the numpy restatement of field_times_kernel (tests/field_times_restate.py) on
hand-made columns -- one per branch of the kernel's statement, the expected values written out --, the declarations and the
Python front end.  No GPU is needed: the checks come before a call asks for a device.

The hand-made columns use values for which every quotient and product of the statement is exact in binary (f = 0, 1/4, 1/2 on
steps of tau that are powers of two), so the literals are what exact arithmetic gives; the two columns with the Wynn sentinel
are not exact and are held to exact rational arithmetic within 3 u of T, u = 2^-53: the two differences and the quotient are
one rounding each, 3 u relative on f; the step of tau is a power of two, so the product is exact; the sum adds u of T.  With
the product no larger than half of T in both columns that is 3 u (T / 2) + u T = 2.5 u T."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import field_times_restate as R
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
ENTRIES = ("ucf_field_ensemble_times", "ucf_debug_field_times")
FIRST, LAST = abi.UCF_TIME_FIRST_ABOVE, abi.UCF_TIME_LAST_ABOVE
SENTINEL = -999999.9


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def addr(a):
    return a.ctypes.data if a is not None else None


def msg_of(so):
    return (so.ucf_last_error() or b"").decode()


def col(a, j):
    return np.ascontiguousarray(np.asarray(a, float)[:, j])


def create(so):
    h = C.c_void_p()
    assert so.ucf_field_create(len(WELLS), col(WELLS, 0), col(WELLS, 1), col(WELLS, 2), col(WELLS, 3), len(LOCATIONS), col(LOCATIONS, 0),
                               col(LOCATIONS, 1), len(TIMES), TIMES, C.byref(h)) == 0
    return h


def test_header_and_exports(so):
    """fails on the parent: the symbols do not exist there"""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucf.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s) and getattr(so, s).argtypes is not None, s
    enum = re.search(r"enum\s*\{\s*UCF_TIME_FIRST_ABOVE\s*=\s*(\d+)\s*,\s*UCF_TIME_LAST_ABOVE\s*=\s*(\d+)\s*\}", code)
    assert enum and (int(enum.group(1)), int(enum.group(2))) == (abi.UCF_TIME_FIRST_ABOVE, abi.UCF_TIME_LAST_ABOVE) == (0, 1)
    assert abi.TIME_KINDS == {"first_above": 0, "last_above": 1}
    # the declared parameters, in number and order of kind, are those of the binding
    for s in ENTRIES:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, code, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        argtypes = getattr(so, s).argtypes
        assert len(params) == len(argtypes), (s, len(params), len(argtypes))
        for p, at in zip(params, argtypes):
            if "*" in p:
                assert at is C.c_void_p or hasattr(at, "contents") or issubclass(at, C._Pointer), (s, p, at)
            else:
                want = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}[p.rsplit(None, 1)[0]]
                assert at is want, (s, p, at)


def times_call(so, h, plan=None, npar=2, ids=(0, 2), nens=None, thetas=((1.0, 1e-4), (1.1, 2e-4), (0.9, 1.5e-4)), weight=None, nz=2,
               z=(145.7, 100.0), tau=None, tau_never=6000.0, limit=(0.5, 0.1), nlim=None, kind=(FIRST, LAST), q=(0.05, 0.5), nq=None,
               horizon=(365.0,), nhor=None, want_quant=False, want_later=False, null=(), no_T=False):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), thetas=np.ascontiguousarray(thetas, dtype=float), z=np.ascontiguousarray(z, dtype=float),
                weight=None if weight is None else np.ascontiguousarray(weight, dtype=float),
                tau=None if tau is None else np.ascontiguousarray(tau, dtype=float), limit=np.ascontiguousarray(limit, dtype=float),
                kind=np.ascontiguousarray(kind, dtype=np.int32), q=np.ascontiguousarray(q, dtype=float),
                horizon=np.ascontiguousarray(horizon, dtype=float))
    nens = len(arrs["thetas"]) if nens is None else nens
    nlim = len(arrs["limit"]) if nlim is None else nlim
    nq = len(arrs["q"]) if nq is None else nq
    nhor = len(arrs["horizon"]) if nhor is None else nhor
    for k in null:
        arrs[k] = None
    nout = max(nlim, 1) * len(LOCATIONS) * max(nz, 1)
    quant, later = np.zeros((max(nq, 1), nout)), np.zeros((max(nhor, 1), nout))
    maps = abi.UcfEnsembleMaps(None, None, None, None, addr(quant) if want_quant else None, None, None)
    u, ess, nl = np.zeros(max(nens, 1), np.uint64), C.c_double(-1.0), C.c_int(-1)
    rc = so.ucf_field_ensemble_times(h, plan, npar, addr(arrs["ids"]), nens, addr(arrs["thetas"]), addr(arrs["weight"]), nz, addr(arrs["z"]),
                                     addr(arrs["tau"]), tau_never, nlim, addr(arrs["limit"]), addr(arrs["kind"]), nq, addr(arrs["q"]), nhor,
                                     addr(arrs["horizon"]), None if no_T else C.byref(maps), addr(later) if want_later else None, None, None,
                                     addr(u), C.addressof(ess), C.addressof(nl))
    return rc, msg_of(so), dict(u=u, ess=ess.value, nlaunched=nl.value)


def test_times_refusals_name_the_offender(so):
    import torch
    h = create(so)
    lnt = np.log(TIMES)
    cases = [
        # what ucf_field_ensemble_weighted checks on the shared arguments
        (dict(nz=0), "nz"), (dict(z=(145.7, np.nan)), "z[1]"), (dict(null=("z",)), "NULL z"), (dict(null=("ids",)), "NULL ids"),
        (dict(null=("thetas",)), "NULL thetas"), (dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nens=0), "nens=0"),
        (dict(nens=1025), "nens=1025"), (dict(nq=17), "nq=17"), (dict(q=(0.5, 1.5)), "q[1]"), (dict(null=("q",)), "NULL q"),
        (dict(nq=0, want_quant=True), "quant is asked for"),
        (dict(thetas=((1.0, 1e-4), (1.1, -2e-4))), "member 1"), (dict(thetas=((np.inf, 1e-4),)), "member 0"),
        # the horizons, in the place of an ensemble's limits
        (dict(nhor=17), "nhor=17"), (dict(nhor=-1), "nhor=-1"), (dict(null=("horizon",)), "NULL horizon with nhor=1"),
        (dict(horizon=(365.0, np.inf)), "horizon[1]"), (dict(horizon=(np.nan,)), "horizon[0]"),
        (dict(nhor=0, want_later=True), "plater is asked for with nhor=0"),
        # the limits, their kinds, the abscissa and the censoring value
        (dict(no_T=True), "NULL T"), (dict(nlim=0), "nlim=0"), (dict(nlim=17), "nlim=17"), (dict(nlim=-3), "nlim=-3"),
        (dict(null=("limit",)), "NULL limit"), (dict(null=("kind",)), "NULL kind"), (dict(limit=(0.5, np.inf)), "limit[1]"),
        (dict(limit=(np.nan, 0.1)), "limit[0]"), (dict(kind=(FIRST, 2)), "kind[1]=2"), (dict(kind=(-1, LAST)), "kind[0]=-1"),
        (dict(tau=np.r_[lnt[:4], np.nan, lnt[5]]), "tau[4]"), (dict(tau=np.r_[-np.inf, lnt[1:]]), "tau[0]"),
        (dict(tau=np.r_[lnt[:3], lnt[2], lnt[4:]]), "tau[3]"), (dict(tau=lnt[::-1]), "tau[1]"),
        (dict(tau_never=np.inf), "tau_never=inf"), (dict(tau_never=np.nan), "tau_never=nan"), (dict(tau_never=3000.0), "tau_never=3000"),
        (dict(tau_never=2999.0), "tau_never=2999"), (dict(tau=lnt, tau_never=float(lnt[-1])), "tau_never="),
        # the weights, after everything else
        (dict(weight=(1.0, -1.0, 1.0)), "member 1: weight"), (dict(weight=(0.0, 0.0, 0.0)), "all 3 weights"), (dict(weight=(1.0, np.nan, 1.0)), "member 1: weight"),
    ]
    for kw, offender in cases:
        rc, msg, _ = times_call(so, h, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg, _ = times_call(so, None)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device.  The integer weights
    # are written by the checks
    for kw in (dict(), dict(weight=(1.0, 0.0, 0.25)), dict(nq=0, nhor=0), dict(tau=lnt, tau_never=float(np.log(6000.0)), horizon=(np.log(365.0),)),
               dict(limit=np.linspace(0.1, 1.6, 16), kind=[FIRST, LAST] * 8, want_quant=True, want_later=True)):
        rc, msg, out = times_call(so, h, **kw)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
        if "weight" in kw:
            assert out["u"].tolist() == [2 ** 32, 0, 2 ** 30] and out["nlaunched"] == 2 and out["ess"] > 1.0
        else:
            assert out["nlaunched"] == -1 and out["ess"] == -1.0
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_too_many_values_for_one_buffer(so):
    """nens nlim nsite beyond what one buffer may hold, where nens nt nsite is not: 3 times against 16 limits"""
    h = C.c_void_p()
    nloc = 1 << 20
    xy = np.zeros(nloc)
    assert so.ucf_field_create(1, np.zeros(1), np.zeros(1), np.ones(1), np.zeros(1), nloc, xy, xy, 3, np.array([1.0, 2.0, 3.0]), C.byref(h)) == 0
    nens, nz = 1024, 32                                  # 2^35 values per time or limit: 3 of them fit under 2^39 - 256, 16 do not
    thetas, z = np.ones((nens, 1)), np.linspace(1.0, 2.0, nz)
    ids, lim, kind = np.zeros(1, np.int32), np.linspace(0.1, 1.6, 16), np.zeros(16, np.int32)
    maps = abi.UcfEnsembleMaps()
    for nlim, want in ((16, "1024 members x 16 limits x 1048576 locations x 32 depths: too many values"), (3, None)):
        rc = so.ucf_field_ensemble_times(h, None, 1, addr(ids), nens, addr(thetas), None, nz, addr(z), None, 4.0, nlim, addr(lim), addr(kind), 0, None,
                                         0, None, C.byref(maps), None, None, None, None, None, None)
        msg = msg_of(so)
        if want:
            assert rc == BAD and want in msg, (rc, msg)
        else:
            assert "too many" not in msg and rc in (BAD, NO_DEVICE), (rc, msg)      # on to the plan, or to the device
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    nens, nt, nsite, nlim = 2, 3, 5, 2
    a = np.arange(nens * nt * nsite, dtype=float)
    tau, lim, kind = np.array([1.0, 2.0, 4.0]), np.array([3.0, 7.0]), np.array([FIRST, LAST], np.int32)
    T = np.zeros((nens, nlim, nsite))

    def call(nens=nens, nt=nt, nsite=nsite, a=a, tau=tau, tau_never=8.0, nlim=nlim, lim=lim, kind=kind, T=T):
        kind = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
        tau = None if tau is None else np.ascontiguousarray(tau, dtype=float)
        rc = so.ucf_debug_field_times(nens, nt, nsite, addr(a), addr(tau), tau_never, nlim, addr(lim), addr(kind), addr(T))
        return rc, msg_of(so)

    for kw, offender in ((dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"), (dict(nt=0), "nt=0"), (dict(nsite=0), "nsite=0"),
                         (dict(a=None), "NULL a"), (dict(tau=None), "NULL tau"), (dict(T=None), "NULL T"), (dict(nlim=0), "nlim=0"),
                         (dict(nlim=17), "nlim=17"), (dict(lim=None), "NULL limit"), (dict(kind=None), "NULL kind"),
                         (dict(lim=np.array([3.0, np.inf])), "limit[1]"), (dict(kind=[FIRST, 7]), "kind[1]=7"),
                         (dict(tau=[1.0, np.nan, 4.0]), "tau[1]"), (dict(tau=[1.0, 1.0, 4.0]), "tau[1]"), (dict(tau=[1.0, 2.0, 1.5]), "tau[2]"),
                         (dict(tau_never=4.0), "tau_never=4"), (dict(tau_never=np.inf), "tau_never=inf"), (dict(tau_never=np.nan), "tau_never=nan"),
                         (dict(nens=1024, nsite=1 << 20), "more than 2^31-1")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)


# ---- the restatement on hand-made columns

TAU = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
NEVER = 64.0
nan, inf = np.nan, np.inf
# name: (column, FIRST at L = 1, LAST at L = 1, FIRST at L = 0, LAST at L = 0)
COLUMNS = {
    "above at k = 0":             ([2.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1.0, 1.5, 1.0, 2.0),
    "never above 1":              ([0.0, 0.5, 0.25, 0.0, 0.5, 0.75], 64.0, 1.0, 1.0, 64.0),
    "v == L exactly, not above":  ([0.0, 1.0, 1.0, 0.0, 1.0, 0.0], 64.0, 1.0, 1.0, 32.0),
    "v0 == L, f = 0":             ([0.0, 1.0, 3.0, -1.0, 0.0, 0.0], 2.0, 6.0, 1.0, 7.0),
    "a plateau":                  ([0.0, 2.0, 2.0, 2.0, 0.0, 0.0], 1.5, 12.0, 1.0, 16.0),
    "rise, fall, rise":           ([0.0, 4.0, -1.0, 0.0, 2.0, 0.0], 1.25, 24.0, 1.0, 32.0),
    "still above at nt - 1":      ([0.0, 0.0, 0.0, 0.0, 0.0, 2.0], 24.0, 64.0, 16.0, 64.0),
    "NaN before the crossing":    ([0.0, nan, 2.0, 0.0, 0.0, 0.0], nan, nan, nan, nan),
    "NaN after the crossing":     ([0.0, 2.0, nan, 0.0, 0.0, 0.0], 1.5, nan, 1.0, nan),
    "+inf":                       ([0.0, inf, 0.0, 0.0, 0.0, 0.0], nan, nan, nan, nan),
    "-inf before the crossing":   ([0.0, -inf, 2.0, 0.0, 0.0, 0.0], nan, nan, nan, nan),
    "zeros of both signs":        ([-0.0, -0.0, 0.0, -0.0, 0.0, -0.0], 64.0, 1.0, 64.0, 1.0),
}


def test_restatement_on_hand_made_columns():
    a = np.array([c[0] for c in COLUMNS.values()]).T[None]                  # [1][nt][ncol]
    T = R.times(a, TAU, NEVER, [1.0, 1.0, 0.0, 0.0], [FIRST, LAST, FIRST, LAST])
    assert T.shape == (1, 4, len(COLUMNS))
    for i, (name, c) in enumerate(COLUMNS.items()):
        want = np.array(c[1:])
        got = T[0, :, i]
        assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), (name, got.tolist(), want.tolist())
    # -0.0 as the limit is the limit 0.0: nothing of the zeros column is above it
    Tz = R.times(a, TAU, NEVER, [-0.0, -0.0], [FIRST, LAST])
    assert Tz[0, :, -1].tolist() == [64.0, 1.0]
    assert Tz.tobytes() == T[:, 2:].tobytes()
    # the NaN that the statement writes is numpy's
    assert T[0, 0, 7].tobytes() == np.float64(np.nan).tobytes()
    # members and trailing shapes are kept apart
    both = np.concatenate([a, a[:, :, ::-1]])
    T2 = R.times(both.reshape(2, 6, 3, 4), TAU, NEVER, [1.0, 0.0], [LAST, FIRST])
    assert T2.shape == (2, 2, 3, 4) and T2[0].reshape(2, -1).tobytes() == T[0, 1:3].tobytes()
    assert T2[1].reshape(2, -1)[:, ::-1].tobytes() == T[0, 1:3].tobytes()


def test_restatement_with_the_sentinel_against_exact_arithmetic():
    """the Wynn sentinel is finite and takes part: a crossing up from it and a fall down to it"""
    cols = np.array([[SENTINEL, SENTINEL, 3.0, -1.0, 0.0, 0.0], [3.0, SENTINEL, SENTINEL, SENTINEL, SENTINEL, SENTINEL]])
    T = R.times(cols.T[None], TAU, NEVER, [1.0, 0.0], [FIRST, LAST])[0]
    F = lambda v: Fraction(float(v))
    # FIRST at 1 of column 0: between tau[1] and tau[2]; LAST at 0 of column 1: between tau[0] and tau[1]
    want_first = F(2) + (F(1) - F(SENTINEL)) / (F(3) - F(SENTINEL)) * F(2)
    want_last = F(1) + (F(3) - F(0)) / (F(3) - F(SENTINEL)) * F(1)
    u = Fraction(1, 2 ** 53)
    for got, want in ((T[0, 0], want_first), (T[1, 1], want_last)):
        assert abs(F(got) - want) <= 3 * u * want, (got, float(want))
    assert T[0, 0] == 3.9999960000116 and T[1, 1] == 1.0000029999913
    # LAST at 0 of column 0 (3 -> -1 is the last fall) and FIRST at 1 of column 1 (above at k = 0) are exact
    assert T[1, 0] == 7.0 and T[0, 1] == 1.0


def test_a_limit_above_the_maximum():
    """FIRST gives tau_never and LAST gives tau[0], whatever the column holds below the limit"""
    rng = np.random.default_rng(7)
    a = rng.normal(size=(3, 6, 11))
    a[1, 2, 3] = SENTINEL
    top = float(a.max())
    for L in (top, np.nextafter(top, np.inf), top + 1.0):
        T = R.times(a, TAU, NEVER, [L, L], [FIRST, LAST])
        assert (T[:, 0] == NEVER).all() and (T[:, 1] == TAU[0]).all()
    # just below the maximum its column crosses, and no other does
    m, k, e = np.unravel_index(np.argmax(a), a.shape)
    T = R.times(a, TAU, NEVER, [np.nextafter(top, -np.inf)], [FIRST])
    assert T[m, 0, e] < NEVER and (np.delete(T[:, 0].ravel(), m * 11 + e) == NEVER).all()
    # one time only: above gives tau[0] (FIRST) and tau_never (LAST), not above the reverse
    one = np.array([[[2.0, 0.0]]])
    assert R.times(one, [5.0], 9.0, [1.0, 1.0], [FIRST, LAST])[0].tolist() == [[5.0, 9.0], [9.0, 5.0]]


# ---- the Python front end

def test_python_front_end_without_a_gpu():
    import torch
    from unconfined_amd import TimeToLimit, WellField
    field = WellField(WELLS, LOCATIONS, TIMES)
    plan = types.SimpleNamespace(_h=None)
    good = dict(plan=plan, free=["Kr", "Ss"], thetas=[(1.0, 1e-4), (1.1, 2e-4)], z=[145.7, 100.0], limits=[0.5, 0.1])

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return field.time_to_limit(**a)

    for kw in (dict(thetas=[(1.0, 1e-4, 3.0)]), dict(limits=[]), dict(kinds=["first_above"]), dict(kinds="sometime"), dict(abscissa="sqrt"),
               dict(weights=[1.0])):
        with pytest.raises(ValueError):
            call(**kw)
    # what the library refuses reaches the caller with its offender
    for kw, offender in ((dict(limits=[0.5, np.inf]), "limit[1]"), (dict(kinds=[0, 5]), "kind[1]=5"), (dict(never=3000.0), "tau_never=3000"),
                         (dict(never=3000.0, abscissa="lnt"), "tau_never="), (dict(horizons=[np.inf]), "horizon[0]"),
                         (dict(horizons=[-1.0], abscissa="lnt"), "horizon[0]"), (dict(q=[2.0]), "q[0]"), (dict(weights=[0.0, 0.0]), "weights are 0")):
        with pytest.raises(ucflib.UcfError) as e:
            call(**kw)
        assert e.value.status == BAD and offender in e.value.message, (kw, e.value.message)
    for kw in (dict(), dict(kinds=["first_above", "last_above"], abscissa="lnt", horizons=[365.0], weights=[1.0, 0.5], all_times=True),
               dict(kinds=abi.UCF_TIME_LAST_ABOVE, never=1e4, q=None)):
        with pytest.raises(ucflib.UcfError) as e:
            call(**kw)
        assert (e.value.status == NO_DEVICE) if not torch.cuda.is_available() else ("plan" in e.value.message), kw
    assert TimeToLimit(limits=np.zeros(1), kinds=np.zeros(1, np.int32), abscissa="t", never=2.0, mean=np.zeros((1, 1, 1)), nbad=0).quant is None
    field.close()
