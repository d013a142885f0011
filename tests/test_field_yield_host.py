"""The host half of ucf_field_yield (include/ucf.h): every refusal of ucf_field_yield and ucf_debug_field_yield with its offender
named and without a device, the numpy restatement of the ratio test (tests/field_yield_restate.py) against exact rational
arithmetic, the declarations and the Python front end.  No GPU is needed: the checks come before a call asks for a device.

Bound of the restatement against exact arithmetic, u = 2^-53.  The exact candidate of an output is (limit - b) / sum_c x_c r_c on
the SAME doubles.  room = limit - b is one rounded operation on exact inputs: relative error u, whatever cancels.  D is nctl
products and nctl sums, the first sum onto +0.0 exact; the cases below have no cancellation in D (per output every r_c has one
sign, per pattern every x_c has one sign, zeros among both), so each rounding moves D by at most u relative and D carries at
most nctl u (one per product, one per sum after the first: 2 nctl - 1 roundings on terms of which each sees at most nctl).  The
quotient adds one u: (1 + nctl + 1) u = (nctl + 2) u relative to first order on every candidate, hence on hi, on lo and on y.
Without cancellation D == 0 exactly where it is 0 in exact arithmetic, and the sign of room is exact, so `dead` agrees exactly;
feas = (dead == 0 && lo <= hi) agrees wherever the exact ends differ by more than their summed bounds, (nctl + 2) u (|hi| + |lo|)."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import field_yield_restate as Y
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
NOUT = len(TIMES) * len(LOCATIONS) * 2
ENTRIES = ("ucf_field_yield", "ucf_debug_field_yield")
U = Fraction(1, 2 ** 53)


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
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    vals = dict(re.findall(r"#define\s+(UCF_YIELD_\w+)\s+(\d+)", code))
    assert vals == {"UCF_YIELD_MAX_CTL": "8", "UCF_YIELD_MAX_PAT": "4096", "UCF_YIELD_PAT_TILE": str(abi.UCF_YIELD_PAT_TILE)}
    assert (abi.UCF_YIELD_MAX_CTL, abi.UCF_YIELD_MAX_PAT) == (8, 4096)


LIMIT = np.full(NOUT, np.inf)
LIMIT[[3, 17, 40, 59]] = [1.0, 2.5, 0.25, 3.0]


def yield_call(so, h, plan=None, npar=2, ids=(0, 2), nens=None, thetas=((1.0, 1e-4), (1.1, 2e-4), (0.9, 1.5e-4)), weight=None, nz=2,
               z=(145.7, 100.0), nctl=2, ctl=(0, 1, -1, 0), npat=None, x=((1.0, 1.0), (0.5, 2.0), (0.0, -1.0)), limit=LIMIT, smax=4.0, q=(0.05, 0.5),
               nq=None, level=(1.0,), nlev=None, want_quant=False, want_pexc=False, null=()):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), thetas=np.ascontiguousarray(thetas, dtype=float), z=np.ascontiguousarray(z, dtype=float),
                weight=None if weight is None else np.ascontiguousarray(weight, dtype=float), ctl=np.ascontiguousarray(ctl, dtype=np.int32),
                x=np.ascontiguousarray(x, dtype=float), limit=np.ascontiguousarray(limit, dtype=float), q=np.ascontiguousarray(q, dtype=float),
                level=np.ascontiguousarray(level, dtype=float))
    nens = len(arrs["thetas"]) if nens is None else nens
    npat = len(arrs["x"]) if npat is None else npat
    nq = len(arrs["q"]) if nq is None else nq
    nlev = len(arrs["level"]) if nlev is None else nlev
    for k in null:
        arrs[k] = None
    quant, pexc = np.zeros((max(nq, 1), max(npat, 1))), np.zeros((max(nlev, 1), max(npat, 1)))
    maps = abi.UcfEnsembleMaps(None, None, None, None, addr(quant) if want_quant else None, None, None)
    con, ncon = np.full(NOUT, -7, np.int32), C.c_int(-7)
    u, ess, nl = np.zeros(max(nens, 1), np.uint64), C.c_double(-1.0), C.c_int(-1)
    rc = so.ucf_field_yield(h, plan, npar, addr(arrs["ids"]), nens, addr(arrs["thetas"]), addr(arrs["weight"]), nz, addr(arrs["z"]), nctl,
                            addr(arrs["ctl"]), npat, addr(arrs["x"]), addr(arrs["limit"]), smax, nq, addr(arrs["q"]), nlev, addr(arrs["level"]),
                            C.byref(maps), addr(pexc) if want_pexc else None, None, None, None, None, None, None, addr(con), C.addressof(ncon), None,
                            None, addr(u), C.addressof(ess), C.addressof(nl))
    return rc, msg_of(so), dict(con=con, ncon=ncon.value, u=u, ess=ess.value, nlaunched=nl.value)


def test_yield_refusals_name_the_offender(so):
    import torch
    h = create(so)
    nanlim, neglim = LIMIT.copy(), LIMIT.copy()
    nanlim[5], neglim[7] = np.nan, -np.inf
    cases = [
        # what ucf_field_ensemble_weighted checks on the shared arguments
        (dict(nz=0), "nz"), (dict(z=(145.7, np.nan)), "z[1]"), (dict(null=("z",)), "NULL z"), (dict(null=("ids",)), "NULL ids"),
        (dict(null=("thetas",)), "NULL thetas"), (dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nens=0), "nens=0"),
        (dict(nens=1025), "nens=1025"), (dict(nq=17), "nq=17"), (dict(nlev=17), "nlev=17"), (dict(nlev=-1), "nlev=-1"), (dict(q=(0.5, 1.5)), "q[1]"),
        (dict(level=(np.nan,)), "level[0]"), (dict(null=("q",)), "NULL q"), (dict(null=("level",)), "NULL level with nlev=1"),
        (dict(nq=0, want_quant=True), "quant is asked for"), (dict(nlev=0, want_pexc=True), "pexc is asked for with nlev=0"),
        (dict(thetas=((1.0, 1e-4), (1.1, -2e-4))), "member 1"), (dict(thetas=((np.inf, 1e-4),)), "member 0"),
        # controls, patterns, limits, smax
        (dict(null=("ctl",)), "NULL ctl"), (dict(null=("limit",)), "NULL limit"), (dict(null=("x",)), "NULL x"), (dict(nctl=0), "nctl=0"),
        (dict(nctl=9), "nctl=9"), (dict(npat=0), "npat=0"), (dict(npat=4097), "npat=4097"), (dict(x=((1.0, 1.0), (0.5, np.nan))), "x[3]"),
        (dict(x=((np.inf, 1.0),)), "x[0]"), (dict(smax=0.0), "smax=0"), (dict(smax=-1.0), "smax=-1"), (dict(smax=np.inf), "smax=inf"),
        (dict(smax=np.nan), "smax=nan"), (dict(ctl=(0, 1, 2, 0)), "ctl[2]=2"), (dict(ctl=(-2, 1, 0, 0)), "ctl[0]=-2"),
        (dict(ctl=(0, 0, -1, 0)), "control 1 owns no well"), (dict(ctl=(-1, -1, -1, -1), nctl=1, x=((1.0,),)), "control 0 owns no well"),
        (dict(limit=nanlim), "limit[5]"), (dict(limit=neglim), "limit[7]"), (dict(limit=np.full(NOUT, np.inf)), "no finite limit"),
        # the weights, after everything else
        (dict(weight=(1.0, -1.0, 1.0)), "member 1: weight"), (dict(weight=(0.0, 0.0, 0.0)), "all 3 weights"), (dict(weight=(1.0, np.nan, 1.0)), "member 1: weight"),
    ]
    for kw, offender in cases:
        rc, msg, _ = yield_call(so, h, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg, _ = yield_call(so, None)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device.  con, ncon and the
    # integer weights are written by the checks
    for kw in (dict(), dict(weight=(1.0, 0.0, 0.25)), dict(nq=0, nlev=0),
               dict(nctl=1, ctl=(0, 0, 0, 0), x=np.ones((4096, 1)), limit=np.zeros(NOUT))):
        rc, msg, out = yield_call(so, h, **kw)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
        want = np.flatnonzero(np.isfinite(kw.get("limit", LIMIT)))
        assert out["ncon"] == len(want) and out["con"][:len(want)].tolist() == want.tolist() and (out["con"][len(want):] == -7).all()
        if "weight" in kw:
            assert out["u"].tolist() == [2 ** 32, 0, 2 ** 30] and out["nlaunched"] == 2 and out["ess"] > 1.0
        else:
            assert out["nlaunched"] == -1 and out["ess"] == -1.0
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    nctl, nens, ncon, npat = 2, 3, 5, 4
    R = np.arange(nens * (nctl + 1) * ncon, dtype=float)
    x = np.arange(npat * nctl, dtype=float).reshape(npat, nctl) - 2.0
    lim, con = np.linspace(1.0, 2.0, ncon), np.array([0, 3, 4, 9, 11], np.int32)
    nanx, inflim = x.copy(), lim.copy()
    nanx[0, 1], inflim[2] = np.nan, np.inf
    outs = [np.zeros((nens, npat)) for _ in range(4)] + [np.zeros((nens, npat), np.int32) for _ in range(2)]
    nbad = C.c_longlong()

    def call(nctl=nctl, nens=nens, ncon=ncon, npat=npat, R=R, x=x, lim=lim, con=con, smax=3.0):
        con = None if con is None else np.ascontiguousarray(con, dtype=np.int32)
        rc = so.ucf_debug_field_yield(nctl, nens, ncon, npat, addr(R), addr(x), addr(lim), addr(con), smax, *(addr(o) for o in outs), C.addressof(nbad))
        return rc, msg_of(so)

    for kw, offender in ((dict(nctl=0), "nctl=0"), (dict(nctl=9), "nctl=9"), (dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"),
                         (dict(ncon=0), "ncon=0"), (dict(npat=0), "npat=0"), (dict(npat=4097), "npat=4097"),
                         (dict(nens=1024, ncon=1 << 20), "more than 2^31-1"), (dict(R=None), "NULL R"), (dict(x=None), "NULL x"),
                         (dict(lim=None), "NULL limit_con"), (dict(con=None), "NULL con"), (dict(x=nanx), "x[1]"), (dict(lim=inflim), "limit_con[2]"),
                         (dict(con=[0, 3, 3, 9, 11]), "con[2]=3"), (dict(con=[-1, 3, 4, 9, 11]), "con[0]=-1"), (dict(con=[5, 3, 4, 9, 11]), "con[1]=3"),
                         (dict(smax=0.0), "smax=0"), (dict(smax=np.inf), "smax=inf"), (dict(smax=np.nan), "smax=nan")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)


# ---- the restatement against exact arithmetic

def exact(R, x, lim, smax):
    """the largest admissible scale in exact rational arithmetic on the same doubles: (feasible, y, hi, lo, dead)"""
    nctl, ncon = len(R) - 1, R.shape[1]
    hi, lo, dead = Fraction(float(smax)), Fraction(0), False
    for i in range(ncon):
        room = Fraction(float(lim[i])) - Fraction(float(R[nctl, i]))
        D = sum((Fraction(float(x[c])) * Fraction(float(R[c, i])) for c in range(nctl)), Fraction(0))
        if D > 0:
            hi = min(hi, room / D)
        elif D < 0:
            lo = max(lo, room / D)
        elif room < 0:
            dead = True
    feas = (not dead) and lo <= hi
    return feas, (hi if feas else Fraction(0)), hi, lo, dead


def random_case(nctl, seed):
    """ncon = 12 outputs, 8 patterns, 3 members, without cancellation in D: per output one sign for every r_c, per pattern one sign
    for every x_c, zeros among both; outputs whose r is 0 throughout (D == 0), with room < 0 in one member; limits on both sides of b"""
    rng = np.random.default_rng(seed)
    nens, ncon, npat = 3, 12, 8
    sign_i = rng.choice([-1.0, 1.0], ncon, p=[0.3, 0.7])
    R = np.zeros((nens, nctl + 1, ncon))
    R[:, :nctl] = rng.uniform(0.05, 2.0, (nens, nctl, ncon)) * sign_i
    R[:, :nctl] *= rng.random((nens, nctl, ncon)) > 0.15           # zeros among the responses
    R[:, :nctl, 4] = 0.0                                            # D == 0 for every pattern
    R[:, nctl] = rng.uniform(-0.5, 1.0, (nens, ncon))
    lim = R[0, nctl] + rng.uniform(0.2, 3.0, ncon)
    if seed % 3:
        lim[[2, 9]] -= 3.5                                          # room < 0 in every member
    lim[4] = R[:, nctl, 4].max() + 0.1
    lim[4] -= (R[1, nctl, 4] - R[:, nctl, 4].min() + 0.2) * (seed % 2)      # odd seeds: room < 0 at the D == 0 output for some members
    x = rng.uniform(0.1, 2.0, (npat, nctl)) * rng.choice([-1.0, 1.0], (npat, 1), p=[0.3, 0.7])
    x *= rng.random((npat, nctl)) > 0.2
    x[5] = 0.0                                                      # a pattern of all zeros
    return R, x, lim, np.arange(0, 3 * ncon, 3, dtype=np.int32)


@pytest.mark.parametrize("nctl", range(1, 9))
def test_restatement_against_exact_arithmetic(nctl):
    seen = dict(neg=0, zero=0, dead=0, room_neg=0, infeasible=0, feasible=0, bound_by_output=0)
    worst = Fraction(0)
    bound = (nctl + 2) * U
    for seed in range(6):
        R, x, lim, con = random_case(nctl, 100 * nctl + seed)
        smax = 5.0
        got = Y.ratio_test(R, x, lim, con, smax)
        assert got["nbad"] == 0
        for m in range(len(R)):
            room = lim - R[m, nctl]
            seen["room_neg"] += int((room < 0).sum())
            for p in range(len(x)):
                feas, y, hi, lo, dead = exact(R[m], x[p], lim, smax)
                seen["dead"] += dead
                seen["neg"] += lo > 0
                seen["feasible" if feas else "infeasible"] += 1
                assert bool(got["dead"][m, p]) == dead, (seed, m, p)
                for name, want in (("hi", hi), ("lo", lo)):
                    err = abs(Fraction(float(got[name][m, p])) - want)
                    assert err <= bound * abs(want), (name, seed, m, p, float(err / abs(want)) if want else None)
                    if want:
                        worst = max(worst, err / abs(want))
                if abs(hi - lo) > bound * (abs(hi) + abs(lo)) or dead:
                    assert bool(got["fe"][m, p]) == feas, (seed, m, p)
                    assert abs(Fraction(float(got["y"][m, p])) - y) <= bound * abs(y), (seed, m, p)
                if got["bind"][m, p] >= 0:
                    seen["bound_by_output"] += 1
                    assert got["hi"][m, p] <= smax and got["bind"][m, p] in con
                else:
                    assert got["hi"][m, p] == smax
        seen["zero"] += len(R) * len(x)                             # output 4 has D == 0 under every pattern
    print(f"[yield restatement] nctl={nctl}: worst relative error of hi, lo against exact arithmetic {float(worst / U):.3f} u, "
          f"bound {nctl + 2} u; cases {seen}")
    assert all(v > 0 for v in seen.values()), seen


def test_restated_rules():
    """ties take the lowest con; a candidate equal to smax binds; -1 where none reaches smax; an invalid member is NaN and counted"""
    R = np.array([[[1.0, 2.0, 1.0, 0.5], [0.0, 0.0, 0.0, 0.0]],
                  [[1.0, np.nan, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]])
    lim, con = np.array([2.0, 4.0, 2.0, 4.0]), np.array([5, 7, 9, 30], np.int32)
    out = Y.ratio_test(R, [[1.0], [0.25], [0.125]], lim, con, 8.0)
    assert out["hi"][0].tolist() == [2.0, 8.0, 8.0] and out["bind"][0].tolist() == [5, 5, -1] and out["y"][0].tolist() == [2.0, 8.0, 8.0]
    assert np.isnan(out["y"][1]).all() and np.isnan(out["fe"][1]).all() and (out["bind"][1] == -1).all() and out["nbad"] == 1
    red = Y.reduce_members(out["y"], out["fe"], None, [0.5], [1.0])
    assert red["nfin"].tolist() == [1, 1, 1] and red["mean"].tolist() == [2.0, 8.0, 8.0] and red["pfeas"].tolist() == [1.0, 1.0, 1.0]
    assert red["quant"][0].tolist() == [2.0, 8.0, 8.0] and red["pexc"][0].tolist() == [1.0, 1.0, 1.0]


# ---- the Python front end

def test_python_front_end_without_a_gpu():
    import torch
    from unconfined_amd import WellField
    field = WellField(WELLS, LOCATIONS, TIMES)
    plan = types.SimpleNamespace(_h=None)
    thetas = [(1.0, 1e-4), (1.1, 2e-4)]
    good = dict(plan=plan, free=["Kr", "Ss"], thetas=thetas, z=[145.7, 100.0], controls=[0, 1, -1, 0], patterns=[(1.0, 1.0), (0.5, 2.0)], limit=2.0, smax=3.0)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return field.sustainable_yield(**a)

    for kw in (dict(thetas=[(1.0, 1e-4, 3.0)]), dict(controls=[0, 1, -1]), dict(patterns=[(1.0,), (0.5,)]), dict(limit=np.ones((6, 5))),
               dict(weights=[1.0]), dict(patterns=np.zeros((2, 0)))):
        with pytest.raises(ValueError):
            call(**kw)
    # what the library refuses reaches the caller with its offender
    for kw, offender in ((dict(smax=0.0), "smax=0"), (dict(controls=[0, 0, -1, 0]), "control 1 owns no well"), (dict(limit=np.inf), "no finite limit"),
                         (dict(patterns=[(1.0, np.nan)]), "x[1]"), (dict(weights=[0.0, 0.0]), "weights are 0")):
        with pytest.raises(ucflib.UcfError) as e:
            call(**kw)
        assert e.value.status == BAD and offender in e.value.message, (kw, e.value.message)
    with pytest.raises(ucflib.UcfError) as e:
        call(limit=np.where(np.arange(NOUT).reshape(6, 5, 2) % 7 == 0, 2.0, np.inf), levels=[1.0], weights=[1.0, 0.5])
    assert (e.value.status == NO_DEVICE) if not torch.cuda.is_available() else ("plan" in e.value.message)
    field.close()
