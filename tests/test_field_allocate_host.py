"""The host half of ucf_field_allocate (include/ucf.h): every refusal of ucf_field_allocate, ucf_debug_field_allocate,
ucf_allocate_solve and ucf_allocate_select with its offender named and without a device; ucf_allocate_solve, the host twin of
field_allocate_kernel, against the numpy restatement (tests/field_allocate_restate.py) byte for byte on everything the kernel test
uses; programmes whose answer is known in closed form; degenerate programmes; an exact certificate of optimality in rational
arithmetic; the reliability stage on synthetic slots; the declarations and the Python front end.  No GPU is needed.

The certificate has no tolerance: for the reported working set B x = beta and B' lambda = w are solved in fractions.Fraction on
the SAME doubles (beta of an output row is limit - b in exact arithmetic), every one of the 2 nctl + ncon constraints must hold
at that vertex and every multiplier must be >= 0 -- which proves the working set optimal for the double data.  Only then is the
computed x compared with the exact vertex, and the yardstick is not the code under test: numpy.linalg.solve (LAPACK, partial
pivoting) on the same B and the same rounded right-hand side.  A case passes when its error is at most 8 times LAPACK's on that
case; where LAPACK is exact the code must be exact."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import field_allocate_cases as K
import field_allocate_restate as A
import field_yield_restate as Y
from ensemble_weighted_restate import quantise, restate_weighted
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
NOUT = len(TIMES) * len(LOCATIONS) * 2
ENTRIES = ("ucf_field_allocate", "ucf_debug_field_allocate", "ucf_allocate_solve", "ucf_allocate_select")
MARGIN = 8
addr = K.addr


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


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
    vals = dict(re.findall(r"#define\s+(UCF_ALLOC_\w+)\s+(\(?-?[\w.+-]+\)?)", code))
    assert vals == {"UCF_ALLOC_MAX_OBJ": "8", "UCF_ALLOC_MAX_ITER": "256", "UCF_ALLOC_DTOL": "0x1p-40", "UCF_ALLOC_INVALID": "(-1)",
                    "UCF_ALLOC_OPTIMAL": "0", "UCF_ALLOC_ITERATION_CAP": "1", "UCF_ALLOC_INFEASIBLE_AT_ZERO": "2", "UCF_ALLOC_NUMERIC": "3"}
    assert (abi.UCF_ALLOC_MAX_OBJ, abi.UCF_ALLOC_MAX_ITER, abi.UCF_ALLOC_DTOL) == (8, 256, 2.0 ** -40) and A.DTOL == abi.UCF_ALLOC_DTOL
    assert (abi.UCF_ALLOC_INVALID, abi.UCF_ALLOC_OPTIMAL, abi.UCF_ALLOC_ITERATION_CAP, abi.UCF_ALLOC_INFEASIBLE_AT_ZERO, abi.UCF_ALLOC_NUMERIC) == \
        (A.INVALID, A.OPTIMAL, A.ITERATION_CAP, A.INFEASIBLE_AT_ZERO, A.NUMERIC)


# ---- refusals

LIMIT = np.full(NOUT, np.inf)
LIMIT[[3, 17, 40, 59]] = [1.0, 2.5, 0.25, 3.0]


def allocate_call(so, h, plan=None, npar=2, ids=(0, 2), nens=None, thetas=((1.0, 1e-4), (1.1, 2e-4), (0.9, 1.5e-4)), weight=None, nz=2,
                  z=(145.7, 100.0), nctl=2, ctl=(0, 1, -1, 0), nobj=None, w=((1.0, 1.0), (1.0, -0.5)), xmax=(2.0, 3.0), maxit=32, limit=LIMIT,
                  q=(0.05, 0.5), nq=None, want=("quant", "value", "best", "best_x", "gquant"), null=()):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), thetas=np.ascontiguousarray(thetas, dtype=float), z=np.ascontiguousarray(z, dtype=float),
                weight=None if weight is None else np.ascontiguousarray(weight, dtype=float), ctl=np.ascontiguousarray(ctl, dtype=np.int32),
                w=np.ascontiguousarray(w, dtype=float), xmax=np.ascontiguousarray(xmax, dtype=float), limit=np.ascontiguousarray(limit, dtype=float),
                q=np.ascontiguousarray(q, dtype=float))
    nens = len(arrs["thetas"]) if nens is None else nens
    nobj = len(arrs["w"]) if nobj is None else nobj
    nq = len(arrs["q"]) if nq is None else nq
    for k in null:
        arrs[k] = None
    big = np.zeros(16 * 4096 + 64)
    rel = {k: (np.zeros(len(big), np.int32) if k == "best" else big.copy()) if k in want else None for k in ("quant", "value", "best", "best_x", "gquant")}
    con, ncon = np.full(NOUT, -7, np.int32), C.c_int(-7)
    u, ess, nl = np.zeros(max(nens, 1), np.uint64), C.c_double(-1.0), C.c_int(-1)
    rc = so.ucf_field_allocate(h, plan, npar, addr(arrs["ids"]), nens, addr(arrs["thetas"]), addr(arrs["weight"]), nz, addr(arrs["z"]), nctl,
                               addr(arrs["ctl"]), nobj, addr(arrs["w"]), addr(arrs["xmax"]), maxit, addr(arrs["limit"]), None, None, None, None, None,
                               None, nq, addr(arrs["q"]), *(addr(rel[k]) for k in ("quant", "value", "best", "best_x", "gquant")), None, addr(con),
                               C.addressof(ncon), None, None, addr(u), C.addressof(ess), C.addressof(nl))
    return rc, msg_of(so), dict(con=con, ncon=ncon.value, u=u, ess=ess.value, nlaunched=nl.value)


def test_allocate_refusals_name_the_offender(so):
    import torch
    h = create(so)
    nanlim, neglim = LIMIT.copy(), LIMIT.copy()
    nanlim[5], neglim[7] = np.nan, -np.inf
    many = np.tile([[1.0, 1e-4]], (600, 1))
    cases = [
        # what ucf_field_yield checks on the shared arguments
        (dict(nz=0), "nz"), (dict(z=(145.7, np.nan)), "z[1]"), (dict(null=("z",)), "NULL z"), (dict(null=("ids",)), "NULL ids"),
        (dict(null=("thetas",)), "NULL thetas"), (dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nens=0), "nens=0"),
        (dict(nens=1025), "nens=1025"), (dict(nq=17), "nq=17"), (dict(q=(0.5, 1.5)), "q[1]"), (dict(null=("q",)), "NULL q"),
        (dict(nq=0), "quant is asked for"), (dict(nq=0, want=("gquant",)), "quant is asked for"),
        (dict(thetas=((1.0, 1e-4), (1.1, -2e-4))), "member 1"), (dict(thetas=((np.inf, 1e-4),)), "member 0"),
        (dict(null=("ctl",)), "NULL ctl"), (dict(null=("limit",)), "NULL limit"), (dict(nctl=0), "nctl=0"), (dict(nctl=9), "nctl=9"),
        # the programme
        (dict(nobj=0), "nobj=0"), (dict(nobj=9), "nobj=9"), (dict(null=("w",)), "NULL w"), (dict(null=("xmax",)), "NULL xmax"),
        (dict(w=((1.0, 1.0), (np.nan, 1.0))), "w[2]"), (dict(w=((1.0, np.inf),)), "w[1]"), (dict(xmax=(2.0, 0.0)), "xmax[1]=0"),
        (dict(xmax=(-1.0, 1.0)), "xmax[0]=-1"), (dict(xmax=(np.inf, 1.0)), "xmax[0]=inf"), (dict(xmax=(1.0, np.nan)), "xmax[1]=nan"),
        (dict(maxit=0), "maxit=0"), (dict(maxit=257), "maxit=257"),
        (dict(thetas=many, nobj=8, w=np.ones((8, 2))), "600 members x 8 objectives are more than 4096"),
        # the controls and the limits, after the programme
        (dict(ctl=(0, 1, 2, 0)), "ctl[2]=2"), (dict(ctl=(-2, 1, 0, 0)), "ctl[0]=-2"), (dict(ctl=(0, 0, -1, 0)), "control 1 owns no well"),
        (dict(limit=nanlim), "limit[5]"), (dict(limit=neglim), "limit[7]"), (dict(limit=np.full(NOUT, np.inf)), "no finite limit"),
        # the weights, after everything else
        (dict(weight=(1.0, -1.0, 1.0)), "member 1: weight"), (dict(weight=(0.0, 0.0, 0.0)), "all 3 weights"),
    ]
    for kw, offender in cases:
        rc, msg, _ = allocate_call(so, h, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg, _ = allocate_call(so, None)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device.  con, ncon and the
    # integer weights are written by the checks.  Without the reliability stage nq may be 0 and nens nobj is not limited.
    for kw in (dict(), dict(weight=(1.0, 0.0, 0.25)), dict(nq=0, want=()), dict(thetas=many, nobj=8, w=np.ones((8, 2)), want=("gquant",)),
               dict(maxit=256, nobj=8, w=np.zeros((8, 2)))):
        rc, msg, out = allocate_call(so, h, **kw)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
        want = np.flatnonzero(np.isfinite(LIMIT))
        assert out["ncon"] == len(want) and out["con"][:len(want)].tolist() == want.tolist() and (out["con"][len(want):] == -7).all()
        if "weight" in kw:
            assert out["u"].tolist() == [2 ** 32, 0, 2 ** 30] and out["nlaunched"] == 2 and out["ess"] > 1.0
        else:
            assert out["nlaunched"] == -1 and out["ess"] == -1.0
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_entries_on_caller_data_check_then_run(so):
    """ucf_debug_field_allocate asks for a device after its checks; ucf_allocate_solve and ucf_allocate_select need none"""
    import torch
    nctl, nens, ncon, nobj = 2, 3, 5, 2
    R = np.arange(nens * (nctl + 1) * ncon, dtype=float).reshape(nens, nctl + 1, ncon) / 64.0
    lim, con = np.linspace(9.0, 10.0, ncon), np.array([0, 3, 4, 9, 11], np.int32)
    w, xmax = np.array([[1.0, 1.0], [0.0, -1.0]]), np.array([1.0, 2.0])
    nanw, inflim, zerocap = w.copy(), lim.copy(), xmax.copy()
    nanw[1, 0], inflim[2], zerocap[1] = np.nan, np.inf, 0.0
    o = K.outputs(nens, nobj, nctl)
    nbad = C.c_longlong()

    def call(nctl=nctl, nens=nens, ncon=ncon, nobj=nobj, R=R, lim=lim, con=con, w=w, xmax=xmax, maxit=16):
        con = None if con is None else np.ascontiguousarray(con, dtype=np.int32)
        rc = so.ucf_debug_field_allocate(nctl, nens, ncon, nobj, addr(R), addr(lim), addr(con), addr(w), addr(xmax), maxit,
                                         *(addr(o[k]) for k in K.ORDER), C.addressof(nbad))
        return rc, msg_of(so)

    def solve(nctl=nctl, nens=None, ncon=ncon, nobj=nobj, R=R, lim=lim, con=None, w=w, xmax=xmax, maxit=16):
        rc = so.ucf_allocate_solve(nctl, ncon, addr(R), addr(lim), nobj, addr(w), addr(xmax), maxit, *(addr(o[k]) for k in K.ORDER))
        return rc, msg_of(so)

    shared = ((dict(nctl=0), "nctl=0"), (dict(nctl=9), "nctl=9"), (dict(ncon=0), "ncon=0"), (dict(nobj=0), "nobj=0"), (dict(nobj=9), "nobj=9"),
              (dict(maxit=0), "maxit=0"), (dict(maxit=257), "maxit=257"), (dict(R=None), "NULL R"), (dict(lim=None), "NULL limit_con"),
              (dict(w=None), "NULL w"), (dict(xmax=None), "NULL xmax"), (dict(w=nanw), "w[2]"), (dict(lim=inflim), "limit_con[2]"),
              (dict(xmax=zerocap), "xmax[1]=0"))
    own = ((dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"), (dict(nens=1024, ncon=1 << 20), "more than 2^31-1"), (dict(con=None), "NULL con"),
           (dict(con=[0, 3, 3, 9, 11]), "con[2]=3"), (dict(con=[-1, 3, 4, 9, 11]), "con[0]=-1"), (dict(con=[5, 3, 4, 9, 11]), "con[1]=3"))
    for kw, offender in shared + own:
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    for kw, offender in shared:
        rc, msg = solve(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)
    # every output of ucf_allocate_solve may be NULL
    assert so.ucf_allocate_solve(nctl, ncon, addr(R[0]), addr(lim), nobj, addr(w), addr(xmax), 16, None, None, None, None, None, None) == 0
    quant, g, x = np.ones((2, 6)), np.ones((3, 2)), np.ones((3, 2, 2))
    for args, offender in (((0, 3, 2, 2), "nq=0"), ((17, 3, 2, 2), "nq=17"), ((2, 0, 2, 2), "nens=0"), ((2, 3, 9, 2), "nobj=9"), ((2, 3, 2, 0), "nctl=0")):
        assert so.ucf_allocate_select(*args, addr(quant), addr(g), addr(x), None, None, None) == BAD and offender in msg_of(so), args
    for k, name in enumerate(("quant", "g", "x")):
        arrs = [addr(quant), addr(g), addr(x)]
        arrs[k] = None
        assert so.ucf_allocate_select(2, 3, 2, 2, *arrs, None, None, None) == BAD and f"NULL {name}" in msg_of(so)
    assert so.ucf_allocate_select(2, 3, 2, 2, addr(quant), addr(g), addr(x), None, None, None) == 0


# ---- the host twin against the restatement, byte for byte

@pytest.mark.parametrize("nctl", range(1, 9))
def test_host_twin_is_the_restatement_on_what_the_kernel_test_uses(so, nctl):
    seen = set()
    for ncon in K.NCONS:
        R, lim, w, xmax = K.kernel_case(nctl, ncon)
        want = A.allocate(R, lim, w, xmax, K.MAXIT)
        assert want["status"][:, 0].tolist() == [A.OPTIMAL, A.INVALID, A.INFEASIBLE_AT_ZERO] and want["nbad"] == 1
        K.same_bytes(K.host_solve(so, R, lim, w, xmax, K.MAXIT), want, ncon)
        seen |= set(want["iters"].ravel().tolist())
    R, lim, w, xmax = K.kernel_case(nctl, 257)
    want = A.allocate(R, lim, w, xmax, 1)
    assert want["status"][0, 0] == A.ITERATION_CAP and want["iters"][0, 0] == 1 and np.isnan(want["x"][0, 0]).all() and (want["work"][0, 0] == -1).all()
    K.same_bytes(K.host_solve(so, R, lim, w, xmax, 1), want, "maxit 1")
    assert len(seen) >= min(3, nctl + 1), seen                     # programmes of several lengths (one control: 0 or 1 pivots)


def test_degenerate_programmes(so):
    """duplicated rows, rows through a corner of the box, a row through the origin: status 0 or 1 within maxit, and the C code
    and the restatement agree byte for byte whichever it is"""
    for name, R, lim, w, xmax in K.degenerate_cases():
        want = A.allocate(R, lim, w, xmax, K.MAXIT)
        assert set(want["status"].ravel().tolist()) <= {A.OPTIMAL, A.ITERATION_CAP}, (name, want["status"])
        K.same_bytes(K.host_solve(so, R, lim, w, xmax, K.MAXIT), want, name)
        if name == "duplicated rows":
            # rows 1 and 3 are the same and the tightest: id 2 nctl + 1 = 5 enters, never 7
            assert want["status"].tolist() == [[0, 0]] and want["work"].tolist() == [[[1, 5], [0, 5]]]
            assert want["x"].tolist() == [[[2.0, 0.0], [0.0, 1.0]]] and want["g"].tolist() == [[2.0, 3.0]]
        if name == "corner of the box":
            # nctl + 1 = 3 and more constraints meet in (1, 1); the two upper bounds are the lowest ids among them
            assert (want["status"] == 0).all() and (want["x"] == 1.0).all() and (want["work"] == [2, 3]).all()
        if name == "corner in three dimensions":
            assert (want["status"] == 0).all() and (want["x"] == 1.0).all() and (want["work"] == [3, 4, 5]).all()
        if name == "row through the origin":
            assert (want["status"] == 0).all() and (want["x"] == 0.0).all() and want["iters"].tolist() == [[1, 1]]     # one pivot of step 0
        if name.startswith("every output twice"):
            single = A.allocate(R[:, :, ::2], lim[::2], w, xmax, K.MAXIT)
            assert (want["status"] == 0).all() and (single["status"] == 0).all()
            rows = want["work"][want["work"] >= 2 * (R.shape[1] - 1)] - 2 * (R.shape[1] - 1)
            assert len(rows) > 0 and (rows % 2 == 0).all()             # of two equal rows the lower id is the one that binds
            assert np.allclose(want["g"], single["g"], rtol=1e-12, atol=0.0), name


# ---- programmes whose answer is known

def one(so, R, lim, w, xmax, maxit=K.MAXIT):
    """one member, one objective through ucf_allocate_solve, held to the restatement on the way"""
    R = np.asarray(R, dtype=float)[None]
    got = K.host_solve(so, R, lim, [w], xmax, maxit)
    K.same_bytes(got, A.allocate(R, lim, [w], xmax, maxit), "closed form")
    return {k: got[k][0, 0] for k in K.ORDER}


def test_closed_forms(so):
    # one control: the least room / r, or xmax
    r, b, lim = np.array([0.5, 0.3, -0.2, 0.0, 0.7]), np.array([0.1, 0.2, 0.0, 0.3, 0.05]), np.array([1.1, 1.0, 0.5, 0.4, 2.0])
    out = one(so, [r, b], lim, [1.0], [10.0])
    cand = [(lim[i] - b[i]) / r[i] for i in (0, 1, 4)]
    assert out["status"] == 0 and out["x"][0] == min(cand) == 2.0 and out["work"].tolist() == [2 + 0] and out["iters"] == 1
    assert out["g"] == 2.0 and out["lam"][0] == 1.0 / r[0]                  # a unit of limit buys 1 / r of rate
    out = one(so, [r, b], lim, [1.0], [1.5])
    assert out["status"] == 0 and out["x"][0] == 1.5 and out["work"].tolist() == [1] and out["lam"][0] == 1.0
    # two controls, a box and one row: x0 + 2 x1 <= 4 in [0, 3] x [0, 3]; w = (1, 1) ends in (3, 0.5), w = (1, 3) in (0, 2)
    R2 = [[1.0], [2.0], [0.0]]
    out = one(so, R2, [4.0], [1.0, 1.0], [3.0, 3.0])
    assert out["status"] == 0 and out["x"].tolist() == [3.0, 0.5] and out["g"] == 3.5 and out["work"].tolist() == [2, 4] and out["lam"].tolist() == [0.5, 0.5]
    out = one(so, R2, [4.0], [1.0, 3.0], [3.0, 3.0])
    assert out["status"] == 0 and out["x"].tolist() == [0.0, 2.0] and out["g"] == 6.0 and out["work"].tolist() == [0, 4] and out["lam"].tolist() == [0.5, 1.5]
    # w = 0: nothing to gain, x = 0 without a pivot
    out = one(so, R2, [4.0], [0.0, 0.0], [3.0, 3.0])
    assert out["status"] == 0 and out["iters"] == 0 and (out["x"] == 0.0).all() and out["g"] == 0.0 and out["work"].tolist() == [0, 1]
    # a negative weight: the control stays at 0
    out = one(so, R2, [4.0], [1.0, -1.0], [3.0, 3.0])
    assert out["status"] == 0 and out["x"].tolist() == [3.0, 0.0] and out["work"].tolist() == [1, 2] and out["lam"].tolist() == [1.0, 1.0]
    # an all-zero row never binds, whatever its room (zero included)
    out = one(so, [[1.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.5, 0.0]], [4.0, 0.5, 7.0], [1.0, 1.0], [3.0, 3.0])
    assert out["status"] == 0 and out["x"].tolist() == [3.0, 0.5] and out["work"].tolist() == [2, 4]
    # a negative response (a recharge image in the control): control 1 relieves the row, x0 + ... - 0.5 x1 <= 2 with x1 <= 2 gives x0 = 3
    out = one(so, [[1.0], [-0.5], [0.0]], [2.0], [1.0, 0.0], [5.0, 2.0])
    assert out["status"] == 0 and out["x"].tolist() == [3.0, 2.0] and out["g"] == 3.0 and out["work"].tolist() == [3, 4]
    # a negative room: the fixed wells alone exceed a limit
    out = one(so, [[1.0, 1.0], [2.0, 1.0], [0.0, 1.5]], [4.0, 1.0], [1.0, 1.0], [3.0, 3.0])
    assert out["status"] == 2 and out["iters"] == 0 and np.isnan(out["x"]).all() and np.isnan(out["g"]) and np.isnan(out["lam"]).all() and (out["work"] == -1).all()
    # a slot that is not finite: the member is invalid, whatever else holds
    for bad in (np.nan, np.inf, -np.inf):
        out = one(so, [[1.0, 1.0], [2.0, bad], [0.0, 1.5]], [4.0, 1.0], [1.0, 1.0], [3.0, 3.0])
        assert out["status"] == -1 and out["iters"] == 0 and np.isnan(out["x"]).all() and (out["work"] == -1).all()


# ---- the exact certificate

def frac_solve(M, b):
    n = len(b)
    M = [row[:] + [b[r]] for r, row in enumerate(M)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [u - f * v for u, v in zip(M[r], M[c])]
    return [M[r][n] / M[r][r] for r in range(n)]


def exact_rows(Rm, lim, xmax, n):
    """every constraint (a, beta) in exact arithmetic on the doubles, by id"""
    rows = []
    for c in range(n):
        rows.append(([Fraction(-1 if k == c else 0) for k in range(n)], Fraction(0)))
    for c in range(n):
        rows.append(([Fraction(1 if k == c else 0) for k in range(n)], Fraction(float(xmax[c]))))
    for i in range(Rm.shape[1]):
        rows.append(([Fraction(float(Rm[c, i])) for c in range(n)], Fraction(float(lim[i])) - Fraction(float(Rm[n, i]))))
    return rows


def certify(Rm, lim, w, xmax, out):
    """proves out["work"] optimal in exact arithmetic; returns (the exact vertex, the exact optimum)"""
    n = len(w)
    rows = exact_rows(Rm, lim, xmax, n)
    B = [rows[j][0] for j in out["work"]]
    xe = frac_solve([r[:] for r in B], [rows[j][1] for j in out["work"]])
    le = frac_solve([[B[c][r] for c in range(n)] for r in range(n)], [Fraction(float(v)) for v in w])
    for j, (a, beta) in enumerate(rows):
        assert sum(ac * xc for ac, xc in zip(a, xe)) <= beta, ("constraint violated at the exact vertex", j)
    assert all(v >= 0 for v in le), ("negative exact multiplier", le)
    return xe, sum(Fraction(float(wc)) * xc for wc, xc in zip(w, xe))


CERT_NCON, CERT_SEEDS = 40, range(20)


def certificate_cases(nctl):
    for seed in CERT_SEEDS:
        R, lim, w, xmax = K.generic(nctl, CERT_NCON, 50000 + 100 * nctl + seed)
        yield seed, R[0], lim, w[seed % 2], xmax


def lapack_error(Rm, lim, xmax, work, xe):
    """the error of numpy.linalg.solve on the working rows in double and the rounded right-hand sides that the code uses"""
    n = len(xe)
    rows = [A.row_of(Rm, lim, xmax, n, int(j)) for j in work]
    xl = np.linalg.solve(np.array([a for a, _ in rows], dtype=float), np.array([b for _, b in rows], dtype=float))
    return max(abs(Fraction(float(xl[c])) - xe[c]) for c in range(n))


def certificate_ratios(so, nctl):
    """per case of certificate_cases the error of x against the exact vertex over that of LAPACK (None: both exact)"""
    ratios = []
    for seed, Rm, lim, w, xmax in certificate_cases(nctl):
        out = one(so, Rm, lim, w, xmax)
        assert out["status"] == A.OPTIMAL, (nctl, seed, out["status"])
        xe, _ = certify(Rm, lim, w, xmax, out)
        err = max(abs(Fraction(float(out["x"][c])) - xe[c]) for c in range(nctl))
        ref = lapack_error(Rm, lim, xmax, out["work"], xe)
        assert err <= MARGIN * ref, (nctl, seed, float(err), float(ref))
        ratios.append(float(err / ref) if ref else None)
    return ratios


@pytest.mark.parametrize("nctl", range(1, 9))
def test_exact_certificate(so, nctl):
    ratios = certificate_ratios(so, nctl)
    some = [r for r in ratios if r is not None]
    print(f"[allocate certificate] nctl={nctl}: {len(ratios)} working sets proven optimal in exact arithmetic; error of x over LAPACK's on the same "
          f"system: worst {max(some) if some else 0.0:.3f}, both exact in {len(ratios) - len(some)} cases; margin {MARGIN}")


@pytest.mark.parametrize("nctl", range(1, 9))
def test_against_highs(so, nctl):
    """g against scipy.optimize.linprog(method="highs"); the bar is HiGHS's own distance from the exact optimum of the same case,
    times 8, per case.  HiGHS's g is now and then the correctly rounded exact optimum, a small fraction of an ulp from it, and
    the bar is then below one ulp: only the correctly rounded double passes.  That is what the polish of the contract is for
    -- x and g of the final working set in double-double, g rounded once; without it 6 of these 160 cases missed the bar by
    one or two ulp of g."""
    linprog = pytest.importorskip("scipy.optimize").linprog
    worst = 0.0
    for seed, Rm, lim, w, xmax in certificate_cases(nctl):
        out = one(so, Rm, lim, w, xmax)
        _, ge = certify(Rm, lim, w, xmax, out)
        res = linprog(-np.asarray(w), A_ub=Rm[:nctl].T, b_ub=lim - Rm[nctl], bounds=[(0.0, float(v)) for v in xmax], method="highs")
        assert res.status == 0, (nctl, seed, res.message)
        ref = abs(Fraction(float(-res.fun)) - ge)
        err = abs(Fraction(float(out["g"])) - ge)
        assert err <= MARGIN * ref, (nctl, seed, float(err), float(ref))
        if ref:
            worst = max(worst, float(err / ref))
    print(f"[allocate HiGHS] nctl={nctl}: worst error of g over HiGHS's {worst:.3f}, margin {MARGIN}")


# ---- the reliability stage on synthetic slots

def reliability(so, R, lim, w, xmax, q, u=None):
    """the stage as include/ucf.h states it from the restatements under tests/, with ucf_allocate_select for the host step"""
    con = np.arange(len(lim), dtype=np.int32)
    sol = K.host_solve(so, R, lim, w, xmax, K.MAXIT)
    pats = A.patterns(sol["x"], sol["status"])
    y = Y.ratio_test(R, pats, lim, con, 1.0)["y"]
    quant = Y.quantile_linear(y, q) if u is None else restate_weighted(y, u, list(q), [])["quant"]
    nens, nobj, nctl = sol["x"].shape
    value, best, best_x = np.zeros_like(quant), np.zeros((len(q), nobj), np.int32), np.zeros((len(q), nobj, nctl))
    ucflib.check(so.ucf_allocate_select(len(q), nens, nobj, nctl, addr(np.ascontiguousarray(quant)), addr(sol["g"]), addr(sol["x"]), addr(value),
                                        addr(best), addr(best_x)))
    return sol, y, quant, value, best, best_x


def same_with_nan(got, want, what):
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all(), what
    assert got[~np.isnan(want)].tobytes() == want[~np.isnan(want)].tobytes(), what


@pytest.mark.parametrize("weights", [None, (1.0, 0.5, 0.0, 2.0, 1.0)])
def test_reliability_stage(so, weights):
    R, lim, w, xmax = K.generic(3, 30, 4242, nens=5)
    R[3, 1, 7] = np.nan                                            # a member without an optimum: its pattern is all zeros
    q = (0.0, 0.05, 0.5, 1.0)
    u = None if weights is None else quantise(list(weights))[0]
    sol, y, quant, value, best, best_x = reliability(so, R, lim, w, xmax, q, u)
    want_value, want_best, want_x = A.select(quant, sol["g"], sol["x"])
    same_with_nan(value, want_value, "value")
    assert np.array_equal(best, want_best)
    same_with_nan(best_x, want_x, "best_x")
    nens, nobj = sol["g"].shape
    assert (sol["status"][3] == A.INVALID).all() and np.isnan(y[3]).all() and np.isnan(value[:, 3 * nobj:4 * nobj]).all()
    assert (y[[0, 1, 2, 4]] <= 1.0).all() and (y[[0, 1, 2, 4]] >= 0.0).all()
    for m in (0, 1, 2, 4):
        assert (y[m, m * nobj:(m + 1) * nobj] > 1.0 - 1e-12).all()       # a member admits its own optimum
    assert (best >= 0).all() and (best // nobj != 3).all() and (best % nobj == np.arange(nobj)).all()
    live = [m for m in (0, 1, 2, 4) if u is None or u[m] > 0]
    for iq in range(len(q)):
        for o in range(nobj):
            p = best[iq, o]
            assert value[iq, p] == np.nanmax(value[iq, o::nobj]) and best_x[iq, o].tolist() == (quant[iq, p] * sol["x"].reshape(-1, 3)[p]).tolist()
            # the chosen allocation is admissible, within rounding, for the share of members that its level promises
            ok = [m for m in live if (R[m, :3].T @ best_x[iq, o] + R[m, 3] <= lim * (1.0 + 1e-12)).all()]
            mass = len(ok) if u is None else sum(int(u[m]) for m in ok)
            total = len(live) if u is None else sum(int(u[m]) for m in live)
            assert mass >= (1.0 - q[iq]) * total - 1e-9 * total - (1 if u is None else 0), (iq, o, ok)
    assert (best_x <= xmax).all()


def test_reliability_tie_takes_the_lowest_candidate(so):
    """members 0 and 2 have the same slots: their optima and values are the same bits, and the lower candidate is chosen"""
    R, lim, w, xmax = K.generic(2, 12, 99, nens=3)
    R[2] = R[0]
    R[1, :2] *= 4.0                                                # member 1 is far tighter: its optimum is worth less
    sol, y, quant, value, best, best_x = reliability(so, R, lim, w, xmax, (1.0,))
    nobj = 2
    assert value[0, 0] == value[0, 2 * nobj] and value[0, 0] > value[0, nobj] and best[0, 0] == 0
    want_value, want_best, _ = A.select(quant, sol["g"], sol["x"])
    assert np.array_equal(best, want_best) and value.tobytes() == want_value.tobytes()
    # and on constructed numbers: equal values, a NaN between them, -1 where every value is NaN
    quant = np.array([[0.5, 1.0, 1.0, 1.0, 0.25, 1.0]])
    g = np.array([[4.0, np.nan], [np.nan, np.nan], [8.0, np.nan]])
    x = np.arange(12, dtype=float).reshape(3, 2, 2)
    value, best, best_x = np.zeros((1, 6)), np.zeros((1, 2), np.int32), np.zeros((1, 2, 2))
    assert so.ucf_allocate_select(1, 3, 2, 2, addr(quant), addr(g), addr(x), addr(value), addr(best), addr(best_x)) == 0
    assert value[0, [0, 4]].tolist() == [2.0, 2.0] and np.isnan(value[0, [1, 2, 3, 5]]).all()
    assert best.tolist() == [[0, -1]] and best_x[0, 0].tolist() == [0.0, 0.5] and np.isnan(best_x[0, 1]).all()
    wv, wb, wx = A.select(quant, g, x)
    same_with_nan(value, wv, "value")
    assert np.array_equal(best, wb)
    same_with_nan(best_x, wx, "best_x")


# ---- the Python front end

def test_python_front_end_without_a_gpu():
    import torch
    from unconfined_amd import Allocation, WellField
    field = WellField(WELLS, LOCATIONS, TIMES)
    plan = types.SimpleNamespace(_h=None)
    thetas = [(1.0, 1e-4), (1.1, 2e-4)]
    good = dict(plan=plan, free=["Kr", "Ss"], thetas=thetas, z=[145.7, 100.0], controls=[0, 1, -1, 0], objectives=[(1.0, 1.0), (1.0, 0.0)], xmax=3.0,
                limit=2.0)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return field.optimal_rates(**a)

    for kw in (dict(thetas=[(1.0, 1e-4, 3.0)]), dict(controls=[0, 1, -1]), dict(objectives=[(1.0,), (0.5,)]), dict(limit=np.ones((6, 5))),
               dict(weights=[1.0]), dict(objectives=np.zeros((2, 0))), dict(xmax=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            call(**kw)
    for kw, offender in ((dict(xmax=0.0), "xmax[0]=0"), (dict(controls=[0, 0, -1, 0]), "control 1 owns no well"), (dict(limit=np.inf), "no finite limit"),
                         (dict(objectives=[(1.0, np.nan)]), "w[1]"), (dict(maxit=0), "maxit=0"), (dict(q=()), "quant is asked for"),
                         (dict(weights=[0.0, 0.0]), "weights are 0")):
        with pytest.raises(ucflib.UcfError) as e:
            call(**kw)
        assert e.value.status == BAD and offender in e.value.message, (kw, e.value.message)
    for kw in (dict(), dict(q=(), reliability=False), dict(weights=[1.0, 0.5], xmax=[2.0, 3.0])):
        with pytest.raises(ucflib.UcfError) as e:
            call(**kw)
        assert (e.value.status == NO_DEVICE) if not torch.cuda.is_available() else ("plan" in e.value.message)
    field.close()
    res = Allocation(x=np.zeros((1, 1, 2)), work=np.array([[[1, 3]]], np.int32), con=np.array([7, 11], np.int32), status=np.zeros((1, 1), np.int32), nbad=0)
    assert res.binding(0, 0) == [("lower", 1), ("upper", 1)] and res.quant is None
    res.work[0, 0] = [2, 5]
    assert res.binding(0, 0) == [("upper", 0), ("output", 11)]
