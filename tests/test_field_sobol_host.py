"""The host half of ucf_field_sobol (include/ucf.h): the declarations, every refusal of ucf_sobol_design, ucf_field_sobol and
ucf_debug_sobol with its offender named and without a device, ucf_sobol_design against its numpy restatement, the numpy
restatement of field_sobol_kernel (tests/field_sobol_restate.py) on hand-made columns -- one per branch of the statement, the
expected values written out --, the meaning of the indices on the Ishigami function and the Python front end.  No GPU is needed:
the checks come before a call asks for a device.

The hand-made columns use values for which every operation of the statement is exact in binary (n a power of two, 2n - 1 a divisor
of the summed squares, every square root that of a square), so the literals are what exact arithmetic gives.  Two columns
cannot be exact and are held to `fractions.Fraction` arithmetic of the same statement, with bounds counted from the roundings
on the path (u = 2^-53, first order in u, one u of slack for the higher orders):

the Wynn sentinel X, N = 2, A = (X, 0), B = (0, 0), AB = (0, 1).  mean = X / 4 is exact (one non-zero term, a power of two).
    da_0 = X - X/4 rounds once, da_1, db_0, db_1 = -X/4 are exact; a square adds one rounding and doubles what its argument
    carries: da_0^2 3u, the others u.  qA = sum of two: 4u; qB = twice the same term: u; qA + qB and / 3 one each: var 6u -> 7u.
    p_0 = db (0 - X) and pt_0 = X^2 round once, p_1 = -X/4 and pt_1 = 1 are exact; both pairs have one sign, so v1 and vt
    carry 2u, m1 and mt (a division by 2) and 0.5 mt the same; S and ST add var's 6u and one division: 9u -> 10u.
    q1 = p_0^2 (3u) + p_1^2 (u), summed: 4u; m1^2: 5u.  w1 = q1/2 - m1^2 cancels: q1/2 is 2 w1 and m1^2 is w1 up to 1e-6, so
    the absolute error is (2 * 4u + 5u) w1 plus the rounding of the difference: 14u.  n - 1 = 1 is exact; the root halves,
    rounds once: 8u; / var: 6u + u: 15u -> 16u.  seST in the same way with qt = pt_0^2 + pt_1^2 and mt: 16u.
the clamped w, N = 3, A = (1, -1, 0), B = (2, -2, 0), AB = A - d with d = 0x1.68c14p+0 (every difference exact): mean = 0 and
    var = 2 exactly.  pt = d^2 rounds once, pt + pt is exact, + pt and / 3 round once each: mt 3u, 0.5 mt / 2 exact: ST 3u -> 4u.
    p = fb (-d) = -2d, 2d, 0 exactly: v1 = 0 and S = +0.0.  p^2 = 4 d^2 rounds once, their sum is exact (a doubling), / 3
    rounds: w1 2u; / 2 exact, the root halves and rounds once: 2u; / 2 exact: seS 2u -> 3u.  The computed wt is negative, where
    exact arithmetic gives 0: seST = +0.0 exactly."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import field_sobol_restate as R
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
ENTRIES = ("ucf_sobol_design", "ucf_field_sobol", "ucf_debug_sobol")
MAP_KEYS = ("S", "ST", "seS", "seST", "mean", "var", "nrow")
SENTINEL = -999999.9
nan, inf = np.nan, np.inf
# 2 N = 6 draws of two parameters, and their design
DRAWS = np.array([[1.0, 1e-4], [1.1, 2e-4], [0.9, 1.5e-4], [1.2, 1.25e-4], [0.8, 3e-4], [1.05, 0.5e-4]])
DESIGN = R.design(DRAWS)


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


def test_header_exports_and_mirror(so):
    """fails on the parent: the symbols and the struct do not exist there"""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucf.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s) and getattr(so, s).argtypes is not None, s
    limit = re.search(r"#define\s+UCF_SOBOL_MAX_BASE\s+(\d+)", code)
    assert limit and int(limit.group(1)) == abi.UCF_SOBOL_MAX_BASE == 1024
    # the struct: its members in the header's order, all of them addresses, are those of the mirror
    body = re.search(r"typedef\s+struct\s+ucf_sobol_maps\s*\{(.*?)\}\s*ucf_sobol_maps\s*;", code, flags=re.S)
    assert body, "ucf.h does not declare ucf_sobol_maps"
    members = []
    for decl in body.group(1).split(";"):
        if decl.strip():
            kind, names = decl.strip().split(None, 1)
            assert kind in ("double", "int"), decl
            for name in names.split(","):
                assert name.strip().startswith("*"), decl
                members.append(name.strip().lstrip("*").strip())
    assert members == [n for n, _ in abi.UcfSobolMaps._fields_] == ["S", "ST", "seS", "seST", "mean", "var", "all", "nrow"]
    assert all(t is C.c_void_p for _, t in abi.UcfSobolMaps._fields_) and C.sizeof(abi.UcfSobolMaps) == 8 * C.sizeof(C.c_void_p)
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


# ---- refusals

def design_call(so, npar=2, nbase=3, draws=DRAWS, null=()):
    draws = np.ascontiguousarray(draws, dtype=float)
    out = np.zeros(((max(npar, 0) + 2) * max(nbase, 1), max(npar, 1)))
    rc = so.ucf_sobol_design(npar, nbase, None if "draws" in null else addr(draws), None if "thetas" in null else addr(out))
    return rc, msg_of(so), out


def changed(a, at, value):
    a = np.array(a, dtype=float)
    a[at] = value
    return a


def test_design_refusals_name_the_offender(so):
    for kw, offender in ((dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nbase=1), "nbase=1"), (dict(nbase=0), "nbase=0"),
                         (dict(nbase=1025), "nbase=1025"), (dict(null=("draws",)), "NULL draws"), (dict(null=("thetas",)), "NULL thetas"),
                         (dict(draws=changed(DRAWS, (3, 1), 0.0)), "draws[3][1]=0"), (dict(draws=changed(DRAWS, (3, 1), -1.0)), "row 3, parameter 1"),
                         (dict(draws=changed(DRAWS, (5, 0), inf)), "row 5, parameter 0"), (dict(draws=changed(DRAWS, (0, 0), nan)), "row 0, parameter 0")):
        rc, msg, _ = design_call(so, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)


def sobol_call(so, h, plan=None, npar=2, ids=(0, 2), nbase=3, thetas=DESIGN, nz=2, z=(145.7, 100.0), null=()):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), thetas=np.ascontiguousarray(thetas, dtype=float), z=np.ascontiguousarray(z, dtype=float))
    for k in null:
        arrs[k] = None
    nbad = np.full(2, -1, np.int64)
    maps = abi.UcfSobolMaps()
    rc = so.ucf_field_sobol(h, plan, npar, addr(arrs["ids"]), nbase, addr(arrs["thetas"]), nz, addr(arrs["z"]), C.byref(maps), None, addr(nbad), None)
    return rc, msg_of(so)


def on_to_the_plan(rc, msg):
    """every argument that can be checked without a plan is in order: a plan cannot exist without a device"""
    import torch
    if torch.cuda.is_available():
        return rc == BAD and "NULL plan" in msg
    return rc == NO_DEVICE and "no CPU fallback" in msg


def test_sobol_refusals_name_the_offender(so):
    h = create(so)
    N = 3
    swapped = np.concatenate([DESIGN[N:2 * N], DESIGN[:N], DESIGN[2 * N:]])
    cases = [
        # what ucf_field_ensemble checks on the shared arguments
        (dict(nz=0), "nz"), (dict(z=(145.7, nan)), "z[1]"), (dict(null=("z",)), "NULL z"), (dict(null=("ids",)), "NULL ids"),
        (dict(null=("thetas",)), "NULL thetas"), (dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"),
        # the size of the design
        (dict(nbase=1), "nbase=1 outside 2..1024"), (dict(nbase=0), "nbase=0"), (dict(nbase=-2), "nbase=-2"), (dict(nbase=1025), "nbase=1025"),
        # a member that is not positive and finite
        (dict(thetas=changed(DESIGN, (4, 1), -2e-4)), "member 4"), (dict(thetas=changed(DESIGN, (11, 0), inf)), "member 11"),
        (dict(thetas=changed(DESIGN, (0, 0), nan)), "member 0"),
        # the structure: a wrong value in an AB block outside column j, one in column j, A and B swapped
        (dict(thetas=changed(DESIGN, (2 * N + 1, 1), 7e-4)), "block 2, row 1, parameter 1"),
        (dict(thetas=changed(DESIGN, (3 * N + 2, 1), 7e-4)), "block 3, row 2, parameter 1"),
        (dict(thetas=changed(DESIGN, (2 * N + 0, 0), np.nextafter(DESIGN[2 * N, 0], 2.0))), "block 2, row 0, parameter 0"),
        (dict(thetas=swapped), "block 2, row 0, parameter 0"),
        # a change in A or in B shows in the first AB block that copies the value
        (dict(thetas=changed(DESIGN, (1, 1), 7e-4)), "block 2, row 1, parameter 1"), (dict(thetas=changed(DESIGN, (N + 2, 0), 1.5)), "block 2, row 2, parameter 0"),
    ]
    for kw, offender in cases:
        rc, msg = sobol_call(so, h, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
        if "block" in offender:
            assert "not a Saltelli design" in msg, msg
    rc, msg = sobol_call(so, None)
    assert rc == BAD and "field" in msg
    # in order: UCF_ERR_NO_DEVICE comes before "NULL plan"
    for kw in (dict(), dict(npar=1, ids=(0,), nbase=2, thetas=R.design(DRAWS[:4, :1]))):
        assert on_to_the_plan(*sobol_call(so, h, **kw)), kw
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_too_many_values_for_one_buffer(so):
    """(npar + 2) nbase nout beyond what one buffer may hold: 2^25 * 3 outputs under 6144 members, not under 3072"""
    h = C.c_void_p()
    nloc = 1 << 20
    xy = np.zeros(nloc)
    assert so.ucf_field_create(1, np.zeros(1), np.zeros(1), np.ones(1), np.zeros(1), nloc, xy, xy, 3, np.array([1.0, 2.0, 3.0]), C.byref(h)) == 0
    nz, npar = 32, 4
    z, ids = np.linspace(1.0, 2.0, nz), np.arange(npar, dtype=np.int32)
    maps = abi.UcfSobolMaps()
    for nbase, want in ((1024, "6144 members x 3 times x 1048576 locations x 32 depths: too many values"), (512, None)):
        thetas = np.ones(((npar + 2) * nbase, npar))                    # a design: every block is the same
        rc = so.ucf_field_sobol(h, None, npar, addr(ids), nbase, addr(thetas), nz, addr(z), C.byref(maps), None, None, None)
        msg = msg_of(so)
        if want:
            assert rc == BAD and want in msg, (rc, msg)
        else:
            assert on_to_the_plan(rc, msg), (rc, msg)
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    a = np.arange(4 * 3 * 5, dtype=float)
    out = abi.UcfSobolMaps()

    def call(npar=2, nbase=3, nout=5, a=a):
        rc = so.ucf_debug_sobol(npar, nbase, nout, addr(a), C.byref(out), None)
        return rc, msg_of(so)

    for kw, offender in ((dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nbase=1), "nbase=1"), (dict(nbase=1025), "nbase=1025"),
                         (dict(nout=0), "nout=0"), (dict(nout=-1), "nout=-1"), (dict(a=None), "NULL a"),
                         (dict(npar=8, nbase=1024, nout=1 << 26), "nout=67108864")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)


# ---- the design

def test_design_is_its_restatement_and_passes_the_structure_check(so):
    rng = np.random.default_rng(3)
    for npar, nbase in ((1, 2), (2, 3), (4, 16), (8, 5), (3, 1024)):
        draws = np.exp(rng.normal(size=(2 * nbase, npar)))
        rc, msg, got = design_call(so, npar=npar, nbase=nbase, draws=draws)
        assert rc == 0, msg
        A, B = draws[:nbase], draws[nbase:]
        want = np.concatenate([A, B] + [np.where(np.arange(npar) == j, B, A) for j in range(npar)])
        assert got.shape == want.shape == ((npar + 2) * nbase, npar) and got.tobytes() == want.tobytes() == R.design(draws).tobytes()
        h = create(so)
        ids = list(range(npar)) if npar < 8 else [0, 1, 2, 3, 4, 5, 6, 0]
        rc, msg = sobol_call(so, h, npar=npar, ids=ids, nbase=nbase, thetas=got)
        assert "Saltelli" not in msg and "member" not in msg, msg
        if len(set(ids)) == npar:
            assert on_to_the_plan(rc, msg), (npar, nbase, rc, msg)
        so.ucf_field_destroy(h)


# ---- the restatement on hand-made columns

PLAIN = ([-2.0, 4.0, -2.0, 3.0], [0.0, 0.0, -3.0, -4.0], [-2.0, 4.0, -2.0, -1.0])
HALF = dict(nrow=2, mean=0.0, var=32.0, S=[-0.3125], ST=[0.390625], seS=[0.5625], seST=[0.375])      # A = (-4, 0), B = (-4, 8), AB = (3, 1)
NONE = dict(S=[nan], ST=[nan], seS=[nan], seST=[nan])
# name, npar, nbase, the rows A, B, AB_0 .., what the statement gives
CASES = [
    ("plain", 1, 4, PLAIN, dict(nrow=4, mean=-0.5, var=8.0, S=[0.4375], ST=[0.25], seS=[0.4375], seST=[0.25])),
    ("plain, S negative", 1, 4, ([-3.0, 1.0, 3.0, -4.0], [-4.0, 2.0, -3.0, 0.0], [-3.0, -4.0, 3.0, -4.0]),
     dict(nrow=4, mean=-1.0, var=8.0, S=[-0.46875], ST=[0.390625], seS=[0.46875], seST=[0.390625])),
    ("plain, two rows", 1, 2, ([-2.0, -1.0], [-4.0, -1.0], [-0.5, -0.5]), dict(nrow=2, mean=-2.0, var=2.0, S=[-0.625], ST=[0.3125], seS=[0.875], seST=[0.25])),
    ("a row incomplete through A", 1, 3, ([-4.0, nan, 0.0], [-4.0, 5.0, 8.0], [3.0, 7.0, 1.0]), HALF),
    ("a row incomplete through B", 1, 3, ([-4.0, 5.0, 0.0], [-4.0, nan, 8.0], [3.0, 7.0, 1.0]), HALF),
    ("a row incomplete through an AB block", 1, 3, ([-4.0, 5.0, 0.0], [-4.0, 5.0, 8.0], [3.0, nan, 1.0]), HALF),
    ("+inf in A", 1, 3, ([-4.0, inf, 0.0], [-4.0, 5.0, 8.0], [3.0, 7.0, 1.0]), HALF),
    ("-inf in an AB block", 1, 3, ([-4.0, 5.0, 0.0], [-4.0, 5.0, 8.0], [3.0, -inf, 1.0]), HALF),
    ("n = 1: S is defined, its error is not", 1, 2, ([1.0, nan], [5.0, 7.0], [2.0, 8.0]),
     dict(nrow=1, mean=3.0, var=8.0, S=[0.25], ST=[0.0625], seS=[nan], seST=[nan])),
    ("n = 0", 1, 2, ([nan, 1.0], [1.0, inf], [1.0, 1.0]), dict(nrow=0, mean=nan, var=nan, **NONE)),
    ("a constant column", 1, 2, ([3.0, 3.0], [3.0, 3.0], [3.0, 3.0]), dict(nrow=2, mean=3.0, var=0.0, **NONE)),
    ("the sentinel everywhere: finite, takes part", 1, 2, ([SENTINEL] * 2, [SENTINEL] * 2, [SENTINEL] * 2), dict(nrow=2, mean=SENTINEL, var=0.0, **NONE)),
    ("a dead parameter beside a live one", 2, 4, PLAIN + (PLAIN[0],),
     dict(nrow=4, mean=-0.5, var=8.0, S=[0.4375, 0.0], ST=[0.25, 0.0], seS=[0.4375, 0.0], seST=[0.25, 0.0])),
    ("a dead parameter alone, zeros of both signs", 1, 2, ([-0.0, 4.0], [0.0, -4.0], [-0.0, 4.0]),
     dict(nrow=2, mean=0.0, var=32.0 / 3.0, S=[0.0], ST=[0.0], seS=[0.0], seST=[0.0])),
]
CLAMP_D = float.fromhex("0x1.68c14p+0")
CLAMPED = ([1.0, -1.0, 0.0], [2.0, -2.0, 0.0], [1.0 - CLAMP_D, -1.0 - CLAMP_D, 0.0 - CLAMP_D])
WITH_SENTINEL = ([SENTINEL, 0.0], [0.0, 0.0], [0.0, 1.0])


def column(rows):
    return np.array(rows, dtype=float).reshape(-1, 1)


def check_case(name, got, want, npar):
    """bit for bit, the sign of a zero and the NaN included"""
    for key in MAP_KEYS:
        g = np.asarray(got[key]).reshape(-1)
        w = np.asarray(want[key], dtype=g.dtype).reshape(-1)
        assert g.shape == w.shape == ((npar,) if key in MAP_KEYS[:4] else (1,)), (name, key)
        assert g.tobytes() == w.tobytes(), (name, key, g.tolist(), w.tolist())


def test_restatement_on_hand_made_columns():
    for name, npar, nbase, rows, want in CASES:
        got = R.sobol(column(rows), npar, nbase)
        check_case(name, got, want, npar)
        assert got["nbad"] == int(want["nrow"] < nbase), name
    # exact +0.0 of a dead parameter: the sign is part of the statement
    dead = R.sobol(column(CASES[-2][3]), 2, 4)
    assert not any(np.signbit(dead[k][1, 0]) for k in MAP_KEYS[:4])
    # several columns side by side are kept apart
    three = [c for c in CASES if c[1] == 1 and c[2] == 3]
    a = np.concatenate([column(c[3]) for c in three], axis=1)
    got = R.sobol(a, 1, 3)
    assert got["nbad"] == len(three) == 5 and got["S"].shape == (1, 5) and got["nrow"].tolist() == [2] * 5
    for key in MAP_KEYS[:4]:
        assert got[key].tobytes() == np.array(HALF[key] * 5).tobytes(), key


def exact(rows, npar):
    """the statement in rational arithmetic, on complete rows, var > 0 and n >= 2; w (the argument of the root) in place of se"""
    F = lambda v: Fraction(float(v))
    fa, fb = [F(v) for v in rows[0]], [F(v) for v in rows[1]]
    n = len(fa)
    mean = (sum(fa) + sum(fb)) / (2 * n)
    var = (sum((x - mean) ** 2 for x in fa) + sum((x - mean) ** 2 for x in fb)) / (2 * n - 1)
    out = dict(mean=mean, var=var, S=[], ST=[], w1=[], wt=[])
    for j in range(npar):
        fj = [F(v) for v in rows[2 + j]]
        p = [(fb[r] - mean) * (fj[r] - fa[r]) for r in range(n)]
        pt = [(fa[r] - fj[r]) ** 2 for r in range(n)]
        m1, mt = sum(p) / n, sum(pt) / n
        out["S"].append(m1 / var)
        out["ST"].append(mt / 2 / var)
        out["w1"].append(sum(x * x for x in p) / n - m1 * m1)
        out["wt"].append(sum(x * x for x in pt) / n - mt * mt)
    return out


def within(got, want, k):
    """|got - want| <= k u |want|, want a Fraction"""
    return abs(Fraction(float(got)) - want) <= k * Fraction(1, 2 ** 53) * abs(want)


def se_within(got, w, n, var, half, k):
    """got = sqrt(w / (n - 1)) / var (times 0.5 where `half`) within k u: compared in the square, where the relative error doubles"""
    want2 = w / (n - 1) / var ** 2 / (4 if half else 1)
    lo, hi = 1 - k * Fraction(1, 2 ** 53), 1 + k * Fraction(1, 2 ** 53)
    return want2 * lo * lo <= Fraction(float(got)) ** 2 <= want2 * hi * hi


def test_restatement_with_the_sentinel_against_exact_arithmetic():
    """the bounds are derived in the module's docstring"""
    got = R.sobol(column(WITH_SENTINEL), 1, 2)
    want = exact(WITH_SENTINEL, 1)
    assert got["nrow"][0] == 2 and got["nbad"] == 0
    assert got["mean"][0] == SENTINEL / 4.0 and Fraction(float(got["mean"][0])) == want["mean"]
    assert within(got["var"][0], want["var"], 7)
    assert within(got["S"][0, 0], want["S"][0], 10) and within(got["ST"][0, 0], want["ST"][0], 10)
    assert se_within(got["seS"][0, 0], want["w1"][0], 2, want["var"], False, 16)
    assert se_within(got["seST"][0, 0], want["wt"][0], 2, want["var"], True, 16)
    # the sentinel dominates everything: S = 1/2 and ST = 1 up to 1 / |X|
    assert abs(got["S"][0, 0] - 0.5) < 1e-5 and abs(got["ST"][0, 0] - 1.0) < 1e-5


def test_a_negative_w_counts_as_zero():
    """the bounds are derived in the module's docstring"""
    d = np.float64(CLAMP_D)
    # the computed wt of the statement, operation by operation: negative, where exact arithmetic gives 0
    pt = d * d
    mt = ((pt + pt) + pt) / 3.0
    raw = ((pt * pt + pt * pt) + pt * pt) / 3.0 - mt * mt
    assert raw < 0.0
    assert all(a - b == d for a, b in zip(CLAMPED[0], CLAMPED[2]))
    got = R.sobol(column(CLAMPED), 1, 3)
    want = exact(CLAMPED, 1)
    assert want["wt"][0] == 0 and want["mean"] == 0 and want["var"] == 2
    assert got["nrow"][0] == 3 and got["mean"][0] == 0.0 and got["var"][0] == 2.0
    assert got["seST"][0, 0] == 0.0 and not np.signbit(got["seST"][0, 0])
    assert got["S"][0, 0] == 0.0 and not np.signbit(got["S"][0, 0])
    assert within(got["ST"][0, 0], want["ST"][0], 4)
    assert se_within(got["seS"][0, 0], want["w1"][0], 3, want["var"], False, 3)


# ---- what the indices mean

def test_ishigami():
    """f = sin x1 + 7 sin^2 x2 + 0.1 x3^4 sin x1 on [-pi, pi]^3, and a fourth input that it does not read.  The six indices that
    are not trivially 0 lie within 4 of their own standard errors of the analytic values (to four decimals): the errors are
    asymptotically normal, and six comparisons at 4 sigma fail by chance about 4e-4 of the time.  The fourth input: exactly +0.0."""
    N = 4096
    x = np.random.default_rng(0).uniform(-np.pi, np.pi, (2 * N, 4))
    d = R.design(x)
    f = np.sin(d[:, 0]) + 7.0 * np.sin(d[:, 1]) ** 2 + 0.1 * d[:, 2] ** 4 * np.sin(d[:, 0])
    got = R.sobol(f[:, None], 4, N)
    assert got["nrow"][0] == N and got["nbad"] == 0
    S, ST = np.array([0.3139, 0.4424, 0.0]), np.array([0.5576, 0.4424, 0.2437])
    zS, zT = (got["S"][:3, 0] - S) / got["seS"][:3, 0], (got["ST"][:3, 0] - ST) / got["seST"][:3, 0]
    print(f"[ishigami N={N}] S={got['S'][:, 0].tolist()} ST={got['ST'][:, 0].tolist()} (index - analytic) / se: S {zS.tolist()} ST {zT.tolist()}")
    assert (np.abs(zS) <= 4.0).all() and (np.abs(zT) <= 4.0).all(), (zS.tolist(), zT.tolist())
    assert (got["seS"][:3, 0] > 0.0).all() and (got["seST"][:3, 0] > 0.0).all()
    for key in MAP_KEYS[:4]:
        assert got[key][3, 0].tobytes() == np.float64(0.0).tobytes(), key
    # the variance is the analytic one, 1/2 + 49/8 + pi^4/50 + pi^8/1800, within 5 % at this N
    assert abs(got["var"][0] / (0.5 + 49.0 / 8.0 + 0.1 * np.pi ** 4 / 5.0 + 0.01 * np.pi ** 8 / 18.0) - 1.0) < 0.05


# ---- the Python front end

class StubLib:
    """the library below WellField.sobol: the call is recorded and reports success; everything else is the library's"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def ucf_field_sobol(self, *args):
        self.calls.append(args)
        return 0


def test_python_front_end_without_a_gpu():
    from unconfined_amd import SobolMaps, WellField, ensemble_draw, sobol_design
    theta, cov = np.array([1.0, 1e-4]), np.array([[0.04, 0.03], [0.03, 0.09]])
    # only the diagonal of cov is used: the draws are those of the diagonal covariance, not those of cov
    d = sobol_design(theta, cov, 3, seed=1)
    diag = np.diag(np.diag(cov))
    assert d.shape == (12, 2) and d.tobytes() == sobol_design(theta, diag, 3, seed=1).tobytes()
    assert d.tobytes() == R.design(ensemble_draw(theta, diag, 6, seed=1)).tobytes()
    assert d.tobytes() != R.design(ensemble_draw(theta, cov, 6, seed=1)).tobytes()
    assert d.tobytes() != sobol_design(theta, cov, 3, seed=2).tobytes()
    with pytest.raises(ValueError):
        sobol_design(theta, np.eye(3), 3)
    for n, offender in ((1, "nbase=1"), (1025, "nbase=1025")):
        with pytest.raises(ucflib.UcfError) as e:
            sobol_design(theta, cov, n)
        assert e.value.status == BAD and offender in e.value.message
    field = WellField(WELLS, LOCATIONS, TIMES)
    plan = types.SimpleNamespace(_h=None)
    z = [145.7, 100.0]
    for bad in (np.ones((12, 3)), np.ones((11, 2))):
        with pytest.raises(ValueError):
            field.sobol(plan, ["Kr", "Ss"], bad, z)
    # what the library refuses reaches the caller with its offender; a design in order goes on to the plan
    with pytest.raises(ucflib.UcfError) as e:
        field.sobol(plan, ["Kr", "Ss"], changed(d, (7, 0), 2.0), z)
    assert e.value.status == BAD and "block 2, row 1, parameter 0" in e.value.message
    with pytest.raises(ucflib.UcfError) as e:
        field.sobol(plan, ["Kr", "Ss"], d, z)
    assert on_to_the_plan(e.value.status, e.value.message)
    # the shapes, below a library that reports success
    real, field._lib = field._lib, StubLib(field._lib)
    try:
        res = field.sobol(plan, ["Kr", "Ss"], d, z, members=True)
        assert isinstance(res, SobolMaps) and res.nbase == 3 and res.stats is None
        for pre in ("", "d"):
            for key in ("S", "ST", "se_S", "se_ST"):
                assert getattr(res, pre + key).shape == (2, 6, 5, 2), pre + key
            for key in ("mean", "var", "nrow"):
                assert getattr(res, pre + key).shape == (6, 5, 2), pre + key
            assert getattr(res, pre + "all").shape == (12, 6, 5, 2) and getattr(res, pre + "nrow").dtype == np.int32
        assert res.nbad.shape == (2,) and res.nbad.dtype == np.int64
        args = field._lib.calls[-1]
        assert args[2] == 2 and args[4] == 3 and args[6] == 2 and args[9] is not None
        small = field.sobol(plan, ["Kr", "Ss"], d, z, derivative=False, with_stats=True)
        assert small.dS is None and small.dall is None and small.all is None and small.S.shape == (2, 6, 5, 2) and set(small.stats) >= {"nan_scrubbed"}
        assert field._lib.calls[-1][9] is None and "SobolMaps(npar=2, nbase=3" in repr(small)
    finally:
        field._lib = real
    field.close()
