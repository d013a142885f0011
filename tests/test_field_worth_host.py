"""The host half of ucf_field_worth (include/ucf.h): ucf_worth_condition against the numpy restatement of the header
(tests/field_worth_restate.py) and against numpy's linear algebra, every refusal of the three entries with its offender named,
and the declarations.  No GPU is needed: the checks come before a call asks for a device.

Bounds.  The conditioning solves with B = I + sum (w F'j)(w F'j)' through its LDL' factors: the textbook forward bound of a
Cholesky solve is c n u kappa_2(B) relative, here with c = 8 (a prototype of this arithmetic used 1.3 of the u kappa); the
inputs keep kappa_2(B) <= 1e6 and kappa_2(C) small, so that numpy's own inverse of C is exact to a few u and the bound is the
library's alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import field_worth_restate as R
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE, SINGULAR = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE, abi.UCF_ERR_SINGULAR
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
ENTRIES = ("ucf_field_worth", "ucf_worth_condition", "ucf_debug_field_worth")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def addr(a):
    return a.ctypes.data if a is not None else None


def msg_of(so):
    return (so.ucf_last_error() or b"").decode()


def problem(npar, seed, nrow=7, general=False):
    """a well-conditioned covariance with its factor, nrow readings and their weights"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((npar, npar))
    cov = 0.05 * (np.eye(npar) + 0.25 * (M @ M.T) / npar)
    cov = 0.5 * (cov + cov.T)
    F = R.cholesky(cov)
    if general:                                      # any square factor: F Q with Q orthogonal, as it is after a pick
        Q, _ = np.linalg.qr(rng.standard_normal((npar, npar)))
        F = F @ Q
        cov = F @ F.T
    J = rng.standard_normal((nrow, npar)) * rng.uniform(0.2, 3.0, npar)
    w = rng.uniform(5.0, 40.0, nrow)
    return cov, np.ascontiguousarray(F), np.ascontiguousarray(J), w


def condition(so, F, J, w, null=(), npar=None, nrow=None, want_cov=True):
    F = None if F is None else np.ascontiguousarray(F, dtype=float)
    J = None if J is None else np.ascontiguousarray(J, dtype=float)
    w = None if w is None else np.ascontiguousarray(w, dtype=float)
    n = len(F) if npar is None else npar
    m = max(n, 1)
    F_out, cov_out = np.zeros((m, m)), np.zeros((m, m))
    rc = so.ucf_worth_condition(n, None if "F" in null else addr(F), (len(w) if w is not None else 0) if nrow is None else nrow,
                                None if "J" in null else addr(J), None if "w" in null else addr(w),
                                None if "F_out" in null else addr(F_out), addr(cov_out) if want_cov else None)
    return rc, F_out, cov_out, msg_of(so)


def test_header_and_exports(so):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucf.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    vals = dict(re.findall(r"#define\s+(UCF_WORTH_MAX_\w+)\s+(\d+)", code))
    assert vals == {"UCF_WORTH_MAX_TGT": "16", "UCF_WORTH_MAX_PICK": "16"}
    assert (abi.UCF_WORTH_MAX_TGT, abi.UCF_WORTH_MAX_PICK) == (16, 16)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("npar", range(1, 9))
def test_condition_is_the_stated_arithmetic(so, npar, general):
    cov, F, J, w = problem(npar, 100 + npar, general=general)
    rc, F_out, cov_out, msg = condition(so, F, J, w)
    assert rc == 0, msg
    want_F, want_cov = R.condition(F, J, w)
    for name, got, want in (("F_out", F_out, want_F), ("cov_out", cov_out, want_cov)):
        rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        print(f"[worth condition] npar={npar} general={general} {name}: {int((got != want).sum())} of {got.size} values differ from the "
              f"restatement, worst relative difference {float(rel.max()):.2e}")
        assert (rel <= 1e-14).all(), (npar, name, float(rel.max()))
    # cov_out is F_out F_out' in the stated order: symmetric bit for bit
    assert cov_out.tobytes() == cov_out.T.copy().tobytes()


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("npar", range(1, 9))
def test_condition_against_numpy(so, npar, general):
    cov, F, J, w = problem(npar, 200 + npar, general=general)
    B = R.dense_B(F, J, w)
    kB, kC = np.linalg.cond(B), np.linalg.cond(cov)
    assert kB <= 1e6 and kC <= 100.0, (kB, kC)
    rc, F_out, cov_out, msg = condition(so, F, J, w)
    assert rc == 0, msg
    want = np.linalg.inv(np.linalg.inv(cov) + J.T @ np.diag(w * w) @ J)
    bound = 8 * npar * U * kB * np.abs(cov).max()
    err = np.abs(F_out @ F_out.T - want).max()
    print(f"[worth condition] npar={npar} general={general}: kappa(B)={kB:.3g}, |F_out F_out' - inv(inv(C) + J'W^2J)| = {err:.3e}, "
          f"{err / bound:.3f} of the bound {bound:.3e}")
    assert err <= bound
    assert np.abs(cov_out - want).max() <= bound
    # data never add variance
    assert (np.diag(cov_out) <= np.diag(cov) * (1 + 8 * npar * U * kB)).all()


@pytest.mark.parametrize("npar", [1, 4, 8])
def test_no_rows_return_the_factor(so, npar):
    cov, F, _, _ = problem(npar, 300 + npar, general=True)
    for J, w, null in ((np.zeros((0, npar)), np.zeros(0), ()), (None, None, ("J", "w"))):
        rc, F_out, cov_out, msg = condition(so, F, J, w, null=null, nrow=0)
        assert rc == 0, msg
        assert F_out.tobytes() == F.tobytes()
        assert cov_out.tobytes() == R.condition(F, np.zeros((0, npar)), np.zeros(0))[1].tobytes()
    # without cov_out
    rc, F_out, _, msg = condition(so, F, None, None, null=("J", "w"), nrow=0, want_cov=False)
    assert rc == 0 and F_out.tobytes() == F.tobytes(), msg


@pytest.mark.parametrize("npar", range(1, 9))
def test_restated_post_against_numpy(npar):
    """the kernel's arithmetic, restated, against a' solve(B, a): three candidates (no datum, one datum, all), two targets"""
    cov, F, J, w = problem(npar, 400 + npar, nrow=5, general=True)
    rng = np.random.default_rng(npar)
    nt, ncand, dlog = 5, 3, 1e-3
    two_dlog = np.float64(2.0) * np.float64(dlog)
    a = rng.standard_normal((1 + 2 * npar, nt, ncand)) * 1e-3 + 1.0
    a[1:, :, 0] = np.nan
    a[1, 1:, 1] = np.inf
    Jt = rng.standard_normal((2, npar))
    A, prior = R.targets(F, Jt, [True, True])
    ws = 25.0
    post, crit, nused = R.kernel(a, None, two_dlog, F, ws, 0.0, None, A, [1.0, 2.0])
    assert nused.tolist() == [0, 1, nt]
    assert post[:, 0].tobytes() == prior.tobytes()
    for c in range(ncand):
        Jc, wc = R.rows_of(a, None, two_dlog, ws, 0.0, None, c)
        assert len(wc) == nused[c]
        B = R.dense_B(F, Jc, wc)
        kB = np.linalg.cond(B)
        assert kB <= 1e6
        for t in range(2):
            want = A[t] @ np.linalg.solve(B, A[t])
            rel = abs(post[t, c] - want) / want
            print(f"[worth post] npar={npar} candidate {c} target {t}: kappa(B)={kB:.3g}, relative difference {rel:.2e}, "
                  f"{rel / (8 * npar * U * kB):.3f} of the bound")
            assert rel <= 8 * npar * U * kB
            assert post[t, c] <= prior[t] * (1 + 8 * npar * U * kB)
    assert crit.tobytes() == ((0.0 + 1.0 * post[0]) + 2.0 * post[1]).tobytes()


def test_condition_refusals(so):
    _, F, J, w = problem(3, 1)
    nanF, nanJ, infw, negw = F.copy(), J.copy(), w.copy(), w.copy()
    nanF[1, 2], nanJ[2, 1], infw[3], negw[4] = np.nan, np.inf, np.inf, -1.0
    cases = [
        (dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nrow=-1), "nrow=-1"),
        (dict(null=("F",)), "NULL F"), (dict(null=("F_out",)), "NULL F_out"), (dict(null=("J",)), "NULL J"), (dict(null=("w",)), "NULL w"),
        (dict(F=nanF), "F[5]"), (dict(J=nanJ), "J[7]"), (dict(w=infw), "w[3]"), (dict(w=negw), "w[4]"),
    ]
    for kw, offender in cases:
        a = dict(F=F, J=J, w=w)
        a.update(kw)
        rc, _, _, msg = condition(so, **a)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    # overflow is the only way to a pivot that is not positive and finite
    rc, _, _, msg = condition(so, np.eye(2), np.array([[1e200, 0.0]]), np.array([1e10]))
    assert rc == SINGULAR and "d[0]" in msg, (rc, msg)


def test_python_front_end_without_a_gpu():
    from unconfined_amd import worth_condition
    cov, F, J, w = problem(4, 7)
    F_out, cov_out = worth_condition(F, J, w)
    want_F, want_cov = R.condition(F, J, w)
    assert np.allclose(F_out, want_F, rtol=1e-14, atol=0) and np.allclose(cov_out, want_cov, rtol=1e-14, atol=0)
    same, c0 = worth_condition(F, [], [])
    assert same.tobytes() == F.tobytes() and np.allclose(c0, cov, rtol=1e-13)
    with pytest.raises(ValueError):
        worth_condition(F, J, w[:-1])
    with pytest.raises(ucflib.UcfError) as e:
        worth_condition(F, J, -w)
    assert e.value.status == BAD


# ---- ucf_field_worth: every refusal comes without a device

def col(a, j):
    return np.ascontiguousarray(np.asarray(a, float)[:, j])


def create(so):
    h = C.c_void_p()
    assert so.ucf_field_create(len(WELLS), col(WELLS, 0), col(WELLS, 1), col(WELLS, 2), col(WELLS, 3), len(LOCATIONS), col(LOCATIONS, 0),
                               col(LOCATIONS, 1), len(TIMES), TIMES, C.byref(h)) == 0
    return h


COV2 = np.array([[0.01, 0.002], [0.002, 0.03]])


def worth(so, h, plan=None, npar=2, ids=(0, 2), theta=(1.0, 1e-4), dlog=1e-3, cov=COV2, nz=2, z=(145.7, 100.0), sigma_s=0.01, sigma_d=0.05,
          tsel=None, ntgt=None, tgt=((0, 5, 4, 1), (1, 3, 0, 0)), tw=None, npick=2, cmask=None, null=()):
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), theta=np.ascontiguousarray(theta, dtype=float), cov=np.ascontiguousarray(cov, dtype=float),
                z=np.ascontiguousarray(z, dtype=float), tgt=np.ascontiguousarray(tgt, dtype=np.int32),
                tsel=None if tsel is None else np.ascontiguousarray(tsel, dtype=np.int32), tw=None if tw is None else np.ascontiguousarray(tw, dtype=float),
                cmask=None if cmask is None else np.ascontiguousarray(cmask, dtype=np.int32))
    ntgt = len(arrs["tgt"]) if ntgt is None else ntgt
    for k in null:
        arrs[k] = None
    rc = so.ucf_field_worth(h, plan, npar, addr(arrs["ids"]), addr(arrs["theta"]), dlog, addr(arrs["cov"]), nz, addr(arrs["z"]), sigma_s, sigma_d,
                            addr(arrs["tsel"]), ntgt, addr(arrs["tgt"]), addr(arrs["tw"]), npick, addr(arrs["cmask"]), None, None, None, None, None,
                            None, None)
    return rc, msg_of(so)


def test_worth_refusals_name_the_offender(so):
    import torch
    h = create(so)
    cases = [
        # what ucf_field_forecast checks on the shared arguments
        (dict(nz=0), BAD, "nz"), (dict(z=(145.7, np.nan)), BAD, "z[1]"), (dict(null=("z",)), BAD, "NULL z"), (dict(null=("ids",)), BAD, "NULL ids"),
        (dict(null=("theta",)), BAD, "NULL theta"), (dict(npar=0), BAD, "npar=0"), (dict(npar=9), BAD, "npar=9"), (dict(dlog=0.0), BAD, "dlog=0"),
        (dict(dlog=np.inf), BAD, "dlog=inf"),
        # the covariance: required, as the forecast checks it, positive definite
        (dict(null=("cov",)), BAD, "NULL cov"), (dict(cov=[[0.01, np.nan], [np.nan, 0.03]]), BAD, "cov[0][1]"),
        (dict(cov=[[0.01, 0.002], [0.0021, 0.03]]), BAD, "symmetric"), (dict(cov=[[0.01, 0.002], [0.002, -0.03]]), BAD, "cov[1][1]"),
        (dict(cov=[[0.01, 0.02], [0.02, 0.01]]), SINGULAR, "positive definite"), (dict(cov=[[0.25, 0.25], [0.25, 0.25]]), SINGULAR, "positive definite"),
        (dict(cov=[[0.0, 0.0], [0.0, 0.01]]), SINGULAR, "positive definite"),      # semidefinite, in numbers that the factorisation holds exactly
        # the data model
        (dict(sigma_s=0.0), BAD, "sigma_s=0"), (dict(sigma_s=-1.0), BAD, "sigma_s=-1"), (dict(sigma_s=np.inf), BAD, "sigma_s=inf"),
        (dict(sigma_s=np.nan), BAD, "sigma_s=nan"), (dict(sigma_d=-0.5), BAD, "sigma_d=-0.5"), (dict(sigma_d=np.inf), BAD, "sigma_d=inf"),
        (dict(sigma_d=np.nan), BAD, "sigma_d=nan"), (dict(tsel=[0] * 6), BAD, "tsel selects none"),
        # targets
        (dict(ntgt=0), BAD, "ntgt=0"), (dict(tgt=[(0, 0, 0, 0)] * 17), BAD, "ntgt=17"), (dict(null=("tgt",)), BAD, "NULL tgt"),
        (dict(tgt=[(2, 0, 0, 0)]), BAD, "tgt[0]"), (dict(tgt=[(0, 0, 0, 0), (0, 6, 0, 0)]), BAD, "tgt[1]"), (dict(tgt=[(0, 0, 5, 0)]), BAD, "tgt[0]"),
        (dict(tgt=[(0, 0, 0, 2)]), BAD, "tgt[0]"), (dict(tgt=[(0, -1, 0, 0)]), BAD, "tgt[0]"), (dict(tgt=[(-1, 0, 0, 0)]), BAD, "tgt[0]"),
        (dict(tw=[1.0, -1.0]), BAD, "tw[1]"), (dict(tw=[np.nan, 1.0]), BAD, "tw[0]"), (dict(tw=[np.inf, 1.0]), BAD, "tw[0]"),
        # picks
        (dict(npick=0), BAD, "npick=0"), (dict(npick=17), BAD, "npick=17"),
    ]
    for kw, status, offender in cases:
        rc, msg = worth(so, h, **kw)
        assert rc == status and offender in msg, (kw, rc, msg)
    rc, msg = worth(so, None)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device
    for kw in (dict(), dict(sigma_d=0.0, tsel=[0, 0, 1, 0, 0, 0], tw=[0.0, 2.0], npick=16, cmask=[1] * 10), dict(tgt=[(1, 0, 0, 0)] * 16, npick=1)):
        rc, msg = worth(so, h, **kw)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    npar, nt, ncand, ntgt = 2, 3, 4, 2
    a = np.arange((1 + 2 * npar) * nt * ncand, dtype=float)
    F, A = np.array([[0.1, 0.0], [0.02, 0.17]]), np.array([[0.3, 0.1], [0.0, 0.2]])
    nanF = F.copy()
    nanF[1, 0] = np.nan
    post, crit, nused = np.zeros((ntgt, ncand)), np.zeros(ncand), np.zeros(ncand, np.int32)

    def call(npar=npar, nt=nt, ncand=ncand, a_s=a, a_d=a, two_dlog=2e-3, F=F, ws=100.0, wd=20.0, tsel=None, ntgt=ntgt, A=A, tw=None):
        tsel = None if tsel is None else np.ascontiguousarray(tsel, dtype=np.int32)
        tw = None if tw is None else np.ascontiguousarray(tw, dtype=float)
        rc = so.ucf_debug_field_worth(npar, nt, ncand, addr(a_s), addr(a_d), two_dlog, addr(F), ws, wd, addr(tsel), ntgt, addr(A), addr(tw),
                                      addr(post), addr(crit), addr(nused))
        return rc, msg_of(so)

    for kw, offender in ((dict(npar=0), "npar=0"), (dict(npar=9), "npar=9"), (dict(nt=0), "nt=0"), (dict(ncand=0), "ncand=0"),
                         (dict(nt=1 << 20, ncand=1 << 20), "more than 2^31-1"), (dict(a_s=None), "NULL a_s"), (dict(F=None), "NULL F"),
                         (dict(A=None), "NULL A"), (dict(a_d=None), "NULL a_d"), (dict(two_dlog=0.0), "two_dlog=0"), (dict(two_dlog=np.nan), "two_dlog=nan"),
                         (dict(F=nanF), "F[2]"), (dict(ws=0.0), "ws=0"), (dict(ws=np.inf), "ws=inf"), (dict(wd=-1.0), "wd=-1"), (dict(wd=np.nan), "wd=nan"),
                         (dict(ntgt=0), "ntgt=0"), (dict(ntgt=17), "ntgt=17"), (dict(tw=[1.0, -2.0]), "tw[1]"), (dict(tw=[np.inf, 1.0]), "tw[0]"),
                         (dict(tsel=[0, 0, 0]), "tsel selects none")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        for kw in (dict(), dict(a_d=None, wd=0.0), dict(tsel=[0, 1, 0], tw=[0.0, 1.0])):
            rc, msg = call(**kw)
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, rc, msg)
