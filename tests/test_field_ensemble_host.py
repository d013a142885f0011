"""The host half of ucf_field_ensemble (include/ucf.h): the declarations and the layout of ucf_ensemble_maps, every refusal of
the argument checks with its offender named, and ucf_field_ensemble_draw against a Python restatement of the generator that
the header states (splitmix64, Box-Muller, the Cholesky factor of the fit) and against the moments it is meant to have.  No GPU
is needed: the checks come before the call asks for a device."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE, SINGULAR = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE, abi.UCF_ERR_SINGULAR
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
ENTRIES = ("ucf_field_ensemble", "ucf_field_ensemble_draw", "ucf_debug_ensemble")
MAP_FIELDS = ("mean", "sd", "min", "max", "quant", "all", "nfin")


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def col(a, j):
    return np.ascontiguousarray(np.asarray(a, float)[:, j])


def create(so, wells=WELLS, loc=LOCATIONS, t=TIMES):
    h = C.c_void_p()
    assert so.ucf_field_create(len(wells), col(wells, 0), col(wells, 1), col(wells, 2), col(wells, 3), len(loc), col(loc, 0), col(loc, 1),
                               len(t), np.ascontiguousarray(t, dtype=float), C.byref(h)) == 0
    return h


def addr(a):
    return a.ctypes.data if a is not None else None


def test_header_exports_and_layout(so):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucf.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ucf.h"
    int main(void){
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ucf_ensemble_maps), offsetof(ucf_ensemble_maps,mean), offsetof(ucf_ensemble_maps,sd),
             offsetof(ucf_ensemble_maps,min), offsetof(ucf_ensemble_maps,max), offsetof(ucf_ensemble_maps,quant),
             offsetof(ucf_ensemble_maps,all), offsetof(ucf_ensemble_maps,nfin));
      printf("%d %d\n", UCF_ENSEMBLE_MAX, UCF_ENSEMBLE_MAX_Q);
      return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", os.path.join(d, "t")], check=True)
        vals = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    M = abi.UcfEnsembleMaps
    assert [n for n, _ in M._fields_] == list(MAP_FIELDS)
    assert vals[:8] == [C.sizeof(M)] + [getattr(M, n).offset for n in MAP_FIELDS]
    assert vals[8:] == [abi.UCF_ENSEMBLE_MAX, abi.UCF_ENSEMBLE_MAX_Q] == [1024, 16]


def ensemble(so, h, plan=None, npar=2, ids=(0, 2), nens=3, thetas=None, nz=2, z=(145.7, 100.0), q=(0.05, 0.5, 0.95), nq=None,
             limit=(0.5,), nlim=None, nout=60, want=("mean", "quant"), dwant=("mean",), pexc=True, null=()):
    """one call with small host arrays; `want` / `dwant`: the statistics of s / ds that are passed (dwant None: a NULL struct),
    `null`: arguments passed as NULL"""
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32),
                thetas=np.ascontiguousarray(np.ones((max(nens, 1), max(npar, 1))) if thetas is None else thetas, dtype=float),
                z=np.ascontiguousarray(z, dtype=float), q=np.ascontiguousarray(q, dtype=float), limit=np.ascontiguousarray(limit, dtype=float))
    nq = len(arrs["q"]) if nq is None else nq
    nlim = len(arrs["limit"]) if nlim is None else nlim
    for k in null:
        arrs[k] = None
    keep = []

    def maps(names):
        if names is None:
            return None
        m = abi.UcfEnsembleMaps()
        for n in names:
            a = np.zeros(max(nout * max(nq, nens, 1), 1), np.int32 if n == "nfin" else float)
            keep.append(a)
            setattr(m, n, a.ctypes.data)
        keep.append(m)
        return C.byref(m)

    pe = np.zeros(max(nout * max(nlim, 1), 1)) if pexc else None
    nbad = np.zeros(2, np.int64)
    rc = so.ucf_field_ensemble(h, plan, npar, addr(arrs["ids"]), nens, addr(arrs["thetas"]), nz, addr(arrs["z"]), nq, addr(arrs["q"]), nlim,
                               addr(arrs["limit"]), maps(want), maps(dwant), addr(pe), addr(nbad), None)
    return rc, (so.ucf_last_error() or b"").decode()


def test_refusals_name_the_offender(so):
    import torch
    h = create(so)
    th = np.array([[1.0, 1e-4], [1.1, 1e-4], [1.2, 2e-4]])
    cases = [
        # what ucf_field_drawdown checks
        (dict(nz=0), "nz"), (dict(z=(145.7, np.nan)), "z[1]"), (dict(null=("z",)), "NULL z"),
        # NULL ids, thetas
        (dict(null=("ids",)), "NULL ids"), (dict(null=("thetas",)), "NULL thetas"),
        # npar, nens
        (dict(npar=0, ids=(0,)), "npar=0"), (dict(npar=abi.UCF_FIT_MAX_PAR + 1, ids=range(9)), "npar=9"),
        (dict(nens=0), "nens=0"), (dict(nens=abi.UCF_ENSEMBLE_MAX + 1), "nens=1025"), (dict(nens=-1), "nens=-1"),
        # a theta that is not positive and finite: the member and the parameter
        (dict(thetas=[[1.0, 1e-4], [1.1, 0.0], [1.2, 2e-4]]), "member 1: Ss=0"), (dict(thetas=[[1.0, 1e-4], [1.1, 1e-4], [-1.2, 2e-4]]), "member 2: Kr=-1.2"),
        (dict(thetas=[[np.inf, 1e-4], [1.1, 1e-4], [1.2, 2e-4]]), "member 0: Kr=inf"), (dict(thetas=[[1.0, 1e-4], [1.1, np.nan], [1.2, 2e-4]]), "member 1: Ss=nan"),
        # levels and limits
        (dict(nq=-1), "nq=-1"), (dict(q=np.linspace(0, 1, 17)), "nq=17"), (dict(nlim=-1), "nlim=-1"), (dict(limit=np.linspace(0, 1, 17)), "nlim=17"),
        (dict(null=("q",)), "NULL q"), (dict(null=("limit",)), "NULL limit"),
        (dict(q=(0.05, 1.0000001)), "q[1]"), (dict(q=(-1e-9, 0.5)), "q[0]"), (dict(q=(0.05, 0.5, np.nan)), "q[2]"), (dict(q=(np.inf,)), "q[0]"),
        (dict(limit=(0.5, np.nan)), "limit[1]"), (dict(limit=(-np.inf,)), "limit[0]"),
        (dict(q=()), "quant is asked for with nq=0"), (dict(q=(), want=("mean",), dwant=("quant",)), "quant is asked for with nq=0"),
        (dict(limit=()), "pexc is asked for with nlim=0"),
    ]
    for kw, offender in cases:
        a = dict(thetas=th)
        a.update(kw)
        rc, msg = ensemble(so, h, **a)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg = ensemble(so, None, thetas=th)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device
    for kw in (dict(), dict(q=(), want=("mean", "sd", "min", "max", "nfin", "all"), dwant=None), dict(limit=(), pexc=False, want=(), dwant=()),
               dict(q=(0.0, 1.0), limit=(0.0,) * 16, nens=abi.UCF_ENSEMBLE_MAX, thetas=np.ones((abi.UCF_ENSEMBLE_MAX, 2)), want=("quant",), nout=1)):
        a = dict(thetas=th)
        a.update(kw)
        rc, msg = ensemble(so, h, **a)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_refuses_more_values_than_a_buffer_holds(so):
    """70000 times x 40000 locations x 12 depths is a map that ucf_field_drawdown accepts (3.4e10 outputs, below 2^31-1 blocks of
    256); 16 members of it fit into one buffer, 17 do not -- the forecast's rule"""
    loc = np.stack([np.linspace(10.0, 5000.0, 40000), np.zeros(40000)], axis=1)
    h = create(so, np.array([[0.0, 0.0, 1.0, 0.0]]), loc, np.linspace(1.0, 1000.0, 70000))
    z = np.linspace(1.0, 12.0, 12)
    assert 16 * 70000 * 40000 * 12 <= (2 ** 31 - 1) * 256 < 17 * 70000 * 40000 * 12
    rc, msg = ensemble(so, h, nens=17, nz=12, z=z, nout=1, want=(), dwant=None, pexc=False, limit=())
    assert rc == BAD and "17 members" in msg and "too many" in msg, (rc, msg)
    rc, msg = ensemble(so, h, nens=16, nz=12, z=z, nout=1, want=(), dwant=None, pexc=False, limit=())
    assert rc in (NO_DEVICE, BAD) and "too many" not in msg, (rc, msg)
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_debug_entry_checks_then_asks_for_a_device(so):
    import torch
    a = np.arange(12.0)
    q, lim = np.array([0.5]), np.array([3.0])
    m = abi.UcfEnsembleMaps()
    quant = np.zeros(4)
    m.quant = quant.ctypes.data
    pexc, nbad = np.zeros(4), np.zeros(1, np.int64)
    call = lambda nens=3, nout=4, a=a, nq=1, q=q, nlim=1, lim=lim, pexc=pexc: (
        so.ucf_debug_ensemble(nens, nout, addr(a), nq, addr(q), nlim, addr(lim), C.byref(m), addr(pexc), addr(nbad)), (so.ucf_last_error() or b"").decode())
    for kw, offender in ((dict(nens=0), "nens=0"), (dict(nens=1025), "nens=1025"), (dict(nq=0), "quant is asked for with nq=0"),
                         (dict(nlim=0), "pexc is asked for with nlim=0"), (dict(q=np.array([1.5])), "q[0]"), (dict(lim=np.array([np.nan])), "limit[0]"),
                         (dict(a=None), "NULL a"), (dict(nout=0), "nout=0")):
        rc, msg = call(**kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc == NO_DEVICE and "no CPU fallback" in msg, (rc, msg)


# ---- ucf_field_ensemble_draw

MASK = (1 << 64) - 1
THETA = np.array([2.3e-4, 0.35, 1.7e-5, 0.21])
_L = np.tril(0.05 + 0.3 * np.cos(np.arange(16.0).reshape(4, 4)))
COV = _L @ _L.T
COV = 0.5 * (COV + COV.T)


def draw(so, theta, cov, nens, seed, null=()):
    theta, cov = np.ascontiguousarray(theta, dtype=float), np.ascontiguousarray(cov, dtype=float)
    out = np.zeros((max(nens, 1), len(theta)))
    rc = so.ucf_field_ensemble_draw(len(theta), None if "theta" in null else addr(theta), None if "cov" in null else addr(cov), nens, seed,
                                    None if "thetas" in null else addr(out))
    return rc, out, (so.ucf_last_error() or b"").decode()


def restated(theta, cov, nens, seed):
    """the generator as include/ucf.h states it, one operation at a time"""
    n = len(theta)
    L = [[float(cov[i][k]) for k in range(n)] for i in range(n)]
    for j in range(n):
        d = L[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        assert d > 0.0
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, n):
            v = L[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    state = [seed & MASK]

    def uniform():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & MASK
        x = state[0]
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
        x = x ^ (x >> 31)
        return (float(x >> 11) + 0.5) * 2.0 ** -53

    out = np.zeros((nens, n))
    for m in range(nens):
        zeta = [0.0] * (n + 1)
        for i in range(0, n, 2):
            u1 = uniform()
            u2 = uniform()
            rad, ang = math.sqrt(-2.0 * math.log(u1)), 6.283185307179586 * u2
            zeta[i], zeta[i + 1] = rad * math.cos(ang), rad * math.sin(ang)
        for j in range(n):
            acc = 0.0
            for k in range(j + 1):
                acc = acc + L[j][k] * zeta[k]
            out[m, j] = theta[j] * math.exp(acc)
    return out


def test_draw_is_deterministic_positive_and_seeded(so):
    rc, a, msg = draw(so, THETA, COV, 200, 7)
    assert rc == 0, msg
    rc, b, _ = draw(so, THETA, COV, 200, 7)
    rc, c, _ = draw(so, THETA, COV, 200, 8)
    assert a.tobytes() == b.tobytes() and (a != c).all()
    assert np.isfinite(a).all() and (a > 0.0).all()
    # the stream is one for the whole call: the first members of a longer draw are the shorter draw
    rc, d, _ = draw(so, THETA, COV, 50, 7)
    assert d.tobytes() == a[:50].tobytes()
    # the 64 bits of the seed all count
    rc, e, _ = draw(so, THETA, COV, 4, 7 + (1 << 63))
    assert rc == 0 and (e != a[:4]).all()


@pytest.mark.parametrize("npar", [1, 2, 3, 4])
def test_draw_is_the_stated_generator(so, npar):
    """odd npar: the second deviate of the last pair is discarded, the stream still advances by two draws"""
    theta, cov = THETA[:npar], COV[:npar, :npar].copy()
    for seed in (0, 12345, MASK):
        rc, got, msg = draw(so, theta, cov, 33, seed)
        assert rc == 0, msg
        want = restated(theta, cov, 33, seed)
        rel = np.abs(got - want) / want
        print(f"[ensemble draw] npar={npar} seed={seed}: {int((got != want).sum())} of {got.size} values differ from the restatement, "
              f"worst relative difference {float(rel.max()):.2e}")
        assert (rel <= 1e-14).all(), (npar, seed, float(rel.max()))


def test_draw_has_the_moments_of_the_covariance(so):
    N = 4096
    rc, th, msg = draw(so, THETA, COV, N, 20261019)
    assert rc == 0, msg
    x = np.log(th / THETA)
    mean = x.mean(axis=0)
    c = np.cov(x, rowvar=False)
    for j in range(4):
        assert abs(mean[j]) <= 5.0 * np.sqrt(COV[j, j] / N), (j, mean[j])
        for k in range(4):
            se = np.sqrt((COV[j, j] * COV[k, k] + COV[j, k] ** 2) / N)
            print(f"[ensemble draw] cov[{j}][{k}]: sample {c[j, k]:+.5f} stated {COV[j, k]:+.5f}, {abs(c[j, k] - COV[j, k]) / se:.2f} standard errors")
            assert abs(c[j, k] - COV[j, k]) <= 5.0 * se, (j, k, c[j, k], COV[j, k])


def test_draw_refusals(so):
    cases = [
        (dict(theta=[1.0] * 9, cov=np.eye(9)), BAD, "npar=9"), (dict(theta=[], cov=np.zeros((0, 0))), BAD, "npar=0"),
        (dict(null=("theta",)), BAD, "NULL theta"), (dict(null=("cov",)), BAD, "NULL cov"), (dict(null=("thetas",)), BAD, "NULL thetas"),
        (dict(nens=0), BAD, "nens=0"), (dict(nens=-3), BAD, "nens=-3"),
        (dict(theta=[1.0, 0.0]), BAD, "theta[1]"), (dict(theta=[-1.0, 1.0]), BAD, "theta[0]"), (dict(theta=[1.0, np.inf]), BAD, "theta[1]"),
        (dict(cov=[[0.01, np.nan], [np.nan, 0.03]]), BAD, "cov[0][1]"), (dict(cov=[[0.01, 0.002], [0.0021, 0.03]]), BAD, "symmetric"),
        (dict(cov=[[0.01, 0.002], [0.002, -0.03]]), BAD, "cov[1][1]"),
        # not positive definite: a correlation beyond 1, a zero variance
        (dict(cov=[[0.01, 0.02], [0.02, 0.01]]), SINGULAR, "positive definite"), (dict(cov=[[0.0, 0.0], [0.0, 0.01]]), SINGULAR, "positive definite"),
    ]
    for kw, status, offender in cases:
        a = dict(theta=[1.0, 2.0], cov=[[0.01, 0.002], [0.002, 0.03]], nens=4, seed=1)
        a.update(kw)
        rc, _, msg = draw(so, **a)
        assert rc == status and offender in msg, (kw, rc, msg)


def test_python_front_end_without_a_gpu():
    from unconfined_amd import ensemble_draw
    a = ensemble_draw(THETA, COV, 16, seed=3)
    assert a.shape == (16, 4) and (a > 0).all()
    assert a.tobytes() == ensemble_draw(THETA, COV, 16, seed=3).tobytes() != ensemble_draw(THETA, COV, 16, seed=4).tobytes()
    with pytest.raises(ucflib.UcfError) as e:
        ensemble_draw([1.0, 2.0], [[0.01, 0.02], [0.02, 0.01]], 4, seed=1)
    assert e.value.status == SINGULAR
    with pytest.raises(ValueError):
        ensemble_draw([1.0, 2.0], np.eye(3), 4)
