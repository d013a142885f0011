"""The host half of the fitting interface (ucf_fit_* of include/ucf.h), no GPU needed: header / exports / struct layout,
ucf_fit_perturb, ucf_fit_solve_step against numpy, and the validation of ucf_fit_create, which comes before the device
check."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from golden_util import load_deck
from unconfined_amd import abi
from unconfined_amd import lib as ucflib
from unconfined_amd.abi import UcfParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_SYMBOLS = ["ucf_fit_perturb", "ucf_fit_solve_step", "ucf_fit_default_options", "ucf_fit_create", "ucf_fit_destroy",
               "ucf_fit_evaluate", "ucf_fit_lm", "ucf_fit_alloc_count"]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(ucflib.LIB_PATH):
        ucflib.build()
    return ucflib.load()


def test_header_exports_and_options_layout(so):
    text = open(os.path.join(ROOT, "include", "ucf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in FIT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    assert "UCF_FIT_MAX_PAR 8" in code
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ucf.h"
    int main(void){
      printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ucf_fit_options), offsetof(ucf_fit_options,max_iter), offsetof(ucf_fit_options,dlog),
             offsetof(ucf_fit_options,lambda0), offsetof(ucf_fit_options,lambda_up), offsetof(ucf_fit_options,lambda_down),
             offsetof(ucf_fit_options,tol_step), offsetof(ucf_fit_options,tol_phi));
      printf("%d %d %d %d %d %d %d %d %d\n", UCF_PAR_KR, UCF_PAR_KAPPA, UCF_PAR_SS, UCF_PAR_SY, UCF_PAR_AC, UCF_PAR_AK, UCF_PAR_USL,
             UCF_PAR_MOENCH_ALPHA0, UCF_FIT_MAX_PAR);
      printf("%d %d %d %d %d\n", UCF_FIT_CONVERGED, UCF_FIT_MAX_ITER, UCF_FIT_SINGULAR, UCF_FIT_NONFINITE_START, UCF_ERR_SINGULAR);
      return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), p, "-o", os.path.join(d, "t")], check=True)
        vals = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    O = abi.UcfFitOptions
    assert vals[:8] == [C.sizeof(O), O.max_iter.offset, O.dlog.offset, O.lambda0.offset, O.lambda_up.offset, O.lambda_down.offset,
                        O.tol_step.offset, O.tol_phi.offset]
    assert vals[8:17] == [abi.PAR_KR, abi.PAR_KAPPA, abi.PAR_SS, abi.PAR_SY, abi.PAR_AC, abi.PAR_AK, abi.PAR_USL, abi.PAR_MOENCH_ALPHA0,
                          abi.UCF_FIT_MAX_PAR]
    assert vals[17:] == [abi.FIT_CONVERGED, abi.FIT_MAX_ITER, abi.FIT_SINGULAR, abi.FIT_NONFINITE_START, abi.UCF_ERR_SINGULAR]
    o = O()
    assert so.ucf_fit_default_options(C.byref(o)) == 0
    assert o.max_iter >= 1 and o.dlog == 1e-3 and o.lambda_up > 1 and 0 < o.lambda_down < 1


# every id and a deck of every model that reads it
READERS = {
    "Kr": ["c1_theis", "hantush_lay1", "hstorage_partpen_lay1", "c3_moench", "malama_fullpen", "c4_malama_partpen", "mishra_malama", "mishra_fd30"],
    "Ss": ["c1_theis", "hantush_lay1", "hstorage_partpen_lay1", "c3_moench", "malama_fullpen", "c4_malama_partpen", "mishra_malama", "mishra_fd30"],
    "kappa": ["hantush_lay1", "hstorage_partpen_lay1", "c3_moench", "malama_fullpen", "c4_malama_partpen", "mishra_malama", "mishra_fd30"],
    "Sy": ["c3_moench", "malama_fullpen", "c4_malama_partpen", "mishra_malama", "mishra_fd30"],
    "ak": ["mishra_malama", "mishra_fd30"],
    "ac": ["mishra_fd30"],
    "usL": ["mishra_fd30"],
    "MoenchAlpha[0]": ["c3_moench"],
}
FIELD = {"Kr": "Kr", "kappa": "kappa", "Ss": "Ss", "Sy": "Sy", "ac": "ac", "ak": "ak", "usL": "usL"}


def _bytes(P):
    return bytes(C.string_at(C.addressof(P), C.sizeof(P)))


def test_perturb_changes_exactly_the_named_fields(so):
    from unconfined_amd import fit as ufit
    models = set()
    for name, decks in READERS.items():
        for deck in decks:
            _, _, P = load_deck(deck)
            models.add((P.model, P.MNtype if P.model == 6 else 0))
            out = ufit.perturb(P, [name], [1.2345e-3])
            want = UcfParams.from_buffer_copy(_bytes(P))
            if name in FIELD:
                setattr(want, FIELD[name], 1.2345e-3)
            else:
                want.MoenchAlpha[0] = 1.2345e-3
            assert _bytes(out) == _bytes(want), (name, deck)
            assert _bytes(out) != _bytes(P)
    assert {m for m, _ in models} == {0, 1, 2, 3, 4, 5, 6}
    # several at once, in the order given
    _, _, P = load_deck("neuman74_partpen")
    out = ufit.perturb(P, ["Sy", "Kr", "kappa", "Ss"], [0.1, 0.2, 0.3, 0.4])
    want = UcfParams.from_buffer_copy(_bytes(P))
    want.Sy, want.Kr, want.kappa, want.Ss = 0.1, 0.2, 0.3, 0.4
    assert _bytes(out) == _bytes(want)
    # and what it refuses
    th = np.ones(9)
    bad = C.byref(UcfParams())
    for ids, word in (([], b"npar"), (list(range(7)) + [0, 1], b"npar"), ([abi.PAR_KR, abi.PAR_KR], b"duplicate"), ([99], b"no parameter id")):
        a = np.ascontiguousarray(ids if ids else [0], np.int32)
        assert so.ucf_fit_perturb(C.byref(P), len(ids), a, th, bad) == abi.UCF_ERR_BAD_ARGUMENT
        assert word in so.ucf_last_error(), (ids, so.ucf_last_error())


@pytest.mark.parametrize("npar", range(1, 9))
@pytest.mark.parametrize("lam", [0.0, 1e-3, 10.0])
def test_solve_step_against_numpy(so, npar, lam):
    """(A + lam diag A) step = g: a Cholesky solve is backward stable; with the classical constants the forward error is
    below 8 n u cond(A + lam diag A) for the matrices here (Higham, Accuracy and Stability, thm 10.4 / 10.6: backward error
    <= (3n+1) u |R'||R| per triangular stage chain, i.e. a few n u in norm) -- derived, not tuned"""
    from unconfined_amd import fit as ufit
    rng = np.random.default_rng(1000 * npar + int(lam * 1000))
    for trial in range(20):
        B = rng.standard_normal((npar + 3, npar)) * 10.0 ** rng.uniform(-2, 2, npar)
        A = B.T @ B
        A = 0.5 * (A + A.T)
        g = rng.standard_normal(npar) * np.sqrt(np.diag(A))
        M = A + lam * np.diag(np.diag(A))
        step = ufit.solve_step(A, g, lam)
        Ml, gl = M.astype(np.longdouble), g.astype(np.longdouble)
        # reference in extended precision: numpy's solve, refined once
        ref = np.linalg.solve(M, g).astype(np.longdouble)
        ref = ref + np.linalg.solve(M, np.asarray(gl - Ml @ ref, np.float64))
        err = float(np.linalg.norm(np.asarray(step - ref, np.float64)) / np.linalg.norm(np.asarray(ref, np.float64)))
        bound = 8 * npar * U * np.linalg.cond(M)
        assert err <= bound, (npar, lam, trial, err, bound)


def test_solve_step_singular_matrix_gives_a_status_not_a_nan(so):
    v = np.array([1.0, 2.0, -1.0])
    A = np.outer(v, v)                       # rank 1
    step = np.full(3, 7.0)
    rc = so.ucf_fit_solve_step(3, np.ascontiguousarray(A), np.ones(3), 0.0, step)
    assert rc == abi.UCF_ERR_SINGULAR and b"positive definite" in so.ucf_last_error()
    assert np.isfinite(step).all() and (step == 0.0).all()
    assert so.ucf_fit_solve_step(3, np.zeros((3, 3)), np.ones(3), 1.0, step) == abi.UCF_ERR_SINGULAR
    # damping makes the rank-deficient matrix definite
    assert so.ucf_fit_solve_step(3, np.ascontiguousarray(A), np.ones(3), 1e-3, step) == 0 and np.isfinite(step).all()
    assert so.ucf_fit_solve_step(0, A, v, 0.0, step) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_solve_step(3, A, v, -1.0, step) == abi.UCF_ERR_BAD_ARGUMENT


def _create(so, P, ids, t, r, iz, z, obs, w, device=0):
    h = C.c_void_p()
    ids = np.ascontiguousarray(ids, np.int32)
    rc = so.ucf_fit_create(C.byref(P), len(ids), ids if len(ids) else np.zeros(1, np.int32), len(obs), np.ascontiguousarray(t, np.float64),
                           np.ascontiguousarray(r, np.float64), np.ascontiguousarray(iz, np.int32), len(z), np.ascontiguousarray(z, np.float64),
                           np.ascontiguousarray(obs, np.float64), np.ascontiguousarray(w, np.float64), device, C.byref(h))
    assert not h.value or rc == 0
    if h.value:
        so.ucf_fit_destroy(h)
    return rc, so.ucf_last_error()


def test_create_validates_before_it_looks_for_a_device(so):
    _, _, P = load_deck("neuman74_partpen")
    _, _, theis = load_deck("c1_theis")
    _, _, moench = load_deck("c3_moench")
    _, _, malama6 = load_deck("mishra_malama")
    n = 6
    good = dict(ids=[abi.PAR_KR, abi.PAR_KAPPA, abi.PAR_SS, abi.PAR_SY], t=np.logspace(0, 2, n), r=np.full(n, 30.0), iz=np.arange(n) % 2,
                z=[145.7, 100.0], obs=np.ones(n), w=np.ones(n))

    def case(P_=P, **kw):
        a = dict(good)
        a.update(kw)
        return _create(so, P_, a["ids"], a["t"], a["r"], a["iz"], a["z"], a["obs"], a["w"])

    def arr(key, i, v):
        x = np.array(good[key], float)
        x[i] = v
        return {key: x}

    bad = [
        (case(ids=[]), b"npar"),
        (case(ids=list(range(7)) + [abi.PAR_MOENCH_ALPHA0, abi.PAR_MOENCH_ALPHA0 + 1]), b"npar"),
        (case(ids=[abi.PAR_KR, abi.PAR_SS, abi.PAR_KR]), b"duplicate"),
        (case(theis, ids=[abi.PAR_KR, abi.PAR_SY]), b"Sy"),
        (case(theis, ids=[abi.PAR_KAPPA]), b"kappa"),
        (case(moench, ids=[abi.PAR_MOENCH_ALPHA0 + moench.MoenchM]), b"MoenchAlpha"),
        (case(ids=[abi.PAR_MOENCH_ALPHA0]), b"MoenchAlpha"),
        (case(ids=[abi.PAR_AC]), b"ac"), (case(ids=[abi.PAR_AK]), b"ak"), (case(ids=[abi.PAR_USL]), b"usL"),
        (case(malama6, ids=[abi.PAR_USL]), b"usL"),
        (case(t=good["t"][:3], r=good["r"][:3], iz=good["iz"][:3], obs=good["obs"][:3], w=good["w"][:3]), b"nobs"),
        (case(iz=[0, 1, 2, 0, 1, 0]), b"iz[2]"), (case(iz=[0, -1, 0, 0, 1, 0]), b"iz[1]"),
        (case(**arr("w", 4, -1.0)), b"weight[4]"), (case(**arr("w", 0, np.inf)), b"weight[0]"), (case(**arr("w", 5, np.nan)), b"weight[5]"),
        (case(**arr("obs", 3, np.nan)), b"obs[3]"), (case(**arr("obs", 1, np.inf)), b"obs[1]"),
        (case(**arr("t", 2, np.nan)), b"t[2]"), (case(**arr("t", 2, np.inf)), b"t[2]"),
        (case(**arr("r", 5, np.nan)), b"r[5]"), (case(**arr("r", 0, -np.inf)), b"r[0]"),
    ]
    for (rc, msg), word in bad:
        assert rc == abi.UCF_ERR_BAD_ARGUMENT, (word, rc, msg)
        assert word in msg, (word, msg)
    # a base set that the plan builder refuses keeps its own status
    Pbad = UcfParams.from_buffer_copy(_bytes(P))
    Pbad.b = -1.0
    assert case(Pbad)[0] == -3
    # a valid request: the device check comes last
    import torch
    rc, msg = case()
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc == abi.UCF_ERR_NO_DEVICE and b"no CPU fallback" in msg
