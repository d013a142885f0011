"""Every RESAMPLE instantiation of fit_reduce_kernel<NPAR, SOURCE, DERIV, MODE> (ucf_fit.hip: NPAR 0..8 x slots / network / field x
with or without derivative data = 54, each under least squares, Huber and Tukey, the kind being a wave-uniform argument) on
synthetic data, bit for bit against the arithmetic that include/ucf.h states with ucf_fit_set_resample.

ucf_debug_fit_reduce_resampled runs the production launcher (ucf_fit_launch_reduce) on caller data; tests/fit_resample_restate.py
restates the arithmetic in numpy one rounded operation at a time on the inputs of tests/fit_reduce_restate.py;
tests/test_fit_resample_host.py shows on the CPU that with unit multiplicities the restatement is that of the loss.  The kernel is
built without contraction, uses no floating-point atomics and only IEEE +, -, x, / and comparisons: no tolerance anywhere in this
module.  Any NaN stands for any NaN.

Shapes: for every instantiation and kind nobs = 1, 63, 64, 65, 255, 256, 257 and 513 with nsets = 2, nrep = 4, nred = 5, set_of =
[1, 0, 1, 1, 0], rep = [-1, 0, 2, 1, 3]; the rows of mult are all ones, random 0..3 with zeros, 65535 and zeros, and all zero (every
sum but phi_out +0.0, nuse = 0).  The inputs plant non-finite values as the existing edge tests do, so held-out observations that are
not finite occur (they are in neither nbad nor nheld: the restatement's counts, which tests/test_fit_resample_host.py checks against
the pattern).  Per case: every sum and count has the bytes of the restatement; a repeated call gives the same bytes; with identity
set_of and either rep = -1 or the all-ones row, phi | g | A | [phi_d] | phi_w, nbad and ndown have the bytes of
ucf_debug_fit_reduce_loss and, under least squares, phi | g | A | [phi_d] and nbad those of ucf_debug_fit_reduce."""
import time

import numpy as np
import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
import fit_resample_restate as frs
from test_fit_resample_host import KIND_NAMES, NOBS_GPU, SOURCE_NAMES
from test_gpu_field_ensemble import same_bits

pytestmark = pytest.mark.gpu

launched = {}          # (kind, NPAR, source, DERIV) -> [nobs ...] that ran on the device
spent = [0.0]
NSETS = 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def run_case(kind, source, npar, deriv, nobs):
    t0 = time.perf_counter()
    inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, NSETS)
    k, c = frs.KINDS[kind], frs.C_GPU
    mult = frs.gpu_mult(nobs)
    what = (kind, source, npar, deriv, nobs)
    want = frs.restate(inp, k, c, mult, frs.SET_OF, frs.REP)
    got = frs.debug_fit_reduce_resampled(inp, k, c, mult, frs.SET_OF, frs.REP)
    launched.setdefault((kind, npar, source, deriv), []).append(nobs)
    for key in ("sums", "nbad", "counts"):
        same_bits(got[key], want[key], what + (key,))
    # the all-zero row: +0.0 in every sum but phi_out, nothing used, nothing bad
    assert (got["sums"][4, :-1] == 0.0).all() and not np.signbit(got["sums"][4, :-1]).any(), what
    assert got["counts"][4, 0] == 0 and got["counts"][4, 1] == 0 and got["nbad"][4] == 0, what
    again = frs.debug_fit_reduce_resampled(inp, k, c, mult, frs.SET_OF, frs.REP)
    for key in ("sums", "nbad", "counts"):
        assert again[key].tobytes() == got[key].tobytes(), what + (key, "repeated")
    # unit multiplicities, identity set_of: the reduction without resampling, byte for byte
    ident = np.arange(NSETS, dtype=np.int32)
    n = fr.nsums(npar, deriv)
    unit = [frs.debug_fit_reduce_resampled(inp, k, c, mult, ident, np.zeros(NSETS, np.int32)),          # the all-ones row
            frs.debug_fit_reduce_resampled(inp, k, c, None, None, np.full(NSETS, -1, np.int32)),         # rep = -1, set_of NULL
            frs.debug_fit_reduce_resampled(inp, k, c, mult, ident, None)]                                # rep NULL
    if kind == "l2":
        plain = fr.debug_fit_reduce(inp, want=())
    else:
        loss = fl.debug_fit_reduce_loss(inp, k, c, want=("ndown",))
    for u in unit:
        assert (u["sums"][:, -1] == 0.0).all() and (u["counts"][:, 2] == 0).all(), what
        if kind == "l2":
            assert np.ascontiguousarray(u["sums"][:, :n]).tobytes() == plain["sums"].tobytes(), what + ("unit, l2",)
            assert u["sums"][:, n].tobytes() == plain["sums"][:, 0].tobytes(), what + ("phi_w = phi",)
            assert u["nbad"].tobytes() == plain["nbad"].tobytes() and (u["counts"][:, 3] == 0).all(), what
        else:
            assert np.ascontiguousarray(u["sums"][:, :-1]).tobytes() == loss["sums"].tobytes(), what + ("unit",)
            assert u["nbad"].tobytes() == loss["nbad"].tobytes(), what
            assert u["counts"][:, 3].tobytes() == loss["ndown"].tobytes(), what
    spent[0] += time.perf_counter() - t0


@pytest.mark.parametrize("npar", range(9))
@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_resample_instantiation_bit_for_bit(gpu, kind, source, deriv, npar):
    for nobs in NOBS_GPU:
        run_case(kind, source, npar, deriv, nobs)


def test_every_resample_instantiation_was_launched(gpu):
    """the list of (kind, NPAR, source, DERIV) that this module ran on the device and their count: 3 kinds x 54 (a combination that
    the tests above did not run -- the module was cut down with -k -- runs its smallest case here)"""
    for kind in KIND_NAMES:
        for source in SOURCE_NAMES:
            for deriv in (False, True):
                for npar in range(9):
                    if (kind, npar, source, deriv) not in launched:
                        run_case(kind, source, npar, deriv, 1)
    print(f"[fit resample edges] {len(launched)} combinations, {sum(len(v) for v in launched.values())} cases, {spent[0]:.1f} s in them")
    assert len(launched) == 162
