"""Every ROBUST instantiation of fit_reduce_kernel<NPAR, SOURCE, DERIV, ROBUST> (ucf_fit.hip: NPAR 0..8 x slots / network / field x
with or without derivative data = 54, each under both kinds of loss, the kind being a wave-uniform argument) on synthetic data,
bit for bit against the arithmetic that include/ucf.h states with ucf_fit_set_loss.

ucf_debug_fit_reduce_loss runs the production launcher (ucf_fit_launch_reduce) on caller data; tests/fit_loss_restate.py restates
the arithmetic in numpy one rounded operation at a time on the inputs of tests/fit_reduce_restate.py; tests/test_fit_loss_host.py
shows on the CPU that the restatement computes the loss and that, with c = fit_loss_restate.C_GPU, every case has at least 10 % of
its residual terms on each side of c.  The kernel is built without contraction, uses no floating-point atomics and only IEEE +,
-, x, / and comparisons: no tolerance anywhere in this module.  Any NaN stands for any NaN.

Shapes: for every instantiation and kind nobs = 1, 64 and 257 with 3 parameter sets; for NPAR 0, 1, 4, 8 also nobs = 63, 65, 256
and 513 with 2 sets.  Per case: every sum (phi, g, upper A, phi_d, phi_w), nbad, ndown, b, bd and J, sim, Jd, simd in full have
the bytes of the restatement; a repeated call gives the same bytes; a call that asks for none of the optional outputs gives the
same sums and nbad; Huber with c = 1e300 gives the bytes of ucf_debug_fit_reduce in phi, g, A, phi_d, nbad, J, sim, Jd, simd, phi_w
the bytes of phi, ndown = 0 and b = 1.0 where the observation counts."""
import time

import numpy as np
import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
from test_fit_loss_host import KIND_NAMES, SOURCE_NAMES, loss_cases_of
from test_gpu_field_ensemble import same_bits

pytestmark = pytest.mark.gpu

launched = {}          # (kind, NPAR, source, DERIV) -> [nobs ...] that ran on the device
spent = [0.0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def run_case(kind, source, npar, deriv, nobs, nsets):
    t0 = time.perf_counter()
    inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, nsets)
    k, c = fl.KINDS[kind], fl.C_GPU
    want = fl.restate(inp, k, c)
    got = fl.debug_fit_reduce_loss(inp, k, c)
    launched.setdefault((kind, npar, source, deriv), []).append(nobs)
    what = (kind, source, npar, deriv, nobs)
    keys = ("sums", "nbad", "ndown", "b", "J", "sim") + (("bd", "Jd", "simd") if deriv else ())
    assert sorted(got) == sorted(keys), what
    for key in keys:
        same_bits(got[key], want[key], what + (key,))
    assert (got["ndown"] > 0).all() or nobs == 1, what + (got["ndown"],)
    # a repeated call gives the same bytes; asking for none of the optional outputs changes nothing
    again = fl.debug_fit_reduce_loss(inp, k, c)
    less = fl.debug_fit_reduce_loss(inp, k, c, want=())
    assert sorted(less) == ["nbad", "sums"], what
    for key in keys:
        assert again[key].tobytes() == got[key].tobytes(), what + (key, "repeated")
        if key in less:
            assert less[key].tobytes() == got[key].tobytes(), what + (key, "asked for alone")
    if kind == "huber":
        # c beyond every residual: least squares, byte for byte
        big = fl.debug_fit_reduce_loss(inp, k, 1.0e300)
        plain = fr.debug_fit_reduce(inp)
        n = fr.nsums(npar, deriv)
        assert np.ascontiguousarray(big["sums"][:, :n]).tobytes() == plain["sums"].tobytes(), what + ("c = 1e300",)
        assert big["sums"][:, -1].tobytes() == plain["sums"][:, 0].tobytes(), what + ("phi_w = phi",)
        for key in ("nbad", "J", "sim") + (("Jd", "simd") if deriv else ()):
            assert big[key].tobytes() == plain[key].tobytes(), what + (key, "c = 1e300")
        assert (big["ndown"] == 0).all(), what
        counted = want["counted"]
        assert (big["b"][counted] == 1.0).all() and np.isnan(big["b"][~counted]).all(), what
        if deriv:
            assert (big["bd"][want["weighted"]] == 1.0).all() and np.isnan(big["bd"][~want["weighted"]]).all(), what
    spent[0] += time.perf_counter() - t0


@pytest.mark.parametrize("npar", range(9))
@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_robust_instantiation_bit_for_bit(gpu, kind, source, deriv, npar):
    for nobs, nsets in loss_cases_of(npar):
        run_case(kind, source, npar, deriv, nobs, nsets)


def test_every_robust_instantiation_was_launched(gpu):
    """the list of (kind, NPAR, source, DERIV) that this module ran on the device and their count: all 108 (a combination that
    the tests above did not run -- the module was cut down with -k -- runs its smallest case here)"""
    for kind in KIND_NAMES:
        for source in SOURCE_NAMES:
            for deriv in (False, True):
                for npar in range(9):
                    if (kind, npar, source, deriv) not in launched:
                        run_case(kind, source, npar, deriv, 1, 3)
    for key in sorted(launched):
        print(f"[fit loss edges] {key[0]} NPAR={key[1]} {key[2]} DERIV={key[3]}: nobs {launched[key]}")
    print(f"[fit loss edges] {len(launched)} combinations, {sum(len(v) for v in launched.values())} cases, {spent[0]:.1f} s in them")
    assert len(launched) == 108
