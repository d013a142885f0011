"""Every instantiation of fit_reduce_kernel<NPAR, SOURCE, DERIV> (ucf_fit.hip: NPAR 0..8 x slots / network / field x with or
without derivative data = 54) on synthetic data, bit for bit against the documented arithmetic.

ucf_debug_fit_reduce runs the production launcher (ucf_fit_launch_reduce, hence the same choice of instantiation as a real
fit) on caller data; tests/fit_reduce_restate.py restates the arithmetic in numpy one rounded operation at a time and builds the
inputs; tests/test_fit_reduce_restate.py shows on the CPU that the restatement computes the right quantity and that the data
tell the documented order of the sums from three changed ones.  The kernel is built without contraction, uses no
floating-point atomics and only IEEE +, -, x and /: no tolerance anywhere in this module.  Any NaN stands for any NaN.

Shapes: for every instantiation nobs = 1 (one lane of one wave), 64 (a wave exactly full) and 257 (a workgroup full and one
observation past it) with 3 parameter sets (workgroups 1 and 2: plan0 = set x NPLANS); for NPAR 0, 1, 4, 8 also nobs = 63, 65,
255, 256, 300, 513 (a third pass) and 1025 (a fifth) with 2 sets.  Inputs (fit_reduce_restate.synthetic): values of mixed sign
over six decades, Hc different per plan, two_dlog = 2e-3, weights that are not 1; observations of every kind by i % 12 -- base
value NaN, one perturbed plan +Inf, w = 0, wd = 0 over NaN in every sd[k] and in dobs (must count), wd > 0 over one sd[k] that is
not finite (must not), wd > 0 with w = 0, the Wynn sentinel; refs in three groups of different prefix and stride, at > 0,
counts 1, 2 (the loop of network_h runs no iteration), 3, 5, 32; field observations of 0 (+0.0, finite, counted), 1, 2, 3 and 7
terms, negative q, tfac = 1 and > 1.

Per case: every sum (phi, g, upper A, phi_d), nbad, and J, sim, Jd, simd in full -- the rows of observations that do not count
hold what was computed -- have the bytes of the restatement; nbad is the number the rule excludes, counted from the pattern of
kinds alone; a call that asks for none of J, sim, Jd, simd, and a repeated call, give the same bytes; with every wd = 0 the call
with derivative data has the bits of the call without on the same h, and phi_d = +0.0."""
import time

import numpy as np
import pytest

import fit_reduce_restate as fr
from test_fit_reduce_restate import SOURCE_NAMES, cases_of
from test_gpu_field_ensemble import same_bits

pytestmark = pytest.mark.gpu

launched = {}          # (NPAR, source, DERIV) -> [nobs ...] that ran on the device
spent = [0.0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def run_case(source, npar, deriv, nobs, nsets):
    t0 = time.perf_counter()
    src = fr.SOURCES[source]
    inp, nterm = fr.synthetic(src, npar, deriv, nobs, nsets)
    want = fr.restate(inp)
    got = fr.debug_fit_reduce(inp)
    launched.setdefault((npar, source, deriv), []).append(nobs)
    what = (source, npar, deriv, nobs)
    keys = ("sums", "nbad", "J", "sim") + (("Jd", "simd") if deriv else ())
    assert sorted(got) == sorted(keys), what
    for k in keys:
        same_bits(got[k], want[k], what + (k,))
    bad = fr.expected_bad(src, npar, deriv, nobs, nterm)
    assert (got["nbad"] == int(bad.sum())).all(), what + (got["nbad"], int(bad.sum()))
    # asking for less changes nothing; a repeated call gives the same bytes
    less = fr.debug_fit_reduce(inp, want=())
    assert sorted(less) == ["nbad", "sums"], what
    again = fr.debug_fit_reduce(inp)
    for k in keys:
        assert again[k].tobytes() == got[k].tobytes(), what + (k, "repeated")
        if k in less:
            assert less[k].tobytes() == got[k].tobytes(), what + (k, "asked for alone")
    if deriv:
        # every derivative weight zero: the bits of the reduction without derivative data, whatever dh and dobs hold
        off = fr.debug_fit_reduce({**inp, "wd": np.zeros(nobs)})
        plain = fr.debug_fit_reduce({**inp, "dh": None, "dobs": None, "wd": None})
        assert off["sums"][:, :-1].tobytes() == plain["sums"].tobytes(), what + ("all wd = 0",)
        assert off["sums"][:, -1].tobytes() == np.zeros(nsets).tobytes(), what + ("phi_d = +0.0",)
        for k in ("nbad", "J", "sim"):
            assert off[k].tobytes() == plain[k].tobytes(), what + (k, "all wd = 0")
        same_bits(off["simd"], got["simd"], what + ("simd, all wd = 0",))
        assert (plain["nbad"] == int(fr.expected_bad(src, npar, False, nobs, nterm).sum())).all(), what
    spent[0] += time.perf_counter() - t0


@pytest.mark.parametrize("npar", range(9))
@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
def test_instantiation_bit_for_bit(gpu, source, deriv, npar):
    for nobs, nsets in cases_of(npar):
        run_case(source, npar, deriv, nobs, nsets)


def test_every_instantiation_was_launched(gpu):
    """the list of (NPAR, source, DERIV) that this module ran on the device and their count: all 54 (a combination that the
    tests above did not run -- the module was cut down with -k -- runs its smallest case here)"""
    for source in SOURCE_NAMES:
        for deriv in (False, True):
            for npar in range(9):
                if (npar, source, deriv) not in launched:
                    run_case(source, npar, deriv, 1, 3)
    for key in sorted(launched):
        print(f"[fit reduce edges] NPAR={key[0]} {key[1]} DERIV={key[2]}: nobs {launched[key]}")
    print(f"[fit reduce edges] {len(launched)} instantiations, {sum(len(v) for v in launched.values())} cases, {spent[0]:.1f} s in them")
    assert len(launched) == 54
