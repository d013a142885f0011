"""The host side of derivative data in a fit (ucf_fit_derivative_check, the tfac rule of a field fit, the declarations of
include/ucf.h): no GPU.  The device side is tests/test_gpu_fit_deriv.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from golden_util import load_deck
from unconfined_amd import fit as ufit
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -11
NEW = ("ucf_fit_derivative_check", "ucf_fit_set_derivative", "ucf_fit_evaluate_joint", "ucf_fit_debug_dh")


def refused(dobs, dweight):
    with pytest.raises(ucflib.UcfError) as e:
        ufit.derivative_check(dobs, dweight)
    assert e.value.status == BAD_ARGUMENT
    return e.value.message


def test_derivative_check_names_its_offender():
    n = 6
    d, w = np.linspace(0.1, 0.6, n), np.ones(n)
    assert "dobs" in refused(None, w) and "NULL" in refused(None, w)
    assert "dweight" in refused(d, None) and "NULL" in refused(d, None)
    for bad in (-1.0, -0.0 - 1e-300, np.nan, np.inf, -np.inf):
        x = w.copy(); x[4] = bad
        assert "dweight[4]" in refused(d, x), bad
    for bad in (np.nan, np.inf, -np.inf):
        x = d.copy(); x[2] = bad
        assert "dobs[2]" in refused(x, w), bad
        assert "dobs[2]" in refused(x, np.full(n, 1e-300)), bad      # any positive weight
    # the first offender in index order is the one named
    x, y = d.copy(), w.copy()
    x[1], y[3] = np.nan, -2.0
    assert "dobs[1]" in refused(x, y)
    x[1], y[0] = 0.2, np.nan
    assert "dweight[0]" in refused(x, y)


def test_derivative_gaps_are_accepted_and_nd_is_counted():
    n = 7
    d, w = np.linspace(0.1, 0.7, n), np.ones(n)
    assert ufit.derivative_check(d, w) == n
    assert ufit.derivative_check(d, np.zeros(n)) == 0
    assert ufit.derivative_check(np.full(n, np.nan), np.zeros(n)) == 0          # gaps: anything under a zero weight
    x, y = d.copy(), w.copy()
    x[[0, 5]] = [np.nan, np.inf]
    y[[0, 5]] = 0.0
    y[3] = 2.5
    assert ufit.derivative_check(x, y) == n - 2
    y[6] = -0.0                                                                  # -0.0 is a zero weight
    x[6] = np.nan
    assert ufit.derivative_check(x, y) == n - 3
    assert ufit.derivative_check(np.zeros(0), np.zeros(0)) == 0


def test_tfac_is_one_division_of_the_observation_time_by_the_term_time():
    """a hand-written field: P0 starts at 0, P1 at 2.5; tfac[k] = t[i] / term_t[k] with term_t from ucf_fit_field_terms, redone
    here.  A term towards a well that starts at 0 has term_t = t - 0 = t and tfac exactly 1; one towards P1 has
    t / (t - 2.5), the tfac of ucf_field_group for that group; an observation before a start has no term towards it"""
    _, _, P = load_deck("c1_theis")
    wells = [(0.0, 0.0, 1.0, 0.0), (3.0, 4.0, -0.5, 2.5)]
    obs_wells = [(1.0, 1.0), (-2.0, 0.5)]
    t = np.array([0.7, 2.5, 3.0, 10.0, 1.0e3 / 3.0])
    well = np.array([0, 1, 0, 1, 0], np.int32)
    tm = ufit.field_terms(P, wells, obs_wells, t, well)
    first, pump, term_t = tm["term_first"], tm["term_pump"], tm["term_t"]
    assert first.tolist() == [0, 1, 2, 4, 6, 8] and pump.tolist() == [0, 0, 0, 1, 0, 1, 0, 1]
    t_of_term = np.repeat(t, np.diff(first))
    tfac = t_of_term / term_t
    assert (tfac[pump == 0] == 1.0).all()
    want = np.array([3.0 / (3.0 - 2.5), 10.0 / (10.0 - 2.5), (1.0e3 / 3.0) / (1.0e3 / 3.0 - 2.5)])
    assert tfac[pump == 1].tobytes() == want.tobytes()
    assert (tfac[pump == 1] > 1.0).all()


def test_header_declares_and_library_exports_the_new_entries():
    so = ucflib.load()
    for s in NEW:
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    src = r'''
    #include "ucf.h"
    int main(void){
      int (*a)(int, const double*, const double*, int*) = ucf_fit_derivative_check;
      int (*b)(ucf_fit*, const double*, const double*) = ucf_fit_set_derivative;
      int (*c)(ucf_fit*, int, const double*, double, double*, double*, double*, int*, double*, double*, double*, double*, double*) =
          ucf_fit_evaluate_joint;
      int (*d)(ucf_fit*, int, int, int, double*, int*) = ucf_fit_debug_dh;
      return (a && b && c && d) ? 0 : 1; }'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        open(p, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", p, "-o", os.path.join(d, "t.o")],
                       check=True)
