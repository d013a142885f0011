"""Byte-level check of unconfined_amd/output.py against files written by the reference binary
(oracle/_ref/O2/unconfined, stored under tests/golden/refout/ by oracle/gen_refout.py).  Numbers are
taken from the reference file itself, so this tests formatting only."""
import os

import numpy as np
import pytest

from golden_util import DECKS, load_deck, ref_out_lines
from unconfined_amd import output


@pytest.mark.parametrize("name", ["neuman74_partpen", "c3_moench", "mishra_fd30", "hantush_lay2", "theis_pulse",
                                  "mishra_malama", "hstorage_partpen_lay2"])
def test_timeseries_file_matches_reference_bytes(oracle, name):
    dk, ts, P = load_deck(name)
    ref_lines = ref_out_lines(name)
    rows_ref = [ln for ln in ref_lines if ln and not ln.startswith("#")]
    vals = np.array([[float(x) for x in ln.split()] for ln in rows_ref])
    D = oracle.nondim(P)
    z = oracle.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd)
    head = output.timeseries_header(dk, D, dk.rval, dk.rval / D.Lc, z[0], z[0] / D.Lc, len(vals))
    mine = head + output.timeseries_rows(vals[:, 0], vals[:, 1], vals[:, 2])
    ref_clean = [ln for ln in ref_lines if ln != ""]
    assert len(mine) == len(ref_clean)
    for a, b in zip(mine, ref_clean):
        assert a == b, (a, b)


def test_es_edit_descriptors():
    assert output.rfmt(0.1) == " 1.0000000E-01"
    assert output.rfmt(-123456.789) == "-1.2345679E+05"
    assert output.hfmt(4.417735711365508e-03) == " 4.417735711365508E-0003"
    assert output.hfmt(-1.436398020545476) == "-1.436398020545476E+0000"
    assert output.rfmt(0.0) == " 0.0000000E+00"
    assert output.rfmt(1e-100) == "*" * 14          # exponent does not fit E2
    assert output.hfmt(float("nan")).strip() == "NaN"


def test_contour_file_matches_reference_bytes(oracle):
    """contour mode (timeseries = F): header of driver_io.f90:760-845 and rows of driver.f90:259-271.
    (Values of the reference are only trustworthy for its first radius, SURVEY.md quirk Q1 -- this test
    re-formats the reference's own numbers.)"""
    from unconfined_amd.deck import Deck, SpaceSpec
    name = "contour_neuman"
    dk = Deck.read(os.path.join(DECKS, f"{name}.in"))
    ref_lines = [ln for ln in ref_out_lines(name) if ln != ""]
    vals = np.array([[float(x) for x in ln.split()] for ln in ref_lines if not ln.startswith("#")])
    from unconfined_amd.abi import params_from_deck
    D = oracle.nondim(params_from_deck(dk))
    sp = SpaceSpec.read(os.path.join(DECKS, dk.spaceFileName))
    r = oracle.linspace(sp.min_r, sp.max_r, sp.n_r)
    z = oracle.linspace(sp.min_z, sp.max_z, sp.n_z)
    head = output.contour_header(dk, D, r, z, dk.tval, dk.tval / D.Tc)
    h = vals[:, 2].reshape(len(r), len(z)); dh = vals[:, 3].reshape(len(r), len(z))
    mine = head + output.contour_rows(z, r, h, dh)
    assert len(mine) == len(ref_lines)
    for a, b in zip(mine, ref_lines):
        assert a == b, (a, b)
