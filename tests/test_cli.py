"""`python -m unconfined_amd deck` against `./unconfined deck` (what the reference binary writes, stored under
tests/golden/refout/ by oracle/gen_refout.py): identical header bytes, identical time/space columns, values within
the end-to-end gate."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from golden_util import DECKS, REFOUT, e2e_gate_bounds, load_e2e, ref_out_lines, rel_err
from unconfined_amd.deck import Deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _cli(tmp_path, name, mode="faithful"):
    dk = Deck.read(os.path.join(DECKS, f"{name}.in"))
    for fn in (f"{name}.in", dk.timeFileName if dk.timeseries else dk.spaceFileName):
        shutil.copy(os.path.join(DECKS, fn), tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, "-m", "unconfined_amd", f"{name}.in", "--mode", mode, "--out", "ours.out"],
                         cwd=tmp_path, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return dk, [ln for ln in open(tmp_path / "ours.out").read().split("\n") if ln]


@pytest.mark.parametrize("name", ["neuman74_partpen", "c3_moench"])
def test_cli_time_series_file(tmp_path, oracle, name):
    dk, ours = _cli(tmp_path, name)
    ref = [ln for ln in ref_out_lines(name) if ln]
    assert len(ours) == len(ref)
    assert [a for a in ours if a.startswith("#")] == [b for b in ref if b.startswith("#")]
    va = np.array([[float(x) for x in a.split()] for a in ours if not a.startswith("#")])
    vb = np.array([[float(x) for x in b.split()] for b in ref if not b.startswith("#")])
    assert np.array_equal(va[:, 0], vb[:, 0])
    e2e = load_e2e(name)
    ir = int(np.argmin(np.abs(e2e["radii"] - dk.rval)))
    fix, bh, bd = e2e_gate_bounds(oracle, name, ir)          # the gate of tests/test_gpu_parity.py, per row
    assert np.array_equal(fix, vb)                            # the stored file holds what the e2e fixture holds
    assert (rel_err(va[:, 1], vb[:, 1], 1e-3) <= bh).all()
    assert (rel_err(va[:, 2], vb[:, 2], 1e-3) <= bd).all()


def test_cli_contour_file_every_radius(tmp_path):
    """contour mode: header bytes and (z, r) columns against the reference's contour run; VALUES at every (r, z)
    against one reference TIME-SERIES run per point -- the reference's own contour values are wrong for every radius
    after the first (it keeps the first radius' tanh-sinh abscissae), its single-point runs are
    not.  Gate: max(1e-10, 20 x the reference's -O2 / -O3-native spread at that point).  The reference's runs are
    stored: tests/golden/refout/contour_neuman.out and contour_points.npz (oracle/gen_refout.py)."""
    name = "contour_neuman"
    dk, ours = _cli(tmp_path, name)
    ref = [ln for ln in ref_out_lines(name) if ln]
    assert len(ours) == len(ref)
    assert [a for a in ours if a.startswith("#")] == [b for b in ref if b.startswith("#")]
    va = np.array([[float(x) for x in a.split()] for a in ours if not a.startswith("#")])
    vb = np.array([[float(x) for x in b.split()] for b in ref if not b.startswith("#")])
    assert np.array_equal(va[:, :2], vb[:, :2])
    pts = np.load(os.path.join(REFOUT, "contour_points.npz"))
    assert np.array_equal(pts["zr"], vb[:, :2])              # one stored point run per (z, r) of the contour, in its order
    wrong_in_reference = 0
    for row_ours, row_contour, p0, p1 in zip(va, vb, pts["O2"], pts["O3native"]):
        z, r = row_ours[0], row_ours[1]
        (t0, h0, d0), (_, h1, d1) = p0, p1
        assert t0 == dk.tval
        bh = max(1e-10, 20.0 * float(rel_err(h1, h0, 1e-3)))
        bd = max(1e-10, 20.0 * float(rel_err(d1, d0, 1e-3)))
        assert rel_err(row_ours[2], h0, 1e-3) <= bh, (z, r, row_ours[2], h0)
        assert rel_err(row_ours[3], d0, 1e-3) <= bd, (z, r, row_ours[3], d0)
        wrong_in_reference += int(rel_err(row_contour[2], h0, 1e-3) > 1e-6)
    assert wrong_in_reference > 0            # quirk Q1 is real: the reference's contour file disagrees with its own point runs
