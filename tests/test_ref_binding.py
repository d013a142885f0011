"""The reference-side binding of INTEGRATION.md section 2, compiled once (oracle/ref_binding_driver.f90, test
infrastructure): the REFERENCE's own read_input fills its types, the INTEGRATION.md mapping copies them into ucf_params
through the shipped ISO_C_BINDING module, and the loop nest of driver.f90:100-232 is one call into libucf.so.

  * no GPU: ucf_nondimensionalise of the mapped block == what read_input left in w / f / s (driver_io.f90:531-567), bit
    for bit, for every model; times, radii, depths, layers and split indices that the call receives == the product's
    own deck path (unconfined_amd.engine.grids_from_deck);
  * GPU: the file the binding driver writes (header by the reference's own writer) against the reference binary's.
The reference's side of both is also stored (tests/golden/refout/, oracle/gen_refout.py): the nondim listing's reference
column, checked against the library's own mapping of the deck wherever the driver is absent too, and the header lines.
The driver links the reference's modules from oracle/_ref/O2 (built where /root/reference exists; the binaries travel to
the GPU box).  Nothing here is product code."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from golden_util import DECKS, REFOUT, e2e_gate_bounds, load_deck, load_e2e, ref_out_lines, rel_err, unhx
from unconfined_amd.deck import Deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "O2", "ref_binding_driver")

NAMES = ["neuman74_partpen", "c1_theis", "hantush_lay3", "hstorage_partpen_lay2", "c3_moench", "malama_fullpen", "c4_malama_partpen",
         "mishra_malama", "c5_mishra_fd64", "neuman_sched2"]


def _run(tmp_path, name, *args):
    dk = Deck.read(os.path.join(DECKS, f"{name}.in"))
    for fn in (f"{name}.in", dk.timeFileName if dk.timeseries else dk.spaceFileName):
        shutil.copy(os.path.join(DECKS, fn), tmp_path)
    return subprocess.run([DRIVER, f"{name}.in", *args], cwd=tmp_path, capture_output=True, text=True), dk


def _need_driver():
    if not os.path.exists(DRIVER):
        pytest.skip("oracle/_ref/O2/ref_binding_driver not built (needs /root/reference + flang: __graft_entry__.build())")


def _stored_nondim(name):
    """the reference's column of `ref_binding_driver <deck>.in nondim` (tests/golden/refout/<deck>.nondim)"""
    with open(os.path.join(REFOUT, f"{name}.nondim")) as f:
        return [ln.split() for ln in f if ln.strip()]


def _reference_side(rows):
    return [r[:4] if r[0] == "sizes" else r[:3] if r[0] in ("tD", "rD", "zD") else r[:2] for r in rows]


def _hx(x):
    return "%016X" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.mark.parametrize("name", NAMES)
def test_mapped_params_reproduce_read_input(tmp_path, oracle, name):
    _need_driver()
    res, dk = _run(tmp_path, name, "nondim")
    assert res.returncode == 0, res.stdout + res.stderr
    rows = [ln.split() for ln in res.stdout.split("\n") if ln.strip()]
    assert _reference_side(rows) == _stored_nondim(name)        # the stored reference column is this driver's
    _check_nondim_rows(oracle, name, dk, rows)


@pytest.mark.parametrize("name", NAMES)
def test_stored_read_input_matches_library_nondim(oracle, name):
    """the same checks on the stored reference column (no driver needed): the library's side here is
    ucf_nondimensionalise of the product's own mapping of the deck (unconfined_amd.abi.params_from_deck), not the
    Fortran binding -- that one is test_mapped_params_reproduce_read_input's"""
    from unconfined_amd import lib as ucflib
    from unconfined_amd.abi import UcfDerived, params_from_deck
    dk = Deck.read(os.path.join(DECKS, f"{name}.in"))
    D = UcfDerived()
    ucflib.check(ucflib.load().ucf_nondimensionalise(C.byref(params_from_deck(dk)), C.byref(D)))
    rows, m = [], 0
    for r in _stored_nondim(name):
        if r[0] == "sizes":
            rows.append(r + [str(D.nj0z)])
        elif r[0] in ("tD", "rD", "zD"):
            rows.append(r)
        elif r[0] == "MoenchGamma":
            rows.append(r + [_hx(D.MoenchGamma[m])])
            m += 1
        else:
            rows.append(r + [_hx(getattr(D, r[0]))])
    _check_nondim_rows(oracle, name, dk, rows)


def _check_nondim_rows(oracle, name, dk, rows):
    from unconfined_amd import engine
    pairs = [(r[0], r[1], r[2]) for r in rows if r[0] not in ("sizes", "tD", "rD", "zD")]
    assert len(pairs) >= 10
    for nm, ref_bits, lib_bits in pairs:
        assert ref_bits == lib_bits, (name, nm, unhx(ref_bits), unhx(lib_bits))
    sizes = next(r for r in rows if r[0] == "sizes")
    assert sizes[1:3] == [str(2 * dk.M + 1), str(2 ** dk.k - 1)] and sizes[3] == sizes[4]      # np, N, size(h%j0z) == nj0z
    # what the call receives: the reference's tD / sv, rD, zD / zLay against the product's own deck path (host
    # arithmetic of the library through ctypes: ucf_logspace, ucf_linspace; the layer and split rules from the oracle)
    from unconfined_amd.abi import params_from_deck
    P = params_from_deck(dk)
    D = oracle.nondim(P)
    _, ts, _ = load_deck(name)
    t = engine.logspace(ts.min_log, ts.max_log, ts.n)
    tD = np.array([unhx(r[1]) for r in rows if r[0] == "tD"])
    sv = np.array([int(r[2]) for r in rows if r[0] == "tD"])
    assert np.array_equal(tD, t / D.Tc)
    assert np.array_equal(sv, oracle.split_vector(list(dk.j0s), tD))
    rD = np.array([unhx(r[1]) for r in rows if r[0] == "rD"])
    assert np.array_equal(rD, np.array([dk.rval / D.Lc]))
    zD = np.array([unhx(r[1]) for r in rows if r[0] == "zD"])
    zl = np.array([int(r[2]) for r in rows if r[0] == "zD"])
    zz = engine.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd)
    assert np.array_equal(zD, zz / D.Lc)
    assert np.array_equal(zl, oracle.zlay(D, zD))


def test_binding_driver_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _need_driver()
    res, dk = _run(tmp_path, "neuman74_partpen", "gpu")
    assert res.returncode != 0
    assert "no CPU fallback" in res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("neuman74_partpen", "faithful"), ("neuman74_partpen", "fast"), ("c3_moench", "fast"),
                                       ("hstorage_partpen_lay2", "faithful"), ("mishra_fd30", "fast")])
def test_binding_driver_file_matches_reference(tmp_path, oracle, name, mode):
    """the reference's driver with its loop nest replaced by ucf_drawdown_grid: header lines identical to the reference
    binary's file (they come from the reference's own writer), rows within the end-to-end gate (2)"""
    assert os.path.exists(DRIVER), "oracle/_ref/O2/ref_binding_driver must travel with the repository"
    res, dk = _run(tmp_path, name, "gpu", mode)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in open(tmp_path / dk.outFileName, errors="replace").read().split("\n") if ln]
    rows = np.array([[float(x) for x in ln.split()[:3]] for ln in lines if not ln.startswith("#")])
    e2e = load_e2e(name)
    ir = int(np.argmin(np.abs(e2e["radii"] - dk.rval)))
    assert e2e["radii"][ir] == dk.rval
    ref, bh, bd = e2e_gate_bounds(oracle, name, ir)
    assert rows.shape == ref.shape
    assert np.array_equal(rows[:, 0], ref[:, 0])
    assert (rel_err(rows[:, 1], ref[:, 1], 1e-3) <= bh).all()
    assert (rel_err(rows[:, 2], ref[:, 2], 1e-3) <= bd).all()
    theirs = [ln for ln in ref_out_lines(name) if ln.startswith("#")]     # the reference binary's file, stored
    assert [ln for ln in lines if ln.startswith("#")] == theirs
