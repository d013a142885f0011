#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- stores what the reference binaries write, so that the tests that compare against them need
nothing outside the repository (tests/golden/refout/).

Runs only where `make -C oracle ref` has built oracle/_ref/ (flavours O2 and O3native, and the binding driver):
  <deck>.out            the file oracle/_ref/O2/unconfined writes for tests/golden/decks/<deck>.in, byte for byte
                        (tests/test_output_format.py, tests/test_cli.py, tests/test_fortran_host.py)
  contour_points.npz    contour_neuman.in: for every (z, r) of its contour the single-point time-series run of both
                        flavours, columns t, h, dh (tests/test_cli.py::test_cli_contour_file_every_radius)
  <deck>.nondim         the REFERENCE side of `ref_binding_driver <deck>.in nondim`: what its read_input leaves in
                        w / f / s as bit patterns, and the times, radii, depths it hands on
                        (tests/test_ref_binding.py::test_mapped_params_reproduce_read_input)
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from unconfined_amd.deck import Deck, TimeSpec  # noqa: E402

DECKS = os.path.join(ROOT, "tests", "golden", "decks")
OUT = os.path.join(ROOT, "tests", "golden", "refout")
REF = {f: os.path.join(HERE, "_ref", f, "unconfined") for f in ("O2", "O3native")}
DRIVER = os.path.join(HERE, "_ref", "O2", "ref_binding_driver")

OUT_DECKS = ["neuman74_partpen", "c3_moench", "mishra_fd30", "hantush_lay2", "theis_pulse", "mishra_malama",
             "hstorage_partpen_lay2", "c1_theis", "malama_partpen_b1", "contour_neuman"]
NONDIM_DECKS = ["neuman74_partpen", "c1_theis", "hantush_lay3", "hstorage_partpen_lay2", "c3_moench", "malama_fullpen",
                "c4_malama_partpen", "mishra_malama", "c5_mishra_fd64", "neuman_sched2"]
ENV = dict(os.environ, OMP_NUM_THREADS="4")


def stage(work, name):
    dk = Deck.read(os.path.join(DECKS, f"{name}.in"))
    for fn in (f"{name}.in", dk.timeFileName if dk.timeseries else dk.spaceFileName):
        shutil.copy(os.path.join(DECKS, fn), work)
    return dk


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in OUT_DECKS:
        with tempfile.TemporaryDirectory() as work:
            dk = stage(work, name)
            subprocess.run([REF["O2"], f"{name}.in"], cwd=work, env=ENV, check=True, capture_output=True)
            shutil.copyfile(os.path.join(work, dk.outFileName), os.path.join(OUT, f"{name}.out"))
    # contour: one time-series run per (z, r) of the contour, both flavours
    name = "contour_neuman"
    with tempfile.TemporaryDirectory() as work:
        dk = stage(work, name)
        subprocess.run([REF["O2"], f"{name}.in"], cwd=work, env=ENV, check=True, capture_output=True)
        rows = [ln for ln in open(os.path.join(work, dk.outFileName), errors="replace").read().split("\n") if ln and not ln.startswith("#")]
        zr = np.array([[float(x) for x in ln.split()[:2]] for ln in rows])
        TimeSpec(False, 0, 1, 1, times=[dk.tval]).write(os.path.join(work, "one_time.dat"))
        pts = {f: [] for f in REF}
        for z, r in zr:
            d = dk.replace(timeseries=True, piezometer=True, rval=float(r), zTop=float(z), zBot=float(z), timeFileName="one_time.dat",
                           outFileName="pt.out")
            d.write(os.path.join(work, "pt.in"))
            for f, exe in REF.items():
                subprocess.run([exe, "pt.in"], cwd=work, env=ENV, check=True, capture_output=True)
                pr = [ln for ln in open(os.path.join(work, "pt.out"), errors="replace").read().split("\n") if ln and not ln.startswith("#")]
                assert len(pr) == 1
                pts[f].append([float(x) for x in pr[0].split()])
        np.savez(os.path.join(OUT, "contour_points.npz"), zr=zr, **{f: np.array(v) for f, v in pts.items()})
    # the reference side of the binding driver's nondim listing (its third column, the library's bits, is dropped)
    for name in NONDIM_DECKS:
        with tempfile.TemporaryDirectory() as work:
            stage(work, name)
            res = subprocess.run([DRIVER, f"{name}.in", "nondim"], cwd=work, capture_output=True, text=True, check=True)
        keep = []
        for ln in res.stdout.split("\n"):
            r = ln.split()
            if not r or r[0] in ("Fortran", "IEEE"):
                continue
            keep.append(" ".join(r[:4] if r[0] == "sizes" else r[:2] if r[0] not in ("tD", "rD", "zD") else r[:3]))
        with open(os.path.join(OUT, f"{name}.nondim"), "w") as f:
            f.write("\n".join(keep) + "\n")


if __name__ == "__main__":
    main()
