"""Writes the fixtures of tests/test_gpu_field.py: tests/golden/field_<deck>.npz.  CPU only (the oracle and its binary128
build, tests/oracle_lib.py; the launched arrays come from ucf_field_group_from_params, host arithmetic that
tests/test_field_host.py checks against numpy); about a minute and a half.

    python tools/gen_field_fixture.py [neuman74_partpen | c2_neuman74_fullpen | c1_theis]

The field (the smallest that reaches every branch of ucf_field_drawdown), in units of the deck's length scale `unit`:
  wells      0 (0, 0) q = 1 and 1 (2, 0) q = 0.6 start at t0 = 0;  2 (0, 1.5) q = -0.5 (an injection) and 3 (1, -1) q = 0.8 start
             at t0 = 5: two groups;
  locations  five, of which (1, 0.7) is equidistant from wells 0 and 1: one shared column in group 0;
  times      six, of which 0.5 and 2 precede the later start: group 1 launches four.  Chosen among fourteen candidates from 0.3
             to 3000 so that every launched value of the grid path itself meets its bound b in both flavours (the times 0.3, 1,
             10, 20, 60 and 400 have a term that does not: the path misses its per-value gate there, whatever is summed);
  depths     two.
Stored:
  geometry   deck, wells [4][4] = (x, y, q, t0), locations [5][2], times [6], z [2];
  per group  g<g>_k0, g<g>_tD, g<g>_sv, g<g>_rD, g<g>_col, g<g>_tfac: the arrays of ucf_field_group;
             g<g>_ref_h, g<g>_ref_dh [nt_g][nr_g][nz]: the ORACLE's h x Hc and dh x Hc at every launched (tD, rD, z);
             g<g>_noise_h, g<g>_noise_dh: its distance from the binary128 build, |oracle - binary128| / max(|binary128|, 1e-3);
  reference  s_ref, ds_ref [6][5][2]: the oracle's values superposed by the arithmetic that include/ucf.h states (x Hc at the
             end).  Every stored value is asserted finite.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_deck          # noqa: E402
from oracle_lib import Oracle              # noqa: E402
from unconfined_amd.field import WellField  # noqa: E402

WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])
DECKS = {
    "neuman74_partpen": dict(unit=100.0, z=[145.7, 100.0]),
    "c2_neuman74_fullpen": dict(unit=100.0, z=[145.7, 100.0]),
    "c1_theis": dict(unit=3.0, z=[5.0, 9.0]),
}


def superpose(wells, groups, h, dh, nt, nloc, nz, Hc):
    """the arithmetic of field_superpose_kernel on per-group arrays h[g], dh[g] of shape [nt_g][nr_g][nz]"""
    s = np.zeros((nt, nloc, nz)); ds = np.zeros((nt, nloc, nz))
    for k in range(nt):
        for i in range(nloc):
            for iz in range(nz):
                a = b = np.float64(0.0)
                for j in range(len(wells)):
                    G = next(g for g, grp in enumerate(groups) if grp["col"][i, j] >= 0)
                    grp = groups[G]
                    if k < grp["k0"]:
                        continue
                    kk, c = k - grp["k0"], grp["col"][i, j]
                    a = a + wells[j, 2] * h[G][kk, c, iz]
                    b = b + wells[j, 2] * (grp["tfac"][kk] * dh[G][kk, c, iz])
                s[k, i, iz], ds[k, i, iz] = a * Hc, b * Hc
    return s, ds


def generate(deck, times=TIMES, path=None):
    cfg = DECKS[deck]
    dk, _, P = load_deck(deck)
    O, Q = Oracle(), Oracle(quad=True)
    D = O.nondim(P)
    wells = WELLS.copy(); wells[:, :2] *= cfg["unit"]
    loc = LOCATIONS * cfg["unit"]
    z = np.array(cfg["z"])
    zD = z / D.Lc
    zl = O.zlay(D, zD)
    field = WellField(wells, loc, times)
    groups = field.groups(P)
    out = dict(deck=np.array(deck), wells=wells, locations=loc, times=np.asarray(times, float), z=z)
    h, dh = [], []
    for g, grp in enumerate(groups):
        nt_g, nr_g = len(grp["tD"]), len(grp["rD"])
        assert (grp["sv"] == O.split_vector(list(dk.j0s), grp["tD"])).all()
        TT, RR = np.meshgrid(grp["tD"], grp["rD"], indexing="ij")
        sv = np.repeat(grp["sv"], nr_g)
        ho, dho = O.batch(P, TT.ravel(), RR.ravel(), sv, zD, zl, 8)
        ht, dht = Q.batch(P, TT.ravel(), RR.ravel(), sv, zD, zl, 16)
        shape = (nt_g, nr_g, len(z))
        h.append(ho.reshape(shape)); dh.append(dho.reshape(shape))
        for name, ref, truth in (("h", ho, ht), ("dh", dho, dht)):
            ref, truth = (ref * D.Hc).reshape(shape), (truth * D.Hc).reshape(shape)
            noise = np.abs(ref - truth) / np.maximum(np.abs(truth), 1e-3)
            assert np.isfinite(ref).all() and np.isfinite(noise).all(), (deck, g, name)
            out[f"g{g}_ref_{name}"], out[f"g{g}_noise_{name}"] = ref, noise
            print(deck, "group", g, name, "worst noise", noise.max(), "|ref| from", np.abs(ref).min(), "to", np.abs(ref).max(), flush=True)
        for key in ("tD", "sv", "rD", "col", "tfac"):
            out[f"g{g}_{key}"] = grp[key]
        out[f"g{g}_k0"] = np.array(grp["k0"], np.int32)
    s, ds = superpose(wells, groups, h, dh, len(times), len(loc), len(z), D.Hc)
    assert np.isfinite(s).all() and np.isfinite(ds).all()
    out["s_ref"], out["ds_ref"] = s, ds
    path = path or os.path.join(ROOT, "tests", "golden", f"field_{deck}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(groups), "groups,", sum(v.size for v in h), "oracle values")


if __name__ == "__main__":
    for deck in (sys.argv[1:] or list(DECKS)):
        generate(deck)
