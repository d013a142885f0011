"""Writes the fixtures of tests/test_gpu_field_forecast.py: tests/golden/field_forecast_<deck>.npz.  CPU only, in the manner
of tools/gen_field_fixture.py, whose field (WELLS, LOCATIONS, DECKS; of its TIMES those that serve) and `superpose` it reuses:
the oracle and its binary128 build at every parameter set that ucf_field_forecast evaluates; a few minutes.

    python tools/gen_field_forecast_fixture.py [neuman74_partpen | c1_theis]

The forecasts:
  neuman74_partpen   free = Kr, kappa, Ss, Sy (9 parameter sets);
  c1_theis           free = Kr, Ss (5 parameter sets);
  theta              the deck's own values, dlog = 1e-3: the sets of ucf_field_forecast_sets, host arithmetic that
                     tests/test_field_forecast_host.py checks against numpy;
  cov                L L' with the fixed lower-triangular L below (entries of order 0.05: variances of order 0.05^2 in ln theta),
                     symmetric by construction and positive definite because the diagonal of L is positive;
  times              six per deck, two of them before the later start (TIMES below), picked by the procedure of
                     tools/gen_field_fixture.py: candidate times from 0.3 to 3000 are evaluated by the oracle at EVERY
                     parameter set of the forecast, the unchanged grid path is run at them in both flavours, and a time is
                     kept only if every launched value (either group, h and dh, every set) meets its per-value gate b.  No gate
                     is widened; the misses are the grid path's behaviour at those times, whatever is summed.  With the
                     perturbed sets more times miss than at the deck's parameters alone:
                       neuman74_partpen   29 candidates; 0.3, 0.7, 0.8, 1, 4, 6, 7, 10, 15, 20 and 30 have a value that misses
                                          (7, of the field fixture, at the set with Kr moved down: 5.0 b in the faithful
                                          flavour); 0.4, 0.5, 1.5, 2, 2.5, 3, 3.5, 8 and every candidate from 40 to 3000 meet
                                          it.  Kept: the field fixture's times with 40 in the place of 7.
                       c1_theis           35 candidates; 2.5, 15, 20 and every candidate from 40 to 3000 miss in at least one
                                          flavour (the fast flavour's dh at late time, up to 8.2 b at 700), all others from 0.3
                                          to 12 and 30 meet it.  Kept: 0.5 and 2 of the field fixture, then 6, 10, 12 and 30.
Stored:
  geometry   deck, wells, locations, times, z as in field_<deck>.npz;  free (names), theta, dlog, cov;
  per set k and group g   k<k>_g<g>_ref_h, _ref_dh [nt_g][nr_g][nz]: the oracle's h x Hc and dh x Hc of set k at every launched
             (tD, rD, z) of ucf_field_group_from_params(sets[k]);  k<k>_g<g>_noise_h, _noise_dh: its distance from the
             binary128 build, |oracle - binary128| / max(|binary128|, 1e-3) -- what field_<deck>.npz holds for the base set;
  reference  s_all_ref, ds_all_ref [1 + 2 npar][nt][nloc][nz]: the oracle's values superposed by the arithmetic of include/ucf.h;
  bounds     bound_s, bound_ds [1 + 2 npar][nt][nloc][nz] = sum_j |q_j| tfac b_j of tests/test_gpu_field.py with
             b = max(1e-10, 10 noise) max(|ref|, 1e-3), its gate (tfac = 1 for s).
Every stored value is asserted finite.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from golden_util import load_deck                                            # noqa: E402
from oracle_lib import Oracle                                                # noqa: E402
from gen_field_fixture import DECKS, LOCATIONS, WELLS, superpose             # noqa: E402
from unconfined_amd.field import WellField, forecast_sets                    # noqa: E402

DLOG = 1e-3
FREE = {"neuman74_partpen": ["Kr", "kappa", "Ss", "Sy"], "c1_theis": ["Kr", "Ss"]}
TIMES = {"neuman74_partpen": np.array([0.5, 2.0, 40.0, 150.0, 1000.0, 3000.0]), "c1_theis": np.array([0.5, 2.0, 6.0, 10.0, 12.0, 30.0])}
# cov = L L'
L4 = np.array([[0.05, 0.0, 0.0, 0.0],
               [0.02, 0.06, 0.0, 0.0],
               [-0.03, 0.01, 0.04, 0.0],
               [0.01, -0.02, 0.03, 0.07]])


def gate(ref, noise):
    """the per-value gate of tests/test_gpu_field.py"""
    return np.maximum(1e-10, 10.0 * noise) * np.maximum(np.abs(ref), 1e-3)


def covariance(npar):
    L = L4[:npar, :npar]
    cov = L @ L.T
    cov = 0.5 * (cov + cov.T)                          # bitwise symmetric
    assert (cov == cov.T).all() and (np.linalg.eigvalsh(cov) > 0.0).all()
    return cov


def generate(deck, times=None, path=None):
    times = TIMES[deck] if times is None else times
    cfg = DECKS[deck]
    dk, _, P = load_deck(deck)
    free = FREE[deck]
    theta = np.array([getattr(P, n) for n in free])
    sets = forecast_sets(P, free, theta, DLOG)
    O, Q = Oracle(), Oracle(quad=True)
    wells = WELLS.copy(); wells[:, :2] *= cfg["unit"]
    loc = LOCATIONS * cfg["unit"]
    z = np.array(cfg["z"])
    nt, nloc, nz = len(times), len(loc), len(z)
    field = WellField(wells, loc, times)
    absw = wells.copy(); absw[:, 2] = np.abs(wells[:, 2])
    out = dict(deck=np.array(deck), wells=wells, locations=loc, times=np.asarray(times, float), z=z, free=np.array(free), theta=theta,
               dlog=np.array(DLOG), cov=covariance(len(free)))
    s_all, ds_all, bound_s, bound_ds = [], [], [], []
    for k, Pk in enumerate(sets):
        D = O.nondim(Pk)
        zD = z / D.Lc
        zl = O.zlay(D, zD)
        groups = field.groups(Pk)
        h, dh, b_h, b_dh = [], [], [], []
        for g, grp in enumerate(groups):
            nt_g, nr_g = len(grp["tD"]), len(grp["rD"])
            assert (grp["sv"] == O.split_vector(list(dk.j0s), grp["tD"])).all()
            TT, RR = np.meshgrid(grp["tD"], grp["rD"], indexing="ij")
            sv = np.repeat(grp["sv"], nr_g)
            ho, dho = O.batch(Pk, TT.ravel(), RR.ravel(), sv, zD, zl, 8)
            ht, dht = Q.batch(Pk, TT.ravel(), RR.ravel(), sv, zD, zl, 16)
            shape = (nt_g, nr_g, nz)
            h.append(ho.reshape(shape)); dh.append(dho.reshape(shape))
            for name, ref, truth, keep in (("h", ho, ht, b_h), ("dh", dho, dht, b_dh)):
                ref, truth = (ref * D.Hc).reshape(shape), (truth * D.Hc).reshape(shape)
                noise = np.abs(ref - truth) / np.maximum(np.abs(truth), 1e-3)
                assert np.isfinite(ref).all() and np.isfinite(noise).all(), (deck, k, g, name)
                out[f"k{k}_g{g}_ref_{name}"], out[f"k{k}_g{g}_noise_{name}"] = ref, noise
                keep.append(gate(ref, noise))
                print(deck, "set", k, "group", g, name, "worst noise", noise.max(), flush=True)
        s, ds = superpose(wells, groups, h, dh, nt, nloc, nz, D.Hc)
        one = [dict(g, tfac=np.ones_like(g["tfac"])) for g in groups]
        bs, _ = superpose(absw, one, b_h, b_h, nt, nloc, nz, 1.0)
        _, bds = superpose(absw, groups, b_dh, b_dh, nt, nloc, nz, 1.0)
        for v in (s, ds, bs, bds):
            assert np.isfinite(v).all(), (deck, k)
        s_all.append(s); ds_all.append(ds); bound_s.append(bs); bound_ds.append(bds)
    out["s_all_ref"], out["ds_all_ref"] = np.stack(s_all), np.stack(ds_all)
    out["bound_s"], out["bound_ds"] = np.stack(bound_s), np.stack(bound_ds)
    path = path or os.path.join(ROOT, "tests", "golden", f"field_forecast_{deck}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(sets), "parameter sets")


if __name__ == "__main__":
    for deck in (sys.argv[1:] or list(FREE)):
        generate(deck)
