"""Writes the fixtures of tests/test_gpu_fit_network.py and tests/test_fit_network_host.py:
tests/golden/fit_network_<problem>.npz.  CPU only (the oracle and its binary128 build, tests/oracle_lib.py); about a minute.

    python tools/gen_fit_network_fixture.py [neuman74 | theis]

The network (the smallest that reaches every branch of ucf_fit_create_network):
  A   5 times, one depth below the screen bottom (layer 1), the LARGEST radius of its group;
  B   70 times, one depth above the screen top (layer 3): two blocks of 64 points, the second one padded;
  C   9 times, three depths spanning the screen, observed as their screen average, and once more at one of those times
      at its middle depth alone: a shared (well, time) point and mixed iz;
  D   three depths, never named by an observation: never launched, so it has no values here (t_D is what a dense
      evaluation of the network would still have to visit).
Stored:
  wells        well_r, well_nz, well_z as ucf_fit_create_network takes them;
  observations t, well, iz in a shuffled order, e_first / e_count: the entries of the value list below that observation i
               reads (one, or all depths of its well);
  values       per (set, row, entry): the ORACLE's dimensionless-to-dimensional drawdown h x Hc and its distance from the
               binary128 build, |oracle - binary128| / max(|binary128|, 1e-3); entries run well by well, time by time
               (ascending), depth by depth (e_well, e_time, e_depth); rows as in sim_all of ucf_fit_evaluate (base,
               parameter j up, parameter j down) for the two parameter sets eval_theta and the step eval_dlog.  As in the
               library, the split vector of a parameter set is taken over all observed times of the network.
               Every stored value is asserted finite;
  fitting      obs = the oracle at theta_star (set 0, row 0) through the screen-average rule, no noise added; two starts.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_deck          # noqa: E402
from oracle_lib import Oracle              # noqa: E402
from unconfined_amd import fit as ufit     # noqa: E402  (ucf_fit_perturb: host arithmetic, no GPU)

T_A = np.array([0.3, 4.0, 50.0, 600.0, 7000.0])
T_B = 10.0 ** np.linspace(-1, 4, 70)
T_C = 10.0 ** np.linspace(-0.5, 3.5, 9)
T_D = np.array([1.0, 10.0, 100.0])
PROBLEMS = {
    "neuman74": dict(deck="neuman74_partpen", free=["Kr", "Sy"], seed=74,
                     wells=[(300.0, [50.0]), (30.0, [150.0]), (85.1, [105.0, 123.0, 141.0]), (150.0, [20.0, 80.0, 155.0])]),
    # Theis has no shared launch (and reads neither kappa nor Sy): plan by plan, well by well
    "theis": dict(deck="c1_theis", free=["Kr", "Ss"], seed=1,
                  wells=[(8.0, [1.0]), (0.5, [9.0]), (2.0, [3.0, 5.0, 7.0]), (4.0, [0.5, 5.0, 9.5])]),
}
EVAL_FACTORS = np.array([[1.0, 1.0], [1.3, 0.9]])
EVAL_DLOG = 1.0e-3
START_FACTORS = np.array([[0.5, 2.0], [1.8, 0.6]])
C_EXTRA = 4            # the time of C that is observed at the middle depth as well


def screen_average(v):
    """ucf_screen_average for one point (driver.f90:234-243)"""
    n = len(v)
    if n == 1:
        return v[0]
    s = v[1]
    for j in range(2, n):
        s = s + v[j]
    return ((v[0] + 2.0 * s) + v[n - 1]) / (2 * n)


def rows(theta, dlog):
    out = [np.array(theta, float)]
    for j in range(len(theta)):
        for f in (np.exp(dlog), np.exp(-dlog)):
            th = np.array(theta, float); th[j] = th[j] * f
            out.append(th)
    return out


def generate(key):
    pr = PROBLEMS[key]
    dk, _, P0 = load_deck(pr["deck"])
    O, Q = Oracle(), Oracle(quad=True)
    wells = pr["wells"]
    times = [T_A, T_B, T_C]                       # of the wells that are observed: A, B, C
    # observations, then shuffled once
    t = np.concatenate([T_A, T_B, T_C, T_C[C_EXTRA:C_EXTRA + 1]])
    well = np.concatenate([np.full(len(T_A), 0), np.full(len(T_B), 1), np.full(len(T_C) + 1, 2)]).astype(np.int32)
    iz = np.concatenate([np.zeros(len(T_A)), np.zeros(len(T_B)), np.full(len(T_C), -1), [1]]).astype(np.int32)
    perm = np.random.default_rng(pr["seed"]).permutation(len(t))
    t, well, iz = t[perm], well[perm], iz[perm]
    # the value list
    e_well, e_time, e_depth, first = [], [], [], {}
    for w, tw in enumerate(times):
        for q in range(len(tw)):
            first[(w, q)] = len(e_well)
            for j in range(len(wells[w][1])):
                e_well.append(w); e_time.append(q); e_depth.append(j)
    e_first = np.zeros(len(t), np.int32); e_count = np.zeros(len(t), np.int32)
    for i in range(len(t)):
        q = int(np.searchsorted(times[well[i]], t[i]))
        assert times[well[i]][q] == t[i]
        e_first[i] = first[(int(well[i]), q)] + (iz[i] if iz[i] >= 0 else 0)
        e_count[i] = 1 if iz[i] >= 0 else len(wells[well[i]][1])
    all_t = np.concatenate(times)

    def values(theta, oracle, threads):
        Pp = ufit.perturb(P0, pr["free"], theta)
        D = O.nondim(Pp)
        sv_all = O.split_vector(list(dk.j0s), all_t / D.Tc)
        out, at = [], 0
        for w, tw in enumerate(times):
            zD = np.array(wells[w][1]) / D.Lc
            h, _ = oracle.batch(Pp, tw / D.Tc, np.full(len(tw), wells[w][0] / D.Lc), sv_all[at:at + len(tw)], zD, O.zlay(D, zD), threads)
            out.append((h * D.Hc).ravel())
            at += len(tw)
        return np.concatenate(out)

    theta_star = np.array([getattr(P0, n) for n in pr["free"]])
    thetas = theta_star * EVAL_FACTORS
    ref = np.zeros((len(thetas), 1 + 2 * len(theta_star), len(e_well))); noise = np.zeros_like(ref)
    for s, th in enumerate(thetas):
        for k, row in enumerate(rows(th, EVAL_DLOG)):
            ref[s, k] = values(row, O, 8)
            truth = values(row, Q, 16)
            noise[s, k] = np.abs(ref[s, k] - truth) / np.maximum(np.abs(truth), 1e-3)
        print(key, "set", s, "worst noise", noise[s].max(), flush=True)
    assert np.isfinite(ref).all() and np.isfinite(noise).all()
    obs = np.array([screen_average(ref[0, 0, e_first[i]:e_first[i] + e_count[i]]) for i in range(len(t))])
    assert np.isfinite(obs).all()
    out = dict(deck=np.array(pr["deck"]), free=np.array(pr["free"]), theta_star=theta_star,
               well_r=np.array([r for r, _ in wells]), well_nz=np.array([len(z) for _, z in wells], np.int32),
               well_z=np.concatenate([np.array(z, float) for _, z in wells]), t_D=T_D,
               t=t, well=well, iz=iz, e_first=e_first, e_count=e_count,
               e_well=np.array(e_well, np.int32), e_time=np.array(e_time, np.int32), e_depth=np.array(e_depth, np.int32),
               eval_theta=thetas, eval_dlog=np.array(EVAL_DLOG), ref=ref, noise=noise, obs=obs,
               starts=theta_star * START_FACTORS)
    path = os.path.join(ROOT, "tests", "golden", f"fit_network_{key}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(t), "observations,", len(e_well), "values per row")


if __name__ == "__main__":
    for key in (sys.argv[1:] or list(PROBLEMS)):
        generate(key)
