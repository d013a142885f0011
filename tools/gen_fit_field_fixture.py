"""Writes the fixtures of tests/test_gpu_fit_field.py and tests/test_fit_field_host.py:
tests/golden/fit_field_<problem>.npz.  CPU only (the oracle and its binary128 build, tests/oracle_lib.py).  On 8 cores theis
takes half a minute and neuman74 twelve minutes: the binary128 build of 220 values x 10 rows dominates, and the 66 times of A
towards two wells that both start at t = 0 are what the two-block branch needs.

    python tools/gen_fit_field_fixture.py [neuman74 | theis]

The field (the smallest that reaches every branch of ucf_fit_create_field), coordinates in the deck's own length scale:
  P0  at the origin, q = 1, t0 = 0;
  P1  q = 0.6, t0 = 20: later observations see it, earlier ones do not;
  P2  the constant-head image of P0 in the line x = c, taken from ucf_field_images: q = -1, so terms cancel.
  A   one depth, 66 times: its virtual wells towards P0 and P2 have two blocks of 64 points each, the second one padded, and
      the one towards P1 fewer times than those;
  B   three depths, observed as its screen average at 6 times and once more, at one of those times, at its middle depth
      alone: a shared (virtual well, time) point and mixed iz;
  C   one depth, 4 times, all before t0 = 20: no term from P1;
  D   three depths, never named by an observation: it has virtual wells but no values.
Stored:
  wells        pump [npump, 4] rows of (x, y, q, t0); well_x, well_y, well_nz, well_z as ucf_fit_create_field takes them;
  observations t, well, iz in a shuffled order;
  terms        formed HERE in numpy, by the rules of include/ucf.h (tests hold the library to them): virt_well, virt_r,
               term_first, term_pump, term_virt, term_t;  e_first / e_count: the entries of the value list below that term k
               reads (one, or all depths of its well);
  values       per (set, row, entry): the ORACLE's h x Hc and its distance from the binary128 build, |oracle - binary128| /
               max(|binary128|, 1e-3); entries run virtual well by virtual well, time by time (ascending), depth by depth
               (e_virt, e_time, e_depth); rows as in sim_all of ucf_fit_evaluate (base, parameter j up, parameter j down)
               for the two parameter sets eval_theta and the step eval_dlog.  As in the library, the split vector of a
               parameter set is taken over all term times.  The distance is stored as max(distance, NOISE_FLOOR): gate() of
               tests/test_gpu_fit.py reads max(1e-10, 10 x distance), so nothing below 1e-11 changes a bound, and the floored
               array compresses to almost nothing.  Every stored value is asserted finite;
  fitting      obs = the oracle's superposition at theta_star (set 0, row 0): acc = +0.0; acc = acc + q * v over the terms,
               v the dimensionless h or its screen average; acc * Hc.  No noise added; two starts.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden_util import load_deck                   # noqa: E402
from oracle_lib import Oracle                       # noqa: E402
from unconfined_amd import field as ufield          # noqa: E402  (ucf_field_images: host arithmetic, no GPU)
from unconfined_amd import fit as ufit              # noqa: E402  (ucf_fit_perturb: host arithmetic, no GPU)

T_A = 10.0 ** np.linspace(-1, 3.5, 66)
T_B = 10.0 ** np.linspace(0, 3.5, 6)
T_C = np.array([0.5, 2.0, 6.0, 15.0])
B_EXTRA = 3            # the time of B that is observed at the middle depth as well
T0_P1 = 20.0
NOISE_FLOOR = 1.0e-11
PROBLEMS = {
    "neuman74": dict(deck="neuman74_partpen", free=["Kr", "Sy"], seed=74, p1=(-60.0, 90.0), line=100.0,
                     obs_wells=[(30.0, 10.0, [50.0]), (60.0, -50.0, [105.0, 123.0, 141.0]), (-40.0, 70.0, [150.0]),
                                (80.0, -20.0, [20.0, 80.0, 155.0])]),
    # Theis has no shared launch (and reads neither kappa nor Sy): plan by plan, virtual well by virtual well
    "theis": dict(deck="c1_theis", free=["Kr", "Ss"], seed=1, p1=(-2.0, 3.0), line=3.3,
                  obs_wells=[(1.0, 0.3, [1.0]), (2.0, -1.7, [3.0, 5.0, 7.0]), (-1.3, 2.3, [9.0]), (2.7, -0.7, [0.5, 5.0, 9.5])]),
}
EVAL_FACTORS = np.array([[1.0, 1.0], [1.3, 0.9]])
EVAL_DLOG = 1.0e-3
START_FACTORS = np.array([[0.5, 2.0], [1.8, 0.6]])


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


def terms_of(pump, well_x, well_y, t, well):
    """the layout rules of ucf_fit_create_field, every operation a numpy float64 operation of its own"""
    virt_well, virt_r, vmap = [], [], {}
    for w in range(len(well_x)):
        dx, dy = well_x[w] - pump[:, 0], well_y[w] - pump[:, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        for r in np.unique(dist):                       # ascending
            for j in np.flatnonzero(dist == r):
                vmap[(w, int(j))] = len(virt_well)
            virt_well.append(w); virt_r.append(float(r))
    first, tp, tv, tt = [0], [], [], []
    for i in range(len(t)):
        for j in range(len(pump)):
            if t[i] > pump[j, 3]:
                tp.append(j); tv.append(vmap[(int(well[i]), j)]); tt.append(t[i] - pump[j, 3])
        first.append(len(tp))
    return (np.array(virt_well, np.int32), np.array(virt_r), np.array(first, np.int32), np.array(tp, np.int32), np.array(tv, np.int32),
            np.array(tt))


def generate(key):
    pr = PROBLEMS[key]
    dk, _, P0 = load_deck(pr["deck"])
    O, Q = Oracle(), Oracle(quad=True)
    image = ufield.images([(0.0, 0.0, 1.0, 0.0)], line=(1.0, 0.0, pr["line"]), kind="constant_head")[1]
    pump = np.array([(0.0, 0.0, 1.0, 0.0), pr["p1"] + (0.6, T0_P1), tuple(image)])
    assert pump[2, 2] == -1.0 and pump[2, 3] == 0.0
    obs_wells = pr["obs_wells"]
    well_x, well_y = np.array([w[0] for w in obs_wells]), np.array([w[1] for w in obs_wells])
    depths = [np.array(w[2], float) for w in obs_wells]
    # observations, then shuffled once
    t = np.concatenate([T_A, T_B, T_B[B_EXTRA:B_EXTRA + 1], T_C])
    well = np.concatenate([np.full(len(T_A), 0), np.full(len(T_B) + 1, 1), np.full(len(T_C), 2)]).astype(np.int32)
    iz = np.concatenate([np.zeros(len(T_A)), np.full(len(T_B), -1), [1], np.zeros(len(T_C))]).astype(np.int32)
    perm = np.random.default_rng(pr["seed"]).permutation(len(t))
    t, well, iz = t[perm], well[perm], iz[perm]
    virt_well, virt_r, term_first, term_pump, term_virt, term_t = terms_of(pump, well_x, well_y, t, well)
    assert (T_C < T0_P1).all() and not ((well[np.repeat(np.arange(len(t)), np.diff(term_first))] == 2) & (term_pump == 1)).any()
    # the value list: per used virtual well its distinct term times, ascending, every depth of the well
    times = {int(v): np.unique(term_t[term_virt == v]) for v in np.unique(term_virt)}
    e_virt, e_time, e_depth, first = [], [], [], {}
    for v, tv in times.items():
        for q in range(len(tv)):
            first[(v, q)] = len(e_virt)
            for j in range(len(depths[virt_well[v]])):
                e_virt.append(v); e_time.append(q); e_depth.append(j)
    nterm = len(term_t)
    e_first, e_count = np.zeros(nterm, np.int32), np.zeros(nterm, np.int32)
    for i in range(len(t)):
        for k in range(term_first[i], term_first[i + 1]):
            v = int(term_virt[k])
            q = int(np.searchsorted(times[v], term_t[k]))
            assert times[v][q] == term_t[k]
            e_first[k] = first[(v, q)] + (iz[i] if iz[i] >= 0 else 0)
            e_count[k] = 1 if iz[i] >= 0 else len(depths[virt_well[v]])
    all_t = np.concatenate([times[v] for v in times])

    def values(theta, oracle, threads):
        """dimensionless h per entry, and Hc"""
        Pp = ufit.perturb(P0, pr["free"], theta)
        D = O.nondim(Pp)
        sv_all = O.split_vector(list(dk.j0s), all_t / D.Tc)
        out, at = [], 0
        for v, tv in times.items():
            zD = depths[virt_well[v]] / D.Lc
            h, _ = oracle.batch(Pp, tv / D.Tc, np.full(len(tv), virt_r[v] / D.Lc), sv_all[at:at + len(tv)], zD, O.zlay(D, zD), threads)
            out.append(h.ravel())
            at += len(tv)
        return np.concatenate(out), D.Hc

    theta_star = np.array([getattr(P0, n) for n in pr["free"]])
    thetas = theta_star * EVAL_FACTORS
    ref = np.zeros((len(thetas), 1 + 2 * len(theta_star), len(e_virt))); noise = np.zeros_like(ref)
    obs = None
    for s, th in enumerate(thetas):
        for k, row in enumerate(rows(th, EVAL_DLOG)):
            h, Hc = values(row, O, 8)
            ref[s, k] = h * Hc
            truth = values(row, Q, 8)[0] * Hc
            noise[s, k] = np.abs(ref[s, k] - truth) / np.maximum(np.abs(truth), 1e-3)
            if s == 0 and k == 0:
                obs = np.zeros(len(t))
                for i in range(len(t)):
                    acc = 0.0
                    for q in range(term_first[i], term_first[i + 1]):
                        acc = acc + pump[term_pump[q], 2] * screen_average(h[e_first[q]:e_first[q] + e_count[q]])
                    obs[i] = acc * Hc
        print(key, "set", s, "worst noise", noise[s].max(), "share above the floor", float((noise[s] > NOISE_FLOOR).mean()), flush=True)
    assert np.isfinite(ref).all() and np.isfinite(noise).all() and np.isfinite(obs).all()
    out = dict(deck=np.array(pr["deck"]), free=np.array(pr["free"]), theta_star=theta_star, pump=pump,
               well_x=well_x, well_y=well_y, well_nz=np.array([len(z) for z in depths], np.int32), well_z=np.concatenate(depths),
               t=t, well=well, iz=iz, virt_well=virt_well, virt_r=virt_r, term_first=term_first, term_pump=term_pump,
               term_virt=term_virt, term_t=term_t, e_first=e_first, e_count=e_count,
               e_virt=np.array(e_virt, np.int32), e_time=np.array(e_time, np.int32), e_depth=np.array(e_depth, np.int32),
               eval_theta=thetas, eval_dlog=np.array(EVAL_DLOG), ref=ref, noise=np.maximum(noise, NOISE_FLOOR), obs=obs,
               starts=theta_star * START_FACTORS)
    path = os.path.join(ROOT, "tests", "golden", f"fit_field_{key}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(t), "observations,", nterm, "terms,", len(e_virt), "values per row")


if __name__ == "__main__":
    for key in (sys.argv[1:] or list(PROBLEMS)):
        generate(key)
