"""Writes the fixtures of tests/test_gpu_fit_deriv.py: tests/golden/fit_deriv_<problem>.npz for the problems neuman74, theis,
network and field.  CPU only (the oracle and its binary128 build, tests/oracle_lib.py); about ten minutes on 8 cores.

    python tools/gen_fit_deriv_fixture.py [neuman74 | theis | network | field]

neuman74, theis: the problems and the observation layout of tools/gen_fit_fixture.py (22 observations), with the log-time
derivative t ds/dt beside every drawdown:
  obs, dobs      the ORACLE's dimensional h x Hc and dh x Hc at the deck's own parameters theta_star;
  noise, dnoise  per observation |oracle - binary128| / max(|binary128|, 1e-3) of either;
  eval_*         the three parameter sets of gen_fit_fixture.py at dlog = 1e-3: the oracle's h and dh (eval_ref, eval_dref) and
                 their noise of the base plan and of every plan with one parameter moved by e^{+-dlog}, rows as in sim_all;
  starts         the first 4 starts of fit_synthetic_<problem>.npz;
  lm_*           Levenberg-Marquardt as ucf_fit_lm runs it, in numpy ON THE ORACLE ALONE from those starts, once jointly (unit
                 weights on both curves) and once on the derivative alone (weight 0 on every h): all must converge (asserted),
                 cond(A) at theta_star must be < 1e8 (asserted); the iteration counts are stored;
  hfin_*         (neuman74) a point of the overflow regime where the oracle's h is finite under every plan of the evaluation
                 sets and its dh is not, if a scan around the NaN point of tests/test_gpu_fit.py finds one (hfin_found).
network: deck neuman74_partpen, free = Kr, Sy, the wells A, B, C of tools/gen_fit_network_fixture.py with 5, 8 and 6 times; C
  is observed as its screen average and once more at its middle depth alone.  Values per (set, row, entry) as there, for h
  (ref, noise) and dh (dref, dnoise); obs, dobs through the screen-average rule at theta_star.
field: the same deck and parameters, the pumping wells P0, P1 and the constant-head image of P0 of
  tools/gen_fit_field_fixture.py, its observation wells A (12 times) and B (screen average at 6 times, once its middle depth).
  Terms and entries as there; tfac per term = t / term_t; ref, noise, dref, dnoise per entry; obs and dobs are the
  superpositions acc = acc + q v and acc = acc + q (tfac v) at theta_star, times Hc.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from golden_util import GOLD, load_deck                                                   # noqa: E402
from oracle_lib import Oracle                                                             # noqa: E402
from unconfined_amd import field as ufield                                                # noqa: E402  (host arithmetic, no GPU)
from unconfined_amd import fit as ufit                                                    # noqa: E402  (host arithmetic, no GPU)
import gen_fit_fixture as plain                                                           # noqa: E402
from gen_fit_field_fixture import T0_P1, terms_of                                         # noqa: E402
from gen_fit_network_fixture import rows, screen_average                                  # noqa: E402

LM = plain.LM
DLOG = 1.0e-3
NSTARTS = 4
THREADS = 8
NAN_T, NAN_R = 3.1e-4, 1.6                  # tests/test_gpu_fit.py: the oracle's h is NaN there
NET = dict(deck="neuman74_partpen", free=["Kr", "Sy"], seed=74,
           wells=[(300.0, [50.0]), (30.0, [150.0]), (85.1, [105.0, 123.0, 141.0])],
           times=[np.array([0.3, 4.0, 50.0, 600.0, 7000.0]), 10.0 ** np.linspace(-1, 4, 8), 10.0 ** np.linspace(-0.5, 3.5, 6)], extra=3)
FLD = dict(deck="neuman74_partpen", free=["Kr", "Sy"], seed=74, p1=(-60.0, 90.0), line=100.0,
           obs_wells=[(30.0, 10.0, [50.0]), (60.0, -50.0, [105.0, 123.0, 141.0])],
           times=[10.0 ** np.linspace(-1, 3.5, 12), 10.0 ** np.linspace(0, 3.5, 6)], extra=3)
EVAL2 = np.array([[1.0, 1.0], [1.3, 0.9]])


def rel(a, truth):
    return np.abs(a - truth) / np.maximum(np.abs(truth), 1e-3)


class Problem(plain.Problem):
    def sim2(self, theta, oracle=None, threads=THREADS):
        """dimensional drawdown and log-time derivative of every observation at the parameters theta"""
        O = oracle or self.O
        P = ufit.perturb(self.P0, self.free, theta)
        D = self.O.nondim(P)
        tD, rD, zD = self.t / D.Tc, self.r / D.Lc, self.z / D.Lc
        sv = self.O.split_vector(list(self.dk.j0s), tD)
        h, dh = O.batch(P, tD, rD, sv, zD, self.O.zlay(D, zD), threads)
        i = np.arange(len(self.t))
        return h[i, self.iz] * D.Hc, dh[i, self.iz] * D.Hc

    def with_noise2(self, theta):
        h, dh = self.sim2(theta)
        th, tdh = self.sim2(theta, self.Q, threads=16)
        return h, rel(h, th), dh, rel(dh, tdh)

    def normal2(self, theta, obs, dobs, w, wd):
        """phi, g, A of the joint problem: the rows of h (weights w) stacked on the rows of dh (weights wd)"""
        s = [self.sim2(th) for th in self.rows(theta, LM["dlog"])]
        P = len(theta)
        J = np.stack([np.concatenate([w * (s[1 + 2 * j][0] - s[2 + 2 * j][0]), wd * (s[1 + 2 * j][1] - s[2 + 2 * j][1])]) / (2 * LM["dlog"])
                      for j in range(P)], axis=1)
        res = np.concatenate([w * (obs - s[0][0]), wd * (dobs - s[0][1])])
        return float(res @ res), J.T @ res, J.T @ J

    def phi2(self, theta, obs, dobs, w, wd):
        h, dh = self.sim2(theta)
        res = np.concatenate([w * (obs - h), wd * (dobs - dh)])
        return float(res @ res)

    def lm2(self, theta0, obs, dobs, w, wd, o):
        """ucf_fit_lm for one start; returns theta, phi, iterations, converged"""
        x = np.log(theta0); lam = o["lambda0"]; it = 0
        phi, g, A = self.normal2(np.exp(x), obs, dobs, w, wd)
        while True:
            step = ufit.solve_step(A, g, lam)
            ph = self.phi2(np.exp(x + step), obs, dobs, w, wd)
            it += 1
            done = np.max(np.abs(step)) <= o["tol_step"]
            if np.isfinite(ph) and ph <= phi:
                if phi - ph <= o["tol_phi"] * phi:
                    done = True
                x = x + step; lam *= o["lambda_down"]
                if not done and it < o["max_iter"]:
                    phi, g, A = self.normal2(np.exp(x), obs, dobs, w, wd)
                phi = ph
            else:
                lam *= o["lambda_up"]
            if done:
                return np.exp(x), phi, it, True
            if it >= o["max_iter"]:
                return np.exp(x), phi, it, False


def find_h_finite_dh_not(pb, thetas):
    """a point near the NaN point of tests/test_gpu_fit.py where, under every plan of the evaluation sets, the oracle's h
    is finite and its dh is not; None if the scan finds none"""
    plans = [row for th in thetas for row in pb.rows(th, DLOG)]
    for fr in (1.0, 1.5, 2.0, 3.0, 5.0, 8.0):
        for ft in 10.0 ** np.linspace(-1.0, 2.0, 13):
            t, r = NAN_T * ft, NAN_R * fr
            good = True
            for row in plans:
                P = ufit.perturb(pb.P0, pb.free, row)
                D = pb.O.nondim(P)
                zD = pb.z / D.Lc
                h, dh = pb.O.batch(P, np.array([t / D.Tc]), np.array([r / D.Lc]), np.array([1], np.int32), zD, pb.O.zlay(D, zD))
                good = good and np.isfinite(h[0, 0]) and not np.isfinite(dh[0, 0])
                if not good:
                    break
            if good:
                return t, r
    return None


def generate_plain(key):
    pb = Problem(key)
    P = len(pb.free)
    n = len(pb.t)
    out = dict(t=pb.t, r=pb.r, z=pb.z, iz=pb.iz, free=np.array(pb.free), theta_star=pb.theta_star, deck=np.array(plain.PROBLEMS[key]["deck"]))
    out["obs"], out["noise"], out["dobs"], out["dnoise"] = pb.with_noise2(pb.theta_star)
    assert np.isfinite(out["obs"]).all() and np.isfinite(out["dobs"]).all()
    print(key, "worst noise of h", out["noise"].max(), "of dh", out["dnoise"].max(), flush=True)
    thetas = pb.theta_star * plain.EVAL_FACTORS[:, :P]
    ref = np.zeros((len(thetas), 1 + 2 * P, n)); noise = np.zeros_like(ref); dref = np.zeros_like(ref); dnoise = np.zeros_like(ref)
    for s, th in enumerate(thetas):
        for k, row in enumerate(pb.rows(th, DLOG)):
            ref[s, k], noise[s, k], dref[s, k], dnoise[s, k] = pb.with_noise2(row)
        print(key, "evaluation set", s, "worst noise of h", noise[s].max(), "of dh", dnoise[s].max(), flush=True)
    assert np.isfinite(ref).all() and np.isfinite(dref).all()
    out.update(eval_theta=thetas, eval_dlog=np.array(DLOG), eval_ref=ref, eval_noise=noise, eval_dref=dref, eval_dnoise=dnoise)
    starts = np.load(os.path.join(GOLD, f"fit_synthetic_{key}.npz"))["starts"][:NSTARTS]
    one, zero = np.ones(n), np.zeros(n)
    for name, w in (("joint", one), ("deriv", zero)):
        _, _, A = pb.normal2(pb.theta_star, out["obs"], out["dobs"], w, one)
        cond = float(np.linalg.cond(A))
        assert cond < 1e8, (key, name, cond)
        iters = []
        for s in range(NSTARTS):
            th, phi, it, ok = pb.lm2(starts[s], out["obs"], out["dobs"], w, one, LM)
            print(key, name, "start", s, "iters", it, "phi", phi, "ln(theta/theta_star)", np.log(th / pb.theta_star), flush=True)
            assert ok, (key, name, s, "the oracle alone does not converge from this start")
            assert np.max(np.abs(np.log(th / pb.theta_star))) < 1e-4, (key, name, s, th)
            iters.append(it)
        out[f"cond_{name}"] = np.array(cond)
        out[f"lm_iters_{name}"] = np.array(iters)
    out.update(starts=starts, lm_options=np.array([LM[k] for k in ("max_iter", "dlog", "lambda0", "lambda_up", "lambda_down", "tol_step", "tol_phi")]))
    if key == "neuman74":
        found = find_h_finite_dh_not(pb, thetas)
        print(key, "h finite, dh not:", found, flush=True)
        out.update(hfin_found=np.array(found is not None), hfin_t=np.array(found[0] if found else np.nan),
                   hfin_r=np.array(found[1] if found else np.nan))
    save(key, out)


def entry_values(P0, dk, free, theta, all_t, groups, O, oracle, threads):
    """dimensionless h and dh per entry -- group by group (radius, depths, times), time by time, depth by depth -- and Hc"""
    Pp = ufit.perturb(P0, free, theta)
    D = O.nondim(Pp)
    sv_all = O.split_vector(list(dk.j0s), all_t / D.Tc)
    hs, ds, at = [], [], 0
    for r, z, tv in groups:
        zD = np.array(z, float) / D.Lc
        h, dh = oracle.batch(Pp, tv / D.Tc, np.full(len(tv), r / D.Lc), sv_all[at:at + len(tv)], zD, O.zlay(D, zD), threads)
        hs.append(h.ravel()); ds.append(dh.ravel())
        at += len(tv)
    return np.concatenate(hs), np.concatenate(ds), D.Hc


def evaluate_entries(P0, dk, free, all_t, groups, nentries):
    """ref, noise, dref, dnoise [sets][rows][entries] (dimensional), and the dimensionless h, dh and Hc at theta_star"""
    O, Q = Oracle(), Oracle(quad=True)
    theta_star = np.array([getattr(P0, n) for n in free])
    thetas = theta_star * EVAL2
    shape = (len(thetas), 1 + 2 * len(free), nentries)
    ref, noise, dref, dnoise = (np.zeros(shape) for _ in range(4))
    star = None
    for s, th in enumerate(thetas):
        for k, row in enumerate(rows(th, DLOG)):
            h, dh, Hc = entry_values(P0, dk, free, row, all_t, groups, O, O, THREADS)
            th_, tdh, _ = entry_values(P0, dk, free, row, all_t, groups, O, Q, 16)
            ref[s, k], dref[s, k] = h * Hc, dh * Hc
            noise[s, k], dnoise[s, k] = rel(h * Hc, th_ * Hc), rel(dh * Hc, tdh * Hc)
            if s == 0 and k == 0:
                star = (h, dh, Hc)
        print("set", s, "worst noise of h", noise[s].max(), "of dh", dnoise[s].max(), flush=True)
    assert all(np.isfinite(a).all() for a in (ref, noise, dref, dnoise))
    return theta_star, thetas, ref, noise, dref, dnoise, star


def generate_network():
    pr = NET
    dk, _, P0 = load_deck(pr["deck"])
    wells, times = pr["wells"], pr["times"]
    t = np.concatenate(times + [times[2][pr["extra"]:pr["extra"] + 1]])
    well = np.concatenate([np.full(len(tw), w) for w, tw in enumerate(times)] + [[2]]).astype(np.int32)
    iz = np.concatenate([np.zeros(len(times[0])), np.zeros(len(times[1])), np.full(len(times[2]), -1), [1]]).astype(np.int32)
    perm = np.random.default_rng(pr["seed"]).permutation(len(t))
    t, well, iz = t[perm], well[perm], iz[perm]
    first, n = {}, 0
    for w, tw in enumerate(times):
        for q in range(len(tw)):
            first[(w, q)] = n
            n += len(wells[w][1])
    e_first = np.zeros(len(t), np.int32); e_count = np.zeros(len(t), np.int32)
    for i in range(len(t)):
        q = int(np.searchsorted(times[well[i]], t[i]))
        assert times[well[i]][q] == t[i]
        e_first[i] = first[(int(well[i]), q)] + (iz[i] if iz[i] >= 0 else 0)
        e_count[i] = 1 if iz[i] >= 0 else len(wells[well[i]][1])
    groups = [(wells[w][0], wells[w][1], times[w]) for w in range(len(wells))]
    theta_star, thetas, ref, noise, dref, dnoise, _ = evaluate_entries(P0, dk, pr["free"], np.concatenate(times), groups, n)
    obs = np.array([screen_average(ref[0, 0, a:a + c]) for a, c in zip(e_first, e_count)])
    dobs = np.array([screen_average(dref[0, 0, a:a + c]) for a, c in zip(e_first, e_count)])
    save("network", dict(deck=np.array(pr["deck"]), free=np.array(pr["free"]), theta_star=theta_star,
                         well_r=np.array([r for r, _ in wells]), well_nz=np.array([len(z) for _, z in wells], np.int32),
                         well_z=np.concatenate([np.array(z, float) for _, z in wells]), t=t, well=well, iz=iz, e_first=e_first, e_count=e_count,
                         eval_theta=thetas, eval_dlog=np.array(DLOG), ref=ref, noise=noise, dref=dref, dnoise=dnoise, obs=obs, dobs=dobs))


def generate_field():
    pr = FLD
    dk, _, P0 = load_deck(pr["deck"])
    image = ufield.images([(0.0, 0.0, 1.0, 0.0)], line=(1.0, 0.0, pr["line"]), kind="constant_head")[1]
    pump = np.array([(0.0, 0.0, 1.0, 0.0), pr["p1"] + (0.6, T0_P1), tuple(image)])
    assert pump[2, 2] == -1.0 and pump[2, 3] == 0.0
    obs_wells, times = pr["obs_wells"], pr["times"]
    well_x, well_y = np.array([w[0] for w in obs_wells]), np.array([w[1] for w in obs_wells])
    depths = [np.array(w[2], float) for w in obs_wells]
    t = np.concatenate(times + [times[1][pr["extra"]:pr["extra"] + 1]])
    well = np.concatenate([np.full(len(times[0]), 0), np.full(len(times[1]) + 1, 1)]).astype(np.int32)
    iz = np.concatenate([np.zeros(len(times[0])), np.full(len(times[1]), -1), [1]]).astype(np.int32)
    perm = np.random.default_rng(pr["seed"]).permutation(len(t))
    t, well, iz = t[perm], well[perm], iz[perm]
    assert len(t) <= 30
    virt_well, virt_r, term_first, term_pump, term_virt, term_t = terms_of(pump, well_x, well_y, t, well)
    tfac = np.repeat(t, np.diff(term_first)) / term_t
    assert (tfac[term_pump != 1] == 1.0).all() and (tfac[term_pump == 1] > 1.0).all() and (np.diff(term_first) == 2).any()
    vtimes = {int(v): np.unique(term_t[term_virt == v]) for v in np.unique(term_virt)}
    first, n = {}, 0
    for v, tv in vtimes.items():
        for q in range(len(tv)):
            first[(v, q)] = n
            n += len(depths[virt_well[v]])
    nterm = len(term_t)
    e_first, e_count = np.zeros(nterm, np.int32), np.zeros(nterm, np.int32)
    for i in range(len(t)):
        for k in range(term_first[i], term_first[i + 1]):
            v = int(term_virt[k])
            q = int(np.searchsorted(vtimes[v], term_t[k]))
            assert vtimes[v][q] == term_t[k]
            e_first[k] = first[(v, q)] + (iz[i] if iz[i] >= 0 else 0)
            e_count[k] = 1 if iz[i] >= 0 else len(depths[virt_well[v]])
    groups = [(virt_r[v], depths[virt_well[v]], tv) for v, tv in vtimes.items()]
    all_t = np.concatenate([tv for tv in vtimes.values()])
    theta_star, thetas, ref, noise, dref, dnoise, (h, dh, Hc) = evaluate_entries(P0, dk, pr["free"], all_t, groups, n)
    obs, dobs = np.zeros(len(t)), np.zeros(len(t))
    for i in range(len(t)):
        acc, dacc = 0.0, 0.0
        for k in range(term_first[i], term_first[i + 1]):
            q = pump[term_pump[k], 2]
            acc = acc + q * screen_average(h[e_first[k]:e_first[k] + e_count[k]])
            dacc = dacc + q * (tfac[k] * screen_average(dh[e_first[k]:e_first[k] + e_count[k]]))
        obs[i], dobs[i] = acc * Hc, dacc * Hc
    assert np.isfinite(obs).all() and np.isfinite(dobs).all()
    save("field", dict(deck=np.array(pr["deck"]), free=np.array(pr["free"]), theta_star=theta_star, pump=pump, well_x=well_x, well_y=well_y,
                       well_nz=np.array([len(z) for z in depths], np.int32), well_z=np.concatenate(depths), t=t, well=well, iz=iz,
                       virt_well=virt_well, virt_r=virt_r, term_first=term_first, term_pump=term_pump, term_virt=term_virt, term_t=term_t,
                       tfac=tfac, e_first=e_first, e_count=e_count, eval_theta=thetas, eval_dlog=np.array(DLOG), ref=ref, noise=noise,
                       dref=dref, dnoise=dnoise, obs=obs, dobs=dobs))


def save(key, out):
    path = os.path.join(GOLD, f"fit_deriv_{key}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    for key in (sys.argv[1:] or ["neuman74", "theis", "network", "field"]):
        {"network": generate_network, "field": generate_field}.get(key, lambda k=key: generate_plain(k))()
