"""The fit reduction under multiplicities (the RESAMPLE instantiations of fit_reduce_kernel, unconfined_amd/csrc/ucf_fit.hip) restated
in numpy from the arithmetic that include/ucf.h states with ucf_fit_set_resample, one rounded fp64 operation at a time; the call of
ucf_debug_fit_reduce_resampled; the multiplicities of the GPU cases; and the block bootstrap in pure Python.  The sources, the
order of the sums and the synthetic inputs are those of tests/fit_reduce_restate.py, the loss that of tests/fit_loss_restate.py;
neither module is changed.  A helper module: no tests here.

    reduction r: the plans of set set_of[r] under m = mult[rep[r]][i] (rep[r] == -1: every m = 1); `ok` is the counting rule
    m == 0 and ok:      phi_out += wr * wr;  where wd_i > 0 also phi_out += wrd * wrd;  nheld++          (not ok: in no count)
    m  > 0 and not ok:  nbad++
    m  > 0 and ok:      fm = (double)m;  (rho, b) of x;  fb = fm * b;  phi += fm * rho;  phi_w += fb * (x * x);  bw_j = fb * wd_j;
                        g_j += bw_j * x;  A_jk += bw_j * wd_k;  ndown++ where b < 1.0;  nuse += m;  the derivative term the same
                        where wd_i > 0, also phi_d += fm * rho and nuse_d += m
    sums per reduction: phi | g | upper A | [phi_d] | phi_w | phi_out;  counts: nuse, nuse_d, nheld, ndown"""
import numpy as np

import fit_loss_restate as fl
import fit_reduce_restate as fr
from unconfined_amd.abi import LOSS_HUBER as HUBER, LOSS_L2 as L2, LOSS_TUKEY as TUKEY

KINDS = {"l2": L2, "huber": HUBER, "tukey": TUKEY}
C_GPU = fl.C_GPU
# the reductions of the GPU cases: nsets = 2, nrep = 4, nred = 5
SET_OF = np.array([1, 0, 1, 1, 0], np.int32)
REP = np.array([-1, 0, 2, 1, 3], np.int32)
MASK64 = (1 << 64) - 1


def nsums(npar, deriv):
    return fr.nsums(npar, deriv) + 2


def gpu_mult(nobs, seed=0):
    """the four rows of the GPU cases: all ones; random 0..3 that holds zeros (nobs > 1); 65535 and zeros in turn; all zero"""
    rng = np.random.default_rng([nobs, seed, 77])
    mult = np.zeros((4, nobs), np.uint16)
    mult[0] = 1
    mult[1] = rng.integers(0, 4, nobs)
    if nobs > 1:
        mult[1, rng.integers(0, nobs)] = 0
        mult[1, (np.flatnonzero(mult[1] == 0)[0] + 1) % nobs] = 3
    mult[2, ::2] = 65535
    return mult


def restate(inp, kind, c, mult, set_of, rep):
    """dict of sums [nred][nsums], nbad [nred], counts [nred][4]; also per reduction `used`, `held` [nred][nobs] (observations
    that count with m > 0, with m == 0)"""
    npar, nsets, nobs = inp["npar"], inp["nsets"], inp["nobs"]
    deriv = inp["dh"] is not None
    P, NS = 1 + 2 * npar, nsums(npar, deriv)
    NT = 1 + npar + npar * (npar + 1) // 2                       # phi | g | A of one residual term
    two_dlog = np.float64(inp["two_dlog"])
    set_of = np.arange(len(rep)) if set_of is None else np.asarray(set_of)
    nred = len(set_of)
    rep = np.full(nred, -1) if rep is None else np.asarray(rep)
    out = dict(sums=np.zeros((nred, NS)), nbad=np.zeros(nred, np.int32), counts=np.zeros((nred, 4), np.int32),
               used=np.zeros((nred, nobs), bool), held=np.zeros((nred, nobs), bool))
    base = {}                                                    # per parameter set: what does not depend on the multiplicities

    def curve(s, h, derivative, wt, target):
        """s[k], x, wd[j], rho and the unscaled b of one curve of set s"""
        sv = np.stack([fr.source_value(inp, h, s * P + k, derivative) * inp["Hc"][s * P + k] for k in range(P)])
        d = [(sv[1 + 2 * j] - sv[2 + 2 * j]) / two_dlog for j in range(npar)]
        x = wt * (target - sv[0])
        rho, b = fl.loss_terms(kind, c, x)
        return sv, x, [wt * d[j] for j in range(npar)], rho, b

    def terms(fm, x, wd, rho, b):
        """phi | g | A, then phi_w, under the multiplicities"""
        frho, fb = fm * rho, fm * b
        bw = [fb * wd[j] for j in range(npar)]
        t = [frho] + [bw[j] * x for j in range(npar)] + [bw[j] * wd[k] for j in range(npar) for k in range(j, npar)]
        return np.stack(t), fb * (x * x)
    with np.errstate(all="ignore"):
        for r in range(nred):
            s = int(set_of[r])
            m = np.ones(nobs, np.int64) if rep[r] < 0 else np.asarray(mult)[rep[r]].astype(np.int64)
            fm = m.astype(np.float64)
            if s not in base:
                one = curve(s, inp["h"], False, inp["w"], inp["obs"])
                ok = np.isfinite(one[0]).all(axis=0)
                two = None
                if deriv:
                    two = curve(s, inp["dh"], True, inp["wd"], inp["dobs"])
                    ok = ok & ((inp["wd"] == 0.0) | np.isfinite(two[0]).all(axis=0))
                base[s] = (one, two, ok)
            one, two, ok = base[s]
            _, x, wd, rho, b = one
            t, tw = terms(fm, x, wd, rho, b)
            t1, t2, active = np.zeros((NS, nobs)), np.zeros((NS, nobs)), np.zeros(nobs, bool)
            t1[:NT], t1[NS - 2], t1[NS - 1] = t, tw, x * x
            bd = np.ones(nobs)
            if deriv:
                _, xd, wdd, rhod, bd = two
                td, twd = terms(fm, xd, wdd, rhod, bd)
                active = inp["wd"] > 0.0
                t2[:NT], t2[NS - 3], t2[NS - 2], t2[NS - 1] = td, td[0], twd, xd * xd
            used, held = ok & (m > 0), ok & (m == 0)
            out["used"][r], out["held"][r] = used, held
            out["nbad"][r] = int((~ok & (m > 0)).sum())
            out["counts"][r] = (int(m[used].sum()), int(m[used & active].sum()), int(held.sum()),
                                int((used & (b < 1.0)).sum()) + int((used & active & (bd < 1.0)).sum()))
            # which rows an observation adds to: phi_out alone where it is held out, every other row where it is used; the drawdown
            # term adds nothing to phi_d (not even +0.0)
            M1, M2 = np.zeros((NS, nobs), bool), np.zeros((NS, nobs), bool)
            M1[:NS - 1], M1[NS - 1] = used, held
            if deriv:
                M1[NS - 3] = False
            M2[:NS - 1], M2[NS - 1] = used & active, held & active
            acc = np.zeros((NS, fr.LANES))
            for i0 in range(0, nobs, fr.LANES):          # lane l takes l, l + 256, ... in ascending order
                n = min(fr.LANES, nobs - i0)
                sl = slice(i0, i0 + n)
                a = np.where(M1[:, sl], acc[:, :n] + t1[:, sl], acc[:, :n])
                acc[:, :n] = np.where(M2[:, sl], a + t2[:, sl], a)
            out["sums"][r] = fr.reduce_lanes(acc, "documented")
    return out


def debug_fit_reduce_resampled(inp, kind, c, mult, set_of, rep, nrep=None, nred=None):
    """ucf_debug_fit_reduce_resampled on an input set: dict of sums, nbad, counts"""
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    addr = fr.addr
    npar, nsets, nobs = inp["npar"], inp["nsets"], inp["nobs"]
    deriv = inp.get("dh") is not None
    f64 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.float64)
    i32 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.int32)
    i64 = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.int64)
    a = {k: f64(k) for k in ("h", "dh", "Hc", "obs", "w", "dobs", "wd", "q", "tfac")}
    a.update({k: i32(k) for k in ("slot", "at", "count", "first")})
    a.update({k: i64(k) for k in ("prefix", "stride")})
    mult = None if mult is None else np.ascontiguousarray(mult, dtype=np.uint16)
    set_of = None if set_of is None else np.ascontiguousarray(set_of, dtype=np.int32)
    rep = None if rep is None else np.ascontiguousarray(rep, dtype=np.int32)
    if nrep is None:
        nrep = 0 if mult is None else mult.shape[0]
    if nred is None:
        nred = len(set_of) if set_of is not None else (len(rep) if rep is not None else nsets)
    nr = max(nred, 0)
    out = dict(sums=np.full((nr, nsums(max(npar, 0), deriv)), -7.0), nbad=np.full(nr, -7, np.int32), counts=np.full((nr, 4), -7, np.int32))
    nref = inp["nref"] if "nref" in inp else (0 if a["prefix"] is None else len(a["prefix"]))
    ucflib.check(so.ucf_debug_fit_reduce_resampled(int(kind), float(c), inp["source"], npar, nsets, nobs, float(inp["two_dlog"]),
                                                   inp.get("nh", len(a["h"])), addr(a["h"]), addr(a["dh"]), addr(a["Hc"]), addr(a["obs"]), addr(a["w"]),
                                                   addr(a["dobs"]), addr(a["wd"]), addr(a["slot"]), int(inp.get("plan_stride", 0)), nref,
                                                   addr(a["prefix"]), addr(a["stride"]), addr(a["at"]), addr(a["count"]), addr(a["q"]), addr(a["tfac"]),
                                                   addr(a["first"]), int(nrep), addr(mult), int(nred), addr(set_of), addr(rep),
                                                   addr(out["sums"]) if not inp.get("null_sums") else None, addr(out["nbad"]),
                                                   addr(out["counts"]) if not inp.get("null_counts") else None))
    return out


# ---- the block bootstrap in pure Python: splitmix64 and a big-integer product

def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK64
    x = state
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return state, x ^ (x >> 31)


def blocks_restate(nobs, block, nrep, seed):
    block = list(range(nobs)) if block is None else [int(b) for b in block]
    nb = max(block) + 1
    state = seed & MASK64
    mult = np.zeros((nrep, nobs), np.int64)
    for r in range(nrep):
        drawn = [0] * nb
        for _ in range(nb):
            state, x = splitmix64(state)
            drawn[(x * nb) >> 64] += 1
        mult[r] = [drawn[b] for b in block]
    return mult
