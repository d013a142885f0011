"""The fit reduction under a robust loss (the ROBUST instantiations of fit_reduce_kernel, unconfined_amd/csrc/ucf_fit.hip) restated
in numpy from the arithmetic that include/ucf.h states with ucf_fit_set_loss, one rounded fp64 operation at a time; the call of
ucf_debug_fit_reduce_loss; and the exact values of rho and b in rational arithmetic.  The sources, the order of the sums and the
synthetic inputs are those of tests/fit_reduce_restate.py.  A helper module: no tests here.

    a = fabs(x)
    HUBER:  a <= c :  b = 1.0;            rho = x * x
            else   :  b = c / a;          rho = c * (2.0 * a - c)
    TUKEY:  c2 = c * c;  u = x / c
            a <  c :  v = 1.0 - u * u;  b = v * v;  rho = (c2 * (1.0 - b * v)) / 3.0
            else   :  b = 0.0;            rho = c2 / 3.0
    phi += rho (derivative term: also phi_d += rho);  phi_w += b * (x * x);  bw_j = b * wd_j;  g_j += bw_j * x;  A_jk += bw_j * wd_k
    sums per set: phi | g | upper A | [phi_d] | phi_w;  ndown = counted residual terms with b < 1.0"""
from fractions import Fraction

import numpy as np

import fit_reduce_restate as fr
from unconfined_amd.abi import LOSS_HUBER as HUBER, LOSS_L2 as L2, LOSS_TUKEY as TUKEY

KINDS = {"huber": HUBER, "tukey": TUKEY}
# The constant of the GPU cases.  With 2.0 one case (network, no derivative data, NPAR 0, nobs 257) has 92 % of its residual terms
# inside c; with 1.25 every case has between 33 % and 77 % inside.  tests/test_fit_loss_host.py holds the inputs to 10 % a side.
C_GPU = 1.25


def nsums(npar, deriv):
    return fr.nsums(npar, deriv) + 1


def loss_terms(kind, c, x):
    """(rho, b) of the weighted residuals x, operation for operation as stated above"""
    x = np.asarray(x, np.float64)
    c = np.float64(c)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        if kind == L2:
            return x * x, np.ones(x.shape)
        if kind == HUBER:
            inl = a <= c
            return np.where(inl, x * x, c * (2.0 * a - c)), np.where(inl, 1.0, c / a)
        c2, u = c * c, x / c
        v = 1.0 - u * u
        bb = v * v
        inl = a < c
        return np.where(inl, (c2 * (1.0 - bb * v)) / 3.0, c2 / 3.0), np.where(inl, bb, 0.0)


def exact_terms(kind, c, x):
    """(rho, b) of one finite x as Fractions: the loss itself, no rounding"""
    X, Cc = Fraction(float(x)), Fraction(float(c))
    a = abs(X)
    if kind == HUBER:
        return (X * X, Fraction(1)) if a <= Cc else (Cc * (2 * a - Cc), Cc / a)
    if a >= Cc:
        return Cc * Cc / 3, Fraction(0)
    v = 1 - (X / Cc) ** 2
    return Cc * Cc * (1 - v ** 3) / 3, v * v


def restate(inp, kind, c):
    """dict of sums [nsets][nsums], nbad, ndown [nsets], b, bd [nsets][nobs] (bd with dh only), J, sim, Jd, simd as
    fit_reduce_restate.restate gives them; also per set the residuals `x`, `xd`, and `counted`, `weighted` [nsets][nobs]"""
    npar, nsets, nobs = inp["npar"], inp["nsets"], inp["nobs"]
    deriv = inp["dh"] is not None
    P, NS = 1 + 2 * npar, nsums(npar, deriv)
    NT = 1 + npar + npar * (npar + 1) // 2                       # phi | g | A of one residual term
    two_dlog = np.float64(inp["two_dlog"])
    out = dict(sums=np.zeros((nsets, NS)), nbad=np.zeros(nsets, np.int32), ndown=np.zeros(nsets, np.int32), b=np.full((nsets, nobs), np.nan),
               J=np.zeros((nsets, nobs, npar)), sim=np.zeros((nsets * P, nobs)), x=np.zeros((nsets, nobs)), xd=np.zeros((nsets, nobs)),
               counted=np.zeros((nsets, nobs), bool), weighted=np.zeros((nsets, nobs), bool))
    if deriv:
        out.update(Jd=np.zeros((nsets, nobs, npar)), simd=np.zeros((nsets * P, nobs)), bd=np.full((nsets, nobs), np.nan))
    with np.errstate(all="ignore"):
        for s in range(nsets):
            def side(h, derivative, wt, target):
                """s[k], d[j], x, b and the terms phi | g | A, then phi_w, of one curve"""
                sv = np.stack([fr.source_value(inp, h, s * P + k, derivative) * inp["Hc"][s * P + k] for k in range(P)])
                d = [(sv[1 + 2 * j] - sv[2 + 2 * j]) / two_dlog for j in range(npar)]
                x = wt * (target - sv[0])
                wd = [wt * d[j] for j in range(npar)]
                rho, b = loss_terms(kind, c, x)
                bw = [b * wd[j] for j in range(npar)]
                t = [rho] + [bw[j] * x for j in range(npar)] + [bw[j] * wd[k] for j in range(npar) for k in range(j, npar)]
                return sv, d, x, b, np.stack(t), b * (x * x)
            sv, d, x, b, t, tw = side(inp["h"], False, inp["w"], inp["obs"])
            out["sim"][s * P:(s + 1) * P] = sv
            out["J"][s] = np.stack(d, axis=1) if npar else np.zeros((nobs, 0))
            ok = np.isfinite(sv).all(axis=0)
            t1, t2, active = np.zeros((NS, nobs)), np.zeros((NS, nobs)), np.zeros(nobs, bool)
            t1[:NT], t1[NS - 1] = t, tw
            if deriv:
                sd, dd, xd, bd, td, twd = side(inp["dh"], True, inp["wd"], inp["dobs"])
                out["simd"][s * P:(s + 1) * P] = sd
                out["Jd"][s] = np.stack(dd, axis=1) if npar else np.zeros((nobs, 0))
                ok = ok & ((inp["wd"] == 0.0) | np.isfinite(sd).all(axis=0))
                active = inp["wd"] > 0.0
                t2[:NT], t2[NS - 2], t2[NS - 1] = td, td[0], twd         # phi_d += rho
                out["bd"][s] = np.where(ok & active, bd, np.nan)
                out["xd"][s] = xd
                out["ndown"][s] += int((ok & active & (bd < 1.0)).sum())
            out["b"][s] = np.where(ok, b, np.nan)
            out["x"][s] = x
            out["ndown"][s] += int((ok & (b < 1.0)).sum())
            out["nbad"][s] = int((~ok).sum())
            out["counted"][s], out["weighted"][s] = ok, ok & active
            acc = np.zeros((NS, fr.LANES))
            for i0 in range(0, nobs, fr.LANES):          # lane l takes l, l + 256, ... in ascending order
                n = min(fr.LANES, nobs - i0)
                sl = slice(i0, i0 + n)
                a = np.where(ok[sl], acc[:, :n] + t1[:, sl], acc[:, :n])
                if deriv:
                    a[NS - 2] = acc[NS - 2, :n]          # the drawdown term adds nothing to phi_d (not even +0.0)
                # the derivative term: skipped, not added as zero, where it has no weight
                acc[:, :n] = np.where(ok[sl] & active[sl], a + t2[:, sl], a)
            out["sums"][s] = fr.reduce_lanes(acc, "documented")
    return out


def longdouble_sums(inp, res, kind, c, s):
    with np.errstate(all="ignore"):        # rows of observations that do not count hold NaN and Inf; they are dropped
        return _longdouble_sums(inp, res, kind, c, s)


def _longdouble_sums(inp, res, kind, c, s):
    """(sums, sum|terms|) of set s in np.longdouble: from the residuals x, the factors b (exact values of the loss are held on
    their own) and the Jacobian as fp64 holds them, every product and sum in np.longdouble"""
    L = np.longdouble
    npar = inp["npar"]

    def side(x, b, jac, wt, keep):
        x, b, wt = x.astype(L), b.astype(L), wt.astype(L)
        wd = [wt * jac[:, j].astype(L) for j in range(npar)]
        cc, a = L(c), np.abs(x)
        if kind == HUBER:
            rho = np.where(a <= cc, x * x, cc * (L(2) * a - cc))
        else:
            v = L(1) - (x / cc) * (x / cc)
            rho = np.where(a < cc, cc * cc * (L(1) - v * v * v) / L(3), cc * cc / L(3))
        t = [rho] + [b * wd[j] * x for j in range(npar)] + [b * wd[j] * wd[k] for j in range(npar) for k in range(j, npar)]
        return np.stack(t)[:, keep], (b * x * x)[keep]
    keep = res["counted"][s]
    t, tw = side(res["x"][s], np.where(keep, res["b"][s], 0.0), res["J"][s], inp["w"], keep)
    tot, mag = t.sum(axis=1), np.abs(t).sum(axis=1)
    totw, magw = tw.sum(), np.abs(tw).sum()
    if inp["dh"] is not None:
        keep = res["weighted"][s]
        td, twd = side(res["xd"][s], np.where(keep, res["bd"][s], 0.0), res["Jd"][s], inp["wd"], keep)
        tot, mag = tot + td.sum(axis=1), mag + np.abs(td).sum(axis=1)
        tot, mag = np.append(tot, td[0].sum()), np.append(mag, np.abs(td[0]).sum())
        totw, magw = totw + twd.sum(), magw + np.abs(twd).sum()
    return np.append(tot, totw), np.append(mag, magw)


def debug_fit_reduce_loss(inp, kind, c, want=("J", "sim", "Jd", "simd", "ndown", "b", "bd")):
    """ucf_debug_fit_reduce_loss on an input set: dict of sums, nbad and the arrays of `want` that the call can give"""
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
    ns, npos, nob = max(nsets, 0), max(npar, 0), max(nobs, 0)
    nplans = ns * (1 + 2 * npos)
    out = dict(sums=np.full((ns, nsums(npos, deriv)), -7.0), nbad=np.full(ns, -7, np.int32))
    shapes = dict(J=(ns, nob, npos), Jd=(ns, nob, npos), sim=(nplans, nob), simd=(nplans, nob), b=(ns, nob), bd=(ns, nob))
    for k in want:
        if k == "ndown":
            out[k] = np.full(ns, -7, np.int32)
        elif deriv or k in ("J", "sim", "b") or (k == "bd" and inp.get("force_bd")):
            out[k] = np.full(shapes[k], -7.0)
    nref = inp["nref"] if "nref" in inp else (0 if a["prefix"] is None else len(a["prefix"]))
    ucflib.check(so.ucf_debug_fit_reduce_loss(int(kind), float(c), inp["source"], npar, nsets, nobs, float(inp["two_dlog"]), inp.get("nh", len(a["h"])),
                                              addr(a["h"]), addr(a["dh"]), addr(a["Hc"]), addr(a["obs"]), addr(a["w"]), addr(a["dobs"]), addr(a["wd"]),
                                              addr(a["slot"]), int(inp.get("plan_stride", 0)), nref, addr(a["prefix"]), addr(a["stride"]), addr(a["at"]),
                                              addr(a["count"]), addr(a["q"]), addr(a["tfac"]), addr(a["first"]), addr(out["sums"]), addr(out["nbad"]),
                                              addr(out.get("J")), addr(out.get("sim")), addr(out.get("Jd")), addr(out.get("simd")),
                                              addr(out.get("ndown")), addr(out.get("b")), addr(out.get("bd"))))
    return out
