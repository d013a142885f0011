"""The arithmetic of ucf_field_yield as include/ucf.h states it -- field_response_kernel, field_yield_kernel and the member
reduction -- restated in numpy one rounded operation at a time.  Shared by the CPU tests, which hold the ratio test to exact
rational arithmetic, and the GPU tests, which hold the kernels to it bit for bit."""
import numpy as np

from ensemble_weighted_restate import restate_weighted


def constrained(limit):
    """con (ascending flat indices of the outputs with a finite limit) and their limits"""
    lim = np.asarray(limit, dtype=np.float64).ravel()
    con = np.flatnonzero(np.isfinite(lim)).astype(np.int32)
    return con, lim[con]


def response(wells, groups, h, ctl, nctl, con, nloc, nz, Hc):
    """R [nctl + 1][ncon] of one member: wells [nwell][4] (x, y, q, t0), groups as WellField.groups states them, h[g]
    [nt_g][nr_g][nz] the dimensionless group results (None: not launched), Hc the member's scale"""
    owner = [next(g for g, grp in enumerate(groups) if grp["col"][0, j] >= 0) for j in range(len(wells))]
    R = np.zeros((nctl + 1, len(con)))
    for c in range(nctl + 1):
        mine = -1 if c == nctl else c
        for i, e in enumerate(con):
            iz, p = int(e) % nz, int(e) // nz
            iloc, k = p % nloc, p // nloc
            acc = np.float64(0.0)
            for j in range(len(wells)):
                grp = groups[owner[j]]
                if ctl[j] != mine or k < grp["k0"]:
                    continue
                acc = acc + np.float64(wells[j][2]) * h[owner[j]][k - grp["k0"], grp["col"][iloc, j], iz]
            R[c, i] = acc * np.float64(Hc)
    return R


def ratio_test(R, x, limit_con, con, smax):
    """R [nens][nctl + 1][ncon], x [npat][nctl]: dict of y, fe, hi, lo [nens][npat] (float64), bind, dead (int32) and nbad, the
    members with a slot value that is not finite.  The outputs are walked in ascending i with the header's statements."""
    R = np.asarray(R, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    nens, nslot, ncon = R.shape
    nctl, npat = nslot - 1, len(x)
    smax = np.float64(smax)
    y, fe, hi, lo = (np.zeros((nens, npat)) for _ in range(4))
    bind, dead = np.full((nens, npat), -1, np.int32), np.zeros((nens, npat), np.int32)
    nbad = 0
    with np.errstate(all="ignore"):
        for m in range(nens):
            if not np.isfinite(R[m]).all():
                nbad += 1
                y[m] = fe[m] = hi[m] = lo[m] = np.nan
                continue
            room = np.asarray(limit_con, dtype=np.float64) - R[m, nctl]
            for p in range(npat):
                D = np.zeros(ncon)
                for c in range(nctl):
                    D = D + x[p, c] * R[m, c]
                cand = room / D
                h, l, b, d = smax, np.float64(0.0), -1, 0
                for i in range(ncon):
                    if D[i] > 0.0:
                        if cand[i] < h or (cand[i] == h and b == -1):
                            h, b = cand[i], int(con[i])
                    elif D[i] < 0.0:
                        if cand[i] > l:
                            l = cand[i]
                    elif D[i] == 0.0:
                        if room[i] < 0.0:
                            d = 1
                feas = d == 0 and l <= h
                hi[m, p], lo[m, p], bind[m, p], dead[m, p] = h, l, b, d
                y[m, p] = h if feas else 0.0
                fe[m, p] = 1.0 if feas else 0.0
    return dict(y=y, fe=fe, hi=hi, lo=lo, bind=bind, dead=dead, nbad=nbad)


def reduce_members(y, fe, u, q, levels):
    """the member reduction with nout = npat: the statistics of y (quant at q, pexc at levels) and pfeas = the share of the
    valid members with fe > 0.5.  u: the integer weights; None = every member 2^32, which gives mean, sd, min, max, nfin and
    the shares the bits of the unweighted kernels -- the unweighted quantile (interpolated) is `quantile_linear`."""
    nens = len(y)
    uu = np.full(nens, 2 ** 32, np.uint64) if u is None else u
    out = restate_weighted(np.asarray(y), uu, list(q) if u is not None else [], list(levels))
    if u is None:
        out["quant"] = quantile_linear(np.asarray(y), q)
    out["pfeas"] = restate_weighted(np.asarray(fe), uu, [], [0.5])["pexc"][0]
    return out


def quantile_linear(a, levels):
    """the order statistics of ucf_field_ensemble: x_k + g (x_{k+1} - x_k) on the stable sort of the finite members, [nq][nout]"""
    nens, nout = a.shape
    out = np.full((len(levels), nout), np.nan)
    for e in range(nout):
        v = a[:, e]
        xs = v[np.isfinite(v)]
        xs = xs[np.argsort(xs, kind="stable")]
        n = len(xs)
        if n == 0:
            continue
        for i, p in enumerate(levels):
            pos = np.float64(p) * np.float64(n - 1)
            k = int(np.floor(pos))
            if k >= n - 1:
                out[i, e] = xs[n - 1]
            else:
                g = pos - np.float64(k)
                out[i, e] = xs[k] + g * (xs[k + 1] - xs[k])
    return out
