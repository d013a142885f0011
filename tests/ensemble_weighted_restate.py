"""The arithmetic of the weighted ensemble reduction as include/ucf.h states it (ucf_ensemble_quantise,
field_ensemble_wmoments_kernel, field_ensemble_wquantile_kernel), restated in numpy one rounded operation at a time.  Shared by
the CPU tests, which hold it to the unweighted restatement and to numpy's weighted quantile, and the GPU tests, which hold the
kernels to it bit for bit."""
import math

import numpy as np

TWO32 = 4294967296.0


def quantise(weight):
    """(u [nens] uint64, ess) by the rule of ucf_ensemble_quantise; the checks are the library's and are not restated"""
    w = np.asarray(weight, dtype=np.float64)
    wmax = w.max()
    u = np.array([int(math.floor(float(x / wmax) * TWO32 + 0.5)) for x in w], dtype=np.uint64)
    U = sum(int(x) for x in u)
    U2 = 0.0
    for x in u:
        U2 = U2 + float(x) * float(x)
    return u, float(U) * float(U) / U2


def restate_weighted(a, u, levels, limits):
    """a [nens][...], u [nens] integer weights: dict of nfin, mean, sd (numpy's square root), min, max, quant [nq][...], pexc
    [nlim][...], nbad.  F = the members with u > 0 and a finite value, in member order."""
    nens, shape = len(a), a.shape[1:]
    v = a.reshape(nens, -1)
    nout = v.shape[1]
    ui = np.array([int(x) for x in u], dtype=np.int64)              # at most 2^32 each: sums of 1024 of them are exact in int64
    du = ui.astype(np.float64)
    inF = np.isfinite(v) & (ui > 0)[:, None]
    n = inF.sum(axis=0)
    U = np.where(inF, ui[:, None], 0).sum(axis=0)                   # integer
    dU = U.astype(np.float64)
    nan = np.full(nout, np.nan)
    with np.errstate(all="ignore"):
        acc, U2, lo, hi = np.zeros(nout), np.zeros(nout), nan.copy(), nan.copy()
        for m in range(nens):
            acc = np.where(inF[m], acc + du[m] * v[m], acc)
            U2 = np.where(inF[m], U2 + du[m] * du[m], U2)
            lo = np.where(inF[m] & ~(v[m] >= lo), v[m], lo)
            hi = np.where(inF[m] & ~(v[m] < hi), v[m], hi)
        mean = acc / dU
        ss = np.zeros(nout)
        for m in range(nens):
            d = v[m] - mean
            ss = np.where(inF[m], ss + du[m] * (d * d), ss)
        den = dU - U2 / dU
        sd = np.where((n < 2) | ~(den > 0.0), np.nan, np.sqrt(ss / den))
        pexc = [np.where(inF & (v > np.float64(lim)), ui[:, None], 0).sum(axis=0).astype(np.float64) / dU for lim in limits]
        pexc = np.stack(pexc) if len(limits) else np.zeros((0, nout))
        # the stable order: ascending, ties in member order; members outside F go last with weight 0 and never match
        order = np.argsort(np.where(inF, v, np.inf), axis=0, kind="stable")
        xs = np.take_along_axis(v, order, axis=0)
        us = np.take_along_axis(np.where(inF, ui[:, None], 0), order, axis=0)
        E = np.cumsum(us, axis=0) - us                              # the weight in front of a member, an integer
        Ef, Euf = E.astype(np.float64), (E + us).astype(np.float64)
        quant = []
        for p in levels:
            tgt = np.float64(p) * dU
            match = (us > 0) & (((Ef < tgt) & (tgt <= Euf)) | ((tgt == 0.0) & (E == 0)))
            assert (match.sum(axis=0) == (n > 0)).all(), "the intervals (E, E + u] partition (0, U]: exactly one member matches"
            quant.append(np.where(n == 0, np.nan, np.take_along_axis(xs, match.argmax(axis=0)[None], axis=0)[0]))
    out = dict(nfin=n.astype(np.int32).reshape(shape), mean=mean.reshape(shape), sd=sd.reshape(shape), min=lo.reshape(shape), max=hi.reshape(shape),
               pexc=pexc.reshape((len(limits),) + shape), nbad=int((n < int((ui > 0).sum())).sum()))
    out["quant"] = np.stack(quant).reshape((len(levels),) + shape) if len(levels) else np.zeros((0,) + shape)
    return out


def order_statistic(a, levels):
    """with equal weights: the value of index ceil(p n) - 1 (0 at p = 0) of the stable sort of the finite members, [nq][...]"""
    nens, shape = len(a), a.shape[1:]
    v = a.reshape(nens, -1)
    fin = np.isfinite(v)
    n = fin.sum(axis=0)
    xs = np.take_along_axis(v, np.argsort(np.where(fin, v, np.inf), axis=0, kind="stable"), axis=0)
    out = []
    for p in levels:
        k = np.clip(np.ceil(np.float64(p) * n.astype(np.float64)).astype(np.int64) - 1, 0, np.maximum(n - 1, 0))
        out.append(np.where(n == 0, np.nan, np.take_along_axis(xs, k[None], axis=0)[0]))
    return np.stack(out).reshape((len(levels),) + shape)
