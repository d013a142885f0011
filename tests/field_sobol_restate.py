"""field_sobol_kernel (unconfined_amd/csrc/ucf_field_sobol.hip) and ucf_sobol_design restated in numpy, operation by operation as
include/ucf.h states them with ucf_field_sobol.  Vectorised over the outputs and sequential in the base row r: a row that is not
complete at an output leaves that output's sums untouched (``np.where(c_r, acc + x, acc)``), so every sum adds the complete rows
in ascending r from +0.0, each addition rounded on its own.  Every NaN written is numpy's, 0x7ff8000000000000."""
import numpy as np


def design(draws, npar=None):
    """ucf_sobol_design: draws [2 N][npar] -> thetas [(npar + 2) N][npar]; pure copies"""
    draws = np.asarray(draws, dtype=np.float64)
    N, npar = len(draws) // 2, draws.shape[1]
    A, B = draws[:N], draws[N:]
    return np.concatenate([A, B] + [np.where(np.arange(npar) == j, B, A) for j in range(npar)])


def _out(x):
    """x, or the one NaN that the statement writes"""
    return np.where(np.isnan(x), np.nan, x)


def sobol(a, npar, nbase):
    """a [(npar + 2) nbase][nout] -> dict of S, ST, seS, seST [npar][nout], mean, var [nout], nrow [nout] (int32), nbad"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    N = int(nbase)
    assert a.ndim == 2 and a.shape[0] == (npar + 2) * N
    nout = a.shape[1]
    blocks = a.reshape(npar + 2, N, nout)
    fa, fb, fj = blocks[0], blocks[1], blocks[2:]
    complete = np.isfinite(blocks).all(axis=0)                               # [N][nout]
    zero = np.zeros(nout)
    with np.errstate(all="ignore"):
        n = complete.sum(axis=0).astype(np.int32)
        sA, sB = zero.copy(), zero.copy()
        for r in range(N):
            c = complete[r]
            sA = np.where(c, sA + fa[r], sA)
            sB = np.where(c, sB + fb[r], sB)
        dn = n.astype(np.float64)
        mean = (sA + sB) / (2 * n).astype(np.float64)
        qA, qB = zero.copy(), zero.copy()
        v1, q1, vt, qt = (np.zeros((npar, nout)) for _ in range(4))
        for r in range(N):
            c = complete[r]
            da, db = fa[r] - mean, fb[r] - mean
            qA = np.where(c, qA + da * da, qA)
            qB = np.where(c, qB + db * db, qB)
            for j in range(npar):
                p = db * (fj[j, r] - fa[r])
                v1[j] = np.where(c, v1[j] + p, v1[j])
                q1[j] = np.where(c, q1[j] + p * p, q1[j])
                dt = fa[r] - fj[j, r]
                pt = dt * dt
                vt[j] = np.where(c, vt[j] + pt, vt[j])
                qt[j] = np.where(c, qt[j] + pt * pt, qt[j])
        var = np.where(n == 0, np.nan, (qA + qB) / (2 * n - 1).astype(np.float64))
        pos = var > 0.0
        two = pos & (n >= 2)
        dn1 = (n - 1).astype(np.float64)
        m1, mt = v1 / dn, vt / dn
        S = np.where(pos, _out(m1 / var), np.nan)
        ST = np.where(pos, _out((0.5 * mt) / var), np.nan)
        w1 = q1 / dn - m1 * m1
        wt = qt / dn - mt * mt
        w1 = np.where(w1 < 0.0, 0.0, w1)
        wt = np.where(wt < 0.0, 0.0, wt)
        seS = np.where(two, _out(np.sqrt(w1 / dn1) / var), np.nan)
        seST = np.where(two, _out((0.5 * np.sqrt(wt / dn1)) / var), np.nan)
    return dict(S=S, ST=ST, seS=seS, seST=seST, mean=_out(mean), var=_out(var), nrow=n, nbad=int((n < N).sum()))
