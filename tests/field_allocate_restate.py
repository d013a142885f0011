"""The arithmetic of ucf_field_allocate as include/ucf.h states it -- the primal active-set simplex of one (member, objective), the
small solves, the ratio test, and the host step of the reliability stage -- restated with numpy scalars one rounded operation at a
time.  Shared by the CPU tests, which hold ucf_allocate_solve to it byte for byte and its working sets to exact rational
arithmetic, and the GPU tests, which hold field_allocate_kernel to both."""
from fractions import Fraction

import numpy as np

INVALID, OPTIMAL, ITERATION_CAP, INFEASIBLE_AT_ZERO, NUMERIC = -1, 0, 1, 2, 3
F = np.float64
DBL_MAX = np.finfo(np.float64).max
DTOL = F(2.0 ** -40)


def solve(A, b):
    """Gaussian elimination with partial pivoting on copies: the solution [n], or None where a pivot is zero or not finite"""
    n = len(b)
    A = [[F(A[r][c]) for c in range(n)] for r in range(n)]
    b = [F(v) for v in b]
    for col in range(n):
        piv = col
        best = abs(A[col][col])
        for r in range(col + 1, n):
            v = abs(A[r][col])
            if v > best:
                best = v
                piv = r
        if not (best > 0.0) or not (best <= DBL_MAX):
            return None
        if piv != col:
            A[col], A[piv] = A[piv], A[col]
            b[col], b[piv] = b[piv], b[col]
        for r in range(col + 1, n):
            f = A[r][col] / A[col][col]
            for c in range(col + 1, n):
                prod = f * A[col][c]
                A[r][c] = A[r][c] - prod
            prod = f * b[col]
            b[r] = b[r] - prod
    y = [F(0.0)] * n
    for r in range(n - 1, -1, -1):
        s = b[r]
        for c in range(r + 1, n):
            prod = A[r][c] * y[c]
            s = s - prod
        y[r] = s / A[r][r]
    return y


def row_of(Rm, lim, xmax, n, j):
    """(a [n], beta) of constraint id j"""
    if j < n:
        a = [F(0.0)] * n
        a[j] = F(-1.0)
        return a, F(0.0)
    if j < 2 * n:
        a = [F(0.0)] * n
        a[j - n] = F(1.0)
        return a, F(xmax[j - n])
    i = j - 2 * n
    return [F(Rm[c, i]) for c in range(n)], F(lim[i]) - F(Rm[n, i])


def two_sum(a, b):
    """(s, err) with s + err = a + b exactly"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def product_error(a, b, p):
    """a b - p exactly, p = the rounded product: what fma(a, b, -p) returns (the difference is a double; no fma is used here)"""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(p)):
        return F(np.nan)
    return F(float(Fraction(float(a)) * Fraction(float(b)) - Fraction(float(p))))


def dd_add(h, l, p, e):
    """(h, l) + (p, e), renormalised"""
    s, t = two_sum(h, p)
    low = l + (t + e)
    h = s + low
    return h, low - (h - s)


def dd_add_product(h, l, sign, a, xh, xl):
    """(h, l) + sign a (xh + xl): a xh exactly, a xl rounded"""
    p = a * xh
    e = product_error(a, xh, p)
    return dd_add(h, l, sign * p, sign * (e + a * xl))


def polish(Rm, lim, xmax, n, W, B, x):
    """two steps of iterative refinement of the vertex on the final working set with the residual in double-double: (x, xl)"""
    x, xl = list(x), [F(0.0)] * n
    for _ in range(2):
        r = []
        for s in range(n):
            if W[s] < n:
                h, l = F(0.0), F(0.0)
            elif W[s] < 2 * n:
                h, l = F(xmax[W[s] - n]), F(0.0)
            else:
                h, l = two_sum(F(lim[W[s] - 2 * n]), -F(Rm[n, W[s] - 2 * n]))
            for c in range(n):
                h, l = dd_add_product(h, l, F(-1.0), B[s][c], x[c], xl[c])
            r.append(h)
        e = solve(B, r)
        if e is None:
            return x, xl
        for c in range(n):
            x[c], xl[c] = dd_add(x[c], xl[c], e[c], F(0.0))
    return x, xl


def solve_one(Rm, lim, w, xmax, maxit):
    """one (member, objective): dict of x, lam [n], g, status, iters, work [n]"""
    Rm = np.asarray(Rm, dtype=np.float64)
    n, ncon = Rm.shape[0] - 1, Rm.shape[1]
    nan = F(np.nan)
    none = dict(x=[nan] * n, lam=[nan] * n, g=nan, work=[-1] * n)
    with np.errstate(all="ignore"):
        if not np.isfinite(Rm).all():
            return dict(none, status=INVALID, iters=0)
        room_v = np.asarray(lim, dtype=np.float64) - Rm[n]
        if (room_v < 0.0).any():
            return dict(none, status=INFEASIBLE_AT_ZERO, iters=0)
        W = list(range(n))
        x = [F(0.0)] * n
        iters = 0
        for _ in range(maxit):
            rows = [row_of(Rm, lim, xmax, n, j) for j in W]
            B = [a for a, _ in rows]
            # 1. the multipliers
            lam = solve([[B[c][r] for c in range(n)] for r in range(n)], [F(w[r]) for r in range(n)])
            if lam is None:
                return dict(none, status=NUMERIC, iters=iters)
            # 2. Bland: the lowest id among the negative multipliers
            k, low = -1, None
            for s in range(n):
                if lam[s] < 0.0 and (low is None or W[s] < low):
                    k, low = s, W[s]
            if k < 0:
                x, xl = polish(Rm, lim, xmax, n, W, B, x)
                g, gl = F(0.0), F(0.0)
                for c in range(n):
                    g, gl = dd_add_product(g, gl, F(1.0), F(w[c]), x[c], xl[c])
                order = sorted(range(n), key=lambda s: W[s])
                return dict(x=x, lam=[lam[s] for s in order], g=g, status=OPTIMAL, iters=iters, work=[W[s] for s in order])
            # 3. the direction
            d = solve(B, [F(-1.0) if s == k else F(0.0) for s in range(n)])
            if d is None:
                return dict(none, status=NUMERIC, iters=iters)
            # 4. the ratio test: the lexicographic minimum of (cand, id)
            best, enter = F(np.inf), None
            dmax = max(abs(v) for v in d)
            for j in range(2 * n):
                if j in W:
                    continue
                if j < n:
                    D = -d[j]
                    slack = x[j]
                else:
                    D = d[j - n]
                    slack = F(xmax[j - n]) - x[j - n]
                if D > DTOL * dmax:
                    if slack < 0.0:
                        slack = F(0.0)
                    cand = slack / D
                    if cand < best or (cand == best and (enter is None or j < enter)):
                        best, enter = cand, j
            # the output rows, every i at once: each line below is one rounded operation per element
            Dv, Sv, ax = np.zeros(ncon), np.zeros(ncon), np.zeros(ncon)
            for c in range(n):
                prod = Rm[c] * d[c]
                Dv = Dv + prod
                Sv = Sv + np.abs(prod)
                prod = Rm[c] * x[c]
                ax = ax + prod
            slack = room_v - ax
            slack = np.where(slack < 0.0, 0.0, slack)
            cand = slack / Dv
            open_ = Dv > DTOL * Sv
            for j in W:
                if j >= 2 * n:
                    open_[j - 2 * n] = False
            open_ &= ~np.isnan(cand)
            if open_.any():
                least = cand[open_].min()
                j = 2 * n + int(np.flatnonzero(open_ & (cand == least))[0])
                if least < best or (least == best and (enter is None or j < enter)):
                    best, enter = least, j
            if enter is None:
                return dict(none, status=NUMERIC, iters=iters)
            # 5. the new working set and its vertex
            W[k] = enter
            rows = [row_of(Rm, lim, xmax, n, j) for j in W]
            x = solve([a for a, _ in rows], [beta for _, beta in rows])
            if x is None:
                return dict(none, status=NUMERIC, iters=iters)
            iters += 1
        return dict(none, status=ITERATION_CAP, iters=iters)


def allocate(R, lim, w, xmax, maxit):
    """R [nens][nctl + 1][ncon], w [nobj][nctl]: dict of x, lam [nens][nobj][nctl] (float64), g [nens][nobj], status, iters
    [nens][nobj], work [nens][nobj][nctl] (int32) and nbad, the members with a slot value that is not finite"""
    R = np.asarray(R, dtype=np.float64)
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    nens, n, nobj = len(R), R.shape[1] - 1, len(w)
    out = dict(x=np.zeros((nens, nobj, n)), lam=np.zeros((nens, nobj, n)), g=np.zeros((nens, nobj)), status=np.zeros((nens, nobj), np.int32),
               iters=np.zeros((nens, nobj), np.int32), work=np.zeros((nens, nobj, n), np.int32), nbad=0)
    for m in range(nens):
        for o in range(nobj):
            one = solve_one(R[m], lim, w[o], xmax, maxit)
            for key in ("x", "lam", "g", "status", "iters", "work"):
                out[key][m, o] = one[key]
        out["nbad"] += int(out["status"][m, 0] == INVALID)
    return out


def patterns(x, status):
    """the rate patterns [nens nobj][nctl] of the reliability stage: x where the status is OPTIMAL, +0.0 elsewhere"""
    nens, nobj, n = x.shape
    return np.where((status == OPTIMAL)[:, :, None], x, 0.0).reshape(nens * nobj, n)


def select(quant, g, x):
    """value [nq][npat], best [nq][nobj] (int32), best_x [nq][nobj][nctl] of the reliability stage from quant [nq][nens nobj]"""
    quant = np.asarray(quant, dtype=np.float64)
    nens, nobj, n = x.shape
    nq = len(quant)
    gf, xf = np.asarray(g, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).reshape(nens * nobj, n)
    value = np.zeros((nq, nens * nobj))
    best = np.full((nq, nobj), -1, np.int32)
    best_x = np.full((nq, nobj, n), np.nan)
    with np.errstate(all="ignore"):
        for iq in range(nq):
            for p in range(nens * nobj):
                value[iq, p] = quant[iq, p] * gf[p]
            for o in range(nobj):
                at, top = -1, None
                for m in range(nens):
                    v = value[iq, m * nobj + o]
                    if not np.isnan(v) and (at < 0 or v > top):
                        at, top = m * nobj + o, v
                best[iq, o] = at
                if at >= 0:
                    for c in range(n):
                        best_x[iq, o, c] = quant[iq, at] * xf[at, c]
    return value, best, best_x
