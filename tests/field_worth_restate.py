"""The arithmetic of ucf_field_worth as include/ucf.h states it, restated in numpy: the kernel, the targets, the pick and the
conditioning, one rounded operation per statement.  Everything is elementwise on float64 arrays (one element per candidate; a
0-d array for the host functions), and numpy's +, -, *, / and sqrt on float64 are the correctly rounded IEEE operations: no
contraction, no reassociation.  The tests hold the library to these functions; nothing here calls the library."""
import numpy as np

U = 2.0 ** -53


def cholesky(cov):
    """the lower factor of ucf_field_ensemble_draw, the upper triangle +0.0; None where a pivot is not positive and finite"""
    n = len(cov)
    L = np.array(cov, dtype=np.float64)
    for j in range(n):
        d = L[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not (d > 0.0 and np.isfinite(d)):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            v = L[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    return np.tril(L)


def jac(a, two_dlog):
    """a [1 + 2 npar, ...] -> J [npar, ...] and ok [...]: every one of the 2 npar perturbed slot values is finite"""
    npar = (len(a) - 1) // 2
    with np.errstate(invalid="ignore", over="ignore"):
        J = [(a[1 + 2 * j] - a[2 + 2 * j]) / two_dlog for j in range(npar)]
    return J, np.isfinite(a[1:]).all(axis=0)


def ftj(F, J):
    """g = F' J: g_j = +0.0; g_j = g_j + F[i][j] * J_i, i ascending"""
    n = len(F)
    g = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(n):
            acc = np.zeros_like(J[0])
            for i in range(n):
                acc = acc + F[i, j] * J[i]
            g.append(acc)
    return g


def start(n, like):
    return [[np.full_like(like, 1.0 if i == j else 0.0) for j in range(i + 1)] for i in range(n)]


def add_datum(B, F, J, ok, w):
    """B_ij = B_ij + (w g_i)(w g_j), i >= j, where ok"""
    n = len(F)
    with np.errstate(invalid="ignore", over="ignore"):
        wg = [w * g for g in ftj(F, J)]
        for i in range(n):
            for j in range(i + 1):
                B[i][j] = np.where(ok, B[i][j] + wg[i] * wg[j], B[i][j])


def ldl(B):
    """B = L D L' without square roots: l (strict lower triangle), d"""
    n = len(B)
    l = [[None] * n for _ in range(n)]
    d = [None] * n
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(n):
            v = B[j][j]
            for k in range(j):
                v = v - (l[j][k] * l[j][k]) * d[k]
            d[j] = v
            for i in range(j + 1, n):
                v = B[i][j]
                for k in range(j):
                    v = v - (l[i][k] * l[j][k]) * d[k]
                l[i][j] = v / d[j]
    return l, d


def kernel(a_s, a_d, two_dlog, F, ws, wd, tsel, A, tw):
    """field_worth_kernel: a_s, a_d [1 + 2 npar, nt, ncand] (a_d None ok where wd == 0), F [npar, npar], tsel [nt] or None, A
    [ntgt, npar], tw [ntgt] or None -> post [ntgt, ncand], crit [ncand], nused [ncand] (int32)"""
    a_s = np.asarray(a_s, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    n, nt, ncand = len(F), a_s.shape[1], a_s.shape[2]
    ntgt = len(A)
    tw = np.ones(ntgt) if tw is None else np.asarray(tw, dtype=np.float64)
    B = start(n, a_s[0, 0])
    nused = np.zeros(ncand, np.int32)
    for k in range(nt):
        if tsel is not None and tsel[k] == 0:
            continue
        for a, w in ((a_s, ws), (a_d, wd)):
            if not w > 0.0:
                continue
            J, ok = jac(np.asarray(a, dtype=np.float64)[:, k, :], two_dlog)
            nused = nused + ok.astype(np.int32)
            add_datum(B, F, J, ok, np.float64(w))
    l, d = ldl(B)
    good = np.ones(ncand, bool)
    for j in range(n):
        good = good & (d[j] > 0.0) & np.isfinite(d[j])
    post = np.zeros((ntgt, ncand))
    crit = np.zeros(ncand)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(ntgt):
            v = np.zeros(ncand)
            y = [None] * n
            for j in range(n):
                yj = np.full(ncand, A[t, j])
                for k in range(j):
                    yj = yj - l[j][k] * y[k]
                y[j] = yj
                v = v + (yj * yj) / d[j]
            post[t] = np.where(good, v, np.nan)
            crit = crit + tw[t] * post[t]
    return post, crit, nused


def targets(F, Jt, ok):
    """A [ntgt, npar] and prior [ntgt] of the targets with sensitivities Jt [ntgt, npar]; a target that is not ok: NaN"""
    F = np.asarray(F, dtype=np.float64)
    n = len(F)
    A = np.zeros((len(Jt), n))
    prior = np.zeros(len(Jt))
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(Jt)):
            g = ftj(F, [np.float64(v) for v in Jt[t]])
            p = np.float64(0.0)
            for j in range(n):
                A[t, j] = g[j] if ok[t] else np.nan
                p = p + A[t, j] * A[t, j]
            prior[t] = p
    return A, prior


def pick(crit, cmask=None, taken=()):
    """the allowed, unpicked candidate of least finite crit, the lowest index on a tie; -1: none"""
    best = -1
    crit = np.asarray(crit).ravel()
    for c, v in enumerate(crit):
        if (cmask is None or cmask[c] != 0) and c not in taken and np.isfinite(v) and (best < 0 or v < crit[best]):
            best = c
    return best


def condition(F, J, w):
    """ucf_worth_condition: F_out, cov_out (and B's l, d for the tests)"""
    F = np.asarray(F, dtype=np.float64)
    n = len(F)
    J = np.asarray(J, dtype=np.float64).reshape(-1, n)
    B = start(n, np.float64(0.0))
    for r in range(len(J)):
        add_datum(B, F, [np.float64(v) for v in J[r]], True, np.float64(w[r]))
    l, d = ldl(B)
    X = np.zeros((n, n))
    F_out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            x = F[i, j]
            for k in range(j):
                x = x - X[i, k] * l[j][k]
            X[i, j] = x
    for i in range(n):
        for j in range(n):
            F_out[i, j] = X[i, j] / np.sqrt(d[j])
    cov_out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            acc = np.float64(0.0)
            for k in range(n):
                acc = acc + F_out[i, k] * F_out[j, k]
            cov_out[i, j] = acc
    return F_out, cov_out


def dense_B(F, J, w):
    """I + sum (w F'j)(w F'j)' as a matrix, by numpy: for condition numbers and textbook solves, not part of the restatement"""
    F = np.asarray(F, dtype=np.float64)
    G = (np.asarray(J, dtype=np.float64).reshape(-1, len(F)) @ F) * np.asarray(w, dtype=np.float64).reshape(-1, 1)
    return np.eye(len(F)) + G.T @ G


def rows_of(a_s, a_d, two_dlog, ws, wd, tsel, c):
    """the used data of candidate c in kernel order: J [nrow, npar], w [nrow]"""
    J, w = [], []
    for k in range(a_s.shape[1]):
        if tsel is not None and tsel[k] == 0:
            continue
        for a, wk in ((a_s, ws), (a_d, wd)):
            if not wk > 0.0:
                continue
            Jk, ok = jac(np.asarray(a, dtype=np.float64)[:, k, c], two_dlog)
            if ok:
                J.append([float(v) for v in Jk])
                w.append(wk)
    return np.array(J, dtype=np.float64).reshape(len(w), (len(a_s) - 1) // 2), np.array(w, dtype=np.float64)


def worth(s_all, ds_all, dlog, cov, sigma_s, sigma_d, tsel, tgt, tw, npick, cmask=None):
    """ucf_field_worth on the slots s_all, ds_all [1 + 2 npar, nt, nloc, nz] of a forecast: a dict with prior [npick, ntgt], post
    [npick, ntgt, ncand], crit [npick, ncand], nused [ncand], pick [npick], cov_post, and F, the factor of every round"""
    nset, nt = s_all.shape[:2]
    npar = (nset - 1) // 2
    a_s, a_d = s_all.reshape(nset, nt, -1), ds_all.reshape(nset, nt, -1)
    ncand = a_s.shape[2]
    nloc, nz = s_all.shape[2], s_all.shape[3]
    two_dlog = np.float64(2.0) * np.float64(dlog)
    ws = np.float64(1.0) / np.float64(sigma_s)
    wd = np.float64(1.0) / np.float64(sigma_d) if sigma_d > 0.0 else 0.0
    F = cholesky(cov)
    assert F is not None
    Jt, ok = [], []
    for kind, k, i, z in tgt:
        J, good = jac((a_d if kind else a_s)[:, k, i * nz + z], two_dlog)
        Jt.append([float(v) for v in J])
        ok.append(bool(good))
    ntgt = len(tgt)
    out = dict(prior=np.full((npick, ntgt), np.nan), post=np.full((npick, ntgt, ncand), np.nan), crit=np.full((npick, ncand), np.nan),
               nused=None, pick=np.full(npick, -1, np.int32), F=[])
    taken = []
    for r in range(npick):
        out["F"].append(F.copy())
        A, out["prior"][r] = targets(F, Jt, ok)
        out["post"][r], out["crit"][r], nused = kernel(a_s, a_d, two_dlog, F, ws, wd, tsel, A, tw)
        if r == 0:
            out["nused"] = nused
        best = pick(out["crit"][r], cmask, taken)
        if best < 0:
            break
        out["pick"][r] = best
        taken.append(best)
        J, w = rows_of(a_s, a_d, two_dlog, ws, wd, tsel, best)
        F, _ = condition(F, J, w)
    out["F_last"] = F
    out["cov_post"] = condition(F, np.zeros((0, npar)), np.zeros(0))[1]
    return out
