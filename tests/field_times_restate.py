"""field_times_kernel (unconfined_amd/csrc/ucf_field_times.hip) restated in numpy from the arithmetic that include/ucf.h states
with ucf_field_ensemble_times, one rounded fp64 operation at a time, vectorised over the columns (member, site).  Nothing here
is derived from the kernel's source: the statements are

    FIRST_ABOVE   for k ascending, v = a[m][k][e]:  v not finite -> NaN, stop;  v > L -> stop with tau[0] where k == 0, otherwise
                  f = (L - v0) / (v - v0), T = tau[k-1] + f * (tau[k] - tau[k-1]) with v0 = a[m][k-1][e];  no stop -> tau_never.
    LAST_ABOVE    any of the nt values not finite -> NaN;  k* = the last k with a[m][k][e] > L:  none -> tau[0];  k* == nt-1 ->
                  tau_never;  otherwise f = (v0 - L) / (v0 - v1), T = tau[k*] + f * (tau[k*+1] - tau[k*]), v0 = a[k*], v1 = a[k*+1].

Used by tests/test_field_times_host.py and tests/test_gpu_field_times.py."""
import numpy as np

FIRST_ABOVE, LAST_ABOVE = 0, 1


def first_above(a, tau, tau_never, L):
    """a [nens][nt][nsite] -> T [nens][nsite]"""
    a = np.asarray(a, dtype=np.float64)
    nens, nt, nsite = a.shape
    L = np.float64(L)
    T = np.full((nens, nsite), np.float64(tau_never))
    open_ = np.ones((nens, nsite), bool)                 # the walk of the column has not stopped
    with np.errstate(all="ignore"):
        for k in range(nt):
            v = a[:, k, :]
            bad = open_ & ~np.isfinite(v)
            T[bad] = np.nan
            open_ &= ~bad
            hit = open_ & (v > L)
            if k == 0:
                T[hit] = tau[0]
            else:
                v0 = a[:, k - 1, :]
                f = (L - v0) / (v - v0)
                step = np.float64(tau[k]) - np.float64(tau[k - 1])
                prod = f * step
                T = np.where(hit, np.float64(tau[k - 1]) + prod, T)
            open_ &= ~hit
    return T


def last_above(a, tau, tau_never, L):
    """a [nens][nt][nsite] -> T [nens][nsite]"""
    a = np.asarray(a, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    nens, nt, nsite = a.shape
    L = np.float64(L)
    bad = ~np.isfinite(a).all(axis=1)
    above = a > L
    ks = np.where(above.any(axis=1), nt - 1 - np.argmax(above[:, ::-1, :], axis=1), -1)      # the last k above; -1: none
    inner = (ks >= 0) & (ks < nt - 1)
    k0 = np.clip(ks, 0, max(nt - 2, 0))
    k1 = np.minimum(k0 + 1, nt - 1)
    with np.errstate(all="ignore"):
        v0 = np.take_along_axis(a, k0[:, None, :], axis=1)[:, 0, :]
        v1 = np.take_along_axis(a, k1[:, None, :], axis=1)[:, 0, :]
        f = (v0 - L) / (v0 - v1)
        step = tau[k1] - tau[k0]
        prod = f * step
        T = tau[k0] + prod
    T = np.where(inner, T, np.where(ks < 0, tau[0], np.float64(tau_never)))
    return np.where(bad, np.nan, T)


def times(a, tau, tau_never, limit, kind):
    """T [nens][nlim][nsite] of a [nens][nt][nsite] (any trailing shape of the sites is kept: a [nens][nt][...] gives
    T [nens][nlim][...])"""
    a = np.asarray(a, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    shape = a.shape[2:]
    v = a.reshape(a.shape[0], a.shape[1], -1)
    assert len(tau) == v.shape[1] and len(limit) == len(kind)
    rows = [(first_above if int(k) == FIRST_ABOVE else last_above)(v, tau, tau_never, L) for L, k in zip(limit, kind)]
    return np.stack(rows, axis=1).reshape((a.shape[0], len(limit)) + shape)
