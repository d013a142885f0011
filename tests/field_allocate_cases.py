"""Programmes for the tests of ucf_field_allocate, shared by tests/test_field_allocate_host.py and tests/test_gpu_field_allocate.py
(so that the host test holds ucf_allocate_solve to the restatement on everything the kernel test uses), and the ctypes calls of
the two entries on caller data."""
import ctypes as C

import numpy as np

NCONS = (1, 63, 64, 65, 255, 256, 257, 1000)
MAXIT = 64


def addr(a):
    return a.ctypes.data if a is not None else None


def generic(nctl, ncon, seed, nens=1):
    """R [nens][nctl + 1][ncon], limits, w [2][nctl], xmax: responses mostly positive (a few recharge images: negative), room > 0,
    the first objective the total abstraction, the second with weights of both signs"""
    rng = np.random.default_rng(seed)
    R = np.zeros((nens, nctl + 1, ncon))
    R[:, :nctl] = rng.uniform(0.05, 1.0, (nens, nctl, ncon)) * rng.choice([-1.0, 1.0], (nens, nctl, ncon), p=[0.1, 0.9])
    R[:, nctl] = rng.uniform(0.0, 0.5, (nens, ncon))
    lim = 1.0 + rng.uniform(0.0, 1.0, ncon)
    w = np.ones((2, nctl))
    w[1] = rng.uniform(-0.5, 1.5, nctl)
    xmax = rng.uniform(0.5, 3.0, nctl)
    return R, lim, w, xmax


def kernel_case(nctl, ncon):
    """what the kernel test launches per (nctl, ncon): three members -- one clean, one with a NaN slot, one with a negative room --
    and two objectives"""
    R, lim, w, xmax = generic(nctl, ncon, 1000 * nctl + ncon, nens=3)
    R[1, nctl // 2, ncon // 2] = np.nan
    R[2, nctl, ncon - 1] = lim[ncon - 1] + 0.25
    return R, lim, w, xmax


def degenerate_cases():
    """(name, R [1][nctl + 1][ncon], lim, w [nobj][nctl], xmax): duplicated rows -- the lowest id enters --, rows through a
    corner of the box -- nctl + 1 constraints meet in a point --, and a row through the origin"""
    cases = []
    # two controls, rows 1 and 3 equal and the tightest
    R = np.array([[[1.0, 0.5, 0.25, 0.5, 0.125], [0.5, 1.0, 0.25, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]]])
    lim = np.array([4.0, 1.0, 8.0, 1.0, 16.0])
    cases.append(("duplicated rows", R, lim, np.array([[1.0, 1.0], [1.0, 3.0]]), np.array([3.0, 3.0])))
    # x0 + x1 <= 2 passes through the corner (1, 1) of the box [0, 1]^2; so does 2 x0 + x1 <= 3
    R = np.array([[[1.0, 2.0, 0.25], [1.0, 1.0, 0.25], [0.5, 0.5, 0.0]]])
    lim = np.array([2.5, 3.5, 9.0])
    cases.append(("corner of the box", R, lim, np.array([[1.0, 1.0], [2.0, 1.0], [1.0, 2.0]]), np.array([1.0, 1.0])))
    # three controls: four rows and the three upper bounds meet in (1, 1, 1)
    R = np.zeros((1, 4, 4))
    R[0, :3] = np.array([[1.0, 1.0, 0.0, 1.0], [1.0, 0.0, 1.0, 2.0], [1.0, 1.0, 1.0, 0.0]])
    lim = np.array([3.0, 2.0, 2.0, 3.0])
    cases.append(("corner in three dimensions", R, lim, np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 3.0], [3.0, 1.0, 2.0]]), np.array([1.0, 1.0, 1.0])))
    # room == 0 on a row with positive responses: the origin is the optimum of every increasing objective, degenerate from the start
    R = np.array([[[1.0, 0.5], [1.0, 0.25], [2.0, 0.0]]])
    lim = np.array([2.0, 4.0])
    cases.append(("row through the origin", R, lim, np.array([[1.0, 1.0], [1.0, -1.0]]), np.array([2.0, 2.0])))
    # every output twice with numbers that round, as at two depths of a fully penetrating well: the twin of a working row has
    # D = 0 up to rounding noise and must not enter (with D > 0 as the test most of these end NUMERIC on a singular B)
    for nctl in (2, 5, 8):
        R, lim, w, xmax = generic(nctl, 24, 7000 + nctl)
        cases.append((f"every output twice, {nctl} controls", np.repeat(R, 2, axis=2), np.repeat(lim, 2), w, xmax))
    return cases


def outputs(nens, nobj, nctl):
    out = dict(x=np.zeros((nens, nobj, nctl)), g=np.zeros((nens, nobj)), status=np.zeros((nens, nobj), np.int32),
               iters=np.zeros((nens, nobj), np.int32), work=np.zeros((nens, nobj, nctl), np.int32), lam=np.zeros((nens, nobj, nctl)))
    return out


ORDER = ("x", "g", "status", "iters", "work", "lam")


def host_solve(so, R, lim, w, xmax, maxit):
    """ucf_allocate_solve member by member, in the layout of the kernel's outputs"""
    from unconfined_amd import lib as ucflib
    R, lim, w, xmax = (np.ascontiguousarray(a, dtype=float) for a in (R, lim, np.atleast_2d(w), xmax))
    nens, nslot, ncon = R.shape
    nobj, nctl = w.shape
    out = outputs(nens, nobj, nctl)
    out["nbad"] = 0
    for m in range(nens):
        one = outputs(1, nobj, nctl)
        ucflib.check(so.ucf_allocate_solve(nctl, ncon, addr(R[m]), addr(lim), nobj, addr(w), addr(xmax), int(maxit), *(addr(one[k]) for k in ORDER)))
        for k in ORDER:
            out[k][m] = one[k][0]
        out["nbad"] += int(out["status"][m, 0] == -1)
    return out


def debug(so, R, lim, w, xmax, maxit, con=None):
    """one launch of field_allocate_kernel through the library's launcher on caller data"""
    from unconfined_amd import lib as ucflib
    R, lim, w, xmax = (np.ascontiguousarray(a, dtype=float) for a in (R, lim, np.atleast_2d(w), xmax))
    nens, nslot, ncon = R.shape
    nobj, nctl = w.shape
    con = np.arange(ncon, dtype=np.int32) if con is None else np.ascontiguousarray(con, dtype=np.int32)
    out = outputs(nens, nobj, nctl)
    nbad = C.c_longlong(-1)
    ucflib.check(so.ucf_debug_field_allocate(nctl, nens, ncon, nobj, addr(R), addr(lim), addr(con), addr(w), addr(xmax), int(maxit),
                                             *(addr(out[k]) for k in ORDER), C.addressof(nbad)))
    out["nbad"] = int(nbad.value)
    return out


def same_bytes(got, want, what):
    for k in ORDER:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k, got[k].ravel()[:8], want[k].ravel()[:8])
    assert got["nbad"] == want["nbad"], (what, got["nbad"], want["nbad"])
