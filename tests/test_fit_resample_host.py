"""The host side of resampled fits (ucf_fit_resample_blocks, ucf_fit_resample_jackknife, ucf_fit_resample_cov, the refusals of
ucf_fit_set_resample, ucf_fit_evaluate_resampled, ucf_fit_objective_resampled, ucf_fit_lm_resampled and
ucf_debug_fit_reduce_resampled) and the CPU tests of tests/fit_resample_restate.py, the numpy restatement that
tests/test_gpu_fit_resample_edges.py and tests/test_gpu_fit_resample.py hold the device to bit for bit.  No GPU.

The contract is the text of include/ucf.h at ucf_fit_set_resample.  The refusals that need a fit object (a set_of or a rep out of
range, a replicate named without attached multiplicities) are in tests/test_gpu_fit_resample.py: a fit cannot be made without a
device.

ucf_fit_resample_cov against np.longdouble (u = 2^-53, first order).  x = log(theta) is taken as the host's log gives it, so the
reference starts from the same x.  mean_j: n - 1 additions and one division, |error| <= n u max|partial sum| <= n u S_j with
S_j = sum |x_rj|.  A deviation d = x - mean then carries u |d| + n u S_j absolutely; a product of two, u |d d'| + (|d| + |d'|) n u
S; the sum of n of them adds n u sum |d d'|; the final division or product two more roundings (the factor (n - 1) / n one of its
own).  With D_j = max_r |d_rj| + n u S_j the bound used is
    |cov_jk - exact| <= u * ((n + 4) * T_jk + 2 n (D_j S_k + D_k S_j) n) * factor,   T_jk = sum_r |d_rj d_rk|,
which is loose by the factor n on the mean's term and still of the order of 1e-13 relative on these inputs."""
import ctypes as C

import numpy as np
import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
import fit_resample_restate as frs
from test_fit_loss_host import bad, status_of
from unconfined_amd import abi
from unconfined_amd import fit as ufit
from unconfined_amd import lib as ucflib

U = 2.0 ** -53
SOURCE_NAMES = sorted(fr.SOURCES, key=fr.SOURCES.get)
KIND_NAMES = sorted(frs.KINDS, key=frs.KINDS.get)
NOBS_GPU = (1, 63, 64, 65, 255, 256, 257, 513)


def test_signatures_are_present():
    so = ucflib.load()
    for name in ("ucf_fit_set_resample", "ucf_fit_evaluate_resampled", "ucf_fit_objective_resampled", "ucf_fit_lm_resampled",
                 "ucf_fit_resample_blocks", "ucf_fit_resample_jackknife", "ucf_fit_resample_cov", "ucf_debug_fit_reduce_resampled"):
        assert name in ucflib.EXPORTS and getattr(so, name).argtypes is not None, name
    assert len(so.ucf_fit_evaluate_resampled.argtypes) == 15
    assert len(so.ucf_fit_objective_resampled.argtypes) == 12
    assert len(so.ucf_fit_lm_resampled.argtypes) == 12
    assert len(so.ucf_debug_fit_reduce_resampled.argtypes) == 2 + 23 + 8
    assert (abi.RESAMPLE_BOOTSTRAP, abi.RESAMPLE_JACKKNIFE) == (0, 1)
    for name in ("set_resample", "evaluate_resampled", "objective_resampled", "lm_resampled", "bootstrap"):
        assert callable(getattr(ufit.Fit, name))


# ---- the block bootstrap

@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1, 0x123456789ABCDEF])
def test_blocks_are_the_pure_python_restatement_bit_for_bit(seed):
    rng = np.random.default_rng(5)
    for nobs, block in ((1, None), (7, None), (300, None), (12, [0, 0, 1, 1, 2, 2, 3, 3, 0, 1, 2, 3]), (257, rng.permutation(np.arange(257) % 9))):
        got = ufit.resample_blocks(nobs, 5, block=block, seed=seed)
        want = frs.blocks_restate(nobs, block, 5, seed)
        assert got.dtype == np.uint16 and got.shape == (5, nobs)
        assert (got.astype(np.int64) == want).all(), (nobs, seed)


def test_blocks_row_sums_and_members():
    mult = ufit.resample_blocks(500, 40, seed=3).astype(np.int64)
    assert (mult.sum(axis=1) == 500).all()                   # iid: nobs draws, each adds one
    assert (mult == 0).any() and (mult > 1).any()
    block = np.arange(500) % 7
    mult = ufit.resample_blocks(500, 40, block=block, seed=3).astype(np.int64)
    for b in range(7):
        assert (mult[:, block == b] == mult[:, block == b][:, :1]).all()         # the members of a block stay equal
    assert (mult[:, :7].sum(axis=1) == 7).all()              # one member per block: 7 draws
    # one stream for the whole call: the first replicates of a longer call are those of a shorter one
    assert (ufit.resample_blocks(500, 3, block=block, seed=3) == mult[:3]).all()
    assert not (ufit.resample_blocks(500, 3, block=block, seed=4) == mult[:3]).all()


def test_jackknife_rows():
    mult = ufit.resample_jackknife(6)
    assert mult.dtype == np.uint16 and (mult == 1 - np.eye(6, dtype=np.uint16)).all()
    block = np.array([2, 0, 1, 1, 0, 2, 2], np.int32)
    mult = ufit.resample_jackknife(7, block)
    assert mult.shape == (3, 7)
    for b in range(3):
        assert (mult[b] == (block != b)).all()


def longdouble_cov(kind, x, use):
    L = np.longdouble
    xs = x[use].astype(L)
    n = len(xs)
    mean = xs.sum(axis=0) / L(n)
    d = xs - mean
    c = d.T @ d
    cov = c / L(n - 1) if kind == "bootstrap" else c * (L(n - 1) / L(n))
    S = np.abs(xs).sum(axis=0)
    D = np.abs(d).max(axis=0) + n * U * S
    T = np.abs(d).T @ np.abs(d)
    factor = 1.0 / (n - 1) if kind == "bootstrap" else (n - 1) / n
    bound = U * ((n + 4) * T + 2.0 * n * n * (np.outer(D, S) + np.outer(S, D))) * factor
    return mean, cov, n * U * S, bound


@pytest.mark.parametrize("kind", ["bootstrap", "jackknife"])
def test_resample_cov_against_longdouble(kind):
    rng = np.random.default_rng(9)
    for n, P in ((2, 1), (5, 3), (200, 8), (1024, 4)):
        Lc = rng.normal(size=(P, P)) * 0.1
        thetas = np.exp(rng.normal(size=(n, P)) @ Lc.T + rng.uniform(-8.0, 3.0, P))
        use = np.ones(n, bool)
        if n > 4:
            use[rng.integers(0, n, n // 5)] = False
            thetas[np.flatnonzero(~use)[0]] = np.nan             # an unused replicate is not read
        got = ufit.resample_cov(kind, thetas, use.astype(np.int32))
        mean, cov, mb, cb = longdouble_cov(kind, np.log(np.where(use[:, None], thetas, 1.0)), use)
        assert got["nused"] == int(use.sum())
        assert (np.abs(got["mean"].astype(np.longdouble) - mean) <= mb).all(), (n, P)
        assert (np.abs(got["cov"].astype(np.longdouble) - cov) <= cb).all(), (n, P)
        assert (got["cov"] == got["cov"].T).all() and (np.diag(got["cov"]) > 0).all()
        if use.all():
            assert got["cov"].tobytes() == ufit.resample_cov(kind, thetas)["cov"].tobytes()      # use NULL: all
    # the two kinds differ by the factor alone
    th = np.exp(rng.normal(size=(10, 2)))
    a, b = ufit.resample_cov("bootstrap", th)["cov"], ufit.resample_cov("jackknife", th)["cov"]
    assert np.allclose(b, a * 9.0 * 9.0 / 10.0, rtol=1e-14)


def test_resample_cov_states_its_operation_order():
    """the header's order, one rounded operation at a time"""
    rng = np.random.default_rng(2)
    th = np.exp(rng.normal(size=(37, 3)))
    x = np.log(th)
    n = len(x)
    mean = np.zeros(3)
    for j in range(3):
        s = np.float64(0.0)
        for r in range(n):
            s = s + x[r, j]
        mean[j] = s / np.float64(n)
    cov = np.zeros((3, 3))
    for j in range(3):
        for k in range(j, 3):
            c = np.float64(0.0)
            for r in range(n):
                c = c + (x[r, j] - mean[j]) * (x[r, k] - mean[k])
            cov[j, k] = cov[k, j] = c * (np.float64(n - 1) / np.float64(n))
    got = ufit.resample_cov("jackknife", th)
    # log is the host library's: the mean and cov follow bit for bit from the x it gives where numpy's log agrees with it
    lib_x = np.log(th)
    assert lib_x.tobytes() == x.tobytes()
    if got["mean"].tobytes() == mean.tobytes():
        assert got["cov"].tobytes() == cov.tobytes()
    else:                                                     # a libm whose log differs from numpy's in the last bit
        assert np.allclose(got["mean"], mean, rtol=0, atol=4 * U * np.abs(x).sum(axis=0))


# ---- refusals, none of which needs a device

def test_host_entries_refuse_bad_arguments():
    so = ucflib.load()
    bad(lambda: ufit.resample_blocks(0, 3), "nobs=0")
    bad(lambda: ufit.resample_blocks(2 ** 24 + 1, 1), "nobs=")
    bad(lambda: ufit.resample_blocks(5, 0), "nrep=0")
    bad(lambda: ufit.resample_blocks(5, 65537), "nrep=65537")
    bad(lambda: ufit.resample_blocks(4, 2, block=[0, 1, -1, 0]), "block[2]")
    bad(lambda: ufit.resample_blocks(4, 2, block=[0, 1, 4, 0]), "block[2]")
    bad(lambda: ufit.resample_blocks(4, 2, block=[0, 3, 3, 0]), "block id 1")
    bad(lambda: ufit.resample_jackknife(0), "nobs=0")
    bad(lambda: ufit.resample_jackknife(3, [0, 2, 2]), "block id 1")
    assert so.ucf_fit_resample_jackknife(3, None, None) == abi.UCF_ERR_BAD_ARGUMENT
    nb = C.c_int()
    assert so.ucf_fit_resample_blocks(6, np.array([0, 1, 1, 0, 2, 2], np.int32).ctypes.data, 1, 0, None, C.addressof(nb)) == 0 and nb.value == 3
    # (a count beyond 65535 needs one of more than 65535 blocks drawn more than 65535 times in as many draws: the refusal is
    # there for the type's sake and no seed reaches it.)  Many observations in few blocks: as many draws as blocks
    block = np.zeros(2 ** 17, np.int32)
    block[-1] = 1
    assert ufit.resample_blocks(2 ** 17, 3, block=block).astype(np.int64).sum(axis=1).max() <= 2 * 2 ** 17
    assert ufit.resample_blocks(2 ** 17, 3, block=block).max() <= 2
    th = np.ones((3, 2))
    bad(lambda: ufit.resample_cov(2, th), "kind=2")
    bad(lambda: ufit.resample_cov("bootstrap", th[:1]), "at least two")
    bad(lambda: ufit.resample_cov("bootstrap", th, [1, 0, 0]), "at least two")
    bad(lambda: ufit.resample_cov("jackknife", np.ones((3, 9))), "npar=9")
    bad(lambda: ufit.resample_cov("jackknife", np.array([[1.0, 2.0], [1.0, -2.0], [1.0, 1.0]])), "replicate 1: parameter 1")
    bad(lambda: ufit.resample_cov("jackknife", np.array([[1.0, 2.0], [1.0, 2.0], [np.inf, 1.0]])), "replicate 2: parameter 0")
    assert so.ucf_fit_resample_cov(0, 3, 2, None, None, None, None, None) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_resample_cov(0, 0, 2, th.ctypes.data, None, None, None, None) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_resample_cov(0, 3, 2, th.ctypes.data, None, None, None, None) == 0           # every output may be NULL
    # the entries on a fit: the NULL fit comes first
    m = np.ones((2, 3), np.uint16)
    x = np.ones(3)
    assert so.ucf_fit_set_resample(None, 2, m.ctypes.data) == abi.UCF_ERR_BAD_ARGUMENT and b"NULL" in so.ucf_last_error()
    assert so.ucf_fit_evaluate_resampled(None, 1, x.ctypes.data, 1e-3, 1, *([None] * 10)) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_objective_resampled(None, 1, x.ctypes.data, 1, *([None] * 8)) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_lm_resampled(None, 1, x.ctypes.data, None, None, *([None] * 7)) == abi.UCF_ERR_BAD_ARGUMENT


def accepted(inp, kind, c, mult, set_of, rep):
    """passes every check: without a GPU the answer is UCF_ERR_NO_DEVICE, with one the call succeeds"""
    import torch
    if torch.cuda.is_available():
        assert (frs.debug_fit_reduce_resampled(inp, kind, c, mult, set_of, rep)["nbad"] >= 0).all()
        return
    status, message = status_of(lambda: frs.debug_fit_reduce_resampled(inp, kind, c, mult, set_of, rep))
    assert status == abi.UCF_ERR_NO_DEVICE, message


def test_the_debug_entry_refuses_before_it_needs_a_device():
    slots, _ = fr.synthetic(fr.SLOTS, 2, True, 65, 2)
    net, _ = fr.synthetic(fr.NETWORK, 2, False, 65, 2)
    mult = frs.gpu_mult(65)
    no = lambda word, inp=slots, kind=frs.TUKEY, c=2.0, mult=mult, set_of=frs.SET_OF, rep=frs.REP, **kw: bad(
        lambda: frs.debug_fit_reduce_resampled(inp, kind, c, mult, set_of, rep, **kw), word)
    no("kind=3", kind=3)
    no("kind=-1", kind=-1)
    for c in (0.0, -2.0, np.nan, np.inf):
        no("c=", kind=frs.HUBER, c=c)
        no("c=", kind=frs.TUKEY, c=c, inp=net)
    no("nrep=", nrep=-1)
    no("nrep=", nrep=65537)
    no("NULL mult", mult=None, nrep=4)
    no("nred=0", nred=0)
    no("nred=65537", nred=65537)
    no("exceeds nsets", set_of=None, rep=[-1, -1, -1])
    no("set_of[2]", set_of=[1, 0, 2, 1, 0])
    no("set_of[4]", set_of=[1, 0, 1, 1, -1])
    no("rep[1]", rep=[-1, 4, 2, 1, 3])
    no("rep[0]", rep=[-2, 0, 2, 1, 3])
    no("rep[3]", mult=None, rep=[-1, -1, -1, 0, -1])           # no multiplicities: only -1 is legal
    no("counts", inp={**slots, "null_counts": True})
    no("sums", inp={**slots, "null_sums": True})
    heavy = np.zeros((1, 65), np.uint16)
    heavy[0, :] = 65535
    accepted(slots, frs.HUBER, 2.0, heavy, [0], [0])           # 65 x 65535 lies within an int
    # the checks of ucf_debug_fit_reduce, inherited
    no("slot[7]", inp={**slots, "slot": np.where(np.arange(65) == 7, slots["plan_stride"], slots["slot"]).astype(np.int32)})
    no("plan_stride", inp={**slots, "plan_stride": 0})
    no("beyond h", inp={**net, "nh": 1})
    # and what passes: least squares (c is not read), no multiplicities with every rep -1, NULL set_of and rep
    accepted(slots, frs.L2, np.nan, mult, frs.SET_OF, frs.REP)
    accepted(net, frs.TUKEY, 2.0, None, [1, 0, 0], [-1, -1, -1])
    accepted(net, frs.HUBER, 2.0, mult, None, None)


def test_a_row_that_overflows_the_counts_is_refused():
    nobs = 2 ** 15 + 1
    inp, _ = fr.synthetic(fr.SLOTS, 0, False, nobs, 1)
    mult = np.full((2, nobs), 65535, np.uint16)
    mult[0] = 1
    bad(lambda: frs.debug_fit_reduce_resampled(inp, frs.L2, 0.0, mult, [0], [1]), "replicate 1")


# ---- the restatement

@pytest.mark.parametrize("kind", ["huber", "tukey"])
@pytest.mark.parametrize("source", SOURCE_NAMES)
def test_restatement_with_unit_multiplicities_is_the_loss_restatement(kind, source):
    for npar, deriv, nobs in ((0, True, 65), (2, False, 257), (3, True, 300)):
        inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, 2)
        want = fl.restate(inp, fl.KINDS[kind], fl.C_GPU)
        ones = np.ones((1, nobs), np.uint16)
        for mult, rep in ((None, [-1, -1]), (ones, [0, 0]), (ones, None)):
            got = frs.restate(inp, frs.KINDS[kind], fl.C_GPU, mult, [0, 1], rep)
            assert np.ascontiguousarray(got["sums"][:, :-1]).tobytes() == want["sums"].tobytes(), (kind, source, npar)
            assert (got["sums"][:, -1] == 0.0).all() and not np.signbit(got["sums"][:, -1]).any()
            assert (got["nbad"] == want["nbad"]).all() and (got["counts"][:, 3] == want["ndown"]).all()
            assert (got["counts"][:, 0] == want["counted"].sum(axis=1)).all() and (got["counts"][:, 1] == want["weighted"].sum(axis=1)).all()
            assert (got["counts"][:, 2] == 0).all()


@pytest.mark.parametrize("source", SOURCE_NAMES)
def test_restatement_under_least_squares_is_the_plain_restatement(source):
    for npar, deriv, nobs in ((0, False, 64), (4, True, 257)):
        inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, 2)
        want = fr.restate(inp)
        got = frs.restate(inp, frs.L2, 0.0, None, None, [-1, -1])
        n = fr.nsums(npar, deriv)
        assert np.ascontiguousarray(got["sums"][:, :n]).tobytes() == want["sums"].tobytes()
        assert got["sums"][:, n].tobytes() == want["sums"][:, 0].tobytes()          # phi_w has the bits of phi
        assert (got["nbad"] == want["nbad"]).all() and (got["counts"][:, 3] == 0).all()


def test_restatement_of_the_gpu_rows():
    """what the rows of the GPU cases are for: held-out observations go to phi_out and nheld alone, a held-out observation that is
    not finite to no count, an all-zero row gives +0.0 in every sum but phi_out, a multiplicity scales a term"""
    for nobs in NOBS_GPU:
        inp, _ = fr.synthetic(fr.SLOTS, 2, True, nobs, 2)
        mult = frs.gpu_mult(nobs)
        assert (mult[0] == 1).all() and (mult[3] == 0).all() and mult[2].max() == 65535 and (nobs == 1 or (mult[1] == 0).any())
        got = frs.restate(inp, frs.TUKEY, frs.C_GPU, mult, frs.SET_OF, frs.REP)
        full = fl.restate(inp, fl.TUKEY, frs.C_GPU)
        for r, (s, p) in enumerate(zip(frs.SET_OF, frs.REP)):
            m = np.ones(nobs, np.int64) if p < 0 else mult[p].astype(np.int64)
            ok = full["counted"][s]
            assert got["nbad"][r] == int((~ok & (m > 0)).sum())
            assert got["counts"][r, 2] == int((ok & (m == 0)).sum())                 # held out and not finite: in no count
            assert got["counts"][r, 0] == int(m[ok].sum())
            assert got["nbad"][r] + got["counts"][r, 2] + int((ok & (m > 0)).sum()) + int((~ok & (m == 0)).sum()) == nobs
        last = got["sums"][4]
        assert (last[:-1] == 0.0).all() and not np.signbit(last[:-1]).any() and got["counts"][4, 0] == 0 and got["nbad"][4] == 0
        if nobs > 12:
            assert last[-1] > 0.0
    # one observation twice is that term twice: phi doubles exactly, g and A too (a power of two)
    inp, _ = fr.synthetic(fr.NETWORK, 2, False, 64, 1)
    one = frs.restate(inp, frs.HUBER, frs.C_GPU, np.ones((1, 64), np.uint16), [0], [0])
    two = frs.restate(inp, frs.HUBER, frs.C_GPU, np.full((1, 64), 2, np.uint16), [0], [0])
    assert (two["sums"][:, :-1] == 2.0 * one["sums"][:, :-1]).all() and (two["counts"][:, 0] == 2 * one["counts"][:, 0]).all()
    assert (two["counts"][:, 3] == one["counts"][:, 3]).all()                        # ndown counts an observation once
