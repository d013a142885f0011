"""ucf_field_allocate on the GPU: field_allocate_kernel through ucf_debug_field_allocate on synthetic response slots, and the whole
call on the fixtures of tests/test_gpu_field_yield.py (4 wells, 5 locations, 6 times, 2 depths; c1_theis faithful and
neuman74_partpen fast; 3 members), against the host twin ucf_allocate_solve and the numpy restatement of include/ucf.h
(tests/field_allocate_restate.py).

Bounds.  The kernel, the host twin and the restatement hold +, -, * and / only, each rounded on its own, besides the one fma of
the polish, which returns the exact error of a product (the restatement forms it in rational arithmetic), and the ratio test is
defined without order: x, g, status, iters, work, lam and nbad are compared byte for byte (NaN included: all three write the
same quiet NaN).  The reliability stage is the ratio test and the member reduction of ucf_field_yield, held bit for bit to their
restatements, and one product per value on the host.  The one tolerance is where two statements of the same quantity meet: with one
control and w = 1 the programme's x is room / r with room = limit - b held in double-double (the polish of the contract) and
ucf_field_yield's hi is the rounded room over r: at most 1 ulp apart, which is the bound; the test prints which it saw."""
import os

import numpy as np
import pytest

import field_allocate_cases as K
import field_allocate_restate as A
import field_yield_restate as Y
from ensemble_weighted_restate import quantise, restate_weighted
from golden_util import GOLD, load_deck
from test_gpu_field_ensemble import same_bits

pytestmark = pytest.mark.gpu

CASES = [("c1_theis", "faithful"), ("neuman74_partpen", "fast")]
CTL2 = np.array([0, 1, -1, 0], np.int32)
W2 = np.array([[1.0, 1.0], [1.0, 0.25]])
XMAX2 = np.array([4.0, 6.0])
XMAX1 = 2.5
QS = (0.05, 0.5, 1.0)


@pytest.fixture(scope="module")
def so():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import lib as ucflib
    return ucflib.load()


@pytest.fixture(scope="module")
def eng(so):
    from unconfined_amd import engine
    return engine


@pytest.mark.parametrize("nctl", range(1, 9))
def test_kernel_is_the_stated_arithmetic(so, nctl):
    """every instantiation; ncon at the lane, wave and workgroup edges of the stride; a clean member, one with a NaN slot and one
    with a negative room; two objectives; maxit = 1 once"""
    seen = set()
    pivots = 0
    for ncon in K.NCONS:
        R, lim, w, xmax = K.kernel_case(nctl, ncon)
        want = A.allocate(R, lim, w, xmax, K.MAXIT)
        assert want["status"][:, 0].tolist() == [A.OPTIMAL, A.INVALID, A.INFEASIBLE_AT_ZERO] and want["nbad"] == 1, (ncon, want["status"])
        K.same_bytes(K.host_solve(so, R, lim, w, xmax, K.MAXIT), want, ("host", ncon))
        K.same_bytes(K.debug(so, R, lim, w, xmax, K.MAXIT), want, ("kernel", ncon))
        seen |= set(want["status"].ravel().tolist())
        pivots += int(want["iters"].sum())
    R, lim, w, xmax = K.kernel_case(nctl, 257)
    want = A.allocate(R, lim, w, xmax, 1)
    assert want["status"][0, 0] == A.ITERATION_CAP and want["iters"][0, 0] == 1 and np.isnan(want["x"][0, 0]).all()
    K.same_bytes(K.debug(so, R, lim, w, xmax, 1), want, "maxit 1")
    assert seen >= {A.OPTIMAL, A.INVALID, A.INFEASIBLE_AT_ZERO} and pivots >= len(K.NCONS)


def test_degenerate_programmes(so):
    for name, R, lim, w, xmax in K.degenerate_cases():
        want = A.allocate(R, lim, w, xmax, K.MAXIT)
        assert set(want["status"].ravel().tolist()) <= {A.OPTIMAL, A.ITERATION_CAP}, (name, want["status"])
        K.same_bytes(K.debug(so, R, lim, w, xmax, K.MAXIT), want, name)


# ---- the whole call on the fixtures

_cache = {}


def as_dict(res):
    return {k: v for k, v in res.__dict__.items() if v is not None}


def case(eng, deck, mode):
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField, forecast_sets
        fx = np.load(os.path.join(GOLD, f"field_forecast_{deck}.npz"))
        _, _, P = load_deck(deck)
        free = [str(n) for n in fx["free"]]
        sets = forecast_sets(P, free, fx["theta"], float(fx["dlog"]))[:3]
        thetas = np.array([[getattr(Pk, name) for name in free] for Pk in sets])
        plan = eng.Plan(P, mode=mode)
        wells, loc, times, z = fx["wells"], fx["locations"], fx["times"], fx["z"]
        other = WellField(wells, loc, times)
        ens = other.ensemble(plan, free, thetas, z, quantiles=None, derivative=False, all_maps=True)
        other.close()
        # the limits of tests/test_gpu_field_yield.py: half again the largest drawdown of the members on 23 outputs
        s = ens["s_all"]
        limit = np.full(s.shape[1:], np.inf)
        top = np.abs(s).max(axis=0)
        limit[-2:] = 1.5 * top[-2:] + 1e-3 * top.max()
        for k, i, iz in ((0, 1, 0), (2, 4, 1), (3, 0, 0)):
            limit[k, i, iz] = 1.5 * top[k, i, iz] + 1e-3 * top.max()
        field = WellField(wells, loc, times)
        args = (plan, free, thetas, z)
        ykw = dict(limit=limit, q=QS, with_stats=True)
        akw = dict(limit=limit, q=QS, maxit=K.MAXIT, with_stats=True)
        y_before = field.sustainable_yield(*args, CTL2, [[1.0, 1.0], [0.5, 2.0]], smax=10.0, **ykw)
        two = field.optimal_rates(*args, CTL2, W2, XMAX2, **akw)
        n = field.alloc_count()
        again = field.optimal_rates(*args, CTL2, W2, XMAX2, **akw)
        n_again = field.alloc_count()
        y_after = field.sustainable_yield(*args, CTL2, [[1.0, 1.0], [0.5, 2.0]], smax=10.0, **ykw)
        weighted = field.optimal_rates(*args, CTL2, W2, XMAX2, weights=[1.0, 0.0, 0.5], **akw)
        y_weighted = field.sustainable_yield(*args, CTL2, [[1.0, 1.0]], smax=10.0, weights=[1.0, 0.0, 0.5], **ykw)
        one = field.optimal_rates(*args, np.zeros(4, np.int32), [[1.0]], XMAX1, **akw)
        y_one = field.sustainable_yield(*args, np.zeros(4, np.int32), [[1.0]], smax=XMAX1, **ykw)
        _cache[(deck, mode)] = dict(limit=limit, field=field, plan=plan, y_before=y_before, y_after=y_after, two=two, again=again, n=n, n_again=n_again,
                                    weighted=weighted, y_weighted=y_weighted, one=one, y_one=y_one)
    return _cache[(deck, mode)]


def check_call(so, res, w, xmax, limit, u=None):
    """the programmes against the kernel alone on the returned slots, and the reliability stage against the restatements"""
    con, lim_con = Y.constrained(limit)
    assert res.con.dtype == np.int32 and np.array_equal(res.con, con)
    alone = K.debug(so, res.resp, lim_con, w, xmax, K.MAXIT, con=con)
    got = dict(as_dict(res), nbad=res.nbad + (0 if u is None else int((u == 0).sum())))
    K.same_bytes(got, alone, "call against the kernel alone")
    K.same_bytes(got, A.allocate(res.resp, lim_con, w, xmax, K.MAXIT), "call against the restatement")
    # reliability: the optima as patterns at smax = 1, the member reduction, the host step
    pats = A.patterns(res.x, res.status)
    y = Y.ratio_test(res.resp, pats, lim_con, con, 1.0)["y"]
    quant = Y.quantile_linear(y, QS) if u is None else restate_weighted(y, u, list(QS), [])["quant"]
    same_bits(res.quant, quant, "quant")
    value, best, best_x = A.select(quant, res.g, res.x)
    same_bits(res.value, value, "value")
    assert res.best.dtype == np.int32 and np.array_equal(res.best, best), (res.best, best)
    same_bits(res.best_x, best_x, "best_x")
    gq = Y.quantile_linear(res.g, QS) if u is None else restate_weighted(res.g, u, list(QS), [])["quant"]
    same_bits(res.gquant, gq, "gquant")
    return y


@pytest.mark.parametrize("deck,mode", CASES)
def test_two_controls_and_a_fixed_well(so, eng, deck, mode):
    c = case(eng, deck, mode)
    res = c["two"]
    assert res.resp.tobytes() == c["y_before"]["resp"].tobytes()          # the member loop of ucf_field_yield
    assert res.stats == c["y_before"]["stats"] and res.nbad == 0
    y = check_call(so, res, W2, XMAX2, c["limit"])
    assert (res.status == A.OPTIMAL).all() and (res.x >= 0.0).all() and (res.x <= XMAX2).all()
    # the rates as given are admissible with half the room to spare: the optimum pumps more than today's total
    assert (res.g[:, 0] > 2.0).all() and (res.lam >= 0.0).all()
    # a member admits its own optimum at full scale up to rounding; at level 1 (the scale that the most permissive member
    # admits, at most 1) no candidate is worth more than the largest g
    own = np.array([[y[m, m * 2 + o] for o in range(2)] for m in range(3)])
    assert (own > 1.0 - 1e-12).all(), own
    assert QS[-1] == 1.0 and (res.value[-1].reshape(3, 2).max(axis=0) <= res.gquant[-1]).all()
    assert (res.best >= 0).all() and (res.best % 2 == np.arange(2)).all()
    print(f"[allocate {deck} {mode}] g {res.g.tolist()}, iters {res.iters.tolist()}, binding {[res.binding(m, 0) for m in range(3)]}, "
          f"best {res.best.tolist()}, value of best {np.nanmax(res.value.reshape(len(QS), 3, 2), axis=1).tolist()}, gquant {res.gquant.tolist()}")


@pytest.mark.parametrize("deck,mode", CASES)
def test_one_control_is_the_ratio_test(so, eng, deck, mode):
    c = case(eng, deck, mode)
    res, yo = c["one"], c["y_one"]
    check_call(so, res, np.ones((1, 1)), np.full(1, XMAX1), c["limit"])
    assert (res.status == A.OPTIMAL).all() and (yo["y"][:, 0] > 0.0).all()
    x, hi = res.x[:, 0, 0], yo["y"][:, 0]
    ulps = np.abs(x - hi) / np.spacing(hi)
    print(f"[allocate {deck} {mode}] one control: x {x.tolist()}, min(xmax, hi) {hi.tolist()}, apart by {ulps.tolist()} ulp")
    assert (ulps <= 1.0).all(), (x, hi)
    for m in range(3):
        # at the capacity the upper bound binds, below it the output that binds hi
        b = res.binding(m, 0)[0]
        assert b == (("upper", 0) if yo["bind"][m, 0] < 0 else ("output", int(yo["bind"][m, 0]))), (m, b, yo["bind"][m, 0])


@pytest.mark.parametrize("deck,mode", CASES)
def test_a_member_of_weight_zero_is_not_launched(so, eng, deck, mode):
    c = case(eng, deck, mode)
    res, two = c["weighted"], c["two"]
    u, ess = quantise([1.0, 0.0, 0.5])
    assert res.u.tobytes() == u.tobytes() and res.ess == ess and res.nlaunched == 2 and res.nbad == 0
    assert res.stats == c["y_weighted"]["stats"]                           # what ucf_field_yield launches for the same weights
    assert np.isnan(res.resp[1]).all() and np.isnan(res.x[1]).all() and np.isnan(res.g[1]).all() and np.isnan(res.lam[1]).all()
    assert (res.status[1] == A.INVALID).all() and (res.work[1] == -1).all() and (res.iters[1] == 0).all()
    for key in ("resp", "x", "g", "lam", "status", "iters", "work"):
        for m in (0, 2):
            assert getattr(res, key)[m].tobytes() == getattr(two, key)[m].tobytes(), (key, m)
    check_call(so, res, W2, XMAX2, c["limit"], u=u)
    assert (res.best // 2 != 1).all()


@pytest.mark.parametrize("deck,mode", CASES)
def test_repetition_and_the_yield_calls_around_it(so, eng, deck, mode):
    c = case(eng, deck, mode)
    assert c["n"] > 0 and c["n_again"] == c["n"]
    for key, v in as_dict(c["two"]).items():
        if isinstance(v, np.ndarray):
            assert getattr(c["again"], key).tobytes() == v.tobytes(), key
        else:
            assert getattr(c["again"], key) == v, key
    for key, v in c["y_before"].items():
        if isinstance(v, np.ndarray):
            assert c["y_after"][key].tobytes() == v.tobytes(), key
        else:
            assert c["y_after"][key] == v, key
