"""ucf_field_worth on the GPU: field_worth_kernel through ucf_debug_field_worth on synthetic slots, and the whole call on the
fixtures of tests/test_gpu_field_forecast.py (4 wells, 5 locations, 6 times, 2 depths; decks neuman74_partpen with free Kr,
kappa, Ss, Sy and c1_theis with free Kr, Ss), against the numpy restatement of include/ucf.h (tests/field_worth_restate.py).

Bounds.  The kernel holds +, -, * and / only, each rounded on its own: post, crit and nused are compared bit for bit (the
payload of a NaN aside).  Where two operation orders of one quantity meet, the bound is worked out, never fitted:
  prior vs se^2   both are j' C j, once as |F'j|^2 and once as sum_j J_j (sum_k C_jk J_k), plus the rounding of the factorisation:
                  8 npar u sum_jk |J_j| (|F||F'|)_jk |J_k|;
  post <= prior   and prior[r+1] vs post[r] at the pick: a solve with B = I + sum (w F'j)(w F'j)' through LDL', the textbook forward
                  bound 8 npar u kappa_2(B), relative; kappa_2(B) is computed here per candidate, nothing is assumed about it."""
import ctypes as C
import os

import numpy as np
import pytest

import field_worth_restate as R
from golden_util import GOLD, load_deck
from test_gpu_fit import NAN_R, NAN_T

pytestmark = pytest.mark.gpu

DECKS = ["neuman74_partpen", "c1_theis"]
MODES = ["faithful", "fast"]
U = 2.0 ** -53
SIGMA_S, SIGMA_D = 0.01, 0.05
TARGETS = [("s", 5, 4, 1), ("ds", 3, 0, 0)]
TGT = [(0, 5, 4, 1), (1, 3, 0, 0)]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def addr(a):
    return a.ctypes.data if a is not None else None


def debug(a_s, a_d, two_dlog, F, ws, wd, tsel, A, tw):
    """one launch of field_worth_kernel through the library's launcher on caller data"""
    from unconfined_amd import lib as ucflib
    so = ucflib.load()
    a_s = np.ascontiguousarray(a_s, dtype=float)
    a_d = None if a_d is None else np.ascontiguousarray(a_d, dtype=float)
    F, A = np.ascontiguousarray(F, dtype=float), np.ascontiguousarray(A, dtype=float)
    tsel = None if tsel is None else np.ascontiguousarray(tsel, dtype=np.int32)
    tw = None if tw is None else np.ascontiguousarray(tw, dtype=float)
    npar, (nset, nt, ncand), ntgt = len(F), a_s.shape, len(A)
    assert nset == 1 + 2 * npar and A.shape == (ntgt, npar)
    post, crit, nused = np.zeros((ntgt, ncand)), np.zeros(ncand), np.zeros(ncand, np.int32)
    ucflib.check(so.ucf_debug_field_worth(npar, nt, ncand, addr(a_s), addr(a_d), float(two_dlog), addr(F), float(ws), float(wd), addr(tsel), ntgt,
                                          addr(A), addr(tw), addr(post), addr(crit), addr(nused)))
    return post, crit, nused


def same_bits(got, want, what):
    """equal NaN positions, equal bytes elsewhere (the payload of a NaN is not part of the contract)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    assert got[~nan].tobytes() == want[~nan].tobytes(), (what, int((got[~nan] != want[~nan]).sum()))


def synthetic(npar, ncand, seed):
    """slots of s and ds [1 + 2 npar, 5, ncand] with J of order 1 at dlog = 1e-3, a general F, and the candidates that the
    kernel has to treat apart: slot 0 is NaN throughout (it is never read)"""
    rng = np.random.default_rng(seed)
    nt = 5
    a_s = 1.0 + 1e-3 * rng.standard_normal((1 + 2 * npar, nt, ncand))
    a_d = 0.3 + 2e-3 * rng.standard_normal((1 + 2 * npar, nt, ncand))
    a_s[0], a_d[0] = np.nan, np.nan
    M = rng.standard_normal((npar, npar))
    F = 0.2 * np.eye(npar) + 0.05 * M                  # neither triangular nor symmetric
    special = {}
    if ncand == 1:
        special["all_bad" if npar % 2 == 0 else "single"] = 0
    else:
        special = dict(all_bad=3, single=5, pinf=7, ninf=9, sentinel=11, nan_one=64 if ncand > 64 else 13)
    for name, c in special.items():
        if name == "all_bad":                          # every datum has one value that is not finite, in another slot each time
            for k in range(nt):
                a_s[1 + (k % (2 * npar)), k, c] = np.nan
                a_d[2 * npar - (k % (2 * npar)), k, c] = np.inf
        elif name == "single":                         # only the drawdown at k = 2 survives
            a_s[1, [0, 1, 3, 4], c] = [np.nan, np.inf, -np.inf, np.nan]
            a_d[2 * npar, :, c] = np.nan
        elif name == "pinf":
            a_s[2 * npar, 1, c] = np.inf
        elif name == "ninf":
            a_d[1, 4, c] = -np.inf
        elif name == "sentinel":                       # finite: it takes part
            a_s[1, 0, c] = -999999.9
            a_d[2 * npar, 2, c] = -999999.9
        elif name == "nan_one":
            a_d[1, 0, c] = np.nan
    return a_s, a_d, F, special


@pytest.mark.parametrize("ncand", [1, 70, 257])
@pytest.mark.parametrize("npar", range(1, 9))
def test_kernel_is_the_stated_arithmetic(eng, npar, ncand):
    """under, over and across a wave of 64; per case one launch with one target, drawdown data only and every time, and one with
    16 targets, derivative data and a tsel with zeros"""
    a_s, a_d, F, special = synthetic(npar, ncand, 1000 * npar + ncand)
    rng = np.random.default_rng(npar + ncand)
    two_dlog = np.float64(2.0) * np.float64(1e-3)
    A16 = rng.standard_normal((16, npar)) * 0.1
    tw16 = rng.uniform(0.0, 2.0, 16)
    tw16[3] = 0.0
    tsel = np.array([1, 0, 1, 1, 0], np.int32)
    for label, (ad, ws, wd, ts, A, tw) in (("s only", (None, 100.0, 0.0, None, A16[:1], None)),
                                            ("s and ds", (a_d, 100.0, 20.0, tsel, A16, tw16))):
        got = debug(a_s, ad, two_dlog, F, ws, wd, ts, A, tw)
        want = R.kernel(a_s, ad, two_dlog, F, ws, wd, ts, A, tw)
        for name, g, w in zip(("post", "crit", "nused"), got, want):
            same_bits(g, w, (label, name))
        post, crit, nused = got
        # (a sentinel among the readings takes part; it makes kappa_2(B) of the order of 1e20, beyond 1 / u, where rounding may
        # leave a d_j that is not positive: then post is NaN, in the restatement and on the device alike)
        usual = np.ones(ncand, bool)
        if "sentinel" in special:
            usual[special["sentinel"]] = False
        assert np.isfinite(post[:, usual]).all() and np.isfinite(crit[usual]).all() and (post[:, usual] > 0.0).all(), label
        _, prior = R.targets(np.eye(npar), A, [True] * len(A))          # sum_j A_tj^2
        per_time = 1 if wd == 0.0 else 2
        ntime = 5 if ts is None else int(ts.sum())
        full = np.full(ncand, per_time * ntime, np.int32)
        if "all_bad" in special:
            c = special["all_bad"]
            assert nused[c] == 0 and post[:, c].tobytes() == prior.tobytes(), label
            full[c] = 0
        if "single" in special:
            c = special["single"]
            Jc, wc = R.rows_of(a_s, ad, two_dlog, ws, wd, ts, c)
            kB = np.linalg.cond(R.dense_B(F, Jc, wc))
            assert nused[c] == 1 == len(wc) and (post[:, c] <= prior * (1 + 8 * npar * U * kB)).all() and (post[:, c] != prior).any(), label
            full[c] = 1
        if "pinf" in special:
            full[special["pinf"]] -= 0 if (ts is not None and ts[1] == 0) else 1
        if "ninf" in special and wd > 0.0:
            full[special["ninf"]] -= 0 if (ts is not None and ts[4] == 0) else 1
        if "nan_one" in special and wd > 0.0:
            full[special["nan_one"]] -= 1
        assert nused.tolist() == full.tolist(), label
    # a target on a slot that is not finite: its row and crit are NaN, the other rows are what they were
    A = A16[:3].copy()
    A[1] = np.nan
    post, crit, nused = debug(a_s, a_d, two_dlog, F, 100.0, 20.0, tsel, A, None)
    want = R.kernel(a_s, a_d, two_dlog, F, 100.0, 20.0, tsel, A, None)
    for name, g, w in zip(("post", "crit", "nused"), (post, crit, nused), want):
        same_bits(g, w, ("nan target", name))
    assert np.isnan(post[1]).all() and np.isnan(crit).all() and np.isfinite(post[[0, 2]][:, usual]).all()


# ---- the whole call on the fixtures

_cache = {}


def case(eng, deck, mode):
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField
        fx = np.load(os.path.join(GOLD, f"field_forecast_{deck}.npz"))
        _, _, P = load_deck(deck)
        free, theta, dlog = [str(n) for n in fx["free"]], fx["theta"], float(fx["dlog"])
        plan = eng.Plan(P, mode=mode)
        other = WellField(fx["wells"], fx["locations"], fx["times"])
        before = other.drawdown(plan, fx["z"])
        field = WellField(fx["wells"], fx["locations"], fx["times"])
        fc = field.forecast(plan, free, theta, fx["z"], cov=fx["cov"], dlog=dlog, all_maps=True)
        out = field.worth(plan, free, theta, fx["cov"], fx["z"], TARGETS, SIGMA_S, sigma_d=SIGMA_D, dlog=dlog, with_stats=True)
        fc2 = field.forecast(plan, free, theta, fx["z"], cov=fx["cov"], dlog=dlog, all_maps=True, with_stats=True)
        after = other.drawdown(plan, fx["z"])
        other.close()
        want = R.worth(fc["s_all"], fc["ds_all"], dlog, fx["cov"], SIGMA_S, SIGMA_D, None, TGT, None, 1)
        _cache[(deck, mode)] = dict(fx=fx, free=free, theta=theta, dlog=dlog, plan=plan, field=field, fc=fc, fc2=fc2, out=out, want=want,
                                    before=before, after=after)
    return _cache[(deck, mode)]


def check_against(out, want, nloc, nz):
    npick = len(want["pick"])
    same_bits(out["prior"], want["prior"], "prior")
    same_bits(out["post"], want["post"].reshape(out["post"].shape), "post")
    same_bits(out["crit"], want["crit"].reshape(out["crit"].shape), "crit")
    assert out["nused"].dtype == np.int32 and out["nused"].tobytes() == want["nused"].reshape(nloc, nz).tobytes()
    assert out["pick"] == [None if c < 0 else (int(c) // nz, int(c) % nz) for c in want["pick"]] and len(out["pick"]) == npick
    same_bits(out["cov_post"], want["cov_post"], "cov_post")
    with np.errstate(invalid="ignore", divide="ignore"):
        same_bits(out["reduction"], 1.0 - out["post"] / out["prior"][:, :, None, None], "reduction")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_end_to_end_is_the_restatement_on_the_forecast_slots(eng, deck, mode):
    c = case(eng, deck, mode)
    fx, out, fc, want = c["fx"], c["out"], c["fc"], c["want"]
    npar, (nt, nloc, nz) = len(c["free"]), fc["s"].shape
    assert out["post"].shape == (1, 2, nloc, nz) and out["crit"].shape == (1, nloc, nz) and out["prior"].shape == (1, 2)
    check_against(out, want, nloc, nz)
    assert out["pick"][0] is not None and (out["nused"] == 2 * nt).all()
    assert np.isfinite(out["post"]).all() and (out["post"] > 0.0).all()
    # the worth call evaluated what the forecast evaluates
    assert out["stats"] == c["fc2"]["stats"]
    # prior against the forecast's own standard error at the targets
    F = want["F"][0]
    two_dlog = np.float64(2.0) * np.float64(c["dlog"])
    for t, (kind, k, i, z) in enumerate(TGT):
        a = (fc["ds_all"] if kind else fc["s_all"])[:, k, i, z]
        J = np.abs(np.array([(a[1 + 2 * j] - a[2 + 2 * j]) / two_dlog for j in range(npar)]))
        bound = 8 * npar * U * (J @ (np.abs(F) @ np.abs(F).T) @ J)
        se2 = float((fc["dse"] if kind else fc["se"])[k, i, z]) ** 2
        err = abs(out["prior"][0, t] - se2)
        print(f"[worth {deck} {mode}] target {t}: prior {out['prior'][0, t]:.6e}, se^2 {se2:.6e}, |difference| = {err:.3e}, {err / bound:.3f} of the bound")
        assert err <= bound, (t, err, bound)
    # data never add variance: per candidate, with the condition number of its own B
    a_s, a_d = fc["s_all"].reshape(1 + 2 * npar, nt, -1), fc["ds_all"].reshape(1 + 2 * npar, nt, -1)
    post = out["post"].reshape(1, 2, -1)
    worst = 0.0
    for cand in range(nloc * nz):
        J, w = R.rows_of(a_s, a_d, two_dlog, 1.0 / SIGMA_S, 1.0 / SIGMA_D, None, cand)
        kB = np.linalg.cond(R.dense_B(F, J, w))
        worst = max(worst, kB)
        assert (post[0, :, cand] <= out["prior"][0] * (1 + 8 * npar * U * kB)).all(), cand
    print(f"[worth {deck} {mode}] largest kappa_2(B) over the candidates: {worst:.4g}; largest reduction {float(out['reduction'].max()):.4f}")
    assert (out["reduction"] > 0.0).any()


@pytest.mark.parametrize("deck,mode", [("neuman74_partpen", "fast"), ("c1_theis", "faithful")])
def test_worthless_data_leave_the_prior(eng, deck, mode):
    """sigma_s = 1e200 and no derivative data: every (w g)(w g) underflows to 0, B is the identity and post has the bits of prior"""
    c = case(eng, deck, mode)
    fx = c["fx"]
    out = c["field"].worth(c["plan"], c["free"], c["theta"], fx["cov"], fx["z"], TARGETS, 1e200, sigma_d=0.0, dlog=c["dlog"])
    assert out["prior"].tobytes() == c["out"]["prior"].tobytes()
    for t in range(2):
        assert (out["post"][0, t].view(np.uint64) == out["prior"][0, t:t + 1].view(np.uint64)[0]).all(), t
    assert (out["nused"] == len(fx["times"])).all() and out["pick"] == [(0, 0)]
    assert (out["reduction"] == 0.0).all()


def test_greedy_network(eng):
    """three picks on the neuman74 field with every location twice (location i + 5 is location i): each candidate has a twin with
    the same bits, so every round ends in a tie"""
    from unconfined_amd import WellField, worth_condition
    c = case(eng, "neuman74_partpen", "fast")
    fx, free, theta, dlog, plan = c["fx"], c["free"], c["theta"], c["dlog"], c["plan"]
    npar, nz = len(free), len(fx["z"])
    loc = np.concatenate([fx["locations"], fx["locations"]])
    nloc = len(loc)
    tsel = np.array([1, 1, 0, 1, 1, 1])
    tw = [1.0, 0.5]
    field = WellField(fx["wells"], loc, fx["times"])
    fc = field.forecast(plan, free, theta, fx["z"], cov=fx["cov"], dlog=dlog, all_maps=True)
    assert fc["s_all"][:, :, :5].tobytes() == fc["s_all"][:, :, 5:].tobytes()
    out = field.worth(plan, free, theta, fx["cov"], fx["z"], TARGETS, SIGMA_S, sigma_d=SIGMA_D, times=tsel, picks=3, weights=tw, dlog=dlog)
    want = R.worth(fc["s_all"], fc["ds_all"], dlog, fx["cov"], SIGMA_S, SIGMA_D, tsel, TGT, tw, 3)
    check_against(out, want, nloc, nz)
    picks = out["pick"]
    assert None not in picks and len(set(picks)) == 3
    # a pick and its twin have the same criterion in that round, and the lower twin goes first
    assert picks[0][0] < 5
    for r, (i, z) in enumerate(picks):
        assert out["crit"][r, i, z].tobytes() == out["crit"][r, (i + 5) % 10, z].tobytes(), (r, i, z)
        assert i < 5 or (i - 5, z) in picks[:r], (r, i, z)
    # round r + 1 is one launch with the factor that worth_condition gives for the pick of round r
    nset, nt = fc["s_all"].shape[:2]
    a_s, a_d = fc["s_all"].reshape(nset, nt, -1), fc["ds_all"].reshape(nset, nt, -1)
    two_dlog = np.float64(2.0) * np.float64(dlog)
    ws, wd = 1.0 / SIGMA_S, 1.0 / SIGMA_D
    F = R.cholesky(fx["cov"])
    Jt = [R.jac((a_d if kind else a_s)[:, k, i * nz + z], two_dlog)[0] for kind, k, i, z in TGT]
    for r in range(3):
        A, prior = R.targets(F, Jt, [True, True])
        post, crit, nused = debug(a_s, a_d, two_dlog, F, ws, wd, tsel, A, tw)
        assert post.tobytes() == out["post"][r].tobytes() and crit.tobytes() == out["crit"][r].tobytes(), r
        assert prior.tobytes() == out["prior"][r].tobytes() and nused.tobytes() == out["nused"].tobytes(), r
        cand = picks[r][0] * nz + picks[r][1]
        J, w = R.rows_of(a_s, a_d, two_dlog, ws, wd, tsel, cand)
        assert len(w) == 2 * int(tsel.sum())
        kB = np.linalg.cond(R.dense_B(F, J, w))
        F, cov_next = worth_condition(F, J, w)
        if r < 2:
            rel = np.abs(out["prior"][r + 1] - post[:, cand]) / post[:, cand]
            print(f"[worth greedy] round {r}: pick {picks[r]}, kappa_2(B) = {kB:.4g}, |prior[r+1] - post[r][pick]| / post = {rel.max():.3e}, "
                  f"{rel.max() / (8 * npar * U * kB):.3f} of the bound")
            assert (rel <= 8 * npar * U * kB).all(), (r, rel)
    assert out["cov_post"].tobytes() == cov_next.tobytes() == R.condition(F, np.zeros((0, npar)), np.zeros(0))[1].tobytes()
    # with the lower twin of the first pick not allowed, the first pick is its twin: same criterion, the next index
    allowed = np.ones((nloc, nz), np.int32)
    allowed[picks[0]] = 0
    n = field.alloc_count()
    masked = field.worth(plan, free, theta, fx["cov"], fx["z"], TARGETS, SIGMA_S, sigma_d=SIGMA_D, times=tsel, picks=3, weights=tw, allowed=allowed,
                         dlog=dlog)
    assert field.alloc_count() == n
    assert masked["pick"][0] == (picks[0][0] + 5, picks[0][1]) and picks[0] not in masked["pick"]
    assert masked["crit"][0].tobytes() == out["crit"][0].tobytes() and masked["prior"][1].tobytes() == out["prior"][1].tobytes()
    check_against(masked, R.worth(fc["s_all"], fc["ds_all"], dlog, fx["cov"], SIGMA_S, SIGMA_D, tsel, TGT, tw, 3, cmask=allowed.ravel()), nloc, nz)
    # nothing allowed: no pick, the later rounds do not run
    none = field.worth(plan, free, theta, fx["cov"], fx["z"], TARGETS, SIGMA_S, picks=2, allowed=np.zeros((nloc, nz)), dlog=dlog)
    assert none["pick"] == [None, None] and np.isfinite(none["crit"][0]).all() and np.isnan(none["crit"][1]).all()
    assert np.isnan(none["prior"][1]).all() and np.isnan(none["post"][1]).all()
    assert none["cov_post"].tobytes() == R.condition(R.cholesky(fx["cov"]), np.zeros((0, npar)), np.zeros(0))[1].tobytes()
    field.close()


def test_a_target_on_a_nan_slot(eng):
    """the field of tests/test_gpu_field_forecast.py whose first output is NaN in the oracle itself: a target there has a NaN prior,
    NaN rows and no pick, the call succeeds; a target elsewhere on the same map is served, and the readings that are not finite
    are not counted"""
    from unconfined_amd import WellField
    _, _, P = load_deck("neuman74_partpen")
    free, theta = ["Kr", "kappa", "Ss", "Sy"], np.array([P.Kr, P.kappa, P.Ss, P.Sy])
    z, times = np.array([145.7, 100.0]), np.array([NAN_T, 1.0, 100.0])
    cov = np.diag([0.0025, 0.0036, 0.0016, 0.0049])
    plan = eng.Plan(P, mode="fast")
    field = WellField([(0.0, 0.0, 1.0, 0.0)], [(NAN_R, 0.0), (0.0, 85.1)], times)
    fc = field.forecast(plan, free, theta, z, cov=cov, all_maps=True)
    assert not np.isfinite(fc["s_all"][1:, 0, 0, 0]).all()
    bad = field.worth(plan, free, theta, cov, z, [("s", 0, 0, 0), ("s", 2, 1, 1)], SIGMA_S, picks=2)
    assert bad["pick"] == [None, None]
    assert np.isnan(bad["prior"][0, 0]) and np.isfinite(bad["prior"][0, 1]) and np.isnan(bad["prior"][1]).all()
    assert np.isnan(bad["post"][0, 0]).all() and np.isfinite(bad["post"][0, 1]).all() and np.isnan(bad["crit"]).all() and np.isnan(bad["post"][1]).all()
    check_against(bad, R.worth(fc["s_all"], fc["ds_all"], 1e-3, cov, SIGMA_S, 0.0, None, [(0, 0, 0, 0), (0, 2, 1, 1)], None, 2), 2, 2)
    good = field.worth(plan, free, theta, cov, z, [("s", 2, 1, 1)], SIGMA_S, picks=2)
    want = R.worth(fc["s_all"], fc["ds_all"], 1e-3, cov, SIGMA_S, 0.0, None, [(0, 2, 1, 1)], None, 2)
    check_against(good, want, 2, 2)
    assert None not in good["pick"] and good["nused"][0, 0] < 3 and good["nused"].max() <= 3
    assert good["nused"].ravel().tolist() == np.isfinite(fc["s_all"][1:]).all(axis=0).sum(axis=0).ravel().tolist()
    field.close(); plan.close()


def test_housekeeping(eng):
    """a repeated call gives the same bytes and allocates nothing; the caller's plan is untouched; a forecast after a worth on the
    same field has its own bits"""
    c = case(eng, "neuman74_partpen", "fast")
    fx, field = c["fx"], c["field"]
    assert c["before"][0].tobytes() == c["after"][0].tobytes() == c["fc"]["s"].tobytes()
    assert c["before"][1].tobytes() == c["after"][1].tobytes() == c["fc"]["ds"].tobytes()
    for key in ("s", "ds", "sens", "dsens", "se", "dse", "s_all", "ds_all", "nbad"):
        assert c["fc"][key].tobytes() == c["fc2"][key].tobytes(), key
    n = field.alloc_count()
    again = field.worth(c["plan"], c["free"], c["theta"], fx["cov"], fx["z"], TARGETS, SIGMA_S, sigma_d=SIGMA_D, dlog=c["dlog"])
    assert n > 0 and field.alloc_count() == n
    for key in ("prior", "post", "crit", "nused", "cov_post", "reduction"):
        assert again[key].tobytes() == c["out"][key].tobytes(), key
    assert again["pick"] == c["out"]["pick"]
