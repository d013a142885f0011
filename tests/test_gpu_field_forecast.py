"""ucf_field_forecast on the GPU (fixtures: tools/gen_field_forecast_fixture.py): the field of tests/test_gpu_field.py -- 4 wells
in 2 start-time groups, 5 locations, 6 times (two before the later start; the fixture tool says how they were picked), 2
depths -- under the base parameter set and its 2 npar log-perturbed neighbours, decks neuman74_partpen (free Kr, kappa, Ss,
Sy) and c1_theis (free Kr, Ss), dlog = 1e-3.

Bounds.  Every slot is checked bit for bit against ucf_field_drawdown on a fresh field and a fresh plan of that set, and the
combination bit for bit against the recurrence that include/ucf.h states, restated in numpy (the square root within 1 ulp).
Against the oracle nothing is chosen: a launched value is held to b = gate(ref, noise) of tests/test_gpu_field.py, a slot to
the fixture's bound[k] = sum_j |q_j| tfac b_j, a sensitivity to lim_j = (bound[1+2j] + bound[2+2j]) / (2 dlog) -- the J gate
of tests/test_gpu_fit.py: the truncation error of the central difference is common to both sides and cancels -- and the
standard error to sum_j sqrt(cov[j][j]) lim_j: se = |L' J| with cov = L L', so by the triangle inequality
| |L' J| - |L' J_or| | <= |L' (J - J_or)| <= sum_j |J_j - J_or_j| |row j of L| and |row j of L| = sqrt(cov[j][j]).  The roundings
of the combination itself, a few u of the largest term, lie orders of magnitude below the 1e-10 floor of b divided by 2 dlog."""
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_field import direct, gate
from test_gpu_fit import NAN_R, NAN_T

pytestmark = pytest.mark.gpu

DECKS = ["neuman74_partpen", "c1_theis"]
MODES = ["faithful", "fast"]
MAPS = ("s", "ds", "sens", "dsens", "se", "dse", "s_all", "ds_all")


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def combine(a, cov, dlog):
    """the arithmetic of field_forecast_kernel as include/ucf.h states it: a [1 + 2 npar][...] -> J [npar][...], var"""
    two_dlog = np.float64(2.0) * np.float64(dlog)
    npar = (len(a) - 1) // 2
    J = [(a[1 + 2 * j] - a[2 + 2 * j]) / two_dlog for j in range(npar)]
    var = None
    if cov is not None:
        var = np.zeros_like(a[0])
        for j in range(npar):
            inner = np.zeros_like(a[0])
            for k in range(npar):
                inner = inner + cov[j, k] * J[k]
            var = var + J[j] * inner
    return np.stack(J), var


def se_of(var):
    with np.errstate(invalid="ignore"):
        return np.where(var < 0.0, 0.0, np.sqrt(var))


def every_set_alone(eng, sets, mode, wells, locations, times, z, launched=True):
    """per parameter set: ucf_field_drawdown on a fresh field and a fresh plan (s, ds, stats), and where asked what its groups
    launch, called directly (dimensional h, dh per group)"""
    from unconfined_amd import WellField
    out = []
    for Pk in sets:
        plan = eng.Plan(Pk, mode=mode)
        field = WellField(wells, locations, times)
        s, ds, st = field.drawdown(plan, z, with_stats=True)
        h = dh = None
        if launched:
            h, dh = direct(plan, field.groups(plan), z)
            Hc = plan.derived.Hc
            h, dh = [v * Hc for v in h], [v * Hc for v in dh]
        out.append(dict(s=s, ds=ds, stats=st, h=h, dh=dh))
        field.close(); plan.close()
    return out


def check_slots(out, alone):
    for k, ref in enumerate(alone):
        assert out["s_all"][k].tobytes() == ref["s"].tobytes(), k
        assert out["ds_all"][k].tobytes() == ref["ds"].tobytes(), k
    assert out["s"].tobytes() == out["s_all"][0].tobytes() and out["ds"].tobytes() == out["ds_all"][0].tobytes()
    assert out["stats"] == {key: sum(ref["stats"][key] for ref in alone) for key in out["stats"]}


def check_combination(out, cov, dlog):
    """sens, dsens byte for byte, se, dse within 1 ulp, nbad = the outputs with a value that is not finite; returns the number
    of se / dse values that differ from numpy's square root (by 1 ulp)"""
    off = 0
    for i, (maps, sens, se) in enumerate((("s_all", "sens", "se"), ("ds_all", "dsens", "dse"))):
        with np.errstate(invalid="ignore"):
            J, var = combine(out[maps], cov, dlog)
        nan = np.isnan(J)                             # (the payload of a NaN is not part of the contract)
        assert (np.isnan(out[sens]) == nan).all() and out[sens][~nan].tobytes() == J[~nan].tobytes(), sens
        assert out["nbad"][i] == int((~np.isfinite(out[maps])).any(axis=0).sum()), (maps, out["nbad"])
        if cov is None:
            continue
        want = se_of(var)
        fin = np.isfinite(want)
        assert (np.isfinite(out[se]) == fin).all(), se
        assert (np.abs(out[se][fin] - want[fin]) <= np.spacing(want[fin])).all(), se
        off += int((out[se][fin] != want[fin]).sum())
    return off


_cache = {}


def case(eng, deck, mode):
    """(fixture, parameter sets, the forecast with every map, every set alone, the caller's plan before and after)"""
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField, forecast_sets
        fx = np.load(os.path.join(GOLD, f"field_forecast_{deck}.npz"))
        _, _, P = load_deck(deck)
        free, theta, dlog = [str(n) for n in fx["free"]], fx["theta"], float(fx["dlog"])
        sets = forecast_sets(P, free, theta, dlog)
        plan = eng.Plan(P, mode=mode)
        other = WellField(fx["wells"], fx["locations"], fx["times"])
        before = other.drawdown(plan, fx["z"])
        field = WellField(fx["wells"], fx["locations"], fx["times"])
        out = field.forecast(plan, free, theta, fx["z"], cov=fx["cov"], dlog=dlog, all_maps=True, with_stats=True)
        after = other.drawdown(plan, fx["z"])
        alone = every_set_alone(eng, sets, mode, fx["wells"], fx["locations"], fx["times"], fx["z"])
        other.close()
        _cache[(deck, mode)] = dict(fx=fx, P=P, free=free, theta=theta, dlog=dlog, sets=sets, plan=plan, field=field, out=out, alone=alone,
                                    before=before, after=after)
    return _cache[(deck, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_every_slot_is_the_existing_entry(eng, deck, mode):
    c = case(eng, deck, mode)
    assert len(c["sets"]) == 1 + 2 * len(c["free"]) == len(c["out"]["s_all"])
    check_slots(c["out"], c["alone"])
    assert np.isfinite(c["out"]["s_all"]).all() and np.isfinite(c["out"]["ds_all"]).all()
    assert c["out"]["s_all"][1].tobytes() != c["out"]["s_all"][2].tobytes()
    # the caller's plan was not modified: its own map is what it was
    assert c["before"][0].tobytes() == c["after"][0].tobytes() == c["out"]["s"].tobytes()
    assert c["before"][1].tobytes() == c["after"][1].tobytes() == c["out"]["ds"].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_the_combination_is_the_stated_arithmetic(eng, deck, mode):
    c = case(eng, deck, mode)
    out, fx = c["out"], c["fx"]
    off = check_combination(out, fx["cov"], c["dlog"])
    print(f"[forecast {deck} {mode}] se / dse values 1 ulp from numpy's square root: {off} of {2 * out['se'].size}")
    assert out["nbad"].tolist() == [0, 0]
    assert (out["se"] > 0.0).all() and (out["sens"] != 0.0).any()
    # without a covariance and without the standard errors the other outputs are the same
    plain = c["field"].forecast(c["plan"], c["free"], c["theta"], fx["z"], dlog=c["dlog"], all_maps=True)
    assert "se" not in plain and "dse" not in plain and "stats" not in plain
    for key in ("s", "ds", "sens", "dsens", "s_all", "ds_all", "nbad"):
        assert plain[key].tobytes() == out[key].tobytes(), key
    # ... and the base maps alone
    bare = c["field"].forecast(c["plan"], c["free"], c["theta"], fx["z"], dlog=c["dlog"], sensitivities=False)
    assert sorted(bare) == ["ds", "nbad", "s"]
    assert bare["s"].tobytes() == out["s"].tobytes() and bare["ds"].tobytes() == out["ds"].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_against_the_oracle(eng, deck, mode):
    c = case(eng, deck, mode)
    fx, out, dlog = c["fx"], c["out"], c["dlog"]
    nset, npar, cov = len(c["sets"]), len(c["free"]), fx["cov"]
    # the launched values of every set, term by term: the grid path itself
    for k in range(nset):
        for g in range(len(c["alone"][k]["h"])):
            for name in ("h", "dh"):
                got, ref = c["alone"][k][name][g], fx[f"k{k}_g{g}_ref_{name}"]
                b = gate(ref, fx[f"k{k}_g{g}_noise_{name}"])
                err = np.abs(got - ref)
                print(f"[forecast {deck} {mode}] set {k} group {g} {name}: worst |grid - oracle| / b = {float((err / b).max()):.3f}")
                assert (err <= b).all(), (deck, mode, k, g, name, float((err / b).max()))
    for maps, ref_key, bound_key, sens, se in (("s_all", "s_all_ref", "bound_s", "sens", "se"), ("ds_all", "ds_all_ref", "bound_ds", "dsens", "dse")):
        ref, bound = fx[ref_key], fx[bound_key]
        assert (bound > 0.0).all()
        err = np.abs(out[maps] - ref)
        print(f"[forecast {deck} {mode}] {maps}: worst |slot - oracle| / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (deck, mode, maps, float((err / bound).max()))
        J_or, var_or = combine(ref, cov, dlog)
        lim = np.stack([(bound[1 + 2 * j] + bound[2 + 2 * j]) / (2 * dlog) for j in range(npar)])
        err = np.abs(out[sens] - J_or)
        for j in range(npar):
            print(f"[forecast {deck} {mode}] {sens}[{j}]: worst |J - J_or| / bound = {float((err[j] / lim[j]).max()):.3f}")
        assert (err <= lim).all(), (deck, mode, sens, float((err / lim).max()))
        se_lim = sum(np.sqrt(cov[j, j]) * lim[j] for j in range(npar))
        err = np.abs(out[se] - se_of(var_or))
        print(f"[forecast {deck} {mode}] {se}: worst |se - se_or| / bound = {float((err / se_lim).max()):.3f}")
        assert (err <= se_lim).all(), (deck, mode, se, float((err / se_lim).max()))


def moench4():
    """deck c3_moench with a fourth alpha: eight free parameters"""
    _, _, P = load_deck("c3_moench")
    P.MoenchM = 4
    P.MoenchAlpha[3] = 2.5
    free = ["Kr", "kappa", "Ss", "Sy"] + [f"MoenchAlpha[{i}]" for i in range(4)]
    theta = np.array([P.Kr, P.kappa, P.Ss, P.Sy] + [P.MoenchAlpha[i] for i in range(4)])
    return P, free, theta


def test_every_width_and_partial_blocks(eng):
    """npar = 8 and npar = 1 on 45 locations x 6 times x 2 depths = 540 outputs: three workgroups of 256 threads, the last with
    28 threads -- no full wave.  Fast flavour; the byte identities only."""
    from unconfined_amd import WellField, forecast_sets
    fx = np.load(os.path.join(GOLD, "field_forecast_neuman74_partpen.npz"))
    P, free, theta = moench4()
    xs, ys = np.meshgrid(np.linspace(-1.2, 2.8, 9), np.linspace(-1.4, 1.9, 5), indexing="ij")
    loc = np.stack([xs.ravel(), ys.ravel()], axis=1) * 100.0
    z, dlog = fx["z"], 1e-3
    assert len(loc) * len(fx["times"]) * len(z) == 540
    L = np.tril(0.02 + 0.05 * np.cos(np.arange(64.0).reshape(8, 8)))
    cov = L @ L.T
    cov = 0.5 * (cov + cov.T)
    plan = eng.Plan(P, mode="fast")
    field = WellField(fx["wells"], loc, fx["times"])
    sets = forecast_sets(P, free, theta, dlog)
    alone = every_set_alone(eng, sets, "fast", fx["wells"], loc, fx["times"], z, launched=False)
    for npar in (8, 1):
        c = cov[:npar, :npar].copy()
        out = field.forecast(plan, free[:npar], theta[:npar], z, cov=c, dlog=dlog, all_maps=True, with_stats=True)
        assert out["s_all"].shape == (1 + 2 * npar, 6, 45, 2) and out["sens"].shape == (npar, 6, 45, 2)
        check_slots(out, alone[:1 + 2 * npar])
        check_combination(out, c, dlog)
        assert (out["s_all"][1] != out["s_all"][2]).any()
    field.close(); plan.close()


def test_a_nonfinite_value_propagates_and_is_counted(eng, oracle):
    """one well at the origin; location 0 at distance NAN_R, first time NAN_T: the oracle itself gives NaN there at z = 145.7.
    The overflow is one of the time (the CPU oracle gives NaN at NAN_T at every distance from 1.6 to 300 and both depths, under
    all nine parameter sets), so the first time of the second location is affected as well: it is counted like the other, and
    location 1 as a whole -- its finite values bit for bit, its values that are not finite as such -- is the same call
    without location 0.  Every output at the later times is finite."""
    from unconfined_amd import WellField
    _, _, P = load_deck("neuman74_partpen")
    free, theta = ["Kr", "kappa", "Ss", "Sy"], np.array([P.Kr, P.kappa, P.Ss, P.Sy])
    z, times = np.array([145.7, 100.0]), np.array([NAN_T, 1.0, 100.0])
    D = oracle.nondim(P)
    zD = z / D.Lc
    ho, _ = oracle.batch(P, np.array([NAN_T / D.Tc]), np.array([NAN_R / D.Lc]), np.array([1], np.int32), zD, oracle.zlay(D, zD))
    assert np.isnan(ho[0, 0]), ho                      # the oracle alone
    cov = np.diag([0.0025, 0.0036, 0.0016, 0.0049])
    plan = eng.Plan(P, mode="fast")
    well = [(0.0, 0.0, 1.0, 0.0)]
    both = WellField(well, [(NAN_R, 0.0), (0.0, 85.1)], times)
    out = both.forecast(plan, free, theta, z, cov=cov, all_maps=True)
    for i, (maps, sens, se, s) in enumerate((("s_all", "sens", "se", "s"), ("ds_all", "dsens", "dse", "ds"))):
        hit = (~np.isfinite(out[maps])).any(axis=0)
        print(f"[forecast nonfinite] {maps}: {int(hit.sum())} outputs with a value that is not finite, nbad = {out['nbad'][i]}")
        assert out["nbad"][i] == hit.sum()
        assert not hit[1:].any()
        for key in (s, se):
            assert np.isfinite(out[key][~hit]).all(), key
        assert np.isfinite(out[sens][:, ~hit]).all()
    hit = (~np.isfinite(out["s_all"])).any(axis=0)
    assert hit[0, 0, 0] and out["nbad"][0] >= 1
    assert not np.isfinite(out["s"][0, 0, 0]) and not np.isfinite(out["se"][0, 0, 0]) and not np.isfinite(out["sens"][:, 0, 0, 0]).any()
    check_combination(out, cov, 1e-3)
    # every other output: the same call without that location
    rest = WellField(well, [(0.0, 85.1)], times)
    ref = rest.forecast(plan, free, theta, z, cov=cov, all_maps=True)
    for i, maps in enumerate(("s_all", "ds_all")):
        assert ref["nbad"][i] == (~np.isfinite(out[maps][:, :, 1:, :])).any(axis=0).sum()
    for key in MAPS:
        got = out[key][..., 1:, :]
        fin = np.isfinite(got)
        assert (np.isfinite(ref[key]) == fin).all() and got[fin].tobytes() == ref[key][fin].tobytes(), key
        assert fin[..., 1:, :, :].all(), key
    both.close(); rest.close(); plan.close()


def test_repetition(eng):
    """a second call allocates nothing and gives the same bits; a plan of another model rebuilds the scratch plan"""
    from unconfined_amd import WellField, forecast_sets
    fx = np.load(os.path.join(GOLD, "field_forecast_neuman74_partpen.npz"))
    _, _, P = load_deck("neuman74_partpen")
    free, theta, dlog, z = [str(n) for n in fx["free"]], fx["theta"], float(fx["dlog"]), fx["z"]
    plan = eng.Plan(P, mode="fast")
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    a = field.forecast(plan, free, theta, z, cov=fx["cov"], dlog=dlog, all_maps=True)
    n = field.alloc_count()
    b = field.forecast(plan, free, theta, z, cov=fx["cov"], dlog=dlog, all_maps=True)
    assert n > 0 and field.alloc_count() == n
    for key in MAPS + ("nbad",):
        assert a[key].tobytes() == b[key].tobytes(), key
    # Moench parameters on the same field: the scratch plan cannot be refreshed, it is made anew -- one allocation
    _, _, M = load_deck("c3_moench")
    mfree, mtheta = ["Kr", "Sy", "MoenchAlpha[1]"], np.array([M.Kr, M.Sy, M.MoenchAlpha[1]])
    mplan = eng.Plan(M, mode="fast")
    c = field.forecast(mplan, mfree, mtheta, z, dlog=dlog, all_maps=True, with_stats=True)
    assert field.alloc_count() == n + 1
    check_slots(c, every_set_alone(eng, forecast_sets(M, mfree, mtheta, dlog), "fast", fx["wells"], fx["locations"], fx["times"], z,
                                   launched=False))
    check_combination(c, None, dlog)
    # ... and back
    d = field.forecast(plan, free, theta, z, cov=fx["cov"], dlog=dlog, all_maps=True)
    assert field.alloc_count() == n + 2
    for key in MAPS + ("nbad",):
        assert a[key].tobytes() == d[key].tobytes(), key
    field.close(); plan.close(); mplan.close()
