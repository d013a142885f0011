"""ucf_field_drawdown on the GPU (fixtures: tools/gen_field_fixture.py): the superposed drawdown of 4 wells in 2 start-time
groups at 5 locations, 6 times and 2 depths, decks neuman74_partpen, c2_neuman74_fullpen and c1_theis.

Bounds.  The sums are checked bit for bit against the stated arithmetic (numpy on the results of ucf_drawdown_grid for the
arrays of ucf_field_group).  Against the oracle a launched value is held to b = gate(ref, noise) of tests/test_gpu_fit.py
(max(1e-10, 10 x the oracle's distance from its binary128 build at that value) x max(|ref|, 1e-3), dimensional), and an
output to sum_j |q_j| tfac b_j -- the triangle inequality over its terms (tfac = 1 for s); the roundings of the sum itself,
a few u of the largest term, are five orders of magnitude below the 1e-10 floor of b."""
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck

pytestmark = pytest.mark.gpu

DECKS = ["neuman74_partpen", "c2_neuman74_fullpen", "c1_theis"]
MODES = ["faithful", "fast"]
UNIT = {"neuman74_partpen": 100.0, "c2_neuman74_fullpen": 100.0, "c1_theis": 3.0}


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine
    return engine


def gate(ref, noise):
    return np.maximum(1e-10, 10.0 * noise) * np.maximum(np.abs(ref), 1e-3)


def superpose(wells, groups, h, dh, nt, nloc, nz, scale):
    """the arithmetic of field_superpose_kernel as include/ucf.h states it; h[g], dh[g]: [nt_g][nr_g][nz] (None: not launched)"""
    s = np.zeros((nt, nloc, nz)); ds = np.zeros((nt, nloc, nz))
    owner = [next(g for g, grp in enumerate(groups) if grp["col"][0, j] >= 0) for j in range(len(wells))]
    for k in range(nt):
        for i in range(nloc):
            for iz in range(nz):
                a = b = np.float64(0.0)
                for j in range(len(wells)):
                    grp = groups[owner[j]]
                    if k < grp["k0"]:
                        continue
                    kk, c = k - grp["k0"], grp["col"][i, j]
                    a = a + wells[j, 2] * h[owner[j]][kk, c, iz]
                    b = b + wells[j, 2] * (grp["tfac"][kk] * dh[owner[j]][kk, c, iz])
                if scale is not None:
                    a, b = a * scale, b * scale
                s[k, i, iz], ds[k, i, iz] = a, b
    return s, ds


def direct(plan, groups, z):
    """ucf_drawdown_grid once per group with the arrays of ucf_field_group (dimensionless h, dh)"""
    zD = z / plan.derived.Lc
    zl = plan.zlay(zD)
    out = [plan.drawdown_grid(g["tD"], g["sv"], g["rD"], zD, zl) if len(g["tD"]) else (None, None) for g in groups]
    return [o[0] for o in out], [o[1] for o in out]


_cache = {}


def case(eng, deck, mode):
    """(fixture, plan, field, groups, directly called h and dh per group) -- computed once per deck and flavour"""
    if (deck, mode) not in _cache:
        from unconfined_amd import WellField
        fx = np.load(os.path.join(GOLD, f"field_{deck}.npz"))
        _, _, P = load_deck(deck)
        plan = eng.Plan(P, mode=mode)
        field = WellField(fx["wells"], fx["locations"], fx["times"])
        groups = field.groups(plan)
        h, dh = direct(plan, groups, fx["z"])
        _cache[(deck, mode)] = (fx, P, plan, field, groups, h, dh)
    return _cache[(deck, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_the_sum_is_the_stated_arithmetic(eng, deck, mode):
    fx, P, plan, field, groups, h, dh = case(eng, deck, mode)
    # what is launched is what the fixture was made for, and the plan states what its parameter set states
    for g, (a, b) in enumerate(zip(groups, field.groups(P))):
        assert a["k0"] == b["k0"] == int(fx[f"g{g}_k0"])
        for key in ("tD", "sv", "rD", "col", "tfac"):
            assert a[key].tobytes() == b[key].tobytes() == fx[f"g{g}_{key}"].tobytes(), (g, key)
    nt, nloc, nz = len(fx["times"]), len(fx["locations"]), len(fx["z"])
    for dimensionless, scale in ((True, None), (False, plan.derived.Hc)):
        want_s, want_ds = superpose(fx["wells"], groups, h, dh, nt, nloc, nz, scale)
        s, ds = field.drawdown(plan, fx["z"], dimensionless=dimensionless)
        assert s.tobytes() == want_s.tobytes(), (deck, mode, dimensionless, np.abs(s - want_s).max())
        assert ds.tobytes() == want_ds.tobytes(), (deck, mode, dimensionless, np.abs(ds - want_ds).max())
    assert np.isfinite(s).all() and np.isfinite(ds).all()
    assert (s[:2, :, :] != 0.0).all()                 # before the later start the first group alone


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_a_single_well_is_the_grid_entry(eng, deck, mode):
    """q = 1, t0 = 0 at the origin, locations in order of distance: 0 + 1 x h and 1 x (t / (t - 0) x dh) are h and dh themselves"""
    from unconfined_amd import WellField
    fx, P, plan, _, _, _, _ = case(eng, deck, mode)
    loc = np.array([[0.3, 0.4], [1.0, 0.0], [-0.9, 1.2], [0.0, -2.5]]) * UNIT[deck]
    field = WellField([(0.0, 0.0, 1.0, 0.0)], loc, fx["times"])
    (g,) = field.groups(plan)
    assert g["col"].ravel().tolist() == [0, 1, 2, 3] and (g["tfac"] == 1.0).all()
    D = plan.derived
    tD, rD, zD = fx["times"] / D.Tc, np.sqrt(loc[:, 0] * loc[:, 0] + loc[:, 1] * loc[:, 1]) / D.Lc, fx["z"] / D.Lc
    assert g["tD"].tobytes() == tD.tobytes() and g["rD"].tobytes() == rD.tobytes()
    h, dh, st = plan.drawdown_grid(tD, plan.split_vector(tD), rD, zD, plan.zlay(zD), with_stats=True)
    s, ds, fst = field.drawdown(plan, fx["z"], dimensionless=True, with_stats=True)
    assert s.tobytes() == h.tobytes() and ds.tobytes() == dh.tobytes()
    assert fst == st
    field.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("deck", DECKS)
def test_against_the_oracle(eng, deck, mode):
    fx, P, plan, field, groups, h, dh = case(eng, deck, mode)
    Hc = plan.derived.Hc
    wells = fx["wells"]
    # the launched values first, term by term: the grid path itself
    b_h, b_dh, worst = [], [], 0.0
    for g in range(len(groups)):
        for name, got, keep in (("h", h[g], b_h), ("dh", dh[g], b_dh)):
            ref, b = fx[f"g{g}_ref_{name}"], gate(fx[f"g{g}_ref_{name}"], fx[f"g{g}_noise_{name}"])
            err = np.abs(got * Hc - ref)
            worst = max(worst, float((err / b).max()))
            print(f"[field {deck} {mode}] group {g} {name}: worst |grid - oracle| / b = {float((err / b).max()):.3f}")
            keep.append(b)
            assert (err <= b).all(), (deck, mode, g, name, float((err / b).max()))
    # the outputs: sum_j |q_j| tfac b_j
    nt, nloc, nz = len(fx["times"]), len(fx["locations"]), len(fx["z"])
    one = [dict(g, tfac=np.ones_like(g["tfac"])) for g in groups]
    absw = wells.copy(); absw[:, 2] = np.abs(wells[:, 2])
    bound_s, _ = superpose(absw, one, b_h, b_h, nt, nloc, nz, None)
    _, bound_ds = superpose(absw, groups, b_dh, b_dh, nt, nloc, nz, None)
    s, ds = field.drawdown(plan, fx["z"])
    for name, got, ref, bound in (("s", s, fx["s_ref"], bound_s), ("ds", ds, fx["ds_ref"], bound_ds)):
        err = np.abs(got - ref)
        print(f"[field {deck} {mode}] {name}: worst |field - oracle| / bound = {float((err / bound).max()):.3f}")
        assert (bound > 0.0).all()
        assert (err <= bound).all(), (deck, mode, name, float((err / bound).max()))


@pytest.mark.parametrize("deck", DECKS)
def test_constant_head_boundary(eng, deck):
    """a well at the origin and its image in x = 2 of opposite sign: on the line both distances share one column and the
    terms cancel exactly; between well and line the drawdown is positive and below that of the well alone"""
    from unconfined_amd import WellField, images
    fx, P, plan, _, _, _, _ = case(eng, deck, "fast")
    u = UNIT[deck]
    well = [(0.0, 0.0, 1.0, 0.0)]
    loc = np.array([[2.0, 0.0], [2.0, 3.0], [1.0, 0.0]]) * u
    field = WellField(images(well, (1.0, 0.0, 2.0 * u), "constant_head"), loc, fx["times"])
    alone = WellField(well, loc, fx["times"])
    s, ds = field.drawdown(plan, fx["z"])
    s1, _ = alone.drawdown(plan, fx["z"])
    zero = np.zeros((len(fx["times"]), 2, len(fx["z"])))
    assert s[:, :2, :].tobytes() == zero.tobytes() and ds[:, :2, :].tobytes() == zero.tobytes()
    assert (s[:, 2, :] > 0.0).all() and (s[:, 2, :] < s1[:, 2, :]).all(), (s[:, 2, :], s1[:, 2, :])
    field.close(); alone.close()


@pytest.mark.parametrize("deck", DECKS)
def test_repetition(eng, deck):
    from unconfined_amd import WellField
    from unconfined_amd.abi import UcfParams
    fx, P, _, _, _, _, _ = case(eng, deck, "fast")
    plan = eng.Plan(P, mode="fast")
    field = WellField(fx["wells"], fx["locations"], fx["times"])
    a = field.drawdown(plan, fx["z"])
    n = field.alloc_count()
    b = field.drawdown(plan, fx["z"])
    assert n > 0 and field.alloc_count() == n
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # other parameters through ucf_plan_update: the result of a fresh field on a fresh plan
    P2 = UcfParams.from_buffer_copy(P)
    P2.Kr, P2.Sy = P.Kr * 1.7, P.Sy * 0.6
    plan.update(P2)
    c = field.drawdown(plan, fx["z"])
    assert field.alloc_count() == n
    fresh_plan = eng.Plan(P2, mode="fast")
    fresh = WellField(fx["wells"], fx["locations"], fx["times"])
    d = fresh.drawdown(fresh_plan, fx["z"])
    assert c[0].tobytes() == d[0].tobytes() and c[1].tobytes() == d[1].tobytes()
    assert c[0].tobytes() != a[0].tobytes()
    field.close(); fresh.close()
