"""The fast evaluators' shared reciprocal seeds against the binary128 evaluation.

fast_eta takes |q| and 1/|q|^2 from one v_rsq_f64 seed (rsq_pair), and the folded water-table kernel with one depth per
launch (integrate_kernel<2, 1, ..., FOLD, ..., NZC = 1>, the lane = time grid of a fully penetrating well) takes e^{-Re eta}
and e^{-Re eta zD} from one reciprocal of their product (prim_pair).  Both add a rounding or two to a sample.  This test looks
at the C2 deck (Neuman 1974, fully penetrating) where those roundings could show: the smallest p of a sweep (large tD) at the
first tanh-sinh abscissae, where |q| = |p + a^2| is tiny; every point's abscissa loop runs Re eta up to and past maxexp = 12,
where E E_z is largest; the depths zD = 0 and zD = 1, one per call; both the lane = time layout (grid: the paired kernel)
and the lane = point layout (list: rsq_pair only).

Measure: per point, the level sums, J0-interval areas and totlap of ucf_debug_stages against Oracle(quad=True).point, each
in the max norm over the Laplace samples relative to the vector's largest modulus; the worst over the points of a regime.
Bar: 1.5 x what the same measurement gave for the library before the shared seeds (BEFORE, measured on an MI355X with
that library).  Measured, worst of level sums / interval areas / totlap, before -> after (both layouts alike):
    zD = 0  small p  1.4683e-06 -> 1.4683e-06      rest  2.8277e-05 -> 2.8277e-05
    zD = 1  small p  1.4686e-06 -> 1.4686e-06      rest  4.52036e-03 -> 4.52036e-03
The worst entries agree to 10 digits before and after: what sets them is not the roundings the shared seeds add, and this
bar keeps those roundings from ever growing to that size."""
import numpy as np
import pytest

from golden_util import load_deck

pytestmark = pytest.mark.gpu

DECK = "c2_neuman74_fullpen"
TD = np.array([1.0e-2, 1.0, 1.0e2, 1.0e4, 1.0e6, 1.0e8])      # the last two: the smallest p of a sweep
RD = np.array([0.05, 0.6, 4.0])
SMALL_P = 1.0e6
BEFORE = {
    ("grid", 0.0, "small_p"): 1.4682963536792738e-06, ("grid", 0.0, "rest"): 2.827721358821262e-05,
    ("grid", 1.0, "small_p"): 1.4686199781808164e-06, ("grid", 1.0, "rest"): 4.520355527139786e-03,
    ("list", 0.0, "small_p"): 1.4682963536792738e-06, ("list", 0.0, "rest"): 2.827721358821262e-05,
    ("list", 1.0, "small_p"): 1.4686199781808164e-06, ("list", 1.0, "rest"): 4.520355527139786e-03,
}
FACTOR = 1.5


def _vec_err(got, ref):
    scale = np.maximum(np.abs(ref).max(axis=-1, keepdims=True), 1e-300)
    return float((np.abs(got - ref) / scale).max())


def measure(engine, oracle_quad):
    """{(layout, zD, regime): worst error}: layout 'grid' (lane = time) or 'list' (lane = point)"""
    dk, ts, P = load_deck(DECK)
    D = oracle_quad.nondim(P)
    j0z = oracle_quad.j0_zeros(D.nj0z)
    sv = np.array(oracle_quad.split_vector(list(dk.j0s), TD), np.int32)
    plan = engine.Plan(P, mode="fast")
    R, nacc = P.R, P.nacc
    out = {}
    for zD in (0.0, 1.0):
        z = np.array([zD])
        zl = np.array(oracle_quad.zlay(D, z), np.int32)
        ref = {}
        for it, t in enumerate(TD):
            for ir, r in enumerate(RD):
                _, _, b = oracle_quad.point(P, D, j0z, t, r, sv[it], z, zl, stages=True)
                ref[it, ir] = b
        nt = len(TD)
        runs = {"grid": (plan.debug_stages(TD, sv, RD, z, zl, grid=True), lambda it, ir: it * len(RD) + ir),
                "list": (plan.debug_stages(np.tile(TD, len(RD)), np.tile(sv, len(RD)), np.repeat(RD, nt), z, zl, grid=False),
                         lambda it, ir: ir * nt + it)}
        for lay, (st, idx) in runs.items():
            assert st["has_state"]
            for it, t in enumerate(TD):
                for ir, r in enumerate(RD):
                    q = idx(it, ir)
                    b = ref[it, ir]
                    cz = lambda a: a[..., 0] + 1j * a[..., 1]
                    s = st["state"][q]                                            # [np, R+1+nacc, nz]
                    arg = j0z[sv[it] - 1] / r
                    tmp = np.transpose(s[:, :R, :], (1, 2, 0)) * (arg / 2.0)
                    gl = np.transpose(s[:, R + 1:, :], (1, 2, 0))
                    e = max(_vec_err(tmp, cz(b["tmp"])), _vec_err(gl, cz(b["glarea"])), _vec_err(st["totlap"][q], cz(b["totlap"])))
                    key = (lay, zD, "small_p" if t >= SMALL_P else "rest")
                    out[key] = max(out.get(key, 0.0), e)
    return out


@pytest.fixture(scope="module")
def engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import engine as e
    return e


def test_shared_seeds_keep_the_samples_accuracy(engine, oracle_quad):
    got = measure(engine, oracle_quad)
    assert set(got) == set(BEFORE)
    bad = {k: (v, BEFORE[k]) for k, v in got.items() if not v <= FACTOR * BEFORE[k]}
    assert not bad, bad
