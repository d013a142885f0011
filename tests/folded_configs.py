"""The configurations at which the folded one-depth water-table kernel (integrate_kernel<2, 1, W, false, FOLD, false, NZC = 1,
...>: what bench.py times) is held to the oracle, in one place: oracle/gen_midstages_folded.py writes a stage fixture per
entry, tests/test_folded_loop_classifiers_configs.py checks the classifiers' soundness at every entry on the CPU,
tests/test_midstages_folded.py the fixtures, tests/test_gpu_stages_folded.py the device.  A plain module, no conftest.

Every limit of the kernel's loop classifiers (zpair_unit_bounds / zpair_bound_limit, zpair_interval_class) is a function of the
plan's kappa, of the depth zD and of Re p, Im p (tD, M, alpha, tol).  An entry is a tag, overrides of the C2 deck
(Deck.replace; params_from_deck) and a depth:

    k003 / k04 / k4 x z04 / z1     kappa 0.03, 0.4, 4 at zD = 0.4 and at the water table, Neuman 1974 (model 5), beta = 0
    k04_z0_moench                  zD = 0: UCF_PH_SH is never set.  Moench's boundary (model 3, the alphas of the c3 deck) with
                                   d = 0 and l = b as C2 has them: dp.fold_dD and dp.fold_lD1 hold, plan_launch (ucf_launch_plan.h)
                                   picks the folded kernel for one depth, and tests/test_gpu_stages_folded.py asserts from
                                   plan.kernel_times() that it ran
    k003_beta2 / k4_beta2          Malama's boundary (model 4) with beta = 2: the BETA arm of the proven loops
    k003_malama_numerics           kappa 0.03 with the numerics of the Malama decks: M = 18 (37 Laplace samples), k = 7 (127
                                   tanh-sinh nodes), R = 5, 12 accelerated intervals of 38 Gauss-Lobatto nodes, split index 2.
                                   zD = 0.2: with the split index 2 the lowest interval starts at j0z[1] / 30 = 0.18, and only
                                   below zD = 0.35 sqrt(0.03) / 0.18 = 0.33 is there a cosh/sinh interval without UCF_PH_SH

The grid is the same for all: four waves of 64 times, half a decade each from 10^-2, 10, 10^4 and 10^7, times five radii."""
import numpy as np

DECK = "c2_neuman74_fullpen"
TD_CLUSTERS = (-2.0, 1.0, 4.0, 7.0)
RD = (0.05, 0.3, 2.0, 10.0, 30.0)
MOENCH = dict(model=3, MoenchM=3, MoenchAlpha=[0.000278, 0.0168, 0.416])
# tag, overrides of the deck, zD
CONFIGS = (
    ("k003_z04", dict(kappa=0.03), 0.4),
    ("k003_z1", dict(kappa=0.03), 1.0),
    ("k04_z04", dict(kappa=0.4), 0.4),
    ("k04_z1", dict(kappa=0.4), 1.0),
    ("k4_z04", dict(kappa=4.0), 0.4),
    ("k4_z1", dict(kappa=4.0), 1.0),
    ("k04_z0_moench", dict(kappa=0.4, **MOENCH), 0.0),
    ("k003_beta2", dict(kappa=0.03, model=4, beta=2.0), 0.4),
    ("k4_beta2", dict(kappa=4.0, model=4, beta=2.0), 0.9106),
    ("k003_malama_numerics", dict(kappa=0.03, M=18, k=7, R=5, nacc=12, ord=40, j0s=[2, 2]), 0.2),
)
TAGS = tuple(c[0] for c in CONFIGS)
assert len(CONFIGS) <= 10 and len(set(TAGS)) == len(TAGS)


# the loops of the kernel (UCF_IV_UNPROVEN, CS_TAB, CS_SHORT, EX_TAB, EX_SHORT and the two _SH twins), in the order of the
# model's CLASSES with the twins behind them: the codes of the fixtures' `loops` arrays
LOOPS = ("cs_tab", "cs_short", "ex_tab", "ex_short", "unproven", "cs_tab_sh", "cs_short_sh")


def reachable_loops(zD):
    """the loops a depth can reach at all.  zD = 0: sinh(eta zD) = 0 stays with its series, UCF_ZB_SH is infinite and the bit
    is never set -- no _SH twin.  zD = 1: the sin/cos argument of the exponential form is Im eta (1 - zD) = 0 < UCF_SC_SMALL
    at every node, UCF_ZB_YL is infinite and both classifiers call every exponential unit short -- no ex_tab."""
    out = [l for l in LOOPS if not (zD == 0.0 and l.endswith("_sh")) and not (zD == 1.0 and l == "ex_tab")]
    return tuple(out)


def reachable_classes(zD):
    return tuple(l for l in reachable_loops(zD) if not l.endswith("_sh"))


def times():
    """the 256 dimensionless times"""
    return np.concatenate([np.logspace(c, c + 0.5, 64) for c in TD_CLUSTERS])


def radii():
    return np.array(RD)


def config(tag):
    return next(c for c in CONFIGS if c[0] == tag)


def deck_of(tag):
    """(deck with the entry's overrides, its parameter block, zD)"""
    from golden_util import load_deck
    from unconfined_amd.abi import params_from_deck
    _, over, zD = config(tag)
    dk = load_deck(DECK)[0].replace(**over)
    return dk, params_from_deck(dk), zD
