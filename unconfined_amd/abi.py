"""ctypes mirrors of the POD structs in include/ucf.h (layout must match exactly;
tests/test_abi.py checks sizes/offsets against the compiled library)."""
from __future__ import annotations

import ctypes as C

UCF_MAX_MOENCH = 16
UCF_MAX_NZ = 32
UCF_MAX_LAP_M = 127
UCF_MAX_SCHEDULE = 100
UCF_FIT_MAX_PAR = 8
UCF_ENSEMBLE_MAX = 1024       # members of one ucf_field_ensemble
UCF_ENSEMBLE_MAX_Q = 16       # quantile levels, and drawdown limits, per call
UCF_WORTH_MAX_TGT = 16        # forecast targets of one ucf_field_worth
UCF_WORTH_MAX_PICK = 16       # wells that one ucf_field_worth picks
UCF_YIELD_MAX_CTL = 8         # controls of one ucf_field_yield
UCF_YIELD_MAX_PAT = 4096      # rate patterns of one ucf_field_yield
UCF_YIELD_PAT_TILE = 8        # patterns per workgroup of field_yield_kernel
UCF_ALLOC_MAX_OBJ = 8         # objectives of one ucf_field_allocate
UCF_ALLOC_MAX_ITER = 256      # the largest maxit of ucf_field_allocate
UCF_ALLOC_DTOL = 2.0 ** -40   # its ratio test: a D that is not above this times its scale is zero up to rounding
# the status of one linear programme of ucf_field_allocate
UCF_ALLOC_INVALID, UCF_ALLOC_OPTIMAL, UCF_ALLOC_ITERATION_CAP, UCF_ALLOC_INFEASIBLE_AT_ZERO, UCF_ALLOC_NUMERIC = -1, 0, 1, 2, 3
UCF_TIME_FIRST_ABOVE = 0      # kinds of ucf_field_ensemble_times: the first up-crossing of a limit
UCF_TIME_LAST_ABOVE = 1       # ... and the abscissa from which the value stays at or below it
UCF_SOBOL_MAX_BASE = 1024     # base rows N of one Saltelli design; ucf_field_sobol runs (npar + 2) N members
TIME_KINDS = {"first_above": UCF_TIME_FIRST_ABOVE, "last_above": UCF_TIME_LAST_ABOVE}
# parameter ids of a fit (enum UCF_PAR_* of include/ucf.h); a Moench alpha is PAR_MOENCH_ALPHA0 + i
PAR_KR, PAR_KAPPA, PAR_SS, PAR_SY, PAR_AC, PAR_AK, PAR_USL, PAR_MOENCH_ALPHA0 = range(8)
PAR_IDS = {"Kr": PAR_KR, "kappa": PAR_KAPPA, "Ss": PAR_SS, "Sy": PAR_SY, "ac": PAR_AC, "ak": PAR_AK, "usL": PAR_USL}
# status of a start of ucf_fit_lm (enum UCF_FIT_*)
FIT_CONVERGED, FIT_MAX_ITER, FIT_SINGULAR, FIT_NONFINITE_START = range(4)
# iz of an observation of ucf_fit_create_network / ucf_fit_create_field that is the screen average of its well's depths (UCF_FIT_SCREEN)
FIT_SCREEN = -1
# source of ucf_debug_fit_reduce: how an observation finds its simulated value in h
FIT_SLOTS, FIT_NETWORK, FIT_FIELD = range(3)
# loss of a fit (enum UCF_LOSS_* of include/ucf.h: ucf_fit_set_loss)
LOSS_L2, LOSS_HUBER, LOSS_TUKEY = range(3)
LOSS_KINDS = {"l2": LOSS_L2, "huber": LOSS_HUBER, "tukey": LOSS_TUKEY}
# kind of ucf_fit_resample_cov (enum UCF_RESAMPLE_*)
RESAMPLE_BOOTSTRAP, RESAMPLE_JACKKNIFE = range(2)
RESAMPLE_KINDS = {"bootstrap": RESAMPLE_BOOTSTRAP, "jackknife": RESAMPLE_JACKKNIFE}
UCF_ERR_BAD_ARGUMENT, UCF_ERR_NO_DEVICE, UCF_ERR_SINGULAR = -11, -12, -16


class UcfParams(C.Structure):
    _fields_ = [
        ("model", C.c_int), ("MNtype", C.c_int), ("order", C.c_int), ("timeType", C.c_int),
        ("timePar", C.c_double * 2),
        ("Q", C.c_double), ("l", C.c_double), ("d", C.c_double), ("rw", C.c_double), ("rc", C.c_double),
        ("gammaSkin", C.c_double), ("b", C.c_double), ("Kr", C.c_double), ("kappa", C.c_double),
        ("Ss", C.c_double), ("Sy", C.c_double), ("beta", C.c_double),
        ("MoenchM", C.c_int), ("_pad0", C.c_int),
        ("MoenchAlpha", C.c_double * UCF_MAX_MOENCH),
        ("ac", C.c_double), ("ak", C.c_double), ("psia", C.c_double), ("psik", C.c_double), ("usL", C.c_double),
        ("M", C.c_int), ("k", C.c_int), ("R", C.c_int), ("nacc", C.c_int), ("ord", C.c_int),
        ("j0s", C.c_int * 2), ("_pad1", C.c_int),
        ("alpha", C.c_double), ("tol", C.c_double),
        ("rwobs", C.c_double), ("sF", C.c_double),
        ("timeParExt", C.c_double * (2 * UCF_MAX_SCHEDULE + 1)),
    ]


class UcfDerived(C.Structure):
    _fields_ = [
        ("Lc", C.c_double), ("Tc", C.c_double), ("Hc", C.c_double),
        ("sigma", C.c_double), ("alphaD", C.c_double), ("betaD", C.c_double),
        ("lD", C.c_double), ("dD", C.c_double), ("bD", C.c_double), ("rDw", C.c_double), ("rDwobs", C.c_double),
        ("acD", C.c_double), ("akD", C.c_double), ("lambdaD", C.c_double), ("psiaD", C.c_double),
        ("psikD", C.c_double), ("usLD", C.c_double), ("b1", C.c_double), ("PsiD", C.c_double),
        ("MoenchGamma", C.c_double * UCF_MAX_MOENCH),
        ("l_eff", C.c_double), ("d_eff", C.c_double), ("ac_eff", C.c_double),
        ("np", C.c_int), ("N", C.c_int), ("nj0z", C.c_int), ("nabs", C.c_int),
    ]


class UcfStats(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in
                ("nan_scrubbed", "zero_vectors", "wynn_truncated", "wynn_sentinel", "wynn_early_exit", "wynn_all_zero")]


class UcfFitOptions(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("dlog", C.c_double), ("lambda0", C.c_double), ("lambda_up", C.c_double),
                ("lambda_down", C.c_double), ("tol_step", C.c_double), ("tol_phi", C.c_double)]


class UcfEnsembleMaps(C.Structure):
    """ucf_ensemble_maps: the statistics of one map of an ensemble; every address may be NULL"""
    _fields_ = [("mean", C.c_void_p), ("sd", C.c_void_p), ("min", C.c_void_p), ("max", C.c_void_p), ("quant", C.c_void_p),
                ("all", C.c_void_p), ("nfin", C.c_void_p)]


class UcfSobolMaps(C.Structure):
    """ucf_sobol_maps: the Sobol statistics of one map of a Saltelli design; every address may be NULL"""
    _fields_ = [("S", C.c_void_p), ("ST", C.c_void_p), ("seS", C.c_void_p), ("seST", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p),
                ("all", C.c_void_p), ("nrow", C.c_void_p)]


def params_from_deck(dk) -> UcfParams:
    """Deck (unconfined_amd.deck.Deck) -> ucf_params; values only, no arithmetic."""
    P = UcfParams()
    P.model, P.MNtype, P.order, P.timeType = dk.model, dk.MNtype, dk.order, dk.timeType
    tp = list(dk.timePar) + [0.0, 0.0]
    P.timePar[0], P.timePar[1] = tp[0], tp[1]
    if dk.timeType < 0:
        for i, v in enumerate(dk.timePar[:2 * UCF_MAX_SCHEDULE + 1]):
            P.timeParExt[i] = v
    for n in ("Q", "l", "d", "rw", "rc", "gammaSkin", "b", "Kr", "kappa", "Ss", "Sy", "beta",
              "ac", "ak", "psia", "psik", "usL", "alpha", "tol", "rwobs", "sF"):
        setattr(P, n, float(getattr(dk, n)))
    P.MoenchM = dk.MoenchM
    for i, a in enumerate(dk.MoenchAlpha[:UCF_MAX_MOENCH]):
        P.MoenchAlpha[i] = a
    P.M, P.k, P.R, P.nacc, P.ord = dk.M, dk.k, dk.R, dk.nacc, dk.ord
    P.j0s[0], P.j0s[1] = dk.j0s
    return P
