"""ctypes binding of the product library ``unconfined_amd/libucf.so`` (the C ABI of
include/ucf.h: HIP kernels for gfx950 + host-side plan builder).

There is deliberately no fallback: if the shared library is missing or no HIP
device is usable, every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .abi import UcfDerived, UcfEnsembleMaps, UcfFitOptions, UcfParams, UcfSobolMaps, UcfStats

HERE = os.path.dirname(os.path.abspath(__file__))
# UCF_LIB_PATH: an experimental build of the SAME library (tools/ubench/build_variant.sh) for A/B timing; the product
# path is unconfined_amd/libucf.so and nothing else is ever loaded without that variable
LIB_PATH = os.environ.get("UCF_LIB_PATH") or os.path.join(HERE, "libucf.so")

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

EXPORTS = [
    "ucf_version", "ucf_last_error", "ucf_status_string",
    "ucf_plan_create", "ucf_plan_create_on", "ucf_device_count", "ucf_plan_destroy", "ucf_plan_update", "ucf_plan_derived", "ucf_nondimensionalise", "ucf_plan_j0z", "ucf_plan_tanh_sinh",
    "ucf_plan_gauss_lobatto", "ucf_plan_set_mode", "ucf_plan_set_timing", "ucf_plan_kernel_ms", "ucf_plan_kernel_times",
    "ucf_plan_reserve", "ucf_plan_alloc_count", "ucf_build_id",
    "ucf_shard_rows", "ucf_drawdown_grid_shard_device", "ucf_drawdown_grid_multi", "ucf_drawdown_batch_multi",
    "ucf_drawdown_grid_allgather", "ucf_comm_unique_id", "ucf_comm_create", "ucf_comm_destroy",
    "ucf_logspace", "ucf_linspace", "ucf_zlay", "ucf_split_vector",
    "ucf_drawdown_batch", "ucf_drawdown_batch_device", "ucf_drawdown_grid", "ucf_drawdown_grid_device",
    "ucf_drawdown_multi", "ucf_screen_average",
    "ucf_eval_samples", "ucf_pvalues", "ucf_dehoog", "ucf_wynn_epsilon", "ucf_extraptozero", "ucf_bessel_k01",
    "ucf_debug_stages", "ucf_debug_wynn", "ucf_debug_dehoog_tiles",
    "ucf_fp64_fma_peak", "ucf_sincos_table", "ucf_exp2_table",
    "ucf_fit_perturb", "ucf_fit_solve_step", "ucf_fit_default_options", "ucf_fit_create", "ucf_fit_destroy", "ucf_fit_evaluate",
    "ucf_fit_lm", "ucf_fit_alloc_count",
    "ucf_fit_create_network", "ucf_fit_eval_counts", "ucf_fit_network_eval_counts", "ucf_fit_debug_h",
    "ucf_fit_create_field", "ucf_fit_field_terms",
    "ucf_fit_derivative_check", "ucf_fit_set_derivative", "ucf_fit_evaluate_joint", "ucf_fit_debug_dh",
    "ucf_field_create", "ucf_field_destroy", "ucf_field_group_count", "ucf_field_group", "ucf_field_group_from_params",
    "ucf_field_drawdown", "ucf_field_alloc_count", "ucf_field_images",
    "ucf_field_forecast_sets", "ucf_field_forecast",
    "ucf_field_ensemble", "ucf_field_ensemble_draw", "ucf_debug_ensemble", "ucf_debug_fit_reduce",
    "ucf_fit_objective", "ucf_ensemble_quantise", "ucf_ensemble_likelihood_weights", "ucf_field_ensemble_weighted",
    "ucf_debug_ensemble_weighted",
    "ucf_field_worth", "ucf_worth_condition", "ucf_debug_field_worth",
    "ucf_field_yield", "ucf_debug_field_yield",
    "ucf_field_allocate", "ucf_debug_field_allocate", "ucf_allocate_solve", "ucf_allocate_select",
    "ucf_field_ensemble_times", "ucf_debug_field_times",
    "ucf_sobol_design", "ucf_field_sobol", "ucf_debug_sobol",
    "ucf_fit_loss_terms", "ucf_fit_robust_scale", "ucf_fit_set_loss", "ucf_fit_get_loss", "ucf_fit_loss_report", "ucf_debug_fit_reduce_loss",
    "ucf_fit_set_resample", "ucf_fit_evaluate_resampled", "ucf_fit_objective_resampled", "ucf_fit_lm_resampled",
    "ucf_fit_resample_blocks", "ucf_fit_resample_jackknife", "ucf_fit_resample_cov", "ucf_debug_fit_reduce_resampled",
]


class UcfError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"ucf status {status}: {message}")
        self.status = status
        self.message = message


def build(verbose: bool = False) -> str:
    """compile the HIP library in-tree (hipcc, gfx950); returns the .so path"""
    res = subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j6"], capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode:
        raise RuntimeError("building libucf.so failed")
    return LIB_PATH


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the drawdown path)")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.ucf_version.restype = C.c_int
    lib.ucf_last_error.restype = C.c_char_p
    lib.ucf_status_string.restype = C.c_char_p
    lib.ucf_status_string.argtypes = [C.c_int]
    lib.ucf_plan_create.argtypes = [C.POINTER(UcfParams), C.POINTER(vp)]
    lib.ucf_plan_destroy.argtypes = [vp]
    lib.ucf_plan_create_on.argtypes = [C.POINTER(UcfParams), C.c_int, C.POINTER(vp)]
    lib.ucf_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.ucf_plan_update.argtypes = [vp, C.POINTER(UcfParams)]
    lib.ucf_plan_destroy.restype = None
    lib.ucf_plan_derived.argtypes = [vp, C.POINTER(UcfDerived)]
    lib.ucf_nondimensionalise.argtypes = [C.POINTER(UcfParams), C.POINTER(UcfDerived)]
    lib.ucf_plan_j0z.argtypes = [vp, C.c_int, _dp]
    lib.ucf_plan_tanh_sinh.argtypes = [vp, C.c_int, C.c_int, _dp, vp]
    lib.ucf_plan_gauss_lobatto.argtypes = [vp, C.c_int, _dp, _dp]
    lib.ucf_plan_set_mode.argtypes = [vp, C.c_int]
    lib.ucf_plan_set_timing.argtypes = [vp, C.c_int]
    lib.ucf_plan_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    lib.ucf_plan_kernel_times.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    lib.ucf_plan_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.ucf_plan_alloc_count.argtypes = [vp]
    lib.ucf_plan_alloc_count.restype = C.c_longlong
    lib.ucf_build_id.restype = C.c_char_p
    lib.ucf_shard_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.ucf_drawdown_grid_shard_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, _dp, _ip, vp, vp, vp, vp]
    lib.ucf_drawdown_grid_allgather.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, _dp, _ip, vp, vp, vp, vp, vp]
    lib.ucf_comm_unique_id.argtypes = [C.c_char_p]
    lib.ucf_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    lib.ucf_comm_destroy.argtypes = [vp]
    lib.ucf_drawdown_grid_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, _dp, _ip, C.c_int, _dp, C.c_int, _dp, _ip, _dp, _dp,
                                            C.POINTER(UcfStats)]
    lib.ucf_drawdown_batch_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, _dp, _dp, _ip, C.c_int, _dp, _ip, _dp, _dp, C.POINTER(UcfStats)]
    lib.ucf_logspace.argtypes = [C.c_int, C.c_int, C.c_int, _dp]
    lib.ucf_linspace.argtypes = [C.c_double, C.c_double, C.c_int, _dp]
    lib.ucf_zlay.argtypes = [vp, C.c_int, _dp, _ip]
    lib.ucf_split_vector.argtypes = [vp, C.c_int, _dp, _ip]
    lib.ucf_drawdown_batch.argtypes = [vp, C.c_int, _dp, _dp, _ip, C.c_int, _dp, _ip, _dp, _dp, C.POINTER(UcfStats)]
    lib.ucf_drawdown_batch_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, _dp, _ip, vp, vp, vp, vp]
    lib.ucf_drawdown_grid.argtypes = [vp, C.c_int, _dp, _ip, C.c_int, _dp, C.c_int, _dp, _ip, _dp, _dp, C.POINTER(UcfStats)]
    lib.ucf_drawdown_grid_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, _dp, _ip, vp, vp, vp, vp]
    lib.ucf_drawdown_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp]
    lib.ucf_screen_average.argtypes = [C.c_int, C.c_int, _dp, _dp]
    lib.ucf_eval_samples.argtypes = [vp, C.c_int, _dp, C.c_double, C.c_int, _dp, C.c_int, _dp, _ip, _dp]
    lib.ucf_pvalues.argtypes = [vp, C.c_double, _dp]
    lib.ucf_dehoog.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp, _dp, _dp]
    lib.ucf_wynn_epsilon.argtypes = [C.c_int, C.c_int, _dp, _dp, _ip]
    lib.ucf_extraptozero.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
    lib.ucf_bessel_k01.argtypes = [C.c_int, _dp, _dp, _ip]
    lib.ucf_debug_stages.argtypes = [vp, C.c_int, C.c_int, _dp, _ip, C.c_int, _dp, C.c_int, _dp, _ip, _dp, _ip, _dp, _dp, _dp, _ip]
    lib.ucf_debug_wynn.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp, _ip]
    lib.ucf_debug_dehoog_tiles.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp, _dp, _dp]
    lib.ucf_fp64_fma_peak.argtypes = [C.POINTER(C.c_double)]
    lib.ucf_sincos_table.argtypes = [C.POINTER(C.c_double)]
    lib.ucf_exp2_table.argtypes = [C.POINTER(C.c_double)]
    lib.ucf_fit_perturb.argtypes = [C.POINTER(UcfParams), C.c_int, _ip, _dp, C.POINTER(UcfParams)]
    lib.ucf_fit_solve_step.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp]
    lib.ucf_fit_default_options.argtypes = [C.POINTER(UcfFitOptions)]
    lib.ucf_fit_create.argtypes = [C.POINTER(UcfParams), C.c_int, _ip, C.c_int, _dp, _dp, _ip, C.c_int, _dp, _dp, _dp, C.c_int, C.POINTER(vp)]
    lib.ucf_fit_destroy.argtypes = [vp]
    lib.ucf_fit_destroy.restype = None
    lib.ucf_fit_evaluate.argtypes = [vp, C.c_int, _dp, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.ucf_fit_lm.argtypes = [vp, C.c_int, _dp, C.POINTER(UcfFitOptions), _dp, _dp, _ip, _ip, vp]
    lib.ucf_fit_alloc_count.argtypes = [vp]
    lib.ucf_fit_alloc_count.restype = C.c_longlong
    lib.ucf_fit_create_network.argtypes = [C.POINTER(UcfParams), C.c_int, _ip, C.c_int, _dp, _ip, _dp, C.c_int, _dp, _ip, _ip, _dp, _dp, C.c_int,
                                           C.POINTER(vp)]
    lib.ucf_fit_eval_counts.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.ucf_fit_network_eval_counts.argtypes = [C.c_int, _ip, C.c_int, _dp, _ip, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.ucf_fit_debug_h.argtypes = [vp, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]
    lib.ucf_fit_create_field.argtypes = [C.POINTER(UcfParams), C.c_int, _ip, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _ip, _dp,
                                         C.c_int, _dp, _ip, _ip, _dp, _dp, C.c_int, C.POINTER(vp)]
    lib.ucf_fit_field_terms.argtypes = [C.POINTER(UcfParams), C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _ip,
                                        C.POINTER(C.c_int), _ip, _dp, _ip, _ip, _ip, _dp]
    lib.ucf_fit_derivative_check.argtypes = [C.c_int, vp, vp, C.POINTER(C.c_int)]
    lib.ucf_fit_set_derivative.argtypes = [vp, vp, vp]
    lib.ucf_fit_evaluate_joint.argtypes = [vp, C.c_int, _dp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.ucf_fit_debug_dh.argtypes = [vp, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(C.c_int)]
    lib.ucf_field_create.argtypes = [C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, C.POINTER(vp)]
    lib.ucf_field_destroy.argtypes = [vp]
    lib.ucf_field_destroy.restype = None
    lib.ucf_field_group_count.argtypes = [vp, C.POINTER(C.c_int)]
    _group_out = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, _ip, C.POINTER(C.c_int), _dp, _ip, _dp]
    lib.ucf_field_group.argtypes = [vp, vp] + _group_out
    lib.ucf_field_group_from_params.argtypes = [vp, C.POINTER(UcfParams)] + _group_out
    lib.ucf_field_drawdown.argtypes = [vp, vp, C.c_int, _dp, C.c_int, _dp, _dp, C.POINTER(UcfStats)]
    lib.ucf_field_alloc_count.argtypes = [vp]
    lib.ucf_field_alloc_count.restype = C.c_longlong
    lib.ucf_field_images.argtypes = [C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp, _dp, _dp]
    lib.ucf_field_forecast_sets.argtypes = [C.POINTER(UcfParams), C.c_int, vp, vp, C.c_double, C.POINTER(UcfParams)]
    # ids, theta, cov and every output may be NULL: plain addresses
    lib.ucf_field_forecast.argtypes = [vp, vp, C.c_int, vp, vp, C.c_double, vp, C.c_int, vp] + [vp] * 8 + [vp, C.POINTER(UcfStats)]
    # ids, thetas, z, q, limit and every output may be NULL: plain addresses
    lib.ucf_field_ensemble.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp,
                                       C.POINTER(UcfEnsembleMaps), C.POINTER(UcfEnsembleMaps), vp, vp, C.POINTER(UcfStats)]
    lib.ucf_field_ensemble_draw.argtypes = [C.c_int, vp, vp, C.c_int, C.c_ulonglong, vp]
    lib.ucf_debug_ensemble.argtypes = [C.c_int, C.c_longlong, vp, C.c_int, vp, C.c_int, vp, C.POINTER(UcfEnsembleMaps), vp, vp]
    # theta and every output may be NULL: plain addresses
    lib.ucf_fit_objective.argtypes = [vp, C.c_int] + [vp] * 6
    lib.ucf_ensemble_quantise.argtypes = [C.c_int, vp, vp, vp]
    lib.ucf_ensemble_likelihood_weights.argtypes = [C.c_int, vp, vp, C.c_double, vp, vp, vp]
    # as ucf_field_ensemble, the weights behind thetas, u, ess and nlaunched at the end
    lib.ucf_field_ensemble_weighted.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp,
                                                C.POINTER(UcfEnsembleMaps), C.POINTER(UcfEnsembleMaps), vp, vp, C.POINTER(UcfStats), vp, vp, vp]
    lib.ucf_debug_ensemble_weighted.argtypes = [C.c_int, C.c_longlong, vp, vp, C.c_int, vp, C.c_int, vp, C.POINTER(UcfEnsembleMaps), vp, vp]
    # every array may be NULL: plain addresses.  field, plan, npar, ids, theta, dlog, cov, nz, z | sigma_s, sigma_d, tsel | ntgt,
    # tgt, tw | npick, cmask | prior, post, crit, nused, pick, cov_post | stats
    lib.ucf_field_worth.argtypes = ([vp, vp, C.c_int, vp, vp, C.c_double, vp, C.c_int, vp] + [C.c_double, C.c_double, vp] + [C.c_int, vp, vp] +
                                    [C.c_int, vp] + [vp] * 6 + [C.POINTER(UcfStats)])
    lib.ucf_worth_condition.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp]
    # npar, nt, ncand, a_s, a_d, two_dlog, F, ws, wd, tsel, ntgt, A, tw, post, crit, nused
    lib.ucf_debug_field_worth.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, C.c_double, vp, C.c_double, C.c_double, vp, C.c_int, vp, vp, vp, vp, vp]
    # every array may be NULL: plain addresses.  field, plan, npar, ids, nens, thetas, weight, nz, z | nctl, ctl, npat, x, limit,
    # smax | nq, q, nlev, level | ystat, pexc, pfeas | hi, lo, bind, dead | resp, con, ncon, nbad | stats | u, ess, nlaunched
    lib.ucf_field_yield.argtypes = ([vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp] + [C.c_int, vp, C.c_int, vp, vp, C.c_double] +
                                    [C.c_int, vp, C.c_int, vp] + [C.POINTER(UcfEnsembleMaps), vp, vp] + [vp] * 4 + [vp] * 4 +
                                    [C.POINTER(UcfStats)] + [vp] * 3)
    # nctl, nens, ncon, npat, R, x, limit_con, con, smax, y, fe, hi, lo, bind, dead, nbad
    lib.ucf_debug_field_yield.argtypes = [C.c_int] * 4 + [vp] * 4 + [C.c_double] + [vp] * 7
    # every array may be NULL: plain addresses.  field, plan, npar, ids, nens, thetas, weight, nz, z | nctl, ctl | nobj, w, xmax,
    # maxit | limit | x, g, status, iters, work, lam | nq, q | quant, value, best, best_x, gquant | resp, con, ncon, nbad | stats | u,
    # ess, nlaunched
    lib.ucf_field_allocate.argtypes = ([vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp] + [C.c_int, vp] + [C.c_int, vp, vp, C.c_int] + [vp] +
                                       [vp] * 6 + [C.c_int, vp] + [vp] * 5 + [vp] * 4 + [C.POINTER(UcfStats)] + [vp] * 3)
    # nctl, nens, ncon, nobj, R, limit_con, con, w, xmax, maxit, x, g, status, iters, work, lam, nbad
    lib.ucf_debug_field_allocate.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.c_int] + [vp] * 7
    # nctl, ncon, R_m, limit_con, nobj, w, xmax, maxit, x, g, status, iters, work, lam
    lib.ucf_allocate_solve.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 6
    # nq, nens, nobj, nctl, quant, g, x, value, best, best_x
    lib.ucf_allocate_select.argtypes = [C.c_int] * 4 + [vp] * 6
    # every array may be NULL: plain addresses.  field, plan, npar, ids, nens, thetas, weight, nz, z | tau, tau_never | nlim, limit,
    # kind | nq, q, nhor, horizon | T, plater, nbad | stats | u, ess, nlaunched
    lib.ucf_field_ensemble_times.argtypes = ([vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp] + [vp, C.c_double] + [C.c_int, vp, vp] +
                                             [C.c_int, vp, C.c_int, vp] + [C.POINTER(UcfEnsembleMaps), vp, vp] + [C.POINTER(UcfStats)] + [vp] * 3)
    # nens, nt, nsite, a, tau, tau_never, nlim, limit, kind, T
    lib.ucf_debug_field_times.argtypes = [C.c_int, C.c_int, C.c_longlong, vp, vp, C.c_double, C.c_int, vp, vp, vp]
    # every array may be NULL: plain addresses.  npar, nbase, draws, thetas
    lib.ucf_sobol_design.argtypes = [C.c_int, C.c_int, vp, vp]
    # field, plan, npar, ids, nbase, thetas, nz, z | s, ds | nbad | stats
    lib.ucf_field_sobol.argtypes = ([vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp] + [C.POINTER(UcfSobolMaps), C.POINTER(UcfSobolMaps)] +
                                    [vp, C.POINTER(UcfStats)])
    # npar, nbase, nout, a, out, nbad
    lib.ucf_debug_sobol.argtypes = [C.c_int, C.c_int, C.c_longlong, vp, C.POINTER(UcfSobolMaps), vp]
    # every array may be NULL for a source or a call that does not read it: plain addresses
    lib.ucf_debug_fit_reduce.argtypes = ([C.c_int] * 4 + [C.c_double, C.c_longlong] + [vp] * 8 + [C.c_longlong, C.c_int] + [vp] * 7 + [vp] * 6)
    # x, rho, b, scale and every output may be NULL: plain addresses
    lib.ucf_fit_loss_terms.argtypes = [C.c_int, C.c_double, C.c_int, vp, vp, vp]
    lib.ucf_fit_robust_scale.argtypes = [C.c_int, vp, vp]
    lib.ucf_fit_set_loss.argtypes = [vp, C.c_int, C.c_double]
    lib.ucf_fit_get_loss.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    lib.ucf_fit_loss_report.argtypes = [vp, C.c_int] + [vp] * 7
    # kind, c, then the arguments of ucf_debug_fit_reduce, then ndown, b, bd
    lib.ucf_debug_fit_reduce_loss.argtypes = [C.c_int, C.c_double] + lib.ucf_debug_fit_reduce.argtypes + [vp] * 3
    # resampling: mult, set_of, rep and every output may be NULL: plain addresses
    lib.ucf_fit_set_resample.argtypes = [vp, C.c_int, vp]
    lib.ucf_fit_evaluate_resampled.argtypes = [vp, C.c_int, vp, C.c_double, C.c_int] + [vp] * 10
    lib.ucf_fit_objective_resampled.argtypes = [vp, C.c_int, vp, C.c_int] + [vp] * 8
    lib.ucf_fit_lm_resampled.argtypes = [vp, C.c_int, vp, vp, C.POINTER(UcfFitOptions)] + [vp] * 7
    lib.ucf_fit_resample_blocks.argtypes = [C.c_int, vp, C.c_int, C.c_ulonglong, vp, vp]
    lib.ucf_fit_resample_jackknife.argtypes = [C.c_int, vp, vp]
    lib.ucf_fit_resample_cov.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 5
    # kind, c, then the arguments of ucf_debug_fit_reduce up to `first`, then nrep, mult, nred, set_of, rep, sums, nbad, counts
    lib.ucf_debug_fit_reduce_resampled.argtypes = ([C.c_int, C.c_double] + lib.ucf_debug_fit_reduce.argtypes[:-6] +
                                                   [C.c_int, vp, C.c_int, vp, vp, vp, vp, vp])
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        lib = load()
        raise UcfError(rc, (lib.ucf_last_error() or b"").decode() or lib.ucf_status_string(rc).decode())
