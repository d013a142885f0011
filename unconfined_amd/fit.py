"""Parameter fitting over the C ABI (ucf_fit_* of include/ucf.h): the observations live on the GPU, base and perturbed
parameter sets run through the launch sequence of ``ucf_drawdown_multi``, and residuals, objective, Jacobian and normal
equations are formed on the device; this module only marshals arrays.

    fit = Fit(params, free=["Kr", "kappa", "Ss", "Sy"], t=t, r=r, z=z, iz=iz, obs=obs)
    out = fit.evaluate(theta, dlog=1e-3)          # phi, g, A, nbad (J, sim_all on request) for many parameter sets
    res = fit.lm(theta0, max_iter=40)             # Levenberg-Marquardt from many starting points at once
    net = Fit.network(params, free, wells=[(r0, [z0]), (r1, [za, zb, zc])], t=t, well=well, iz=iz, obs=obs)
                                                  # an observation network: per-well radius and depths, iz = -1: screen average
    fit.set_derivative(dobs)                      # fit the log-time derivative t ds/dt jointly; evaluate(..., derivative=True)
    fld = Fit.field(params, free, wells=[(0, 0, 1, 0), (40, 30, 0.6, 20)], obs_wells=[(10, 5, [z0]), (25, -8, [za, zb, zc])],
                    t=t, well=well, iz=iz, obs=obs)
                                                  # an interference test: pumping wells (x, y, q, t0) as WellField / images take them
    obj = fit.objective(thetas)                   # phi, nbad of many parameter sets without a Jacobian: one plan per set
    lw = likelihood_weights(obj["phi"], obj["nbad"])          # weights for WellField.ensemble(..., weights=lw["weight"])
    fit.set_loss("huber", 1.345)                  # a robust loss: evaluate, objective and lm reduce with it from here on
    rep = fit.loss_report(res["theta"], factors=True)         # b (and bd): the factor of every residual; b == 0: an outlier
    bs = fit.bootstrap(res["theta"][0], 1024, block=well)     # one-step block bootstrap: one evaluation, 1024 reductions;
                                                              # bs["thetas"] feed WellField.ensemble, bs["cov"] replaces cov
    jk = fit.lm_resampled(np.tile(th, (nwell, 1)), rep=np.arange(nwell))   # after set_resample(resample_jackknife(nobs, well))

Parameters are positive and fitted in their logarithm; ``theta`` arrays hold the parameters themselves.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Union

import numpy as np

from . import lib as _libmod
from .abi import FIT_CONVERGED, FIT_MAX_ITER, FIT_SCREEN, LOSS_KINDS, LOSS_L2, PAR_IDS, PAR_MOENCH_ALPHA0, RESAMPLE_KINDS, UcfFitOptions, UcfParams


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def par_id(name: Union[str, int]) -> int:
    """'Kr', 'kappa', 'Ss', 'Sy', 'ac', 'ak', 'usL', 'MoenchAlpha[i]' (or the id itself) -> UCF_PAR_*"""
    if isinstance(name, (int, np.integer)):
        return int(name)
    if name in PAR_IDS:
        return PAR_IDS[name]
    if name.startswith("MoenchAlpha[") and name.endswith("]"):
        return PAR_MOENCH_ALPHA0 + int(name[len("MoenchAlpha["):-1])
    raise ValueError(f"unknown parameter {name!r}")


def perturb(params: UcfParams, free: Sequence[Union[str, int]], theta) -> UcfParams:
    """the parameter set ``params`` with the free parameters set to ``theta`` (ucf_fit_perturb; no GPU)"""
    lib = _libmod.load()
    ids = _i32([par_id(n) for n in free])
    out = UcfParams()
    _libmod.check(lib.ucf_fit_perturb(C.byref(params), len(ids), ids, _f64(theta), C.byref(out)))
    return out


def solve_step(A, g, lam: float) -> np.ndarray:
    """(A + lam diag A) step = g (ucf_fit_solve_step; no GPU); raises UcfError (UCF_ERR_SINGULAR) if not positive definite"""
    lib = _libmod.load()
    A = _f64(A)
    g = _f64(g)
    step = np.zeros(len(g))
    _libmod.check(lib.ucf_fit_solve_step(len(g), A, g, float(lam), step))
    return step


def default_options() -> UcfFitOptions:
    opt = UcfFitOptions()
    _libmod.check(_libmod.load().ucf_fit_default_options(C.byref(opt)))
    return opt


def pack_wells(wells):
    """a sequence of (r, z_array) -> the arrays of ucf_fit_create_network: well_r [nwell], well_nz [nwell] and well_z, the
    depths of all wells one after the other"""
    wells = list(wells)
    well_r = _f64([float(r) for r, _ in wells])
    zs = [np.atleast_1d(_f64(z)).ravel() for _, z in wells]
    well_nz = _i32([len(z) for z in zs])
    well_z = _f64(np.concatenate(zs)) if zs else np.zeros(0)
    return well_r, well_nz, well_z


def network_eval_counts(wells, t, well) -> tuple:
    """(launched, dense) of the network fit over these observations (ucf_fit_network_eval_counts; no GPU)"""
    _, well_nz, _ = pack_wells(wells)
    t, well = _f64(t), _i32(well)
    a, b = C.c_longlong(), C.c_longlong()
    _libmod.check(_libmod.load().ucf_fit_network_eval_counts(len(well_nz), well_nz, len(t), t, well, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def _pump_wells(wells):
    w = np.atleast_2d(_f64(wells))
    if w.ndim != 2 or w.shape[1] != 4:
        raise ValueError("wells: one (x, y, q, t0) per pumping well")
    return tuple(_f64(w[:, k]) for k in range(4))


def pack_obs_wells(obs_wells):
    """a sequence of (x, y, z_array) -> the arrays of ucf_fit_create_field: well_x, well_y [nwell], well_nz [nwell] and
    well_z, the depths of all wells one after the other"""
    obs_wells = list(obs_wells)
    well_x = _f64([float(x) for x, _, _ in obs_wells])
    well_y = _f64([float(y) for _, y, _ in obs_wells])
    _, well_nz, well_z = pack_wells([(0.0, z) for _, _, z in obs_wells])
    return well_x, well_y, well_nz, well_z


def field_terms(params: UcfParams, wells, obs_wells, t, well) -> dict:
    """what a field fit launches and sums (ucf_fit_field_terms; no GPU): virt_well, virt_r per virtual well -- one per
    (observation well, distinct distance to a pumping well) -- term_first [nobs + 1], and per term term_pump, term_virt and
    term_t = t[i] - t0 of its pumping well.  ``obs_wells`` may hold (x, y) or (x, y, z_array)."""
    xw, yw, qw, t0w = _pump_wells(wells)
    well_x = _f64([float(o[0]) for o in obs_wells])
    well_y = _f64([float(o[1]) for o in obs_wells])
    t, well = _f64(t), _i32(well)
    if len(t) != len(well):
        raise ValueError("t and well must have one entry per observation")
    nvirt = C.c_int()
    npair, nmax = max(len(well_x) * len(xw), 1), max(len(t) * len(xw), 1)
    virt_well, virt_r = np.zeros(npair, np.int32), np.zeros(npair)
    first = np.zeros(len(t) + 1, np.int32)
    pump, virt, tt = np.zeros(nmax, np.int32), np.zeros(nmax, np.int32), np.zeros(nmax)
    _libmod.check(_libmod.load().ucf_fit_field_terms(C.byref(params), len(xw), xw, yw, qw, t0w, len(well_x), well_x, well_y, len(t), t,
                                                     well, C.byref(nvirt), virt_well, virt_r, first, pump, virt, tt))
    n = int(first[-1])
    return {"virt_well": virt_well[:nvirt.value].copy(), "virt_r": virt_r[:nvirt.value].copy(), "term_first": first,
            "term_pump": pump[:n].copy(), "term_virt": virt[:n].copy(), "term_t": tt[:n].copy()}


def derivative_check(dobs, dweight) -> int:
    """the checks of ``Fit.set_derivative`` (ucf_fit_derivative_check; no GPU): raises UcfError naming the offender -- a
    weight that is negative or not finite, a derivative that is not finite under a positive weight -- and returns nd, the
    number of positive weights.  ``None`` for an array is passed on as NULL."""
    dobs = None if dobs is None else _f64(dobs)
    dweight = None if dweight is None else _f64(dweight)
    if dobs is not None and dweight is not None and len(dobs) != len(dweight):
        raise ValueError("dobs and dweight must have one entry per observation")
    n = len(dobs) if dobs is not None else (len(dweight) if dweight is not None else 0)
    nd = C.c_int()
    _libmod.check(_libmod.load().ucf_fit_derivative_check(n, None if dobs is None else dobs.ctypes.data,
                                                          None if dweight is None else dweight.ctypes.data, C.byref(nd)))
    return int(nd.value)


def likelihood_weights(phi, nbad=None, s2: float = 1.0) -> dict:
    """likelihood weights of the members whose objectives are ``phi`` (ucf_ensemble_likelihood_weights; no GPU): weight
    [nens] = exp(-0.5 (phi - phi[best]) / s2), 0 for a member whose phi is not finite or whose ``nbad`` is not 0; best, the
    admissible member of least phi; nadmissible.  ``s2`` is the variance factor: 1 where the fit's weights are true 1 / sigma;
    otherwise e.g. phi[best] / (nobs + nd - npar), the factor of cov in ``Fit.lm``."""
    phi = np.atleast_1d(_f64(phi))
    nb = None if nbad is None else np.atleast_1d(_i32(nbad))
    if nb is not None and len(nb) != len(phi):
        raise ValueError("phi and nbad must have one entry per member")
    w = np.zeros(len(phi))
    best, nadm = C.c_int(-1), C.c_int(0)
    _libmod.check(_libmod.load().ucf_ensemble_likelihood_weights(len(phi), phi.ctypes.data, None if nb is None else nb.ctypes.data,
                                                                 float(s2), w.ctypes.data, C.addressof(best), C.addressof(nadm)))
    return {"weight": w, "best": int(best.value), "nadmissible": int(nadm.value)}


def loss_kind(kind: Union[str, int]) -> int:
    """'l2', 'huber', 'tukey' (or the number itself) -> UCF_LOSS_*"""
    if isinstance(kind, (int, np.integer)):
        return int(kind)
    if str(kind).lower() in LOSS_KINDS:
        return LOSS_KINDS[str(kind).lower()]
    raise ValueError(f"unknown loss {kind!r}")


def loss_terms(kind, c: float, x) -> tuple:
    """(rho, b) of the weighted residuals ``x`` under a loss (ucf_fit_loss_terms; no GPU): the arithmetic of the device
    reduction, operation for operation.  ``c`` is not read for 'l2'."""
    x = np.atleast_1d(_f64(x))
    rho, b = np.zeros(x.shape), np.zeros(x.shape)
    _libmod.check(_libmod.load().ucf_fit_loss_terms(loss_kind(kind), float(c), x.size, x.ctypes.data, rho.ctypes.data, b.ctypes.data))
    return rho, b


def robust_scale(x) -> float:
    """1.4826 x the median of |x| over the finite entries (ucf_fit_robust_scale; no GPU): sigma of weighted residuals that
    hold outliers.  A multiple of it is the usual ``c`` of ``Fit.set_loss``."""
    x = np.atleast_1d(_f64(x)).ravel()
    s = C.c_double()
    _libmod.check(_libmod.load().ucf_fit_robust_scale(len(x), x.ctypes.data if len(x) else None, C.addressof(s)))
    return float(s.value)


def _u16(a):
    return np.ascontiguousarray(a, dtype=np.uint16)


def _blocks(block, nobs):
    if block is None:
        return None, int(nobs)
    block = _i32(block)
    if nobs is not None and len(block) != nobs:
        raise ValueError("block must have one entry per observation")
    return block, len(block)


def resample_blocks(nobs: int, nrep: int, block=None, seed: int = 0) -> np.ndarray:
    """mult [nrep][nobs] (uint16) of a block bootstrap (ucf_fit_resample_blocks; no GPU): per replicate as many draws as there
    are blocks, every observation of a drawn block gains 1.  ``block`` [nobs] holds block ids 0..nb-1 (wells, time windows);
    None: every observation is its own block, the iid bootstrap."""
    block, nobs = _blocks(block, nobs)
    mult = np.zeros((max(int(nrep), 1), max(nobs, 1)), np.uint16)          # (the call refuses an nrep or nobs below 1)
    _libmod.check(_libmod.load().ucf_fit_resample_blocks(nobs, None if block is None else block.ctypes.data, int(nrep),
                                                         int(seed) & 0xFFFFFFFFFFFFFFFF, mult.ctypes.data, None))
    return mult


def resample_jackknife(nobs: int, block=None) -> np.ndarray:
    """mult [nb][nobs] (uint16) of the delete-one-block jackknife (ucf_fit_resample_jackknife; no GPU): row b is 0 on block b
    and 1 elsewhere.  Leave one well out with the well index as ``block``; k-fold cross-validation with fold ids."""
    block, nobs = _blocks(block, nobs)
    nb = C.c_int()
    lib = _libmod.load()
    _libmod.check(lib.ucf_fit_resample_blocks(nobs, None if block is None else block.ctypes.data, 1, 0, None, C.addressof(nb)))
    mult = np.zeros((nb.value, nobs), np.uint16)
    _libmod.check(lib.ucf_fit_resample_jackknife(nobs, None if block is None else block.ctypes.data, mult.ctypes.data))
    return mult


def resample_cov(kind, thetas, use=None) -> dict:
    """mean [npar] and cov [npar][npar] in ln(theta) over the replicates ``thetas`` [nrep][npar] with use[r] != 0
    (ucf_fit_resample_cov; no GPU); kind 'bootstrap' divides the sum of products by n - 1, 'jackknife' multiplies it by
    (n - 1) / n.  Also nused = n."""
    k = kind if isinstance(kind, (int, np.integer)) else RESAMPLE_KINDS[str(kind).lower()]
    thetas = np.atleast_2d(_f64(thetas))
    n, P = thetas.shape
    use = None if use is None else _i32(use)
    if use is not None and len(use) != n:
        raise ValueError("use must have one entry per replicate")
    out = {"mean": np.zeros(P), "cov": np.zeros((P, P))}
    nused = C.c_int()
    _libmod.check(_libmod.load().ucf_fit_resample_cov(int(k), n, P, thetas.ctypes.data, None if use is None else use.ctypes.data,
                                                      out["mean"].ctypes.data, out["cov"].ctypes.data, C.addressof(nused)))
    out["nused"] = int(nused.value)
    return out


def quantise_weights(w) -> tuple:
    """(u, ess): the integer weights u [nens] (uint64, 0 .. 2^32, the largest weight 2^32) that a weighted ensemble reduces
    with, and Kish's effective sample size of them (ucf_ensemble_quantise; no GPU).  A member with u = 0 is not in the ensemble."""
    w = np.atleast_1d(_f64(w))
    u = np.zeros(len(w), np.uint64)
    ess = C.c_double()
    _libmod.check(_libmod.load().ucf_ensemble_quantise(len(w), w.ctypes.data, u.ctypes.data, C.addressof(ess)))
    return u, float(ess.value)


class Fit:
    """observations (dimensional drawdown at time t[i], radius r[i], depth z[iz[i]], z up from the aquifer base) of one
    parameter set ``params`` whose ``free`` parameters are to be estimated.  All depths of ``z`` are evaluated at every
    point and ``iz`` selects one."""

    def __init__(self, params: UcfParams, free, t, r, z, iz, obs, weight=None, device: int = 0):
        self._lib = _libmod.load()
        self._h = C.c_void_p()
        self.params = params
        self.free = list(free)
        self.ids = _i32([par_id(n) for n in free])
        self.npar = len(self.ids)
        t, r, z, obs = _f64(t), _f64(r), _f64(z), _f64(obs)
        iz = _i32(iz)
        weight = np.ones(len(obs)) if weight is None else _f64(weight)
        if not (len(t) == len(r) == len(iz) == len(obs) == len(weight)):
            raise ValueError("t, r, iz, obs and weight must have one entry per observation")
        self.nobs = len(obs)
        _libmod.check(self._lib.ucf_fit_create(C.byref(params), self.npar, self.ids, self.nobs, t, r, iz, len(z), z, obs, weight,
                                               int(device), C.byref(self._h)))

    @classmethod
    def network(cls, params: UcfParams, free, wells, t, well, iz, obs, weight=None, device: int = 0) -> "Fit":
        """an observation network (ucf_fit_create_network): ``wells`` is a sequence of (r, z_array), observation i is the
        drawdown at time t[i] in well well[i], at depth iz[i] of that well or, with iz[i] = -1 (``abi.FIT_SCREEN``), the
        screen average over all depths of that well.  A point is evaluated at the depths of its own well only."""
        self = cls.__new__(cls)
        self._lib = _libmod.load()
        self._h = C.c_void_p()
        self.params = params
        self.free = list(free)
        self.ids = _i32([par_id(n) for n in free])
        self.npar = len(self.ids)
        well_r, well_nz, well_z = pack_wells(wells)
        t, obs = _f64(t), _f64(obs)
        well, iz = _i32(well), _i32(iz)
        weight = np.ones(len(obs)) if weight is None else _f64(weight)
        if not (len(t) == len(well) == len(iz) == len(obs) == len(weight)):
            raise ValueError("t, well, iz, obs and weight must have one entry per observation")
        self.nobs = len(obs)
        _libmod.check(self._lib.ucf_fit_create_network(C.byref(params), self.npar, self.ids, len(well_r), well_r, well_nz, well_z,
                                                       self.nobs, t, well, iz, obs, weight, int(device), C.byref(self._h)))
        return self

    @classmethod
    def field(cls, params: UcfParams, free, wells, obs_wells, t, well, iz, obs, weight=None, device: int = 0) -> "Fit":
        """an interference test (ucf_fit_create_field): ``wells`` are the pumping wells, rows of (x, y, q, t0) as ``WellField``
        and ``images`` use them (an image well is a plain row); ``obs_wells`` is a sequence of (x, y, z_array); observation
        i is the drawdown at time t[i] in observation well well[i], at depth iz[i] of that well or, with iz[i] = -1, its
        screen average.  Its simulated value is the sum over the pumping wells that started before t[i] of q times the
        drawdown at time t[i] - t0 and the distance between the two wells.  ``debug_h`` takes a term index here
        (``field_terms``)."""
        self = cls.__new__(cls)
        self._lib = _libmod.load()
        self._h = C.c_void_p()
        self.params = params
        self.free = list(free)
        self.ids = _i32([par_id(n) for n in free])
        self.npar = len(self.ids)
        xw, yw, qw, t0w = _pump_wells(wells)
        well_x, well_y, well_nz, well_z = pack_obs_wells(obs_wells)
        t, obs = _f64(t), _f64(obs)
        well, iz = _i32(well), _i32(iz)
        weight = np.ones(len(obs)) if weight is None else _f64(weight)
        if not (len(t) == len(well) == len(iz) == len(obs) == len(weight)):
            raise ValueError("t, well, iz, obs and weight must have one entry per observation")
        self.nobs = len(obs)
        _libmod.check(self._lib.ucf_fit_create_field(C.byref(params), self.npar, self.ids, len(xw), xw, yw, qw, t0w, len(well_x), well_x,
                                                     well_y, well_nz, well_z, self.nobs, t, well, iz, obs, weight, int(device),
                                                     C.byref(self._h)))
        return self

    def eval_counts(self) -> tuple:
        """(launched, dense): (point, depth) evaluations per parameter set that this fit launches, padding included, and
        that every depth of the network at every (well, time) would take"""
        a, b = C.c_longlong(), C.c_longlong()
        _libmod.check(self._lib.ucf_fit_eval_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def debug_h(self, plan: int, i: int) -> np.ndarray:
        """diagnostic (ucf_fit_debug_h): the dimensionless h behind observation i (of a field fit: behind TERM i) under plan
        ``plan`` of the last evaluate"""
        h = np.zeros(64)
        n = C.c_int()
        _libmod.check(self._lib.ucf_fit_debug_h(self._h, int(plan), int(i), len(h), h, C.byref(n)))
        return h[:n.value].copy()

    def debug_dh(self, plan: int, i: int) -> np.ndarray:
        """diagnostic (ucf_fit_debug_dh): the dimensionless dh = t dh/dt behind observation i (of a field fit: behind TERM
        i) under plan ``plan`` of the last evaluate"""
        dh = np.zeros(64)
        n = C.c_int()
        _libmod.check(self._lib.ucf_fit_debug_dh(self._h, int(plan), int(i), len(dh), dh, C.byref(n)))
        return dh[:n.value].copy()

    def set_derivative(self, dobs, dweight=None):
        """attach the observed log-time derivative t ds/dt (dimensional, one per observation) and its weights
        (ucf_fit_set_derivative; None: unit weights).  A weight of 0 marks an observation without a derivative datum; its
        dobs may be NaN.  From here on ``evaluate`` and ``lm`` return the joint objective of both curves."""
        dobs = _f64(dobs)
        dweight = np.ones(len(dobs)) if dweight is None else _f64(dweight)
        if not (len(dobs) == len(dweight) == self.nobs):
            raise ValueError("dobs and dweight must have one entry per observation")
        _libmod.check(self._lib.ucf_fit_set_derivative(self._h, dobs.ctypes.data, dweight.ctypes.data))
        self._deriv = True

    def clear_derivative(self):
        """detach the derivative data: ``evaluate`` and ``lm`` are those of the drawdown alone again"""
        _libmod.check(self._lib.ucf_fit_set_derivative(self._h, None, None))
        self._deriv = False

    def set_loss(self, kind, c: float = 0.0):
        """the loss of the fit (ucf_fit_set_loss): 'l2' (least squares, the default; detaches a loss), 'huber' or 'tukey' with
        the constant ``c`` in units of the weighted residual.  ``evaluate``, ``objective`` and ``lm`` reduce with it from here
        on; cov of ``lm`` is then that of the weighted least-squares problem of the final factors (no sandwich estimator)."""
        _libmod.check(self._lib.ucf_fit_set_loss(self._h, loss_kind(kind), float(c)))

    def clear_loss(self):
        """back to least squares"""
        _libmod.check(self._lib.ucf_fit_set_loss(self._h, LOSS_L2, 0.0))

    def get_loss(self) -> tuple:
        """(kind, c) as ucf_fit_get_loss returns them; c = 0.0 under least squares"""
        k, c = C.c_int(), C.c_double()
        _libmod.check(self._lib.ucf_fit_get_loss(self._h, C.byref(k), C.byref(c)))
        return int(k.value), float(c.value)

    def loss_report(self, thetas, factors: bool = False) -> dict:
        """thetas [nsets][npar] -> phi, phi_w, nbad, ndown [nsets] under the fit's loss (ucf_fit_loss_report: base plans only);
        with ``factors`` b [nsets][nobs], the factor of every drawdown residual (NaN where the observation does not count),
        and on a fit with derivative data bd, that of the derivative residual (NaN also where its weight is 0).  A factor
        of 0 under Tukey, or below 1 under Huber, flags an outlier."""
        thetas = np.atleast_2d(_f64(thetas))
        n, P = thetas.shape
        if P != self.npar:
            raise ValueError(f"thetas has {P} columns, the fit has {self.npar} free parameters")
        out = {"phi": np.zeros(n), "phi_w": np.zeros(n), "nbad": np.zeros(n, np.int32), "ndown": np.zeros(n, np.int32)}
        if factors:
            out["b"] = np.zeros((n, self.nobs))
            if getattr(self, "_deriv", False):
                out["bd"] = np.zeros((n, self.nobs))
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _libmod.check(self._lib.ucf_fit_loss_report(self._h, n, thetas.ctypes.data, ptr("phi"), ptr("phi_w"), ptr("nbad"), ptr("ndown"),
                                                    ptr("b"), ptr("bd")))
        return out

    def set_resample(self, mult):
        """attach the multiplicities mult [nrep][nobs] (uint16, caller's observation order) of bootstrap or jackknife
        replicates (ucf_fit_set_resample; ``resample_blocks``, ``resample_jackknife``); None detaches them.  Only the
        ``*_resampled`` entries read them; ``evaluate``, ``objective``, ``lm`` and ``loss_report`` are unchanged."""
        if mult is None:
            _libmod.check(self._lib.ucf_fit_set_resample(self._h, 0, None))
            self.nrep = 0
            return
        mult = np.atleast_2d(_u16(mult))
        if mult.shape[1] != self.nobs:
            raise ValueError(f"mult has {mult.shape[1]} columns, the fit has {self.nobs} observations")
        _libmod.check(self._lib.ucf_fit_set_resample(self._h, mult.shape[0], mult.ctypes.data))
        self.nrep = mult.shape[0]

    def _reductions(self, nsets, set_of, rep):
        set_of = None if set_of is None else np.atleast_1d(_i32(set_of))
        rep = None if rep is None else np.atleast_1d(_i32(rep))
        if set_of is not None and rep is not None and len(set_of) != len(rep):
            raise ValueError("set_of and rep must have one entry per reduction")
        nred = len(set_of) if set_of is not None else (len(rep) if rep is not None else nsets)
        return nred, set_of, rep

    def evaluate_resampled(self, theta, dlog: float, set_of=None, rep=None) -> dict:
        """theta [nsets][npar] evaluated once, then nred reductions in one launch (ucf_fit_evaluate_resampled): reduction r
        reads the plans of set set_of[r] (None: r) under replicate rep[r] of the attached multiplicities (-1, or None: every
        multiplicity 1).  Per reduction phi, g, A, nbad, phi_w, phi_out (the held-out sum of squares), counts [nred][4] =
        nuse, nuse_d, nheld, ndown, and on a fit with derivative data phi_d."""
        theta = np.atleast_2d(_f64(theta))
        n, P = theta.shape
        if P != self.npar:
            raise ValueError(f"theta has {P} columns, the fit has {self.npar} free parameters")
        nred, set_of, rep = self._reductions(n, set_of, rep)
        out = {"phi": np.zeros(nred), "g": np.zeros((nred, P)), "A": np.zeros((nred, P, P)), "nbad": np.zeros(nred, np.int32),
               "phi_w": np.zeros(nred), "phi_out": np.zeros(nred), "counts": np.zeros((nred, 4), np.int32)}
        if getattr(self, "_deriv", False):
            out["phi_d"] = np.zeros(nred)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _libmod.check(self._lib.ucf_fit_evaluate_resampled(self._h, n, theta.ctypes.data, float(dlog), nred,
                                                           None if set_of is None else set_of.ctypes.data,
                                                           None if rep is None else rep.ctypes.data, ptr("phi"), ptr("g"), ptr("A"),
                                                           ptr("nbad"), ptr("phi_d"), ptr("phi_w"), ptr("phi_out"), ptr("counts")))
        return out

    def objective_resampled(self, thetas, set_of=None, rep=None) -> dict:
        """``evaluate_resampled`` on the base plans only (ucf_fit_objective_resampled): phi, nbad, phi_w, phi_out, counts (and
        phi_d) per reduction, no g or A.  phi_out of jackknife replicates at one theta is the cross-validation score."""
        thetas = np.atleast_2d(_f64(thetas))
        n, P = thetas.shape
        if P != self.npar:
            raise ValueError(f"thetas has {P} columns, the fit has {self.npar} free parameters")
        nred, set_of, rep = self._reductions(n, set_of, rep)
        out = {"phi": np.zeros(nred), "nbad": np.zeros(nred, np.int32), "phi_w": np.zeros(nred), "phi_out": np.zeros(nred),
               "counts": np.zeros((nred, 4), np.int32)}
        if getattr(self, "_deriv", False):
            out["phi_d"] = np.zeros(nred)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _libmod.check(self._lib.ucf_fit_objective_resampled(self._h, n, thetas.ctypes.data, nred,
                                                            None if set_of is None else set_of.ctypes.data,
                                                            None if rep is None else rep.ctypes.data, ptr("phi"), ptr("nbad"),
                                                            ptr("phi_d"), ptr("phi_w"), ptr("phi_out"), ptr("counts")))
        return out

    def lm_resampled(self, theta0, rep=None, cov: bool = True, **opt) -> dict:
        """``lm`` with start s reduced under replicate rep[s] of the attached multiplicities (ucf_fit_lm_resampled; None: all
        -1, the bytes of ``lm``).  Adds phi_out [nstarts] and counts [nstarts][4] at the final point; cov of a start is
        phi_w / (nuse + nuse_d - npar) A^-1 of its own replicate."""
        theta0 = np.atleast_2d(_f64(theta0))
        n, P = theta0.shape
        if P != self.npar:
            raise ValueError(f"theta0 has {P} columns, the fit has {self.npar} free parameters")
        rep = None if rep is None else np.atleast_1d(_i32(rep))
        if rep is not None and len(rep) != n:
            raise ValueError("rep must have one entry per start")
        o = default_options()
        for k, v in opt.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k!r}")
            setattr(o, k, v)
        out = {"theta": np.zeros((n, P)), "phi": np.zeros(n), "iters": np.zeros(n, np.int32), "status": np.zeros(n, np.int32),
               "phi_out": np.zeros(n), "counts": np.zeros((n, 4), np.int32)}
        if cov:
            out["cov"] = np.zeros((n, P, P))
        _libmod.check(self._lib.ucf_fit_lm_resampled(self._h, n, theta0.ctypes.data, None if rep is None else rep.ctypes.data, C.byref(o),
                                                     out["theta"].ctypes.data, out["phi"].ctypes.data, out["iters"].ctypes.data,
                                                     out["status"].ctypes.data, out["cov"].ctypes.data if cov else None,
                                                     out["phi_out"].ctypes.data, out["counts"].ctypes.data))
        return out

    def bootstrap(self, theta_hat, nrep: int, block=None, seed: int = 0, refit: bool = False, dlog: float = 1.0e-3, **opt) -> dict:
        """``nrep`` block-bootstrap replicates of the fit around theta_hat [npar] (``resample_blocks`` with ``block`` and
        ``seed``; the multiplicities stay attached).  refit=False: the one-step (linearised) bootstrap -- ONE evaluation at
        theta_hat, every replicate a reduction of it, then step_r = solve_step(A_r, g_r, 0) and theta_r = theta_hat exp(step_r);
        refit=True: ``lm_resampled`` from theta_hat (options as ``lm``).  Returns thetas [nrep][npar], ready for
        ``WellField.ensemble`` or ``sustainable_yield``; used [nrep] (bool: the step could be solved and no counted
        observation was non-finite, or the refit did not end in a non-finite start or a singular matrix); mean, cov, nused of
        ``resample_cov('bootstrap', thetas, used)``; mult."""
        theta_hat = _f64(theta_hat).ravel()
        if len(theta_hat) != self.npar:
            raise ValueError(f"theta_hat has {len(theta_hat)} entries, the fit has {self.npar} free parameters")
        mult = resample_blocks(self.nobs, nrep, block=block, seed=seed)
        self.set_resample(mult)
        rep = np.arange(nrep, dtype=np.int32)
        thetas = np.tile(theta_hat, (nrep, 1))
        if refit:
            res = self.lm_resampled(thetas, rep=rep, cov=False, dlog=dlog, **opt)
            thetas = res["theta"]
            used = (res["status"] == FIT_CONVERGED) | (res["status"] == FIT_MAX_ITER)
        else:
            ev = self.evaluate_resampled(theta_hat, dlog, set_of=np.zeros(nrep, np.int32), rep=rep)
            used = ev["nbad"] == 0
            for r in np.flatnonzero(used):
                try:
                    thetas[r] = theta_hat * np.exp(solve_step(ev["A"][r], ev["g"][r], 0.0))
                except _libmod.UcfError:
                    used[r] = False
        used &= np.isfinite(thetas).all(axis=1) & (thetas > 0.0).all(axis=1)
        out = {"thetas": thetas, "used": used, "mult": mult}
        out.update(resample_cov("bootstrap", np.where(used[:, None], thetas, 1.0), used.astype(np.int32)))
        return out

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ucf_fit_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc_count(self) -> int:
        """device allocations made so far by the fit and its plans"""
        return int(self._lib.ucf_fit_alloc_count(self._h))

    def evaluate(self, theta, dlog: float, jacobian: bool = False, sim_all: bool = False, derivative: bool = False) -> dict:
        """theta [nsets][npar] -> phi [nsets], g [nsets][npar], A [nsets][npar][npar], nbad [nsets]; on request J
        [nsets][nobs][npar] and sim_all [nsets][1 + 2 npar][nobs] (row 0 base, 1 + 2j parameter j up, 2 + 2j down).
        ``derivative=True`` (ucf_fit_evaluate_joint; the fit must have derivative data) adds phi_d [nsets], the derivative
        terms' share of phi, and Jd / simd_all, shaped as J / sim_all, under the same two flags."""
        theta = np.atleast_2d(_f64(theta))
        n, P = theta.shape
        if P != self.npar:
            raise ValueError(f"theta has {P} columns, the fit has {self.npar} free parameters")
        out = {"phi": np.zeros(n), "g": np.zeros((n, P)), "A": np.zeros((n, P, P)), "nbad": np.zeros(n, np.int32)}
        if jacobian:
            out["J"] = np.zeros((n, self.nobs, P))
        if sim_all:
            out["sim_all"] = np.zeros((n, 1 + 2 * P, self.nobs))
        ptr = lambda k: out[k].ctypes.data if k in out else None
        if derivative:
            out["phi_d"] = np.zeros(n)
            if jacobian:
                out["Jd"] = np.zeros((n, self.nobs, P))
            if sim_all:
                out["simd_all"] = np.zeros((n, 1 + 2 * P, self.nobs))
            _libmod.check(self._lib.ucf_fit_evaluate_joint(self._h, n, np.ascontiguousarray(theta), float(dlog), ptr("phi"), ptr("g"),
                                                           ptr("A"), ptr("nbad"), ptr("J"), ptr("sim_all"), ptr("phi_d"), ptr("Jd"),
                                                           ptr("simd_all")))
            return out
        _libmod.check(self._lib.ucf_fit_evaluate(self._h, n, np.ascontiguousarray(theta), float(dlog), ptr("phi"), ptr("g"), ptr("A"),
                                                 ptr("nbad"), ptr("J"), ptr("sim_all")))
        return out

    def objective(self, thetas, sim: bool = False) -> dict:
        """thetas [nsets][npar] -> phi [nsets], nbad [nsets] without a Jacobian (ucf_fit_objective): one plan per set, what ``lm``
        runs at its trial points; with ``sim`` the simulated values sim [nsets][nobs].  On a fit with derivative data phi is
        the joint objective, phi_d [nsets] the derivative terms' share of it, and ``sim`` adds simd."""
        thetas = np.atleast_2d(_f64(thetas))
        n, P = thetas.shape
        if P != self.npar:
            raise ValueError(f"thetas has {P} columns, the fit has {self.npar} free parameters")
        out = {"phi": np.zeros(n), "nbad": np.zeros(n, np.int32)}
        if sim:
            out["sim"] = np.zeros((n, self.nobs))
        if getattr(self, "_deriv", False):
            out["phi_d"] = np.zeros(n)
            if sim:
                out["simd"] = np.zeros((n, self.nobs))
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _libmod.check(self._lib.ucf_fit_objective(self._h, n, thetas.ctypes.data, ptr("phi"), ptr("nbad"), ptr("sim"), ptr("phi_d"),
                                                  ptr("simd")))
        return out

    def lm(self, theta0, cov: bool = True, loss=None, **opt) -> dict:
        """Levenberg-Marquardt from the starting points theta0 [nstarts][npar], all in one call; options as the fields of
        ucf_fit_options (max_iter, dlog, lambda0, lambda_up, lambda_down, tol_step, tol_phi).  Returns theta, phi, iters,
        status (abi.FIT_*) per start and, unless cov=False, the covariance in ln(theta).  ``loss`` = (kind, c) applies for
        this call only: the fit's own loss is put back afterwards, also when the call raises."""
        if loss is not None:
            kind, c = (loss, 0.0) if isinstance(loss, (str, int, np.integer)) else loss
            before = self.get_loss()
            self.set_loss(kind, c)
            try:
                return self.lm(theta0, cov=cov, **opt)
            finally:
                self.set_loss(*before)
        theta0 = np.atleast_2d(_f64(theta0))
        n, P = theta0.shape
        if P != self.npar:
            raise ValueError(f"theta0 has {P} columns, the fit has {self.npar} free parameters")
        o = default_options()
        for k, v in opt.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k!r}")
            setattr(o, k, v)
        out = {"theta": np.zeros((n, P)), "phi": np.zeros(n), "iters": np.zeros(n, np.int32), "status": np.zeros(n, np.int32)}
        if cov:
            out["cov"] = np.zeros((n, P, P))
        _libmod.check(self._lib.ucf_fit_lm(self._h, n, np.ascontiguousarray(theta0), C.byref(o), out["theta"], out["phi"], out["iters"],
                                           out["status"], out["cov"].ctypes.data if cov else None))
        return out
