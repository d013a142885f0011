"""Well fields over the C ABI (ucf_field_* of include/ucf.h): the drawdown of several pumping wells -- wells that start at
different times, image wells for a river or an outcrop -- as the sum over wells of q_j h(t - t0_j, |x - x_j|, z).  Per group
of wells that share a start time the library runs ONE product grid (times after the start x distinct distances) through
``ucf_drawdown_grid_device``, keeps h and dh on the GPU and forms the sums there; this module only marshals arrays.

    wells = images([(0.0, 0.0, 1.0, 0.0)], line=(1.0, 0.0, 40.0), kind="constant_head")      # (x, y, q, t0) per well
    field = WellField(wells, locations=[(10.0, 0.0), (40.0, 5.0)], times=[1.0, 10.0, 100.0])
    s, ds = field.drawdown(plan, z=[145.7, 100.0])                                            # [nt, nloc, nz] each

All wells share the plan's aquifer, well geometry and time behaviour; q multiplies the plan's Q (negative: injection).

A forecast takes what a fit returns as it is -- ``theta`` and ``cov`` of ``Fit.lm`` -- and maps, besides s and ds of the fitted
parameters, their sensitivities to ln theta_j and their first-order standard error sqrt(j' cov j) (ucf_field_forecast):

    out = field.forecast(plan, ["Kr", "Ss"], res["theta"][0], z=[145.7, 100.0], cov=res["cov"][0])
    out["s"], out["se"], out["sens"]                                                          # [nt, nloc, nz], same, [npar, nt, nloc, nz]

An ensemble asks what the linearisation cannot answer -- the 5 % / 50 % / 95 % maps, the chance that a limit is exceeded -- from
many parameter sets, drawn from the fit's covariance or taken from the rows of a multi-start fit (ucf_field_ensemble):

    thetas = ensemble_draw(res["theta"][0], res["cov"][0], 256, seed=1)                       # [256, npar]
    out = field.ensemble(plan, ["Kr", "Ss"], thetas, z=[145.7, 100.0], limits=[0.5])
    out["quant"], out["pexc"]                                                                 # [3, nt, nloc, nz], [1, nt, nloc, nz]

Members that are a design and not a sample -- a Latin hypercube, the rows of a multi-start fit -- count by their likelihood
(ucf_field_ensemble_weighted); a member whose weight rounds to 0 is not evaluated:

    lw = likelihood_weights(fit.objective(thetas)["phi"])
    out = field.ensemble(plan, ["Kr", "Ss"], thetas, z=[145.7, 100.0], limits=[0.5], weights=lw["weight"])
    out["quant"], out["ess"], out["nlaunched"]                                                # weighted inverse CDF, effective sample size

Where the next observation wells have to go so that a forecast becomes sure -- every (location, depth) of the map is a candidate,
the maps stay on the GPU and the picks cost one small launch each (ucf_field_worth):

    out = field.worth(plan, ["Kr", "Ss"], res["theta"][0], res["cov"][0], z=[145.7, 100.0], targets=[("s", 2, 1, 0)], sigma=0.01, picks=3)
    out["pick"], out["reduction"], out["cov_post"]                                            # [(i, z)] * 3, [3, ntgt, nloc, nz], [npar, npar]

How much the wells may pump before a permitted drawdown is exceeded somewhere, and how sure that is -- drawdown is linear in the
rates, so one ensemble's worth of evaluations answers every rate pattern (ucf_field_yield); here the real well and its image are
one control and 64 splits between two such pairs are tried, up to three times today's rates:

    patterns = [(a, 1.0 - a) for a in np.linspace(0.0, 1.0, 64)]
    out = field.sustainable_yield(plan, ["Kr", "Ss"], thetas, z=[145.7, 100.0], controls=[0, 1, 0, 1], patterns=patterns,
                                  limit=2.0, smax=3.0, levels=[1.0])
    out["quant"][0], out["pexc"], out["bind"]                                                 # the scale that 95 % admit, P(scale > 1), where it binds

How the pumping should be split between the controls so that the total is largest and every limit holds, what limits it and how
sure that is -- one linear programme per member, solved on the GPU on the same response slots (ucf_field_allocate):

    res = field.optimal_rates(plan, ["Kr", "Ss"], thetas, z=[145.7, 100.0], controls=[0, 1, 0, 1], objectives=[[1.0, 1.0]],
                              xmax=[3.0, 3.0], limit=2.0)
    res.x[:, 0], res.binding(0, 0), res.lam[0, 0], res.best_x[0, 0]                           # per member; what binds; shadow prices; the rates 95 % admit

When the drawdown first passes a permitted value, from when on it stays below one after the pumps have stopped, and how sure that
is -- one time per member, limit, location and depth, formed and reduced on the GPU (ucf_field_ensemble_times):

    res = field.time_to_limit(plan, ["Kr", "Ss"], thetas, z=[145.7, 100.0], limits=[0.5, 0.1], kinds=["first_above", "last_above"],
                              horizons=[365.0], abscissa="lnt")
    res.quant[1], 1.0 - res.later[0]                                                          # the median time, P(crossed within a year)

Which parameter causes the spread of the forecast where the posterior is too wide to linearise -- first-order and total Sobol
indices per output with their standard errors, from a Saltelli design of (npar + 2) n members that stay on the GPU (ucf_field_sobol):

    design = sobol_design(res["theta"][0], res["cov"][0], 64, seed=1)                         # [(npar + 2) 64, npar]
    sob = field.sobol(plan, ["Kr", "Ss"], design, z=[145.7, 100.0])
    sob.S, sob.ST - sob.S, sob.se_S                                                           # alone, through interactions, how sure
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _libmod
from .abi import TIME_KINDS, UcfEnsembleMaps, UcfParams, UcfSobolMaps, UcfStats
from .fit import par_id

KINDS = {"no_flow": 0, "constant_head": 1, 0: 0, 1: 1}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _addr(a):
    return a.ctypes.data if a is not None else None


def forecast_sets(params: UcfParams, free, theta, dlog: float) -> list:
    """the 1 + 2 npar parameter sets that a forecast evaluates (ucf_field_forecast_sets; no GPU): the base set, then per free
    parameter the set with it moved by +dlog and by -dlog in its logarithm"""
    ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
    theta = np.atleast_1d(_f64(theta))
    if len(theta) != len(ids):
        raise ValueError("theta: one value per free parameter")
    sets = (UcfParams * (1 + 2 * len(ids)))()
    _libmod.check(_libmod.load().ucf_field_forecast_sets(C.byref(params), len(ids), _addr(ids), _addr(theta), float(dlog), sets))
    return [UcfParams.from_buffer_copy(p) for p in sets]


def ensemble_draw(theta, cov, n: int, seed: int = 0):
    """n parameter sets [n, npar] drawn from the log-normal distribution that a fit states with ``theta`` and ``cov`` (in
    ln theta, as ``Fit.lm`` returns it): theta_j exp((L zeta)_j), L the Cholesky factor of cov, zeta standard normal deviates
    from the generator that include/ucf.h states; the same seed gives the same bits (ucf_field_ensemble_draw; no GPU)"""
    theta = np.atleast_1d(_f64(theta))
    cov = np.atleast_2d(_f64(cov))
    if cov.shape != (len(theta), len(theta)):
        raise ValueError("cov: [npar, npar]")
    out = np.zeros((max(int(n), 0), len(theta)))
    _libmod.check(_libmod.load().ucf_field_ensemble_draw(len(theta), _addr(theta), _addr(cov), int(n), int(seed) & (2 ** 64 - 1), _addr(out)))
    return out


def sobol_design(theta, cov, n: int, seed: int = 0):
    """the Saltelli design [(npar + 2) n, npar] of ``n`` base rows for ``WellField.sobol``: 2 n parameter sets are drawn as
    ``ensemble_draw(theta, diag(diag(cov)), 2 n, seed)`` does, the first n are A, the next n are B, and block 2 + j is A with
    column j taken from B (ucf_sobol_design; no GPU).  ONLY THE DIAGONAL of ``cov`` is used: the variance decomposition behind S
    and ST presupposes independent parameters, and with correlated draws the indices, though still computed, would not mean
    the shares of the variance that they are read as."""
    theta = np.atleast_1d(_f64(theta))
    cov = np.atleast_2d(_f64(cov))
    if cov.shape != (len(theta), len(theta)):
        raise ValueError("cov: [npar, npar]")
    n = int(n)
    draws = ensemble_draw(theta, np.diag(np.diag(cov)), 2 * n, seed)
    out = np.zeros(((len(theta) + 2) * max(n, 0), len(theta)))
    _libmod.check(_libmod.load().ucf_sobol_design(len(theta), n, _addr(draws), _addr(out)))
    return out


def worth_condition(F, J, w):
    """the factor of the covariance after the readings (J [nrow, npar] their sensitivities in ln theta, w [nrow] = 1 / sigma):
    F_out and cov_out = F_out F_out' = (C^-1 + sum w^2 j j')^-1 with C = F F' (ucf_worth_condition; no GPU).  F is any square
    factor of C; no rows returns F itself."""
    F = np.atleast_2d(_f64(F))
    n = len(F)
    if F.shape != (n, n):
        raise ValueError("F: [npar, npar]")
    J = _f64(J).reshape(-1, n) if np.size(J) else np.zeros((0, n))
    w = np.atleast_1d(_f64(w)) if np.size(w) else np.zeros(0)
    if len(w) != len(J):
        raise ValueError("w: one weight per row of J")
    F_out, cov_out = np.zeros((n, n)), np.zeros((n, n))
    _libmod.check(_libmod.load().ucf_worth_condition(n, _addr(F), len(J), _addr(J) if len(J) else None, _addr(w) if len(J) else None,
                                                     _addr(F_out), _addr(cov_out)))
    return F_out, cov_out


def _wells(wells):
    w = np.atleast_2d(_f64(wells))
    if w.ndim != 2 or w.shape[1] != 4:
        raise ValueError("wells: one (x, y, q, t0) per well")
    return w


def images(wells, line, kind):
    """the wells (x, y, q, t0) followed by their mirror images in the line a x + b y = c (``line`` = (a, b, c)); an image has
    q = +q for ``kind`` 'no_flow' and -q for 'constant_head' and the t0 of its real well (ucf_field_images; no GPU).
    Returns an array [2 nwell, 4]."""
    w = _wells(wells)
    n = len(w)
    a, b, c = (float(v) for v in line)
    out = [np.zeros(2 * n) for _ in range(4)]
    _libmod.check(_libmod.load().ucf_field_images(n, _f64(w[:, 0]), _f64(w[:, 1]), _f64(w[:, 2]), _f64(w[:, 3]), a, b, c, KINDS[kind],
                                                  *out))
    return np.stack(out, axis=1)


class TimeToLimit:
    """what ``WellField.time_to_limit`` returns.  limits [nlim], kinds [nlim] (int32, UCF_TIME_*), abscissa ('t' or 'lnt'), never,
    q [nq], horizons [nhor]; mean, sd, min, max, nfin [nlim, nloc, nz]; quant [nq, nlim, nloc, nz]; later [nhor, nlim, nloc, nz], the
    share of members whose time lies beyond a horizon (the chance of crossing by then is 1 - later); all [nens, nlim, nloc, nz]
    where asked for; nbad, the outputs where a member that counts has no time (a drawdown that is not finite); with weights u,
    ess, nlaunched.  An array that was not asked for is None.  Everything is a time EXCEPT, where ``log_moments`` is true (abscissa
    'lnt'), mean and sd: those are the mean and the standard deviation of ln(time).  A member that does not cross within the
    field's times takes part with ``never``."""

    def __init__(self, **kw):
        self.quant = self.later = self.all = self.u = self.ess = self.nlaunched = self.stats = None
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"TimeToLimit(limits={self.limits.tolist()}, kinds={self.kinds.tolist()}, abscissa={self.abscissa!r}, never={self.never!r}, "
                f"shape={self.mean.shape}, nbad={self.nbad})")


class Allocation:
    """what ``WellField.optimal_rates`` returns.  Per member and objective, [nens, nobj] leading: x [.., nctl], the multipliers on
    the wells' q that maximise the objective, and g, its value; status (int32: 0 optimal, 1 iteration cap, 2 the fixed wells alone
    exceed a limit, 3 numeric, -1 the member is not finite -- x, g and lam are NaN unless it is 0) and iters; work [.., nctl]
    (int32), the constraints that bind at the optimum, ascending -- id c: x_c = 0, id nctl + c: x_c = xmax[c], id 2 nctl + i: the
    constrained output con[i] --, and lam [.., nctl], their shadow prices: the gain in g per unit of relaxed limit.  ``binding``
    translates work into ('lower', c), ('upper', c) or ('output', flat index into the map).  resp [nens, nctl + 1, ncon] and con
    [ncon] as in ``sustainable_yield``; nbad; q [nq]; gquant [nq, nobj], the quantiles of g over the members (the wait-and-see
    figure).  With ``reliability``: quant [nq, nens nobj], the scale of candidate p = m nobj + o that a share 1 - q of the
    members admits, value = quant g, best [nq, nobj] (int32; -1: none) the candidate of every objective with the largest value and
    best_x [nq, nobj, nctl] its scaled rates: a FEASIBLE allocation at reliability 1 - q chosen among the members' optima, a lower
    bound on the chance-constrained optimum.  With weights u, ess, nlaunched.  An array that was not asked for is None."""

    def __init__(self, **kw):
        self.quant = self.value = self.best = self.best_x = self.gquant = self.u = self.ess = self.nlaunched = self.stats = None
        self.__dict__.update(kw)

    def binding(self, m: int, o: int) -> list:
        nctl = self.x.shape[2]
        out = []
        for j in self.work[m, o]:
            j = int(j)
            out.append(None if j < 0 else ("lower", j) if j < nctl else ("upper", j - nctl) if j < 2 * nctl else ("output", int(self.con[j - 2 * nctl])))
        return out

    def __repr__(self):
        return f"Allocation(nens={self.x.shape[0]}, nobj={self.x.shape[1]}, nctl={self.x.shape[2]}, optimal={int((self.status == 0).sum())}, nbad={self.nbad})"


class SobolMaps:
    """what ``WellField.sobol`` returns.  S, ST, se_S, se_ST [npar, nt, nloc, nz]: the first-order and the total Sobol index of
    every free parameter for the drawdown and their standard errors; mean, var [nt, nloc, nz], the pooled mean and variance of
    the two base samples; nrow (int32) the base rows that are complete at an output -- the others take part in nothing; with the
    derivative dS, dST, dse_S, dse_ST, dmean, dvar, dnrow of t ds/dt; with the members all (and dall) [(npar + 2) n, nt, nloc, nz];
    nbad [2], the outputs of s and of ds where a base row is not complete; nbase; stats where asked for.  An array that was not
    asked for is None.  An index is NaN where the variance is not positive."""

    def __init__(self, **kw):
        self.dS = self.dST = self.dse_S = self.dse_ST = self.dmean = self.dvar = self.dnrow = self.all = self.dall = self.stats = None
        self.__dict__.update(kw)

    def __repr__(self):
        return f"SobolMaps(npar={self.S.shape[0]}, nbase={self.nbase}, shape={self.mean.shape}, nbad={self.nbad.tolist()})"


class WellField:
    """wells (x, y, q, t0), locations (x, y) and strictly increasing times, all dimensional"""

    def __init__(self, wells, locations, times):
        self._lib = _libmod.load()
        self._h = C.c_void_p()
        w = _wells(wells)
        loc = np.atleast_2d(_f64(locations))
        if loc.ndim != 2 or loc.shape[1] != 2:
            raise ValueError("locations: one (x, y) per location")
        t = np.atleast_1d(_f64(times))
        self.nwell, self.nloc, self.nt = len(w), len(loc), len(t)
        self._times = t.copy()
        _libmod.check(self._lib.ucf_field_create(self.nwell, _f64(w[:, 0]), _f64(w[:, 1]), _f64(w[:, 2]), _f64(w[:, 3]), self.nloc,
                                                 _f64(loc[:, 0]), _f64(loc[:, 1]), self.nt, t, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ucf_field_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def group_count(self) -> int:
        n = C.c_int()
        _libmod.check(self._lib.ucf_field_group_count(self._h, C.byref(n)))
        return n.value

    def groups(self, plan) -> list:
        """what every group launches under ``plan`` (ucf_field_group; host arithmetic, no launch): a list of dicts with k0, tD,
        sv, rD, col [nloc, nwell] (-1: the well is not in the group) and tfac.  ``plan`` may also be a parameter set
        (``UcfParams``): the same arrays without a plan or a GPU (ucf_field_group_from_params)."""
        out = []
        for g in range(self.group_count()):
            k0, nt_g, nr_g = C.c_int(), C.c_int(), C.c_int()
            tD, tfac, sv = np.zeros(self.nt), np.zeros(self.nt), np.zeros(self.nt, np.int32)
            rD, col = np.zeros(self.nloc * self.nwell), np.zeros((self.nloc, self.nwell), np.int32)
            args = (g, C.byref(k0), C.byref(nt_g), tD, sv, C.byref(nr_g), rD, col, tfac)
            if isinstance(plan, UcfParams):
                _libmod.check(self._lib.ucf_field_group_from_params(self._h, C.byref(plan), *args))
            else:
                _libmod.check(self._lib.ucf_field_group(self._h, plan._h, *args))
            n = nt_g.value
            out.append({"k0": k0.value, "tD": tD[:n].copy(), "sv": sv[:n].copy(), "rD": rD[:nr_g.value].copy(), "col": col,
                        "tfac": tfac[:n].copy()})
        return out

    def drawdown(self, plan, z, dimensionless: bool = False, with_stats: bool = False):
        """s, ds of shape [nt, nloc, nz]: superposed drawdown and its logarithmic time derivative t ds/dt at the depths z (up
        from the aquifer base), dimensional unless ``dimensionless``; in the plan's current flavour"""
        z = np.atleast_1d(_f64(z))
        s = np.zeros((self.nt, self.nloc, len(z)))
        ds = np.zeros_like(s)
        st = UcfStats()
        _libmod.check(self._lib.ucf_field_drawdown(self._h, plan._h, len(z), z, 1 if dimensionless else 0, s, ds,
                                                   C.byref(st) if with_stats else None))
        if with_stats:
            return s, ds, {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return s, ds

    def forecast(self, plan, free, theta, z, cov=None, dlog: float = 1e-3, sensitivities: bool = True, all_maps: bool = False,
                 with_stats: bool = False) -> dict:
        """the field under ``plan``'s parameter set with the free parameters (names as for ``fit.par_id``) at ``theta``, all
        dimensional: s, ds [nt, nloc, nz]; with ``sensitivities`` sens, dsens [npar, nt, nloc, nz], the central differences
        of s and ds in ln theta_j with step ``dlog``; with ``cov`` [npar, npar] (in ln theta, as ``Fit.lm`` returns it) se, dse
        [nt, nloc, nz], the first-order standard errors; with ``all_maps`` s_all, ds_all [1 + 2 npar, nt, nloc, nz], the maps
        of every parameter set of ``forecast_sets``; nbad [2], the outputs of s and of ds with a value that is not finite
        under any of the sets.  ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        theta = np.atleast_1d(_f64(theta))
        if len(theta) != len(ids):
            raise ValueError("theta: one value per free parameter")
        npar = len(ids)
        z = np.atleast_1d(_f64(z))
        if cov is not None:
            cov = _f64(cov)
            if cov.shape != (npar, npar):
                raise ValueError("cov: [npar, npar]")
        shape = (self.nt, self.nloc, len(z))
        out = {"s": np.zeros(shape), "ds": np.zeros(shape)}
        if sensitivities:
            out["sens"], out["dsens"] = np.zeros((npar,) + shape), np.zeros((npar,) + shape)
        if cov is not None:
            out["se"], out["dse"] = np.zeros(shape), np.zeros(shape)
        if all_maps:
            out["s_all"], out["ds_all"] = np.zeros((1 + 2 * npar,) + shape), np.zeros((1 + 2 * npar,) + shape)
        out["nbad"] = np.zeros(2, np.int64)
        st = UcfStats()
        _libmod.check(self._lib.ucf_field_forecast(
            self._h, plan._h, npar, _addr(ids), _addr(theta), float(dlog), _addr(cov), len(z), _addr(z),
            *(_addr(out.get(k)) for k in ("s", "ds", "sens", "dsens", "se", "dse", "s_all", "ds_all")), _addr(out["nbad"]),
            C.byref(st) if with_stats else None))
        if with_stats:
            out["stats"] = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return out

    def ensemble(self, plan, free, thetas, z, quantiles=(0.05, 0.5, 0.95), limits=None, derivative: bool = True,
                 all_maps: bool = False, with_stats: bool = False, weights=None) -> dict:
        """the field under the parameter sets ``thetas`` [nens, npar] of the free parameters (names as for ``fit.par_id``; the
        other parameters are ``plan``'s), reduced over the members on the GPU, all dimensional: mean, sd, min, max [nt, nloc,
        nz] of the drawdown, quant [nq, nt, nloc, nz] at the levels ``quantiles``, nfin (int32) the members that are finite at
        an output -- the others take part in no statistic; with ``limits`` pexc [nlim, nt, nloc, nz], the fraction of the
        finite members whose drawdown exceeds a limit; with ``derivative`` dmean, dsd, dmin, dmax, dquant, dnfin of t ds/dt;
        with ``all_maps`` s_all (and ds_all) [nens, nt, nloc, nz], the member maps; nbad [2], the outputs of s and of ds where
        a member is not finite.  ``plan`` is not modified.
        With ``weights`` [nens] (e.g. ``fit.likelihood_weights``) the members count by their weight (ucf_field_ensemble_weighted):
        mean, sd and pexc are the weighted ones, quant is the inverse of the weighted distribution function (no interpolation), a
        member whose integer weight is 0 is not evaluated and is not in the ensemble (its row of s_all is NaN), and the result
        gains u [nens] (uint64, the integer weights), ess (the effective sample size) and nlaunched."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        thetas = np.atleast_2d(_f64(thetas))
        if thetas.ndim != 2 or thetas.shape[1] != len(ids):
            raise ValueError("thetas: [nens, npar], one value per free parameter")
        nens = len(thetas)
        z = np.atleast_1d(_f64(z))
        q = np.atleast_1d(_f64(quantiles if quantiles is not None else []))
        lim = np.atleast_1d(_f64(limits if limits is not None else []))
        shape = (self.nt, self.nloc, len(z))
        out, keep = {}, []
        for pre in ("", "d") if derivative else ("",):
            for key in ("mean", "sd", "min", "max"):
                out[pre + key] = np.zeros(shape)
            if len(q):
                out[pre + "quant"] = np.zeros((len(q),) + shape)
            out[pre + "nfin"] = np.zeros(shape, np.int32)
            if all_maps:
                out[pre + "s_all"] = np.zeros((nens,) + shape)
            m = UcfEnsembleMaps(*(_addr(out.get(pre + key)) for key in ("mean", "sd", "min", "max", "quant", "s_all", "nfin")))
            keep.append(m)
        if len(lim):
            out["pexc"] = np.zeros((len(lim),) + shape)
        out["nbad"] = np.zeros(2, np.int64)
        st = UcfStats()
        levels = (len(z), _addr(z), len(q), _addr(q) if len(q) else None, len(lim), _addr(lim) if len(lim) else None, C.byref(keep[0]),
                  C.byref(keep[1]) if derivative else None, _addr(out.get("pexc")), _addr(out["nbad"]), C.byref(st) if with_stats else None)
        if weights is None:
            _libmod.check(self._lib.ucf_field_ensemble(self._h, plan._h, len(ids), _addr(ids), nens, _addr(thetas), *levels))
        else:
            w = np.atleast_1d(_f64(weights))
            if len(w) != nens:
                raise ValueError("weights: one value per member")
            out["u"] = np.zeros(nens, np.uint64)
            ess, nl = C.c_double(), C.c_int()
            _libmod.check(self._lib.ucf_field_ensemble_weighted(self._h, plan._h, len(ids), _addr(ids), nens, _addr(thetas), _addr(w), *levels,
                                                                _addr(out["u"]), C.addressof(ess), C.addressof(nl)))
            out["ess"], out["nlaunched"] = float(ess.value), int(nl.value)
        if with_stats:
            out["stats"] = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return out

    def worth(self, plan, free, theta, cov, z, targets, sigma, sigma_d: float = 0.0, times=None, picks: int = 1, weights=None,
              allowed=None, dlog: float = 1e-3, with_stats: bool = False) -> dict:
        """where the next observation wells have to go (ucf_field_worth): every (location, depth) of the map is a candidate well
        that records the drawdown with standard deviation ``sigma`` (and, with ``sigma_d`` > 0, its log-time derivative) at the
        times selected by ``times`` (a mask [nt]; None: all).  ``targets`` are forecasts of the same map, (kind, k, i, z) each
        with kind 's' or 'ds' and the indices of time, location and depth; ``weights`` [ntgt] weigh them in the criterion
        (None: 1).  ``theta`` and ``cov`` are those of ``Fit.lm``.  Greedily ``picks`` wells are chosen among the candidates
        that ``allowed`` [nloc, nz] admits (None: all), each conditioning the covariance for the next round.  Returns prior
        [picks, ntgt], the variance of every target before a round; post [picks, ntgt, nloc, nz], what a candidate would leave
        of it; reduction = 1 - post / prior; crit [picks, nloc, nz], the weighted sum of post; nused [nloc, nz] (int32), the
        readings of a candidate that are finite; pick, per round (location, depth) or None; cov_post [npar, npar], the
        covariance after the last pick made.  ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        theta = np.atleast_1d(_f64(theta))
        if len(theta) != len(ids):
            raise ValueError("theta: one value per free parameter")
        npar = len(ids)
        cov = _f64(cov)
        if cov.shape != (npar, npar):
            raise ValueError("cov: [npar, npar]")
        z = np.atleast_1d(_f64(z))
        nz, picks = len(z), int(picks)
        kinds = {"s": 0, "ds": 1, 0: 0, 1: 1}
        tgt = np.ascontiguousarray([(kinds[t[0]], int(t[1]), int(t[2]), int(t[3])) for t in targets], dtype=np.int32).reshape(-1, 4)
        ntgt = len(tgt)
        tw = None if weights is None else np.atleast_1d(_f64(weights))
        if tw is not None and len(tw) != ntgt:
            raise ValueError("weights: one value per target")
        tsel = None if times is None else np.ascontiguousarray(np.asarray(times) != 0, dtype=np.int32)
        if tsel is not None and tsel.shape != (self.nt,):
            raise ValueError("times: a mask [nt]")
        cmask = None if allowed is None else np.ascontiguousarray(np.asarray(allowed) != 0, dtype=np.int32)
        if cmask is not None and cmask.size != self.nloc * nz:
            raise ValueError("allowed: a mask [nloc, nz]")
        n = max(picks, 0)
        out = {"prior": np.zeros((n, ntgt)), "post": np.zeros((n, ntgt, self.nloc, nz)), "crit": np.zeros((n, self.nloc, nz)),
               "nused": np.zeros((self.nloc, nz), np.int32), "cov_post": np.zeros((npar, npar))}
        pick = np.zeros(n, np.int32)
        st = UcfStats()
        _libmod.check(self._lib.ucf_field_worth(
            self._h, plan._h, npar, _addr(ids), _addr(theta), float(dlog), _addr(cov), nz, _addr(z), float(sigma), float(sigma_d), _addr(tsel),
            ntgt, _addr(tgt), _addr(tw), picks, _addr(cmask), *(_addr(out[k]) for k in ("prior", "post", "crit", "nused")), _addr(pick),
            _addr(out["cov_post"]), C.byref(st) if with_stats else None))
        out["pick"] = [None if c < 0 else (int(c) // nz, int(c) % nz) for c in pick]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["reduction"] = 1.0 - out["post"] / out["prior"][:, :, None, None]
        if with_stats:
            out["stats"] = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return out

    def sustainable_yield(self, plan, free, thetas, z, controls, patterns, limit, smax, weights=None, q=(0.05, 0.5, 0.95), levels=(),
                          with_stats: bool = False) -> dict:
        """how much the wells may pump before a permitted drawdown is exceeded somewhere, under the ensemble ``thetas`` [nens,
        npar] (ucf_field_yield).  ``controls`` [nwell] gives every well its control 0 .. nctl-1 (wells of one control are
        scaled together; -1: the well is fixed), ``patterns`` [npat, nctl] the multipliers on the wells' q that are tried,
        ``limit`` [nt, nloc, nz] (or a scalar) the permitted dimensional drawdown (inf: not constrained) and ``smax`` the
        largest scale of interest.  Pattern p at scale lam pumps well j of control c at lam * patterns[p, c] * q_j.  Returns
        y [nens, npat], the largest admissible scale per member and pattern (0 where none is; NaN for a member with a value
        that is not finite); over the members mean, sd, min, max, nfin [npat], quant [nq, npat] at the levels ``q`` -- the
        level-q quantile is the scale that a share 1 - q of the ensemble admits, the yield at reliability 1 - q --, with
        ``levels`` pexc [nlev, npat], the share of members that admit more than a level, and pfeas [npat], the share that
        admit any scale; hi, lo, bind, dead [nens, npat], the two ends of the admissible interval, the output (an index into
        the flattened map) that binds hi (-1: smax does) and whether an output is over its limit at every scale; resp [nens,
        nctl + 1, ncon], the response slots, con [ncon], the constrained outputs, and nbad, the members that are not finite.
        With ``weights`` the members count by their weight as in ``ensemble`` and the result gains u, ess and nlaunched.
        ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        thetas = np.atleast_2d(_f64(thetas))
        if thetas.ndim != 2 or thetas.shape[1] != len(ids):
            raise ValueError("thetas: [nens, npar], one value per free parameter")
        nens = len(thetas)
        z = np.atleast_1d(_f64(z))
        ctl = np.ascontiguousarray(np.atleast_1d(controls), dtype=np.int32)
        if ctl.shape != (self.nwell,):
            raise ValueError("controls: one control (or -1) per well")
        x = np.atleast_2d(_f64(patterns))
        if x.ndim != 2 or x.shape[1] < 1:
            raise ValueError("patterns: [npat, nctl]")
        npat, nctl = x.shape
        if ctl.max() >= nctl:
            raise ValueError("patterns: one column per control")
        shape = (self.nt, self.nloc, len(z))
        try:
            lim = np.ascontiguousarray(np.broadcast_to(_f64(limit), shape))
        except ValueError:
            raise ValueError("limit: [nt, nloc, nz] or a scalar") from None
        qs = np.atleast_1d(_f64(q if q is not None else []))
        lev = np.atleast_1d(_f64(levels if levels is not None else []))
        w = None if weights is None else np.atleast_1d(_f64(weights))
        if w is not None and len(w) != nens:
            raise ValueError("weights: one value per member")
        nslot = max(int(np.isfinite(lim).sum()), 1)
        out = {"y": np.zeros((nens, npat)), "pfeas": np.zeros(npat), "nfin": np.zeros(npat, np.int32)}
        for key in ("mean", "sd", "min", "max"):
            out[key] = np.zeros(npat)
        if len(qs):
            out["quant"] = np.zeros((len(qs), npat))
        if len(lev):
            out["pexc"] = np.zeros((len(lev), npat))
        out["hi"], out["lo"] = np.zeros((nens, npat)), np.zeros((nens, npat))
        out["bind"], out["dead"] = np.zeros((nens, npat), np.int32), np.zeros((nens, npat), np.int32)
        out["resp"] = np.zeros((nens, nctl + 1, nslot))
        con, ncon, nbad = np.zeros(lim.size, np.int32), C.c_int(), C.c_longlong()
        maps = UcfEnsembleMaps(*(_addr(out.get(key)) for key in ("mean", "sd", "min", "max", "quant", "y", "nfin")))
        st = UcfStats()
        u, ess, nl = np.zeros(nens, np.uint64), C.c_double(), C.c_int()
        _libmod.check(self._lib.ucf_field_yield(
            self._h, plan._h, len(ids), _addr(ids), nens, _addr(thetas), _addr(w), len(z), _addr(z), nctl, _addr(ctl), npat, _addr(x),
            _addr(lim), float(smax), len(qs), _addr(qs) if len(qs) else None, len(lev), _addr(lev) if len(lev) else None, C.byref(maps),
            _addr(out.get("pexc")), _addr(out["pfeas"]), *(_addr(out[k]) for k in ("hi", "lo", "bind", "dead", "resp")), _addr(con),
            C.addressof(ncon), C.addressof(nbad), C.byref(st) if with_stats else None, _addr(u), C.addressof(ess), C.addressof(nl)))
        out["con"], out["nbad"] = con[:ncon.value].copy(), int(nbad.value)
        if w is not None:
            out["u"], out["ess"], out["nlaunched"] = u, float(ess.value), int(nl.value)
        if with_stats:
            out["stats"] = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return out

    def optimal_rates(self, plan, free, thetas, z, controls, objectives, xmax, limit, weights=None, q=(0.05, 0.5, 0.95), maxit: int = 64,
                      reliability: bool = True, with_stats: bool = False) -> "Allocation":
        """how the abstraction should be distributed over the wells so that an objective is largest and every constrained output
        stays within its limit, under the ensemble ``thetas`` [nens, npar] (ucf_field_allocate): per member and objective one
        linear programme in the multipliers x_c on the q of the wells of control c, solved on the GPU on the response slots of
        ``sustainable_yield``.  ``controls`` [nwell] and ``limit`` as there; ``objectives`` [nobj, nctl] (or [nctl]) are the weights
        of g = sum_c w_c x_c (all ones: the total abstraction in units of today's rates); ``xmax`` [nctl] (or a scalar) the pump
        capacities, 0 <= x_c <= xmax_c; ``maxit`` the pivots allowed per programme.  With ``reliability`` the members' optima are
        scaled down to what a share 1 - q of the ensemble admits and the best of them is returned per level and objective.
        Returns an ``Allocation``.  ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        thetas = np.atleast_2d(_f64(thetas))
        if thetas.ndim != 2 or thetas.shape[1] != len(ids):
            raise ValueError("thetas: [nens, npar], one value per free parameter")
        nens = len(thetas)
        z = np.atleast_1d(_f64(z))
        ctl = np.ascontiguousarray(np.atleast_1d(controls), dtype=np.int32)
        if ctl.shape != (self.nwell,):
            raise ValueError("controls: one control (or -1) per well")
        w = np.atleast_2d(_f64(objectives))
        if w.ndim != 2 or w.shape[1] < 1:
            raise ValueError("objectives: [nobj, nctl]")
        nobj, nctl = w.shape
        if ctl.max() >= nctl:
            raise ValueError("objectives: one column per control")
        try:
            cap = np.ascontiguousarray(np.broadcast_to(_f64(xmax), (nctl,)))
        except ValueError:
            raise ValueError("xmax: [nctl] or a scalar") from None
        shape = (self.nt, self.nloc, len(z))
        try:
            lim = np.ascontiguousarray(np.broadcast_to(_f64(limit), shape))
        except ValueError:
            raise ValueError("limit: [nt, nloc, nz] or a scalar") from None
        qs = np.atleast_1d(_f64(q if q is not None else []))
        wt = None if weights is None else np.atleast_1d(_f64(weights))
        if wt is not None and len(wt) != nens:
            raise ValueError("weights: one value per member")
        nslot = max(int(np.isfinite(lim).sum()), 1)
        out = {"x": np.zeros((nens, nobj, nctl)), "g": np.zeros((nens, nobj)), "status": np.zeros((nens, nobj), np.int32),
               "iters": np.zeros((nens, nobj), np.int32), "work": np.zeros((nens, nobj, nctl), np.int32), "lam": np.zeros((nens, nobj, nctl))}
        if len(qs):
            out["gquant"] = np.zeros((len(qs), nobj))
        if reliability:
            npat = nens * nobj
            out["quant"], out["value"] = np.zeros((len(qs), npat)), np.zeros((len(qs), npat))
            out["best"], out["best_x"] = np.zeros((len(qs), nobj), np.int32), np.zeros((len(qs), nobj, nctl))
        out["resp"] = np.zeros((nens, nctl + 1, nslot))
        con, ncon, nbad = np.zeros(lim.size, np.int32), C.c_int(), C.c_longlong()
        st = UcfStats()
        u, ess, nl = np.zeros(nens, np.uint64), C.c_double(), C.c_int()
        _libmod.check(self._lib.ucf_field_allocate(
            self._h, plan._h, len(ids), _addr(ids), nens, _addr(thetas), _addr(wt), len(z), _addr(z), nctl, _addr(ctl), nobj, _addr(w), _addr(cap),
            int(maxit), _addr(lim), *(_addr(out[k]) for k in ("x", "g", "status", "iters", "work", "lam")), len(qs), _addr(qs) if len(qs) else None,
            *(_addr(out.get(k)) for k in ("quant", "value", "best", "best_x", "gquant")), _addr(out["resp"]), _addr(con), C.addressof(ncon),
            C.addressof(nbad), C.byref(st) if with_stats else None, _addr(u), C.addressof(ess), C.addressof(nl)))
        res = Allocation(objectives=w, xmax=cap, q=qs, con=con[:ncon.value].copy(), nbad=int(nbad.value), **out)
        if wt is not None:
            res.u, res.ess, res.nlaunched = u, float(ess.value), int(nl.value)
        if with_stats:
            res.stats = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return res

    def time_to_limit(self, plan, free, thetas, z, limits, kinds="first_above", weights=None, q=(0.05, 0.5, 0.95), horizons=(),
                      abscissa: str = "t", never=None, all_times: bool = False, with_stats: bool = False) -> "TimeToLimit":
        """when the drawdown passes a limit, and how sure that is under the ensemble ``thetas`` [nens, npar]
        (ucf_field_ensemble_times).  ``limits`` [nlim] are dimensional drawdowns; ``kinds`` (one for all, or one per limit) is
        'first_above', the time of the first up-crossing, or 'last_above', the time from which the drawdown stays at or below
        the limit (the recovery time).  Per member, limit, location and depth the time is interpolated linearly in the
        ``abscissa`` -- 't', or 'lnt', the logarithm of the field's times -- between the two times of the field that bracket the
        crossing; a member that does not cross within the field's times gets ``never`` (default 2 t[-1]).  The members are
        reduced on the GPU as in ``ensemble``, with ``weights`` as there.  Returns a ``TimeToLimit`` whose arrays are
        [nlim, nloc, nz], a leading axis for quantile levels, horizons or members before it: mean, sd, min, max, nfin, quant at
        the levels ``q``, later [nhor, ...], the share of members whose time lies beyond a horizon (given as times) and, with
        ``all_times``, all [nens, ...].  With 'lnt' min, max, quant, all (and never, horizons) are times, exponentiated back --
        monotone, hence exact in rank; a censored value comes back as ``never`` itself --, while mean and sd stay in ln t:
        ``log_moments`` says so.  ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        thetas = np.atleast_2d(_f64(thetas))
        if thetas.ndim != 2 or thetas.shape[1] != len(ids):
            raise ValueError("thetas: [nens, npar], one value per free parameter")
        nens = len(thetas)
        z = np.atleast_1d(_f64(z))
        lim = np.atleast_1d(_f64(limits))
        if lim.ndim != 1 or len(lim) < 1:
            raise ValueError("limits: at least one drawdown limit")
        if isinstance(kinds, (str, int)):
            kinds = [kinds] * len(lim)
        try:
            kind = np.ascontiguousarray([TIME_KINDS.get(k, k) for k in kinds], dtype=np.int32)
        except (TypeError, ValueError):
            raise ValueError("kinds: 'first_above' or 'last_above'") from None
        if kind.shape != lim.shape:
            raise ValueError("kinds: one for all limits, or one per limit")
        if abscissa not in ("t", "lnt"):
            raise ValueError("abscissa: 't' or 'lnt'")
        log = abscissa == "lnt"
        w = None if weights is None else np.atleast_1d(_f64(weights))
        if w is not None and len(w) != nens:
            raise ValueError("weights: one value per member")
        qs = np.atleast_1d(_f64(q if q is not None else []))
        hor = np.atleast_1d(_f64(horizons if horizons is not None else []))
        never = 2.0 * self._times[-1] if never is None else float(never)
        tau = np.log(self._times) if log else None
        with np.errstate(invalid="ignore", divide="ignore"):
            tau_never, hor_tau = (float(np.log(never)), np.log(hor)) if log else (never, hor)
        shape = (len(lim), self.nloc, len(z))
        out = {key: np.zeros(shape) for key in ("mean", "sd", "min", "max")}
        out["nfin"] = np.zeros(shape, np.int32)
        if len(qs):
            out["quant"] = np.zeros((len(qs),) + shape)
        if all_times:
            out["all"] = np.zeros((nens,) + shape)
        if len(hor):
            out["later"] = np.zeros((len(hor),) + shape)
        maps = UcfEnsembleMaps(*(_addr(out.get(key)) for key in ("mean", "sd", "min", "max", "quant", "all", "nfin")))
        nbad, st = C.c_longlong(), UcfStats()
        u, ess, nl = np.zeros(nens, np.uint64), C.c_double(), C.c_int()
        _libmod.check(self._lib.ucf_field_ensemble_times(
            self._h, plan._h, len(ids), _addr(ids), nens, _addr(thetas), _addr(w), len(z), _addr(z), _addr(tau), tau_never, len(lim),
            _addr(lim), _addr(kind), len(qs), _addr(qs) if len(qs) else None, len(hor), _addr(hor_tau) if len(hor) else None,
            C.byref(maps), _addr(out.get("later")), C.addressof(nbad), C.byref(st) if with_stats else None, _addr(u), C.addressof(ess),
            C.addressof(nl)))
        if log:
            for key in ("min", "max", "quant", "all"):
                if key in out:
                    censored = out[key] == tau_never         # exp(ln(never)) need not be never: the censoring value comes back as given
                    np.exp(out[key], out=out[key])
                    out[key][censored] = never
        res = TimeToLimit(limits=lim, kinds=kind, abscissa=abscissa, never=never, q=qs, horizons=hor, log_moments=log, nbad=int(nbad.value), **out)
        if w is not None:
            res.u, res.ess, res.nlaunched = u, float(ess.value), int(nl.value)
        if with_stats:
            res.stats = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return res

    def sobol(self, plan, free, thetas, z, derivative: bool = True, members: bool = False, with_stats: bool = False) -> "SobolMaps":
        """which parameter causes the spread of the drawdown (ucf_field_sobol): ``thetas`` [(npar + 2) n, npar] is a Saltelli
        design of the free parameters as ``sobol_design`` makes it (the library checks its structure); all its members are
        evaluated as ``ensemble`` evaluates them, stay on the GPU and are reduced there, per output, to the first-order index S
        (the share of the variance that a parameter explains alone), the total index ST (its share with every interaction) and
        their standard errors.  Returns a ``SobolMaps``.  ``plan`` is not modified."""
        ids = np.ascontiguousarray([par_id(n) for n in free], dtype=np.int32)
        thetas = np.atleast_2d(_f64(thetas))
        npar = len(ids)
        if thetas.ndim != 2 or thetas.shape[1] != npar:
            raise ValueError("thetas: [(npar + 2) n, npar], one value per free parameter")
        if len(thetas) % (npar + 2):
            raise ValueError("thetas: (npar + 2) n rows, the blocks of a Saltelli design")
        nbase, nmem = len(thetas) // (npar + 2), len(thetas)
        z = np.atleast_1d(_f64(z))
        shape = (self.nt, self.nloc, len(z))
        out, keep = {}, []
        for pre in ("", "d") if derivative else ("",):
            for key in ("S", "ST", "se_S", "se_ST"):
                out[pre + key] = np.zeros((npar,) + shape)
            out[pre + "mean"], out[pre + "var"] = np.zeros(shape), np.zeros(shape)
            out[pre + "nrow"] = np.zeros(shape, np.int32)
            if members:
                out[pre + "all"] = np.zeros((nmem,) + shape)
            keep.append(UcfSobolMaps(*(_addr(out.get(pre + key)) for key in ("S", "ST", "se_S", "se_ST", "mean", "var", "all", "nrow"))))
        out["nbad"] = np.zeros(2, np.int64)
        st = UcfStats()
        _libmod.check(self._lib.ucf_field_sobol(self._h, plan._h, npar, _addr(ids), nbase, _addr(thetas), len(z), _addr(z), C.byref(keep[0]),
                                                C.byref(keep[1]) if derivative else None, _addr(out["nbad"]), C.byref(st) if with_stats else None))
        res = SobolMaps(nbase=nbase, **out)
        if with_stats:
            res.stats = {k: getattr(st, k) for k, _ in UcfStats._fields_}
        return res

    def alloc_count(self) -> int:
        """device allocations made so far by the field"""
        return int(self._lib.ucf_field_alloc_count(self._h))
