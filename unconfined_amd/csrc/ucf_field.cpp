// ucf_field.cpp -- well fields (include/ucf.h): the superposed drawdown of several pumping and image wells through the grid path
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "ucf_host.h"
#include "ucf_field.h"

using namespace ucf_host;

int ucf_host::field_check_finite(const char* name, int n, const double* v)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return fail(UCF_ERR_BAD_ARGUMENT, "%s[%d]=%g is not finite", name, i, v[i]);
    return UCF_OK;
}

struct field_group {
    double t0 = 0.0;
    std::vector<int> wells;                // in the caller's order
};

struct ucf_field {
    int nwell = 0, nloc = 0, nt = 0;
    std::vector<double> xw, yw, qw, t0w, x, y, t;
    std::vector<field_group> groups;       // ascending t0
    std::vector<int> well_group;
    int device = -1;                       // where the buffers live: the device of the plan of the first ucf_field_drawdown
    ucf_buffer b_tD, b_sv, b_rD, b_tfac, b_col, b_wells, b_h, b_dh, b_s, b_ds, b_stats;      // grown on demand, kept
    // ucf_field_forecast: the slots [1 + 2 npar][nout] of s and ds, the staging of sens / dsens / se / dse, cov, the two counts
    ucf_buffer b_sall, b_dsall, b_sens, b_dsens, b_se, b_dse, b_cov, b_nbad;
    // ucf_field_ensemble: its slots [nens][nout] are b_sall / b_dsall; the levels, the limits and the staging of every statistic
    ucf_buffer b_ens;
    // ucf_field_ensemble_weighted: the integer weights u [nens]
    ucf_buffer b_u;
    // ucf_field_worth: its slots are b_sall / b_dsall; post [ntgt][ncand], crit [ncand], nused [ncand]; F, A, tw in one image
    // and tsel [nt]; the indices and the values of a gather
    ucf_buffer b_wpost, b_wcrit, b_wnused, b_wsmall, b_wtsel, b_widx, b_wval;
    // ucf_field_yield: the response slots R [nens][nctl + 1][ncon]; con [ncon] and ctl [nwell]; x [npat][nctl] and the limits
    // [ncon]; y, fe, hi, lo [4][nens][npat]; bind, dead [2][nens][npat].  Its statistics are staged in b_ens.
    ucf_buffer b_yR, b_yint, b_ysmall, b_yval, b_yidx;
    // ucf_field_allocate: x, lam [2][nens][nobj][nctl] and g [nens][nobj]; status, iters [2][nens][nobj] and work
    // [nens][nobj][nctl].  Its slots, limits and controls are those of ucf_field_yield (w, xmax and the patterns of the reliability
    // stage in b_ysmall), the reliability stage runs in b_yval / b_yidx and its statistics are staged in b_ens.
    ucf_buffer b_aval, b_aidx;
    // ucf_field_ensemble_times: T [nens][nlim][nloc][nz]; its series are b_sall, its tau, limits and kinds are staged in b_ens
    ucf_buffer b_tall;
    // ucf_field_sobol: its slots [(npar + 2) nbase][nout] are b_sall / b_dsall; the staging of every statistic of both maps
    ucf_buffer b_sob;
    ucf_plan* scratch = nullptr;           // the plan that ucf_field_forecast refreshes for every parameter set
    long long n_alloc = 0;
    // every device buffer above: the one list (ucf_field_destroy frees through it)
    std::array<ucf_buffer*, 37> buffers()
    {
        return {{&b_tD, &b_sv, &b_rD, &b_tfac, &b_col, &b_wells, &b_h, &b_dh, &b_s, &b_ds, &b_stats, &b_sall, &b_dsall, &b_sens, &b_dsens,
                 &b_se, &b_dse, &b_cov, &b_nbad, &b_ens, &b_u, &b_wpost, &b_wcrit, &b_wnused, &b_wsmall, &b_wtsel, &b_widx, &b_wval,
                 &b_yR, &b_yint, &b_ysmall, &b_yval, &b_yidx, &b_tall, &b_sob, &b_aval, &b_aidx}};
    }
};

namespace {
// what group g launches: the arrays of ucf_field_group
struct field_launch {
    int k0 = 0, nt = 0, nr = 0;
    std::vector<double> tD, rD, tfac;
    std::vector<int> sv, col;              // col [nloc][nwell], -1 = well not in g
};

int field_group_core(const ucf_field* f, const ucf_params& P, const ucf_derived& D, int g, field_launch& A)
{
    const field_group& G = f->groups[g];
    int k0 = 0;
    while (k0 < f->nt && !(f->t[k0] > G.t0)) k0++;
    A.k0 = k0;
    A.nt = f->nt - k0;
    A.tD.resize(A.nt); A.tfac.resize(A.nt); A.sv.assign(A.nt, 0);
    for (int i = 0; i < A.nt; i++) {
        const double dt = f->t[k0 + i] - G.t0;
        A.tD[i] = dt / D.Tc;
        A.tfac[i] = f->t[k0 + i] / dt;
    }
    const size_t nw = G.wells.size();
    std::vector<double> r((size_t)f->nloc * nw);
    for (int i = 0; i < f->nloc; i++)
        for (size_t a = 0; a < nw; a++) {
            const int j = G.wells[a];
            const double dx = f->x[i] - f->xw[j], dy = f->y[i] - f->yw[j];
            const double dist = std::sqrt(dx * dx + dy * dy);
            if (!std::isfinite(dist)) return fail(UCF_ERR_BAD_ARGUMENT, "the distance of location %d from well %d is not finite", i, j);
            if (dist < P.rw)
                return fail(UCF_ERR_BAD_ARGUMENT, "location %d lies %g from well %d: inside its bore (rw = %g)", i, dist, j, P.rw);
            r[i * nw + a] = dist / D.Lc;
        }
    A.rD = r;
    std::sort(A.rD.begin(), A.rD.end());
    A.rD.erase(std::unique(A.rD.begin(), A.rD.end()), A.rD.end());      // (positive and finite: equal values are equal bits)
    A.nr = (int)A.rD.size();
    A.col.assign((size_t)f->nloc * f->nwell, -1);
    for (int i = 0; i < f->nloc; i++)
        for (size_t a = 0; a < nw; a++)
            A.col[(size_t)i * f->nwell + G.wells[a]] = (int)(std::lower_bound(A.rD.begin(), A.rD.end(), r[i * nw + a]) - A.rD.begin());
    if ((long long)A.nt * A.nr > 0x7fffffffLL)
        return fail(UCF_ERR_BAD_ARGUMENT, "group %d: %d times x %d distinct distances is a grid larger than 2^31-1 points", g, A.nt, A.nr);
    if (A.nt > 0) {
        split_vector(P.j0s, A.nt, A.tD.data(), A.sv.data());
        int rc = check_grid_sv_of(P, D, A.nt, A.sv.data());
        if (rc) return rc;
    }
    return UCF_OK;
}

int field_group_out(const ucf_field* f, const ucf_params& P, const ucf_derived& D, int g, int* k0, int* nt_g, double* tD, int* sv,
                    int* nr_g, double* rD, int* col, double* tfac)
{
    if (g < 0 || g >= (int)f->groups.size()) return fail(UCF_ERR_BAD_ARGUMENT, "group %d outside 0..%d", g, (int)f->groups.size() - 1);
    field_launch A;
    int rc = field_group_core(f, P, D, g, A);
    if (rc) return rc;
    if (k0) *k0 = A.k0;
    if (nt_g) *nt_g = A.nt;
    if (nr_g) *nr_g = A.nr;
    if (tD) std::copy(A.tD.begin(), A.tD.end(), tD);
    if (sv) std::copy(A.sv.begin(), A.sv.end(), sv);
    if (rD) std::copy(A.rD.begin(), A.rD.end(), rD);
    if (col) std::copy(A.col.begin(), A.col.end(), col);
    if (tfac) std::copy(A.tfac.begin(), A.tfac.end(), tfac);
    return UCF_OK;
}

// every group's block of a shared buffer starts at a multiple of 32 entries (256 bytes of doubles)
size_t field_pad(size_t n) { return (n + 31) & ~(size_t)31; }

// what ucf_field_drawdown checks before it looks at the plan (null_what: the message for a NULL array, NULL if there is none);
// nout = nt nloc nz
int field_check_call(const ucf_field* f, int nz, const char* null_what, const double* z, long long& nout)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL field");
    if (nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nz=%d: at least one depth", nz);
    if (null_what) return fail(UCF_ERR_BAD_ARGUMENT, "%s", null_what);
    int rc = field_check_finite("z", nz, z);
    if (rc) return rc;
    nout = (long long)f->nt * f->nloc * nz;
    if (nout > 0x7fffffffLL * 256) return fail(UCF_ERR_BAD_ARGUMENT, "%d times x %d locations x %d depths: too many outputs for one call", f->nt, f->nloc, nz);
    return UCF_OK;
}

// The kernel that finishes a map once the group results lie in b_h / b_dh and the wells, columns and time factors in their
// buffers: `launch` enqueues it on the stream of the plan that ran the groups and returns a launcher's status.
struct field_finish {
    const char* what;
    std::function<int(const ucf_plan*, hipStream_t)> launch;
};

// field_superpose_kernel into s, ds [nt][nloc][nz] at d_s, d_ds -- device memory of the caller on the plan's device
field_finish field_superpose_into(ucf_field* f, int nz, int dimensionless, double* d_s, double* d_ds)
{
    return {"superposition", [=](const ucf_plan* pl, hipStream_t st) {
                return ucf_field_launch_superpose(f->nt, f->nloc, nz, f->nwell, (const ucf_field_well*)f->b_wells.p, (const int*)f->b_col.p,
                                                  (const double*)f->b_tfac.p, (const double*)f->b_h.p, (const double*)f->b_dh.p,
                                                  dimensionless ? 0 : 1, pl->D.Hc, d_s, d_ds, st);
            }};
}

// One map of the field under plan pl, whose launch arrays are L (field_group_core under pl's parameters): the arrays go to the
// device, every group takes one call of the grid path, and `finish` (field_superpose_kernel for a map, field_response_kernel
// for the slots of ucf_field_yield) forms its outputs from the group results; pl's device is current.  The counters of the
// groups are ADDED to *stats (NULL ok).  The plan's stream has drained when the call returns.
int field_map_core(ucf_field* f, ucf_plan* pl, const std::vector<field_launch>& L, int nz, const double* z, const field_finish& finish,
                   ucf_stats* stats)
{
    const int ng = (int)f->groups.size();
    // zD, zLay as in ucf_drawdown_multi
    std::vector<double> zD(nz);
    std::vector<int> zl(nz);
    for (int j = 0; j < nz; j++) zD[j] = z[j] / pl->D.Lc;
    int rc = ucf_zlay(pl, nz, zD.data(), zl.data());
    if (rc) return rc;
    // one staging image per array, the groups one after the other
    std::vector<size_t> toff(ng), roff(ng), hoff(ng);
    size_t nT = 0, nR = 0, nH = 0;
    for (int g = 0; g < ng; g++) {
        toff[g] = nT; roff[g] = nR; hoff[g] = nH;
        nT += field_pad(L[g].nt); nR += field_pad(L[g].nr); nH += field_pad((size_t)L[g].nt * L[g].nr * nz);
    }
    if (nT > 0x7fffffffULL) return fail(UCF_ERR_BAD_ARGUMENT, "too many launched times");
    std::vector<double> tD(nT, 1.0), rD(nR, 1.0), tfac(nT, 0.0);
    std::vector<int> sv(nT, 0), col((size_t)f->nloc * f->nwell);
    std::vector<ucf_field_well> wells(f->nwell);
    for (int g = 0; g < ng; g++) {
        std::copy(L[g].tD.begin(), L[g].tD.end(), tD.begin() + toff[g]);
        std::copy(L[g].sv.begin(), L[g].sv.end(), sv.begin() + toff[g]);
        std::copy(L[g].tfac.begin(), L[g].tfac.end(), tfac.begin() + toff[g]);
        std::copy(L[g].rD.begin(), L[g].rD.end(), rD.begin() + roff[g]);
    }
    for (int j = 0; j < f->nwell; j++) {
        const int g = f->well_group[j];
        wells[j] = ucf_field_well{f->qw[j], (long long)hoff[g], L[g].k0, L[g].nr, (int)toff[g], 0};
        for (int i = 0; i < f->nloc; i++) col[(size_t)i * f->nwell + j] = L[g].col[(size_t)i * f->nwell + j];
    }
    if ((rc = grow_buffer(f->b_tD, sizeof(double) * nT, "group times", f->n_alloc)) || (rc = grow_buffer(f->b_sv, sizeof(int) * nT, "split vectors", f->n_alloc)) ||
        (rc = grow_buffer(f->b_tfac, sizeof(double) * nT, "time factors", f->n_alloc)) || (rc = grow_buffer(f->b_rD, sizeof(double) * nR, "group distances", f->n_alloc)) ||
        (rc = grow_buffer(f->b_col, sizeof(int) * col.size(), "columns", f->n_alloc)) || (rc = grow_buffer(f->b_wells, sizeof(ucf_field_well) * wells.size(), "wells", f->n_alloc)) ||
        (rc = grow_buffer(f->b_h, sizeof(double) * nH, "group drawdowns", f->n_alloc)) || (rc = grow_buffer(f->b_dh, sizeof(double) * nH, "group derivatives", f->n_alloc)) ||
        (rc = grow_buffer(f->b_stats, sizeof(ucf_stats) * ng, "counters", f->n_alloc))) return rc;
    hipStream_t st = plan_stream(pl);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};                     // the staging above outlives the copies
    if (hipMemcpyAsync(f->b_tD.p, tD.data(), sizeof(double) * nT, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(f->b_sv.p, sv.data(), sizeof(int) * nT, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(f->b_tfac.p, tfac.data(), sizeof(double) * nT, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(f->b_rD.p, rD.data(), sizeof(double) * nR, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(f->b_col.p, col.data(), sizeof(int) * col.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(f->b_wells.p, wells.data(), sizeof(ucf_field_well) * wells.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(f->b_stats.p, 0, sizeof(ucf_stats) * ng, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the field's launch arrays failed: %s", hipGetErrorString(hipGetLastError()));
    // per group one call of the grid path, results into the field's buffers
    for (int g = 0; g < ng; g++) {
        if (L[g].nt == 0) continue;
        rc = ucf_drawdown_grid_device(pl, L[g].nt, (const double*)f->b_tD.p + toff[g], (const int*)f->b_sv.p + toff[g], L[g].nr,
                                      (const double*)f->b_rD.p + roff[g], nz, zD.data(), zl.data(), (double*)f->b_h.p + hoff[g],
                                      (double*)f->b_dh.p + hoff[g], stats ? (ucf_stats*)f->b_stats.p + g : nullptr, st);
        if (rc) return rc;
    }
    rc = finish.launch(pl, st);
    if (rc) return fail(rc, "%s kernel launch failed: %s", finish.what, hipGetErrorString(hipGetLastError()));
    if (!stats) return UCF_OK;
    std::vector<ucf_stats> gst(ng);
    if ((rc = copy_back({{gst.data(), f->b_stats.p, sizeof(ucf_stats) * ng}}, st, pl->device))) return rc;
    for (int g = 0; g < ng; g++) stats_add(*stats, gst[g]);
    return UCF_OK;
}

// the status of a parameter set of a forecast that a check refused, naming the set and the parameter moved (as fit_evaluate)
int forecast_set_failed(int rc, int k, const int* ids, double dlog)
{
    std::string why = ucf_last_error();
    char nb[32];
    if (k == 0) return fail(rc, "set 0: %s", why.c_str());
    return fail(rc, "set %d, %s moved by %+g in its logarithm: %s", k, fit_par_name(ids[(k - 1) / 2], nb, sizeof(nb)), (k & 1) ? dlog : -dlog, why.c_str());
}

// the same for member m of an ensemble, naming the member and its parameter values
int ensemble_member_failed(int rc, int m, int npar, const int* ids, const double* theta)
{
    std::string why = ucf_last_error(), vals;
    char nb[32], one[96];
    for (int j = 0; j < npar; j++) {
        snprintf(one, sizeof(one), "%s%s=%g", j ? ", " : "", fit_par_name(ids[j], nb, sizeof(nb)), theta[j]);
        vals += one;
    }
    return fail(rc, "member %d (%s): %s", m, vals.c_str(), why.c_str());
}

// what ucf_field_forecast and ucf_field_ensemble check on a covariance in ln theta
int field_check_cov(int npar, const double* cov)
{
    for (int j = 0; j < npar; j++)
        for (int k = 0; k < npar; k++) {
            const double c = cov[j * npar + k];
            if (!std::isfinite(c)) return fail(UCF_ERR_BAD_ARGUMENT, "cov[%d][%d]=%g is not finite", j, k, c);
            if (c != cov[k * npar + j]) return fail(UCF_ERR_BAD_ARGUMENT, "cov[%d][%d]=%g differs from cov[%d][%d]=%g: not symmetric", j, k, c, k, j, cov[k * npar + j]);
            if (j == k && c < 0.0) return fail(UCF_ERR_BAD_ARGUMENT, "cov[%d][%d]=%g: a negative variance", j, j, c);
        }
    return UCF_OK;
}

// The field's scratch plan for a sequence of parameter sets that begins with `first`, on pl's device and in pl's mode: made
// once, refreshed per set; made anew where the caller's plan has another model or other settings
int field_scratch_plan(ucf_field* f, const ucf_plan* pl, const ucf_params& first)
{
    const int mode = pl->mode | (pl->force_layout0 << 1);
    if (f->scratch && ucf_plan_update(f->scratch, &first) != UCF_OK) {
        ucf_plan_destroy(f->scratch);
        f->scratch = nullptr;
    }
    if (!f->scratch) {
        int rc = ucf_plan_create_on(&first, pl->device, &f->scratch);
        if (rc) return rc;
        f->n_alloc++;
    }
    (void)ucf_plan_set_mode(f->scratch, mode);
    return UCF_OK;
}

// What every call that launches does between its last check and its first launch: a device there is, the field's buffers
// live on the plan's device (from here on they do), *stats (NULL ok) starts at zero, and -- where the call runs a sequence
// of parameter sets, `first` the one that runs first -- the scratch plan holds it.
int field_begin_launches(ucf_field* f, const ucf_plan* pl, ucf_stats* stats, const ucf_params* first)
{
    int rc = require_device();
    if (rc) return rc;
    if (f->device >= 0 && f->device != pl->device)
        return fail(UCF_ERR_BAD_ARGUMENT, "the field's buffers live on device %d, the plan on device %d", f->device, pl->device);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (first && (rc = field_scratch_plan(f, pl, *first))) return rc;
    f->device = pl->device;
    return UCF_OK;
}

// What ucf_field_forecast and ucf_field_ensemble run per parameter set, for k = 0 .. nset-1 in this order: the scratch plan
// (which holds the first set that runs) refreshed to sets[k], then field_map_core under the launch arrays that launch_of(k, L) hands out --
// kept from the checks (forecast) or formed again (ensemble) -- finished by finish_of(k): field_slot_superpose, into slot k of
// b_sall / b_dsall [nset][nout], dimensional; for ucf_field_yield the response slots of member k.
// A set that anything refuses: failed(rc, k).  With u (ucf_field_ensemble_weighted) a set with u[k] == 0 is left out, its slot
// untouched; the scratch plan then holds the first set that is not.
template <class Launch, class Finish, class Failed>
int field_map_sets(ucf_field* f, int nset, const ucf_params* sets, Launch launch_of, int nz, const double* z, Finish finish_of,
                   ucf_stats* stats, Failed failed, const unsigned long long* u = nullptr)
{
    ucf_plan* sp = f->scratch;
    bool held = true;                      // the scratch plan holds the next set that runs
    for (int k = 0; k < nset; k++) {
        int rc;
        if (u && u[k] == 0) continue;
        if (!held && (rc = ucf_plan_update(sp, &sets[k]))) return failed(rc, k);
        held = false;
        const std::vector<field_launch>* L = nullptr;
        if ((rc = launch_of(k, L))) return failed(rc, k);
        rc = field_map_core(f, sp, *L, nz, z, finish_of(k), stats);
        if (rc) return failed(rc, k);
    }
    return UCF_OK;
}

// finish_of for the maps of a forecast or an ensemble: slot k of b_sall / b_dsall [nset][nout] (grown before the call), dimensional
auto field_slot_superpose(ucf_field* f, int nz, long long nout)
{
    return [=](int k) { return field_superpose_into(f, nz, 0, (double*)f->b_sall.p + (size_t)k * nout, (double*)f->b_dsall.p + (size_t)k * nout); };
}

// the launch arrays of every group of the field under P
int field_launches_of(const ucf_field* f, const ucf_params& P, std::vector<field_launch>& L)
{
    ucf_derived D;
    nondimensionalise(P, D);
    L.resize(f->groups.size());
    for (size_t g = 0; g < L.size(); g++) {
        int rc = field_group_core(f, P, D, (int)g, L[g]);
        if (rc) return rc;
    }
    return UCF_OK;
}

// What ucf_field_forecast and ucf_field_worth share: the 1 + 2 npar parameter sets of a forecast and what every group launches
// under each of them
struct forecast_work {
    ucf_params sets[1 + 2 * UCF_FIT_MAX_PAR];
    std::vector<std::vector<field_launch>> L;
};

// all of W under pl's parameters, before any launch
int forecast_sets_of(const ucf_field* f, const ucf_plan* pl, int npar, const int* ids, const double* theta, double dlog, forecast_work& W)
{
    int rc = ucf_field_forecast_sets(&pl->P, npar, ids, theta, dlog, W.sets);
    if (rc) return rc;
    const int nset = 1 + 2 * npar, ng = (int)f->groups.size();
    W.L.assign(nset, std::vector<field_launch>(ng));
    for (int k = 0; k < nset; k++) {
        ucf_derived D;
        nondimensionalise(W.sets[k], D);
        for (int g = 0; g < ng; g++)
            if ((rc = field_group_core(f, W.sets[k], D, g, W.L[k][g]))) return forecast_set_failed(rc, k, ids, dlog);
    }
    return UCF_OK;
}

// the slots b_sall / b_dsall [1 + 2 npar][nout], grown and filled by field_map_sets; field_begin_launches has run with W.sets[0]
// and the plan's device is current
int forecast_slots(ucf_field* f, int npar, const int* ids, double dlog, const forecast_work& W, int nz, const double* z, long long nout,
                   ucf_stats* stats)
{
    const int nset = 1 + 2 * npar;
    const size_t sa = sizeof(double) * (size_t)nout * nset;
    int rc;
    if ((rc = grow_buffer(f->b_sall, sa, "drawdown of every set", f->n_alloc)) || (rc = grow_buffer(f->b_dsall, sa, "derivative of every set", f->n_alloc)))
        return rc;
    return field_map_sets(f, nset, W.sets, [&](int k, const std::vector<field_launch>*& Lk) { Lk = &W.L[k]; return UCF_OK; }, nz, z,
                          field_slot_superpose(f, nz, nout), stats,
                          [&](int rc_k, int k) { return forecast_set_failed(rc_k, k, ids, dlog); });
}

// ---- data worth (ucf_field_worth, ucf_worth_condition, ucf_debug_field_worth): the host arithmetic that include/ucf.h states

// J of one datum from its 2 npar slot values v (v[2j]: slot 1 + 2j, v[2j + 1]: slot 2 + 2j); false where one is not finite
bool worth_J(int npar, const double* v, double two_dlog, double* J)
{
    bool ok = true;
    for (int j = 0; j < npar; j++) {
        ok = ok && std::isfinite(v[2 * j]) && std::isfinite(v[2 * j + 1]);
        J[j] = (v[2 * j] - v[2 * j + 1]) / two_dlog;
    }
    return ok;
}

// g = F' J
void worth_FtJ(int npar, const double* F, const double* J, double* g)
{
    for (int j = 0; j < npar; j++) {
        double acc = 0.0;
        for (int i = 0; i < npar; i++) acc = acc + F[i * npar + j] * J[i];
        g[j] = acc;
    }
}

// what ucf_field_worth and ucf_debug_field_worth check on the targets' weights and on the selection of times
int worth_check_weights(int ntgt, const double* tw, int nt, const int* tsel)
{
    if (ntgt < 1 || ntgt > UCF_WORTH_MAX_TGT) return fail(UCF_ERR_BAD_ARGUMENT, "ntgt=%d outside 1..%d", ntgt, UCF_WORTH_MAX_TGT);
    for (int t = 0; tw && t < ntgt; t++)
        if (!(tw[t] >= 0.0) || !std::isfinite(tw[t])) return fail(UCF_ERR_BAD_ARGUMENT, "tw[%d]=%g must be finite and not negative", t, tw[t]);
    bool any = !tsel;
    for (int k = 0; tsel && k < nt; k++) any = any || tsel[k] != 0;
    if (!any) return fail(UCF_ERR_BAD_ARGUMENT, "tsel selects none of the %d times: a well that is never read", nt);
    return UCF_OK;
}

// The 2 npar perturbed slot values of the outputs e[0 .. ne) of both maps, to the host: hs, hd [ne][2 npar], value v of output q
// from slot 1 + v.  b_widx and b_wval hold at least 2 npar ne and 4 npar ne entries.  The stream has drained on return.
int worth_fetch(ucf_field* f, hipStream_t st, int device, int npar, long long nout, int ne, const long long* e, double* hs, double* hd)
{
    const int n = 2 * npar * ne;
    std::vector<long long> idx((size_t)n);
    for (int q = 0; q < ne; q++)
        for (int v = 0; v < 2 * npar; v++) idx[(size_t)q * 2 * npar + v] = (long long)(1 + v) * nout + e[q];
    drain drained{st};                     // idx outlives its copy
    if (hipMemcpyAsync(f->b_widx.p, idx.data(), sizeof(long long) * n, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the gather's indices failed: %s", hipGetErrorString(hipGetLastError()));
    double* d_val = (double*)f->b_wval.p;
    int rc = ucf_field_launch_gather(n, (const long long*)f->b_widx.p, (const double*)f->b_sall.p, d_val, st);
    if (rc == UCF_OK) rc = ucf_field_launch_gather(n, (const long long*)f->b_widx.p, (const double*)f->b_dsall.p, d_val + n, st);
    if (rc) return fail(rc, "gather kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return copy_back({{hs, d_val, sizeof(double) * n}, {hd, d_val + n, sizeof(double) * n}}, st, device);
}

// splitmix64 (include/ucf.h states it with ucf_field_ensemble_draw)
double ensemble_uniform(unsigned long long& state)
{
    state += 0x9E3779B97F4A7C15ULL;
    unsigned long long x = state;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    x = x ^ (x >> 31);
    return ((double)(x >> 11) + 0.5) * 0x1p-53;
}
}  // namespace

int ucf_host::ensemble_check_levels(int nens, int nq, const double* q, int nlim, const double* limit, bool want_quant, bool want_pexc,
                                    const char* nlim_name, const char* limit_name)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (nq < 0 || nq > UCF_ENSEMBLE_MAX_Q) return fail(UCF_ERR_BAD_ARGUMENT, "nq=%d outside 0..%d", nq, UCF_ENSEMBLE_MAX_Q);
    if (nlim < 0 || nlim > UCF_ENSEMBLE_MAX_Q) return fail(UCF_ERR_BAD_ARGUMENT, "%s=%d outside 0..%d", nlim_name, nlim, UCF_ENSEMBLE_MAX_Q);
    if (nq > 0 && !q) return fail(UCF_ERR_BAD_ARGUMENT, "NULL q with nq=%d", nq);
    if (nlim > 0 && !limit) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s with %s=%d", limit_name, nlim_name, nlim);
    for (int i = 0; i < nq; i++)
        if (!std::isfinite(q[i]) || q[i] < 0.0 || q[i] > 1.0) return fail(UCF_ERR_BAD_ARGUMENT, "q[%d]=%g is not a level in [0,1]", i, q[i]);
    int rc = field_check_finite(limit_name, nlim, limit);
    if (rc) return rc;
    if (want_quant && nq == 0) return fail(UCF_ERR_BAD_ARGUMENT, "quant is asked for with nq=0: no level to form it at");
    if (want_pexc && nlim == 0) return fail(UCF_ERR_BAD_ARGUMENT, "pexc is asked for with %s=0: no %s to exceed", nlim_name, limit_name);
    return UCF_OK;
}

extern "C" {

int ucf_field_create(int nwell, const double* xw, const double* yw, const double* qw, const double* t0w, int nloc, const double* x,
                     const double* y, int nt, const double* t, ucf_field** out)
{
    if (out) *out = nullptr;
    if (!out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (nwell < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nwell=%d: at least one well", nwell);
    if (nloc < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nloc=%d: at least one location", nloc);
    if (nt < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nt=%d: at least one time", nt);
    if (!xw || !yw || !qw || !t0w || !x || !y || !t) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    int rc;
    if ((rc = field_check_finite("xw", nwell, xw)) || (rc = field_check_finite("yw", nwell, yw)) || (rc = field_check_finite("qw", nwell, qw)) ||
        (rc = field_check_finite("t0w", nwell, t0w)) || (rc = field_check_finite("x", nloc, x)) || (rc = field_check_finite("y", nloc, y)) ||
        (rc = field_check_finite("t", nt, t))) return rc;
    for (int j = 0; j < nwell; j++) {
        if (qw[j] == 0.0) return fail(UCF_ERR_BAD_ARGUMENT, "qw[%d] is 0: a well without a rate", j);
        if (!(t0w[j] >= 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "t0w[%d]=%g is negative", j, t0w[j]);
    }
    if (!(t[0] > 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "t[0]=%g is not a positive time", t[0]);
    for (int k = 1; k < nt; k++)
        if (!(t[k] > t[k - 1])) return fail(UCF_ERR_BAD_ARGUMENT, "t[%d]=%g does not lie after t[%d]=%g: times must increase strictly", k, t[k], k - 1, t[k - 1]);
    ucf_field* f = new (std::nothrow) ucf_field();
    if (!f) return fail(UCF_ERR_NOMEM, "host allocation failed");
    f->nwell = nwell; f->nloc = nloc; f->nt = nt;
    f->xw.assign(xw, xw + nwell); f->yw.assign(yw, yw + nwell); f->qw.assign(qw, qw + nwell); f->t0w.assign(t0w, t0w + nwell);
    f->x.assign(x, x + nloc); f->y.assign(y, y + nloc); f->t.assign(t, t + nt);
    for (double& v : f->t0w) v = v + 0.0;                        // -0.0 is the start time +0.0
    // wells with the same start time form a group; groups in ascending t0, wells in the caller's order
    std::vector<double> starts = f->t0w;
    std::sort(starts.begin(), starts.end());
    starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
    f->groups.resize(starts.size());
    f->well_group.resize(nwell);
    for (size_t g = 0; g < starts.size(); g++) f->groups[g].t0 = starts[g];
    for (int j = 0; j < nwell; j++) {
        const int g = (int)(std::lower_bound(starts.begin(), starts.end(), f->t0w[j]) - starts.begin());
        f->well_group[j] = g;
        f->groups[g].wells.push_back(j);
    }
    *out = f;
    return UCF_OK;
}

void ucf_field_destroy(ucf_field* f)
{
    if (!f) return;
    ucf_plan_destroy(f->scratch);
    if (f->device >= 0) {
        device_switch sw(f->device);
        for (ucf_buffer* b : f->buffers()) free_buffer(*b);
    }
    delete f;
}

int ucf_field_group_count(const ucf_field* f, int* ngroups)
{
    if (!f || !ngroups) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *ngroups = (int)f->groups.size();
    return UCF_OK;
}

int ucf_field_group(const ucf_field* f, const ucf_plan* pl, int g, int* k0, int* nt_g, double* tD, int* sv, int* nr_g, double* rD,
                    int* col, double* tfac)
{
    if (!f || !pl) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    return field_group_out(f, pl->P, pl->D, g, k0, nt_g, tD, sv, nr_g, rD, col, tfac);
}

int ucf_field_group_from_params(const ucf_field* f, const ucf_params* P, int g, int* k0, int* nt_g, double* tD, int* sv, int* nr_g,
                                double* rD, int* col, double* tfac)
{
    if (!f || !P) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = validate(*P);
    if (rc) return rc;
    ucf_derived D;
    nondimensionalise(*P, D);
    return field_group_out(f, *P, D, g, k0, nt_g, tD, sv, nr_g, rD, col, tfac);
}

long long ucf_field_alloc_count(const ucf_field* f) { return f ? f->n_alloc : 0; }

int ucf_field_drawdown(ucf_field* f, ucf_plan* pl, int nz, const double* z, int dimensionless, double* s, double* ds, ucf_stats* stats)
{
    long long nout = 0;
    int rc = field_check_call(f, nz, (!z || !s || !ds) ? "NULL array" : nullptr, z, nout);
    if (rc) return rc;
    if (!pl) {
        // a plan cannot exist without a device: say that first where it is the reason
        rc = require_device();
        return rc ? rc : fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    }
    const int ng = (int)f->groups.size();
    std::vector<field_launch> L(ng);
    for (int g = 0; g < ng; g++)
        if ((rc = field_group_core(f, pl->P, pl->D, g, L[g]))) return rc;
    if ((rc = field_begin_launches(f, pl, stats, nullptr))) return rc;
    device_switch dg(pl->device);
    const size_t so = sizeof(double) * (size_t)nout;
    if ((rc = grow_buffer(f->b_s, so, "superposed drawdown", f->n_alloc)) || (rc = grow_buffer(f->b_ds, so, "superposed derivative", f->n_alloc))) return rc;
    rc = field_map_core(f, pl, L, nz, z, field_superpose_into(f, nz, dimensionless, (double*)f->b_s.p, (double*)f->b_ds.p), stats);
    if (rc) return rc;
    return copy_back({{s, f->b_s.p, so}, {ds, f->b_ds.p, so}}, plan_stream(pl), pl->device);
}

int ucf_field_forecast_sets(const ucf_params* base, int npar, const int* ids, const double* theta, double dlog, ucf_params* sets)
{
    if (!base || !theta || !sets) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = ucf_fit_perturb(base, npar, ids, theta, &sets[0]);      // the checks on npar and ids
    if (rc) return rc;
    char nb[32];
    for (int j = 0; j < npar; j++)
        if (!(theta[j] > 0.0) || !std::isfinite(theta[j]))
            return fail(UCF_ERR_BAD_ARGUMENT, "%s=%g must be positive and finite (sensitivities are taken in the logarithm of a parameter)",
                        fit_par_name(ids[j], nb, sizeof(nb)), theta[j]);
    if (!(dlog > 0.0) || !std::isfinite(dlog)) return fail(UCF_ERR_BAD_ARGUMENT, "dlog=%g must be positive and finite", dlog);
    rc = fit_theta_sets(*base, npar, ids, theta, dlog, 1 + 2 * npar, sets);
    if (rc) return rc;
    for (int k = 0; k <= 2 * npar; k++)
        if ((rc = validate(sets[k]))) return forecast_set_failed(rc, k, ids, dlog);
    return UCF_OK;
}

int ucf_field_forecast(ucf_field* f, ucf_plan* pl, int npar, const int* ids, const double* theta, double dlog, const double* cov, int nz,
                       const double* z, double* s, double* ds, double* sens, double* dsens, double* se, double* dse, double* s_all,
                       double* ds_all, long long* nbad, ucf_stats* stats)
{
    long long nout = 0;
    int rc = field_check_call(f, nz, !z ? "NULL z" : !s ? "NULL s" : !ds ? "NULL ds" : !ids ? "NULL ids" : !theta ? "NULL theta" : nullptr, z, nout);
    if (rc) return rc;
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!(dlog > 0.0) || !std::isfinite(dlog)) return fail(UCF_ERR_BAD_ARGUMENT, "dlog=%g must be positive and finite", dlog);
    if ((se || dse) && !cov) return fail(UCF_ERR_BAD_ARGUMENT, "%s is asked for without cov: a standard error needs the covariance", se ? "se" : "dse");
    if (cov && (rc = field_check_cov(npar, cov))) return rc;
    const int nset = 1 + 2 * npar;
    if (nset * nout > 0x7fffffffLL * 256)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d parameter sets x %d times x %d locations x %d depths: too many values for one buffer", nset, f->nt, f->nloc, nz);
    if (!pl) {
        rc = require_device();
        return rc ? rc : fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    }
    // the parameter sets and what every group launches under each of them: all of it before any launch
    forecast_work W;
    if ((rc = forecast_sets_of(f, pl, npar, ids, theta, dlog, W))) return rc;
    if ((rc = field_begin_launches(f, pl, stats, &W.sets[0]))) return rc;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    const size_t so = sizeof(double) * (size_t)nout, sa = so * nset, sj = so * npar;
    if ((rc = grow_buffer(f->b_nbad, sizeof(long long) * 2, "counts", f->n_alloc)) ||
        (sens && (rc = grow_buffer(f->b_sens, sj, "sensitivities", f->n_alloc))) || (dsens && (rc = grow_buffer(f->b_dsens, sj, "derivative sensitivities", f->n_alloc))) ||
        (se && (rc = grow_buffer(f->b_se, so, "standard error", f->n_alloc))) || (dse && (rc = grow_buffer(f->b_dse, so, "derivative standard error", f->n_alloc))) ||
        (cov && (rc = grow_buffer(f->b_cov, sizeof(double) * UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR, "cov", f->n_alloc)))) return rc;
    if ((rc = forecast_slots(f, npar, ids, dlog, W, nz, z, nout, stats))) return rc;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};
    if (hipMemsetAsync(f->b_nbad.p, 0, sizeof(long long) * 2, st) != hipSuccess ||
        (cov && hipMemcpyAsync(f->b_cov.p, cov, sizeof(double) * npar * npar, hipMemcpyHostToDevice, st) != hipSuccess))
        return fail(UCF_ERR_HIP, "upload of the forecast's arrays failed: %s", hipGetErrorString(hipGetLastError()));
    const double two_dlog = 2.0 * dlog;
    rc = ucf_field_launch_forecast(npar, nout, two_dlog, (const double*)f->b_sall.p, cov ? (const double*)f->b_cov.p : nullptr,
                                   sens ? (double*)f->b_sens.p : nullptr, se ? (double*)f->b_se.p : nullptr, (long long*)f->b_nbad.p, st);
    if (rc == UCF_OK)
        rc = ucf_field_launch_forecast(npar, nout, two_dlog, (const double*)f->b_dsall.p, cov ? (const double*)f->b_cov.p : nullptr,
                                       dsens ? (double*)f->b_dsens.p : nullptr, dse ? (double*)f->b_dse.p : nullptr, (long long*)f->b_nbad.p + 1, st);
    if (rc) return fail(rc, "forecast kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    // s, ds are slot 0 as it stands; everything else only where asked for
    return copy_back({{s, f->b_sall.p, so}, {ds, f->b_dsall.p, so}, {sens, f->b_sens.p, sj}, {dsens, f->b_dsens.p, sj}, {se, f->b_se.p, so},
                      {dse, f->b_dse.p, so}, {s_all, f->b_sall.p, sa}, {ds_all, f->b_dsall.p, sa}, {nbad, f->b_nbad.p, sizeof(long long) * 2}},
                     st, pl->device);
}

int ucf_worth_condition(int npar, const double* F, int nrow, const double* J, const double* w, double* F_out, double* cov_out)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (nrow < 0) return fail(UCF_ERR_BAD_ARGUMENT, "nrow=%d is negative", nrow);
    if (!F || !F_out || (nrow > 0 && (!J || !w))) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !F ? "F" : !F_out ? "F_out" : !J ? "J" : "w");
    int rc;
    if ((rc = field_check_finite("F", npar * npar, F))) return rc;
    if ((long long)nrow * npar > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "nrow=%d: too many rows", nrow);
    if ((rc = field_check_finite("J", nrow * npar, J)) || (rc = field_check_finite("w", nrow, w))) return rc;
    for (int r = 0; r < nrow; r++)
        if (w[r] < 0.0) return fail(UCF_ERR_BAD_ARGUMENT, "w[%d]=%g is negative", r, w[r]);
    const int n = npar;
    double B[UCF_FIT_MAX_PAR][UCF_FIT_MAX_PAR], d[UCF_FIT_MAX_PAR], X[UCF_FIT_MAX_PAR][UCF_FIT_MAX_PAR], g[UCF_FIT_MAX_PAR];
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) B[i][j] = (i == j) ? 1.0 : 0.0;
    for (int r = 0; r < nrow; r++) {
        worth_FtJ(n, F, J + (size_t)r * n, g);
        for (int j = 0; j < n; j++) g[j] = w[r] * g[j];
        for (int i = 0; i < n; i++)
            for (int j = 0; j <= i; j++) B[i][j] = B[i][j] + g[i] * g[j];
    }
    // B = L D L': l in the strict lower triangle of B
    for (int j = 0; j < n; j++) {
        double v = B[j][j];
        for (int k = 0; k < j; k++) v = v - (B[j][k] * B[j][k]) * d[k];
        d[j] = v;
        if (!(v > 0.0) || !std::isfinite(v)) return fail(UCF_ERR_SINGULAR, "d[%d]=%g of I + sum (w F'j)(w F'j)' is not positive and finite", j, v);
        for (int i = j + 1; i < n; i++) {
            double u = B[i][j];
            for (int k = 0; k < j; k++) u = u - (B[i][k] * B[j][k]) * d[k];
            B[i][j] = u / d[j];
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double x = F[i * n + j];
            for (int k = 0; k < j; k++) x = x - X[i][k] * B[j][k];
            X[i][j] = x;
        }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) F_out[i * n + j] = X[i][j] / std::sqrt(d[j]);
    if (cov_out)
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double acc = 0.0;
                for (int k = 0; k < n; k++) acc = acc + F_out[i * n + k] * F_out[j * n + k];
                cov_out[i * n + j] = acc;
            }
    return UCF_OK;
}

int ucf_field_worth(ucf_field* f, ucf_plan* pl, int npar, const int* ids, const double* theta, double dlog, const double* cov, int nz,
                    const double* z, double sigma_s, double sigma_d, const int* tsel, int ntgt, const int* tgt, const double* tw, int npick,
                    const int* cmask, double* prior, double* post, double* crit, int* nused, int* pick, double* cov_post, ucf_stats* stats)
{
    long long nout = 0;
    int rc = field_check_call(f, nz, !z ? "NULL z" : !ids ? "NULL ids" : !theta ? "NULL theta" : nullptr, z, nout);
    if (rc) return rc;
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!(dlog > 0.0) || !std::isfinite(dlog)) return fail(UCF_ERR_BAD_ARGUMENT, "dlog=%g must be positive and finite", dlog);
    if (!cov) return fail(UCF_ERR_BAD_ARGUMENT, "NULL cov: the worth of data is measured against the covariance of the fit");
    if ((rc = field_check_cov(npar, cov))) return rc;
    if (!(sigma_s > 0.0) || !std::isfinite(sigma_s)) return fail(UCF_ERR_BAD_ARGUMENT, "sigma_s=%g must be positive and finite", sigma_s);
    if (!(sigma_d >= 0.0) || !std::isfinite(sigma_d)) return fail(UCF_ERR_BAD_ARGUMENT, "sigma_d=%g must be finite and not negative (0: no derivative data)", sigma_d);
    if ((rc = worth_check_weights(ntgt, tw, f->nt, tsel))) return rc;
    if (!tgt) return fail(UCF_ERR_BAD_ARGUMENT, "NULL tgt");
    for (int t = 0; t < ntgt; t++) {
        const int* g = tgt + 4 * t;
        if (g[0] < 0 || g[0] > 1 || g[1] < 0 || g[1] >= f->nt || g[2] < 0 || g[2] >= f->nloc || g[3] < 0 || g[3] >= nz)
            return fail(UCF_ERR_BAD_ARGUMENT, "tgt[%d] = (kind %d, time %d, location %d, depth %d) outside (0..1, 0..%d, 0..%d, 0..%d)", t, g[0], g[1],
                        g[2], g[3], f->nt - 1, f->nloc - 1, nz - 1);
    }
    if (npick < 1 || npick > UCF_WORTH_MAX_PICK) return fail(UCF_ERR_BAD_ARGUMENT, "npick=%d outside 1..%d", npick, UCF_WORTH_MAX_PICK);
    const int nset = 1 + 2 * npar;
    if (nset * nout > 0x7fffffffLL * 256)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d parameter sets x %d times x %d locations x %d depths: too many values for one buffer", nset, f->nt, f->nloc, nz);
    if ((long long)f->nloc * nz > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "%d locations x %d depths: too many candidates for one call", f->nloc, nz);
    // cov = F F'
    double F[UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR];
    for (int i = 0; i < npar * npar; i++) F[i] = cov[i];
    if (fit_cholesky_factor(npar, F) != UCF_OK) return fail(UCF_ERR_SINGULAR, "cov is not positive definite (%d x %d): it has no Cholesky factor", npar, npar);
    for (int i = 0; i < npar; i++)
        for (int j = i + 1; j < npar; j++) F[i * npar + j] = 0.0;
    if (!pl) {
        rc = require_device();
        return rc ? rc : fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    }
    forecast_work W;
    if ((rc = forecast_sets_of(f, pl, npar, ids, theta, dlog, W))) return rc;
    if ((rc = field_begin_launches(f, pl, stats, &W.sets[0]))) return rc;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    const int nt = f->nt, ncand = f->nloc * nz, nfetch = std::max(ntgt, nt) * 2 * npar;
    const size_t nc = (size_t)ncand;
    // b_wsmall: F [MAX_PAR^2], A [MAX_TGT][MAX_PAR], tw [MAX_TGT]
    constexpr int OFF_A = UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR, OFF_TW = OFF_A + UCF_WORTH_MAX_TGT * UCF_FIT_MAX_PAR, NSMALL = OFF_TW + UCF_WORTH_MAX_TGT;
    if ((rc = grow_buffer(f->b_wpost, sizeof(double) * nc * ntgt, "posterior variances", f->n_alloc)) ||
        (rc = grow_buffer(f->b_wcrit, sizeof(double) * nc, "criterion", f->n_alloc)) || (rc = grow_buffer(f->b_wnused, sizeof(int) * nc, "data counts", f->n_alloc)) ||
        (rc = grow_buffer(f->b_wsmall, sizeof(double) * NSMALL, "factor and targets", f->n_alloc)) || (rc = grow_buffer(f->b_wtsel, sizeof(int) * nt, "time selection", f->n_alloc)) ||
        (rc = grow_buffer(f->b_widx, sizeof(long long) * nfetch, "gather indices", f->n_alloc)) || (rc = grow_buffer(f->b_wval, sizeof(double) * 2 * nfetch, "gathered values", f->n_alloc)))
        return rc;
    if ((rc = forecast_slots(f, npar, ids, dlog, W, nz, z, nout, stats))) return rc;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    const double two_dlog = 2.0 * dlog, ws = 1.0 / sigma_s, wd = sigma_d > 0.0 ? 1.0 / sigma_d : 0.0;
    std::vector<int> sel(nt, 1);
    for (int k = 0; tsel && k < nt; k++) sel[k] = tsel[k] != 0;
    double small[NSMALL] = {};
    for (int t = 0; t < ntgt; t++) small[OFF_TW + t] = tw ? tw[t] : 1.0;
    drain drained{st};                     // sel and small outlive their copies
    if (hipMemcpyAsync(f->b_wtsel.p, sel.data(), sizeof(int) * nt, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the time selection failed: %s", hipGetErrorString(hipGetLastError()));
    // the targets' sensitivities, once
    std::vector<long long> e((size_t)std::max(ntgt, nt));
    std::vector<double> hs((size_t)nfetch), hd((size_t)nfetch);
    for (int t = 0; t < ntgt; t++) e[t] = ((long long)tgt[4 * t + 1] * f->nloc + tgt[4 * t + 2]) * nz + tgt[4 * t + 3];
    if ((rc = worth_fetch(f, st, pl->device, npar, nout, ntgt, e.data(), hs.data(), hd.data()))) return rc;
    double Jt[UCF_WORTH_MAX_TGT][UCF_FIT_MAX_PAR];
    bool tgt_ok[UCF_WORTH_MAX_TGT];
    for (int t = 0; t < ntgt; t++) tgt_ok[t] = worth_J(npar, (tgt[4 * t] ? hd.data() : hs.data()) + (size_t)t * 2 * npar, two_dlog, Jt[t]);
    // what the rounds that do not run leave behind
    const double nan = std::nan("");
    if (prior) std::fill(prior, prior + (size_t)npick * ntgt, nan);
    if (post) std::fill(post, post + (size_t)npick * ntgt * nc, nan);
    if (crit) std::fill(crit, crit + (size_t)npick * nc, nan);
    if (pick) std::fill(pick, pick + npick, -1);
    std::vector<double> hcrit(nc), rows, wrow;
    std::vector<char> taken(nc, 0);
    for (int r = 0; r < npick; r++) {
        for (int t = 0; t < ntgt; t++) {
            double* A = small + OFF_A + t * npar;
            worth_FtJ(npar, F, Jt[t], A);
            double p = 0.0;
            for (int j = 0; j < npar; j++) {
                if (!tgt_ok[t]) A[j] = nan;
                p = p + A[j] * A[j];
            }
            if (prior) prior[(size_t)r * ntgt + t] = p;
        }
        for (int i = 0; i < npar * npar; i++) small[i] = F[i];
        if (hipMemcpyAsync(f->b_wsmall.p, small, sizeof(small), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(UCF_ERR_HIP, "upload of the factor and the targets failed: %s", hipGetErrorString(hipGetLastError()));
        const double* d_small = (const double*)f->b_wsmall.p;
        rc = ucf_field_launch_worth(npar, nt, ncand, (const double*)f->b_sall.p, (const double*)f->b_dsall.p, two_dlog, d_small, ws, wd,
                                    (const int*)f->b_wtsel.p, ntgt, d_small + OFF_A, d_small + OFF_TW, (double*)f->b_wpost.p, (double*)f->b_wcrit.p,
                                    (int*)f->b_wnused.p, st);
        if (rc) return fail(rc, "worth kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        if ((rc = copy_back({{post ? post + (size_t)r * ntgt * nc : nullptr, f->b_wpost.p, sizeof(double) * nc * ntgt}, {hcrit.data(), f->b_wcrit.p, sizeof(double) * nc},
                             {r == 0 ? nused : nullptr, f->b_wnused.p, sizeof(int) * nc}}, st, pl->device))) return rc;
        if (crit) std::copy(hcrit.begin(), hcrit.end(), crit + (size_t)r * nc);
        // the allowed, unpicked candidate of least finite crit; the lowest index on a tie
        int best = -1;
        for (int c = 0; c < ncand; c++)
            if ((!cmask || cmask[c] != 0) && !taken[c] && std::isfinite(hcrit[c]) && (best < 0 || hcrit[c] < hcrit[best])) best = c;
        if (best < 0) break;
        if (pick) pick[r] = best;
        taken[best] = 1;
        if (r + 1 == npick && !cov_post) break;
        // the used data of the picked candidate in kernel order, and the factor after them
        int ne = 0;
        for (int k = 0; k < nt; k++)
            if (sel[k]) e[ne++] = (long long)k * ncand + best;
        if ((rc = worth_fetch(f, st, pl->device, npar, nout, ne, e.data(), hs.data(), hd.data()))) return rc;
        rows.clear(); wrow.clear();
        double J[UCF_FIT_MAX_PAR];
        for (int q = 0; q < ne; q++)
            for (int kind = 0; kind < 2; kind++) {
                const double wk = kind ? wd : ws;
                if (!(wk > 0.0) || !worth_J(npar, (kind ? hd.data() : hs.data()) + (size_t)q * 2 * npar, two_dlog, J)) continue;
                rows.insert(rows.end(), J, J + npar);
                wrow.push_back(wk);
            }
        if ((rc = ucf_worth_condition(npar, F, (int)wrow.size(), rows.data(), wrow.data(), F, nullptr))) return rc;
    }
    if (cov_post) {
        double same[UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR];
        if ((rc = ucf_worth_condition(npar, F, 0, nullptr, nullptr, same, cov_post))) return rc;
    }
    return UCF_OK;
}

int ucf_debug_field_worth(int npar, int nt, int ncand, const double* a_s, const double* a_d, double two_dlog, const double* F, double ws,
                          double wd, const int* tsel, int ntgt, const double* A, const double* tw, double* post, double* crit, int* nused)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (nt < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nt=%d: at least one time", nt);
    if (ncand < 1) return fail(UCF_ERR_BAD_ARGUMENT, "ncand=%d: at least one candidate", ncand);
    const long long nval = (long long)(1 + 2 * npar) * nt * ncand;
    if (nval > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "%d slots x %d times x %d candidates: more than 2^31-1 values", 1 + 2 * npar, nt, ncand);
    if (!a_s || !F || !A) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !a_s ? "a_s" : !F ? "F" : "A");
    if (!(two_dlog > 0.0) || !std::isfinite(two_dlog)) return fail(UCF_ERR_BAD_ARGUMENT, "two_dlog=%g must be positive and finite", two_dlog);
    int rc = field_check_finite("F", npar * npar, F);
    if (rc) return rc;
    if (!(ws > 0.0) || !std::isfinite(ws)) return fail(UCF_ERR_BAD_ARGUMENT, "ws=%g must be positive and finite", ws);
    if (!(wd >= 0.0) || !std::isfinite(wd)) return fail(UCF_ERR_BAD_ARGUMENT, "wd=%g must be finite and not negative (0: no derivative data)", wd);
    if (wd > 0.0 && !a_d) return fail(UCF_ERR_BAD_ARGUMENT, "NULL a_d with wd=%g", wd);
    if ((rc = worth_check_weights(ntgt, tw, nt, tsel))) return rc;
    if ((rc = require_device())) return rc;
    const size_t sa = sizeof(double) * (size_t)nval, nc = (size_t)ncand;
    std::vector<int> sel(nt, 1);
    for (int k = 0; tsel && k < nt; k++) sel[k] = tsel[k] != 0;
    double w1[UCF_WORTH_MAX_TGT];
    for (int t = 0; t < ntgt; t++) w1[t] = tw ? tw[t] : 1.0;
    dev_buf b_as, b_ad, b_F, b_sel, b_A, b_tw, b_post, b_crit, b_nused;
    if (b_as.alloc(sa) || (wd > 0.0 && b_ad.alloc(sa)) || b_F.alloc(sizeof(double) * npar * npar) || b_sel.alloc(sizeof(int) * nt) ||
        b_A.alloc(sizeof(double) * ntgt * npar) || b_tw.alloc(sizeof(double) * ntgt) || b_post.alloc(sizeof(double) * nc * ntgt) ||
        b_crit.alloc(sizeof(double) * nc) || b_nused.alloc(sizeof(int) * nc))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_as.p, a_s, sa, hipMemcpyHostToDevice));
    if (wd > 0.0) HIP_TRY(hipMemcpy(b_ad.p, a_d, sa, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_F.p, F, sizeof(double) * npar * npar, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_sel.p, sel.data(), sizeof(int) * nt, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_A.p, A, sizeof(double) * ntgt * npar, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_tw.p, w1, sizeof(double) * ntgt, hipMemcpyHostToDevice));
    rc = ucf_field_launch_worth(npar, nt, ncand, (const double*)b_as.p, (const double*)b_ad.p, two_dlog, (const double*)b_F.p, ws, wd,
                                (const int*)b_sel.p, ntgt, (const double*)b_A.p, (const double*)b_tw.p, (double*)b_post.p, (double*)b_crit.p,
                                (int*)b_nused.p, nullptr);
    if (rc) return fail(rc, "worth kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{post, b_post.p, sizeof(double) * nc * ntgt}, {crit, b_crit.p, sizeof(double) * nc}, {nused, b_nused.p, sizeof(int) * nc}});
}

// What ucf_field_ensemble, ucf_field_ensemble_weighted and ucf_field_yield share on their members, in the order of their checks
struct ensemble_members {
    std::vector<ucf_params> sets;          // member m = ucf_fit_perturb(plan, thetas[m])
    std::vector<unsigned long long> u;     // the integer weights; empty: unweighted
    int first = 0, nrun = 0;               // the first member that is launched, and how many are
};

static int ensemble_check_thetas(int npar, const int* ids, int nens, const double* thetas)
{
    char nb[32];
    for (int m = 0; m < nens; m++)
        for (int j = 0; j < npar; j++) {
            const double v = thetas[(size_t)m * npar + j];
            if (!(v > 0.0) || !std::isfinite(v))
                return fail(UCF_ERR_BAD_ARGUMENT, "member %d: %s=%g must be positive and finite", m, fit_par_name(ids[j], nb, sizeof(nb)), v);
        }
    return UCF_OK;
}

// the weights quantised (weighted == false: every member runs, nothing is written); u_out, ess, nlaunched: NULL ok
static int ensemble_weights_of(int nens, const double* weight, bool weighted, unsigned long long* u_out, double* ess, int* nlaunched,
                               ensemble_members& E)
{
    E.first = 0;
    E.nrun = nens;
    if (!weighted) return UCF_OK;
    E.u.resize(nens);
    double e = 0.0;
    int rc = ucf_ensemble_quantise(nens, weight, E.u.data(), &e);
    if (rc) return rc;
    E.nrun = 0;
    for (int m = nens - 1; m >= 0; m--)
        if (E.u[m] != 0) { E.first = m; E.nrun++; }
    if (u_out) std::copy(E.u.begin(), E.u.end(), u_out);
    if (ess) *ess = e;
    if (nlaunched) *nlaunched = E.nrun;
    return UCF_OK;
}

// a plan there must be; then every member and what every group launches under it: checked before any launch, the arrays not kept
static int ensemble_sets_of(const ucf_field* f, const ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, ensemble_members& E)
{
    int rc;
    if (!pl) {
        rc = require_device();
        return rc ? rc : fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    }
    E.sets.resize(nens);
    std::vector<field_launch> L;
    for (int m = 0; m < nens; m++) {
        const double* theta = thetas + (size_t)m * npar;
        if ((rc = ucf_fit_perturb(&pl->P, npar, ids, theta, &E.sets[m]))) return m == 0 ? rc : ensemble_member_failed(rc, m, npar, ids, theta);
        if ((rc = validate(E.sets[m])) || (rc = field_launches_of(f, E.sets[m], L))) return ensemble_member_failed(rc, m, npar, ids, theta);
    }
    return UCF_OK;
}

// What ucf_field_ensemble_times asks of field_ensemble_core beyond an ensemble: the abscissa (tau NULL: the field's t), the
// limits on the drawdown and their kinds
struct times_request {
    const double* tau;
    double tau_never;
    int nlim;
    const double *limit;
    const int* kind;
};

// what ucf_field_ensemble_times and ucf_debug_field_times check on the abscissa, the limits and the kinds
static int times_check(int nt, const double* tau, double tau_never, int nlim, const double* limit, const int* kind)
{
    if (nlim < 1 || nlim > UCF_ENSEMBLE_MAX_Q) return fail(UCF_ERR_BAD_ARGUMENT, "nlim=%d outside 1..%d", nlim, UCF_ENSEMBLE_MAX_Q);
    if (!limit || !kind) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !limit ? "limit" : "kind");
    int rc = field_check_finite("limit", nlim, limit);
    if (rc) return rc;
    for (int l = 0; l < nlim; l++)
        if (kind[l] != UCF_TIME_FIRST_ABOVE && kind[l] != UCF_TIME_LAST_ABOVE)
            return fail(UCF_ERR_BAD_ARGUMENT, "kind[%d]=%d is neither UCF_TIME_FIRST_ABOVE (0) nor UCF_TIME_LAST_ABOVE (1)", l, kind[l]);
    if ((rc = field_check_finite("tau", nt, tau))) return rc;
    for (int k = 1; k < nt; k++)
        if (!(tau[k] > tau[k - 1]))
            return fail(UCF_ERR_BAD_ARGUMENT, "tau[%d]=%g does not lie after tau[%d]=%g: the abscissa must increase strictly", k, tau[k], k - 1, tau[k - 1]);
    if (!std::isfinite(tau_never) || !(tau_never > tau[nt - 1]))
        return fail(UCF_ERR_BAD_ARGUMENT, "tau_never=%g must be finite and lie after tau[%d]=%g", tau_never, nt - 1, tau[nt - 1]);
    return UCF_OK;
}

// ucf_field_ensemble (weighted == false: weight, u_out, ess, nlaunched are not read) and ucf_field_ensemble_weighted: one
// sequence.  The weighted call differs in three places: the weights are quantised among the checks; a member with u = 0 is
// validated but not launched, and its slots are filled with NaN bytes; the reduction runs with the weights.
// ucf_field_ensemble_times (tr not NULL) is the same sequence with field_times_kernel between the members and the reduction:
// the reduction then runs once, on T [nens][nlim nsite] in b_tall; s takes the maps of T, ds is NULL, nlim / limit are the
// horizons (named so in the messages) and pexc is plater.
static int field_ensemble_core(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, int nz, const double* z,
                               int nq, const double* q, int nlim, const double* limit, const ucf_ensemble_maps* s, const ucf_ensemble_maps* ds,
                               double* pexc, long long* nbad, ucf_stats* stats, bool weighted, const double* weight,
                               unsigned long long* u_out, double* ess, int* nlaunched, const times_request* tr = nullptr)
{
    long long nout = 0;
    int rc = field_check_call(f, nz, !z ? "NULL z" : !ids ? "NULL ids" : !thetas ? "NULL thetas" : nullptr, z, nout);
    if (rc) return rc;
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if ((rc = ensemble_check_levels(nens, nq, q, nlim, limit, (s && s->quant) || (ds && ds->quant), !tr && pexc != nullptr, tr ? "nhor" : "nlim",
                                    tr ? "horizon" : "limit"))) return rc;
    if ((rc = ensemble_check_thetas(npar, ids, nens, thetas))) return rc;
    if (nens * nout > 0x7fffffffLL * 256)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d times x %d locations x %d depths: too many values for one buffer", nens, f->nt, f->nloc, nz);
    // what the reduction works on: the nout outputs of a map, or the times of nlim limits at the nsite = nloc nz sites
    const long long nsite = nout / f->nt, nred = tr ? tr->nlim * nsite : nout;
    const double* tau = tr && tr->tau ? tr->tau : f->t.data();
    if (tr) {
        if (!s) return fail(UCF_ERR_BAD_ARGUMENT, "NULL T");
        if (pexc && nlim == 0) return fail(UCF_ERR_BAD_ARGUMENT, "plater is asked for with nhor=0: no horizon to lie beyond");
        if ((rc = times_check(f->nt, tau, tr->tau_never, tr->nlim, tr->limit, tr->kind))) return rc;
        if (nens * nred > 0x7fffffffLL * 256)
            return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d limits x %d locations x %d depths: too many values for one buffer", nens, tr->nlim, f->nloc, nz);
    }
    ensemble_members E;
    if ((rc = ensemble_weights_of(nens, weighted ? weight : nullptr, weighted, u_out, ess, nlaunched, E)) ||
        (rc = ensemble_sets_of(f, pl, npar, ids, nens, thetas, E))) return rc;
    std::vector<ucf_params>& sets = E.sets;
    std::vector<unsigned long long>& u = E.u;
    std::vector<field_launch> L;
    auto failed = [&](int rc_m, int m) { return ensemble_member_failed(rc_m, m, npar, ids, thetas + (size_t)m * npar); };
    if ((rc = field_begin_launches(f, pl, stats, &sets[E.first]))) return rc;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    // b_ens: q [MAX_Q], limit [MAX_Q], then per map what is asked for of mean, sd, min, max [nout], quant [nq][nout], nfin
    // [nout] (ints, padded to whole doubles), then pexc [nlim][nout]; for the times nout = nlim nsite, and behind pexc tau [nt],
    // the limits [nlim] and the kinds [nlim] (ints, padded)
    const size_t no = (size_t)nred, so = sizeof(double) * no, sa = sizeof(double) * (size_t)nout * nens;
    const ucf_ensemble_maps none = {};
    const ucf_ensemble_maps* want[2] = {s ? s : &none, ds ? ds : &none};
    struct map_at { double *mean, *sd, *min, *max, *quant; int* nfin; } at[2];
    size_t used = 2 * UCF_ENSEMBLE_MAX_Q;                 // in doubles
    auto take = [&](bool asked, size_t n) { const size_t o = used; if (asked) used += n; return asked ? o : (size_t)-1; };
    size_t off[2][6], off_pexc;
    for (int i = 0; i < 2; i++) {
        off[i][0] = take(want[i]->mean, no); off[i][1] = take(want[i]->sd, no); off[i][2] = take(want[i]->min, no);
        off[i][3] = take(want[i]->max, no); off[i][4] = take(want[i]->quant, no * nq); off[i][5] = take(want[i]->nfin, (no + 1) / 2);
    }
    off_pexc = take(pexc, no * nlim);
    const size_t off_tau = take(tr != nullptr, f->nt), off_tlim = take(tr != nullptr, tr ? tr->nlim : 0), off_kind = take(tr != nullptr, tr ? (tr->nlim + 1) / 2 : 0);
    if ((rc = grow_buffer(f->b_sall, sa, "drawdown of every member", f->n_alloc)) || (rc = grow_buffer(f->b_dsall, sa, "derivative of every member", f->n_alloc)) ||
        (rc = grow_buffer(f->b_nbad, sizeof(long long) * 2, "counts", f->n_alloc)) ||
        (rc = grow_buffer(f->b_ens, sizeof(double) * used, "ensemble statistics", f->n_alloc)) ||
        (weighted && (rc = grow_buffer(f->b_u, sizeof(unsigned long long) * nens, "ensemble weights", f->n_alloc))) ||
        (tr && (rc = grow_buffer(f->b_tall, so * nens, "times of every member", f->n_alloc)))) return rc;
    double* base = (double*)f->b_ens.p;
    auto dev = [&](size_t o) { return o == (size_t)-1 ? nullptr : base + o; };
    for (int i = 0; i < 2; i++) at[i] = map_at{dev(off[i][0]), dev(off[i][1]), dev(off[i][2]), dev(off[i][3]), dev(off[i][4]), (int*)dev(off[i][5])};
    double* d_pexc = dev(off_pexc);
    rc = field_map_sets(f, nens, sets.data(), [&](int m, const std::vector<field_launch>*& Lm) { Lm = &L; return field_launches_of(f, sets[m], L); },
                        nz, z, field_slot_superpose(f, nz, nout), stats, failed, weighted ? u.data() : nullptr);
    if (rc) return rc;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};
    double ql[2 * UCF_ENSEMBLE_MAX_Q];
    ensemble_pack_levels(nq, q, nlim, limit, ql);
    if (hipMemsetAsync(f->b_nbad.p, 0, sizeof(long long) * 2, st) != hipSuccess ||
        hipMemcpyAsync(base, ql, sizeof(ql), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the ensemble's arrays failed: %s", hipGetErrorString(hipGetLastError()));
    const size_t sm = sizeof(double) * (size_t)nout;      // a member's slot
    const double* slots[2] = {(const double*)f->b_sall.p, (const double*)f->b_dsall.p};
    if (weighted) {
        // the weights, and NaN bytes into the slots of the members that were not launched, so that `all` is defined
        bool ok = hipMemcpyAsync(f->b_u.p, u.data(), sizeof(unsigned long long) * nens, hipMemcpyHostToDevice, st) == hipSuccess;
        for (int m = 0; m < nens && ok; m++)
            if (u[m] == 0)
                ok = hipMemsetAsync((double*)f->b_sall.p + (size_t)m * nout, 0xff, sm, st) == hipSuccess &&
                     hipMemsetAsync((double*)f->b_dsall.p + (size_t)m * nout, 0xff, sm, st) == hipSuccess;
        if (!ok) return fail(UCF_ERR_HIP, "upload of the ensemble's weights failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (tr) {
        // the s slots become times: T [nens][nlim][nsite], the only map that is reduced
        if (hipMemcpyAsync(dev(off_tau), tau, sizeof(double) * f->nt, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(dev(off_tlim), tr->limit, sizeof(double) * tr->nlim, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(dev(off_kind), tr->kind, sizeof(int) * tr->nlim, hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(UCF_ERR_HIP, "upload of the abscissa, limits and kinds failed: %s", hipGetErrorString(hipGetLastError()));
        ucf_times_args ta = {};
        ta.nens = nens; ta.nt = f->nt; ta.nsite = nsite; ta.d_a = slots[0]; ta.d_tau = dev(off_tau); ta.tau_never = tr->tau_never;
        ta.nlim = tr->nlim; ta.d_limit = dev(off_tlim); ta.d_kind = (const int*)dev(off_kind); ta.d_T = (double*)f->b_tall.p;
        if ((rc = ucf_field_launch_times(&ta, st))) return fail(rc, "times kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        slots[0] = (const double*)f->b_tall.p;
        slots[1] = nullptr;
    }
    const int nmap = tr ? 1 : 2;
    for (int i = 0; i < nmap && rc == UCF_OK; i++) {
        ucf_ensemble_reduce_args ra = {};
        ra.nens = nens; ra.nout = nred; ra.d_a = slots[i];
        ra.d_u = weighted ? (const unsigned long long*)f->b_u.p : nullptr;
        ra.nq = nq; ra.d_q = base; ra.nlim = nlim; ra.d_limit = base + UCF_ENSEMBLE_MAX_Q;
        ra.d_mean = at[i].mean; ra.d_sd = at[i].sd; ra.d_min = at[i].min; ra.d_max = at[i].max; ra.d_nfin = at[i].nfin;
        ra.d_quant = at[i].quant; ra.d_pexc = i == 0 ? d_pexc : nullptr; ra.d_nbad = (long long*)f->b_nbad.p + i;
        rc = ucf_field_launch_ensemble_reduce(&ra, st);
    }
    if (rc) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    // only what is asked for crosses the bus
    std::vector<device_copy> back = {{pexc, d_pexc, so * nlim}, {nbad, f->b_nbad.p, sizeof(long long) * nmap}};
    for (int i = 0; i < nmap; i++) {
        const ucf_ensemble_maps* w = want[i];
        back.insert(back.end(), {{w->mean, at[i].mean, so}, {w->sd, at[i].sd, so}, {w->min, at[i].min, so}, {w->max, at[i].max, so},
                                 {w->quant, at[i].quant, so * nq}, {w->all, slots[i], so * nens}, {w->nfin, at[i].nfin, sizeof(int) * no}});
    }
    return copy_back(back, st, pl->device);
}

int ucf_field_ensemble(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, int nz, const double* z,
                       int nq, const double* q, int nlim, const double* limit, const ucf_ensemble_maps* s, const ucf_ensemble_maps* ds,
                       double* pexc, long long* nbad, ucf_stats* stats)
{
    return field_ensemble_core(f, pl, npar, ids, nens, thetas, nz, z, nq, q, nlim, limit, s, ds, pexc, nbad, stats, false, nullptr, nullptr,
                               nullptr, nullptr);
}

int ucf_field_ensemble_weighted(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, const double* weight,
                                int nz, const double* z, int nq, const double* q, int nlim, const double* limit, const ucf_ensemble_maps* s,
                                const ucf_ensemble_maps* ds, double* pexc, long long* nbad, ucf_stats* stats, unsigned long long* u, double* ess,
                                int* nlaunched)
{
    return field_ensemble_core(f, pl, npar, ids, nens, thetas, nz, z, nq, q, nlim, limit, s, ds, pexc, nbad, stats, true, weight, u, ess,
                               nlaunched);
}

int ucf_field_ensemble_times(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, const double* weight,
                             int nz, const double* z, const double* tau, double tau_never, int nlim, const double* limit, const int* kind,
                             int nq, const double* q, int nhor, const double* horizon, const ucf_ensemble_maps* T, double* plater,
                             long long* nbad, ucf_stats* stats, unsigned long long* u, double* ess, int* nlaunched)
{
    const times_request tr = {tau, tau_never, nlim, limit, kind};
    return field_ensemble_core(f, pl, npar, ids, nens, thetas, nz, z, nq, q, nhor, horizon, T, nullptr, plater, nbad, stats, weight != nullptr,
                               weight, u, ess, nlaunched, &tr);
}

int ucf_debug_field_times(int nens, int nt, long long nsite, const double* a, const double* tau, double tau_never, int nlim,
                          const double* limit, const int* kind, double* T)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (nt < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nt=%d: at least one time", nt);
    if (nsite < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nsite=%lld: at least one site", nsite);
    if (!a || !tau || !T) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !a ? "a" : !tau ? "tau" : "T");
    int rc = times_check(nt, tau, tau_never, nlim, limit, kind);
    if (rc) return rc;
    if (nens * nsite > 0x7fffffffLL / (nt > nlim ? nt : nlim))
        return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d times or %d limits x %lld sites: more than 2^31-1 values", nens, nt, nlim, nsite);
    if ((rc = require_device())) return rc;
    const size_t sa = sizeof(double) * nens * nt * (size_t)nsite, sT = sizeof(double) * nens * nlim * (size_t)nsite;
    dev_buf b_a, b_tau, b_lim, b_kind, b_T;
    if (b_a.alloc(sa) || b_tau.alloc(sizeof(double) * nt) || b_lim.alloc(sizeof(double) * nlim) || b_kind.alloc(sizeof(int) * nlim) || b_T.alloc(sT))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_a.p, a, sa, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_tau.p, tau, sizeof(double) * nt, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_lim.p, limit, sizeof(double) * nlim, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_kind.p, kind, sizeof(int) * nlim, hipMemcpyHostToDevice));
    ucf_times_args ta = {};
    ta.nens = nens; ta.nt = nt; ta.nsite = nsite; ta.d_a = (const double*)b_a.p; ta.d_tau = (const double*)b_tau.p; ta.tau_never = tau_never;
    ta.nlim = nlim; ta.d_limit = (const double*)b_lim.p; ta.d_kind = (const int*)b_kind.p; ta.d_T = (double*)b_T.p;
    if ((rc = ucf_field_launch_times(&ta, nullptr))) return fail(rc, "times kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{T, ta.d_T, sT}});
}

// what ucf_sobol_design, ucf_field_sobol and ucf_debug_sobol check on the size of a design
static int sobol_check_size(int npar, int nbase)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (nbase < 2 || nbase > UCF_SOBOL_MAX_BASE) return fail(UCF_ERR_BAD_ARGUMENT, "nbase=%d outside 2..%d", nbase, UCF_SOBOL_MAX_BASE);
    return UCF_OK;
}

// thetas [(npar + 2) nbase][npar] has the structure of ucf_sobol_design, bit for bit
static int sobol_check_structure(int npar, int nbase, const double* thetas)
{
    const size_t N = (size_t)nbase;
    for (int j = 0; j < npar; j++)
        for (int r = 0; r < nbase; r++)
            for (int k = 0; k < npar; k++) {
                const double got = thetas[((2 + j) * N + r) * npar + k], want = thetas[((k == j ? N : 0) + r) * npar + k];
                if (std::memcmp(&got, &want, sizeof(double)) != 0)
                    return fail(UCF_ERR_BAD_ARGUMENT, "thetas is not a Saltelli design: block %d, row %d, parameter %d is %.17g, but %s[%d][%d] is %.17g",
                                2 + j, r, k, got, k == j ? "B" : "A", r, k, want);
            }
    return UCF_OK;
}

// the maps of one ucf_sobol_maps in the order of their staging: four [npar][nout], two [nout], then nrow
static std::array<double*, 6> sobol_doubles(const ucf_sobol_maps& w) { return {{w.S, w.ST, w.seS, w.seST, w.mean, w.var}}; }

int ucf_sobol_design(int npar, int nbase, const double* draws, double* thetas)
{
    int rc = sobol_check_size(npar, nbase);
    if (rc) return rc;
    if (!draws || !thetas) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !draws ? "draws" : "thetas");
    for (int r = 0; r < 2 * nbase; r++)
        for (int k = 0; k < npar; k++) {
            const double v = draws[(size_t)r * npar + k];
            if (!(v > 0.0) || !std::isfinite(v))
                return fail(UCF_ERR_BAD_ARGUMENT, "draws[%d][%d]=%g: row %d, parameter %d must be positive and finite", r, k, v, r, k);
        }
    const size_t N = (size_t)nbase;
    std::copy(draws, draws + 2 * N * npar, thetas);
    for (int j = 0; j < npar; j++)
        for (size_t r = 0; r < N; r++)
            for (int k = 0; k < npar; k++) thetas[((2 + j) * N + r) * npar + k] = draws[((k == j ? N : 0) + r) * npar + k];
    return UCF_OK;
}

// The members run as those of ucf_field_ensemble run (field_map_sets into the slots of field_slot_superpose); what differs is
// their number, the check of the design and the reduction.
int ucf_field_sobol(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nbase, const double* thetas, int nz, const double* z,
                    const ucf_sobol_maps* s, const ucf_sobol_maps* ds, long long* nbad, ucf_stats* stats)
{
    long long nout = 0;
    int rc = field_check_call(f, nz, !z ? "NULL z" : !ids ? "NULL ids" : !thetas ? "NULL thetas" : nullptr, z, nout);
    if (rc) return rc;
    if ((rc = sobol_check_size(npar, nbase))) return rc;
    const int nmem = (npar + 2) * nbase;
    if ((rc = ensemble_check_thetas(npar, ids, nmem, thetas)) || (rc = sobol_check_structure(npar, nbase, thetas))) return rc;
    if (nmem * nout > 0x7fffffffLL * 256)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d times x %d locations x %d depths: too many values for one buffer", nmem, f->nt, f->nloc, nz);
    ensemble_members E;
    if ((rc = ensemble_weights_of(nmem, nullptr, false, nullptr, nullptr, nullptr, E)) ||
        (rc = ensemble_sets_of(f, pl, npar, ids, nmem, thetas, E))) return rc;
    std::vector<ucf_params>& sets = E.sets;
    std::vector<field_launch> L;
    auto failed = [&](int rc_m, int m) { return ensemble_member_failed(rc_m, m, npar, ids, thetas + (size_t)m * npar); };
    if ((rc = field_begin_launches(f, pl, stats, &sets[0]))) return rc;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    // b_sob: per map what is asked for of S, ST, seS, seST [npar][nout], mean, var [nout], nrow [nout] (ints, padded to whole doubles)
    const size_t no = (size_t)nout, so = sizeof(double) * no, sa = so * nmem;
    const ucf_sobol_maps none = {};
    const ucf_sobol_maps* want[2] = {s ? s : &none, ds ? ds : &none};
    size_t used = 0, off[2][7];                          // in doubles
    for (int i = 0; i < 2; i++) {
        const std::array<double*, 6> w = sobol_doubles(*want[i]);
        for (int v = 0; v < 7; v++) {
            const bool asked = v < 6 ? w[v] != nullptr : want[i]->nrow != nullptr;
            off[i][v] = asked ? used : (size_t)-1;
            if (asked) used += v < 4 ? no * npar : v < 6 ? no : (no + 1) / 2;
        }
    }
    if ((rc = grow_buffer(f->b_sall, sa, "drawdown of every member", f->n_alloc)) || (rc = grow_buffer(f->b_dsall, sa, "derivative of every member", f->n_alloc)) ||
        (rc = grow_buffer(f->b_nbad, sizeof(long long) * 2, "counts", f->n_alloc)) ||
        (used && (rc = grow_buffer(f->b_sob, sizeof(double) * used, "Sobol statistics", f->n_alloc)))) return rc;
    double* base = (double*)f->b_sob.p;
    auto dev = [&](size_t o) { return o == (size_t)-1 ? nullptr : base + o; };
    rc = field_map_sets(f, nmem, sets.data(), [&](int m, const std::vector<field_launch>*& Lm) { Lm = &L; return field_launches_of(f, sets[m], L); },
                        nz, z, field_slot_superpose(f, nz, nout), stats, failed);
    if (rc) return rc;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};
    if (hipMemsetAsync(f->b_nbad.p, 0, sizeof(long long) * 2, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
    const double* slots[2] = {(const double*)f->b_sall.p, (const double*)f->b_dsall.p};
    for (int i = 0; i < 2 && rc == UCF_OK; i++) {
        ucf_sobol_args ka = {};
        ka.npar = npar; ka.nbase = nbase; ka.nout = nout; ka.d_a = slots[i];
        ka.d_S = dev(off[i][0]); ka.d_ST = dev(off[i][1]); ka.d_seS = dev(off[i][2]); ka.d_seST = dev(off[i][3]);
        ka.d_mean = dev(off[i][4]); ka.d_var = dev(off[i][5]); ka.d_nrow = (int*)dev(off[i][6]); ka.d_nbad = (long long*)f->b_nbad.p + i;
        rc = ucf_field_launch_sobol(&ka, st);
    }
    if (rc) return fail(rc, "Sobol kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    // only what is asked for crosses the bus
    std::vector<device_copy> back = {{nbad, f->b_nbad.p, sizeof(long long) * 2}};
    for (int i = 0; i < 2; i++) {
        const std::array<double*, 6> w = sobol_doubles(*want[i]);
        for (int v = 0; v < 6; v++) back.push_back({w[v], dev(off[i][v]), v < 4 ? so * npar : so});
        back.push_back({want[i]->nrow, dev(off[i][6]), sizeof(int) * no});
        back.push_back({want[i]->all, slots[i], sa});
    }
    return copy_back(back, st, pl->device);
}

int ucf_debug_sobol(int npar, int nbase, long long nout, const double* a, const ucf_sobol_maps* out, long long* nbad)
{
    int rc = sobol_check_size(npar, nbase);
    if (rc) return rc;
    const long long nmem = (long long)(npar + 2) * nbase;
    if (nout < 1 || nout > 0x7fffffffLL * 256 / nmem)
        return fail(UCF_ERR_BAD_ARGUMENT, "nout=%lld: at least one output, at most 2^39 values in %lld members", nout, nmem);
    if (!a) return fail(UCF_ERR_BAD_ARGUMENT, "NULL a");
    if ((rc = require_device())) return rc;
    const ucf_sobol_maps none = {};
    const std::array<double*, 6> w = sobol_doubles(out ? *out : none);
    int* nrow = out ? out->nrow : nullptr;
    const size_t no = (size_t)nout, so = sizeof(double) * no, sa = so * (size_t)nmem;
    dev_buf b_a, b_w[6], b_nrow, b_nbad;
    bool short_of = b_a.alloc(sa) || b_nbad.alloc(sizeof(long long)) || (nrow && b_nrow.alloc(sizeof(int) * no));
    for (int v = 0; v < 6 && !short_of; v++) short_of = w[v] && b_w[v].alloc(v < 4 ? so * npar : so);
    if (short_of) return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_a.p, a, sa, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_nbad.p, 0, sizeof(long long)));
    ucf_sobol_args ka = {};
    ka.npar = npar; ka.nbase = nbase; ka.nout = nout; ka.d_a = (const double*)b_a.p;
    ka.d_S = (double*)b_w[0].p; ka.d_ST = (double*)b_w[1].p; ka.d_seS = (double*)b_w[2].p; ka.d_seST = (double*)b_w[3].p;
    ka.d_mean = (double*)b_w[4].p; ka.d_var = (double*)b_w[5].p; ka.d_nrow = (int*)b_nrow.p; ka.d_nbad = (long long*)b_nbad.p;
    if ((rc = ucf_field_launch_sobol(&ka, nullptr))) return fail(rc, "Sobol kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    std::vector<device_copy> back = {{nbad, b_nbad.p, sizeof(long long)}, {nrow, b_nrow.p, sizeof(int) * no}};
    for (int v = 0; v < 6; v++) back.push_back({w[v], b_w[v].p, v < 4 ? so * npar : so});
    return copy_back_sync(back);
}

// ---- the response slots R [nens][nctl + 1][ncon] of an ensemble: what ucf_field_yield and ucf_field_allocate share, in one
// place.  response_prepare is every check in the order of ucf_field_yield (check_own: the caller's own arguments, where
// ucf_field_yield checks its patterns), con and *ncon, the weights, the members and field_begin_launches; response_grow the
// buffers; response_members the uploads and the member loop with field_response_kernel; response_unlaunched the weights on the
// device and NaN bytes into the slots of the members that were not launched.  The caller holds the device switch, the stream
// and its drain between them.
struct response_call {
    ucf_field* f;
    ucf_plan* pl;
    int npar;
    const int* ids;
    int nens;
    const double *thetas, *weight;
    int nz;
    const double* z;
    int nctl;
    const int* ctl;
    const double* limit;
    int nq;
    const double* q;
    int nlev;
    const double* level;
    bool want_quant, want_pexc;
    int *con, *ncon;
    ucf_stats* stats;
    unsigned long long* u_out;
    double* ess;
    int* nlaunched;
};
struct response_slots {
    std::vector<int> hcon;                 // the staging of con and the limits: it outlives its copies
    std::vector<double> hlim;
    int nc = 0;
    size_t nslot = 0;                      // (nctl + 1) ncon
    bool weighted = false;
    ensemble_members E;
    double *d_R = nullptr, *d_small = nullptr, *d_lim = nullptr;       // b_yR; b_ysmall: the caller's own doubles, then the limits [ncon]
    int *d_con = nullptr, *d_ctl = nullptr;                            // b_yint
};

static int response_prepare(const response_call& a, const std::function<int()>& check_own, response_slots& S)
{
    ucf_field* f = a.f;
    const int nctl = a.nctl, nens = a.nens, npar = a.npar, nz = a.nz;
    long long nout = 0;
    int rc = field_check_call(f, nz, !a.z ? "NULL z" : !a.ids ? "NULL ids" : !a.thetas ? "NULL thetas" : nullptr, a.z, nout);
    if (rc) return rc;
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if ((rc = ensemble_check_levels(nens, a.nq, a.q, a.nlev, a.level, a.want_quant, a.want_pexc, "nlev", "level")) ||
        (rc = ensemble_check_thetas(npar, a.ids, nens, a.thetas))) return rc;
    if (!a.ctl || !a.limit) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !a.ctl ? "ctl" : "limit");
    if ((rc = check_own())) return rc;
    int owned[UCF_YIELD_MAX_CTL] = {};
    for (int j = 0; j < f->nwell; j++) {
        if (a.ctl[j] < -1 || a.ctl[j] >= nctl) return fail(UCF_ERR_BAD_ARGUMENT, "ctl[%d]=%d outside -1..%d", j, a.ctl[j], nctl - 1);
        if (a.ctl[j] >= 0) owned[a.ctl[j]]++;
    }
    for (int c = 0; c < nctl; c++)
        if (!owned[c]) return fail(UCF_ERR_BAD_ARGUMENT, "control %d owns no well", c);
    if (nout > 0x7fffffffLL)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d times x %d locations x %d depths: more than 2^31-1 outputs (con and bind are ints)", f->nt, f->nloc, nz);
    // con: the outputs with a finite limit, ascending, and their limits
    for (long long e = 0; e < nout; e++) {
        const double v = a.limit[e];
        if (std::isnan(v) || (std::isinf(v) && v < 0.0))
            return fail(UCF_ERR_BAD_ARGUMENT, "limit[%lld]=%g: a limit is finite, or +inf where the output is not constrained", e, v);
        if (std::isfinite(v)) { S.hcon.push_back((int)e); S.hlim.push_back(v); }
    }
    if (S.hcon.empty()) return fail(UCF_ERR_BAD_ARGUMENT, "no finite limit among the %lld outputs: nothing is constrained", nout);
    const int nc = S.nc = (int)S.hcon.size();
    S.nslot = (size_t)(nctl + 1) * nc;
    if ((long long)nens * (nctl + 1) * nc > 0x7fffffffLL * 256)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d slots x %d constrained outputs: too many values for one buffer", nens, nctl + 1, nc);
    if (a.con) std::copy(S.hcon.begin(), S.hcon.end(), a.con);
    if (a.ncon) *a.ncon = nc;
    S.weighted = a.weight != nullptr;
    if ((rc = ensemble_weights_of(nens, a.weight, S.weighted, a.u_out, a.ess, a.nlaunched, S.E)) ||
        (rc = ensemble_sets_of(f, a.pl, npar, a.ids, nens, a.thetas, S.E)))
        return rc;
    return field_begin_launches(f, a.pl, a.stats, &S.E.sets[S.E.first]);
}

// b_yR, b_yint and b_ysmall with own_small doubles of the caller's in front of the limits
static int response_grow(const response_call& a, size_t own_small, response_slots& S)
{
    ucf_field* f = a.f;
    int rc;
    if ((rc = grow_buffer(f->b_yR, sizeof(double) * a.nens * S.nslot, "response slots", f->n_alloc)) ||
        (rc = grow_buffer(f->b_yint, sizeof(int) * ((size_t)S.nc + f->nwell), "constrained outputs and controls", f->n_alloc)) ||
        (rc = grow_buffer(f->b_ysmall, sizeof(double) * (own_small + S.nc), "patterns and limits", f->n_alloc))) return rc;
    S.d_R = (double*)f->b_yR.p;
    S.d_small = (double*)f->b_ysmall.p;
    S.d_lim = S.d_small + own_small;
    S.d_con = (int*)f->b_yint.p;
    S.d_ctl = S.d_con + S.nc;
    return UCF_OK;
}

static int response_members(const response_call& a, const response_slots& S, hipStream_t st)
{
    ucf_field* f = a.f;
    const int nc = S.nc, nctl = a.nctl, nz = a.nz, npar = a.npar;
    const size_t nslot = S.nslot;
    double* d_R = S.d_R;
    int *d_con = S.d_con, *d_ctl = S.d_ctl;
    if (hipMemcpyAsync(d_con, S.hcon.data(), sizeof(int) * nc, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_ctl, a.ctl, sizeof(int) * f->nwell, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(S.d_lim, S.hlim.data(), sizeof(double) * nc, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the controls, patterns and limits failed: %s", hipGetErrorString(hipGetLastError()));
    const int* ids = a.ids;
    const double* thetas = a.thetas;
    auto failed = [&](int rc_m, int m) { return ensemble_member_failed(rc_m, m, npar, ids, thetas + (size_t)m * npar); };
    // per member the groups as in ucf_field_ensemble, finished by field_response_kernel into the member's slots (the buffers
    // of the groups may grow from member to member: their addresses are read at the launch)
    auto response_of = [=](int m) {
        return field_finish{"response", [=](const ucf_plan* p, hipStream_t s) {
                                return ucf_field_launch_response(nc, nctl, f->nloc, nz, f->nwell, (const ucf_field_well*)f->b_wells.p,
                                                                 (const int*)f->b_col.p, d_ctl, d_con, (const double*)f->b_h.p, p->D.Hc,
                                                                 d_R + (size_t)m * nslot, s);
                            }};
    };
    std::vector<field_launch> L;
    return field_map_sets(f, a.nens, S.E.sets.data(), [&](int m, const std::vector<field_launch>*& Lm) { Lm = &L; return field_launches_of(f, S.E.sets[m], L); },
                          nz, a.z, response_of, a.stats, failed, S.weighted ? S.E.u.data() : nullptr);
}

// b_u (grown by the caller) and NaN bytes into the slots of the members that were not launched
static int response_unlaunched(const response_call& a, const response_slots& S, hipStream_t st)
{
    if (!S.weighted) return UCF_OK;
    bool ok = hipMemcpyAsync(a.f->b_u.p, S.E.u.data(), sizeof(unsigned long long) * a.nens, hipMemcpyHostToDevice, st) == hipSuccess;
    for (int m = 0; m < a.nens && ok; m++)
        if (S.E.u[m] == 0) ok = hipMemsetAsync(S.d_R + (size_t)m * S.nslot, 0xff, sizeof(double) * S.nslot, st) == hipSuccess;
    if (!ok) return fail(UCF_ERR_HIP, "upload of the ensemble's weights failed: %s", hipGetErrorString(hipGetLastError()));
    return UCF_OK;
}

// what ucf_field_yield and ucf_debug_field_yield check on the controls' count, the patterns and smax
static int yield_check_patterns(int nctl, int npat, const double* x, double smax)
{
    if (nctl < 1 || nctl > UCF_YIELD_MAX_CTL) return fail(UCF_ERR_BAD_ARGUMENT, "nctl=%d outside 1..%d", nctl, UCF_YIELD_MAX_CTL);
    if (npat < 1 || npat > UCF_YIELD_MAX_PAT) return fail(UCF_ERR_BAD_ARGUMENT, "npat=%d outside 1..%d", npat, UCF_YIELD_MAX_PAT);
    if (!x) return fail(UCF_ERR_BAD_ARGUMENT, "NULL x");
    int rc = field_check_finite("x", npat * nctl, x);
    if (rc) return rc;
    if (!(smax > 0.0) || !std::isfinite(smax)) return fail(UCF_ERR_BAD_ARGUMENT, "smax=%g must be positive and finite", smax);
    return UCF_OK;
}

int ucf_field_yield(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, const double* weight, int nz,
                    const double* z, int nctl, const int* ctl, int npat, const double* x, const double* limit, double smax, int nq,
                    const double* q, int nlev, const double* level, const ucf_ensemble_maps* ystat, double* pexc, double* pfeas, double* hi,
                    double* lo, int* bind, int* dead, double* resp, int* con, int* ncon, long long* nbad, ucf_stats* stats,
                    unsigned long long* u_out, double* ess, int* nlaunched)
{
    response_call a = {f, pl, npar, ids, nens, thetas, weight, nz, z, nctl, ctl, limit, nq, q, nlev, level, ystat && ystat->quant, pexc != nullptr,
                       con, ncon, stats, u_out, ess, nlaunched};
    response_slots S;
    int rc = response_prepare(a, [&] { return yield_check_patterns(nctl, npat, x, smax); }, S);
    if (rc) return rc;
    const int nc = S.nc;
    const bool weighted = S.weighted;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    // b_ens: q [MAX_Q], level [MAX_Q], the limit 0.5 of pfeas, then what is asked for of mean, sd, min, max [npat], quant
    // [nq][npat], nfin [npat] (ints, padded to whole doubles), pexc [nlev][npat], pfeas [npat]
    const size_t np = (size_t)npat, nmp = (size_t)nens * np, nslot = S.nslot, so = sizeof(double) * np;
    const ucf_ensemble_maps none = {};
    const ucf_ensemble_maps* want = ystat ? ystat : &none;
    constexpr size_t OFF_HALF = 2 * UCF_ENSEMBLE_MAX_Q;
    size_t used = OFF_HALF + 1;                           // in doubles
    auto take = [&](bool asked, size_t n) { const size_t o = used; if (asked) used += n; return asked ? o : (size_t)-1; };
    const size_t o_mean = take(want->mean, np), o_sd = take(want->sd, np), o_min = take(want->min, np), o_max = take(want->max, np),
                 o_quant = take(want->quant, np * nq), o_nfin = take(want->nfin, (np + 1) / 2), o_pexc = take(pexc, np * nlev),
                 o_pfeas = take(pfeas, np);
    if ((rc = response_grow(a, np * nctl, S)) ||
        (rc = grow_buffer(f->b_yval, sizeof(double) * 4 * nmp, "admissible scales", f->n_alloc)) ||
        (rc = grow_buffer(f->b_yidx, sizeof(int) * 2 * nmp, "binding outputs", f->n_alloc)) ||
        (rc = grow_buffer(f->b_nbad, sizeof(long long) * 3, "counts", f->n_alloc)) ||
        (rc = grow_buffer(f->b_ens, sizeof(double) * used, "ensemble statistics", f->n_alloc)) ||
        (weighted && (rc = grow_buffer(f->b_u, sizeof(unsigned long long) * nens, "ensemble weights", f->n_alloc)))) return rc;
    double* base = (double*)f->b_ens.p;
    auto dev = [&](size_t o) { return o == (size_t)-1 ? nullptr : base + o; };
    double *d_R = S.d_R, *d_x = S.d_small, *d_lim = S.d_lim;
    double *d_y = (double*)f->b_yval.p, *d_fe = d_y + nmp, *d_hi = d_fe + nmp, *d_lo = d_hi + nmp;
    int *d_con = S.d_con, *d_bind = (int*)f->b_yidx.p, *d_dead = d_bind + nmp;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};                     // the staging outlives its copies
    if (hipMemcpyAsync(d_x, x, sizeof(double) * np * nctl, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the controls, patterns and limits failed: %s", hipGetErrorString(hipGetLastError()));
    if ((rc = response_members(a, S, st))) return rc;
    double ql[2 * UCF_ENSEMBLE_MAX_Q];
    ensemble_pack_levels(nq, q, nlev, level, ql);
    const double half = 0.5;
    if (hipMemsetAsync(f->b_nbad.p, 0, sizeof(long long) * 3, st) != hipSuccess ||
        hipMemcpyAsync(base, ql, sizeof(ql), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(base + OFF_HALF, &half, sizeof(half), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the ensemble's arrays failed: %s", hipGetErrorString(hipGetLastError()));
    if ((rc = response_unlaunched(a, S, st))) return rc;
    long long* d_nbad = (long long*)f->b_nbad.p;
    ucf_yield_args ya = {};
    ya.nctl = nctl; ya.nens = nens; ya.ncon = nc; ya.npat = npat; ya.d_R = d_R; ya.d_x = d_x; ya.d_lim = d_lim; ya.d_con = d_con; ya.smax = smax;
    ya.d_y = d_y; ya.d_fe = d_fe; ya.d_hi = d_hi; ya.d_lo = d_lo; ya.d_bind = d_bind; ya.d_dead = d_dead; ya.d_nbad = d_nbad + 2;
    if ((rc = ucf_field_launch_yield(&ya, st))) return fail(rc, "yield kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    // the member reduction of ucf_field_ensemble with nout = npat: on y, then on fe against 0.5
    ucf_ensemble_reduce_args ra = {};
    ra.nens = nens; ra.nout = npat; ra.d_a = d_y;
    ra.d_u = weighted ? (const unsigned long long*)f->b_u.p : nullptr;
    ra.nq = nq; ra.d_q = base; ra.nlim = nlev; ra.d_limit = base + UCF_ENSEMBLE_MAX_Q;
    ra.d_mean = dev(o_mean); ra.d_sd = dev(o_sd); ra.d_min = dev(o_min); ra.d_max = dev(o_max); ra.d_nfin = (int*)dev(o_nfin);
    ra.d_quant = dev(o_quant); ra.d_pexc = dev(o_pexc); ra.d_nbad = d_nbad;
    rc = ucf_field_launch_ensemble_reduce(&ra, st);
    if (rc == UCF_OK && pfeas) {
        ucf_ensemble_reduce_args rf = {};
        rf.nens = nens; rf.nout = npat; rf.d_a = d_fe; rf.d_u = ra.d_u;
        rf.nlim = 1; rf.d_limit = base + OFF_HALF; rf.d_pexc = dev(o_pfeas); rf.d_nbad = d_nbad + 1;
        rc = ucf_field_launch_ensemble_reduce(&rf, st);
    }
    if (rc) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    long long invalid = 0;
    const size_t sm = sizeof(double) * nmp;
    rc = copy_back({{want->mean, dev(o_mean), so}, {want->sd, dev(o_sd), so}, {want->min, dev(o_min), so}, {want->max, dev(o_max), so},
                    {want->quant, dev(o_quant), so * nq}, {want->nfin, dev(o_nfin), sizeof(int) * np}, {want->all, d_y, sm},
                    {pexc, dev(o_pexc), so * nlev}, {pfeas, dev(o_pfeas), so}, {hi, d_hi, sm}, {lo, d_lo, sm}, {bind, d_bind, sizeof(int) * nmp},
                    {dead, d_dead, sizeof(int) * nmp}, {resp, d_R, sizeof(double) * nens * nslot}, {&invalid, d_nbad + 2, sizeof(long long)}},
                   st, pl->device);
    if (rc) return rc;
    if (nbad) *nbad = invalid - (nens - S.E.nrun);        // a member that was not launched is not counted
    return UCF_OK;
}

int ucf_debug_field_yield(int nctl, int nens, int ncon, int npat, const double* R, const double* x, const double* limit_con, const int* con,
                          double smax, double* y, double* fe, double* hi, double* lo, int* bind, int* dead, long long* nbad)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (ncon < 1) return fail(UCF_ERR_BAD_ARGUMENT, "ncon=%d: at least one constrained output", ncon);
    int rc = yield_check_patterns(nctl, npat, x, smax);
    if (rc) return rc;
    const long long nval = (long long)nens * (nctl + 1) * ncon;
    if (nval > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d slots x %d constrained outputs: more than 2^31-1 values", nens, nctl + 1, ncon);
    if (!R || !limit_con || !con) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !R ? "R" : !limit_con ? "limit_con" : "con");
    if ((rc = field_check_finite("limit_con", ncon, limit_con))) return rc;
    for (int i = 0; i < ncon; i++)
        if (con[i] < 0 || (i > 0 && con[i] <= con[i - 1]))
            return fail(UCF_ERR_BAD_ARGUMENT, "con[%d]=%d: the constrained outputs are not negative and ascend strictly", i, con[i]);
    if ((rc = require_device())) return rc;
    const size_t nmp = (size_t)nens * npat, sR = sizeof(double) * (size_t)nval, sx = sizeof(double) * npat * nctl, sm = sizeof(double) * nmp;
    dev_buf b_R, b_x, b_lim, b_con, b_val, b_idx, b_nbad;
    if (b_R.alloc(sR) || b_x.alloc(sx) || b_lim.alloc(sizeof(double) * ncon) || b_con.alloc(sizeof(int) * ncon) || b_val.alloc(4 * sm) ||
        b_idx.alloc(sizeof(int) * 2 * nmp) || b_nbad.alloc(sizeof(long long)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_R.p, R, sR, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_x.p, x, sx, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_lim.p, limit_con, sizeof(double) * ncon, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_con.p, con, sizeof(int) * ncon, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_nbad.p, 0, sizeof(long long)));
    ucf_yield_args ya = {};
    ya.nctl = nctl; ya.nens = nens; ya.ncon = ncon; ya.npat = npat; ya.smax = smax;
    ya.d_R = (const double*)b_R.p; ya.d_x = (const double*)b_x.p; ya.d_lim = (const double*)b_lim.p; ya.d_con = (const int*)b_con.p;
    ya.d_y = (double*)b_val.p; ya.d_fe = ya.d_y + nmp; ya.d_hi = ya.d_fe + nmp; ya.d_lo = ya.d_hi + nmp;
    ya.d_bind = (int*)b_idx.p; ya.d_dead = ya.d_bind + nmp; ya.d_nbad = (long long*)b_nbad.p;
    if ((rc = ucf_field_launch_yield(&ya, nullptr))) return fail(rc, "yield kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{y, ya.d_y, sm}, {fe, ya.d_fe, sm}, {hi, ya.d_hi, sm}, {lo, ya.d_lo, sm}, {bind, ya.d_bind, sizeof(int) * nmp},
                           {dead, ya.d_dead, sizeof(int) * nmp}, {nbad, b_nbad.p, sizeof(long long)}});
}

int ucf_field_allocate(ucf_field* f, ucf_plan* pl, int npar, const int* ids, int nens, const double* thetas, const double* weight, int nz,
                       const double* z, int nctl, const int* ctl, int nobj, const double* w, const double* xmax, int maxit, const double* limit,
                       double* x, double* g, int* status, int* iters, int* work, double* lam, int nq, const double* q, double* quant,
                       double* value, int* best, double* best_x, double* gquant, double* resp, int* con, int* ncon, long long* nbad,
                       ucf_stats* stats, unsigned long long* u_out, double* ess, int* nlaunched)
{
    const bool reliability = quant || value || best || best_x;
    response_call a = {f, pl, npar, ids, nens, thetas, weight, nz, z, nctl, ctl, limit, nq, q, 0, nullptr, reliability || gquant != nullptr, false,
                       con, ncon, stats, u_out, ess, nlaunched};
    response_slots S;
    int rc = response_prepare(a, [&] {
        int rc_own = allocate_check_programme(nctl, nobj, w, xmax, maxit);
        if (rc_own == UCF_OK && reliability && (long long)nens * nobj > UCF_YIELD_MAX_PAT)
            rc_own = fail(UCF_ERR_BAD_ARGUMENT, "the reliability stage: %d members x %d objectives are more than %d rate patterns", nens, nobj, UCF_YIELD_MAX_PAT);
        return rc_own;
    }, S);
    if (rc) return rc;
    const int nc = S.nc;
    ucf_plan* sp = f->scratch;
    device_switch dg(pl->device);
    // b_ysmall: w [nobj][nctl], xmax [nctl], the patterns [nens nobj][nctl] of the reliability stage, then the limits
    // b_ens: q [MAX_Q] and MAX_Q unused limits, then quant [nq][npat] and gquant [nq][nobj] where they are formed
    const size_t nmo = (size_t)nens * nobj, nw = (size_t)nobj * nctl, nx = nmo * nctl, npat = nmo;
    const size_t o_quant = 2 * UCF_ENSEMBLE_MAX_Q, o_gquant = o_quant + (reliability ? npat * nq : 0), used = o_gquant + (gquant ? (size_t)nobj * nq : 0);
    if ((rc = response_grow(a, nw + nctl + (reliability ? nx : 0), S)) ||
        (rc = grow_buffer(f->b_aval, sizeof(double) * (2 * nx + nmo), "allocations", f->n_alloc)) ||
        (rc = grow_buffer(f->b_aidx, sizeof(int) * (2 * nmo + nx), "working sets", f->n_alloc)) ||
        (reliability && ((rc = grow_buffer(f->b_yval, sizeof(double) * 4 * nens * npat, "admissible scales", f->n_alloc)) ||
                         (rc = grow_buffer(f->b_yidx, sizeof(int) * 2 * nens * npat, "binding outputs", f->n_alloc)))) ||
        (rc = grow_buffer(f->b_nbad, sizeof(long long) * 4, "counts", f->n_alloc)) ||
        (rc = grow_buffer(f->b_ens, sizeof(double) * used, "ensemble statistics", f->n_alloc)) ||
        (S.weighted && (rc = grow_buffer(f->b_u, sizeof(unsigned long long) * nens, "ensemble weights", f->n_alloc)))) return rc;
    double* base = (double*)f->b_ens.p;
    double *d_w = S.d_small, *d_xmax = d_w + nw, *d_xpat = reliability ? d_xmax + nctl : nullptr;
    double *d_x = (double*)f->b_aval.p, *d_lam = d_x + nx, *d_g = d_lam + nx;
    int *d_status = (int*)f->b_aidx.p, *d_iters = d_status + nmo, *d_work = d_iters + nmo;
    hipStream_t st = plan_stream(sp);
    if (!st) return fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", pl->device);
    drain drained{st};                     // the staging outlives its copies
    double ql[2 * UCF_ENSEMBLE_MAX_Q];
    ensemble_pack_levels(nq, q, 0, nullptr, ql);
    if (hipMemcpyAsync(d_w, w, sizeof(double) * nw, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_xmax, xmax, sizeof(double) * nctl, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(base, ql, sizeof(ql), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(f->b_nbad.p, 0, sizeof(long long) * 4, st) != hipSuccess)
        return fail(UCF_ERR_HIP, "upload of the objectives and capacities failed: %s", hipGetErrorString(hipGetLastError()));
    if ((rc = response_members(a, S, st)) || (rc = response_unlaunched(a, S, st))) return rc;
    long long* d_nbad = (long long*)f->b_nbad.p;
    ucf_allocate_args aa = {};
    aa.nctl = nctl; aa.nens = nens; aa.ncon = nc; aa.nobj = nobj; aa.maxit = maxit; aa.d_R = S.d_R; aa.d_lim = S.d_lim; aa.d_w = d_w; aa.d_xmax = d_xmax;
    aa.d_x = d_x; aa.d_g = d_g; aa.d_lam = d_lam; aa.d_status = d_status; aa.d_iters = d_iters; aa.d_work = d_work; aa.d_xpat = d_xpat;
    aa.d_nbad = d_nbad + 3;
    if ((rc = ucf_field_launch_allocate(&aa, st))) return fail(rc, "allocate kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    const unsigned long long* d_u = S.weighted ? (const unsigned long long*)f->b_u.p : nullptr;
    if (reliability) {
        // the optima as rate patterns through the ratio test of ucf_field_yield with smax = 1, then its member reduction
        const size_t nmp = (size_t)nens * npat;
        ucf_yield_args ya = {};
        ya.nctl = nctl; ya.nens = nens; ya.ncon = nc; ya.npat = (int)npat; ya.d_R = S.d_R; ya.d_x = d_xpat; ya.d_lim = S.d_lim; ya.d_con = S.d_con;
        ya.smax = 1.0;
        ya.d_y = (double*)f->b_yval.p; ya.d_fe = ya.d_y + nmp; ya.d_hi = ya.d_fe + nmp; ya.d_lo = ya.d_hi + nmp;
        ya.d_bind = (int*)f->b_yidx.p; ya.d_dead = ya.d_bind + nmp; ya.d_nbad = d_nbad + 2;
        if ((rc = ucf_field_launch_yield(&ya, st))) return fail(rc, "yield kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        ucf_ensemble_reduce_args ra = {};
        ra.nens = nens; ra.nout = (long long)npat; ra.d_a = ya.d_y; ra.d_u = d_u; ra.nq = nq; ra.d_q = base; ra.d_quant = base + o_quant; ra.d_nbad = d_nbad;
        if ((rc = ucf_field_launch_ensemble_reduce(&ra, st))) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    if (gquant) {
        ucf_ensemble_reduce_args rg = {};
        rg.nens = nens; rg.nout = nobj; rg.d_a = d_g; rg.d_u = d_u; rg.nq = nq; rg.d_q = base; rg.d_quant = base + o_gquant; rg.d_nbad = d_nbad + 1;
        if ((rc = ucf_field_launch_ensemble_reduce(&rg, st))) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    }
    // the host step of the reliability stage reads quant, g and x whether the caller asked for them or not
    std::vector<double> hquant(reliability ? npat * nq : 0), hg(reliability ? nmo : 0), hx(reliability ? nx : 0);
    long long invalid = 0;
    rc = copy_back({{x, d_x, sizeof(double) * nx}, {g, d_g, sizeof(double) * nmo}, {lam, d_lam, sizeof(double) * nx}, {status, d_status, sizeof(int) * nmo},
                    {iters, d_iters, sizeof(int) * nmo}, {work, d_work, sizeof(int) * nx}, {hquant.data(), base + o_quant, sizeof(double) * hquant.size()},
                    {hg.data(), d_g, sizeof(double) * hg.size()}, {hx.data(), d_x, sizeof(double) * hx.size()},
                    {gquant, base + o_gquant, sizeof(double) * nobj * nq}, {resp, S.d_R, sizeof(double) * nens * S.nslot},
                    {&invalid, d_nbad + 3, sizeof(long long)}},
                   st, pl->device);
    if (rc) return rc;
    if (reliability) {
        if (quant) std::copy(hquant.begin(), hquant.end(), quant);
        if ((rc = ucf_allocate_select(nq, nens, nobj, nctl, hquant.data(), hg.data(), hx.data(), value, best, best_x))) return rc;
    }
    if (nbad) *nbad = invalid - (nens - S.E.nrun);        // a member that was not launched is not counted
    return UCF_OK;
}

int ucf_debug_field_allocate(int nctl, int nens, int ncon, int nobj, const double* R, const double* limit_con, const int* con, const double* w,
                             const double* xmax, int maxit, double* x, double* g, int* status, int* iters, int* work, double* lam, long long* nbad)
{
    int rc = allocate_check_programme(nctl, nobj, w, xmax, maxit);
    if (rc || (rc = allocate_check_slots(nctl, nens, ncon, R, limit_con))) return rc;
    if (!con) return fail(UCF_ERR_BAD_ARGUMENT, "NULL con");
    for (int i = 0; i < ncon; i++)
        if (con[i] < 0 || (i > 0 && con[i] <= con[i - 1]))
            return fail(UCF_ERR_BAD_ARGUMENT, "con[%d]=%d: the constrained outputs are not negative and ascend strictly", i, con[i]);
    if ((rc = require_device())) return rc;
    const size_t nmo = (size_t)nens * nobj, nx = nmo * nctl, nw = (size_t)nobj * nctl, sR = sizeof(double) * nens * (nctl + 1) * (size_t)ncon;
    dev_buf b_R, b_small, b_val, b_idx, b_nbad;
    if (b_R.alloc(sR) || b_small.alloc(sizeof(double) * (nw + nctl + ncon)) || b_val.alloc(sizeof(double) * (2 * nx + nmo)) ||
        b_idx.alloc(sizeof(int) * (2 * nmo + nx)) || b_nbad.alloc(sizeof(long long)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    double *d_w = (double*)b_small.p, *d_xmax = d_w + nw, *d_lim = d_xmax + nctl;
    HIP_TRY(hipMemcpy(b_R.p, R, sR, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_w, w, sizeof(double) * nw, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_xmax, xmax, sizeof(double) * nctl, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lim, limit_con, sizeof(double) * ncon, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_nbad.p, 0, sizeof(long long)));
    ucf_allocate_args aa = {};
    aa.nctl = nctl; aa.nens = nens; aa.ncon = ncon; aa.nobj = nobj; aa.maxit = maxit;
    aa.d_R = (const double*)b_R.p; aa.d_lim = d_lim; aa.d_w = d_w; aa.d_xmax = d_xmax;
    aa.d_x = (double*)b_val.p; aa.d_lam = aa.d_x + nx; aa.d_g = aa.d_lam + nx;
    aa.d_status = (int*)b_idx.p; aa.d_iters = aa.d_status + nmo; aa.d_work = aa.d_iters + nmo; aa.d_nbad = (long long*)b_nbad.p;
    if ((rc = ucf_field_launch_allocate(&aa, nullptr))) return fail(rc, "allocate kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{x, aa.d_x, sizeof(double) * nx}, {g, aa.d_g, sizeof(double) * nmo}, {lam, aa.d_lam, sizeof(double) * nx},
                           {status, aa.d_status, sizeof(int) * nmo}, {iters, aa.d_iters, sizeof(int) * nmo}, {work, aa.d_work, sizeof(int) * nx},
                           {nbad, b_nbad.p, sizeof(long long)}});
}

int ucf_ensemble_quantise(int nens, const double* weight, unsigned long long* u, double* ess)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (!weight || !u) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !weight ? "weight" : "u");
    double wmax = 0.0;
    for (int m = 0; m < nens; m++) {
        if (!(weight[m] >= 0.0) || !std::isfinite(weight[m]))
            return fail(UCF_ERR_BAD_ARGUMENT, "member %d: weight=%g must be finite and not negative", m, weight[m]);
        if (weight[m] > wmax) wmax = weight[m];
    }
    if (!(wmax > 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "all %d weights are 0: no member is in the ensemble", nens);
    unsigned long long U = 0;
    double U2 = 0.0;
    for (int m = 0; m < nens; m++) {
        const double r = weight[m] / wmax;
        u[m] = (unsigned long long)std::floor(r * 4294967296.0 + 0.5);
        U += u[m];
        U2 = U2 + (double)u[m] * (double)u[m];
    }
    if (ess) *ess = (double)U * (double)U / U2;
    return UCF_OK;
}

int ucf_ensemble_likelihood_weights(int nens, const double* phi, const int* nbad, double s2, double* weight, int* best, int* nadmissible)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (!phi || !weight) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !phi ? "phi" : "weight");
    if (!(s2 > 0.0) || !std::isfinite(s2)) return fail(UCF_ERR_BAD_ARGUMENT, "s2=%g must be positive and finite", s2);
    int b = -1, nadm = 0;
    for (int m = 0; m < nens; m++) {
        if (!std::isfinite(phi[m]) || (nbad && nbad[m] != 0)) continue;
        nadm++;
        if (b < 0 || phi[m] < phi[b]) b = m;
    }
    if (b < 0) return fail(UCF_ERR_BAD_ARGUMENT, "no admissible member among %d: every phi is not finite or has nbad > 0", nens);
    for (int m = 0; m < nens; m++) {
        const bool adm = std::isfinite(phi[m]) && !(nbad && nbad[m] != 0);
        weight[m] = adm ? std::exp(-0.5 * ((phi[m] - phi[b]) / s2)) : 0.0;
    }
    if (best) *best = b;
    if (nadmissible) *nadmissible = nadm;
    return UCF_OK;
}

int ucf_field_ensemble_draw(int npar, const double* theta, const double* cov, int nens, unsigned long long seed, double* thetas)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!theta || !cov || !thetas) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !theta ? "theta" : !cov ? "cov" : "thetas");
    if (nens < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d: at least one member", nens);
    for (int j = 0; j < npar; j++)
        if (!(theta[j] > 0.0) || !std::isfinite(theta[j])) return fail(UCF_ERR_BAD_ARGUMENT, "theta[%d]=%g must be positive and finite", j, theta[j]);
    int rc = field_check_cov(npar, cov);
    if (rc) return rc;
    double L[UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR];
    for (int i = 0; i < npar * npar; i++) L[i] = cov[i];
    if (fit_cholesky_factor(npar, L) != UCF_OK) return fail(UCF_ERR_SINGULAR, "cov is not positive definite (%d x %d): it has no Cholesky factor", npar, npar);
    unsigned long long state = seed;
    double zeta[UCF_FIT_MAX_PAR + 1];
    for (int m = 0; m < nens; m++) {
        for (int i = 0; i < npar; i += 2) {
            const double u1 = ensemble_uniform(state), u2 = ensemble_uniform(state);
            const double rad = std::sqrt(-2.0 * std::log(u1)), ang = 6.283185307179586 * u2;
            zeta[i] = rad * std::cos(ang);
            zeta[i + 1] = rad * std::sin(ang);
        }
        for (int j = 0; j < npar; j++) {
            double acc = 0.0;
            for (int k = 0; k <= j; k++) acc = acc + L[j * npar + k] * zeta[k];
            thetas[(size_t)m * npar + j] = theta[j] * std::exp(acc);
        }
    }
    return UCF_OK;
}

int ucf_field_images(int nwell, const double* xw, const double* yw, const double* qw, const double* t0w, double a, double b, double c,
                     int kind, double* xo, double* yo, double* qo, double* t0o)
{
    if (nwell < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nwell=%d: at least one well", nwell);
    if (!xw || !yw || !qw || !t0w || !xo || !yo || !qo || !t0o) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    if (kind != 0 && kind != 1) return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d: 0 (no-flow) or 1 (constant head)", kind);
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c)) return fail(UCF_ERR_BAD_ARGUMENT, "the line a x + b y = c has a coefficient that is not finite");
    if (a == 0.0 && b == 0.0) return fail(UCF_ERR_BAD_ARGUMENT, "a = b = 0 describes no line");
    int rc;
    if ((rc = field_check_finite("xw", nwell, xw)) || (rc = field_check_finite("yw", nwell, yw)) || (rc = field_check_finite("qw", nwell, qw)) ||
        (rc = field_check_finite("t0w", nwell, t0w))) return rc;
    // the mirror point x - 2 a d, y - 2 b d with d = (a x + b y - c) / (a^2 + b^2), in extended precision and rounded once
    const long double la = a, lb = b, lc = c, n2 = la * la + lb * lb;
    for (int j = 0; j < nwell; j++) {
        const long double d = (la * xw[j] + lb * yw[j] - lc) / n2;
        if (d == 0.0L) return fail(UCF_ERR_BAD_ARGUMENT, "well %d lies on the boundary line", j);
        xo[j] = xw[j]; yo[j] = yw[j]; qo[j] = qw[j]; t0o[j] = t0w[j];
        xo[nwell + j] = (double)(xw[j] - 2.0L * la * d);
        yo[nwell + j] = (double)(yw[j] - 2.0L * lb * d);
        qo[nwell + j] = kind == 0 ? qw[j] : -qw[j];
        t0o[nwell + j] = t0w[j];
    }
    return UCF_OK;
}

}  // extern "C"
