// ucf_fit.cpp -- parameter fitting (ucf.h: ucf_fit_*): observations resident on the device, base and perturbed parameter sets through
// the shared core of ucf_drawdown_multi, residuals / objective / Jacobian / normal equations in fit_reduce_kernel
// (ucf_fit.hip, one launcher: ucf_fit_launch_reduce), Levenberg-Marquardt for many starts at once on the host (npar x npar
// arithmetic).  An observation network (ucf_fit_create_network) launches per-well blocks; a field fit
// (ucf_fit_create_field) is the network of its virtual wells -- one per (observation well, distinct distance to a pumping
// well) -- whose reduction sums over pumping wells.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "ucf_host.h"
#include "ucf_fit.h"

using namespace ucf_host;

// Points per block of a network launch: one tile of the lane = point layout, so that a wave never straddles two blocks.
#define UCF_FIT_PPP UCF_WAVE
// The used wells of a network that have `nz` depths each, in order of radius.  Per plan the group evaluates
// pts = 64 x (blocks of all its wells) points: the distinct times of a well in ascending order, its last block padded by
// repeating the last time.  In the buffers of an evaluation over nplans plans the group's points start at
// nplans * pt_prefix (values: nplans * prefix), plan k of it at k * pts (k * stride).
struct fit_group {
    int nz = 0;
    std::vector<int> wells, blk0, nt;      // per used well: its index, its first block, its distinct times
    std::vector<int> blk_well;             // per block: position of its well in `wells`
    std::vector<double> t, r;              // [pts] dimensional times and radii of one plan
    size_t pts = 0, stride = 0;            // stride = pts * nz
    size_t pt_prefix = 0, prefix = 0;      // sums of pts / stride over the groups before this one
};

struct ucf_fit {
    ucf_params base = {};
    int npar = 0, ids[UCF_FIT_MAX_PAR] = {};
    int nobs = 0, nz = 0, device = 0;
    std::vector<double> t_s, r_s, z;       // observation times / radii in order of radius (the order the core evaluates in), depths
    std::vector<ucf_plan*> plans;          // the pool: made once, refreshed by ucf_plan_update
    multi_io io;
    ucf_buffer b_slot, b_obs, b_w;         // fixed at create
    ucf_buffer b_t, b_r, b_s, b_h, b_d, b_hc, b_sums, b_nbad, b_J, b_sim;      // grown on demand
    std::vector<double> h_hc, h_sums;
    long long n_alloc = 0;                 // device allocations of the fit itself + plans created
    // where observation i finds its value in b_h (host copy; ucf_fit_create: prefix 0, stride nobs * nz, at = its slot)
    std::vector<ucf_fit_obs_ref> refs;
    int last_nplans = 0;                   // plans of the last evaluation (ucf_fit_debug_h)
    // how an observation finds its value: ucf_fit_create | ucf_fit_create_network | ucf_fit_create_field.  A field fit is
    // a network for everything but the reduction.
    ucf_fit_source kind = UCF_FIT_SLOTS;
    bool is_network() const { return kind != UCF_FIT_SLOTS; }
    // an observation network
    std::vector<double> well_r, well_z;    // radius per well; depths of well w at well_z[well_z0[w] ..)
    std::vector<int> well_nz, well_z0;
    std::vector<fit_group> groups;         // wells with the same number of depths: one launch sequence each
    size_t net_pts = 0, net_vals = 0;      // per plan, all groups: points launched, (point, depth) values
    long long dense = 0;                   // (point, depth) evaluations per plan of the dense form
    ucf_buffer b_ref;
    // a field fit (ucf_fit_create_field): a network whose wells are the virtual wells and whose `refs` are per TERM;
    // observation i sums the terms b_first[i] .. b_first[i + 1] of b_term (ucf_fit_term: place and rate factor)
    ucf_buffer b_term, b_first;
    std::vector<double> term_tobs, term_t; // per term: the time of its observation, and that time minus the start of its pumping well
    // derivative data (ucf_fit_set_derivative): observed t ds/dt and its weight per observation, nd of them with a positive
    // weight; a field fit also holds tfac per term.  The buffers stay when the data are detached.
    bool deriv = false;
    int nd = 0;
    ucf_buffer b_dobs, b_wd, b_tfac;
    ucf_buffer b_Jd, b_simd;               // grown on demand, as b_J and b_sim
    // the loss (ucf_fit_set_loss): a kind and its constant, nothing on the device.  The factors that ucf_fit_loss_report asks
    // for are grown on demand.
    int loss = UCF_LOSS_L2;
    double loss_c = 0.0;
    ucf_buffer b_ndown, b_bfac, b_bdfac;
    // resampling (ucf_fit_set_resample): nrep rows of nobs multiplicities on the device, 0 when detached (the buffer stays); what
    // a resampled reduction reads and writes per reduction is grown on demand
    int nrep = 0;
    ucf_buffer b_mult, b_setof, b_rep, b_counts;
    // every device buffer above: the one list (ucf_fit_destroy frees through it)
    std::array<ucf_buffer*, 28> buffers()
    {
        return {{&b_slot, &b_obs, &b_w, &b_t, &b_r, &b_s, &b_h, &b_d, &b_hc, &b_sums, &b_nbad, &b_J, &b_sim, &b_ref, &b_term, &b_first,
                 &b_dobs, &b_wd, &b_tfac, &b_Jd, &b_simd, &b_ndown, &b_bfac, &b_bdfac, &b_mult, &b_setof, &b_rep, &b_counts}};
    }
    std::vector<double> st_t;              // staging of one plan: its tD over all groups ...
    std::vector<int> st_s;                 // ... and their split vector
};

const char* ucf_host::fit_par_name(int id, char* buf, size_t n)
{
    static const char* const names[] = {"Kr", "kappa", "Ss", "Sy", "ac", "ak", "usL"};
    if (id >= 0 && id < UCF_PAR_MOENCH_ALPHA0) return names[id];
    std::snprintf(buf, n, "MoenchAlpha[%d]", id - UCF_PAR_MOENCH_ALPHA0);
    return buf;
}

int ucf_host::fit_theta_sets(const ucf_params& base, int npar, const int* ids, const double* theta, double dlog, int count, ucf_params* sets)
{
    const double up = std::exp(dlog), down = std::exp(-dlog);
    double th[UCF_FIT_MAX_PAR];
    for (int v = 0; v < count; v++) {
        for (int j = 0; j < npar && j < UCF_FIT_MAX_PAR; j++) th[j] = theta[j];
        if (v > 0 && (v - 1) / 2 < UCF_FIT_MAX_PAR) th[(v - 1) / 2] = th[(v - 1) / 2] * ((v & 1) ? up : down);
        int rc = ucf_fit_perturb(&base, npar, ids, th, &sets[v]);      // (refuses an npar outside 1..UCF_FIT_MAX_PAR)
        if (rc) return rc;
    }
    return UCF_OK;
}

namespace {
double* fit_field(ucf_params& P, int id)
{
    switch (id) {
    case UCF_PAR_KR: return &P.Kr;
    case UCF_PAR_KAPPA: return &P.kappa;
    case UCF_PAR_SS: return &P.Ss;
    case UCF_PAR_SY: return &P.Sy;
    case UCF_PAR_AC: return &P.ac;
    case UCF_PAR_AK: return &P.ak;
    case UCF_PAR_USL: return &P.usL;
    default: break;
    }
    if (id >= UCF_PAR_MOENCH_ALPHA0 && id < UCF_PAR_MOENCH_ALPHA0 + UCF_MAX_MOENCH) return &P.MoenchAlpha[id - UCF_PAR_MOENCH_ALPHA0];
    return nullptr;
}

// does the model of P read parameter `id`?  (Kr, Ss: every model; kappa: all but Theis; Sy: the unconfined models 3..6;
// ak: model 6; ac, usL: model 6 in its finite-difference form -- the Malama form replaces ac by ak and has no usL;
// Moench alpha i: model 3, i < MoenchM)
bool fit_reads(const ucf_params& P, int id)
{
    switch (id) {
    case UCF_PAR_KR: case UCF_PAR_SS: return true;
    case UCF_PAR_KAPPA: return P.model >= 1;
    case UCF_PAR_SY: return P.model >= 3;
    case UCF_PAR_AK: return P.model == 6;
    case UCF_PAR_AC: case UCF_PAR_USL: return P.model == 6 && P.MNtype != 1;
    default: break;
    }
    return P.model == 3 && id >= UCF_PAR_MOENCH_ALPHA0 && id < UCF_PAR_MOENCH_ALPHA0 + P.MoenchM;
}

int fit_check_ids(const ucf_params& P, int npar, const int* ids)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!ids) return fail(UCF_ERR_BAD_ARGUMENT, "ids is NULL");
    char nb[32];
    for (int j = 0; j < npar; j++) {
        if (ids[j] < 0 || ids[j] >= UCF_PAR_MOENCH_ALPHA0 + UCF_MAX_MOENCH) return fail(UCF_ERR_BAD_ARGUMENT, "ids[%d]=%d is no parameter id", j, ids[j]);
        for (int k = 0; k < j; k++)
            if (ids[k] == ids[j]) return fail(UCF_ERR_BAD_ARGUMENT, "ids[%d] and ids[%d] both name %s (duplicate id %d)", k, j, fit_par_name(ids[j], nb, sizeof(nb)), ids[j]);
        if (!fit_reads(P, ids[j]))
            return fail(UCF_ERR_BAD_ARGUMENT, "ids[%d]=%d (%s) is not read by model %d%s", j, ids[j], fit_par_name(ids[j], nb, sizeof(nb)), P.model,
                        P.model == 3 ? " with this number of Moench alphas" : (P.model == 6 ? " in this Mishra/Neuman form" : ""));
    }
    return UCF_OK;
}

// Cholesky of the n x n matrix M (row-major, overwritten by its lower factor): UCF_ERR_SINGULAR if a pivot is not positive
int fit_cholesky(int n, double* M)
{
    for (int j = 0; j < n; j++) {
        double d = M[j * n + j];
        for (int k = 0; k < j; k++) d -= M[j * n + k] * M[j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return UCF_ERR_SINGULAR;
        d = std::sqrt(d);
        M[j * n + j] = d;
        for (int i = j + 1; i < n; i++) {
            double v = M[i * n + j];
            for (int k = 0; k < j; k++) v -= M[i * n + k] * M[j * n + k];
            M[i * n + j] = v / d;
        }
    }
    return UCF_OK;
}
void fit_chol_solve(int n, const double* L, const double* b, double* x)
{
    for (int i = 0; i < n; i++) {
        double v = b[i];
        for (int k = 0; k < i; k++) v -= L[i * n + k] * x[k];
        x[i] = v / L[i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = x[i];
        for (int k = i + 1; k < n; k++) v -= L[k * n + i] * x[k];
        x[i] = v / L[i * n + i];
    }
}

// The layout of a network: per well the distinct times that observations name, ascending; the used wells grouped by their
// number of depths (groups in ascending number, wells by radius where radii are given); pt_of[i] = place of observation
// i's point among the points of one plan of its group.  The arguments have been validated.
void network_layout(int nwell, const double* well_r, const int* well_nz, int nobs, const double* t, const int* well,
                    std::vector<fit_group>& groups, std::vector<int>* grp_of, std::vector<int>* pt_of, long long* distinct_points)
{
    std::vector<std::vector<double>> times(nwell);
    for (int i = 0; i < nobs; i++) times[well[i]].push_back(t[i]);
    long long npoints = 0;
    for (auto& v : times) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        npoints += (long long)v.size();
    }
    if (distinct_points) *distinct_points = npoints;
    groups.clear();
    std::vector<int> first_pt(nwell, 0), grp_w(nwell, -1);
    for (int nz = 1; nz <= UCF_MAX_NZ; nz++) {
        fit_group G;
        G.nz = nz;
        for (int w = 0; w < nwell; w++)
            if (well_nz[w] == nz && !times[w].empty()) G.wells.push_back(w);
        if (G.wells.empty()) continue;
        if (well_r) std::stable_sort(G.wells.begin(), G.wells.end(), [&](int a, int b) { return well_r[a] < well_r[b]; });
        int nblk = 0;
        for (size_t j = 0; j < G.wells.size(); j++) {
            const int w = G.wells[j];
            const std::vector<double>& tw = times[w];
            const int nb = ((int)tw.size() + UCF_FIT_PPP - 1) / UCF_FIT_PPP;
            G.blk0.push_back(nblk);
            G.nt.push_back((int)tw.size());
            first_pt[w] = nblk * UCF_FIT_PPP;
            grp_w[w] = (int)groups.size();
            for (int b = 0; b < nb; b++) G.blk_well.push_back((int)j);
            for (int q = 0; q < nb * UCF_FIT_PPP; q++) {
                G.t.push_back(tw[q < (int)tw.size() ? q : (int)tw.size() - 1]);      // padding: the last time again
                G.r.push_back(well_r ? well_r[w] : 0.0);
            }
            nblk += nb;
        }
        G.pts = (size_t)nblk * UCF_FIT_PPP;
        G.stride = G.pts * nz;
        if (!groups.empty()) { G.pt_prefix = groups.back().pt_prefix + groups.back().pts; G.prefix = groups.back().prefix + groups.back().stride; }
        groups.push_back(std::move(G));
    }
    if (!grp_of) return;
    grp_of->resize(nobs); pt_of->resize(nobs);
    for (int i = 0; i < nobs; i++) {
        const std::vector<double>& tw = times[well[i]];
        (*grp_of)[i] = grp_w[well[i]];
        (*pt_of)[i] = first_pt[well[i]] + (int)(std::lower_bound(tw.begin(), tw.end(), t[i]) - tw.begin());
    }
}

int network_check(int nwell, const int* well_nz, int nobs, const double* t, const int* well)
{
    if (nwell < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nwell=%d: at least one well", nwell);
    if (nobs < 0 || nobs > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d: too many observations", nobs);
    if (!well_nz || (nobs > 0 && (!t || !well))) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    for (int w = 0; w < nwell; w++)
        if (well_nz[w] < 1 || well_nz[w] > UCF_MAX_NZ) return fail(UCF_ERR_BAD_ARGUMENT, "well_nz[%d]=%d outside 1..%d", w, well_nz[w], UCF_MAX_NZ);
    for (int i = 0; i < nobs; i++) {
        if (well[i] < 0 || well[i] >= nwell) return fail(UCF_ERR_BAD_ARGUMENT, "well[%d]=%d outside 0..%d", i, well[i], nwell - 1);
        if (!std::isfinite(t[i]) || !(t[i] > 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "t[%d]=%g is not a finite positive time", i, t[i]);
    }
    return UCF_OK;
}

// The geometry of a field fit (ucf_fit_field_terms states it): the virtual wells -- per observation well its distinct
// distances to the pumping wells, ascending -- and per observation its terms, one per pumping well that started before it.
struct field_geometry {
    std::vector<int> virt_well;            // per virtual well: its observation well
    std::vector<double> virt_r;            // ... and its distance, dimensional
    std::vector<int> first, pump, virt;    // first [nobs + 1]; per term: pumping well, virtual well
    std::vector<double> t;                 // per term: t[i] - t0w[j]
};

// the checks of ucf_field_create on the pumping wells, then those on the observation wells' positions
int field_check(int npump, const double* xw, const double* yw, const double* qw, const double* t0w, int nwell, const double* well_x,
                const double* well_y)
{
    if (npump < 1) return fail(UCF_ERR_BAD_ARGUMENT, "npump=%d: at least one pumping well", npump);
    if (nwell < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nwell=%d: at least one well", nwell);
    if ((long long)nwell * npump > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "%d observation wells x %d pumping wells: too many pairs", nwell, npump);
    if (!xw || !yw || !qw || !t0w || !well_x || !well_y) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    int rc;
    if ((rc = field_check_finite("xw", npump, xw)) || (rc = field_check_finite("yw", npump, yw)) || (rc = field_check_finite("qw", npump, qw)) ||
        (rc = field_check_finite("t0w", npump, t0w)) || (rc = field_check_finite("well_x", nwell, well_x)) ||
        (rc = field_check_finite("well_y", nwell, well_y))) return rc;
    for (int j = 0; j < npump; j++) {
        if (qw[j] == 0.0) return fail(UCF_ERR_BAD_ARGUMENT, "qw[%d] is 0: a well without a rate", j);
        if (!(t0w[j] >= 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "t0w[%d]=%g is negative", j, t0w[j]);
    }
    return UCF_OK;
}

// The arguments have passed field_check and network_check.  Distances as in field_group_core: every operation rounded on
// its own (host code is compiled without FMA contraction).
int field_layout(const ucf_params& P, int npump, const double* xw, const double* yw, const double* t0w, int nwell, const double* well_x,
                 const double* well_y, int nobs, const double* t, const int* well, field_geometry& F)
{
    if ((long long)nobs * npump > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "%d observations x %d pumping wells: too many terms", nobs, npump);
    std::vector<int> vmap((size_t)nwell * npump);      // virtual well of the pair (observation well, pumping well)
    std::vector<double> d(npump), u;
    for (int w = 0; w < nwell; w++) {
        for (int j = 0; j < npump; j++) {
            const double dx = well_x[w] - xw[j], dy = well_y[w] - yw[j];
            const double dist = std::sqrt(dx * dx + dy * dy);
            if (!std::isfinite(dist)) return fail(UCF_ERR_BAD_ARGUMENT, "the distance of observation well %d from pumping well %d is not finite", w, j);
            if (dist < P.rw)
                return fail(UCF_ERR_BAD_ARGUMENT, "observation well %d lies %g from pumping well %d: inside its bore (rw = %g)", w, dist, j, P.rw);
            d[j] = dist;
        }
        u = d;
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());      // (positive and finite: equal values are equal bits)
        for (int j = 0; j < npump; j++)
            vmap[(size_t)w * npump + j] = (int)F.virt_well.size() + (int)(std::lower_bound(u.begin(), u.end(), d[j]) - u.begin());
        for (double r : u) { F.virt_well.push_back(w); F.virt_r.push_back(r); }
    }
    F.first.resize((size_t)nobs + 1);
    for (int i = 0; i < nobs; i++) {
        F.first[i] = (int)F.pump.size();
        for (int j = 0; j < npump; j++)
            if (t[i] > t0w[j]) { F.pump.push_back(j); F.virt.push_back(vmap[(size_t)well[i] * npump + j]); F.t.push_back(t[i] - t0w[j]); }
    }
    F.first[nobs] = (int)F.pump.size();
    return UCF_OK;
}

// After network_check: the radii (where the wells have one: well_r may be NULL) and depths of the wells, then iz, weight and
// obs of every observation.  z0[w] = place of well w's depths in well_z, z0[nwell] = their number.
int network_check_wells(int nwell, const double* well_r, const int* well_nz, const double* well_z, int nobs, const int* well, const int* iz,
                        const double* obs, const double* weight, std::vector<int>& z0)
{
    z0.assign((size_t)nwell + 1, 0);
    int nzs = 0;
    for (int w = 0; w < nwell; w++) {
        if (well_r && (!std::isfinite(well_r[w]) || !(well_r[w] > 0.0))) return fail(UCF_ERR_BAD_ARGUMENT, "well_r[%d]=%g is not a finite positive radius", w, well_r[w]);
        z0[w] = nzs;
        for (int j = 0; j < well_nz[w]; j++)
            if (!std::isfinite(well_z[nzs + j])) return fail(UCF_ERR_BAD_ARGUMENT, "well_z[%d]=%g (depth %d of well %d) is not finite", nzs + j, well_z[nzs + j], j, w);
        nzs += well_nz[w];
    }
    z0[nwell] = nzs;
    for (int i = 0; i < nobs; i++) {
        if (iz[i] < UCF_FIT_SCREEN || iz[i] >= well_nz[well[i]])
            return fail(UCF_ERR_BAD_ARGUMENT, "iz[%d]=%d outside -1..%d (well %d)", i, iz[i], well_nz[well[i]] - 1, well[i]);
        if (!(weight[i] >= 0.0) || !std::isfinite(weight[i])) return fail(UCF_ERR_BAD_ARGUMENT, "weight[%d]=%g is negative or not finite", i, weight[i]);
        if (!std::isfinite(obs[i])) return fail(UCF_ERR_BAD_ARGUMENT, "obs[%d]=%g is not finite", i, obs[i]);
    }
    return UCF_OK;
}

// The launches of a network fit over the first nplans plans of the pool; the dimensionless h, dh stay in f->io.d_h, d_d in
// the layout of fit_group.  As multi_core: every stream the call used has drained when it returns.
int network_core(ucf_fit* f, int nplans)
{
    ucf_plan* const* plans = f->plans.data();
    multi_io& io = f->io;
    const size_t P = f->net_pts, ptot = (size_t)nplans * P;
    const int nwell = (int)f->well_nz.size(), nzs = (int)f->well_z.size();
    std::vector<double>&tD = io.tD, &rD = io.rD, &zD = io.zD;      // tD, rD, sv as uploaded; zD, zl: [nplans][all depths of all wells]
    std::vector<int>&sv = io.sv, &zl = io.zl;
    tD.resize(ptot); rD.resize(ptot); sv.resize(ptot);
    zD.resize((size_t)nplans * nzs); zl.resize((size_t)nplans * nzs);
    f->st_t.resize(P); f->st_s.resize(P);
    for (int k = 0; k < nplans; k++) {
        const ucf_derived& D = plans[k]->D;
        // the split vector of a plan is taken over all its launched times, whatever group they fall into
        for (const fit_group& G : f->groups)
            for (size_t q = 0; q < G.pts; q++) f->st_t[G.pt_prefix + q] = G.t[q] / D.Tc;
        int rc = ucf_split_vector(plans[k], (int)P, f->st_t.data(), f->st_s.data());
        if (rc) return rc;
        rc = check_sv(plans[k], (int)P, f->st_s.data());
        if (rc) return rc;
        for (const fit_group& G : f->groups) {
            const size_t at = (size_t)nplans * G.pt_prefix + (size_t)k * G.pts;
            for (size_t q = 0; q < G.pts; q++) { tD[at + q] = f->st_t[G.pt_prefix + q]; rD[at + q] = G.r[q] / D.Lc; sv[at + q] = f->st_s[G.pt_prefix + q]; }
        }
        for (int j = 0; j < nzs; j++) zD[(size_t)k * nzs + j] = f->well_z[j] / D.Lc;
        for (int w = 0; w < nwell; w++) {
            rc = ucf_zlay(plans[k], f->well_nz[w], &zD[(size_t)k * nzs + f->well_z0[w]], &zl[(size_t)k * nzs + f->well_z0[w]]);
            if (rc) return rc;
        }
    }
    HIP_TRY(hipMemcpy(io.d_t, tD.data(), sizeof(double) * ptot, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(io.d_r, rD.data(), sizeof(double) * ptot, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(io.d_s, sv.data(), sizeof(int) * ptot, hipMemcpyHostToDevice));
    const bool share = plans_share_launch(plans, nplans);
    hipStream_t streams[8];
    int ns = 0;
    int rc = UCF_OK;
    for (const fit_group& G : f->groups) {
        const int nz = G.nz, nblk = (int)G.blk_well.size();
        const size_t p0 = (size_t)nplans * G.pt_prefix, v0 = (size_t)nplans * G.prefix;
        if (share && (size_t)nplans * nblk > 1) {
            if ((size_t)nplans * G.pts > 0x7fffffffULL) return fail(UCF_ERR_BAD_ARGUMENT, "%d plans x %zu points: too many points for one call", nplans, G.pts);
            // block = (plan, tile of a well): the plan's parameter block with the well's depths and layers
            auto fill = [&](int z0, int nzc, std::vector<ucf_dev_params>& dps) {
                for (int k = 0; k < nplans; k++)
                    for (int b = 0; b < nblk; b++) {
                        const size_t zw = (size_t)k * nzs + f->well_z0[G.wells[G.blk_well[b]]] + z0;
                        int rc2 = fill_call_params(plans[k], nzc, &zD[zw], &zl[zw], dps[(size_t)k * nblk + b], nz, z0);
                        if (rc2) return rc2;
                    }
                return (int)UCF_OK;
            };
            rc = shared_launch(plans[0], nplans * nblk, UCF_FIT_PPP, nz, fill, io.dps, io.d_t + p0, io.d_r + p0, io.d_s + p0, io.d_h + v0, io.d_d + v0);
            if (rc) return rc;
            continue;
        }
        // no shared launch for these plans: plan by plan and well by well (each well has its own depths), unpadded
        if (ns == 0) ns = stream_pool(f->device, nplans, streams);
        if (ns == 0) return fail(UCF_ERR_HIP, "cannot create a HIP stream");
        for (int k = 0; k < nplans && rc == UCF_OK; k++)
            for (size_t j = 0; j < G.wells.size() && rc == UCF_OK; j++) {
                const size_t at = p0 + (size_t)k * G.pts + (size_t)G.blk0[j] * UCF_FIT_PPP;
                const size_t vat = v0 + (size_t)k * G.stride + (size_t)G.blk0[j] * UCF_FIT_PPP * nz;
                const size_t zw = (size_t)k * nzs + f->well_z0[G.wells[j]];
                rc = ucf_drawdown_batch_device(plans[k], G.nt[j], (const double*)io.d_t + at, (const double*)io.d_r + at, (const int*)io.d_s + at,
                                               nz, &zD[zw], &zl[zw], io.d_h + vat, io.d_d + vat, nullptr, streams[k % ns]);
            }
        if (rc) break;
    }
    for (int i = 0; i < ns; i++) (void)hipStreamSynchronize(streams[i]);
    return rc;
}

// the checks of a resampled call that need the fit only: before any GPU work
int fit_resample_check(const ucf_fit* f, int nsets, int nred, const int* set_of, const int* rep)
{
    if (nred < 1 || nred > (1 << 20)) return fail(UCF_ERR_BAD_ARGUMENT, "nred=%d outside 1..2^20", nred);
    if (!set_of && nred > nsets) return fail(UCF_ERR_BAD_ARGUMENT, "set_of is NULL (reduction r reads set r), but nred=%d exceeds nsets=%d", nred, nsets);
    for (int r = 0; r < nred; r++) {
        if (set_of && (set_of[r] < 0 || set_of[r] >= nsets)) return fail(UCF_ERR_BAD_ARGUMENT, "set_of[%d]=%d outside 0..%d", r, set_of[r], nsets - 1);
        if (!rep || rep[r] == -1) continue;
        if (f->nrep < 1) return fail(UCF_ERR_BAD_ARGUMENT, "rep[%d]=%d, but the fit has no multiplicities attached (ucf_fit_set_resample)", r, rep[r]);
        if (rep[r] < -1 || rep[r] >= f->nrep) return fail(UCF_ERR_BAD_ARGUMENT, "rep[%d]=%d outside -1..%d", r, rep[r], f->nrep - 1);
    }
    return UCF_OK;
}

// What one call of fit_evaluate asks for; an output that stays NULL is neither computed nor copied.
//   jac != 0: base and perturbed plans (dlog: the step of the central difference), everything.  jac == 0: the base plans only, the
//   npar = 0 reduction (the trial points of ucf_fit_lm); g, A, J, Jd are not read.
//   phi, g, A, nbad, phi_d (a fit with derivative data only) and phi_w are per set, per reduction when resampled.  phi_w is phi of
//   the weighted problem that the final factors define; a launch without factors (least squares, no ndown, b, bd) gives phi.
//   J, Jd [nsets][nobs][npar], sim_all, simd_all [nsets][plans][nobs], ndown [nsets], b, bd [nsets][nobs] are per set only.  One of
//   the last three on a least-squares fit runs the robust instantiation with every factor 1.0 (ucf_fit.h).
//   resampled (ucf_fit_set_resample): nred reductions in place of one per set; set_of NULL: the identity (nred <= nsets), rep
//   NULL: all -1 (fit_resample_check).  phi_out [nred] and counts [nred][4] are its own.
struct fit_request {
    int jac = 0;
    double dlog = 0.0;
    double *phi = nullptr, *g = nullptr, *A = nullptr, *phi_d = nullptr, *phi_w = nullptr, *phi_out = nullptr;
    double *J = nullptr, *sim_all = nullptr, *Jd = nullptr, *simd_all = nullptr, *b = nullptr, *bd = nullptr;
    int *nbad = nullptr, *ndown = nullptr, *counts = nullptr;
    bool resampled = false;
    int nred = 0;
    const int *set_of = nullptr, *rep = nullptr;
};
// the sizes of one call: plans per set and in all; workgroups of the reduction, what sums, nbad and counts are indexed by; bytes
// of J (Jd), sim_all (simd_all), b (bd)
struct fit_shape {
    int nsets, per, nplans, nout;
    size_t bJ, bsim, bfac;
};

// 1. the arguments, before any GPU work
int fit_check_request(const ucf_fit* f, int nsets, const double* theta, const fit_request& q, fit_shape& sh)
{
    if (!f || !theta) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (nsets < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nsets=%d: at least one parameter set", nsets);
    int rc = q.resampled ? fit_resample_check(f, nsets, q.nred, q.set_of, q.rep) : UCF_OK;
    if (rc) return rc;
    if (q.jac && (!(q.dlog > 0.0) || !std::isfinite(q.dlog))) return fail(UCF_ERR_BAD_ARGUMENT, "dlog=%g must be positive and finite", q.dlog);
    const int npar = f->npar, per = q.jac ? 1 + 2 * npar : 1;
    if ((long long)nsets * per > (1 << 20)) return fail(UCF_ERR_BAD_ARGUMENT, "%d sets x %d plans: too many plans for one call", nsets, per);
    char nb[32];
    for (int s = 0; s < nsets; s++)
        for (int j = 0; j < npar; j++) {
            const double v = theta[(size_t)s * npar + j];
            if (!(v > 0.0) || !std::isfinite(v))
                return fail(UCF_ERR_BAD_ARGUMENT, "set %d: %s=%g must be positive and finite (parameters are fitted in their logarithm)", s,
                            fit_par_name(f->ids[j], nb, sizeof(nb)), v);
        }
    const size_t so = sizeof(double) * (size_t)f->nobs;
    sh = fit_shape{nsets, per, nsets * per, q.resampled ? q.nred : nsets, so * nsets * npar, so * nsets * per, so * nsets};
    return UCF_OK;
}

// 2. the plans of the pool: refreshed in place, made on first use
int fit_refresh_plans(ucf_fit* f, const double* theta, double dlog, const fit_shape& sh)
{
    const int npar = f->npar, per = sh.per;
    char nb[32];
    std::vector<ucf_params> sets(per);
    for (int s = 0; s < sh.nsets; s++) {
        int rc = fit_theta_sets(f->base, npar, f->ids, theta + (size_t)s * npar, dlog, per, sets.data());
        if (rc) return rc;
        for (int v = 0; v < per; v++) {
            const size_t k = (size_t)s * per + v;
            if (k < f->plans.size()) {
                rc = ucf_plan_update(f->plans[k], &sets[v]);
            } else {
                ucf_plan* pl = nullptr;
                rc = ucf_plan_create(&sets[v], &pl);
                if (rc == UCF_OK) { (void)ucf_plan_set_mode(pl, 1); f->plans.push_back(pl); f->n_alloc++; }
            }
            if (rc == UCF_OK) continue;
            std::string why = ucf_last_error();
            if (v == 0) return fail(rc, "set %d: %s", s, why.c_str());
            return fail(rc, "set %d, %s moved by %+g in its logarithm: %s", s, fit_par_name(f->ids[(v - 1) / 2], nb, sizeof(nb)), (v & 1) ? dlog : -dlog, why.c_str());
        }
    }
    return UCF_OK;
}

// 3. The reduction as its launcher sees it (ucf_fit.h), before the buffers grow: which arrays a launch has decides its
// instantiation and so the layout of its sums, and that layout sizes b_sums.  Everything is filled in but the addresses that
// growth may move.  In their place an array that a launch may go without -- d_dh, the outputs and index lists of the request --
// is non-NULL where this one will have it (a host address that nothing reads through); fit_grow puts the buffer's there.
ucf_fit_reduce_args fit_reduce_asked(const ucf_fit* f, const double* theta, const fit_request& q, const fit_shape& sh)
{
    ucf_fit_reduce_args ra = {};
    ra.npar = q.jac ? f->npar : 0; ra.nsets = sh.nsets; ra.nobs = f->nobs;
    ra.nplans = (size_t)sh.nplans; ra.plan_stride = (size_t)f->nobs * f->nz; ra.two_dlog = 2.0 * q.dlog;
    ra.source = f->kind;
    ra.d_slot = (const int*)f->b_slot.p; ra.d_ref = (const ucf_fit_obs_ref*)f->b_ref.p;
    ra.d_term = (const ucf_fit_term*)f->b_term.p; ra.d_first = (const int*)f->b_first.p; ra.d_tfac = (const double*)f->b_tfac.p;
    ra.d_obs = (const double*)f->b_obs.p; ra.d_w = (const double*)f->b_w.p;
    ra.d_dobs = (const double*)f->b_dobs.p; ra.d_wd = (const double*)f->b_wd.p;
    ra.loss = f->loss; ra.loss_c = f->loss_c;
    ra.d_dh = f->deriv ? theta : nullptr;
    ra.d_J = q.J; ra.d_sim = q.sim_all; ra.d_Jd = q.Jd; ra.d_simd = q.simd_all; ra.d_ndown = q.ndown; ra.d_b = q.b; ra.d_bd = q.bd;
    if (q.resampled) {
        ra.nred = sh.nout; ra.d_mult = f->nrep > 0 ? (const unsigned short*)f->b_mult.p : nullptr;
        ra.d_set_of = q.set_of; ra.d_rep = q.rep;
    }
    return ra;
}

// 4. the buffers, grown on demand, and their addresses to where the evaluators (f->io) and the reduction (ra) read them: what
// every evaluation has, then what this one will have; nsum doubles of sums per workgroup
template <class T>
int fit_grow_to(ucf_fit* f, T*& at, ucf_buffer& b, size_t bytes, const char* what)
{
    int rc = grow_buffer(b, bytes, what, f->n_alloc);
    at = (T*)b.p;
    return rc;
}
int fit_grow(ucf_fit* f, ucf_fit_reduce_args& ra, const fit_shape& sh, size_t nsum)
{
    // points and (point, depth) values that are launched: every depth at every observation, or the network's blocks
    const size_t np_ = (size_t)f->nobs, nplans = (size_t)sh.nplans, nout = (size_t)sh.nout;
    const size_t ptot = nplans * (f->is_network() ? f->net_pts : np_), vtot = nplans * (f->is_network() ? f->net_vals : np_ * f->nz);
    multi_io& io = f->io;
    int rc;
    if ((rc = fit_grow_to(f, io.d_t, f->b_t, sizeof(double) * ptot, "tD")) || (rc = fit_grow_to(f, io.d_r, f->b_r, sizeof(double) * ptot, "rD")) ||
        (rc = fit_grow_to(f, io.d_s, f->b_s, sizeof(int) * ptot, "sv")) || (rc = fit_grow_to(f, io.d_h, f->b_h, sizeof(double) * vtot, "h")) ||
        (rc = fit_grow_to(f, io.d_d, f->b_d, sizeof(double) * vtot, "dh")) || (rc = fit_grow_to(f, ra.d_Hc, f->b_hc, sizeof(double) * nplans, "Hc")) ||
        (rc = fit_grow_to(f, ra.d_sums, f->b_sums, sizeof(double) * nout * nsum, "sums")) || (rc = fit_grow_to(f, ra.d_nbad, f->b_nbad, sizeof(int) * nout, "nbad")))
        return rc;
    ra.d_h = io.d_h;
    if (ra.d_dh) ra.d_dh = io.d_d;
    if (ucf_fit_reduce_is_resampled(&ra) && ((rc = fit_grow_to(f, ra.d_counts, f->b_counts, sizeof(int) * 4 * nout, "counts")) ||
                                             (ra.d_set_of && (rc = fit_grow_to(f, ra.d_set_of, f->b_setof, sizeof(int) * nout, "set_of"))) ||
                                             (ra.d_rep && (rc = fit_grow_to(f, ra.d_rep, f->b_rep, sizeof(int) * nout, "rep")))))
        return rc;
    if ((ra.d_J && (rc = fit_grow_to(f, ra.d_J, f->b_J, sh.bJ, "J"))) || (ra.d_sim && (rc = fit_grow_to(f, ra.d_sim, f->b_sim, sh.bsim, "sim_all"))) ||
        (ra.d_Jd && (rc = fit_grow_to(f, ra.d_Jd, f->b_Jd, sh.bJ, "Jd"))) || (ra.d_simd && (rc = fit_grow_to(f, ra.d_simd, f->b_simd, sh.bsim, "simd_all"))) ||
        (ra.d_ndown && (rc = fit_grow_to(f, ra.d_ndown, f->b_ndown, sizeof(int) * sh.nsets, "ndown"))) ||
        (ra.d_b && (rc = fit_grow_to(f, ra.d_b, f->b_bfac, sh.bfac, "b"))) || (ra.d_bd && (rc = fit_grow_to(f, ra.d_bd, f->b_bdfac, sh.bfac, "bd"))))
        return rc;
    return UCF_OK;
}

// 5. the evaluations: the dimensionless h and dh of every plan stay in b_h and b_d, their scales go to b_hc
int fit_simulate(ucf_fit* f, int nplans)
{
    f->last_nplans = 0;
    int rc = f->is_network() ? network_core(f, nplans) : multi_core(f->plans.data(), nplans, f->nobs, f->t_s.data(), f->r_s.data(), f->nz, f->z.data(), f->io);
    if (rc) return rc;
    f->last_nplans = nplans;
    f->h_hc.resize(nplans);
    for (int k = 0; k < nplans; k++) f->h_hc[k] = f->plans[k]->D.Hc;
    HIP_TRY(hipMemcpy(f->b_hc.p, f->h_hc.data(), sizeof(double) * nplans, hipMemcpyHostToDevice));
    return UCF_OK;
}

// 6. the launch, and what was asked for on its way back (the sums to f->h_sums, nsum doubles per workgroup)
int fit_reduce(ucf_fit* f, const fit_request& q, const ucf_fit_reduce_args& ra, const fit_shape& sh, size_t nsum)
{
    const size_t nout = (size_t)sh.nout;
    if (ra.d_set_of) HIP_TRY(hipMemcpy(f->b_setof.p, q.set_of, sizeof(int) * nout, hipMemcpyHostToDevice));
    if (ra.d_rep) HIP_TRY(hipMemcpy(f->b_rep.p, q.rep, sizeof(int) * nout, hipMemcpyHostToDevice));
    int rc = ucf_fit_launch_reduce(&ra, nullptr);
    if (rc) return fail(rc, "fit reduction kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    f->h_sums.resize(nout * nsum);
    return copy_back_sync({{f->h_sums.data(), ra.d_sums, sizeof(double) * nout * nsum}, {q.nbad, ra.d_nbad, sizeof(int) * nout},
                           {q.counts, ra.d_counts, sizeof(int) * 4 * nout}, {q.J, ra.d_J, sh.bJ}, {q.sim_all, ra.d_sim, sh.bsim}, {q.Jd, ra.d_Jd, sh.bJ},
                           {q.simd_all, ra.d_simd, sh.bsim}, {q.ndown, ra.d_ndown, sizeof(int) * sh.nsets}, {q.b, ra.d_b, sh.bfac}, {q.bd, ra.d_bd, sh.bfac}});
}

// 7. f->h_sums to the outputs of the request, through the layout that the launch wrote them in
void fit_unpack(const ucf_fit* f, const fit_request& q, const ucf_fit_sums_layout& at, int nout, int npar)
{
    for (int s = 0; s < nout; s++) {
        const double* v = &f->h_sums[(size_t)s * at.count];
        if (q.phi) q.phi[s] = v[at.phi];
        if (q.phi_d && at.phi_d >= 0) q.phi_d[s] = v[at.phi_d];
        if (q.phi_w) q.phi_w[s] = v[at.phi_w >= 0 ? at.phi_w : at.phi];      // least squares: every factor is 1.0
        if (q.phi_out) q.phi_out[s] = v[at.phi_out];
        if (q.g) for (int j = 0; j < npar; j++) q.g[(size_t)s * npar + j] = v[at.g + j];
        if (!q.A) continue;
        const double* a = v + at.A;
        for (int j = 0; j < npar; j++)
            for (int k = j; k < npar; k++) q.A[((size_t)s * npar + j) * npar + k] = q.A[((size_t)s * npar + k) * npar + j] = *a++;
    }
}

// On a fit with derivative data the sums are the joint ones and phi_d, Jd, simd_all may be asked for.  The fit's loss and what is
// asked for decide the instantiation; a least-squares fit asked for none of ndown, b, bd runs as a fit without a loss.
int fit_evaluate(ucf_fit* f, int nsets, const double* theta, fit_request q)
{
    if (!q.jac) q.g = q.A = q.J = q.Jd = nullptr;
    if (!q.resampled) { q.phi_out = nullptr; q.counts = nullptr; }
    fit_shape sh;
    int rc = fit_check_request(f, nsets, theta, q, sh);
    if (rc) return rc;
    device_switch dg(f->device);
    if ((rc = fit_refresh_plans(f, theta, q.dlog, sh))) return rc;
    ucf_fit_reduce_args ra = fit_reduce_asked(f, theta, q, sh);
    const ucf_fit_sums_layout at = ucf_fit_sums_of(&ra);
    if ((rc = fit_grow(f, ra, sh, (size_t)at.count)) || (rc = fit_simulate(f, sh.nplans)) || (rc = fit_reduce(f, q, ra, sh, (size_t)at.count))) return rc;
    fit_unpack(f, q, at, sh.nout, ra.npar);
    return UCF_OK;
}

// ---- what the three ucf_fit_create* share
// the opening: checks that do not depend on the kind of fit, in the order every kind makes them
int fit_create_check(const ucf_params* base, int npar, const int* ids, int nobs, ucf_fit** out)
{
    if (out) *out = nullptr;
    if (!base || !out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = validate(*base);
    if (rc) return rc;
    rc = fit_check_ids(*base, npar, ids);
    if (rc) return rc;
    if (nobs < npar) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d: fewer observations than the %d parameters to fit", nobs, npar);
    return UCF_OK;
}

// after the checks of the kind: the device, then the fit with what every kind sets
int fit_new(const ucf_params* base, int npar, const int* ids, int nobs, int nz, int device, ucf_fit_source kind, ucf_fit** f_out)
{
    int ndev = 0;
    int rc = ucf_device_count(&ndev);
    if (rc) return rc;
    if (device < 0 || device >= ndev) return fail(UCF_ERR_BAD_ARGUMENT, "device %d does not exist (%d visible)", device, ndev);
    ucf_fit* f = new (std::nothrow) ucf_fit();
    if (!f) return fail(UCF_ERR_NOMEM, "host allocation failed");
    f->base = *base; f->npar = npar; f->nobs = nobs; f->nz = nz; f->device = device; f->kind = kind;
    for (int j = 0; j < npar; j++) f->ids[j] = ids[j];
    *f_out = f;
    return UCF_OK;
}

// the closing: the buffers that are fixed at create, in the order given, and their contents; the fit is destroyed on failure
struct fit_upload {
    ucf_buffer* b;
    const void* from;
    size_t bytes;
    const char* what;
};
int fit_create_upload(ucf_fit* f, std::initializer_list<fit_upload> ups, ucf_fit** out)
{
    device_switch dg(f->device);
    for (const fit_upload& u : ups) {
        int rc = grow_buffer(*u.b, u.bytes, u.what, f->n_alloc);
        if (rc) { ucf_fit_destroy(f); return rc; }
    }
    for (const fit_upload& u : ups)
        if (hipMemcpy(u.b->p, u.from, u.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            ucf_fit_destroy(f);
            return fail(UCF_ERR_HIP, "upload of the observations failed");
        }
    *out = f;
    return UCF_OK;
}

// The network of f's wells (well_r, well_nz, well_z are set) over n places (t[k] in well[k], depth iz[k] or the screen):
// the groups, what a plan launches and f->refs, one per place -- the observations of a network fit, the terms of a field fit.
void fit_network_places(ucf_fit* f, int n, const double* t, const int* well, const int* iz)
{
    std::vector<int> grp_of, pt_of;
    long long npoints = 0;
    network_layout((int)f->well_nz.size(), f->well_r.data(), f->well_nz.data(), n, t, well, f->groups, &grp_of, &pt_of, &npoints);
    f->net_pts = f->groups.back().pt_prefix + f->groups.back().pts;
    f->net_vals = f->groups.back().prefix + f->groups.back().stride;
    f->dense = npoints * (long long)f->well_z.size();
    f->refs.resize(n);
    for (int k = 0; k < n; k++) {
        const fit_group& G = f->groups[grp_of[k]];
        const bool screen = iz[k] == UCF_FIT_SCREEN;
        f->refs[k] = ucf_fit_obs_ref{(long long)G.prefix, (long long)G.stride, pt_of[k] * G.nz + (screen ? 0 : iz[k]), screen ? G.nz : 1};
    }
}
}  // namespace

int ucf_host::fit_cholesky_factor(int n, double* M) { return fit_cholesky(n, M); }

extern "C" {

int ucf_fit_perturb(const ucf_params* base, int npar, const int* ids, const double* theta, ucf_params* out)
{
    if (!base || !theta || !out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = fit_check_ids(*base, npar, ids);
    if (rc) return rc;
    ucf_params P = *base;
    for (int j = 0; j < npar; j++) *fit_field(P, ids[j]) = theta[j];
    *out = P;
    return UCF_OK;
}

int ucf_fit_solve_step(int npar, const double* A, const double* g, double lambda, double* step)
{
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!A || !g || !step) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(UCF_ERR_BAD_ARGUMENT, "lambda=%g must be >= 0 and finite", lambda);
    double M[UCF_FIT_MAX_PAR * UCF_FIT_MAX_PAR];
    for (int i = 0; i < npar; i++)
        for (int k = 0; k < npar; k++) M[i * npar + k] = A[i * npar + k];
    for (int i = 0; i < npar; i++) M[i * npar + i] = A[i * npar + i] + lambda * A[i * npar + i];
    for (int i = 0; i < npar; i++) step[i] = 0.0;
    if (fit_cholesky(npar, M) != UCF_OK) return fail(UCF_ERR_SINGULAR, "A + %g diag A is not positive definite (%d x %d)", lambda, npar, npar);
    fit_chol_solve(npar, M, g, step);
    for (int i = 0; i < npar; i++)
        if (!std::isfinite(step[i])) {
            for (int k = 0; k < npar; k++) step[k] = 0.0;
            return fail(UCF_ERR_SINGULAR, "A + %g diag A is singular to working precision (%d x %d)", lambda, npar, npar);
        }
    return UCF_OK;
}

int ucf_fit_create(const ucf_params* base, int npar, const int* ids, int nobs, const double* t, const double* r, const int* iz,
                   int nz, const double* z, const double* obs, const double* weight, int device, ucf_fit** out)
{
    int rc = fit_create_check(base, npar, ids, nobs, out);
    if (rc) return rc;
    if (nobs > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d: too many observations", nobs);
    if (nz < 1 || nz > 4096) return fail(UCF_ERR_BAD_ARGUMENT, "nz=%d: at least one depth (at most 4096)", nz);
    if (!t || !r || !iz || !z || !obs || !weight) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    for (int j = 0; j < nz; j++)
        if (!std::isfinite(z[j])) return fail(UCF_ERR_BAD_ARGUMENT, "z[%d]=%g is not finite", j, z[j]);
    for (int i = 0; i < nobs; i++) {
        if (iz[i] < 0 || iz[i] >= nz) return fail(UCF_ERR_BAD_ARGUMENT, "iz[%d]=%d outside 0..%d", i, iz[i], nz - 1);
        if (!(weight[i] >= 0.0) || !std::isfinite(weight[i])) return fail(UCF_ERR_BAD_ARGUMENT, "weight[%d]=%g is negative or not finite", i, weight[i]);
        if (!std::isfinite(obs[i])) return fail(UCF_ERR_BAD_ARGUMENT, "obs[%d]=%g is not finite", i, obs[i]);
        if (!std::isfinite(t[i]) || !(t[i] > 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "t[%d]=%g is not a finite positive time", i, t[i]);
        if (!std::isfinite(r[i]) || !(r[i] > 0.0)) return fail(UCF_ERR_BAD_ARGUMENT, "r[%d]=%g is not a finite positive radius", i, r[i]);
    }
    ucf_fit* f = nullptr;
    rc = fit_new(base, npar, ids, nobs, nz, device, UCF_FIT_SLOTS, &f);
    if (rc) return rc;
    // the core evaluates in order of radius (see ucf_drawdown_batch): the observations are ordered once, here
    std::vector<int> perm(nobs);
    for (int i = 0; i < nobs; i++) perm[i] = i;
    std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return r[x] < r[y]; });
    f->t_s.resize(nobs); f->r_s.resize(nobs); f->z.assign(z, z + nz);
    std::vector<int> slot(nobs);
    for (int i = 0; i < nobs; i++) { f->t_s[i] = t[perm[i]]; f->r_s[i] = r[perm[i]]; slot[perm[i]] = i * nz + iz[perm[i]]; }
    f->refs.resize(nobs);
    for (int i = 0; i < nobs; i++) f->refs[i] = ucf_fit_obs_ref{0, (long long)nobs * nz, slot[i], 1};
    f->dense = (long long)nobs * nz;
    return fit_create_upload(f, {{&f->b_slot, slot.data(), sizeof(int) * nobs, "observation places"},
                                 {&f->b_obs, obs, sizeof(double) * nobs, "observations"},
                                 {&f->b_w, weight, sizeof(double) * nobs, "weights"}}, out);
}

void ucf_fit_destroy(ucf_fit* f)
{
    if (!f) return;
    for (ucf_plan* pl : f->plans) ucf_plan_destroy(pl);
    {
        device_switch dg(f->device);
        for (ucf_buffer* b : f->buffers()) free_buffer(*b);
    }
    delete f;
}

int ucf_fit_create_network(const ucf_params* base, int npar, const int* ids, int nwell, const double* well_r, const int* well_nz,
                           const double* well_z, int nobs, const double* t, const int* well, const int* iz, const double* obs,
                           const double* weight, int device, ucf_fit** out)
{
    int rc = fit_create_check(base, npar, ids, nobs, out);
    if (rc) return rc;
    if (!well_r || !well_z || !iz || !obs || !weight) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    rc = network_check(nwell, well_nz, nobs, t, well);
    if (rc) return rc;
    std::vector<int> z0;
    rc = network_check_wells(nwell, well_r, well_nz, well_z, nobs, well, iz, obs, weight, z0);
    if (rc) return rc;
    const int nzs = z0[nwell];
    ucf_fit* f = nullptr;
    rc = fit_new(base, npar, ids, nobs, 0, device, UCF_FIT_NETWORK, &f);
    if (rc) return rc;
    f->well_r.assign(well_r, well_r + nwell); f->well_nz.assign(well_nz, well_nz + nwell);
    f->well_z.assign(well_z, well_z + nzs); f->well_z0.assign(z0.begin(), z0.begin() + nwell);
    fit_network_places(f, nobs, t, well, iz);
    return fit_create_upload(f, {{&f->b_ref, f->refs.data(), sizeof(ucf_fit_obs_ref) * nobs, "observation places"},
                                 {&f->b_obs, obs, sizeof(double) * nobs, "observations"},
                                 {&f->b_w, weight, sizeof(double) * nobs, "weights"}}, out);
}

int ucf_fit_create_field(const ucf_params* base, int npar, const int* ids, int npump, const double* xw, const double* yw, const double* qw,
                         const double* t0w, int nwell, const double* well_x, const double* well_y, const int* well_nz, const double* well_z,
                         int nobs, const double* t, const int* well, const int* iz, const double* obs, const double* weight, int device,
                         ucf_fit** out)
{
    int rc = fit_create_check(base, npar, ids, nobs, out);
    if (rc) return rc;
    if (!well_z || !iz || !obs || !weight) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    rc = field_check(npump, xw, yw, qw, t0w, nwell, well_x, well_y);
    if (rc) return rc;
    rc = network_check(nwell, well_nz, nobs, t, well);
    if (rc) return rc;
    std::vector<int> z0;
    rc = network_check_wells(nwell, nullptr, well_nz, well_z, nobs, well, iz, obs, weight, z0);
    if (rc) return rc;
    field_geometry F;
    rc = field_layout(*base, npump, xw, yw, t0w, nwell, well_x, well_y, nobs, t, well, F);
    if (rc) return rc;
    const int nvirt = (int)F.virt_well.size(), nterm = (int)F.pump.size();
    if (nterm < 1) return fail(UCF_ERR_BAD_ARGUMENT, "no observation lies after the start of a pumping well: nothing to fit");
    ucf_fit* f = nullptr;
    rc = fit_new(base, npar, ids, nobs, 0, device, UCF_FIT_FIELD, &f);
    if (rc) return rc;
    // the network of the virtual wells: each carries the depths of its observation well
    f->well_r = F.virt_r;
    f->well_nz.resize(nvirt); f->well_z0.resize(nvirt);
    for (int v = 0; v < nvirt; v++) {
        const int w = F.virt_well[v];
        f->well_nz[v] = well_nz[w];
        f->well_z0[v] = (int)f->well_z.size();
        f->well_z.insert(f->well_z.end(), well_z + z0[w], well_z + z0[w] + well_nz[w]);
    }
    // a term is a place of that network: the time since its pumping well started, at the depth of its observation
    f->term_t = F.t;
    f->term_tobs.resize(nterm);
    std::vector<int> term_iz(nterm);
    for (int i = 0; i < nobs; i++)
        for (int k = F.first[i]; k < F.first[i + 1]; k++) { f->term_tobs[k] = t[i]; term_iz[k] = iz[i]; }
    fit_network_places(f, nterm, F.t.data(), F.virt.data(), term_iz.data());
    std::vector<ucf_fit_term> terms(nterm);
    for (int k = 0; k < nterm; k++) terms[k] = ucf_fit_term{f->refs[k], qw[F.pump[k]]};
    return fit_create_upload(f, {{&f->b_term, terms.data(), sizeof(ucf_fit_term) * nterm, "terms"},
                                 {&f->b_first, F.first.data(), sizeof(int) * ((size_t)nobs + 1), "term lists"},
                                 {&f->b_obs, obs, sizeof(double) * nobs, "observations"},
                                 {&f->b_w, weight, sizeof(double) * nobs, "weights"}}, out);
}

int ucf_fit_field_terms(const ucf_params* base, int npump, const double* xw, const double* yw, const double* qw, const double* t0w, int nwell,
                        const double* well_x, const double* well_y, int nobs, const double* t, const int* well, int* nvirt, int* virt_well,
                        double* virt_r, int* term_first, int* term_pump, int* term_virt, double* term_t)
{
    if (!base) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = validate(*base);
    if (rc) return rc;
    rc = field_check(npump, xw, yw, qw, t0w, nwell, well_x, well_y);
    if (rc) return rc;
    const std::vector<int> one(nwell, 1);      // the depths play no part in the geometry
    rc = network_check(nwell, one.data(), nobs, t, well);
    if (rc) return rc;
    field_geometry F;
    rc = field_layout(*base, npump, xw, yw, t0w, nwell, well_x, well_y, nobs, t, well, F);
    if (rc) return rc;
    if (nvirt) *nvirt = (int)F.virt_well.size();
    if (virt_well) std::copy(F.virt_well.begin(), F.virt_well.end(), virt_well);
    if (virt_r) std::copy(F.virt_r.begin(), F.virt_r.end(), virt_r);
    if (term_first) std::copy(F.first.begin(), F.first.end(), term_first);
    if (term_pump) std::copy(F.pump.begin(), F.pump.end(), term_pump);
    if (term_virt) std::copy(F.virt.begin(), F.virt.end(), term_virt);
    if (term_t) std::copy(F.t.begin(), F.t.end(), term_t);
    return UCF_OK;
}

int ucf_fit_eval_counts(const ucf_fit* f, long long* launched, long long* dense)
{
    if (!f || !launched || !dense) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *launched = f->is_network() ? (long long)f->net_vals : f->dense;
    *dense = f->dense;
    return UCF_OK;
}

int ucf_fit_network_eval_counts(int nwell, const int* well_nz, int nobs, const double* t, const int* well, long long* launched,
                                long long* dense)
{
    if (!launched || !dense) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = network_check(nwell, well_nz, nobs, t, well);
    if (rc) return rc;
    std::vector<fit_group> groups;
    long long npoints = 0, nzs = 0;
    network_layout(nwell, nullptr, well_nz, nobs, t, well, groups, nullptr, nullptr, &npoints);
    for (int w = 0; w < nwell; w++) nzs += well_nz[w];
    *launched = groups.empty() ? 0 : (long long)(groups.back().prefix + groups.back().stride);
    *dense = npoints * nzs;
    return UCF_OK;
}

// ucf_fit_debug_h / ucf_fit_debug_dh: b_h and b_d have one layout
static int fit_debug_read(ucf_fit* f, bool dh, int plan, int i, int cap, double* h, int* n)
{
    if (!f || !h || !n) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (f->last_nplans < 1) return fail(UCF_ERR_BAD_ARGUMENT, "no evaluation to read from");
    if (plan < 0 || plan >= f->last_nplans) return fail(UCF_ERR_BAD_ARGUMENT, "plan %d outside 0..%d", plan, f->last_nplans - 1);
    const char* what = f->kind == UCF_FIT_FIELD ? "term" : "observation";      // a field fit has one place per term
    if (i < 0 || i >= (int)f->refs.size()) return fail(UCF_ERR_BAD_ARGUMENT, "%s %d outside 0..%d", what, i, (int)f->refs.size() - 1);
    const ucf_fit_obs_ref& o = f->refs[i];
    if (cap < o.count) return fail(UCF_ERR_BAD_ARGUMENT, "cap=%d: %s %d reads %d values", cap, what, i, o.count);
    device_switch dg(f->device);
    const size_t at = (size_t)o.prefix * f->last_nplans + (size_t)plan * o.stride + o.at;
    HIP_TRY(hipMemcpy(h, (const double*)(dh ? f->b_d.p : f->b_h.p) + at, sizeof(double) * o.count, hipMemcpyDeviceToHost));
    *n = o.count;
    return UCF_OK;
}

int ucf_fit_debug_h(ucf_fit* f, int plan, int i, int cap, double* h, int* n) { return fit_debug_read(f, false, plan, i, cap, h, n); }
int ucf_fit_debug_dh(ucf_fit* f, int plan, int i, int cap, double* dh, int* n) { return fit_debug_read(f, true, plan, i, cap, dh, n); }

int ucf_fit_derivative_check(int nobs, const double* dobs, const double* dweight, int* nd)
{
    if (nd) *nd = 0;
    if (nobs < 0) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d is negative", nobs);
    if (!dobs) return fail(UCF_ERR_BAD_ARGUMENT, "dobs is NULL");
    if (!dweight) return fail(UCF_ERR_BAD_ARGUMENT, "dweight is NULL");
    if (!nd) return fail(UCF_ERR_BAD_ARGUMENT, "nd is NULL");
    int count = 0;
    for (int i = 0; i < nobs; i++) {
        if (!(dweight[i] >= 0.0) || !std::isfinite(dweight[i])) return fail(UCF_ERR_BAD_ARGUMENT, "dweight[%d]=%g is negative or not finite", i, dweight[i]);
        if (dweight[i] > 0.0) {
            if (!std::isfinite(dobs[i])) return fail(UCF_ERR_BAD_ARGUMENT, "dobs[%d]=%g is not finite (dweight[%d]=%g)", i, dobs[i], i, dweight[i]);
            count++;
        }
    }
    *nd = count;
    return UCF_OK;
}

int ucf_fit_set_derivative(ucf_fit* f, const double* dobs, const double* dweight)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (!dobs && !dweight) { f->deriv = false; f->nd = 0; return UCF_OK; }
    int nd = 0;
    int rc = ucf_fit_derivative_check(f->nobs, dobs, dweight, &nd);
    if (rc) return rc;
    device_switch dg(f->device);
    const size_t nobs = (size_t)f->nobs, nterm = f->term_t.size();
    if ((rc = grow_buffer(f->b_dobs, sizeof(double) * nobs, "derivative observations", f->n_alloc)) ||
        (rc = grow_buffer(f->b_wd, sizeof(double) * nobs, "derivative weights", f->n_alloc)))
        return rc;
    f->deriv = false;                      // until everything is in place
    HIP_TRY(hipMemcpy(f->b_dobs.p, dobs, sizeof(double) * nobs, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(f->b_wd.p, dweight, sizeof(double) * nobs, hipMemcpyHostToDevice));
    if (f->kind == UCF_FIT_FIELD) {
        // tfac of ucf_field_group, per term: the observation's own time over the term's time, one division
        std::vector<double> tfac(nterm);
        for (size_t k = 0; k < nterm; k++) tfac[k] = f->term_tobs[k] / f->term_t[k];
        if ((rc = grow_buffer(f->b_tfac, sizeof(double) * nterm, "term time factors", f->n_alloc))) return rc;
        HIP_TRY(hipMemcpy(f->b_tfac.p, tfac.data(), sizeof(double) * nterm, hipMemcpyHostToDevice));
    }
    f->deriv = true;
    f->nd = nd;
    return UCF_OK;
}

long long ucf_fit_alloc_count(const ucf_fit* f)
{
    if (!f) return 0;
    long long n = f->n_alloc;
    for (const ucf_plan* pl : f->plans) n += ucf_plan_alloc_count(pl);
    return n;
}

int ucf_fit_evaluate(ucf_fit* f, int nsets, const double* theta, double dlog, double* phi, double* g, double* A, int* nbad, double* J,
                     double* sim_all)
{
    fit_request q;
    q.jac = 1; q.dlog = dlog; q.phi = phi; q.g = g; q.A = A; q.nbad = nbad; q.J = J; q.sim_all = sim_all;
    return fit_evaluate(f, nsets, theta, q);
}

int ucf_fit_evaluate_joint(ucf_fit* f, int nsets, const double* theta, double dlog, double* phi, double* g, double* A, int* nbad, double* J,
                           double* sim_all, double* phi_d, double* Jd, double* simd_all)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (!f->deriv) return fail(UCF_ERR_BAD_ARGUMENT, "the fit has no derivative data (ucf_fit_set_derivative)");
    fit_request q;
    q.jac = 1; q.dlog = dlog; q.phi = phi; q.g = g; q.A = A; q.nbad = nbad; q.J = J; q.sim_all = sim_all;
    q.phi_d = phi_d; q.Jd = Jd; q.simd_all = simd_all;
    return fit_evaluate(f, nsets, theta, q);
}

// the trial-point evaluation of ucf_fit_lm with an entry of its own: base plans only, the npar = 0 reduction; dlog is not read
int ucf_fit_objective(ucf_fit* f, int nsets, const double* theta, double* phi, int* nbad, double* sim, double* phi_d, double* simd)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if ((phi_d || simd) && !f->deriv)
        return fail(UCF_ERR_BAD_ARGUMENT, "%s is asked for, but the fit has no derivative data (ucf_fit_set_derivative)", phi_d ? "phi_d" : "simd");
    fit_request q;
    q.phi = phi; q.nbad = nbad; q.sim_all = sim; q.phi_d = phi_d; q.simd_all = simd;
    return fit_evaluate(f, nsets, theta, q);
}

// ---- robust losses (include/ucf.h states the arithmetic; this file is compiled without contraction)
static int loss_check(int kind, double c)
{
    if (kind != UCF_LOSS_L2 && kind != UCF_LOSS_HUBER && kind != UCF_LOSS_TUKEY)
        return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d is no loss (UCF_LOSS_L2 0, UCF_LOSS_HUBER 1, UCF_LOSS_TUKEY 2)", kind);
    if (kind != UCF_LOSS_L2 && (!(c > 0.0) || !std::isfinite(c))) return fail(UCF_ERR_BAD_ARGUMENT, "c=%g must be positive and finite", c);
    return UCF_OK;
}

int ucf_fit_loss_terms(int kind, double c, int n, const double* x, double* rho, double* b)
{
    int rc = loss_check(kind, c);
    if (rc) return rc;
    if (n < 0) return fail(UCF_ERR_BAD_ARGUMENT, "n=%d is negative", n);
    if (!x || !rho || !b) return fail(UCF_ERR_BAD_ARGUMENT, "NULL x, rho or b");
    const double c2 = c * c;
    for (int i = 0; i < n; i++) {
        const double xi = x[i], a = std::fabs(xi);
        if (kind == UCF_LOSS_L2) { b[i] = 1.0; rho[i] = xi * xi; }
        else if (kind == UCF_LOSS_HUBER) {
            if (a <= c) { b[i] = 1.0; rho[i] = xi * xi; }
            else { b[i] = c / a; rho[i] = c * (2.0 * a - c); }
        } else {
            const double u = xi / c;
            if (a < c) { const double v = 1.0 - u * u; b[i] = v * v; rho[i] = (c2 * (1.0 - b[i] * v)) / 3.0; }
            else { b[i] = 0.0; rho[i] = c2 / 3.0; }
        }
    }
    return UCF_OK;
}

int ucf_fit_robust_scale(int n, const double* x, double* scale)
{
    if (n < 1) return fail(UCF_ERR_BAD_ARGUMENT, "n=%d: at least one residual", n);
    if (!x || !scale) return fail(UCF_ERR_BAD_ARGUMENT, "NULL x or scale");
    std::vector<double> a;
    a.reserve((size_t)n);
    for (int i = 0; i < n; i++)
        if (std::isfinite(x[i])) a.push_back(std::fabs(x[i]));
    if (a.empty()) return fail(UCF_ERR_BAD_ARGUMENT, "none of the %d residuals is finite", n);
    std::sort(a.begin(), a.end());
    const size_t k = a.size();
    const double m = (k & 1) ? a[k / 2] : (a[k / 2 - 1] + a[k / 2]) / 2.0;
    *scale = 1.4826 * m;
    return UCF_OK;
}

int ucf_fit_set_loss(ucf_fit* f, int kind, double c)
{
    int rc = loss_check(kind, c);
    if (rc) return rc;
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL fit");
    f->loss = kind;
    f->loss_c = kind == UCF_LOSS_L2 ? 0.0 : c;
    return UCF_OK;
}

int ucf_fit_get_loss(const ucf_fit* f, int* kind, double* c)
{
    if (!f || !kind || !c) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *kind = f->loss;
    *c = f->loss_c;
    return UCF_OK;
}

// base plans only, the npar = 0 reduction in its robust instantiation (on a least-squares fit with every factor 1.0)
int ucf_fit_loss_report(ucf_fit* f, int nsets, const double* theta, double* phi, double* phi_w, int* nbad, int* ndown, double* b, double* bd)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (bd && !f->deriv) return fail(UCF_ERR_BAD_ARGUMENT, "bd is asked for, but the fit has no derivative data (ucf_fit_set_derivative)");
    fit_request q;
    q.phi = phi; q.nbad = nbad; q.phi_w = phi_w; q.ndown = ndown; q.b = b; q.bd = bd;
    return fit_evaluate(f, nsets, theta, q);
}

int ucf_fit_default_options(ucf_fit_options* opt)
{
    if (!opt) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    opt->max_iter = 50; opt->dlog = 1.0e-3; opt->lambda0 = 1.0e-2; opt->lambda_up = 10.0; opt->lambda_down = 0.1;
    opt->tol_step = 1.0e-6; opt->tol_phi = 1.0e-9;
    return UCF_OK;
}

}  // extern "C"

// ucf_fit_lm and ucf_fit_lm_resampled: one loop.  resampled == false: every evaluation is the plain fit_evaluate (rep, phi_out,
// counts are not read).  resampled == true: start s is reduced under replicate rep[s] (NULL: -1) with set_of the identity, in
// every evaluation of the loop and in the final one, whose phi_w and counts give cov.
static int fit_lm_core(ucf_fit* f, int nstarts, const double* theta0, bool resampled, const int* rep, const ucf_fit_options* opt_in, double* theta,
                       double* phi, int* iters, int* status, double* cov, double* phi_out, int* counts)
{
    if (!f || !theta0 || !theta || !phi || !iters || !status) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (nstarts < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nstarts=%d: at least one start", nstarts);
    if (resampled) {
        if (nstarts > (1 << 20)) return fail(UCF_ERR_BAD_ARGUMENT, "nstarts=%d: at most 2^20 resampled starts", nstarts);
        int rc0 = fit_resample_check(f, nstarts, nstarts, nullptr, rep);
        if (rc0) return rc0;
    }
    ucf_fit_options opt;
    (void)ucf_fit_default_options(&opt);
    if (opt_in) opt = *opt_in;
    if (opt.max_iter < 1 || !(opt.dlog > 0.0) || !(opt.lambda0 > 0.0) || !(opt.lambda_up > 1.0) || !(opt.lambda_down > 0.0) || !(opt.lambda_down < 1.0) ||
        !(opt.tol_step >= 0.0) || !(opt.tol_phi >= 0.0))
        return fail(UCF_ERR_BAD_ARGUMENT, "bad options: max_iter >= 1, dlog > 0, lambda0 > 0, lambda_up > 1, 0 < lambda_down < 1, tolerances >= 0");
    const int P = f->npar;
    const size_t PP = (size_t)P * P;
    std::vector<double> x((size_t)nstarts * P), lam(nstarts, opt.lambda0), g((size_t)nstarts * P), A(nstarts * PP), step((size_t)nstarts * P);
    std::vector<char> active(nstarts, 1), needJ(nstarts, 1), first(nstarts, 1);
    for (int s = 0; s < nstarts; s++) {
        iters[s] = 0; status[s] = UCF_FIT_MAX_ITER; phi[s] = NAN;
        for (int j = 0; j < P; j++) {
            const double v = theta0[(size_t)s * P + j];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(UCF_ERR_BAD_ARGUMENT, "start %d: parameter %d = %g must be positive and finite", s, j, v);
            theta[(size_t)s * P + j] = v;
            x[(size_t)s * P + j] = std::log(v);
        }
    }
    std::vector<int> idx;
    std::vector<double> th, ph, gg, AA;
    std::vector<int> nb, rp;
    int rc = UCF_OK;
    // th = the rows of `from` that idx names, in its order
    auto gather = [&](const double* from) {
        th.resize(idx.size() * P);
        for (size_t q = 0; q < idx.size(); q++) for (int j = 0; j < P; j++) th[q * P + j] = from[(size_t)idx[q] * P + j];
    };
    // phi and nbad of the starts in idx, in its order; resampled: each under its replicate (set_of is the identity over the sets
    // of one evaluation)
    auto request = [&](int jac) {
        ph.resize(idx.size()); nb.resize(idx.size());
        fit_request q;
        q.jac = jac; q.dlog = opt.dlog; q.phi = ph.data(); q.nbad = nb.data();
        if (resampled) {
            rp.resize(idx.size());
            for (size_t k = 0; k < idx.size(); k++) rp[k] = rep ? rep[idx[k]] : -1;
            q.resampled = true; q.nred = (int)idx.size(); q.rep = rp.data();
        }
        return q;
    };
    for (;;) {
        // 1. objective, gradient and normal equations where the point has moved (one call for all of them)
        idx.clear();
        for (int s = 0; s < nstarts; s++) if (active[s] && needJ[s]) idx.push_back(s);
        if (!idx.empty()) {
            const int n = (int)idx.size();
            gather(theta);
            gg.resize((size_t)n * P); AA.resize(n * PP);
            fit_request ask = request(1);
            ask.g = gg.data(); ask.A = AA.data();
            rc = fit_evaluate(f, n, th.data(), ask);
            if (rc) return rc;
            for (int q = 0; q < n; q++) {
                const int s = idx[q];
                needJ[s] = 0;
                if (first[s]) {
                    first[s] = 0;
                    if (nb[q] > 0 || !std::isfinite(ph[q])) { status[s] = UCF_FIT_NONFINITE_START; active[s] = 0; phi[s] = ph[q]; continue; }
                } else if (nb[q] > 0) {
                    // the perturbed plans of an accepted point left the finite range: the point stays, its step is damped as after a rejection
                    lam[s] *= opt.lambda_up;
                }
                phi[s] = ph[q];
                std::memcpy(&g[(size_t)s * P], &gg[(size_t)q * P], sizeof(double) * P);
                std::memcpy(&A[s * PP], &AA[q * PP], sizeof(double) * PP);
            }
        }
        // 2. damped steps and trial points
        idx.clear();
        for (int s = 0; s < nstarts; s++) {
            if (!active[s]) continue;
            if (ucf_fit_solve_step(P, &A[s * PP], &g[(size_t)s * P], lam[s], &step[(size_t)s * P]) != UCF_OK) { status[s] = UCF_FIT_SINGULAR; active[s] = 0; continue; }
            idx.push_back(s);
        }
        if (idx.empty()) break;
        const int n = (int)idx.size();
        th.resize((size_t)n * P);
        for (int q = 0; q < n; q++)
            for (int j = 0; j < P; j++) th[(size_t)q * P + j] = std::exp(x[(size_t)idx[q] * P + j] + step[(size_t)idx[q] * P + j]);
        const fit_request trial = request(0);
        bool finite_trial = true;
        for (double v : th) finite_trial = finite_trial && std::isfinite(v) && v > 0.0;
        if (finite_trial) {
            rc = fit_evaluate(f, n, th.data(), trial);
            if (rc != UCF_OK && rc != UCF_ERR_BAD_ARGUMENT && rc != UCF_ERR_HIP && rc != UCF_ERR_NOMEM && rc != UCF_ERR_NO_DEVICE) finite_trial = false;   // a trial outside the model's range: rejected below
            else if (rc) return rc;
        }
        // 3. accept or reject, per start
        for (int q = 0; q < n; q++) {
            const int s = idx[q];
            iters[s]++;
            double smax = 0.0;
            for (int j = 0; j < P; j++) smax = std::fmax(smax, std::fabs(step[(size_t)s * P + j]));
            const bool ok = finite_trial && nb[q] == 0 && std::isfinite(ph[q]) && ph[q] <= phi[s];
            bool done = smax <= opt.tol_step;
            if (ok) {
                if (phi[s] - ph[q] <= opt.tol_phi * phi[s]) done = true;
                for (int j = 0; j < P; j++) { x[(size_t)s * P + j] += step[(size_t)s * P + j]; theta[(size_t)s * P + j] = th[(size_t)q * P + j]; }
                phi[s] = ph[q];
                lam[s] *= opt.lambda_down;
                needJ[s] = 1;
            } else {
                lam[s] *= opt.lambda_up;
                if (!std::isfinite(lam[s])) done = true;
            }
            if (done) { status[s] = UCF_FIT_CONVERGED; active[s] = 0; }
            else if (iters[s] >= opt.max_iter) { status[s] = UCF_FIT_MAX_ITER; active[s] = 0; }
        }
    }
    if (resampled) {
        if (phi_out) for (int s = 0; s < nstarts; s++) phi_out[s] = NAN;
        if (counts) for (int i = 0; i < 4 * nstarts; i++) counts[i] = 0;
    }
    if (cov || (resampled && (phi_out || counts))) {
        // cov = phi / (nobs + nd - npar) A^-1 at the final point (NaN where A is singular, the start was not finite or no degree
        // of freedom is left); nd = derivative data with a positive weight, 0 on a fit without.  Resampled: phi_w / (nuse + nuse_d -
        // npar) A^-1 with the sums and counts of the start's replicate, from this evaluation, which also gives phi_out and counts
        if (cov) for (size_t i = 0; i < nstarts * PP; i++) cov[i] = NAN;
        idx.clear();
        for (int s = 0; s < nstarts; s++) if (status[s] != UCF_FIT_NONFINITE_START) idx.push_back(s);
        const int dof_all = f->nobs + (f->deriv ? f->nd : 0) - P;
        if (!idx.empty() && (resampled || dof_all > 0)) {
            const int n = (int)idx.size();
            gather(theta);
            AA.resize(n * PP);
            // under a robust loss the variance factor is phi_w of this evaluation: the weighted least-squares problem that the
            // final factors define (include/ucf.h); under least squares it stays the phi the iteration ended with
            const bool robust = resampled || f->loss != UCF_LOSS_L2;
            std::vector<double> pw(robust ? n : 0), po(resampled ? n : 0);
            std::vector<int> cnt(resampled ? 4 * (size_t)n : 0);
            fit_request ask = request(1);
            ask.A = AA.data();
            if (robust) ask.phi_w = pw.data();
            if (resampled) { ask.phi_out = po.data(); ask.counts = cnt.data(); }
            rc = fit_evaluate(f, n, th.data(), ask);
            if (rc) return rc;
            for (int q = 0; q < n; q++) {
                const int s = idx[q];
                if (resampled) {
                    if (phi_out) phi_out[s] = po[q];
                    if (counts) std::memcpy(&counts[4 * (size_t)s], &cnt[4 * (size_t)q], sizeof(int) * 4);
                }
                if (!cov) continue;
                const int dof = resampled ? cnt[4 * (size_t)q] + cnt[4 * (size_t)q + 1] - P : dof_all;
                if (dof <= 0) continue;
                double e[UCF_FIT_MAX_PAR], col[UCF_FIT_MAX_PAR];
                bool good = nb[q] == 0;
                for (int j = 0; j < P && good; j++) {
                    for (int k = 0; k < P; k++) e[k] = (k == j) ? 1.0 : 0.0;
                    good = ucf_fit_solve_step(P, &AA[q * PP], e, 0.0, col) == UCF_OK;
                    for (int k = 0; k < P && good; k++) cov[s * PP + (size_t)k * P + j] = (robust ? pw[q] : phi[s]) / (double)dof * col[k];
                }
                if (!good) for (size_t i = 0; i < PP; i++) cov[s * PP + i] = NAN;
            }
        }
    }
    return UCF_OK;
}

// ---- the host side of resampling (include/ucf.h states the arithmetic; this file is compiled without contraction)
namespace {
// nobs and the block ids of ucf_fit_resample_blocks / _jackknife; *nb = the number of blocks
int resample_check_blocks(int nobs, const int* block, int* nb)
{
    if (nobs < 1 || nobs > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d outside 1..2^24", nobs);
    if (!block) { *nb = nobs; return UCF_OK; }
    int top = -1;
    for (int i = 0; i < nobs; i++) {
        if (block[i] < 0 || block[i] >= nobs) return fail(UCF_ERR_BAD_ARGUMENT, "block[%d]=%d outside 0..%d", i, block[i], nobs - 1);
        top = std::max(top, block[i]);
    }
    std::vector<char> seen((size_t)top + 1, 0);
    for (int i = 0; i < nobs; i++) seen[block[i]] = 1;
    for (int b = 0; b <= top; b++)
        if (!seen[b]) return fail(UCF_ERR_BAD_ARGUMENT, "block id %d is used by no observation (the ids are 0..%d)", b, top);
    *nb = top + 1;
    return UCF_OK;
}
}  // namespace

// a row of multiplicities must sum within an int: nuse and nuse_d of the reduction are int
int ucf_host::fit_resample_check_rows(int nrep, int nobs, const unsigned short* mult)
{
    for (int r = 0; r < nrep; r++) {
        long long sum = 0;
        for (int i = 0; i < nobs; i++) sum += mult[(size_t)r * nobs + i];
        if (sum > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "replicate %d: its multiplicities sum to %lld, beyond 2^31 - 1", r, sum);
    }
    return UCF_OK;
}

extern "C" {

int ucf_fit_lm(ucf_fit* f, int nstarts, const double* theta0, const ucf_fit_options* opt_in, double* theta, double* phi, int* iters,
               int* status, double* cov)
{
    return fit_lm_core(f, nstarts, theta0, false, nullptr, opt_in, theta, phi, iters, status, cov, nullptr, nullptr);
}

int ucf_fit_lm_resampled(ucf_fit* f, int nstarts, const double* theta0, const int* rep, const ucf_fit_options* opt_in, double* theta, double* phi,
                         int* iters, int* status, double* cov, double* phi_out, int* counts)
{
    return fit_lm_core(f, nstarts, theta0, true, rep, opt_in, theta, phi, iters, status, cov, phi_out, counts);
}

int ucf_fit_set_resample(ucf_fit* f, int nrep, const unsigned short* mult)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL fit");
    if (!mult) { f->nrep = 0; return UCF_OK; }
    if (nrep < 1 || nrep > 65536) return fail(UCF_ERR_BAD_ARGUMENT, "nrep=%d outside 1..65536", nrep);
    int rc = fit_resample_check_rows(nrep, f->nobs, mult);
    if (rc) return rc;
    device_switch dg(f->device);
    const size_t bytes = sizeof(unsigned short) * (size_t)nrep * (size_t)f->nobs;
    if ((rc = grow_buffer(f->b_mult, bytes, "multiplicities", f->n_alloc))) return rc;
    f->nrep = 0;                           // until everything is in place
    HIP_TRY(hipMemcpy(f->b_mult.p, mult, bytes, hipMemcpyHostToDevice));
    f->nrep = nrep;
    return UCF_OK;
}

int ucf_fit_evaluate_resampled(ucf_fit* f, int nsets, const double* theta, double dlog, int nred, const int* set_of, const int* rep, double* phi,
                               double* g, double* A, int* nbad, double* phi_d, double* phi_w, double* phi_out, int* counts)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (phi_d && !f->deriv) return fail(UCF_ERR_BAD_ARGUMENT, "phi_d is asked for, but the fit has no derivative data (ucf_fit_set_derivative)");
    fit_request q;
    q.jac = 1; q.dlog = dlog; q.phi = phi; q.g = g; q.A = A; q.nbad = nbad; q.phi_d = phi_d; q.phi_w = phi_w;
    q.resampled = true; q.nred = nred; q.set_of = set_of; q.rep = rep; q.phi_out = phi_out; q.counts = counts;
    return fit_evaluate(f, nsets, theta, q);
}

int ucf_fit_objective_resampled(ucf_fit* f, int nsets, const double* theta, int nred, const int* set_of, const int* rep, double* phi, int* nbad,
                                double* phi_d, double* phi_w, double* phi_out, int* counts)
{
    if (!f) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (phi_d && !f->deriv) return fail(UCF_ERR_BAD_ARGUMENT, "phi_d is asked for, but the fit has no derivative data (ucf_fit_set_derivative)");
    fit_request q;
    q.phi = phi; q.nbad = nbad; q.phi_d = phi_d; q.phi_w = phi_w;
    q.resampled = true; q.nred = nred; q.set_of = set_of; q.rep = rep; q.phi_out = phi_out; q.counts = counts;
    return fit_evaluate(f, nsets, theta, q);
}

int ucf_fit_resample_blocks(int nobs, const int* block, int nrep, unsigned long long seed, unsigned short* mult, int* nblock)
{
    int nb = 0;
    int rc = resample_check_blocks(nobs, block, &nb);
    if (rc) return rc;
    if (nblock) *nblock = nb;
    if (!mult) return UCF_OK;
    if (nrep < 1 || nrep > 65536) return fail(UCF_ERR_BAD_ARGUMENT, "nrep=%d outside 1..65536", nrep);
    std::vector<int> drawn((size_t)nb);
    unsigned long long state = seed;
    for (int r = 0; r < nrep; r++) {
        std::fill(drawn.begin(), drawn.end(), 0);
        for (int d = 0; d < nb; d++) {
            state += 0x9E3779B97F4A7C15ULL;
            unsigned long long x = state;
            x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
            x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
            x = x ^ (x >> 31);
            drawn[(size_t)(((unsigned __int128)x * (unsigned __int128)(unsigned long long)nb) >> 64)]++;
        }
        for (int b = 0; b < nb; b++)
            if (drawn[b] > 65535) return fail(UCF_ERR_BAD_ARGUMENT, "replicate %d: block %d was drawn %d times, beyond 65535", r, b, drawn[b]);
        for (int i = 0; i < nobs; i++) mult[(size_t)r * nobs + i] = (unsigned short)drawn[block ? block[i] : i];
    }
    return UCF_OK;
}

int ucf_fit_resample_jackknife(int nobs, const int* block, unsigned short* mult)
{
    int nb = 0;
    int rc = resample_check_blocks(nobs, block, &nb);
    if (rc) return rc;
    if (!mult) return fail(UCF_ERR_BAD_ARGUMENT, "NULL mult");
    for (int b = 0; b < nb; b++)
        for (int i = 0; i < nobs; i++) mult[(size_t)b * nobs + i] = (block ? block[i] : i) == b ? 0 : 1;
    return UCF_OK;
}

int ucf_fit_resample_cov(int kind, int nrep, int npar, const double* theta, const int* use, double* mean, double* cov, int* nused)
{
    if (nused) *nused = 0;
    if (kind != UCF_RESAMPLE_BOOTSTRAP && kind != UCF_RESAMPLE_JACKKNIFE)
        return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d is no kind of resampling (UCF_RESAMPLE_BOOTSTRAP 0, UCF_RESAMPLE_JACKKNIFE 1)", kind);
    if (nrep < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nrep=%d: at least one replicate", nrep);
    if (npar < 1 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 1..%d", npar, UCF_FIT_MAX_PAR);
    if (!theta) return fail(UCF_ERR_BAD_ARGUMENT, "NULL theta");
    int n = 0;
    for (int r = 0; r < nrep; r++) {
        if (use && !use[r]) continue;
        n++;
        for (int j = 0; j < npar; j++) {
            const double v = theta[(size_t)r * npar + j];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(UCF_ERR_BAD_ARGUMENT, "replicate %d: parameter %d = %g must be positive and finite", r, j, v);
        }
    }
    if (n < 2) return fail(UCF_ERR_BAD_ARGUMENT, "%d replicates in use: at least two", n);
    if (nused) *nused = n;
    std::vector<double> x((size_t)nrep * npar);
    double m[UCF_FIT_MAX_PAR];
    for (int j = 0; j < npar; j++) {
        double s = 0.0;
        for (int r = 0; r < nrep; r++) {
            if (use && !use[r]) continue;
            x[(size_t)r * npar + j] = std::log(theta[(size_t)r * npar + j]);
            s = s + x[(size_t)r * npar + j];
        }
        m[j] = s / (double)n;
        if (mean) mean[j] = m[j];
    }
    if (!cov) return UCF_OK;
    for (int j = 0; j < npar; j++)
        for (int k = j; k < npar; k++) {
            double c = 0.0;
            for (int r = 0; r < nrep; r++) {
                if (use && !use[r]) continue;
                c = c + (x[(size_t)r * npar + j] - m[j]) * (x[(size_t)r * npar + k] - m[k]);
            }
            const double v = kind == UCF_RESAMPLE_BOOTSTRAP ? c / (double)(n - 1) : c * ((double)(n - 1) / (double)n);
            cov[(size_t)j * npar + k] = cov[(size_t)k * npar + j] = v;
        }
    return UCF_OK;
}

}  // extern "C"
