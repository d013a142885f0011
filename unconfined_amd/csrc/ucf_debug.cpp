// ucf_debug.cpp -- the stage hooks and the single-routine entries that tests and tools compare against the reference.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "ucf_host.h"
#include "ucf_field.h"
#include "ucf_fit.h"

using namespace ucf_host;

extern "C" {

// ---- stage hooks
// The intermediate stages of the PRODUCTION launch sequence (driver.f90:129-216: level sums, interval areas, accelerated
// transform): the call runs exactly what ucf_drawdown_grid / ucf_drawdown_batch would run for these sizes -- same lane
// layout, same kernel instantiations, same launch bounds -- and then reads the workspace that those kernels left.
int ucf_debug_stages(ucf_plan* pl, int grid, int nt, const double* tD, const int* sv, int nr, const double* rD,
                     int nz, const double* zD, const int* zLay, double* state, int* ndone, double* totlap,
                     double* h, double* dh, int* info)
{
    if (!pl || !tD || !sv || !rD || !zD || !zLay || !state || !ndone || !totlap || !h || !dh || !info) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    if (nt < 1 || nr < 1 || nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad sizes");
    if (!grid && nr != nt) return fail(UCF_ERR_BAD_ARGUMENT, "a point list has one radius per point (nr == nt)");
    if (nz > z_chunk(pl)) return fail(UCF_ERR_BAD_ARGUMENT, "nz=%d: the hook looks at one launch sequence (at most %d depths for this plan)", nz, z_chunk(pl));
    const long long npl = grid ? (long long)nt * nr : nt;
    if (npl > (1 << 22)) return fail(UCF_ERR_BAD_ARGUMENT, "too many points for the stage hook");
    const int npts = (int)npl, np = pl->D.np;
    int rc = grid ? check_grid_sv(pl, nt, sv) : check_sv(pl, nt, sv);
    if (rc) return rc;
    rc = check_depths(nz, zLay);
    if (rc) return rc;
    device_switch dg(pl->device);
    ucf_dev_params dp;
    rc = fill_call_params(pl, nz, zD, zLay, dp);
    if (rc) return rc;
    const int slots = (int)((size_t)(dp.R + 1 + dp.nacc) * nz);
    const size_t nb = sizeof(double) * (size_t)npts;
    dev_buf b_t, b_r, b_s, b_h, b_d, b_tl0, b_os, b_on;
    if (b_t.alloc(sizeof(double) * nt) || b_r.alloc(sizeof(double) * nr) || b_s.alloc(sizeof(int) * nt) || b_h.alloc(nb * nz) || b_d.alloc(nb * nz) ||
        b_tl0.alloc(nb * nz * np * 2) || b_os.alloc(nb * np * slots * 2) || b_on.alloc(sizeof(int) * (size_t)npts * np))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_t.p, tD, sizeof(double) * nt, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_r.p, rD, sizeof(double) * nr, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_s.p, sv, sizeof(int) * nt, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_tl0.p, 0, nb * nz * np * 2));
    HIP_TRY(hipMemset(b_os.p, 0, nb * np * slots * 2));
    HIP_TRY(hipMemset(b_on.p, 0xff, sizeof(int) * (size_t)npts * np));
    ucf_workspace* ws = ws_for(pl, nullptr);
    if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
    std::lock_guard<std::mutex> g(ws->mu);
    ucf_debug_rec rec;
    rec.d_totlap0 = (double*)b_tl0.p;
    ws->dbg = &rec;
    // UCF_DEBUG_REPS=n (diagnostic, tools/timeline.py): the launch sequence n times back to back, the last one is looked at
    const int reps = ucf_env_get().debug_reps;
    for (int rep = 0; rep < reps && rc == UCF_OK; rep++) {
        rec.count = 0;
        rc = grid ? grid_device_locked(pl, ws, nt, (const double*)b_t.p, (const int*)b_s.p, nr, (const double*)b_r.p, nz, zD, zLay, (double*)b_h.p, (double*)b_d.p, nullptr, nullptr)
                  : batch_device_impl(pl, ws, npts, (const double*)b_t.p, (const double*)b_r.p, (const int*)b_s.p, nz, zD, zLay, (double*)b_h.p, (double*)b_d.p, nullptr, nullptr, true);
    }
    ws->dbg = nullptr;
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (rec.count != 1) return fail(UCF_ERR_UNSUPPORTED, "the call was cut into %d launch sequences: the stage hook looks at one (smaller sizes)", rec.count);
    if (rec.layout == 1 && (rec.ir0 != 0 || rec.nrc != nr)) return fail(UCF_ERR_UNSUPPORTED, "the radii were cut into chunks");
    if (rec.layout == 2) return fail(UCF_ERR_UNSUPPORTED, "2M+1 > 64: no stage hook for the chunked layout");
    info[0] = rec.layout; info[1] = 0; info[2] = np; info[3] = npts;
    std::memset(state, 0, nb * np * slots * 2);
    for (size_t i = 0; i < (size_t)npts * np; i++) ndone[i] = -1;
    if (state_item_bytes(pl, dp) != 0 && ws->state.p) {
        info[1] = slots;
        rc = ucf_faithful::launch_debug_gather(dp, rec.layout, rec.nwork, rec.per_point, rec.nr, rec.nt, rec.ir0, (const double*)ws->state.p,
                                               (const int*)ws->ndone.p + buffers_of(pl, dp, rec.nwork, 0).ndone, (double*)b_os.p, (int*)b_on.p, nullptr);
        if (rc) return fail(rc, "gather kernel launch failed");
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(state, b_os.p, nb * np * slots * 2, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ndone, b_on.p, sizeof(int) * (size_t)npts * np, hipMemcpyDeviceToHost));
    }
    // the accelerated transform totlap(z, m) of every point, from where the layout keeps it
    if (rec.layout == 0) {
        HIP_TRY(hipMemcpy(totlap, b_tl0.p, nb * nz * np * 2, hipMemcpyDeviceToHost));
    } else {
        std::vector<double> raw((size_t)npts * nz * np * 2);
        HIP_TRY(hipMemcpy(raw.data(), ws->totlap.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int q = 0; q < npts; q++)
            for (int z = 0; z < nz; z++)
                for (int m = 0; m < np; m++) {
                    size_t src;
                    if (rec.layout == 1) { const int it = q / nr, ir = q % nr; src = (((size_t)ir * nz + z) * np + m) * nt + it; }
                    else src = ((size_t)z * np + m) * npts + q;
                    const size_t dst = ((size_t)q * nz + z) * np + m;
                    totlap[2 * dst] = raw[2 * src];
                    totlap[2 * dst + 1] = raw[2 * src + 1];
                }
    }
    HIP_TRY(hipMemcpy(h, b_h.p, nb * nz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dh, b_d.p, nb * nz, hipMemcpyDeviceToHost));
    return UCF_OK;
}

// wynn_epsilon as finish_kernel runs it (epsilon table in registers, wynn_regs<12>), in the flavour `mode`
int ucf_debug_wynn(int mode, int n, int nterms, const double* series, double* acc, int* status)
{
    if (n < 1 || nterms < 1 || nterms > 12 || !series || !acc || !status || mode < 0 || mode > 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad Wynn request (at most 12 terms)");
    int rc = require_device();
    if (rc) return rc;
    dev_buf b_s, b_a, b_st;
    if (b_s.alloc(sizeof(double) * 2 * (size_t)n * nterms) || b_a.alloc(sizeof(double) * 2 * n) || b_st.alloc(sizeof(int) * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_s.p, series, sizeof(double) * 2 * (size_t)n * nterms, hipMemcpyHostToDevice));
    rc = flavour(mode).launch_wynn_regs(n, nterms, (const double*)b_s.p, (double*)b_a.p, (int*)b_st.p, nullptr);
    if (rc) return fail(rc, "Wynn kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(acc, b_a.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status, b_st.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

// deHoog_invlap as every grid call runs it: dehoog_tiles_kernel (quotient-difference rhombus per vector, continued
// fraction per lane) on n transforms fp[n][2M+1] at times t[n] (T = 2 t); h[n] = f(t), dh[n] = t d/dt
int ucf_debug_dehoog_tiles(int mode, int n, int M, double alpha, double tol, const double* t, const double* fp, double* h, double* dh)
{
    if (n < 1 || !t || !fp || !h || !dh || mode < 0 || mode > 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad de Hoog request");
    if (M < 1 || M > UCF_MAX_LAP_M) return fail(UCF_ERR_UNSUPPORTED, "M=%d outside 1..%d", M, UCF_MAX_LAP_M);
    int rc = require_device();
    if (rc) return rc;
    const int np = 2 * M + 1;
    ucf_dev_params dp = {};
    dp.M = M; dp.np = np; dp.alpha = alpha; dp.logtol = std::log(tol); dp.nz = 1; dp.nz_out = 1; dp.z_off = 0;
    std::vector<double> tr((size_t)np * n * 2);           // [m][n]
    for (int i = 0; i < n; i++)
        for (int m = 0; m < np; m++) { tr[2 * ((size_t)m * n + i)] = fp[2 * ((size_t)i * np + m)]; tr[2 * ((size_t)m * n + i) + 1] = fp[2 * ((size_t)i * np + m) + 1]; }
    dev_buf b_t, b_f, b_h, b_d;
    if (b_t.alloc(sizeof(double) * n) || b_f.alloc(sizeof(double) * tr.size()) || b_h.alloc(sizeof(double) * n) || b_d.alloc(sizeof(double) * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_t.p, t, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_f.p, tr.data(), sizeof(double) * tr.size(), hipMemcpyHostToDevice));
    rc = flavour(mode).launch_dehoog_tiles_hook(dp, n, (const double*)b_t.p, (const double*)b_f.p, (double*)b_h.p, (double*)b_d.p, nullptr);
    if (rc) return fail(rc, "de Hoog kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(h, b_h.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dh, b_d.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_eval_samples(ucf_plan* pl, int n_a, const double* a, double rD, int np, const double* p_re_im,
                     int nz, const double* zD, const int* zLay, double* fp_re_im)
{
    if (!pl || !a || !p_re_im || !fp_re_im || n_a < 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad sample request");
    if (np != pl->D.np) return fail(UCF_ERR_BAD_ARGUMENT, "np=%d but the plan has 2M+1=%d", np, pl->D.np);
    ucf_dev_params dp;
    int rc = fill_call_params(pl, nz, zD, zLay, dp);
    if (rc) return rc;
    dev_buf b_a, b_p, b_f;
    const size_t nf = sizeof(double) * 2 * (size_t)n_a * nz * np;
    if (b_a.alloc(sizeof(double) * n_a) || b_p.alloc(sizeof(double) * 2 * np) || b_f.alloc(nf))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_a.p, a, sizeof(double) * n_a, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_p.p, p_re_im, sizeof(double) * 2 * np, hipMemcpyHostToDevice));
    rc = flavour_of(pl).launch_samples(dp, n_a, (const double*)b_a.p, rD, (const double*)b_p.p, (double*)b_f.p, nullptr);
    if (rc) return fail(rc, "sample kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(fp_re_im, b_f.p, nf, hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_pvalues(const ucf_plan* pl, double tee, double* p_re_im)
{
    if (!pl || !p_re_im) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    const double PI = 4.0 * std::atan(1.0);
    const double sigma = pl->P.alpha - std::log(pl->P.tol) / (2.0 * tee);      // invlap.f90:165
    for (int i = 0; i <= 2 * pl->P.M; i++) {
        p_re_im[2 * i] = sigma;
        p_re_im[2 * i + 1] = PI * i / tee;                                     // :168
    }
    return UCF_OK;
}

int ucf_dehoog(int n, int M, double alpha, double tol, const double* t, const double* tee, const double* fp, double* ft)
{
    if (n < 1 || !t || !tee || !fp || !ft) return fail(UCF_ERR_BAD_ARGUMENT, "bad de Hoog request");
    if (M < 1 || M > UCF_MAX_LAP_M) return fail(UCF_ERR_UNSUPPORTED, "M=%d outside 1..%d", M, UCF_MAX_LAP_M);
    int rc = require_device();
    if (rc) return rc;
    dev_buf b_t, b_e, b_f, b_o;
    const int np = 2 * M + 1;
    if (b_t.alloc(sizeof(double) * n) || b_e.alloc(sizeof(double) * n) || b_f.alloc(sizeof(double) * 2 * (size_t)n * np) ||
        b_o.alloc(sizeof(double) * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_t.p, t, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_e.p, tee, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_f.p, fp, sizeof(double) * 2 * (size_t)n * np, hipMemcpyHostToDevice));
    rc = ucf_faithful::launch_dehoog(n, M, alpha, std::log(tol), (const double*)b_t.p, (const double*)b_e.p,
                                     (const double*)b_f.p, (double*)b_o.p, nullptr);
    if (rc) return fail(rc, "de Hoog kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(ft, b_o.p, sizeof(double) * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_bessel_k01(int n, const double* z, double* k, int* ierr)
{
    if (n < 1 || !z || !k || !ierr) return fail(UCF_ERR_BAD_ARGUMENT, "bad Bessel request");
    int rc = require_device();
    if (rc) return rc;
    dev_buf b_z, b_k, b_e;
    if (b_z.alloc(sizeof(double) * 2 * n) || b_k.alloc(sizeof(double) * 4 * n) || b_e.alloc(sizeof(int) * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_z.p, z, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    rc = ucf_faithful::launch_bessel(n, (const double*)b_z.p, (double*)b_k.p, (int*)b_e.p, nullptr);
    if (rc) return fail(rc, "Bessel kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(k, b_k.p, sizeof(double) * 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ierr, b_e.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_wynn_epsilon(int n, int nterms, const double* series, double* acc, int* status)
{
    if (n < 1 || nterms < 1 || nterms > 64 || !series || !acc || !status) return fail(UCF_ERR_BAD_ARGUMENT, "bad Wynn request");
    int rc = require_device();
    if (rc) return rc;
    dev_buf b_s, b_a, b_st;
    if (b_s.alloc(sizeof(double) * 2 * (size_t)n * nterms) || b_a.alloc(sizeof(double) * 2 * n) || b_st.alloc(sizeof(int) * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_s.p, series, sizeof(double) * 2 * (size_t)n * nterms, hipMemcpyHostToDevice));
    rc = ucf_faithful::launch_wynn(n, nterms, (const double*)b_s.p, (double*)b_a.p, (int*)b_st.p, nullptr);
    if (rc) return fail(rc, "Wynn kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(acc, b_a.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status, b_st.p, sizeof(int) * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_extraptozero(int n, int R, const double* x, const double* y, double* out)
{
    if (n < 1 || R < 1 || R > UCF_MAX_R || !x || !y || !out) return fail(UCF_ERR_BAD_ARGUMENT, "bad extrapolation request");
    int rc = require_device();
    if (rc) return rc;
    dev_buf b_x, b_y, b_o;
    if (b_x.alloc(sizeof(double) * R) || b_y.alloc(sizeof(double) * 2 * (size_t)n * R) || b_o.alloc(sizeof(double) * 2 * n))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    HIP_TRY(hipMemcpy(b_x.p, x, sizeof(double) * R, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_y.p, y, sizeof(double) * 2 * (size_t)n * R, hipMemcpyHostToDevice));
    rc = ucf_faithful::launch_extrap(n, R, (const double*)b_x.p, (const double*)b_y.p, (double*)b_o.p, nullptr);
    if (rc) return fail(rc, "extrapolation kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out, b_o.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    return UCF_OK;
}

}  // extern "C"

namespace {
// The refs of ucf_debug_fit_reduce, packed as the kernel reads them.  Every double a ref can reach under any of the nplans
// plans -- prefix * nplans + plan * stride + at + (0 .. count - 1), the largest at plan = nplans - 1 -- must lie in [0, nh).
// 128-bit arithmetic: the caller's numbers are arbitrary.
int pack_refs(const char* what, int n, const long long* prefix, const long long* stride, const int* at, const int* count, long long nplans,
              long long nh, std::vector<ucf_fit_obs_ref>& out)
{
    out.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        if (prefix[i] < 0 || stride[i] < 0 || at[i] < 0 || count[i] < 1 || count[i] > UCF_MAX_NZ)
            return fail(UCF_ERR_BAD_ARGUMENT, "%s %d: prefix=%lld stride=%lld at=%d count=%d (none negative, count in 1..%d)", what, i, prefix[i],
                        stride[i], at[i], count[i], UCF_MAX_NZ);
        const __int128 last = (__int128)prefix[i] * nplans + (__int128)(nplans - 1) * stride[i] + at[i] + count[i] - 1;
        if (last >= (__int128)nh)
            return fail(UCF_ERR_BAD_ARGUMENT, "%s %d: its last depth under plan %lld lies beyond h (prefix=%lld stride=%lld at=%d count=%d, nh=%lld)",
                        what, i, nplans - 1, prefix[i], stride[i], at[i], count[i], nh);
        out[(size_t)i] = ucf_fit_obs_ref{prefix[i], stride[i], at[i], count[i]};
    }
    return UCF_OK;
}

// The reduction of ucf_field_ensemble -- weighted: of ucf_field_ensemble_weighted, on the caller's weights through the same
// quantisation -- on caller data a [nens][nout]: the same launcher (and through it the same choice of tile), so the kernels
// are testable at their edges without paying for evaluations.
int debug_ensemble_core(int nens, long long nout, const double* a, bool weighted, const double* weight, int nq, const double* q, int nlim,
                        const double* limit, const ucf_ensemble_maps* out, double* pexc, long long* nbad)
{
    const ucf_ensemble_maps none = {};
    const ucf_ensemble_maps* w = out ? out : &none;
    int rc = ensemble_check_levels(nens, nq, q, nlim, limit, w->quant != nullptr, pexc != nullptr);
    if (rc) return rc;
    if (!a) return fail(UCF_ERR_BAD_ARGUMENT, "NULL a");
    if (nout < 1 || nens * nout > 0x7fffffffLL * 256) return fail(UCF_ERR_BAD_ARGUMENT, "nout=%lld: at least one output, at most 2^39 values", nout);
    std::vector<unsigned long long> u(weighted ? (size_t)nens : 0);
    if (weighted && (rc = ucf_ensemble_quantise(nens, weight, u.data(), nullptr))) return rc;
    if ((rc = require_device())) return rc;
    const size_t no = (size_t)nout, so = sizeof(double) * no, su = sizeof(unsigned long long) * u.size();
    dev_buf b_a, b_u, b_ql, b_mean, b_sd, b_min, b_max, b_quant, b_nfin, b_pexc, b_nbad;
    if (b_a.alloc(so * nens) || (weighted && b_u.alloc(su)) || b_ql.alloc(sizeof(double) * 2 * UCF_ENSEMBLE_MAX_Q) ||
        b_nbad.alloc(sizeof(long long)) || (w->mean && b_mean.alloc(so)) || (w->sd && b_sd.alloc(so)) || (w->min && b_min.alloc(so)) ||
        (w->max && b_max.alloc(so)) || (w->quant && b_quant.alloc(so * nq)) || (w->nfin && b_nfin.alloc(sizeof(int) * no)) ||
        (pexc && b_pexc.alloc(so * nlim)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    double ql[2 * UCF_ENSEMBLE_MAX_Q];
    ensemble_pack_levels(nq, q, nlim, limit, ql);
    HIP_TRY(hipMemcpy(b_a.p, a, so * nens, hipMemcpyHostToDevice));
    if (weighted) HIP_TRY(hipMemcpy(b_u.p, u.data(), su, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_ql.p, ql, sizeof(ql), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_nbad.p, 0, sizeof(long long)));
    ucf_ensemble_reduce_args ra = {};
    ra.nens = nens; ra.nout = nout; ra.d_a = (const double*)b_a.p; ra.d_u = (const unsigned long long*)b_u.p;
    ra.nq = nq; ra.d_q = (const double*)b_ql.p; ra.nlim = nlim; ra.d_limit = (const double*)b_ql.p + UCF_ENSEMBLE_MAX_Q;
    ra.d_mean = (double*)b_mean.p; ra.d_sd = (double*)b_sd.p; ra.d_min = (double*)b_min.p; ra.d_max = (double*)b_max.p;
    ra.d_nfin = (int*)b_nfin.p; ra.d_quant = (double*)b_quant.p; ra.d_pexc = (double*)b_pexc.p; ra.d_nbad = (long long*)b_nbad.p;
    rc = ucf_field_launch_ensemble_reduce(&ra, nullptr);
    if (rc) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{w->mean, b_mean.p, so}, {w->sd, b_sd.p, so}, {w->min, b_min.p, so}, {w->max, b_max.p, so}, {w->quant, b_quant.p, so * nq},
                           {w->nfin, b_nfin.p, sizeof(int) * no}, {pexc, b_pexc.p, so * nlim}, {nbad, b_nbad.p, sizeof(long long)}});
}
}  // namespace

extern "C" {

int ucf_debug_ensemble(int nens, long long nout, const double* a, int nq, const double* q, int nlim, const double* limit,
                       const ucf_ensemble_maps* out, double* pexc, long long* nbad)
{
    return debug_ensemble_core(nens, nout, a, false, nullptr, nq, q, nlim, limit, out, pexc, nbad);
}

int ucf_debug_ensemble_weighted(int nens, long long nout, const double* a, const double* weight, int nq, const double* q, int nlim,
                                const double* limit, const ucf_ensemble_maps* out, double* pexc, long long* nbad)
{
    return debug_ensemble_core(nens, nout, a, true, weight, nq, q, nlim, limit, out, pexc, nbad);
}

}  // extern "C"

namespace {
// ucf_debug_fit_reduce (loss = UCF_LOSS_L2: c, ndown, b, bd are not read) and ucf_debug_fit_reduce_loss: one validation and one
// launch through ucf_fit_launch_reduce.  Everything the kernel could read is checked against the lengths the caller gave
// before anything is allocated or launched.  resampled: ucf_debug_fit_reduce_resampled -- nred reductions in place of one per
// set; sums, nbad and counts are per reduction, and none of J .. bd may be asked for.
// The members are the arguments of the three entries under their names of include/ucf.h, zero where an entry has none.
struct debug_fit_reduce {
    int loss;
    double c;
    int source, npar, nsets, nobs;
    double two_dlog;
    long long nh, plan_stride;
    const double *h, *dh, *Hc, *obs, *w, *dobs, *wd, *q, *tfac;
    const long long *prefix, *stride;
    const int *slot, *at, *count, *first, *set_of, *rep;
    const unsigned short* mult;
    int nref, nrep, nred;
    bool resampled;
    double *sums, *J, *sim, *Jd, *simd, *b, *bd;
    int *nbad, *ndown, *counts;
    int run() const;
};
// what the three entries have in common, from their parameters of the same names
#define UCF_DEBUG_FIT_REDUCE_IN(in)                                                                                              \
    in.source = source; in.npar = npar; in.nsets = nsets; in.nobs = nobs; in.two_dlog = two_dlog; in.nh = nh;                    \
    in.h = h; in.dh = dh; in.Hc = Hc; in.obs = obs; in.w = w; in.dobs = dobs; in.wd = wd; in.slot = slot;                        \
    in.plan_stride = plan_stride; in.nref = nref; in.prefix = prefix; in.stride = stride; in.at = at; in.count = count; in.q = q; \
    in.tfac = tfac; in.first = first; in.sums = sums; in.nbad = nbad

int debug_fit_reduce::run() const
{
    if (loss != UCF_LOSS_L2) {
        if (loss != UCF_LOSS_HUBER && loss != UCF_LOSS_TUKEY)
            return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d: UCF_LOSS_HUBER (1) or UCF_LOSS_TUKEY (2); least squares is ucf_debug_fit_reduce", loss);
        if (!(c > 0.0) || !std::isfinite(c)) return fail(UCF_ERR_BAD_ARGUMENT, "c=%g must be positive and finite", c);
        if (!dh && bd) return fail(UCF_ERR_BAD_ARGUMENT, "bd asked for without dh");
    }
    if (source != UCF_FIT_SLOTS && source != UCF_FIT_NETWORK && source != UCF_FIT_FIELD) return fail(UCF_ERR_BAD_ARGUMENT, "source=%d outside 0..2", source);
    if (npar < 0 || npar > UCF_FIT_MAX_PAR) return fail(UCF_ERR_BAD_ARGUMENT, "npar=%d outside 0..%d", npar, UCF_FIT_MAX_PAR);
    if (nsets < 1 || nsets > (1 << 16)) return fail(UCF_ERR_BAD_ARGUMENT, "nsets=%d outside 1..65536", nsets);
    if (nobs < 1 || nobs > (1 << 24)) return fail(UCF_ERR_BAD_ARGUMENT, "nobs=%d outside 1..2^24", nobs);
    if (nh < 1 || nh > (1LL << 28)) return fail(UCF_ERR_BAD_ARGUMENT, "nh=%lld outside 1..2^28", nh);
    if (!h || !Hc || !obs || !w || !sums || !nbad) return fail(UCF_ERR_BAD_ARGUMENT, "NULL h, Hc, obs, w, sums or nbad");
    if (dh && (!dobs || !wd)) return fail(UCF_ERR_BAD_ARGUMENT, "dh without dobs or wd");
    if (!dh && (Jd || simd)) return fail(UCF_ERR_BAD_ARGUMENT, "Jd or simd asked for without dh");
    const long long nplans = (long long)nsets * (1 + 2 * npar);
    std::vector<ucf_fit_obs_ref> refs;
    std::vector<ucf_fit_term> terms;
    int rc;
    if (resampled) {
        if (!counts) return fail(UCF_ERR_BAD_ARGUMENT, "NULL counts");
        if (nrep < 0 || nrep > 65536) return fail(UCF_ERR_BAD_ARGUMENT, "nrep=%d outside 0..65536", nrep);
        if (nrep > 0 && !mult) return fail(UCF_ERR_BAD_ARGUMENT, "NULL mult with nrep=%d", nrep);
        if (nrep > 0 && (rc = fit_resample_check_rows(nrep, nobs, mult))) return rc;
        if (nred < 1 || nred > (1 << 16)) return fail(UCF_ERR_BAD_ARGUMENT, "nred=%d outside 1..65536", nred);
        if (!set_of && nred > nsets)
            return fail(UCF_ERR_BAD_ARGUMENT, "set_of is NULL (reduction r reads set r), but nred=%d exceeds nsets=%d", nred, nsets);
        for (int r = 0; r < nred; r++) {
            if (set_of && (set_of[r] < 0 || set_of[r] >= nsets))
                return fail(UCF_ERR_BAD_ARGUMENT, "set_of[%d]=%d outside 0..%d", r, set_of[r], nsets - 1);
            if (rep && (rep[r] < -1 || rep[r] >= nrep))
                return fail(UCF_ERR_BAD_ARGUMENT, "rep[%d]=%d outside -1..%d", r, rep[r], nrep - 1);
        }
    }
    if (source == UCF_FIT_SLOTS) {
        if (!slot) return fail(UCF_ERR_BAD_ARGUMENT, "NULL slot");
        if (plan_stride < 1 || (__int128)plan_stride * nplans > (__int128)nh)
            return fail(UCF_ERR_BAD_ARGUMENT, "plan_stride=%lld: %lld plans of it do not fit in nh=%lld", plan_stride, nplans, nh);
        for (int i = 0; i < nobs; i++)
            if (slot[i] < 0 || slot[i] >= plan_stride) return fail(UCF_ERR_BAD_ARGUMENT, "slot[%d]=%d outside 0..plan_stride-1=%lld", i, slot[i], plan_stride - 1);
    } else {
        if (!prefix || !stride || !at || !count) return fail(UCF_ERR_BAD_ARGUMENT, "NULL prefix, stride, at or count");
        if (source == UCF_FIT_NETWORK) {
            if (nref != nobs) return fail(UCF_ERR_BAD_ARGUMENT, "nref=%d: a network has one ref per observation (nobs=%d)", nref, nobs);
            if ((rc = pack_refs("ref", nref, prefix, stride, at, count, nplans, nh, refs))) return rc;
        } else {
            if (nref < 0 || !first || !q || (dh && !tfac)) return fail(UCF_ERR_BAD_ARGUMENT, "nref=%d negative, or NULL first, q or (with dh) tfac", nref);
            if (first[0] < 0) return fail(UCF_ERR_BAD_ARGUMENT, "first[0]=%d negative", first[0]);
            for (int i = 0; i < nobs; i++)
                if (first[i + 1] < first[i]) return fail(UCF_ERR_BAD_ARGUMENT, "first[%d]=%d below first[%d]=%d: not ascending", i + 1, first[i + 1], i, first[i]);
            if (first[nobs] != nref) return fail(UCF_ERR_BAD_ARGUMENT, "first[nobs]=%d is not the number of terms %d", first[nobs], nref);
            if ((rc = pack_refs("term", nref, prefix, stride, at, count, nplans, nh, refs))) return rc;
            terms.resize((size_t)nref);
            for (int k = 0; k < nref; k++) terms[(size_t)k] = ucf_fit_term{refs[(size_t)k], q[k]};
        }
    }
    if ((rc = require_device())) return rc;
    const bool joint = dh != nullptr;
    const size_t so = sizeof(double) * (size_t)nobs, sh = sizeof(double) * (size_t)nh, nt = (size_t)(nref > 0 ? nref : 1);
    const size_t nout = (size_t)(resampled ? nred : nsets);      // workgroups: what sums and nbad are indexed by
    const size_t smult = resampled ? sizeof(unsigned short) * (size_t)nrep * (size_t)nobs : 0;
    const size_t bfac = so * (size_t)nsets;
    const size_t bJ = so * nsets * (npar > 0 ? npar : 1), bsim = so * (size_t)nplans;
    dev_buf b_h, b_dh, b_hc, b_obs, b_w, b_dobs, b_wd, b_slot, b_ref, b_term, b_first, b_tfac, b_sums, b_nbad, b_J, b_sim, b_Jd, b_simd, b_ndown, b_b, b_bd;
    dev_buf b_mult, b_setof, b_rep, b_counts;
    if (resampled && ((smult && b_mult.alloc(smult)) || (set_of && b_setof.alloc(sizeof(int) * nout)) || (rep && b_rep.alloc(sizeof(int) * nout)) ||
                b_counts.alloc(sizeof(int) * 4 * nout)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    if (b_h.alloc(sh) || (joint && b_dh.alloc(sh)) || b_hc.alloc(sizeof(double) * (size_t)nplans) || b_obs.alloc(so) || b_w.alloc(so) ||
        (joint && (b_dobs.alloc(so) || b_wd.alloc(so))) || (source == UCF_FIT_SLOTS && b_slot.alloc(sizeof(int) * (size_t)nobs)) ||
        (source == UCF_FIT_NETWORK && b_ref.alloc(sizeof(ucf_fit_obs_ref) * nt)) ||
        (source == UCF_FIT_FIELD && (b_term.alloc(sizeof(ucf_fit_term) * nt) || b_first.alloc(sizeof(int) * ((size_t)nobs + 1)) ||
                                     (joint && b_tfac.alloc(sizeof(double) * nt)))) ||
        b_nbad.alloc(sizeof(int) * nout) || (J && b_J.alloc(bJ)) || (sim && b_sim.alloc(bsim)) ||
        (Jd && b_Jd.alloc(bJ)) || (simd && b_simd.alloc(bsim)) || (ndown && b_ndown.alloc(sizeof(int) * (size_t)nsets)) || (b && b_b.alloc(bfac)) ||
        (bd && b_bd.alloc(bfac)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    ucf_fit_reduce_args ra = {};
    ra.npar = npar; ra.nsets = nsets; ra.nobs = nobs;
    ra.nplans = (size_t)nplans; ra.plan_stride = (size_t)plan_stride; ra.two_dlog = two_dlog;
    ra.d_h = (const double*)b_h.p; ra.d_dh = (const double*)b_dh.p; ra.d_Hc = (const double*)b_hc.p;
    ra.source = (ucf_fit_source)source;
    ra.d_slot = (const int*)b_slot.p; ra.d_ref = (const ucf_fit_obs_ref*)b_ref.p;
    ra.d_term = (const ucf_fit_term*)b_term.p; ra.d_first = (const int*)b_first.p; ra.d_tfac = (const double*)b_tfac.p;
    ra.d_obs = (const double*)b_obs.p; ra.d_w = (const double*)b_w.p; ra.d_dobs = (const double*)b_dobs.p; ra.d_wd = (const double*)b_wd.p;
    ra.d_nbad = (int*)b_nbad.p;
    ra.d_J = (double*)b_J.p; ra.d_sim = (double*)b_sim.p; ra.d_Jd = (double*)b_Jd.p; ra.d_simd = (double*)b_simd.p;
    ra.loss = loss; ra.loss_c = c; ra.d_ndown = (int*)b_ndown.p; ra.d_b = (double*)b_b.p; ra.d_bd = (double*)b_bd.p;
    ra.nred = resampled ? nred : 0; ra.d_mult = (const unsigned short*)b_mult.p; ra.d_set_of = (const int*)b_setof.p;
    ra.d_rep = (const int*)b_rep.p; ra.d_counts = (int*)b_counts.p;
    // the sums last: their number per workgroup follows from the launch that `ra` now describes
    const size_t nsum = (size_t)ucf_fit_sums_of(&ra).count;
    if (b_sums.alloc(sizeof(double) * nout * nsum)) return fail(UCF_ERR_NOMEM, "device allocation failed");
    ra.d_sums = (double*)b_sums.p;
    const struct { void* dev; const void* host; size_t bytes; } up[] = {
        {b_h.p, h, sh}, {b_dh.p, dh, sh}, {b_hc.p, Hc, sizeof(double) * (size_t)nplans}, {b_obs.p, obs, so}, {b_w.p, w, so}, {b_dobs.p, dobs, so},
        {b_wd.p, wd, so}, {b_slot.p, slot, sizeof(int) * (size_t)nobs}, {b_ref.p, refs.data(), sizeof(ucf_fit_obs_ref) * refs.size()},
        {b_term.p, terms.data(), sizeof(ucf_fit_term) * terms.size()}, {b_first.p, first, sizeof(int) * ((size_t)nobs + 1)},
        {b_tfac.p, tfac, sizeof(double) * terms.size()}, {b_mult.p, mult, smult},
        {b_setof.p, set_of, sizeof(int) * nout}, {b_rep.p, rep, sizeof(int) * nout}};
    for (const auto& c : up)
        if (c.dev && c.bytes) HIP_TRY(hipMemcpy(c.dev, c.host, c.bytes, hipMemcpyHostToDevice));
    rc = ucf_fit_launch_reduce(&ra, nullptr);
    if (rc) return fail(rc, "fit reduction kernel launch failed");
    HIP_TRY(hipStreamSynchronize(nullptr));
    return copy_back_sync({{counts, b_counts.p, sizeof(int) * 4 * nout}, {sums, b_sums.p, sizeof(double) * nout * nsum}, {nbad, b_nbad.p, sizeof(int) * nout},
                           {J, b_J.p, npar > 0 ? bJ : 0}, {sim, b_sim.p, bsim}, {Jd, b_Jd.p, npar > 0 ? bJ : 0}, {simd, b_simd.p, bsim},
                           {ndown, b_ndown.p, sizeof(int) * (size_t)nsets}, {b, b_b.p, bfac}, {bd, b_bd.p, bfac}});
}
}  // namespace

extern "C" {

// The fit reduction exactly as ucf_fit_evaluate launches it (ucf_fit_launch_reduce, and through it the same choice of
// instantiation), on caller data: the kernel is testable at its edges without paying for evaluations.
int ucf_debug_fit_reduce(int source, int npar, int nsets, int nobs, double two_dlog, long long nh, const double* h, const double* dh,
                         const double* Hc, const double* obs, const double* w, const double* dobs, const double* wd, const int* slot,
                         long long plan_stride, int nref, const long long* prefix, const long long* stride, const int* at,
                         const int* count, const double* q, const double* tfac, const int* first, double* sums, int* nbad, double* J,
                         double* sim, double* Jd, double* simd)
{
    debug_fit_reduce in = {};
    UCF_DEBUG_FIT_REDUCE_IN(in);
    in.J = J; in.sim = sim; in.Jd = Jd; in.simd = simd;
    return in.run();
}

// the same under a robust loss: kind and c are checked first, with the rest before any device is touched
int ucf_debug_fit_reduce_loss(int kind, double c, int source, int npar, int nsets, int nobs, double two_dlog, long long nh, const double* h,
                              const double* dh, const double* Hc, const double* obs, const double* w, const double* dobs, const double* wd,
                              const int* slot, long long plan_stride, int nref, const long long* prefix, const long long* stride,
                              const int* at, const int* count, const double* q, const double* tfac, const int* first, double* sums, int* nbad,
                              double* J, double* sim, double* Jd, double* simd, int* ndown, double* b, double* bd)
{
    if (kind != UCF_LOSS_HUBER && kind != UCF_LOSS_TUKEY)
        return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d: UCF_LOSS_HUBER (1) or UCF_LOSS_TUKEY (2); least squares is ucf_debug_fit_reduce", kind);
    debug_fit_reduce in = {};
    UCF_DEBUG_FIT_REDUCE_IN(in);
    in.loss = kind; in.c = c; in.J = J; in.sim = sim; in.Jd = Jd; in.simd = simd; in.ndown = ndown; in.b = b; in.bd = bd;
    return in.run();
}

// the same per reduction under multiplicities: kind, c and the resampling arguments are checked with the rest before any device
int ucf_debug_fit_reduce_resampled(int kind, double c, int source, int npar, int nsets, int nobs, double two_dlog, long long nh, const double* h,
                                   const double* dh, const double* Hc, const double* obs, const double* w, const double* dobs, const double* wd,
                                   const int* slot, long long plan_stride, int nref, const long long* prefix, const long long* stride,
                                   const int* at, const int* count, const double* q, const double* tfac, const int* first, int nrep,
                                   const unsigned short* mult, int nred, const int* set_of, const int* rep, double* sums, int* nbad, int* counts)
{
    if (kind != UCF_LOSS_L2 && kind != UCF_LOSS_HUBER && kind != UCF_LOSS_TUKEY)
        return fail(UCF_ERR_BAD_ARGUMENT, "kind=%d is no loss (UCF_LOSS_L2 0, UCF_LOSS_HUBER 1, UCF_LOSS_TUKEY 2)", kind);
    debug_fit_reduce in = {};
    UCF_DEBUG_FIT_REDUCE_IN(in);
    in.loss = kind; in.c = c;
    in.resampled = true; in.nrep = nrep; in.mult = mult; in.nred = nred; in.set_of = set_of; in.rep = rep; in.counts = counts;
    return in.run();
}

}  // extern "C"

#undef UCF_DEBUG_FIT_REDUCE_IN
