// ucf_debug.cpp -- the stage hooks and the single-routine entries that tests and tools compare against the reference.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "ucf_host.h"
#include "ucf_field.h"

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

// The two reduction kernels of ucf_field_ensemble on caller data a [nens][nout]: the same launchers (and through them the
// same choice of tile), so the kernels are testable at their edges without paying for evaluations.
int ucf_debug_ensemble(int nens, long long nout, const double* a, int nq, const double* q, int nlim, const double* limit,
                       const ucf_ensemble_maps* out, double* pexc, long long* nbad)
{
    const ucf_ensemble_maps none = {};
    const ucf_ensemble_maps* w = out ? out : &none;
    int rc = ensemble_check_levels(nens, nq, q, nlim, limit, w->quant != nullptr, pexc != nullptr);
    if (rc) return rc;
    if (!a) return fail(UCF_ERR_BAD_ARGUMENT, "NULL a");
    if (nout < 1 || nens * nout > 0x7fffffffLL * 256) return fail(UCF_ERR_BAD_ARGUMENT, "nout=%lld: at least one output, at most 2^39 values", nout);
    if ((rc = require_device())) return rc;
    const size_t no = (size_t)nout, so = sizeof(double) * no;
    dev_buf b_a, b_ql, b_mean, b_sd, b_min, b_max, b_quant, b_nfin, b_pexc, b_nbad;
    if (b_a.alloc(so * nens) || b_ql.alloc(sizeof(double) * 2 * UCF_ENSEMBLE_MAX_Q) || b_nbad.alloc(sizeof(long long)) ||
        (w->mean && b_mean.alloc(so)) || (w->sd && b_sd.alloc(so)) || (w->min && b_min.alloc(so)) || (w->max && b_max.alloc(so)) ||
        (w->quant && b_quant.alloc(so * nq)) || (w->nfin && b_nfin.alloc(sizeof(int) * no)) || (pexc && b_pexc.alloc(so * nlim)))
        return fail(UCF_ERR_NOMEM, "device allocation failed");
    double ql[2 * UCF_ENSEMBLE_MAX_Q] = {};
    for (int i = 0; i < nq; i++) ql[i] = q[i];
    for (int i = 0; i < nlim; i++) ql[UCF_ENSEMBLE_MAX_Q + i] = limit[i];
    HIP_TRY(hipMemcpy(b_a.p, a, so * nens, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_ql.p, ql, sizeof(ql), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_nbad.p, 0, sizeof(long long)));
    rc = ucf_field_launch_ensemble_moments(nens, nout, (const double*)b_a.p, nlim, (const double*)b_ql.p + UCF_ENSEMBLE_MAX_Q, (double*)b_mean.p,
                                           (double*)b_sd.p, (double*)b_min.p, (double*)b_max.p, (int*)b_nfin.p, (double*)b_pexc.p,
                                           (long long*)b_nbad.p, nullptr);
    if (rc == UCF_OK && w->quant)
        rc = ucf_field_launch_ensemble_quantile(nens, nout, (const double*)b_a.p, nq, (const double*)b_ql.p, (double*)b_quant.p, nullptr);
    if (rc) return fail(rc, "ensemble kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipStreamSynchronize(nullptr));
    const struct { void* host; const void* dev; size_t bytes; } back[] = {
        {w->mean, b_mean.p, so}, {w->sd, b_sd.p, so}, {w->min, b_min.p, so}, {w->max, b_max.p, so}, {w->quant, b_quant.p, so * nq},
        {w->nfin, b_nfin.p, sizeof(int) * no}, {pexc, b_pexc.p, so * nlim}, {nbad, b_nbad.p, sizeof(long long)}};
    for (const auto& c : back)
        if (c.host) HIP_TRY(hipMemcpy(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost));
    return UCF_OK;
}

}  // extern "C"
