// ucf_launchers.h -- the launchers of the kernels of ucf_device.h, included behind it by ucf_kernels_*.hip (UCF_FAST, UCF_NS and
// UCF_TU as there).  What a transform launch sequence does is decided in ucf_launch_plan.h (plan_transform, HIP-free);
// launch_transform_ enqueues the memsets and maps the plan onto template arguments, nothing else.

namespace UCF_NS {

#if !UCF_FAST
// (time, radius) grid -> the point list it stands for, point = it * nr + ir (the grid's own output order)
__global__ void __launch_bounds__(256)
expand_grid_kernel(int nt, int nr, const double* __restrict__ tDv, const int* __restrict__ svv, const double* __restrict__ rDv,
                   double* __restrict__ tDp, double* __restrict__ rDp, int* __restrict__ svp)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)nt * nr) return;
    const int it = (int)(q / nr), ir = (int)(q % nr);
    tDp[q] = tDv[it];
    svp[q] = svv[it];
    rDp[q] = rDv[ir];
}
int launch_expand_grid(int nt, int nr, const double* d_tD, const int* d_sv, const double* d_rD, double* d_tDp, double* d_rDp,
                       int* d_svp, void* stream)
{
    const long long n = (long long)nt * nr;
    hipLaunchKernelGGL(expand_grid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nt, nr, d_tD, d_sv, d_rD,
                       d_tDp, d_rDp, d_svp);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int launch_abscissae(const ucf_dev_params& dp, int nrows, int per_point, int nsv, int svmin, const double* d_rD,
                     const int* d_sv, double* d_tab, void* stream, double* d_ends)
{
    const long long total = (long long)nrows * (dp.N + dp.nacc * dp.ngl);
    const int threads = 256;
    const long long blocks = (total + threads - 1) / threads;
    hipLaunchKernelGGL(abscissa_kernel, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream, dp, nrows, per_point,
                       nsv, svmin, d_rD, d_sv, (double2*)d_tab, d_ends);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
#endif

// one kernel of a launch sequence: the large-LDS attribute on exactly this instantiation, its bracket / trace line, the launch
template <class K, class... A>
static void launch_named(K kernel, const char* name, ucf_timers* tm, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args)
{
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    ucf_tm_mark(tm, name, s);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}
#define UCF_EACH_FAMILY(fam, X) \
    switch (fam) { case 0: X(0); break; case 1: X(1); break; case 2: X(2); break; case 3: X(3); break; case 4: X(4); break; case 5: X(5); break; }
#define UCF_TF(b) ((b) ? "true" : "false")

// The transform stage for `nwork` work items of lane layout LAYOUT: [integrate kernel -> finish_kernel ->] point_kernel,
// as plan_transform (ucf_launch_plan.h) lays it out: every `if` and `case` below compares a field of that plan with a
// template argument, and a plan that names no instantiation of this translation unit is an error.
// tm (optional): every kernel of the stage is bracketed by HIP events on the launch stream (ucf_timers).
// (L.npts is not read here: nwork, from the layout launcher, says how much there is to do)
template <int LAYOUT, bool MULTI>
static int launch_transform_(const ucf_launch& L, int nwork)
{
    const ucf_dev_params& dp = *L.dp;
    const int per_point = L.per_point, nr = L.nr, nsv = L.nsv, svmin = L.svmin, nt = L.nt, ir0 = L.ir0;
    ucf_transform_plan P;
    const int rc = plan_transform(dp, ucf_env_get(), UCF_FAST != 0, LAYOUT, MULTI, nwork, per_point, nr, nt, &P);
    if (rc) return rc;
    const bool split = P.kind != 0;
    if (split && (!L.state || !L.ndone)) return UCF_ERR_BAD_ARGUMENT;
    // the shared buffers (ucf_transform_buffers)
    double2* const d_state = split ? (double2*)L.state : nullptr;
    int* const d_ndone = split ? L.ndone + P.buf.ndone : nullptr;
    int* const d_todo = split ? L.ndone + P.buf.todo : nullptr;
    int* const d_defer = split ? L.ndone + P.buf.defer : nullptr;
    ucf_timers* const tm = L.tm;
    // only a parameter batch reads these; it runs the water-table and Hantush families only (ucf_drawdown_multi), and nothing
    // else is instantiated for it
    const ucf_dev_params* d_params = MULTI ? L.params : nullptr;
    const int ppp = MULTI ? L.ppp : 1, pbase = MULTI ? L.pbase : 0;
#define UCF_BATCHABLE(F) (!MULTI || (F) == 1 || (F) == 2 || (F) == 4)
    char kname[96];
    hipStream_t s = (hipStream_t)L.stream;
    const dim3 block(UCF_WAVE);
    if (split) (void)hipMemsetAsync(d_todo, 0, sizeof(int), s);
#if UCF_FAST
    if (P.kind == 1) {
        // every item starts as "all abscissae done"; the parts that must stop lower it (integrate_kernel)
        (void)hipMemsetD32Async((hipDeviceptr_t)d_ndone, dp.N + dp.nacc * dp.ngl, (size_t)nwork, s);
        int* const d_wcount = L.ndone + P.buf.wcount;
        if (P.persist) (void)hipMemsetAsync(d_wcount, 0, sizeof(int), s);
        double2* const d_ltab = (double2*)((char*)L.state + P.buf.ltab);
#define UCF_LAUNCH_LT(F)                                                                                       \
    if constexpr (UCF_BATCHABLE(F))                                                                            \
        launch_named(laptime_kernel<F, MULTI>, UCF_STR(UCF_NS) "::laptime_kernel", tm, dim3(P.laptime_grid), dim3(256), 0, s, dp, P.nrows, L.tD, d_ltab, d_params, ppp, pbase)
        UCF_EACH_FAMILY(P.fam, UCF_LAUNCH_LT)
#undef UCF_LAUNCH_LT
        // one instantiation; it must be the one the plan names
#define UCF_LAUNCH_I4(F, W, FO, L3, NZC, L1, NF)                                                               \
    do {                                                                                                       \
        if (P.ik.waves != W || P.ik.fold != FO || P.ik.lay3 != L3 || P.ik.nzc != NZC || P.ik.lay1 != L1 || P.ik.nofold != NF) return UCF_ERR_UNSUPPORTED; \
        std::snprintf(kname, sizeof(kname), UCF_STR(UCF_NS) "::integrate_kernel<%d, %d, %d, %s, %s, %s, %d, %s, %s>", F, LAYOUT, W, UCF_TF(MULTI), UCF_TF(FO), UCF_TF(L3), NZC, UCF_TF(L1), UCF_TF(NF)); \
        launch_named(integrate_kernel<F, LAYOUT, W, MULTI, FO, L3, NZC, L1, NF>, kname, tm, dim3(P.integrate_grid), dim3(UCF_WAVE * UCF_IWPB), P.integrate_lds, s, \
                     dp, nwork, per_point, nr, nsv, svmin, L.tD, L.rD, L.sv, (const double2*)L.tab, nt, ir0, d_state, d_ndone, d_todo, d_params, ppp, pbase, \
                     P.lsplit | (P.ltail << 8), (const double2*)d_ltab, P.nrows, P.nhead << P.lsplit, (int)P.nworkw, P.persist ? d_wcount : (int*)nullptr); \
    } while (0)
        // (UCF_NZC / UCF_NZC2, ucf_launch_plan.h: the depth counts that (LAYOUT, F, FO) has an instantiation for; 0 = none)
#define UCF_LAUNCH_I3(F, W, FO, L3, L1, NF)                                                                    \
    do {                                                                                                       \
        if (P.ik.nzc == UCF_NZC(F, FO)) UCF_LAUNCH_I4(F, W, FO, L3, UCF_NZC(F, FO), L1, NF);                   \
        else if (P.ik.nzc == UCF_NZC2(F, FO)) UCF_LAUNCH_I4(F, W, FO, L3, UCF_NZC2(F, FO), L1, NF);            \
        else UCF_LAUNCH_I4(F, W, FO, L3, 0, L1, NF);                                                           \
    } while (0)
        // folded forms exist for one plan only (no parameter batch folds: plan_transform)
#define UCF_LAUNCH_FOLD(F, W) \
    do { if constexpr (!MULTI) UCF_LAUNCH_I3(F, W, true, false, true, false); else return UCF_ERR_UNSUPPORTED; } while (0)
        // three instantiations of an unfolded kernel: every layer / beside and below the screen / beside the screen only
#define UCF_LAUNCH_UNF_(F, W, NF)                                                                              \
    do {                                                                                                       \
        if (P.ik.lay3) UCF_LAUNCH_I3(F, W, false, true, true, NF);                                             \
        else if (P.ik.lay1) UCF_LAUNCH_I3(F, W, false, false, true, NF);                                       \
        else UCF_LAUNCH_I3(F, W, false, false, false, NF);                                                     \
    } while (0)
#define UCF_LAUNCH_UNF(F, W)                                                                                   \
    do {                                                                                                       \
        if constexpr (!UCF_BATCHABLE(F)) return UCF_ERR_UNSUPPORTED;                                           \
        else if (P.ik.nofold) UCF_LAUNCH_UNF_(F, W, true);                                                     \
        else UCF_LAUNCH_UNF_(F, W, false);                                                                     \
    } while (0)
#define UCF_LAUNCH_FU(F, W) do { if (P.ik.fold) UCF_LAUNCH_FOLD(F, W); else UCF_LAUNCH_UNF(F, W); } while (0)
        switch (P.fam) {
        case 0: if (P.ik.waves == 6) UCF_LAUNCH_FOLD(0, 6); else UCF_LAUNCH_FOLD(0, 4); break;
        case 3: UCF_LAUNCH_FOLD(3, 4); break;
        case 5: UCF_LAUNCH_FU(5, 4); break;
        case 1: UCF_LAUNCH_FU(1, 4); break;
        case 2:
            if (P.ik.fold) {
                if (P.ik.waves == 4) UCF_LAUNCH_FOLD(2, 4);
                else if (P.ik.waves == 6) UCF_LAUNCH_FOLD(2, 6);
                else UCF_LAUNCH_FOLD(2, UCF_FOLD_WAVES);
            } else {
                if (P.ik.waves == 3) UCF_LAUNCH_UNF(2, 3);
                else UCF_LAUNCH_UNF(2, UCF_UNFOLD_WAVES);
            }
            break;
        case 4: UCF_LAUNCH_FU(4, 4); break;
        }
#undef UCF_LAUNCH_FU
#undef UCF_LAUNCH_FOLD
#undef UCF_LAUNCH_UNF
#undef UCF_LAUNCH_UNF_
#undef UCF_LAUNCH_I3
#undef UCF_LAUNCH_I4
    }
#else
    if (P.kind == 2) {      // (the fast flavour has integrate_kernel for every family)
#define UCF_LAUNCH_G(F)                                                                                        \
    do {                                                                                                       \
        std::snprintf(kname, sizeof(kname), UCF_STR(UCF_NS) "::integrate_generic_kernel<%d, %d>", F, LAYOUT);  \
        launch_named(integrate_generic_kernel<F, LAYOUT>, kname, tm, dim3((unsigned)nwork), block, P.generic_lds, s, dp, nwork, per_point, nr, nsv, svmin, \
                     L.tD, L.rD, L.sv, (const double2*)L.tab, nt, ir0, d_state, d_ndone);                      \
    } while (0)
        UCF_EACH_FAMILY(P.fam, UCF_LAUNCH_G)
#undef UCF_LAUNCH_G
    }
#endif
    if (split) {
        if (hipGetLastError() != hipSuccess) return UCF_ERR_HIP;
        // tails of the completed items
#define UCF_LAUNCH_FM(PART, WR, MODE, GRID)                                                                     \
    do {                                                                                                       \
        std::snprintf(kname, sizeof(kname), UCF_STR(UCF_NS) "::finish_kernel<%d, %d, %s, %d>", LAYOUT, PART, UCF_TF(WR), MODE); \
        launch_named(finish_kernel<LAYOUT, PART, WR, MODE>, kname, tm, dim3((unsigned)(GRID)), block, P.finish_lds, s, dp, nwork, per_point, nr, nsv, svmin, \
                     L.tD, L.rD, L.sv, L.h, L.dh, L.stats, nt, ir0, (double2*)L.totlap, (const double2*)d_state, (const int*)d_ndone, d_defer); \
    } while (0)
        if (P.fin.two_pass) (void)hipMemsetAsync(d_defer, 0, sizeof(int), s);
        // (two passes: the fast flavour with the epsilon table in registers, and only that)
#define UCF_LAUNCH_F(PART, WR)                                                                                 \
    do {                                                                                                       \
        if (P.fin.two_pass != (UCF_FAST && (WR))) return UCF_ERR_UNSUPPORTED;                                  \
        if constexpr (UCF_FAST && (WR)) {                                                                      \
            UCF_LAUNCH_FM(PART, WR, 1, nwork);                                                                 \
            UCF_LAUNCH_FM(PART, WR, 2, P.finish_grid2);                                                        \
        } else UCF_LAUNCH_FM(PART, WR, 0, nwork);                                                              \
    } while (0)
        if (P.fin.wreg) { if (P.fin.part == 64) UCF_LAUNCH_F(64, true); else if (P.fin.part == 32) UCF_LAUNCH_F(32, true); else UCF_LAUNCH_F(16, true); }
        else if (P.fin.part == 64) UCF_LAUNCH_F(64, false);
        else if (P.fin.part == 32) UCF_LAUNCH_F(32, false);
        else UCF_LAUNCH_F(16, false);
#undef UCF_LAUNCH_F
#undef UCF_LAUNCH_FM
        if (hipGetLastError() != hipSuccess) return UCF_ERR_HIP;
        if (P.kind == 2) { ucf_tm_close(tm, s); return UCF_OK; }      // the generic evaluators leave nothing unfinished
    }
    // kind 1: the unfinished items (overflow regime), over the list integrate_kernel left; kind 0: everything
#define UCF_LAUNCH(F)                                                                                          \
    do {                                                                                                       \
        if constexpr (!UCF_BATCHABLE(F)) return UCF_ERR_UNSUPPORTED;                                           \
        else {                                                                                                 \
            std::snprintf(kname, sizeof(kname), UCF_STR(UCF_NS) "::point_kernel<%d, %d, %s>", F, LAYOUT, UCF_TF(MULTI)); \
            launch_named(point_kernel<F, LAYOUT, MULTI>, kname, tm, dim3(P.point_grid), block, P.point_lds, s, dp, nwork, per_point, nr, nsv, svmin, L.tD, L.rD, L.sv, \
                         (const double2*)L.tab, L.h, L.dh, L.stats, nt, ir0, L.nrc, (double2*)L.totlap, (double2*)(P.global_areas ? L.glscr : nullptr), \
                         d_state, (const int*)d_ndone, (const int*)d_todo, d_params, ppp, pbase);              \
        }                                                                                                      \
    } while (0)
    UCF_EACH_FAMILY(P.fam, UCF_LAUNCH)
#undef UCF_LAUNCH
#undef UCF_BATCHABLE
    ucf_tm_close(tm, s);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

// L.params != NULL: parameter-batched launch (per-point layouts of the fast flavour only), plan k owns points
// [k ppp, (k+1) ppp) and reads L.params[k]; L.dp is plan 0's block
template <int LAYOUT>
static int launch_transform(const ucf_launch& L, int nwork)
{
#if UCF_FAST
    if (L.params) {
        // parameter batches run in the per-point layouts 0, 2, 3 (the lane = time translation unit instantiates none of it)
        if constexpr (LAYOUT == 1) return UCF_ERR_BAD_ARGUMENT;
        else return L.per_point ? launch_transform_<LAYOUT, true>(L, nwork) : UCF_ERR_BAD_ARGUMENT;
    }
#else
    if (L.params) return UCF_ERR_UNSUPPORTED;
#endif
    return launch_transform_<LAYOUT, false>(L, nwork);
}

#if UCF_TU_HAS(0)
// LAYOUT 0 (lane = Laplace sample, de Hoog in the same wave)
int launch_points(const ucf_launch& L)
{
    ucf_launch T = L;
    T.nt = T.ir0 = T.nrc = 0; T.tm = nullptr;      // a point list has neither
    return launch_transform<0>(T, L.npts);
}

#endif

#if UCF_TU_HAS(1)
// LAYOUT 1 (lane = time): transform kernel(s) over (radius chunk x time tiles x Laplace index), then de Hoog
int launch_grid_transposed(const ucf_launch& L)
{
    const ucf_dev_params& dp = *L.dp;
    const int nt = L.nt, nr = L.nr, ir0 = L.ir0, nrc = L.nrc;
    ucf_timers* tm = L.tm;
    hipStream_t s = (hipStream_t)L.stream;
    const int ntiles = (nt + UCF_WAVE - 1) / UCF_WAVE;
    const long long nwork = (long long)nrc * ntiles * dp.np;
    if (nwork > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    ucf_launch T = L;         // one split index for all times, no parameter batch
    T.per_point = 0; T.nsv = 1; T.sv = nullptr; T.params = nullptr;
    int rc = launch_transform<1>(T, (int)nwork);
    if (rc) return rc;
    const long long ntl = (long long)nrc * ((nt + UCF_DH_TILE - 1) / UCF_DH_TILE);
    const size_t dlds = 2 * (size_t)dp.np * (UCF_DH_TILE + 1) * sizeof(lds_c) + 2 * UCF_DH_TILE * sizeof(int);
    // (one workgroup per tile: a capped grid walking the tiles with a stride is SLOWER -- C2 1.34 ms against 1.99 / 1.55 / 1.44 /
    //  1.37 ms with 2 048 / 4 096 / 8 192 / 16 384 workgroups, measured: a static stride cannot rebalance what the dispatcher does)
    const dim3 dgrid((unsigned)(ntl > 0x7fffffffLL ? 0x7fffffff : ntl));
    if (dp.np <= UCF_WAVE) {
        ucf_tm_mark(tm, UCF_STR(UCF_NS) "::dehoog_tiles_kernel<1, false>", s);
        hipLaunchKernelGGL((dehoog_tiles_kernel<1, false>), dgrid, dim3(UCF_WAVE), dlds, s, dp, nt, nr, ir0, nrc, L.tD, (const double2*)L.totlap, L.h, L.dh, L.stats);
    } else {
        ucf_tm_mark(tm, UCF_STR(UCF_NS) "::dehoog_tiles_kernel<1, true>", s);
        hipLaunchKernelGGL((dehoog_tiles_kernel<1, true>), dgrid, dim3(UCF_WAVE), dlds, s, dp, nt, nr, ir0, nrc, L.tD, (const double2*)L.totlap, L.h, L.dh, L.stats);
    }
    ucf_tm_close(tm, s);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

#endif

#if UCF_TU_HAS(3)
// LAYOUT 3 (lane = point of an arbitrary list, 2M+1 <= 64): npts points, ppp of them per plan (npts for one plan);
// transform over (64-point tiles x Laplace index), then the tiled de Hoog with the points in the place of the times
int launch_points_lanes(const ucf_launch& L)
{
    const ucf_dev_params& dp = *L.dp;
    const int npts = L.npts, ppp = L.params ? L.ppp : npts;
    hipStream_t s = (hipStream_t)L.stream;
    if (ppp < 1 || npts % ppp != 0 || dp.np > UCF_WAVE) return UCF_ERR_BAD_ARGUMENT;
    const long long nwork = (long long)(npts / ppp) * ((ppp + UCF_WAVE - 1) / UCF_WAVE) * dp.np;
    if (nwork > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    ucf_launch T = L;         // the transform sees a plan's points as the radii of one row, the launch's points as its times
    T.per_point = 1; T.nr = ppp; T.ppp = ppp; T.nsv = 1; T.svmin = 0; T.nt = npts; T.ir0 = T.nrc = 0;
    T.glscr = nullptr; T.tm = nullptr;
    int rc = launch_transform<3>(T, (int)nwork);
    if (rc) return rc;
    const long long ntl = (npts + UCF_DH_TILE - 1) / UCF_DH_TILE;
    const size_t dlds = 2 * (size_t)dp.np * (UCF_DH_TILE + 1) * sizeof(lds_c) + 2 * UCF_DH_TILE * sizeof(int);
    if (dp.np <= UCF_WAVE)
        hipLaunchKernelGGL((dehoog_tiles_kernel<3, false>), dim3((unsigned)ntl), dim3(UCF_WAVE), dlds, s, dp, npts, 1, 0, 1, L.tD,
                           (const double2*)L.totlap, L.h, L.dh, L.stats);
    else
        hipLaunchKernelGGL((dehoog_tiles_kernel<3, true>), dim3((unsigned)ntl), dim3(UCF_WAVE), dlds, s, dp, npts, 1, 0, 1, L.tD,
                           (const double2*)L.totlap, L.h, L.dh, L.stats);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
#endif

#if UCF_TU_HAS(2)
// LAYOUT 2 (2M+1 > 64): (point, 64-sample chunk) work items write the transform, dehoog_points_kernel inverts.
// Same addressing as launch_points; d_h/d_dh/d_totlap point at this chunk of points.
int launch_points_chunked(const ucf_launch& L)
{
    const ucf_dev_params& dp = *L.dp;
    const int npts = L.npts;
    hipStream_t s = (hipStream_t)L.stream;
    const int nchunk = (dp.np + UCF_WAVE - 1) / UCF_WAVE;
    const long long nwork = (long long)npts * nchunk;
    if (nwork > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    ucf_launch T = L;
    T.nt = T.ir0 = T.nrc = 0; T.tm = nullptr;      // a point list has neither
    int rc = launch_transform<2>(T, (int)nwork);
    if (rc) return rc;
    hipLaunchKernelGGL(dehoog_points_kernel, dim3((unsigned)npts), dim3(UCF_WAVE), 0, s, dp, (long long)npts, 1, L.per_point, L.nr, 0, 0, L.tD,
                       (const double2*)L.totlap, L.h, L.dh, L.stats);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

#endif

#if UCF_TU_HAS(1)
int launch_samples(const ucf_dev_params& dp, int n_a, const double* d_a, double rD, const double* d_p, double* d_fp,
                   void* stream)
{
    const int fam = family_of(dp);
    if (fam < 0) return UCF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = samples_lds_bytes(dp, UCF_FAST != 0);
    dim3 grid(n_a), block(UCF_WAVE);
#define UCF_LAUNCH(F)                                                                                          \
    do {                                                                                                       \
        if (lds > 64 * 1024)                                                                                   \
            (void)hipFuncSetAttribute((const void*)samples_kernel<F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL(samples_kernel<F>, grid, block, lds, s, dp, n_a, d_a, rD, d_p, d_fp);               \
    } while (0)
    switch (fam) {
    case 0: UCF_LAUNCH(0); break;
    case 1: UCF_LAUNCH(1); break;
    case 2: UCF_LAUNCH(2); break;
    case 3: UCF_LAUNCH(3); break;
    case 4: UCF_LAUNCH(4); break;
    case 5: UCF_LAUNCH(5); break;
    }
#undef UCF_LAUNCH
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

#endif

#if !UCF_FAST
int launch_bessel(int n, const double* d_z, double* d_k, int* d_ierr, void* stream)
{
    hipLaunchKernelGGL(bessel_kernel, dim3((n + UCF_WAVE - 1) / UCF_WAVE), dim3(UCF_WAVE), 0, (hipStream_t)stream, n, d_z, d_k, d_ierr);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
int launch_dehoog(int n, int M, double alpha, double logtol, const double* d_t, const double* d_tee,
                  const double* d_fp, double* d_ft, void* stream)
{
    hipLaunchKernelGGL(dehoog_kernel, dim3(n), dim3(UCF_WAVE), 0, (hipStream_t)stream, n, M, alpha, logtol, d_t, d_tee,
                       d_fp, d_ft);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
int launch_wynn(int n, int nterms, const double* d_series, double* d_acc, int* d_status, void* stream)
{
    const size_t lds = 2 * (size_t)nterms * UCF_PART * sizeof(lds_c);
    hipLaunchKernelGGL(wynn_kernel, dim3((n + UCF_WAVE - 1) / UCF_WAVE), dim3(UCF_WAVE), lds, (hipStream_t)stream, n,
                       nterms, d_series, d_acc, d_status);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
int launch_extrap(int n, int R, const double* d_x, const double* d_y, double* d_out, void* stream)
{
    const size_t lds = ((size_t)R * UCF_WAVE + (size_t)R * UCF_PART) * sizeof(lds_c);
    hipLaunchKernelGGL(extrap_kernel, dim3((n + UCF_WAVE - 1) / UCF_WAVE), dim3(UCF_WAVE), lds, (hipStream_t)stream, n,
                       R, d_x, d_y, d_out);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
#endif

}  // namespace UCF_NS
