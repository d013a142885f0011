// ucf_drawdown.cpp -- the hot path of the host side: the per-stream workspaces of a plan, the chunked launch drivers of
// grids and point lists, the device-side ordering of a point list by radius (three small kernels and the rocPRIM radix
// sort: the only host source with kernels), the *_device entries and the host-array entries of one device.
#include <array>
#include <cstring>
#include <new>
#include <mutex>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>   // (after <cstring>: its headers use memset on the host)

#include "ucf_host.h"

using namespace ucf_host;

namespace {

void ws_release_retired(ucf_workspace* ws)
{
    for (void* q : ws->retired) (void)hipFree(q);
    ws->retired.clear();
}

// every device buffer of a workspace (ucf_plan.h): the one list, ws_destroy frees through it
std::array<ucf_buffer*, 8> ws_buffers(ucf_workspace& w)
{
    return {{&w.work, &w.totlap, &w.glscr, &w.expand, &w.sort, &w.state, &w.ndone, &w.pblocks}};
}

// scratch for the finished interval areas of every resident workgroup
int ensure_glscr(ucf_plan* pl, ucf_workspace* ws, int nz)
{
    return ws_ensure(pl, ws, ws->glscr, (size_t)ucf_env_get().grid_slots * pl->P.nacc * nz * UCF_WAVE * 2 * sizeof(double), "interval-area scratch");
}

// (lt_rows: rows of the call's tD array that one launch covers -- the fast flavour keeps lapTime(p) of every (row, m) behind
//  the state of the launch's items; ucf_transform_buffers has the layout of both buffers)
int ensure_state(ucf_plan* pl, ucf_workspace* ws, const ucf_dev_params& dp, size_t items, size_t lt_rows)
{
    const ucf_transform_buffers b = buffers_of(pl, dp, items, lt_rows);
    if (items == 0 || b.state_item_bytes == 0) return UCF_OK;
    int rc = ws_ensure(pl, ws, ws->state, b.state_bytes, "integration state");
    if (rc) return rc;
    return ws_ensure(pl, ws, ws->ndone, b.ints * sizeof(int), "work-item counters");
}

// work items per launch such that their state stays within UCF_STATE_BYTES (default 8 GiB of the 288 GB)
size_t state_budget() { return ucf_env_get().state_bytes; }
// lane layout of arbitrary point lists: 3 = lane is a point (all 64 lanes live whatever M is), 0 = lane is a Laplace
// sample (2M+1 of 64 lanes live).  UCF_BATCH_LAYOUT=0 forces the latter (diagnostic).
int batch_layout() { return ucf_env_get().batch_layout; }

// arbitrary points with the parameter block dp: one abscissa-table row per point, in chunks that keep the table within
// UCF_TABLE_BYTES
int batch_points(ucf_plan* pl, ucf_workspace* ws, const ucf_dev_params& dp, int npts, const double* d_tD, const double* d_rD, const int* d_sv,
                 double* d_h, double* d_dh, ucf_stats* d_stats, void* stream)
{
    const size_t row_bytes = (size_t)pl->D.nabs * 2 * sizeof(double);
    int chunk = (int)(table_budget() / row_bytes);
    if (chunk < 1) chunk = 1;
    if (chunk > npts) chunk = npts;
    int rc = ws_ensure(pl, ws, ws->work, (size_t)chunk * row_bytes, "abscissa table");
    if (rc) return rc;
    ucf_launch L;
    L.dp = &dp; L.per_point = 1; L.nr = 1; L.stats = d_stats; L.stream = stream;
    for (int base = 0; base < npts; base += chunk) {
        L.npts = (npts - base < chunk) ? npts - base : chunk;
        L.tD = d_tD + base; L.rD = d_rD + base; L.sv = d_sv + base;
        L.h = d_h + (size_t)base * dp.nz_out; L.dh = d_dh + (size_t)base * dp.nz_out;
        if (!ws->dry) {
            rc = ucf_faithful::launch_abscissae(dp, L.npts, 1, 1, 0, L.rD, L.sv, (double*)ws->work.p, stream);
            if (rc) return fail(rc, "abscissa kernel launch failed");
        }
        rc = launch_points_any(pl, ws, L, npts);
        if (rc) return rc;
    }
    return UCF_OK;
}

// lane = time needs one split index for all times and fills the wave better than lane = Laplace sample
bool grid_lane_time(const ucf_plan* pl, int nt)
{
    const int* j0s = pl->P.j0s;
    const int nsv = (j0s[0] > j0s[1] ? j0s[0] - j0s[1] : j0s[1] - j0s[0]) + 1;
    const int ntiles = (nt + UCF_WAVE - 1) / UCF_WAVE;
    return nsv == 1 && (double)nt / (64.0 * ntiles) > (double)pl->D.np / (64.0 * ((pl->D.np + 63) / 64)) && !pl->force_layout0;
}

int grid_device_chunk(ucf_plan* pl, ucf_workspace* ws, int nt, const double* d_tD, const int* d_sv, int nr, const double* d_rD,
                      int nz, const double* zD, const int* zLay, int nz_out, int z_off, double* d_h, double* d_dh,
                      ucf_stats* d_stats, void* stream, bool timed)
{
    ucf_dev_params dp;
    int rc = fill_call_params(pl, nz, zD, zLay, dp, nz_out, z_off);
    if (rc) return rc;
    const int* j0s = pl->P.j0s;
    const int svmin = j0s[0] < j0s[1] ? j0s[0] : j0s[1];
    const int nsv = (j0s[0] > j0s[1] ? j0s[0] - j0s[1] : j0s[1] - j0s[0]) + 1;     // driver_io.f90:660-664: sv in [min,max]
    const size_t nabs = (size_t)pl->D.nabs;
    // (the rows, and behind them the ends of every row's J0 intervals: abscissa_ends_offset, ucf_launch_plan.h)
    rc = ws_ensure(pl, ws, ws->work, abscissa_table_doubles((size_t)nr * nsv, nabs, (size_t)pl->P.nacc) * sizeof(double), "abscissa table");
    if (rc) return rc;
    const int ntiles = (nt + UCF_WAVE - 1) / UCF_WAVE;
    const bool lane_time = grid_lane_time(pl, nt);
    // the kernels of a single-chunk lane = time call are bracketed by events when timing is on
    int nrc = nr;
    size_t per_radius = 0;
    if (lane_time) {
        per_radius = (size_t)nt * nz * pl->D.np * 2 * sizeof(double);
        nrc = (int)(((size_t)1 << 30) / per_radius);           // <= 1 GiB of workspace per chunk of radii
        const size_t state_per_radius = state_item_bytes(pl, dp) * ntiles * pl->D.np;
        if (state_per_radius && (size_t)nrc > state_budget() / state_per_radius) nrc = (int)(state_budget() / state_per_radius);
        if (nrc < 1) nrc = 1;
        if (nrc > nr) nrc = nr;
    }
    ucf_timers* tm = nullptr;
    if (timed && lane_time && !ws->dry) {
        tm = &ws->tm;
        tm->n = 0;
        tm->open = 0;
        ws->tm_valid = 1;
        std::lock_guard<std::mutex> g(pl->mu);
        pl->last_timed = ws;
    }
    if (!ws->dry) {
        ucf_tm_mark(tm, "ucf_faithful::abscissa_kernel", stream);
        rc = ucf_faithful::launch_abscissae(dp, nr * nsv, 0, nsv, svmin, d_rD, d_sv, (double*)ws->work.p, stream,
                                            (double*)ws->work.p + abscissa_ends_offset((size_t)nr * nsv, nabs));
        if (rc) return fail(rc, "abscissa kernel launch failed");
    }
    ucf_launch L;
    L.dp = &dp; L.nr = nr; L.nsv = nsv; L.svmin = svmin;
    L.tD = d_tD; L.rD = d_rD; L.sv = d_sv; L.h = d_h; L.dh = d_dh; L.stats = d_stats; L.stream = stream;
    if (lane_time) {
        rc = ensure_state(pl, ws, dp, (size_t)nrc * ntiles * pl->D.np, (size_t)nt);
        if (rc) return rc;
        rc = ws_ensure(pl, ws, ws->totlap, per_radius * nrc, "transform workspace");
        if (rc) return rc;
        rc = ensure_glscr(pl, ws, nz);
        if (rc) return rc;
        if (ws->dry) return UCF_OK;
        L.nt = nt; L.tm = tm;
        L.tab = (double*)ws->work.p; L.totlap = (double*)ws->totlap.p; L.glscr = (double*)ws->glscr.p;
        L.state = (double*)ws->state.p; L.ndone = (int*)ws->ndone.p;
        for (int ir0 = 0; ir0 < nr; ir0 += nrc) {
            const int n = (nr - ir0 < nrc) ? nr - ir0 : nrc;
            L.ir0 = ir0; L.nrc = n;
            if (ws->dbg) {
                ucf_debug_rec& r = *ws->dbg;
                r.count++;
                r.layout = 1; r.per_point = 0; r.nr = nr; r.nt = nt; r.ir0 = ir0; r.nrc = n; r.npts = nt * nr;
                r.nwork = n * ntiles * pl->D.np;
            }
            rc = flavour_of(pl).launch_grid_transposed(L);
            if (rc) return launch_failed(rc, dp);
        }
        return UCF_OK;
    }
    L.npts = nt * nr;          // the grid walked point by point (per_point = 0)
    return launch_points_any(pl, ws, L, L.npts);
}

// (C names, as the code object has always named them: no signature in the kernel names of the library's smallest kernels)
extern "C" __global__ void iota_kernel(int n, int* v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
extern "C" __global__ void gather_points_kernel(int n, const int* __restrict__ perm, const double* __restrict__ tD, const int* __restrict__ sv,
                                     double* __restrict__ tDs, int* __restrict__ svs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { tDs[i] = tD[perm[i]]; svs[i] = sv[perm[i]]; }
}
extern "C" __global__ void scatter_results_kernel(int n, int nz, const int* __restrict__ perm, const double* __restrict__ hs,
                                       const double* __restrict__ dhs, double* __restrict__ h, double* __restrict__ dh)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * nz) return;
    const int i = (int)(e / nz), z = (int)(e % nz);
    h[(size_t)perm[i] * nz + z] = hs[e];
    dh[(size_t)perm[i] * nz + z] = dhs[e];
}

int batch_device_all_depths(ucf_plan* pl, ucf_workspace* ws, int npts, const double* d_tD, const double* d_rD, const int* d_sv,
                            int nz, const double* zD, const int* zLay, double* d_h, double* d_dh, ucf_stats* d_stats, void* stream)
{
    const int zc = z_chunk(pl);
    for (int z0 = 0; z0 < nz; z0 += zc) {
        const int n = (nz - z0 < zc) ? nz - z0 : zc;
        ucf_dev_params dp;
        int rc = fill_call_params(pl, n, zD + z0, zLay + z0, dp, nz, z0);
        if (rc) return rc;
        rc = batch_points(pl, ws, dp, npts, d_tD, d_rD, d_sv, d_h, d_dh, d_stats, stream);
        if (rc) return rc;
    }
    return UCF_OK;
}

int check_sv_of(const ucf_params& P, const ucf_derived& D, int n, const int* sv)
{
    for (int i = 0; i < n; i++)
        if (sv[i] < 1 || sv[i] + P.nacc > D.nj0z)
            return fail(UCF_ERR_BAD_ARGUMENT, "sv[%d]=%d outside 1..%d", i, sv[i], D.nj0z - P.nacc);
    return UCF_OK;
}

}  // namespace

namespace ucf_host {

// the workspace of `stream` inside the plan (created on first use)
ucf_workspace* ws_for(ucf_plan* pl, void* stream)
{
    std::lock_guard<std::mutex> g(pl->mu);
    for (ucf_workspace* w : pl->ws)
        if (w->stream == stream) return w;
    ucf_workspace* w = new (std::nothrow) ucf_workspace();
    if (!w) return nullptr;
    w->stream = stream;
    pl->ws.push_back(w);
    return w;
}

// the plan's own stream (on the plan's device, which the caller has made current)
hipStream_t plan_stream(ucf_plan* pl)
{
    std::lock_guard<std::mutex> g(pl->mu);
    if (!pl->own_stream) {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
        pl->own_stream = s;
    }
    return (hipStream_t)pl->own_stream;
}

// Grow a workspace buffer.  Nothing synchronises here: a buffer that kernels of earlier calls on this stream may still
// read is retired, not freed; retired buffers go when the stream is found idle by a later growth, at ucf_plan_reserve
// or with the plan.  (hipFree waits for the whole device, so it is only ever called when this stream has drained.)
int ws_ensure(ucf_plan* pl, ucf_workspace* ws, ucf_buffer& b, size_t bytes, const char* what)
{
    if (b.bytes >= bytes && b.p) return UCF_OK;
    if (bytes == 0) bytes = 8;
    void *p = nullptr, *base = nullptr;
    if (guarded_malloc(&p, &base, bytes) != hipSuccess) {
        (void)hipGetLastError();
        // last resort before giving up: drain this stream and drop what it no longer needs
        (void)hipStreamSynchronize((hipStream_t)ws->stream);
        ws_release_retired(ws);
        free_buffer(b);
        if (guarded_malloc(&p, &base, bytes) != hipSuccess) return fail(UCF_ERR_NOMEM, "hipMalloc of %zu bytes (%s) failed", bytes, what);
    }
    if (b.p) ws->retired.push_back(b.base);
    b.p = p;
    b.base = base;
    b.bytes = bytes;
    {
        std::lock_guard<std::mutex> g(pl->mu);
        pl->n_alloc++;
    }
    if (ws->dry && !ws->retired.empty() && hipStreamQuery((hipStream_t)ws->stream) == hipSuccess) ws_release_retired(ws);
    return UCF_OK;
}

// with the plan (ucf_plan_destroy: the plan's device is current)
void ws_destroy(ucf_workspace* ws)
{
    for (ucf_buffer* b : ws_buffers(*ws)) free_buffer(*b);
    ws_release_retired(ws);
    for (void* e : ws->tm.ev) if (e) (void)hipEventDestroy((hipEvent_t)e);
    delete ws;
}

// `call`: the points of one abscissa table (dp, npts, per_point, nr, nsv, svmin, tD, rD, sv, h, dh, stats, stream and, for a
// parameter batch, params / ppp / pbase: plan of point q = (pbase + q) / ppp, pbase a multiple of ppp).  The workspace
// pointers are filled in here and the points go out in launches that keep the state within its budget.
// npts_call: points of the whole call that `call` is a part of
int launch_points_any(ucf_plan* pl, ucf_workspace* ws, const ucf_launch& call, int npts_call)
{
    const ucf_dev_params& dp = *call.dp;
    const int npts = call.npts, per_point = call.per_point, nr = call.nr, ppp = call.ppp;
    const bool batch = call.params != nullptr;
    int rc = ensure_glscr(pl, ws, dp.nz);
    if (rc) return rc;
    const bool chunked = pl->D.np > UCF_WAVE;     // more Laplace samples than lanes: (point, 64-sample chunk) work items
    const size_t per_item = state_item_bytes(pl, dp);
    // lane = point when that fills the waves better and the abscissa loop has its own kernel
    // (decided on the size of the whole call, npts_call, so that the chunking of a long list cannot change a bit)
    const bool lanes = batch_layout() == 3 && per_point && !chunked && per_item != 0 && !pl->force_layout0 &&
                       npts_call >= 4 * UCF_WAVE && (!batch || ppp >= UCF_WAVE / 2);
    const int items_per_pt = chunked ? (pl->D.np + UCF_WAVE - 1) / UCF_WAVE : 1;
    // points per launch: bounded by the integration-state budget; a grid (per_point = 0) is cut at whole time rows,
    // a parameter batch in the lane = point layout at whole plans
    size_t step = (size_t)npts;
    size_t items = 0;
    if (lanes) {
        const size_t unit = batch ? (size_t)ppp : UCF_WAVE;                                      // points that go together
        const size_t unit_items = (size_t)((unit + UCF_WAVE - 1) / UCF_WAVE) * pl->D.np;          // their work items
        size_t nunits = state_budget() / (per_item * unit_items);
        if (nunits < 1) nunits = 1;
        step = nunits * unit;
        if (step > (size_t)npts) step = npts;
        items = ((step + unit - 1) / unit) * unit_items;
    } else if (per_item) {
        step = state_budget() / (per_item * items_per_pt);
        if (!per_point) step = (step / nr) * nr;
        if (step < (size_t)(per_point ? 1 : nr)) step = per_point ? 1 : nr;
        if (step > (size_t)npts) step = npts;
        items = step * items_per_pt;
    }
    if (per_item) {
        rc = ensure_state(pl, ws, dp, items, step);
        if (rc) return rc;
    }
    if (chunked || lanes) {
        rc = ws_ensure(pl, ws, ws->totlap, step * dp.nz * pl->D.np * 2 * sizeof(double), "transform workspace");
        if (rc) return rc;
    }
    if (ws->dry) return UCF_OK;
    const ucf_flavour& F = flavour_of(pl);
    const auto launch = lanes ? F.launch_points_lanes : chunked ? F.launch_points_chunked : F.launch_points;
    double* const w_work = (double*)ws->work.p;
    const size_t nabs = (size_t)pl->D.nabs;
    ucf_launch L = call;
    // (lane layout 0 keeps no transform; ucf_debug_stages lends it a buffer)
    L.totlap = (lanes || chunked) ? (double*)ws->totlap.p : ws->dbg ? ws->dbg->d_totlap0 : nullptr;
    L.glscr = (double*)ws->glscr.p;
    L.state = (double*)ws->state.p;
    L.ndone = (int*)ws->ndone.p;
    for (size_t base = 0; base < (size_t)npts; base += step) {
        const int n = (int)(((size_t)npts - base < step) ? (size_t)npts - base : step);
        // per_point: everything is indexed by the point; grid: times (and their split indices) by the row
        const size_t tb = per_point ? base : base / nr;
        L.npts = n;
        L.tD = call.tD + tb;
        L.sv = call.sv + tb;
        L.rD = per_point ? call.rD + base : call.rD;
        L.tab = per_point ? w_work + base * nabs * 2 : w_work;
        L.h = call.h + base * dp.nz_out;
        L.dh = call.dh + base * dp.nz_out;
        L.pbase = call.pbase + (int)base;
        if (ws->dbg) {           // ucf_debug_stages: what is launched, as the gather kernel will decode it
            ucf_debug_rec& r = *ws->dbg;
            r.count++;
            r.layout = lanes ? 3 : chunked ? 2 : 0;
            r.per_point = per_point; r.ir0 = 0; r.nrc = 0; r.npts = n;
            if (lanes) { const int pp = batch ? ppp : n; r.nr = pp; r.nt = n; r.nwork = (int)((size_t)(n / pp) * ((pp + UCF_WAVE - 1) / UCF_WAVE) * pl->D.np); r.per_point = 1; }
            else { r.nr = nr; r.nt = 0; r.nwork = n * items_per_pt; }
        }
        rc = launch(L);
        if (rc) return launch_failed(rc, dp);
    }
    return UCF_OK;
}

// presorted: the caller (ucf_drawdown_batch) already put the points in order of radius
int batch_device_impl(ucf_plan* pl, ucf_workspace* ws, int npts, const double* d_tD, const double* d_rD, const int* d_sv,
                      int nz, const double* zD, const int* zLay, double* d_h, double* d_dh, ucf_stats* d_stats, void* stream,
                      bool presorted)
{
    if (presorted || npts < 4 * UCF_WAVE || batch_layout() != 3)
        return batch_device_all_depths(pl, ws, npts, d_tD, d_rD, d_sv, nz, zD, zLay, d_h, d_dh, d_stats, stream);
    // lane = point wants the 64 points of a wave to be neighbours in radius (see ucf_drawdown_batch): sort by radius on
    // the device (rocPRIM radix sort of (rD, index)), evaluate, scatter the results back to the caller's order
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)npts;
    size_t temp_bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, temp_bytes, d_rD, (double*)nullptr, (int*)nullptr, (int*)nullptr, n, 0, 64, s) != hipSuccess)
        return fail(UCF_ERR_HIP, "rocprim::radix_sort_pairs (size query) failed");
    // one allocation: keys_out | tD_s | h_s | dh_s | idx_in | idx_out | sv_s | sort temp
    const size_t off_keys = 0, off_t = off_keys + n * 8, off_h = off_t + n * 8, off_d = off_h + n * nz * 8, off_i0 = off_d + n * nz * 8,
                 off_i1 = off_i0 + n * 4, off_sv = off_i1 + n * 4, off_tmp = (off_sv + n * 4 + 255) / 256 * 256, total = off_tmp + temp_bytes;
    int rc = ws_ensure(pl, ws, ws->sort, total, "sort workspace");
    if (rc) return rc;
    char* base = (char*)ws->sort.p;
    double* keys = (double*)(base + off_keys);
    double* tDs = (double*)(base + off_t);
    double* hs = (double*)(base + off_h);
    double* dhs = (double*)(base + off_d);
    int* i0 = (int*)(base + off_i0);
    int* i1 = (int*)(base + off_i1);
    int* svs = (int*)(base + off_sv);
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (!ws->dry) {
        hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, s, npts, i0);
        if (rocprim::radix_sort_pairs(base + off_tmp, temp_bytes, d_rD, keys, i0, i1, n, 0, 64, s) != hipSuccess)
            return fail(UCF_ERR_HIP, "rocprim::radix_sort_pairs failed");
        hipLaunchKernelGGL(gather_points_kernel, dim3(nb), dim3(256), 0, s, npts, i1, d_tD, d_sv, tDs, svs);
    }
    rc = batch_device_all_depths(pl, ws, npts, tDs, keys, svs, nz, zD, zLay, hs, dhs, d_stats, stream);
    if (rc || ws->dry) return rc;
    hipLaunchKernelGGL(scatter_results_kernel, dim3((unsigned)((n * nz + 255) / 256)), dim3(256), 0, s, npts, nz, i1, hs, dhs, d_h, d_dh);
    return hipGetLastError() == hipSuccess ? UCF_OK : fail(UCF_ERR_HIP, "sort helper kernels failed");
}

int grid_device_locked(ucf_plan* pl, ucf_workspace* ws, int nt, const double* d_tD, const int* d_sv, int nr, const double* d_rD,
                       int nz, const double* zD, const int* zLay, double* d_h, double* d_dh, ucf_stats* d_stats, void* stream)
{
    {
        // Short time vectors (or several split indices): neither lane = time nor lane = Laplace sample fills the waves.
        // With enough points the grid is expanded into the point list it stands for and runs lane = point, in order of
        // radius like every long list (the outputs of a grid are in point order already: point = it * nr + ir).
        const bool lane_time = grid_lane_time(pl, nt);
        ucf_dev_params one = pl->dev;
        one.nz = 1;
        const long long np_grid = (long long)nt * nr;
        if (!lane_time && batch_layout() == 3 && np_grid >= 4 * UCF_WAVE && pl->D.np <= UCF_WAVE && state_item_bytes(pl, one) != 0 &&
            !pl->force_layout0) {
            int rc = ws_ensure(pl, ws, ws->expand, (size_t)np_grid * (2 * sizeof(double) + sizeof(int)), "expanded grid");
            if (rc) return rc;
            double* e_tD = (double*)ws->expand.p;
            double* e_rD = e_tD + np_grid;
            int* e_sv = (int*)(e_rD + np_grid);
            if (!ws->dry) {
                rc = ucf_faithful::launch_expand_grid(nt, nr, d_tD, d_sv, d_rD, e_tD, e_rD, e_sv, stream);
                if (rc) return fail(rc, "grid expansion kernel launch failed");
            }
            return batch_device_impl(pl, ws, (int)np_grid, e_tD, e_rD, e_sv, nz, zD, zLay, d_h, d_dh, d_stats, stream, false);
        }
    }
    // depths in chunks that fit the wave's LDS budget; each chunk is its own launch sequence on the stream
    const int zc = z_chunk(pl);
    ws->tm_valid = 0;
    for (int z0 = 0; z0 < nz; z0 += zc) {
        const int n = (nz - z0 < zc) ? nz - z0 : zc;
        int rc = grid_device_chunk(pl, ws, nt, d_tD, d_sv, nr, d_rD, n, zD + z0, zLay + z0, nz, z0, d_h, d_dh, d_stats, stream,
                                   pl->timing && nz <= zc);
        if (rc) return rc;
    }
    return UCF_OK;
}

int check_grid_args(const ucf_plan* pl, int nt, const void* d_tD, const void* d_sv, int nr, const void* d_rD, int nz, const double* zD,
                    const int* zLay, const void* d_h, const void* d_dh)
{
    if (!pl) return fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    if (nt < 0 || nr < 0) return fail(UCF_ERR_BAD_ARGUMENT, "negative grid size");
    if (nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nz < 1");
    if ((long long)nt * nr > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "grid larger than 2^31-1 points: split it");
    if (!zD || !zLay) return fail(UCF_ERR_BAD_ARGUMENT, "zD / zLay must not be NULL");
    if (nt > 0 && nr > 0 && (!d_tD || !d_rD || !d_sv || !d_h || !d_dh)) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    return UCF_OK;
}

int check_batch_args(const ucf_plan* pl, int npts, const void* tD, const void* rD, const void* sv, int nz, const double* zD,
                     const int* zLay, const void* h, const void* dh)
{
    if (!pl) return fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    if (npts < 0) return fail(UCF_ERR_BAD_ARGUMENT, "npts < 0");
    if (nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "nz < 1");
    if (!zD || !zLay) return fail(UCF_ERR_BAD_ARGUMENT, "zD / zLay must not be NULL");
    if (npts > 0 && (!tD || !rD || !sv || !h || !dh)) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    return UCF_OK;
}

int check_sv(const ucf_plan* pl, int n, const int* sv) { return check_sv_of(pl->P, pl->D, n, sv); }
int check_grid_sv_of(const ucf_params& P, const ucf_derived& D, int nt, const int* sv)
{
    int rc = check_sv_of(P, D, nt, sv);
    if (rc) return rc;
    const int* j0s = P.j0s;
    const int svmin = j0s[0] < j0s[1] ? j0s[0] : j0s[1], svmax = j0s[0] > j0s[1] ? j0s[0] : j0s[1];
    for (int i = 0; i < nt; i++)
        if (sv[i] < svmin || sv[i] > svmax) return fail(UCF_ERR_BAD_ARGUMENT, "sv[%d]=%d outside the plan's split range %d..%d", i, sv[i], svmin, svmax);
    return UCF_OK;
}
int check_grid_sv(const ucf_plan* pl, int nt, const int* sv) { return check_grid_sv_of(pl->P, pl->D, nt, sv); }
int check_depths(int nz, const int* zLay)
{
    for (int i = 0; i < nz; i++)
        if (zLay[i] < 1 || zLay[i] > 3) return fail(UCF_ERR_BAD_ARGUMENT, "zLay[%d]=%d not in 1..3", i, zLay[i]);
    return UCF_OK;
}

}  // namespace ucf_host

extern "C" {

int ucf_drawdown_grid_device(ucf_plan* pl, int nt, const double* d_tD, const int* d_sv, int nr, const double* d_rD,
                             int nz, const double* zD, const int* zLay, double* d_h, double* d_dh,
                             ucf_stats* d_stats, void* stream)
{
    int rc = check_grid_args(pl, nt, d_tD, d_sv, nr, d_rD, nz, zD, zLay, d_h, d_dh);
    if (rc) return rc;
    if (nt == 0 || nr == 0) return UCF_OK;
    device_switch dg(pl->device);
    ucf_workspace* ws = ws_for(pl, stream);
    if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
    std::lock_guard<std::mutex> g(ws->mu);
    return grid_device_locked(pl, ws, nt, d_tD, d_sv, nr, d_rD, nz, zD, zLay, d_h, d_dh, d_stats, stream);
}

int ucf_drawdown_batch_device(ucf_plan* pl, int npts, const double* d_tD, const double* d_rD, const int* d_sv,
                              int nz, const double* zD, const int* zLay, double* d_h, double* d_dh,
                              ucf_stats* d_stats, void* stream)
{
    int rc = check_batch_args(pl, npts, d_tD, d_rD, d_sv, nz, zD, zLay, d_h, d_dh);
    if (rc) return rc;
    if (npts == 0) return UCF_OK;
    device_switch dg(pl->device);
    ucf_workspace* ws = ws_for(pl, stream);
    if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
    std::lock_guard<std::mutex> g(ws->mu);
    return batch_device_impl(pl, ws, npts, d_tD, d_rD, d_sv, nz, zD, zLay, d_h, d_dh, d_stats, stream, false);
}

// Size the workspaces of `stream` for the calls to come, so that they allocate nothing (and can be captured into a
// hipGraph): a grid of nt x nr points and / or a point list of npts points, nz depths each.
int ucf_plan_reserve(ucf_plan* pl, int nt, int nr, int npts, int nz, void* stream)
{
    if (!pl) return fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    if (nt < 0 || nr < 0 || npts < 0 || nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad sizes");
    if ((long long)nt * nr > 0x7fffffffLL) return fail(UCF_ERR_BAD_ARGUMENT, "grid larger than 2^31-1 points: split it");
    device_switch dg(pl->device);
    ucf_workspace* ws = ws_for(pl, stream);
    if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
    std::lock_guard<std::mutex> g(ws->mu);
    // sizes do not depend on where the depths lie: any depth beside the screen stands for all of them
    std::vector<double> zD(nz, 0.5);
    std::vector<int> zl(nz, 2);
    ws->dry = true;
    int rc = UCF_OK;
    if (nt > 0 && nr > 0)
        rc = grid_device_locked(pl, ws, nt, nullptr, nullptr, nr, nullptr, nz, zD.data(), zl.data(), nullptr, nullptr, nullptr, stream);
    if (rc == UCF_OK && npts > 0)
        rc = batch_device_impl(pl, ws, npts, nullptr, nullptr, nullptr, nz, zD.data(), zl.data(), nullptr, nullptr, nullptr, stream, false);
    ws->dry = false;
    if (!ws->retired.empty() && hipStreamQuery((hipStream_t)stream) == hipSuccess) ws_release_retired(ws);
    return rc;
}

int ucf_drawdown_batch(ucf_plan* pl, int npts, const double* tD, const double* rD, const int* sv,
                       int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats)
{
    int rc = check_batch_args(pl, npts, tD, rD, sv, nz, zD, zLay, h, dh);
    if (rc) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (npts == 0) return UCF_OK;
    rc = check_sv(pl, npts, sv);
    if (rc) return rc;
    rc = check_depths(nz, zLay);
    if (rc) return rc;
    device_switch dg(pl->device);
    dev_buf b_t, b_r, b_s, b_h, b_d, b_st;
    const size_t nb = sizeof(double) * (size_t)npts;
    if (b_t.alloc(nb) || b_r.alloc(nb) || b_s.alloc(sizeof(int) * (size_t)npts) || b_h.alloc(nb * nz) ||
        b_d.alloc(nb * nz) || b_st.alloc(sizeof(ucf_stats)))
        return fail(UCF_ERR_NOMEM, "device allocation failed for %d points", npts);
    // A long list runs with lane = point: the 64 points of a wave should be neighbours in radius, because the wave
    // leaves the fast evaluators at the first lane that must (small radii reach the overflow regime early).  The list
    // is evaluated in order of radius and the results are put back in the caller's order.
    std::vector<double> tS, rS, hS, dS;
    std::vector<int> sS;
    const bool sorted = npts >= 4 * UCF_WAVE && batch_layout() == 3;
    const radius_order ord(sorted ? npts : 0, rD);
    if (sorted) {
        tS = ord.gather(tD); rS = ord.gather(rD); sS = ord.gather(sv);
        tD = tS.data(); rD = rS.data(); sv = sS.data();
    }
    HIP_TRY(hipMemcpy(b_t.p, tD, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_r.p, rD, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_s.p, sv, sizeof(int) * (size_t)npts, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(b_st.p, 0, sizeof(ucf_stats)));
    {
        ucf_workspace* ws = ws_for(pl, nullptr);
        if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
        std::lock_guard<std::mutex> g(ws->mu);
        rc = batch_device_impl(pl, ws, npts, (const double*)b_t.p, (const double*)b_r.p, (const int*)b_s.p, nz, zD,
                               zLay, (double*)b_h.p, (double*)b_d.p, stats ? (ucf_stats*)b_st.p : nullptr, nullptr, true);
    }
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (sorted) {
        hS.resize((size_t)npts * nz); dS.resize((size_t)npts * nz);
        HIP_TRY(hipMemcpy(hS.data(), b_h.p, nb * nz, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dS.data(), b_d.p, nb * nz, hipMemcpyDeviceToHost));
        ord.scatter(1, nz, hS.data(), dS.data(), h, dh);
    } else {
        HIP_TRY(hipMemcpy(h, b_h.p, nb * nz, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dh, b_d.p, nb * nz, hipMemcpyDeviceToHost));
    }
    if (stats) HIP_TRY(hipMemcpy(stats, b_st.p, sizeof(ucf_stats), hipMemcpyDeviceToHost));
    return UCF_OK;
}

int ucf_drawdown_grid(ucf_plan* pl, int nt, const double* tD, const int* sv, int nr, const double* rD,
                      int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats)
{
    ucf_plan* one[1] = {pl};
    return ucf_drawdown_grid_multi(one, 1, nt, tD, sv, nr, rD, nz, zD, zLay, h, dh, stats);
}

}  // extern "C"
