// ucf_multi.cpp -- more than one device or more than one parameter set: row shards and their gather (RCCL, bound at run
// time), the host-array entries over several devices, and the parameter batch (shared_launch, multi_core) that
// ucf_drawdown_multi and the fit (ucf_fit.cpp) evaluate through.
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include <dlfcn.h>

#include "ucf_host.h"

using namespace ucf_host;

namespace {

// RCCL, bound at run time (the library links nothing of it: a host without RCCL loads libucf.so all the same and gets
// UCF_ERR_UNSUPPORTED from the entries that need it)
struct rccl_unique_id { char internal[128]; };                     // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
struct rccl_api {
    void* lib = nullptr;
    int (*get_unique_id)(rccl_unique_id*) = nullptr;
    int (*comm_init_rank)(void**, int, rccl_unique_id, int) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*error_string)(int) = nullptr;
    std::string why;
};
const rccl_api& rccl()
{
    static const rccl_api api = [] {
        rccl_api a;
        // the copy of RCCL the process already has (a host framework's own) before a fresh one
        const char* names[] = {"librccl.so", "librccl.so.1"};
        for (const char* n : names) if (!a.lib) a.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        for (const char* n : names) if (!a.lib) a.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!a.lib) { const char* e = dlerror(); a.why = std::string("RCCL is not loadable: ") + (e ? e : "?"); return a; }
        a.get_unique_id = (int (*)(rccl_unique_id*))dlsym(a.lib, "ncclGetUniqueId");
        a.comm_init_rank = (int (*)(void**, int, rccl_unique_id, int))dlsym(a.lib, "ncclCommInitRank");
        a.comm_destroy = (int (*)(void*))dlsym(a.lib, "ncclCommDestroy");
        a.all_gather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(a.lib, "ncclAllGather");
        a.error_string = (const char* (*)(int))dlsym(a.lib, "ncclGetErrorString");
        if (!a.get_unique_id || !a.comm_init_rank || !a.comm_destroy || !a.all_gather) { a.why = "RCCL lacks an entry point"; a.lib = nullptr; }
        return a;
    }();
    return api;
}
int rccl_fail(const char* what, int code)
{
    const rccl_api& R = rccl();
    return fail(UCF_ERR_HIP, "%s: RCCL error %d (%s)", what, code, R.error_string ? R.error_string(code) : "?");
}
const int RCCL_FLOAT64 = 8;        // ncclFloat64 (rccl.h)

// the plans of ONE device
int drawdown_multi_device(ucf_plan* const* plans, int nplans, int npts, const double* t, const double* r,
                          int nz, const double* z, int dimensionless, double* h, double* dh)
{
    device_switch dg(plans[0]->device);
    const size_t np_ = (size_t)npts, tot = (size_t)nplans * np_;
    // the observation points are evaluated in order of radius (see ucf_drawdown_batch) and put back at the end
    const radius_order ord(npts, r);
    const std::vector<double> t_s = ord.gather(t), r_s = ord.gather(r);
    double* const h_user = h;
    double* const dh_user = dh;
    std::vector<double> h_tmp(tot * nz), dh_tmp(tot * nz);
    h = h_tmp.data(); dh = dh_tmp.data();
    struct unsort_at_exit {
        const radius_order& ord; int nplans, nz; const double* hs; const double* ds; double* h; double* dh;
        ~unsort_at_exit() { ord.scatter(nplans, nz, hs, ds, h, dh); }
    } unsort{ord, nplans, nz, h_tmp.data(), dh_tmp.data(), h_user, dh_user};
    dev_buf b_t, b_r, b_s, b_h, b_d;
    if (b_t.alloc(sizeof(double) * tot) || b_r.alloc(sizeof(double) * tot) || b_s.alloc(sizeof(int) * tot) ||
        b_h.alloc(sizeof(double) * tot * nz) || b_d.alloc(sizeof(double) * tot * nz))
        return fail(UCF_ERR_NOMEM, "device allocation failed for %d plans x %d points", nplans, npts);
    multi_io io;
    io.d_t = (double*)b_t.p; io.d_r = (double*)b_r.p; io.d_s = (int*)b_s.p; io.d_h = (double*)b_h.p; io.d_d = (double*)b_d.p;
    int rc = multi_core(plans, nplans, npts, t_s.data(), r_s.data(), nz, z, io);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(h, b_h.p, sizeof(double) * tot * nz, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dh, b_d.p, sizeof(double) * tot * nz, hipMemcpyDeviceToHost));
    if (!dimensionless)
        for (int k = 0; k < nplans; k++) {
            const double Hc = plans[k]->D.Hc;
            for (size_t i = 0; i < np_ * nz; i++) { h[k * np_ * nz + i] *= Hc; dh[k * np_ * nz + i] *= Hc; }
        }
    return UCF_OK;
}

}  // namespace

namespace ucf_host {

// Plans that differ only in what the evaluators read (hydraulic / geometric parameters) can share one launch sequence:
// anything that shapes the work must agree.
bool plans_share_launch(ucf_plan* const* plans, int nplans)
{
    bool one_launch = true;
    for (int k = 0; k < nplans && one_launch; k++) {
        const ucf_plan* a = plans[0];
        const ucf_plan* b = plans[k];
        const ucf_dev_params &x = a->dev, &y = b->dev;
        one_launch = a->mode == 1 && b->mode == 1 && a->device == b->device && a->force_layout0 == b->force_layout0 &&
                     (x.model == 1 || x.model == 3 || x.model == 4 || x.model == 5 || (x.model == 6 && x.MNtype == 2)) &&   // integrate_kernel models
                     x.model == y.model && x.MNtype == y.MNtype && x.order == y.order && x.MoenchM == y.MoenchM &&
                     x.M == y.M && x.k == y.k && x.R == y.R && x.nacc == y.nacc && x.ngl == y.ngl && x.N == y.N &&
                     x.nj0z == y.nj0z && x.alpha == y.alpha && x.logtol == y.logtol &&
                     a->P.j0s[0] == b->P.j0s[0] && a->P.j0s[1] == b->P.j0s[1] && (x.timeType >= 0) == (y.timeType >= 0) &&
                     (x.timeType >= 0 || x.timeType == y.timeType);
    }
    return one_launch;
}

// One launch sequence over nblk blocks of ppp points each, block b with its own parameter block in device memory
// (the evaluators read block (point / ppp) of the table): a block is a plan (ucf_drawdown_multi) or a (plan, well) tile of
// a network fit.  fill(z0, nzc, dps) writes the nblk parameter blocks of depths [z0, z0 + nzc); block 0's drives the launch.
// d_t, d_r, d_s: [nblk][ppp], d_h, d_d: [nblk][ppp][nz].  The null stream has drained when this returns.
int shared_launch(ucf_plan* pl, int nblk, int ppp, int nz, const fill_blocks& fill, std::vector<ucf_dev_params>& dps, const double* d_t,
                  const double* d_r, const int* d_s, double* d_h, double* d_d)
{
    const size_t np_ = (size_t)ppp, tot = (size_t)nblk * np_;
    ucf_workspace* ws = ws_for(pl, nullptr);
    if (!ws) return fail(UCF_ERR_NOMEM, "host allocation failed");
    std::lock_guard<std::mutex> g(ws->mu);
    dps.resize(nblk);
    // one abscissa row per (block, point), in chunks that keep the table <= 256 MiB
    const size_t row_bytes = (size_t)pl->D.nabs * 2 * sizeof(double);
    size_t chunk_plans = (table_budget() / row_bytes) / np_;      // whole blocks per table chunk
    if (chunk_plans < 1) chunk_plans = 1;
    size_t chunk = chunk_plans * np_;
    if (chunk > tot) chunk = tot;
    int rc = ws_ensure(pl, ws, ws->work, chunk * row_bytes, "abscissa table");
    if (rc) return rc;
    rc = ws_ensure(pl, ws, ws->pblocks, sizeof(ucf_dev_params) * nblk, "parameter blocks");
    if (rc) return rc;
    // depths in the same chunks as every other entry point (LDS budget of the integrate kernels)
    const int zc = z_chunk(pl);
    for (int z0 = 0; z0 < nz && rc == UCF_OK; z0 += zc) {
        const int nzc = (nz - z0 < zc) ? nz - z0 : zc;
        rc = fill(z0, nzc, dps);
        if (rc) return rc;
        for (int k = 1; k < nblk; k++) { dps[0].any_lay3 |= dps[k].any_lay3; dps[0].any_lay1 |= dps[k].any_lay1; dps[0].any_fold |= dps[k].any_fold; }      // block 0's parameters drive the launch
        HIP_TRY(hipStreamSynchronize(nullptr));                       // the previous chunk still reads the parameter blocks
        HIP_TRY(hipMemcpy(ws->pblocks.p, dps.data(), sizeof(ucf_dev_params) * nblk, hipMemcpyHostToDevice));
        ucf_launch L;
        L.dp = &dps[0]; L.per_point = 1; L.nr = 1;
        L.params = (const ucf_dev_params*)ws->pblocks.p; L.ppp = ppp;
        for (size_t base = 0; base < tot && rc == UCF_OK; base += chunk) {
            // points [base, base + npts) of the flattened (block, point) index; block of point q = q / ppp
            L.npts = (int)((tot - base < chunk) ? tot - base : chunk);
            L.pbase = (int)base;
            L.tD = d_t + base; L.rD = d_r + base; L.sv = d_s + base;
            L.h = d_h + base * nz; L.dh = d_d + base * nz;
            rc = ucf_faithful::launch_abscissae(dps[0], L.npts, 1, 1, 0, L.rD, L.sv, (double*)ws->work.p, nullptr);
            if (rc) return fail(rc, "abscissa kernel launch failed");
            rc = launch_points_any(pl, ws, L, (int)tot);
            if (rc) return rc;
            if (base + chunk < tot) HIP_TRY(hipStreamSynchronize(nullptr));      // the next chunk rewrites the table
        }
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    return UCF_OK;
}

// a small pool of streams that lives as long as the process (the plans key their workspaces by stream): up to `want`
// (at most 8) streams of `device`; returns how many
int stream_pool(int device, int want, hipStream_t* streams)
{
    const int NS = 8;
    static std::mutex pool_mu;
    static std::vector<std::pair<int, hipStream_t>> pool;       // (device, stream)
    int ns = 0;
    std::lock_guard<std::mutex> g(pool_mu);
    for (auto& e : pool)
        if (e.first == device && ns < NS) streams[ns++] = e.second;
    for (; ns < NS && ns < want; ns++) {
        if (hipStreamCreateWithFlags(&streams[ns], hipStreamNonBlocking) != hipSuccess) break;
        pool.emplace_back(device, streams[ns]);
    }
    return ns;
}

// The plans of ONE device over points ALREADY ordered by radius (t, r: dimensional, host): per-plan tD, rD, sv are staged
// and uploaded, the launches run, and the dimensionless h, dh [nplans][npts][nz] stay in io.d_h, io.d_d; every stream the
// call used has drained when it returns.  ucf_drawdown_multi and ucf_fit_evaluate are its callers.
int multi_core(ucf_plan* const* plans, int nplans, int npts, const double* t, const double* r, int nz, const double* z, multi_io& io)
{
    const size_t np_ = (size_t)npts, tot = (size_t)nplans * np_;
    // host staging: per plan tD, rD, sv
    std::vector<double>&tD = io.tD, &rD = io.rD, &zD = io.zD;
    std::vector<int>&sv = io.sv, &zl = io.zl;
    tD.resize(tot); rD.resize(tot); zD.resize((size_t)nplans * nz);
    sv.resize(tot); zl.resize((size_t)nplans * nz);
    for (int k = 0; k < nplans; k++) {
        const ucf_derived& D = plans[k]->D;
        for (int i = 0; i < npts; i++) { tD[k * np_ + i] = t[i] / D.Tc; rD[k * np_ + i] = r[i] / D.Lc; }
        for (int j = 0; j < nz; j++) zD[(size_t)k * nz + j] = z[j] / D.Lc;
        int rc = ucf_zlay(plans[k], nz, &zD[(size_t)k * nz], &zl[(size_t)k * nz]);
        if (rc) return rc;
        rc = ucf_split_vector(plans[k], npts, &tD[k * np_], &sv[k * np_]);
        if (rc) return rc;
        rc = check_sv(plans[k], npts, &sv[k * np_]);
        if (rc) return rc;
    }
    // work item = (plan, point), parameter block per plan in device memory; plans that cannot share a launch sequence
    // get their own launches on a pool of streams
    const bool one_launch = (nplans > 1) && (tot <= 0x7fffffffULL) && plans_share_launch(plans, nplans);
    HIP_TRY(hipMemcpy(io.d_t, tD.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(io.d_r, rD.data(), sizeof(double) * tot, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(io.d_s, sv.data(), sizeof(int) * tot, hipMemcpyHostToDevice));
    if (one_launch) {
        auto fill = [&](int z0, int nzc, std::vector<ucf_dev_params>& dps) {
            for (int k = 0; k < nplans; k++) {
                int rc = fill_call_params(plans[k], nzc, &zD[(size_t)k * nz + z0], &zl[(size_t)k * nz + z0], dps[k], nz, z0);
                if (rc) return rc;
            }
            return (int)UCF_OK;
        };
        return shared_launch(plans[0], nplans, npts, nz, fill, io.dps, io.d_t, io.d_r, io.d_s, io.d_h, io.d_d);
    }
    hipStream_t streams[8];
    const int ns = stream_pool(plans[0]->device, nplans, streams);
    if (ns == 0) return fail(UCF_ERR_HIP, "cannot create a HIP stream");
    int rc = UCF_OK;
    for (int k = 0; k < nplans && rc == UCF_OK; k++) {
        rc = ucf_drawdown_batch_device(plans[k], npts, (const double*)io.d_t + k * np_, (const double*)io.d_r + k * np_,
                                       (const int*)io.d_s + k * np_, nz, &zD[(size_t)k * nz], &zl[(size_t)k * nz],
                                       io.d_h + k * np_ * nz, io.d_d + k * np_ * nz, nullptr, streams[k % ns]);
    }
    for (int i = 0; i < ns; i++) (void)hipStreamSynchronize(streams[i]);
    return rc;
}

}  // namespace ucf_host

extern "C" {

int ucf_drawdown_grid_shard_device(ucf_plan* pl, int rank, int world, int nt, const double* d_tD, const int* d_sv, int nr,
                                   const double* d_rD, int nz, const double* zD, const int* zLay, double* d_h, double* d_dh,
                                   ucf_stats* d_stats, void* stream)
{
    int lo = 0, hi = 0;
    int rc = ucf_shard_rows(nt, world, rank, &lo, &hi);
    if (rc) return rc;
    rc = check_grid_args(pl, nt, d_tD, d_sv, nr, d_rD, nz, zD, zLay, d_h, d_dh);
    if (rc) return rc;
    if (hi == lo || nr == 0) return UCF_OK;
    const size_t off = (size_t)lo * nr * nz;
    return ucf_drawdown_grid_device(pl, hi - lo, d_tD + lo, d_sv + lo, nr, d_rD, nz, zD, zLay, d_h + off, d_dh + off, d_stats, stream);
}

// ---- one process per GPU, the gather inside the library
int ucf_comm_unique_id(unsigned char* id128)
{
    if (!id128) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    const rccl_api& R = rccl();
    if (!R.lib) return fail(UCF_ERR_UNSUPPORTED, "%s", R.why.c_str());
    rccl_unique_id id;
    const int rc = R.get_unique_id(&id);
    if (rc) return rccl_fail("ncclGetUniqueId", rc);
    std::memcpy(id128, id.internal, sizeof(id.internal));
    return UCF_OK;
}

int ucf_comm_create(const unsigned char* id128, int world, int rank, void** comm)
{
    if (!id128 || !comm || world < 1 || rank < 0 || rank >= world) return fail(UCF_ERR_BAD_ARGUMENT, "bad communicator request (world=%d rank=%d)", world, rank);
    *comm = nullptr;
    int rcd = require_device();
    if (rcd) return rcd;
    const rccl_api& R = rccl();
    if (!R.lib) return fail(UCF_ERR_UNSUPPORTED, "%s", R.why.c_str());
    rccl_unique_id id;
    std::memcpy(id.internal, id128, sizeof(id.internal));
    const int rc = R.comm_init_rank(comm, world, id, rank);        // on the HIP device that is current
    if (rc) return rccl_fail("ncclCommInitRank", rc);
    return UCF_OK;
}

int ucf_comm_destroy(void* comm)
{
    if (!comm) return UCF_OK;
    const rccl_api& R = rccl();
    if (!R.lib) return fail(UCF_ERR_UNSUPPORTED, "%s", R.why.c_str());
    const int rc = R.comm_destroy(comm);
    return rc ? rccl_fail("ncclCommDestroy", rc) : UCF_OK;
}

int ucf_drawdown_grid_allgather(ucf_plan* pl, int rank, int world, int nt, const double* d_tD, const int* d_sv, int nr,
                                const double* d_rD, int nz, const double* zD, const int* zLay, double* d_h, double* d_dh,
                                ucf_stats* d_stats, void* comm, void* stream)
{
    if (!comm) return fail(UCF_ERR_BAD_ARGUMENT, "NULL communicator");
    const rccl_api& R = rccl();
    if (!R.lib) return fail(UCF_ERR_UNSUPPORTED, "%s", R.why.c_str());
    int rc = ucf_drawdown_grid_shard_device(pl, rank, world, nt, d_tD, d_sv, nr, d_rD, nz, zD, zLay, d_h, d_dh, d_stats, stream);
    if (rc) return rc;
    if (nt == 0 || nr == 0) return UCF_OK;
    // shard g = rows [g B, (g+1) B) of [world B][nr][nz]: in place, sendbuff = recvbuff + rank * count
    const size_t cnt = (size_t)(((long long)nt + world - 1) / world) * nr * nz;
    device_switch dg(pl->device);
    for (double* a : {d_h, d_dh}) {
        const int nrc = R.all_gather(a + (size_t)rank * cnt, a, cnt, RCCL_FLOAT64, comm, (hipStream_t)stream);
        if (nrc) return rccl_fail("ncclAllGather", nrc);
    }
    return UCF_OK;
}

int ucf_drawdown_grid_multi(ucf_plan* const* plans, int ngpu, int nt, const double* tD, const int* sv, int nr, const double* rD,
                            int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats)
{
    if (!plans || ngpu < 1) return fail(UCF_ERR_BAD_ARGUMENT, "no plans");
    for (int g = 0; g < ngpu; g++) if (!plans[g]) return fail(UCF_ERR_BAD_ARGUMENT, "plans[%d] is NULL", g);
    int rc = check_grid_args(plans[0], nt, tD, sv, nr, rD, nz, zD, zLay, h, dh);
    if (rc) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (nt == 0 || nr == 0) return UCF_OK;
    rc = check_grid_sv(plans[0], nt, sv);
    if (rc) return rc;
    rc = check_depths(nz, zLay);
    if (rc) return rc;
    struct shard {
        int lo = 0, hi = 0, dev = 0;
        hipStream_t s = nullptr;
        dev_buf t, r, sv, h, d, st;
    };
    std::vector<shard> sh(ngpu);
    int prev = 0;
    (void)hipGetDevice(&prev);
    struct restore { int d; ~restore() { (void)hipSetDevice(d); } } back{prev};
    // enqueue every shard on its device (asynchronous), then collect: the devices work concurrently
    for (int g = 0; g < ngpu && rc == UCF_OK; g++) {
        shard& S = sh[g];
        (void)ucf_shard_rows(nt, ngpu, g, &S.lo, &S.hi);
        S.dev = plans[g]->device;
        const int n = S.hi - S.lo;
        if (n == 0) continue;
        if (hipSetDevice(S.dev) != hipSuccess) { rc = fail(UCF_ERR_HIP, "hipSetDevice(%d) failed", S.dev); break; }
        const size_t no = sizeof(double) * (size_t)n * nr * nz;
        if (S.t.alloc(sizeof(double) * n) || S.r.alloc(sizeof(double) * nr) || S.sv.alloc(sizeof(int) * n) || S.h.alloc(no) || S.d.alloc(no) ||
            S.st.alloc(sizeof(ucf_stats))) { rc = fail(UCF_ERR_NOMEM, "device allocation failed for rows %d..%d x %d radii on device %d", S.lo, S.hi, nr, S.dev); break; }
        // the plan's own stream: its workspace in the plan is keyed by it and lives as long (a stream per call would leave a
        // workspace per call behind, keyed by a dead handle)
        S.s = plan_stream(plans[g]);
        if (!S.s) { rc = fail(UCF_ERR_HIP, "cannot create a HIP stream on device %d", S.dev); break; }
        if (hipMemcpyAsync(S.t.p, tD + S.lo, sizeof(double) * n, hipMemcpyHostToDevice, S.s) != hipSuccess ||
            hipMemcpyAsync(S.r.p, rD, sizeof(double) * nr, hipMemcpyHostToDevice, S.s) != hipSuccess ||
            hipMemcpyAsync(S.sv.p, sv + S.lo, sizeof(int) * n, hipMemcpyHostToDevice, S.s) != hipSuccess ||
            hipMemsetAsync(S.st.p, 0, sizeof(ucf_stats), S.s) != hipSuccess) { rc = fail(UCF_ERR_HIP, "upload to device %d failed", S.dev); break; }
        rc = ucf_drawdown_grid_device(plans[g], n, (const double*)S.t.p, (const int*)S.sv.p, nr, (const double*)S.r.p, nz, zD, zLay,
                                      (double*)S.h.p, (double*)S.d.p, stats ? (ucf_stats*)S.st.p : nullptr, S.s);
    }
    // the gather: every device's block goes straight to its place in the caller's arrays (rows lo..hi of [nt][nr][nz])
    for (int g = 0; g < ngpu; g++) {
        shard& S = sh[g];
        if (!S.s) continue;
        (void)hipSetDevice(S.dev);
        const int n = S.hi - S.lo;
        const size_t no = sizeof(double) * (size_t)n * nr * nz, off = (size_t)S.lo * nr * nz;
        if (rc == UCF_OK) {
            ucf_stats st;
            if (hipMemcpyAsync(h + off, S.h.p, no, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
                hipMemcpyAsync(dh + off, S.d.p, no, hipMemcpyDeviceToHost, S.s) != hipSuccess ||
                hipMemcpyAsync(&st, S.st.p, sizeof(st), hipMemcpyDeviceToHost, S.s) != hipSuccess ||
                hipStreamSynchronize(S.s) != hipSuccess) {
                rc = fail(UCF_ERR_HIP, "device %d: %s", S.dev, hipGetErrorString(hipGetLastError()));
            } else if (stats) stats_add(*stats, st);
        } else {
            (void)hipStreamSynchronize(S.s);
        }
    }
    return rc;
}

int ucf_drawdown_batch_multi(ucf_plan* const* plans, int ngpu, int npts, const double* tD, const double* rD, const int* sv,
                             int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats)
{
    if (!plans || ngpu < 1) return fail(UCF_ERR_BAD_ARGUMENT, "no plans");
    for (int g = 0; g < ngpu; g++) if (!plans[g]) return fail(UCF_ERR_BAD_ARGUMENT, "plans[%d] is NULL", g);
    int rc = check_batch_args(plans[0], npts, tD, rD, sv, nz, zD, zLay, h, dh);
    if (rc) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (npts == 0) return UCF_OK;
    // block g of the list (ucf_shard_rows over the points) on plans[g]'s device, one host thread per device: each runs the
    // single-device entry (its own radius ordering, uploads, launches, copy of its slice into h and dh) on its own device
    std::vector<int> rcs(ngpu, UCF_OK);
    std::vector<std::string> msgs(ngpu);
    std::vector<ucf_stats> sts(ngpu);
    std::vector<std::thread> th;
    for (int g = 0; g < ngpu; g++) {
        int lo = 0, hi = 0;
        (void)ucf_shard_rows(npts, ngpu, g, &lo, &hi);
        std::memset(&sts[g], 0, sizeof(ucf_stats));
        if (hi <= lo) continue;
        th.emplace_back([&, g, lo, hi] {
            rcs[g] = ucf_drawdown_batch(plans[g], hi - lo, tD + lo, rD + lo, sv + lo, nz, zD, zLay, h + (size_t)lo * nz,
                                        dh + (size_t)lo * nz, stats ? &sts[g] : nullptr);
            if (rcs[g] != UCF_OK) msgs[g] = ucf_last_error();
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < ngpu; g++)
        if (rcs[g] != UCF_OK) return fail(rcs[g], "shard %d of %d (device %d): %s", g, ngpu, plans[g]->device, msgs[g].c_str());
    if (stats)
        for (int g = 0; g < ngpu; g++) stats_add(*stats, sts[g]);
    return UCF_OK;
}

int ucf_drawdown_multi(ucf_plan* const* plans, int nplans, int npts, const double* t, const double* r,
                       int nz, const double* z, int dimensionless, double* h, double* dh)
{
    if (!plans || nplans < 1) return fail(UCF_ERR_BAD_ARGUMENT, "no plans");
    if (npts < 0 || nz < 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad sizes");
    if (npts == 0) return UCF_OK;
    if (!t || !r || !z || !h || !dh) return fail(UCF_ERR_BAD_ARGUMENT, "NULL array");
    for (int k = 0; k < nplans; k++) if (!plans[k]) return fail(UCF_ERR_BAD_ARGUMENT, "plans[%d] is NULL", k);
    // Parameter sets are independent: the plans of one device form a group (a launch sequence of its own, as below),
    // the groups run at the same time, one host thread per device -- the second shard axis of the tool (SURVEY.md 8f-4;
    // which plan lives where is the caller's choice at ucf_plan_create_on, e.g. ucf_shard_rows(nplans, ngpu, g)).
    // UCF_MULTI_GROUPS=n (diagnostic): cut every device's group into n blocks, to exercise the merge on one GPU.
    std::vector<std::vector<int>> groups;
    {
        std::vector<int> devs;
        for (int k = 0; k < nplans; k++) {
            size_t g = 0;
            while (g < devs.size() && devs[g] != plans[k]->device) g++;
            if (g == devs.size()) { devs.push_back(plans[k]->device); groups.emplace_back(); }
            groups[g].push_back(k);
        }
        const int split = ucf_env_get().multi_groups;
        if (split > 1) {
            std::vector<std::vector<int>> cut;
            for (const auto& G : groups)
                for (int b = 0; b < split; b++) {
                    int lo = 0, hi = 0;
                    (void)ucf_shard_rows((int)G.size(), split, b, &lo, &hi);
                    if (hi > lo) cut.emplace_back(G.begin() + lo, G.begin() + hi);
                }
            groups.swap(cut);
        }
    }
    if (groups.size() == 1) return drawdown_multi_device(plans, nplans, npts, t, r, nz, z, dimensionless, h, dh);
    const size_t per_plan = (size_t)npts * nz;
    std::vector<int> rcs(groups.size(), UCF_OK);
    std::vector<std::string> msgs(groups.size());
    std::vector<std::thread> th;
    for (size_t g = 0; g < groups.size(); g++)
        th.emplace_back([&, g] {
            const std::vector<int>& G = groups[g];
            std::vector<ucf_plan*> sub(G.size());
            for (size_t i = 0; i < G.size(); i++) sub[i] = plans[G[i]];
            std::vector<double> hg(G.size() * per_plan), dg(G.size() * per_plan);
            rcs[g] = drawdown_multi_device(sub.data(), (int)G.size(), npts, t, r, nz, z, dimensionless, hg.data(), dg.data());
            if (rcs[g] != UCF_OK) { msgs[g] = ucf_last_error(); return; }
            for (size_t i = 0; i < G.size(); i++) {
                std::memcpy(h + (size_t)G[i] * per_plan, hg.data() + i * per_plan, sizeof(double) * per_plan);
                std::memcpy(dh + (size_t)G[i] * per_plan, dg.data() + i * per_plan, sizeof(double) * per_plan);
            }
        });
    for (auto& x : th) x.join();
    for (size_t g = 0; g < groups.size(); g++)
        if (rcs[g] != UCF_OK) return fail(rcs[g], "plan group %zu of %zu (device %d): %s", g, groups.size(), plans[groups[g][0]]->device, msgs[g].c_str());
    return UCF_OK;
}

}  // extern "C"
