// ucf_host.h -- what the host sources of the library share (ucf_api.cpp, ucf_plan.cpp, ucf_drawdown.cpp, ucf_multi.cpp,
// ucf_debug.cpp, ucf_fit.cpp, ucf_field.cpp, ucf_allocate.cpp).  Internal: everything is in namespace ucf_host with hidden visibility, so
// the names link between the objects and are not exported from libucf.so.  Declarations and a few small inline helpers; the
// comment that explains a declared function stands at its definition, in the file named here.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <vector>

#include "ucf_plan.h"

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(UCF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace ucf_host __attribute__((visibility("hidden"))) {

// ---- ucf_api.cpp
int fail(int code, const char* fmt, ...);      // sets what ucf_last_error() returns; returns code

// What differs between the two builds of the kernels (ucf_kernels_*.hip), indexed by ucf_plan::mode: 0 faithful, 1 fast.
struct ucf_flavour {
    decltype(&ucf_fast::launch_points) launch_points, launch_grid_transposed, launch_points_chunked, launch_points_lanes;
    decltype(&ucf_fast::launch_samples) launch_samples;
    decltype(&ucf_fast::launch_wynn_regs) launch_wynn_regs;
    decltype(&ucf_fast::launch_dehoog_tiles_hook) launch_dehoog_tiles_hook;
};
const ucf_flavour& flavour(int mode);
inline const ucf_flavour& flavour_of(const ucf_plan* pl) { return flavour(pl->mode); }

int launch_failed(int rc, const ucf_dev_params& dp);
void stats_add(ucf_stats& a, const ucf_stats& b);
int require_device();

// Host point lists are evaluated in order of radius (ucf_drawdown_batch says why): the order, and the way back
struct radius_order {
    std::vector<int> perm;       // perm[i]: the caller's index of the i-th point in order of radius
    radius_order(int npts, const double* r);
    template <class T>
    std::vector<T> gather(const T* v) const;      // (double and int)
    // hs, ds: [nblk][npts][nz] in order of radius -> h, dh in the caller's order
    void scatter(int nblk, int nz, const double* hs, const double* ds, double* h, double* dh) const;
};

// runs the rest of the scope with HIP device `dev` current (a process may drive several devices: ucf_drawdown_grid_multi)
struct device_switch {
    int prev = -1;
    bool switched = false;
    explicit device_switch(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = (hipSetDevice(dev) == hipSuccess);
    }
    ~device_switch() { if (switched) (void)hipSetDevice(prev); }
};

// device buffers.  guarded_malloc is the one allocator (UCF_GUARD); dev_buf lives for one call; a ucf_buffer that an
// owner (ucf_fit, ucf_field) keeps between calls grows through grow_buffer and goes through free_buffer; the workspaces
// of a plan have a policy of their own (ws_ensure)
hipError_t guarded_malloc(void** p, void** base, size_t bytes);
struct dev_buf {
    void* p = nullptr;
    void* base = nullptr;
    ~dev_buf() { if (base) (void)hipFree(base); }
    int alloc(size_t bytes) { return guarded_malloc(&p, &base, bytes) == hipSuccess ? 0 : 1; }
};
int grow_buffer(ucf_buffer& b, size_t bytes, const char* what, long long& n_alloc);
void free_buffer(ucf_buffer& b);

// synchronises the stream when the scope ends, however it ends: host staging that asynchronous copies read outlives them
struct drain {
    hipStream_t s;
    ~drain() { (void)hipStreamSynchronize(s); }
};
// Results on their way back: only what was asked for (host not NULL, bytes > 0) crosses the bus.  copy_back enqueues the
// copies on `st` and returns when the stream has drained; copy_back_sync is for callers on the null stream that have
// synchronised already.
struct device_copy {
    void* host;
    const void* dev;
    size_t bytes;
};
inline int copy_back(const std::vector<device_copy>& list, hipStream_t st, int device)
{
    for (const device_copy& c : list)
        if (c.host && c.bytes && hipMemcpyAsync(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
            return fail(UCF_ERR_HIP, "device %d: %s", device, hipGetErrorString(hipGetLastError()));
    if (hipStreamSynchronize(st) != hipSuccess) return fail(UCF_ERR_HIP, "device %d: %s", device, hipGetErrorString(hipGetLastError()));
    return UCF_OK;
}
inline int copy_back_sync(const std::vector<device_copy>& list)
{
    for (const device_copy& c : list)
        if (c.host && c.bytes) HIP_TRY(hipMemcpy(c.host, c.dev, c.bytes, hipMemcpyDeviceToHost));
    return UCF_OK;
}

// ---- ucf_plan.cpp
int validate(const ucf_params& P);
void nondimensionalise(const ucf_params& P, ucf_derived& D);
int z_chunk(const ucf_plan* plan);
int fill_call_params(const ucf_plan* plan, int nz, const double* zD, const int* zLay, ucf_dev_params& dp, int nz_out = 0, int z_off = 0);
void split_vector(const int* j0s, int nt, const double* tD, int* sv);

// ---- ucf_drawdown.cpp
ucf_workspace* ws_for(ucf_plan* pl, void* stream);
void ws_destroy(ucf_workspace* ws);
hipStream_t plan_stream(ucf_plan* pl);
int ws_ensure(ucf_plan* pl, ucf_workspace* ws, ucf_buffer& b, size_t bytes, const char* what);
// the buffers that the kernels of a launch sequence share (ucf_launch_plan.h), in the plan's flavour
inline ucf_transform_buffers buffers_of(const ucf_plan* pl, const ucf_dev_params& dp, size_t items, size_t lt_rows) { return transform_buffers(dp, pl->mode == 1, items, lt_rows); }
// state of a work item between the integrate kernel and finish / point_kernel (0: the abscissa loop has no kernel of its own)
inline size_t state_item_bytes(const ucf_plan* pl, const ucf_dev_params& dp) { return buffers_of(pl, dp, 0, 0).state_item_bytes; }
// abscissa-table bytes per chunk of an arbitrary point list (UCF_TABLE_BYTES, default 256 MiB)
inline size_t table_budget() { return ucf_env_get().table_bytes; }
int launch_points_any(ucf_plan* pl, ucf_workspace* ws, const ucf_launch& call, int npts_call);
int batch_device_impl(ucf_plan* pl, ucf_workspace* ws, int npts, const double* d_tD, const double* d_rD, const int* d_sv,
                      int nz, const double* zD, const int* zLay, double* d_h, double* d_dh, ucf_stats* d_stats, void* stream,
                      bool presorted);
int grid_device_locked(ucf_plan* pl, ucf_workspace* ws, int nt, const double* d_tD, const int* d_sv, int nr, const double* d_rD,
                       int nz, const double* zD, const int* zLay, double* d_h, double* d_dh, ucf_stats* d_stats, void* stream);
int check_grid_args(const ucf_plan* pl, int nt, const void* d_tD, const void* d_sv, int nr, const void* d_rD, int nz, const double* zD,
                    const int* zLay, const void* d_h, const void* d_dh);
int check_batch_args(const ucf_plan* pl, int npts, const void* tD, const void* rD, const void* sv, int nz, const double* zD,
                     const int* zLay, const void* h, const void* dh);
int check_sv(const ucf_plan* pl, int n, const int* sv);
int check_grid_sv_of(const ucf_params& P, const ucf_derived& D, int nt, const int* sv);
int check_grid_sv(const ucf_plan* pl, int nt, const int* sv);
int check_depths(int nz, const int* zLay);

// ---- ucf_multi.cpp
// What one pass of the shared core reads and writes: host staging (kept between calls by an owner that calls often) and
// device arrays that the CALLER owns -- d_t, d_r, d_s: nplans x npts, d_h, d_d: nplans x npts x nz.
struct multi_io {
    std::vector<double> tD, rD, zD;
    std::vector<int> sv, zl;
    std::vector<ucf_dev_params> dps;       // parameter blocks of a shared launch
    double* d_t = nullptr;
    double* d_r = nullptr;
    int* d_s = nullptr;
    double* d_h = nullptr;
    double* d_d = nullptr;
};
bool plans_share_launch(ucf_plan* const* plans, int nplans);
// fill(z0, nzc, dps) writes the parameter blocks of depths [z0, z0 + nzc): once per depth chunk
typedef std::function<int(int z0, int nzc, std::vector<ucf_dev_params>& dps)> fill_blocks;
int shared_launch(ucf_plan* pl, int nblk, int ppp, int nz, const fill_blocks& fill, std::vector<ucf_dev_params>& dps, const double* d_t,
                  const double* d_r, const int* d_s, double* d_h, double* d_d);
int stream_pool(int device, int want, hipStream_t* streams);
int multi_core(ucf_plan* const* plans, int nplans, int npts, const double* t, const double* r, int nz, const double* z, multi_io& io);

// ---- ucf_fit.cpp
const char* fit_par_name(int id, char* buf, size_t n);
// The parameter sets of one theta, in the order a fit evaluates them: sets[0] = ucf_fit_perturb(base, ids, theta), and for
// count = 1 + 2 npar also sets[1 + 2j] / sets[2 + 2j] = the same with theta[j] * exp(+dlog) / theta[j] * exp(-dlog), one
// product each (count = 1: the base set alone, dlog is not read).  Returns what ucf_fit_perturb returns.
int fit_theta_sets(const ucf_params& base, int npar, const int* ids, const double* theta, double dlog, int count, ucf_params* sets);
// the lower Cholesky factor of M [n][n] (symmetric, row-major) in its lower triangle, as ucf_fit_solve_step forms it;
// UCF_ERR_SINGULAR (no message) where a pivot is not positive and finite
int fit_cholesky_factor(int n, double* M);
// UCF_ERR_BAD_ARGUMENT naming the first row of mult [nrep][nobs] whose entries sum beyond 2^31 - 1 (the counts of a resampled
// reduction are int)
int fit_resample_check_rows(int nrep, int nobs, const unsigned short* mult);

// ---- ucf_field.cpp
// UCF_ERR_BAD_ARGUMENT naming name[i] for the first v[i] that is not finite
int field_check_finite(const char* name, int n, const double* v);
// what ucf_field_ensemble and ucf_debug_ensemble check on nens, the levels q [nq] and the limits [nlim]
// (ucf_field_yield calls its limits `level`, nlev of them, and has them named so)
int ensemble_check_levels(int nens, int nq, const double* q, int nlim, const double* limit, bool want_quant, bool want_pexc,
                          const char* nlim_name = "nlim", const char* limit_name = "limit");
// the image of the checked levels and limits that goes to the device: q at [0], limit at [UCF_ENSEMBLE_MAX_Q], the rest 0
inline void ensemble_pack_levels(int nq, const double* q, int nlim, const double* limit, double (&ql)[2 * UCF_ENSEMBLE_MAX_Q])
{
    for (double& v : ql) v = 0.0;
    for (int i = 0; i < nq; i++) ql[i] = q[i];
    for (int i = 0; i < nlim; i++) ql[UCF_ENSEMBLE_MAX_Q + i] = limit[i];
}

// ---- ucf_allocate.cpp
// what ucf_field_allocate, ucf_debug_field_allocate and ucf_allocate_solve check on nctl, the objectives, xmax and maxit
int allocate_check_programme(int nctl, int nobj, const double* w, const double* xmax, int maxit);
// what the two entries on caller slots check on nens, ncon, R and limit_con
int allocate_check_slots(int nctl, int nens, int ncon, const double* R, const double* limit_con);

}  // namespace ucf_host
