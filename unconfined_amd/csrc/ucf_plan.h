// ucf_plan.h -- internal structures shared by the host API and the kernels.
#pragma once
#include "../../include/ucf.h"
#include "ucf_env.h"
#include "ucf_launch_plan.h"     // ucf_dev_params and the sizes that host and kernels share
#include <cstdio>
#include <mutex>
#include <vector>

// HIP events around the kernels of the last lane = time grid call issued through a workspace (measurement only):
// bracket i = ev[2i] .. ev[2i+1] around the kernel called name[i].
#define UCF_MAX_TIMED 96          /* brackets per call: kernels of a launch sequence x chunks of radii */
struct ucf_timers {
    void* ev[2 * UCF_MAX_TIMED];     // hipEvent_t, created on first use
    char name[UCF_MAX_TIMED][96];
    int n;                           // brackets recorded by the last timed call
    int open;                        // a bracket is open
};
// begin a bracket (closing the one before it); no-ops on a NULL timer set
static inline void ucf_tm_close(ucf_timers* tm, void* stream)
{
    if (!tm || !tm->open) return;
    (void)hipEventRecord((hipEvent_t)tm->ev[2 * (tm->n - 1) + 1], (hipStream_t)stream);
    tm->open = 0;
}
static inline void ucf_tm_mark(ucf_timers* tm, const char* name, void* stream)
{
    // UCF_TRACE_LAUNCHES=1 (diagnostic): wait for everything launched so far and name the kernel that comes next on stderr,
    // so that the last line before a device fault names the kernel that faulted
    if (ucf_env_get().trace_launches) {
        const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        std::fprintf(stderr, "[ucf] stream %s; next: %s\n", e == hipSuccess ? "clean" : hipGetErrorString(e), name);
        std::fflush(stderr);
    }
    if (!tm) return;
    ucf_tm_close(tm, stream);
    if (tm->n >= UCF_MAX_TIMED) return;
    const int i = tm->n;
    for (int k = 2 * i; k < 2 * i + 2; k++)
        if (!tm->ev[k]) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; tm->ev[k] = e; }
    std::snprintf(tm->name[i], sizeof(tm->name[i]), "%s", name);
    (void)hipEventRecord((hipEvent_t)tm->ev[2 * i], (hipStream_t)stream);
    tm->n = i + 1;
    tm->open = 1;
}

// ucf_debug_stages: what the launcher did (one record per transform launch sequence of the call)
struct ucf_debug_rec {
    int count = 0;                 // launch sequences seen (the hook wants exactly one)
    int layout = -1, nwork = 0, per_point = 0, nr = 0, nt = 0, ir0 = 0, nrc = 0, npts = 0;
    double* d_totlap0 = nullptr;   // LAYOUT 0 keeps no transform: the hook lends it a buffer [npts][nz][np]
};

// Everything a call in flight writes.  A plan keeps one workspace per HIP stream that has called into it, so calls on
// different streams never share scratch; calls that name the same stream are enqueued under the workspace's lock and
// run in stream order.  Buffers only ever grow; a buffer that is outgrown is RETIRED (kept until ucf_plan_reserve /
// ucf_plan_destroy), never freed while kernels may still read it -- no synchronisation inside the *_device entries.  ws_buffers
// (ucf_drawdown.cpp) lists the buffers of a workspace: a new one goes there too.
struct ucf_buffer {
    void* p = nullptr;
    size_t bytes = 0;
    void* base = nullptr;          // what hipMalloc returned (== p unless UCF_GUARD places the buffer at the END of its pages)
};
struct ucf_workspace {
    void* stream = nullptr;
    std::mutex mu;                 // held while a call enqueues its work on `stream`
    ucf_buffer work;               // abscissa table: rows x nabs x (a, a*J0(a rD))
    ucf_buffer totlap;             // accelerated transform totlap(t, r, z, m) of the lane = time / lane = point layouts, 16 B each
    ucf_buffer glscr;              // finished J0-interval areas of the resident workgroups: [UCF_GRID_SLOTS][nacc][nz][64] complex
    ucf_buffer expand;             // a grid expanded into the point list it stands for: tD | rD | sv per point
    ucf_buffer sort;               // device-side ordering of a point list by radius: keys, permutation, staged inputs/outputs
    ucf_buffer state;              // integrate kernel -> finish/point kernel: [items][(R+1+nacc)*nz][64] complex
    ucf_buffer ndone;              // abscissae done per item | count of unfinished | unfinished items
    ucf_buffer pblocks;            // parameter blocks of a parameter-batched launch (ucf_drawdown_multi)
    std::vector<void*> retired;    // outgrown buffers
    bool dry = false;              // ucf_plan_reserve: size the buffers, launch nothing
    struct ucf_debug_rec* dbg = nullptr;   // ucf_debug_stages: the transform launches of the call in progress are recorded here
    ucf_timers tm = {};
    int tm_valid = 0;
    const char* tm_names[UCF_MAX_TIMED] = {};
};

struct ucf_plan {
    ucf_params P = {};
    ucf_derived D = {};
    ucf_dev_params dev = {};   // zD/zLay/nz filled per call
    int mode = 0;              // 0 faithful, 1 fast
    int force_layout0 = 0;     // diagnostic: never use the lane = time layout
    int timing = 0;            // bracket the kernels of single-chunk grid calls with events
    int device = 0;
    double* d_tables = nullptr;    // one allocation holding all tables
    size_t tables_bytes = 0;
    size_t o_tsx = 0, o_tsw = 0, o_glx = 0, o_glw = 0, o_j0z = 0, o_fde = 0, o_sched = 0, o_sct = 0;     // offsets (doubles) of the tables in it
    // host copies (for the accessor API)
    double* h_j0z = nullptr;
    double* h_ts_x = nullptr;
    double* h_ts_w = nullptr;      // [R][N]
    double* h_gl_x = nullptr;
    double* h_gl_w = nullptr;
    int Nv[UCF_MAX_R] = {};
    // per-stream workspaces (see ucf_workspace); `mu` guards the list and the counters
    std::mutex mu;
    std::vector<ucf_workspace*> ws;
    ucf_workspace* last_timed = nullptr;
    long long n_alloc = 0;         // device allocations made on behalf of calls (ucf_plan_alloc_count)
    // the stream of the host entry points that run asynchronously inside the library (ucf_drawdown_grid, ucf_drawdown_grid_multi):
    // created on first use, destroyed with the plan -- a workspace is keyed by its stream, so the stream must outlive it
    void* own_stream = nullptr;
};

// One launch sequence: everything the layout launchers and launch_transform_ (ucf_launchers.h) read and write.  A caller
// fills one and, inside its chunk loops, moves only the bases and counts.
struct ucf_launch {
    const ucf_dev_params* dp = nullptr;    // the parameter block (plan 0's in a parameter batch)
    // a point list has npts points (per_point = 1: tD, rD, sv per point; 0: point = it * nr + ir of a grid walked point by
    // point); the lane = time layout has nt times x radii [ir0, ir0 + nrc) of nr
    int npts = 0, per_point = 0, nt = 0, nr = 0, ir0 = 0, nrc = 0;
    int nsv = 1, svmin = 0;                // rows of the abscissa table: row = radius * nsv + (sv - svmin)
    const double *tD = nullptr, *rD = nullptr, *tab = nullptr;      // tab: the abscissa table
    const int* sv = nullptr;
    double *h = nullptr, *dh = nullptr;
    ucf_stats* stats = nullptr;
    // workspace.  totlap: the accelerated transform (lane layout 0 keeps none: NULL, or the buffer ucf_debug_stages lends)
    double *totlap = nullptr, *glscr = nullptr, *state = nullptr;
    int* ndone = nullptr;
    void* stream = nullptr;
    ucf_timers* tm = nullptr;              // (lane = time only) brackets the kernels with events
    // parameter batch (fast flavour, per-point layouts): point q of the launch reads params[(pbase + q) / ppp]
    const ucf_dev_params* params = nullptr;
    int ppp = 1, pbase = 0;
};

// launchers implemented in ucf_launchers.h and, the stage hooks, ucf_device.h; compiled by ucf_kernels_*.hip (one set per build flavour)
namespace ucf_faithful {
// abscissa tables (shared by both flavours): tab[row][nabs] of (a, a*J0(a*rD)); d_ends (optional): [row][nacc + 1] ends of the
// row's J0 intervals (abscissa_ends_offset, ucf_launch_plan.h)
int launch_abscissae(const ucf_dev_params& dp, int nrows, int per_point, int nsv, int svmin, const double* d_rD,
                     const int* d_sv, double* d_tab, void* stream, double* d_ends = nullptr);
int launch_expand_grid(int nt, int nr, const double* d_tD, const int* d_sv, const double* d_rD, double* d_tDp, double* d_rDp,
                       int* d_svp, void* stream);
int launch_bessel(int n, const double* d_z, double* d_k, int* d_ierr, void* stream);
int launch_dehoog(int n, int M, double alpha, double logtol, const double* d_t, const double* d_tee,
                  const double* d_fp, double* d_ft, void* stream);
int launch_wynn(int n, int nterms, const double* d_series, double* d_acc, int* d_status, void* stream);
int launch_extrap(int n, int R, const double* d_x, const double* d_y, double* d_out, void* stream);
int launch_debug_gather(const ucf_dev_params& dp, int layout, int nwork, int per_point, int nr, int nt, int ir0, const double* d_state,
                        const int* d_ndone, double* d_out_state, int* d_out_ndone, void* stream);
}
// what both flavours define, entry by entry the ucf_flavour table (ucf_host.h, filled in ucf_api.cpp)
namespace ucf_faithful {
int launch_points(const ucf_launch& L);             // lane layout 0
int launch_grid_transposed(const ucf_launch& L);    // 1
int launch_points_chunked(const ucf_launch& L);     // 2
int launch_points_lanes(const ucf_launch& L);       // 3
int launch_samples(const ucf_dev_params& dp, int n_a, const double* d_a, double rD, const double* d_p, double* d_fp, void* stream);
int launch_wynn_regs(int n, int nterms, const double* d_series, double* d_acc, int* d_status, void* stream);
int launch_dehoog_tiles_hook(const ucf_dev_params& dp, int n, const double* d_tD, const double* d_totlap, double* d_h, double* d_dh, void* stream);
}
namespace ucf_fast {
int launch_points(const ucf_launch& L);             // lane layout 0
int launch_grid_transposed(const ucf_launch& L);    // 1
int launch_points_chunked(const ucf_launch& L);     // 2
int launch_points_lanes(const ucf_launch& L);       // 3
int launch_samples(const ucf_dev_params& dp, int n_a, const double* d_a, double rD, const double* d_p, double* d_fp, void* stream);
int launch_wynn_regs(int n, int nterms, const double* d_series, double* d_acc, int* d_status, void* stream);
int launch_dehoog_tiles_hook(const ucf_dev_params& dp, int n, const double* d_tD, const double* d_totlap, double* d_h, double* d_dh, void* stream);
}
