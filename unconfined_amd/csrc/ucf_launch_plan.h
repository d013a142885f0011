// ucf_launch_plan.h -- what a transform launch sequence is going to do, decided in plain C++: the parameter block the
// kernels read, the one description of the buffers that the host sizes and the launchers index (transform_buffers), and
// plan_transform, which turns (parameter block, environment knobs, flavour, lane layout, work items) into the kernel
// instantiations, grids, LDS sizes and work-item cuts of the sequence.  No HIP, no globals: it compiles with a plain
// C++17 compiler (tests/test_launch_plan.py runs it on the CPU), and launch_transform_ (ucf_launchers.h) only maps the
// plan onto template arguments.  The measurements behind the choices stay beside the code that makes them.
#pragma once
#include "../../include/ucf.h"
#include "ucf_env.h"

#define UCF_WAVE 64
#define UCF_MAX_R 16
#define UCF_LDS_C 16           /* bytes of one complex in LDS (lds_c = double2, ucf_device.h) */

// Everything a kernel needs, passed by value as one kernel argument (lives in
// SGPRs / the scalar cache: it is wave-uniform).  Table pointers are device
// pointers into one small per-plan allocation that stays L2/scalar-cache hot.
struct ucf_dev_params {
    int model, MNtype, order, timeType, MoenchM;
    int M, np, k, N, R, nacc, ngl, nz;
    int tab_premul;        // the abscissa table's Gauss-Lobatto entries carry their quadrature weight (fast flavour; abscissa_kernel)
    int nj0z, any_lay3;    // any_lay3: some depth of the launch (of any plan of a parameter batch) lies above the screen top
    int any_lay1;          // ... below the screen bottom
    int any_fold;          // some plan of the launch folds a screen term (fold_dD or fold_lD1) or is model 4 (no screen terms): 0 = the NOFOLD instantiations may run
    int nz_out, z_off;     // depths of the whole call / offset of this launch's chunk: out index = pt*nz_out + z_off + z
    double timePar[2];
    double kappa, alphaD, beta;
    double lD, dD, bD, dD1, lD1;              // dD1 = 1-dD, lD1 = 1-lD (laplace_hankel_solutions.f90:157-158)
    double MoenchInvGamma[UCF_MAX_MOENCH];    // 1.0/gamma_m (:74)
    double alpha, logtol, maxexp;
    // fast flavour: hoisted reciprocals, plan-level exact folds, validity bound of the fast evaluation
    double inv_kappa, inv_bD, fast_eta_max, fast_im_max;
    int fold_dD, fold_lD1, share_g1top, _pad2;
    double g1_delta;       // (dD1 - 1) + dD, exact: the argument of cosh(eta (dD1 - 1)) is -(dD - g1_delta) (share_g1top = 2)
    // Hantush with wellbore storage (:204-301): rDw, CDw (:250), tDb (:253)
    double hs_rDw, hs_CDw, hs_tDb;
    // Mishra/Neuman (Malama form, :404-442): host-evaluated scalar prefactors
    double mn_vartheta, mn_u0, mn_c3;         // mn_c3 = 1 / (kappa u0^2): (eta1 / u0)^2 = (p vartheta + a^2) mn_c3
    // Mishra/Neuman FD (:444-544)
    double fd_h, fd_invhsq, fd_beta0, fd_beta3, fd_expmb2;   // exp(-beta2)
    double fd_isk, fd_gmax;                   // 1/sqrt(K), K = (1/h^2 - beta3/h)/h^2 (0 if K <= 0); 2^(500/order) - 1 (fd_inverse_B2)
    double hv[UCF_MAX_R];                     // Richardson spacings (driver.f90:91)
    double zD[UCF_MAX_NZ];
    int zLay[UCF_MAX_NZ];
    const double* ts_x;    // [N]      tanh(u2)+1 of the densest level (integration.f90:62 without *s/2)
    const double* ts_w;    // [R][N]   normalised weights of level j in row j-1 (first Nv(j) entries)
    const double* gl_x;    // [ngl]
    const double* gl_w;    // [ngl]
    const double* j0z;     // [nj0z]
    const double* fd_e;    // [order]  exp(-beta1*(j-1)*h)
    const double* sched;   // timeType = -n: [n] start times | [n] rate increments | final time | sum of increments
    const double* sc_tab;  // [256] x (sin, cos)(k pi / 128) | [128] x (hi, lo) of 2^(j/128): copied into LDS by the fast flavour's kernels
                           // (sincos_tab_, exp_tab_)
    double half_inv_kappa; // 0.5 / kappa = 0.5 * inv_kappa exactly (fast_eta<FAMILY, PAIR>); last, so that no other field moves
};
// The limits of the folded one-depth water-table kernel's bound classifier (zpair_unit_bounds, ucf_fastpath.h): the plan's
// limits squared, each pre-multiplied by kappa with its margin -- kappa (Re eta)^2 and (Im p)^2 / (kappa (Re eta)^2) are what
// the bounds compare.  The kernel reads them from the abscissa table (below), not from the parameter block: the block keeps
// its size, and with it every other kernel its code.
//   UCF_ZB_RANGE  kappa (0.99 fast_eta_max)^2     upper bound of kappa (Re eta)^2 below it: in range (0: fast evaluators off)
//   UCF_ZB_IM     kappa fast_im_max^2             (Im p)^2 < it times (Re p + a^2): |Im eta| < fast_im_max / 2
//   UCF_ZB_CS     kappa maxexp^2 / (1 + 2^-19)    upper bound below it: cosh/sinh form
//   UCF_ZB_EX     kappa maxexp^2 / (1 - 2^-19)    lower bound above it: exponential form
//   UCF_ZB_YS     4 kappa UCF_SC_SMALL^2          (Im p)^2 < it times (Re p + a^2): |Im eta| < UCF_SC_SMALL
//   UCF_ZB_YL     that / (1 - zD[0])^2            ... |Im eta| (1 - zD) < UCF_SC_SMALL (infinite at zD = 1: always)
//   UCF_ZB_SH     kappa (UCF_ZB_SINH_SERIES / zD[0])^2 / (1 - 2^-19)
//                                                 lower bound above it: Re eta zD >= UCF_ZB_SINH_SERIES, no sinh by its series
//                                                 (infinite at zD = 0: never)
#define UCF_ZB_SC_SMALL 0.012   /* UCF_SC_SMALL (ucf_math.h) */
#define UCF_ZB_SINH_SERIES 0.35 /* below it prim_from_e (ucf_fastpath.h) takes sinh from its series */
enum { UCF_ZB_RANGE = 0, UCF_ZB_IM, UCF_ZB_CS, UCF_ZB_EX, UCF_ZB_YS, UCF_ZB_YL, UCF_ZB_SH, UCF_ZB_COUNT = 8 };
// limit `which` of a call's parameter block (constexpr: host and device; every operation rounded on its own where
// abscissa_kernel is compiled)
static constexpr double zpair_bound_limit(const ucf_dev_params& dp, int which)
{
    const double lim = 0.99 * dp.fast_eta_max, me2 = dp.kappa * (dp.maxexp * dp.maxexp), c = 1.0 - dp.zD[0];
    const double ys = 4.0 * dp.kappa * (UCF_ZB_SC_SMALL * UCF_ZB_SC_SMALL);
    const double sh = UCF_ZB_SINH_SERIES / dp.zD[0];
    switch (which) {
    case UCF_ZB_RANGE: return lim > 0.0 ? dp.kappa * (lim * lim) : 0.0;
    case UCF_ZB_IM: return dp.kappa * (dp.fast_im_max * dp.fast_im_max);
    case UCF_ZB_CS: return me2 / (1.0 + 0x1p-19);
    case UCF_ZB_EX: return me2 / (1.0 - 0x1p-19);
    case UCF_ZB_YS: return ys;
    case UCF_ZB_YL: return ys / (c * c);
    case UCF_ZB_SH: return dp.kappa * (sh * sh) / (1.0 - 0x1p-19);
    default: return 0.0;
    }
}
// The abscissa table of a grid launch with `nrows` rows of `nabs` (abscissa, weight) pairs, in doubles: the rows, behind them
// the interval ends j0z[sv - 1 + j] / rD, j = 0 .. nacc, of every row, and behind those the UCF_ZB_COUNT limits (abscissa_kernel
// writes all three; point lists have the rows alone)
static constexpr size_t abscissa_ends_offset(size_t nrows, size_t nabs) { return nrows * nabs * 2; }
static constexpr size_t abscissa_limits_offset(size_t nrows, size_t nabs, size_t nacc) { return nrows * (nabs * 2 + nacc + 1); }
static constexpr size_t abscissa_table_doubles(size_t nrows, size_t nabs, size_t nacc) { return abscissa_limits_offset(nrows, nabs, nacc) + UCF_ZB_COUNT; }
#define UCF_SC_ENTRIES (256 + 128)   /* 16-byte units of that table */
#define UCF_IWPB 4             /* waves per workgroup of integrate_kernel: they share the sin/cos table in LDS */

// scratch columns hold UCF_PART lanes per slot: the per-lane tails (Neville, Wynn) run on one
// quarter-wave at a time, which quarters their LDS footprint at ~2 % of the point's time
#define UCF_PART 16
#define UCF_WYNN_REGS 12      /* terms the register-resident Wynn-epsilon of finish_kernel holds */

// build-time defaults of the integrate_kernel choice (tools/ubench/build_variant.sh and tools/probe_kernel.sh override them with -D)
#ifndef UCF_FOLD_WAVES
#define UCF_FOLD_WAVES 5
#endif
#ifndef UCF_UNFOLD_WAVES
#define UCF_UNFOLD_WAVES 4
#endif
// parts (2^k) of the work items of the last round of a launch (plan_transform)
#ifndef UCF_TAIL_LSPLIT_DEFAULT
#define UCF_TAIL_LSPLIT_DEFAULT 3
#endif
// launches of ONE depth of the fully penetrating water-table family in the lane = time layout (the headline sweep) run
// an instantiation that knows nz = 1 at compile time: no depth loop, no running area in LDS (measured on C2: -2.4 %).
// Only there: the unfolded and the finite-difference kernels LOSE 12 ... 46 % to it (C2pp 88 -> 100 ms, C4 237 -> 266,
// C5 204 -> 297: the compiler hoists the depth's constants into registers those kernels do not have)
// Launches of TWO depths in that layout (a screened observation well, C3; every pair of depths of a contour-style call,
// which the host walks two at a time) run NZC = 2 in every family: the two running areas in registers, so that the wave's
// LDS holds the level sums alone and a fourth workgroup fits the CU (C3 130.5 -> 115.2 ms per launch; 21-depth calls on
// 128 x 64 points: +5 ... +27 %, Theis +52 %; tools/gpu_depths.sh).  UCF_NZC2=0 (diagnostic) turns it off.
// (both name LAYOUT, the lane layout: a template argument in launch_transform_, a local of that name in plan_transform)
#ifndef UCF_NZC
#define UCF_NZC(F, FO) (LAYOUT == 1 && (F) == 2 && (FO) ? 1 : 0)
#endif
#ifndef UCF_NZC2
#define UCF_NZC2(F, FO) ((LAYOUT == 1 || LAYOUT == 3) ? 2 : 0)
#endif

static inline int family_of(const ucf_dev_params& dp)
{
    switch (dp.model) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 5;
    case 3: case 4: case 5: return 2;
    case 6: return dp.MNtype == 1 ? 3 : (dp.MNtype == 2 ? 4 : -1);
    default: return -1;
    }
}

// finished interval areas stay in LDS while the footprint still admits 8 single-wave workgroups per CU
static inline bool areas_in_lds(const ucf_dev_params& dp)
{
    const size_t with_areas = ((size_t)(dp.R + 1 + dp.nacc) * dp.nz * UCF_WAVE + (size_t)(2 * dp.nacc > dp.R ? 2 * dp.nacc : dp.R) * UCF_PART) * UCF_LDS_C;
    return with_areas <= 20 * 1024;
}

static inline size_t point_lds_bytes(const ucf_dev_params& dp, bool fast, bool resume = false)
{
    size_t bytes = ((size_t)(dp.R + 1 + ((areas_in_lds(dp) && !resume) ? dp.nacc : 0)) * dp.nz * UCF_WAVE + (size_t)(2 * dp.nacc > dp.R ? 2 * dp.nacc : dp.R) * UCF_PART) * UCF_LDS_C;
    if (!fast && family_of(dp) == 4) bytes += 2 * (size_t)dp.order * UCF_WAVE * UCF_LDS_C;
    return bytes;
}

// dynamic LDS of samples_kernel: the fast flavour's sin/cos table; the finite-difference Thomas buffer of the faithful one
static inline size_t samples_lds_bytes(const ucf_dev_params& dp, bool fast)
{
    if (fast) return UCF_SC_ENTRIES * UCF_LDS_C;
    return family_of(dp) == 4 ? 2 * (size_t)dp.order * UCF_WAVE * UCF_LDS_C : 16;
}

// How the abscissa loop is run: 0 inside point_kernel; 1 integrate_kernel with the fast evaluators (fast flavour,
// Hantush-based models), point_kernel resumes the items it leaves unfinished; 2 integrate_generic_kernel with the
// reference-order evaluators (everything else, unless the finite-difference Thomas buffer makes the footprint huge)
static inline int split_kind(const ucf_dev_params& dp, bool fast)
{
    const int fam = family_of(dp);
    if (fast) {
        if (fam >= 0 && fam <= 5) return 1;
    } else if (fam == 4 && 2 * (size_t)dp.order * UCF_WAVE * UCF_LDS_C > 16 * 1024) return 0;
    return 2;
}

// The two buffers that the kernels of a launch sequence share, for `nwork` work items and `lt_rows` rows of the call's tD.
// The host sizes them from here (ensure_state, ucf_drawdown.cpp) and the launchers index them from here.
//   counters (ints):  [ndone: abscissae done per item | todo: count of unfinished, unfinished items (integrate_kernel ->
//                      point_kernel) | defer: count of (item, depth) pairs left to the guarded epsilon table, those pairs
//                      (pt * nz + z; finish_kernel) | wcount: the work counter of the persistent integrate grid]
//   state (bytes):    [items][(R+1+nacc)*nz][64] complex (integrate kernel -> finish / point kernel; 0: the abscissa loop has no
//                     kernel of its own) | the lapTime table of laptime_kernel, [lt_rows][2M+1] complex (fast flavour)
struct ucf_transform_buffers {
    size_t ndone, todo, defer, wcount;      // offsets (ints) into the counters
    size_t ints;                            // ... and their total
    size_t state_item_bytes;                // state of one work item
    size_t ltab;                            // offset (bytes) of the lapTime table behind the state
    size_t state_bytes;                     // state and table
};
static inline ucf_transform_buffers transform_buffers(const ucf_dev_params& dp, bool fast, size_t nwork, size_t lt_rows)
{
    const int kind = split_kind(dp, fast);
    ucf_transform_buffers b;
    b.ndone = 0;
    b.todo = b.ndone + nwork;
    b.defer = b.todo + 1 + nwork;
    b.wcount = b.defer + 1 + nwork * (size_t)dp.nz;
    b.ints = b.wcount + 2;
    b.state_item_bytes = kind ? (size_t)(dp.R + 1 + dp.nacc) * dp.nz * UCF_WAVE * UCF_LDS_C : 0;
    b.ltab = nwork * b.state_item_bytes;
    b.state_bytes = b.ltab + (kind == 1 ? lt_rows * dp.np * UCF_LDS_C : 0);
    return b;
}

// integrate_kernel<family, LAYOUT, waves, MULTI, fold, lay3, nzc, lay1, nofold>
struct ucf_integrate_choice {
    int waves;             // waves per SIMD the register budget is cut for
    bool fold, lay3;
    int nzc;
    bool lay1, nofold;
};
// finish_kernel<LAYOUT, part, wreg, MODE>: two_pass = MODE 1 over all items, then MODE 2 over what it deferred; else MODE 0
struct ucf_finish_choice {
    int part;
    bool wreg, two_pass;
};
// [laptime_kernel -> integrate_kernel | integrate_generic_kernel -> finish_kernel ->] point_kernel
struct ucf_transform_plan {
    int fam, kind;                         // family_of, split_kind
    size_t point_lds;                      // point_kernel
    unsigned point_grid;
    bool global_areas;                     // ... keeps its finished interval areas in the global scratch (glscr)
    // kind 1
    int lsplit, ltail, ntail, nhead;       // 2^lsplit parts per item, 2^ltail for the last nwork - nhead items
    long long nworkw;                      // work units (parts) in all
    bool persist;
    unsigned integrate_grid;
    int nrows;                             // rows of the lapTime table
    unsigned laptime_grid;
    ucf_integrate_choice ik;
    size_t integrate_lds;
    // kind 2
    size_t generic_lds;                    // integrate_generic_kernel
    // kind 1 and 2
    ucf_finish_choice fin;
    size_t finish_lds;
    unsigned finish_grid2;                 // grid of the second pass
    ucf_transform_buffers buf;             // for nwork items and nrows rows
};

// The transform stage for `nwork` work items of lane layout `layout` (multi: a parameter batch).  per_point, nr, nt: as in
// ucf_launch (ucf_plan.h).  Returns UCF_OK or the error the launch sequence ends with; *out is complete only on UCF_OK.
static inline int plan_transform(const ucf_dev_params& dp, const ucf_env& env, bool fast, int layout, bool multi, int nwork, int per_point,
                                 int nr, int nt, ucf_transform_plan* out)
{
    const int LAYOUT = layout;
    ucf_transform_plan P = {};
    const int fam = P.fam = family_of(dp);
    if (fam < 0) return UCF_ERR_UNSUPPORTED;
    const int kind = P.kind = split_kind(dp, fast);
    const bool split = kind != 0;
    P.point_lds = point_lds_bytes(dp, fast, split);
    if (P.point_lds > 160 * 1024) return UCF_ERR_UNSUPPORTED;
    const bool al = areas_in_lds(dp) || split;
    P.global_areas = !al;
    P.point_grid = (unsigned)((al || nwork < env.grid_slots) ? nwork : env.grid_slots);
    if (kind == 1) {
        // parts per item: launches of fewer than ~8 rounds of resident waves (256 CUs x 4 SIMDs x <= 6 waves) run two parts
        // per item -- measured on the 1/8 shard of C2 (27 136 items, tools/gpu_shard.sh): 5.37 / 5.26 / 5.35 / 5.58 ms with
        // 1 / 2 / 4 / 8 parts (every part pays the item's set-up again).  UCF_NSPLIT (diagnostic): force 1, 2, 4 or 8 parts.
        const int force_split = env.nsplit;
        int lsplit = 0;
        while (lsplit < 1 && ((long long)nwork << lsplit) < 8LL * 256 * 4 * 6) lsplit++;
        if (force_split > 0) { lsplit = 0; while ((1 << (lsplit + 1)) <= force_split && lsplit < 3) lsplit++; }
        if ((1 << lsplit) > dp.nacc + 1) lsplit = 0;
        // ... and the last items of EVERY launch run in finer parts: ntail = one round of resident waves, 2^ltail parts each
        // (UCF_TAIL_ITEMS / UCF_TAIL_LSPLIT: diagnostic overrides; UCF_TAIL_LSPLIT=0 turns the finer tail off).  Measured
        // (tools/gpu_tail_parts.sh): C2 34.78 -> 34.64 ms, its 1/8 shard 4.835 -> 4.79 ms with 8 parts for the last 5 120
        // items (2 or 4 parts, or 10 240 items: the same within 0.2 %) -- a small gain: a wave on an emptying SIMD does
        // speed up enough to hide most of the quantisation of a launch into rounds.  Bit-neutral like every cut
        // (test_results_do_not_depend_on_how_work_items_are_cut).
        const int tail_ls_env = env.tail_lsplit, tail_items_env = env.tail_items;
        int ltail = tail_ls_env >= 0 ? tail_ls_env : UCF_TAIL_LSPLIT_DEFAULT;
        if (ltail > 3) ltail = 3;
        while (ltail > 0 && (1 << ltail) > dp.nacc + 1) ltail--;
        if (ltail < lsplit) ltail = lsplit;
        int ntail = tail_items_env >= 0 ? tail_items_env : 256 * 4 * 5;
        if (ntail > nwork) ntail = nwork;
        const int nhead = (ltail == lsplit) ? nwork : nwork - ntail;
        const long long nworkw = ((long long)nhead << lsplit) + ((long long)(nwork - nhead) << ltail);
        if (nworkw > 0x7fffffffLL) return UCF_ERR_UNSUPPORTED;
        P.lsplit = lsplit; P.ltail = ltail; P.ntail = ntail; P.nhead = nhead; P.nworkw = nworkw;
        // per workgroup: the sin/cos table + UCF_IWPB waves' accumulators; wlds = the footprint one wave accounts for
        const size_t wlds = (size_t)(dp.R + 1) * dp.nz * UCF_WAVE * UCF_LDS_C + UCF_SC_ENTRIES * UCF_LDS_C / UCF_IWPB;
        // persistent grid: at most 8 workgroups per CU (more than any register / LDS budget admits; the ones that do not fit
        // start when others have finished and find the counter exhausted).  UCF_PERSIST=0 (diagnostic): one workgroup per
        // UCF_IWPB work units, as before round 3's last pass
        P.persist = env.persist;
        const long long nwg = (nworkw + UCF_IWPB - 1) / UCF_IWPB;
        P.integrate_grid = (unsigned)((P.persist && nwg > 256 * 8) ? 256 * 8 : nwg);
        // lapTime(p) x constants for every (row of the call's tD, m): rows = the times of a grid / the points of a list.
        // The table lives behind the state of this launch's work items (transform_buffers)
        // (LAYOUT 1: the nt times; 3: the nt points of the launch; 0 / 2: the points, or -- a small grid walked point by point,
        //  per_point = 0 -- the time rows those points stand on: tD has no more entries than that)
        const int npts_l = (LAYOUT == 2) ? nwork / ((dp.np + UCF_WAVE - 1) / UCF_WAVE) : nwork;
        P.nrows = (LAYOUT == 1 || LAYOUT == 3) ? nt : (per_point ? npts_l : (npts_l + nr - 1) / nr);
        P.laptime_grid = (unsigned)(((long long)P.nrows * dp.np + 255) / 256);
        // (parameter batches: the water-table and Hantush families only, ucf_drawdown_multi)
        if (multi && (fam == 0 || fam == 3 || fam == 5)) return UCF_ERR_UNSUPPORTED;
        const bool nzc2_on = env.nzc2;      // diagnostic: 0 = off
        // a depth above the screen top anywhere in the call (in any plan of a parameter batch)?
        const bool lay3 = dp.any_lay3 != 0;
        // ... below the screen bottom?  Three instantiations of an unfolded kernel: every layer / beside and below the screen /
        // beside the screen only (the usual piezometer or observation well)
        const bool lay1 = dp.any_lay1 != 0;
        // neither screen term folds (d > 0 and l < b: the usual partially penetrating well) -- known at compile time in an
        // instantiation of its own (NOFOLD, ucf_fastpath.h); a plan that folds exactly one term, and a parameter batch with
        // such a plan or a fully penetrating one in it, run the general one.  UCF_NOFOLD=0 (diagnostic): always the general one
        const bool nofold = env.nofold && !dp.any_fold;
        // fully penetrating pumping well (every plan of a parameter batch must be): the screen terms are compiled out
        const bool fold = dp.fold_dD && dp.fold_lD1 && !multi;
        // two depths of the water-table family in the lane = time layout: running areas in registers (NZC = 2), level sums
        // alone in LDS -- at R = 4 a workgroup then needs 38 instead of 46 KB and FOUR of them fit a CU (measured on C3:
        // 130.5 -> 115.2 ms per launch with the 4-waves register budget; 127.3 ms with 3)
        const bool nzc2 = UCF_NZC2(2, false) != 0 && fam == 2 && nzc2_on && dp.nz == 2;
        const size_t wlds_eff = (nzc2 || (UCF_NZC(2, true) != 0 && fam == 2 && fold && dp.nz == 1))
                                    ? (size_t)dp.R * dp.nz * UCF_WAVE * UCF_LDS_C + UCF_SC_ENTRIES * UCF_LDS_C / UCF_IWPB : wlds;
        const bool w5 = wlds_eff * 20 <= 160 * 1024;
        int waves = 4;      // families 1, 3, 4, 5
        if (fam == 0) waves = (wlds * 24 <= 160 * 1024) ? 6 : 4;
        else if (fam == 2 && fold) {
            // register budget: 5 waves per SIMD (96 VGPRs, 8 of them spilled around the abscissa loop) where the LDS
            // footprint admits them.  Round 3, C2: 35.8 / 34.8 / 34.8 ms at 4 / 5 / 6 waves -- the sixth wave buys nothing
            // any more and costs 16 more spilled registers per item (2 GB of scratch traffic per sweep); the 1/8 shard
            // runs 5.29 against 5.33 ms.  UCF_FOLD_WAVES_RT (diagnostic): force 4, 5 or 6.
            const int force_w = env.fold_waves_rt;
            if (force_w == 4) waves = 4;
            else if (force_w == 6 && wlds_eff * 24 <= 160 * 1024) waves = 6;
            else if (w5) waves = UCF_FOLD_WAVES;
            else waves = 4;
        } else if (fam == 2) {
            // the screen terms need the registers: 4 waves/SIMD (128 VGPRs, ~60 spilled; 5 waves: -31 %); with two or more
            // depths per launch 3 waves/SIMD and no spills are 3 % faster (C3), with one depth 5 % slower (C2pp)
            const int unf_w = env.unfold_waves_rt;      // diagnostic: 3 or 4
            waves = (unf_w == 3 || (unf_w != 4 && dp.nz >= 2 && !nzc2)) ? 3 : UCF_UNFOLD_WAVES;
        }
        // families 0 and 3 have the folded form only (MNtype 1 is fully penetrating by construction, driver_io.f90:159-186)
        const bool fo = fold || fam == 0 || fam == 3;
        P.ik.waves = waves;
        P.ik.fold = fo;
        P.ik.lay3 = !fo && lay3;
        P.ik.lay1 = fo || lay3 || lay1;
        P.ik.nofold = !fo && nofold;
        P.ik.nzc = (UCF_NZC(fam, fo) && dp.nz == 1) ? UCF_NZC(fam, fo) : (UCF_NZC2(fam, fo) && dp.nz == 2 && nzc2_on) ? UCF_NZC2(fam, fo) : 0;
        P.integrate_lds = ((size_t)(P.ik.nzc ? dp.R : dp.R + 1) * dp.nz * UCF_WAVE * UCF_LDS_C) * UCF_IWPB + UCF_SC_ENTRIES * UCF_LDS_C;
    }
    if (kind == 2) {
        if (multi) return UCF_ERR_UNSUPPORTED;
        P.generic_lds = (size_t)(dp.R + 1) * dp.nz * UCF_WAVE * UCF_LDS_C;
        if (!fast && fam == 4) P.generic_lds += 2 * (size_t)dp.order * UCF_WAVE * UCF_LDS_C;
    }
    if (split) {
        // tails of the completed items.  nacc <= UCF_WYNN_REGS: epsilon table in registers, LDS only for the level sums
        // and the Neville column; else the widest scratch part that still leaves 4 waves per CU (measured on C2:
        // 4.8 / 3.6 / 3.1 ms for parts of 16 / 32 / 64 lanes)
        const bool wreg = dp.nacc <= UCF_WYNN_REGS && !env.finish_part;
        const size_t scols = wreg ? (size_t)dp.R : (size_t)(2 * dp.nacc > dp.R ? 2 * dp.nacc : dp.R);
        auto flds = [&](int part) { return ((size_t)dp.R * dp.nz * UCF_WAVE + scols * part) * UCF_LDS_C; };
        int part = env.finish_part;
        if (part != 16 && part != 32 && part != 64) part = (flds(64) <= 40 * 1024) ? 64 : (flds(32) <= 40 * 1024) ? 32 : 16;
        P.finish_lds = flds(part);
        if (P.finish_lds > 160 * 1024) return UCF_ERR_UNSUPPORTED;
        // fast flavour, epsilon table in registers: the pass with the unguarded table over all items, then the guarded one over
        // what that pass listed (buf.defer: [count | pt * nz + z ...] behind the two lists of integrate_kernel)
        // (a grid-stride pass with 4 096 ... 65 536 workgroups instead of one per item: 0.92 ms on C2 either way -- the pass is
        //  bound by the 3.3 GB of state it reads, not by workgroup launches)
        P.fin.part = part; P.fin.wreg = wreg; P.fin.two_pass = fast && wreg;
        P.finish_grid2 = (unsigned)(nwork < 12288 ? nwork : 12288);      // (4 rounds of resident waves; an empty list costs ~6 us)
        // the unfinished ones (overflow regime): point_kernel over the list integrate_kernel left
        P.point_grid = (unsigned)(nwork < 2048 ? nwork : 2048);
    }
    P.buf = transform_buffers(dp, fast, (size_t)nwork, kind == 1 ? (size_t)P.nrows : 0);
    *out = P;
    return UCF_OK;
}
