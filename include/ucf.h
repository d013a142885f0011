/*
 * ucf.h -- C ABI of the MI355X-native Laplace-Hankel drawdown engine.
 *
 * This is the drop-in boundary for the one hot path of klkuhlm/unconfined: the
 * per-(t,r) loop body of `program Driver` (reference driver.f90:100-276) and the
 * module procedures it imports (reference driver.f90:28-40).  The reference has
 * no FFI for this path (its only ISO_C_BINDING precedent is arb_J/arb_Y,
 * reference laplace_hankel_solutions.f90:310-325: scalars by value, plain
 * numbers); every entry point below therefore names the reference procedure or
 * loop it replaces.  A reference-side binding (Fortran `bind(C)` interface block)
 * is shown in INTEGRATION.md and shipped in unconfined_amd/fortran/.
 *
 * Conventions
 *   - plain C: pointers + sizes, caller-owned contiguous fp64 / int32 arrays;
 *   - complex vectors travel as interleaved (re,im) doubles;
 *   - every function returns UCF_OK (0) or a negative ucf_status; nothing aborts
 *     (the reference `stop`s on bad input, driver_io.f90:78-378; we return the
 *     matching UCF_ERR_* instead and ucf_last_error() gives the message);
 *   - "in-band" numerical rules of the reference (NaN->0 scrub, Wynn-epsilon
 *     truncation/sentinel, epsilon-table early exit, FD underflow guard) are
 *     part of the numerical contract and are reproduced on the device;
 *   - threading / streams (the reference calls its procedures from OpenMP threads with shared read-only
 *     parameter objects, driver.f90:129-230): any number of host threads may call the drawdown entry points on ONE
 *     plan at the same time.  Everything a call writes lives in a workspace that the plan keeps PER HIP STREAM:
 *     calls on different streams share nothing and run concurrently; calls that name the same stream (the host
 *     point-list entry uses the default stream, the host grid entries a stream that the plan owns for its lifetime)
 *     are enqueued one after the other under the workspace's lock and execute in stream order.  The *_device entry points never synchronise; they allocate only when a workspace
 *     must grow (outgrown buffers are kept until the stream has drained, never freed under a running kernel), and not
 *     at all after ucf_plan_reserve -- which is what capturing them into a hipGraph needs.
 *     What may NOT overlap with calls in flight on the same plan: ucf_plan_update, ucf_plan_set_mode,
 *     ucf_plan_set_timing, ucf_plan_destroy (the caller orders those; ucf_plan_update waits for the plan's own
 *     streams before it rewrites a device table).
 *   - there is NO CPU fallback: every compute entry point fails with
 *     UCF_ERR_NO_DEVICE if no gfx950-capable HIP device is usable.
 */
#ifndef UCF_H
#define UCF_H

#ifdef __cplusplus
extern "C" {
#endif

#define UCF_VERSION 100        /* 0.1.0 */
#define UCF_MAX_MOENCH 16      /* max number of Moench alphas (driver_io.f90:142-151) */
#define UCF_MAX_NZ 32          /* depths per LAUNCH; calls with more depths are walked in chunks by the library */
#define UCF_MAX_SCHEDULE 100    /* steps of a piecewise-constant pumping schedule (time.f90:81-95) */
#define UCF_MAX_LAP_M 127      /* 2M+1 <= 256: the wave-cooperative de Hoog holds up to four samples per lane (the reference takes
                                  any M >= 2, driver_io.f90:306-309; its QD table is numerically void long before M = 127) */

typedef enum ucf_status {
    UCF_OK = 0,
    UCF_ERR_INVALID_MODEL = -1,     /* driver_io.f90:90-97   */
    UCF_ERR_GEOMETRY = -2,          /* driver_io.f90:236-258 */
    UCF_ERR_AQUIFER = -3,           /* driver_io.f90:242-252 */
    UCF_ERR_MISHRA_NEUMAN = -4,     /* driver_io.f90:260-276 */
    UCF_ERR_MALAMA_BETA = -5,       /* driver_io.f90:278-281 */
    UCF_ERR_MOENCH = -6,            /* driver_io.f90:142-149,283-290 */
    UCF_ERR_DEHOOG = -7,            /* driver_io.f90:306-309 */
    UCF_ERR_TANH_SINH = -8,         /* driver_io.f90:316-327 */
    UCF_ERR_GAUSS_LOBATTO = -9,     /* driver_io.f90:329-333 */
    UCF_ERR_UNSUPPORTED = -10,      /* valid in the reference, not built here (see ucf_last_error) */
    UCF_ERR_BAD_ARGUMENT = -11,
    UCF_ERR_NO_DEVICE = -12,
    UCF_ERR_HIP = -13,
    UCF_ERR_NOMEM = -14,
    UCF_ERR_OBSERVATION = -15,      /* driver_io.f90:352-383 */
    UCF_ERR_SINGULAR = -16          /* ucf_fit_solve_step: the damped normal matrix is not positive definite */
} ucf_status;

/*
 * POD mirror of the reference's parameter types as read from the 18-line deck
 * (types.f90:31-225: well, formation, solution, invLaplace, TanhSinh,
 * invHankel, GaussLobatto).  Dimensional quantities, exactly as on the deck;
 * non-dimensionalisation (driver_io.f90:531-567) happens in ucf_plan_create.
 */
typedef struct ucf_params {
    int model;            /* 0 Theis, 1 Hantush, 2 Hantush+storage, 3 Moench, 4 Malama full, 5 Malama partial, 6 Mishra/Neuman */
    int MNtype;           /* model 6: 0 naive (ARB, unsupported), 1 Malama, 2 finite difference */
    int order;            /* model 6 / MNtype 2: FD nodes in the vadose zone */
    int timeType;         /* pumping-rate time behaviour (time.f90:46): 1..8; -n (-1..-100) = n-step piecewise-CONSTANT
                             schedule; -(100+n) (-101..-200) = n-segment piecewise-LINEAR schedule (time.f90:97-122);
                             the 2n+1 parameters of either are in timeParExt */
    double timePar[2];
    double Q;             /* pumping rate [L^3/T] */
    double l, d;          /* depth to screen bottom / top from aquifer top [L] */
    double rw, rc;        /* well / casing radius [L] */
    double gammaSkin;
    double b;             /* saturated thickness [L] */
    double Kr, kappa;     /* radial K [L/T], Kz/Kr */
    double Ss, Sy;
    double beta;          /* Malama linearisation parameter */
    int MoenchM;
    int _pad0;
    double MoenchAlpha[UCF_MAX_MOENCH];
    double ac, ak, psia, psik, usL;   /* Mishra/Neuman vadose-zone parameters */
    int M;                /* de Hoog: 2M+1 Laplace samples */
    int k;                /* tanh-sinh: N = 2^k - 1 abscissae */
    int R;                /* Richardson levels */
    int nacc;             /* J0-zero intervals accelerated by Wynn-epsilon */
    int ord;              /* Gauss-Lobatto order (ord-2 interior nodes) */
    int j0s[2];           /* min/max J0 zero at which finite/infinite parts split */
    int _pad1;
    double alpha, tol;    /* de Hoog abscissa of convergence, tolerance */
    double rwobs, sF;     /* observation well radius / shape factor (model 2) */
    /* piecewise constant: tpar(1:n) step start times, tpar(n+1) final time, tpar(n+2:2n+1) rates (types.f90:66-70).
     * piecewise linear: tpar(1:n) knot times t_1 < ... < t_n, tpar(n+1) = t_f, tpar(n+2:2n+1) = the rate at t_2, ..., t_n,
     * t_f; the rate is 0 up to t_1, continuous ("no jumps", time.f90:98), linear between knots, constant after t_f.
     * (The reference reads the n rates as y(t_1..t_n) and then indexes y(n+1), one past its array, time.f90:101,115:
     * its transform only ever uses rate DIFFERENCES, i.e. it assumes a rate that starts from 0 at t_1 -- the reading
     * here is the one under which every parameter is used and nothing is read out of bounds) */
    double timeParExt[2 * UCF_MAX_SCHEDULE + 1];
} ucf_params;

/* Derived, dimensionless quantities (driver_io.f90:531-567) -- read back for tests/headers. */
typedef struct ucf_derived {
    double Lc, Tc, Hc;
    double sigma, alphaD, betaD;
    double lD, dD, bD, rDw, rDwobs;
    double acD, akD, lambdaD, psiaD, psikD, usLD, b1, PsiD;
    double MoenchGamma[UCF_MAX_MOENCH];
    double l_eff, d_eff, ac_eff;   /* after the MNtype==1 overrides (driver_io.f90:159-186) */
    int np;       /* 2M+1 */
    int N;        /* 2^k-1 */
    int nj0z;     /* max(j0s)+nacc+1 */
    int nabs;     /* N + nacc*(ord-2): abscissae per point */
} ucf_derived;

/* Counters of the in-band rules taken during a batch. */
typedef struct ucf_stats {
    long long nan_scrubbed;     /* invlap.f90:71-74  : NaN Laplace samples set to 0        */
    long long zero_vectors;     /* invlap.f90:69,139 : all-zero f(p) -> f(t)=0             */
    long long wynn_truncated;   /* integration.f90:150-158 : series cut at first non-finite */
    long long wynn_sentinel;    /* integration.f90:142-149 : < 4 usable terms -> -999999.9  */
    long long wynn_early_exit;  /* integration.f90:169-177 : |denom| <= 2.2e-16             */
    long long wynn_all_zero;    /* driver.f90:209 : every area exactly 0 -> 0 (quirk Q5)   */
} ucf_stats;

typedef struct ucf_plan ucf_plan;

int ucf_version(void);
const char* ucf_last_error(void);          /* thread-local message of the last failure */
const char* ucf_status_string(int status);

/* ---- plan: replaces read_input's numerical half + the `first`-time setup in the driver
 * (driver_io.f90:531-567,628-647; driver.f90:79-91,121-126,138-151,179-183). ---- */
int ucf_plan_create(const ucf_params* P, ucf_plan** out);        /* bound to the HIP device that is current */
int ucf_plan_create_on(const ucf_params* P, int device, ucf_plan** out);   /* bound to HIP device `device` (0-based) */
int ucf_device_count(int* n);                                    /* UCF_ERR_NO_DEVICE if there is none */
void ucf_plan_destroy(ucf_plan* plan);
/* New hydraulic / geometric / schedule parameters for an existing plan (parameter estimation: thousands of
 * parameter sets, one set of numerical settings): everything that depends on them (driver_io.f90:531-567 and the
 * per-model constants) is recomputed, the quadrature tables, workspaces, flavour and timing switches stay.  The model
 * and the numerical settings (M, k, R, nacc, ord, J0 split, FD order, schedule length, number of Moench terms) must
 * not change: UCF_ERR_BAD_ARGUMENT otherwise.  Microseconds instead of the ~0.3 ms of ucf_plan_create. */
int ucf_plan_update(ucf_plan* plan, const ucf_params* P);
int ucf_plan_derived(const ucf_plan* plan, ucf_derived* out);
/* the same quantities without a plan (host arithmetic only, no GPU needed): read_input's checks (driver_io.f90:88-333)
 * and its non-dimensionalisation (:531-567) */
int ucf_nondimensionalise(const ucf_params* P, ucf_derived* out);
int ucf_plan_j0z(const ucf_plan* plan, int n, double* j0z);             /* driver_io.f90:628-647 */
int ucf_plan_tanh_sinh(const ucf_plan* plan, int level /*1..R*/, int n, double* w, double* x_unit /* tanh(u2)+1, level R only, may be NULL */);
int ucf_plan_gauss_lobatto(const ucf_plan* plan, int n, double* x, double* w);
/* execution mode: 0 = faithful (reference operation order, no FMA contraction),
 *                 1 = fast (same algorithm, FMA contraction + shared subexpressions). */
int ucf_plan_set_mode(ucf_plan* plan, int mode);

/* measurement: when enabled, every kernel of a following grid call in the lane = time layout is bracketed by HIP events
 * on the call's stream.  ucf_plan_kernel_times waits for the brackets of the last such call and returns one row per
 * kernel in order of first launch: total duration [ms], number of launches (a call that walks the radii in chunks
 * launches every kernel once per chunk; may be NULL) and name (as rocprofv3 prints it, without "void " and the
 * argument list); ucf_plan_kernel_ms returns the per-launch duration of the kernel with the largest total. */
int ucf_plan_set_timing(ucf_plan* plan, int enable);
int ucf_plan_kernel_times(ucf_plan* plan, int cap, double* ms, int* launches, const char** names, int* n);
int ucf_plan_kernel_ms(ucf_plan* plan, double* ms, const char** kernel_name);

/* Size the workspaces of `stream` (hipStream_t as void*, NULL = default stream) for calls to come -- a grid of nt x nr
 * points (0 x 0: none) and / or a point list of npts points (0: none), nz depths each -- so that the *_device entry
 * points allocate nothing afterwards.  ucf_plan_alloc_count: device allocations made so far on behalf of calls. */
int ucf_plan_reserve(ucf_plan* plan, int nt, int nr, int npts, int nz, void* stream);
long long ucf_plan_alloc_count(const ucf_plan* plan);

/* sha256 (first 16 hex digits) of the kernel and host sources this library was built from: measurement files under
 * profiles/ carry it, and bench.py refuses a profile whose id differs from the library it runs. */
const char* ucf_build_id(void);

/* ---- host-side helpers that the reference computes in read_input ---- */
int ucf_logspace(int lo, int hi, int n, double* out);                   /* utility.f90:51-57 */
int ucf_linspace(double lo, double hi, int n, double* out);             /* utility.f90:34-49 */
int ucf_zlay(const ucf_plan* plan, int nz, const double* zD, int* zLay);            /* driver_io.f90:575-586 */
int ucf_split_vector(const ucf_plan* plan, int nt, const double* tD, int* sv);      /* driver_io.f90:654-664 */

/* ---- the hot path: replaces the body of the (i,k) loop nest, driver.f90:100-232.
 * Points are independent (flattened t x r); per point: tD, rD, sv (1-based index
 * into j0z).  Outputs h, dh are dimensionless, [npts][nz] row-major, *before* the
 * screen averaging of driver.f90:234-243 (see ucf_screen_average). ---- */
int ucf_drawdown_batch(ucf_plan* plan, int npts,
                       const double* tD, const double* rD, const int* sv,
                       int nz, const double* zD, const int* zLay,
                       double* h, double* dh, ucf_stats* stats /* may be NULL */);

/* Same, all per-point arrays already resident in HBM; asynchronous on `stream`
 * (a hipStream_t passed as void*; NULL = default stream).  `d_stats` may be NULL.
 * Preconditions the library cannot check on device-resident inputs: 1 <= sv[i] <= nj0z - nacc (sv indexes the
 * J0-zero table; the host entry points check it and return UCF_ERR_BAD_ARGUMENT). */
int ucf_drawdown_batch_device(ucf_plan* plan, int npts,
                              const double* d_tD, const double* d_rD, const int* d_sv,
                              int nz, const double* zD, const int* zLay,
                              double* d_h, double* d_dh, ucf_stats* d_stats, void* stream);

/* The same loop body over the product grid the reference's driver actually walks
 * (do i = 1,nt / do k = 1,nr, driver.f90:100,113): nt times (tD[i], sv[i]) x nr radii rD[k].
 * Outputs [nt][nr][nz] row-major.  Abscissae and a*J0(a*rD) depend only on (rD, sv) and are
 * computed once per radius here instead of once per point. */
int ucf_drawdown_grid(ucf_plan* plan, int nt, const double* tD, const int* sv, int nr, const double* rD,
                      int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats);
int ucf_drawdown_grid_device(ucf_plan* plan, int nt, const double* d_tD, const int* d_sv, int nr, const double* d_rD,
                             int nz, const double* zD, const int* zLay, double* d_h, double* d_dh,
                             ucf_stats* d_stats, void* stream);
/* (device-resident sv of a grid must lie in the plan's split range [min(j0s), max(j0s)]: it selects a row of the
 *  per-radius abscissa table; ucf_split_vector produces such values and ucf_drawdown_grid checks them) */

/* ---- the sweep on several GPUs.  Every (t,r) point is independent; the shard axis is the reference's
 * own serial loop nest (do i = 1,nt / do k = 1,nr, driver.f90:100,113): the flattened index i*nr + k is cut into
 * `world` contiguous blocks of whole time rows, B = ceil(nt / world) rows each (the last ones may be short or empty),
 * so that a shard is itself a product grid and its results are one contiguous slice of [nt][nr][nz].
 * No data-path collective; the only exchange is the final gather of the slices. */
int ucf_shard_rows(int nt, int world, int rank, int* lo, int* hi);     /* rows [lo, hi) of shard `rank`; no GPU needed */

/* One process per GPU (the bench, RCCL): the rank computes ITS rows of the sweep and leaves them at their place in the
 * full-size device arrays d_h, d_dh [world*B][nr][nz] (d_tD, d_sv: all nt rows), so that an IN-PLACE all-gather of
 * B*nr*nz doubles per rank (ncclAllGather with sendbuff = recvbuff + rank*count; torch.distributed
 * all_gather_into_tensor on a view) completes the arrays on every rank.  Asynchronous on `stream`. */
int ucf_drawdown_grid_shard_device(ucf_plan* plan, int rank, int world, int nt, const double* d_tD, const int* d_sv,
                                   int nr, const double* d_rD, int nz, const double* zD, const int* zLay,
                                   double* d_h, double* d_dh, ucf_stats* d_stats, void* stream);

/* The same with the gather inside the library: the rank's rows, then one in-place ncclAllGather per array on `stream`
 * (sendbuff = recvbuff + rank * B*nr*nz) over the RCCL communicator `comm` (an ncclComm_t passed as void*: the host's
 * own, or one made by ucf_comm_create).  Asynchronous; d_h, d_dh must hold world*B rows.  RCCL is bound when the first
 * of these entries is called (dlopen: libucf.so itself links no collective library); UCF_ERR_UNSUPPORTED without it.
 * This is the "final RCCL gather over xGMI" of the sweep: the reference writes ONE file from one address space
 * (driver.f90:245-273), every rank ends up holding that whole result. */
int ucf_drawdown_grid_allgather(ucf_plan* plan, int rank, int world, int nt, const double* d_tD, const int* d_sv,
                                int nr, const double* d_rD, int nz, const double* zD, const int* zLay,
                                double* d_h, double* d_dh, ucf_stats* d_stats, void* comm, void* stream);
/* A communicator of the library's own for hosts that have none: rank 0 draws the 128-byte id (ncclGetUniqueId) and hands
 * it to the other ranks by whatever the host has (a file, MPI, torch.distributed ...); every rank then calls
 * ucf_comm_create with the HIP device it computes on current (ncclCommInitRank). */
int ucf_comm_unique_id(unsigned char* id128);
int ucf_comm_create(const unsigned char* id128, int world, int rank, void** comm);
int ucf_comm_destroy(void* comm);

/* One process driving ngpu devices (the Fortran host): plans[g] was created with device g current (ucf_plan_create
 * binds a plan to the current HIP device) from the same parameters.  Host arrays in and out like ucf_drawdown_grid;
 * shard g runs on plans[g]'s device on a stream of its own, all devices at once, and the gather is each device's
 * copy of its slice straight into rows lo..hi of h and dh (one PCIe/xGMI transfer per device: staging the slices
 * through one GPU first would only add a hop).  stats: summed over the shards.  ngpu = 1 is ucf_drawdown_grid. */
int ucf_drawdown_grid_multi(ucf_plan* const* plans, int ngpu, int nt, const double* tD, const int* sv, int nr,
                            const double* rD, int nz, const double* zD, const int* zLay, double* h, double* dh,
                            ucf_stats* stats);

/* The point-list counterpart (ucf_drawdown_batch_multi): block g of the list -- ucf_shard_rows over
 * the npts points -- runs on plans[g]'s device, one host thread per device, each through ucf_drawdown_batch (which
 * orders its block by radius); results land in the caller's order in h, dh [npts][nz].  ngpu = 1 is ucf_drawdown_batch. */
int ucf_drawdown_batch_multi(ucf_plan* const* plans, int ngpu, int npts, const double* tD, const double* rD, const int* sv,
                             int nz, const double* zD, const int* zLay, double* h, double* dh, ucf_stats* stats);

/* Parameter-batched evaluation for inversion / fitting (the tool's real use,
 * reference README.md:45-56): the SAME observation points -- dimensional times t[npts], radii r[npts],
 * depths z[nz] (z up from the aquifer base) -- under nplans parameter sets.  Each plan
 * non-dimensionalises with its own Lc, Tc (driver_io.f90:531-567), gets its own layers and split vector.
 * Fast-flavour plans of the same model and numerical settings (M, k/R, nacc/ord, alpha, tol, J0 split) -- the
 * fitting case: only hydraulic / geometric parameters vary -- share ONE launch sequence over (plan, point) work
 * items with per-plan parameter blocks in device memory; any other mix runs plan by plan on a small pool of
 * HIP streams so that the small launches overlap.  Plan by plan the results ARE the single-plan calls; the shared launch
 * sequence runs other instantiations of the same kernels (parameter blocks in memory, often another lane layout), in
 * which the compiler may contract a product and a sum into an FMA where the single-plan instantiation does not: same
 * formulas, results equal to the rounding noise of the fast flavour -- bit for bit on most decks at their own settings,
 * otherwise as far apart as either is from exact arithmetic (tests/test_gpu_contract.py judges that against binary128).
 * h, dh: [nplans][npts][nz]; dimensional (x Hc of each plan) unless dimensionless != 0. */
int ucf_drawdown_multi(ucf_plan* const* plans, int nplans, int npts, const double* t, const double* r,
                       int nz, const double* z, int dimensionless, double* h, double* dh);

/* ---- parameter fitting: what the batched evaluation above is for (reference README.md:45-56, PEST).  A fit object owns the
 * observations on the device, evaluates base and perturbed parameter sets through the launch sequence of ucf_drawdown_multi
 * (same kernels; the plans come from a pool that the fit makes once and refreshes with ucf_plan_update; h stays in device
 * memory, nothing but kilobytes of sums crosses the bus) and forms residuals, objective, Jacobian and normal equations in
 * one small kernel of its own (fit_reduce_kernel, one workgroup per parameter set, sums in a fixed order: a call repeated
 * gives the same bits).
 *   parameters   all positive, fitted in ln(theta); theta arrays hold the parameters themselves, in the order of `ids`;
 *   observation  a DIMENSIONAL drawdown (h x Hc: what a deck with dimensionless = F prints) at dimensional time t[i], radius
 *                r[i] and depth z[iz[i]], z up from the aquifer base as in ucf_drawdown_multi.
 *   cost         ucf_fit_create: ALL nz depths are evaluated at every observation point and iz selects one.  An observation
 *                network with per-well depths and screened wells is made by ucf_fit_create_network (below): there a point is
 *                evaluated at the depths of its own well only, and the screen average is formed on the device.
 *   sim_i(theta) the fast-flavour result of the plan made from ucf_fit_perturb(base, theta);   r_i = obs_i - sim_i;
 *   J[i][j]      (sim_i(theta e^{+dlog e_j}) - sim_i(theta e^{-dlog e_j})) / (2 dlog): the derivative in ln(theta_j);
 *   phi = sum w_i^2 r_i^2,  g = J' W^2 r,  A = J' W^2 J (full symmetric [npar][npar]).
 *   An observation whose base value or any perturbed value is not finite (the in-band rules of the overflow regime produce
 *   such values) is left out of that set's sums and counted in nbad[set]; its rows of J / sim_all hold what was computed.
 * A fit is used by one host thread at a time; every plan of a fit lives on the fit's device. */
#define UCF_FIT_MAX_PAR 8
enum { UCF_PAR_KR, UCF_PAR_KAPPA, UCF_PAR_SS, UCF_PAR_SY, UCF_PAR_AC, UCF_PAR_AK, UCF_PAR_USL,
       UCF_PAR_MOENCH_ALPHA0 /* + i, i < MoenchM */ };
/* ucf_fit_lm, per start */
enum { UCF_FIT_CONVERGED = 0, UCF_FIT_MAX_ITER = 1, UCF_FIT_SINGULAR = 2 /* A + lambda diag A not positive definite */,
       UCF_FIT_NONFINITE_START = 3 /* nbad > 0 or phi not finite at theta0 */ };
typedef struct ucf_fit ucf_fit;
typedef struct ucf_fit_options { int max_iter; double dlog, lambda0, lambda_up, lambda_down, tol_step, tol_phi; } ucf_fit_options;
/* max_iter 50, dlog 1e-3 (the end-to-end noise floor is 1e-10 relative; its cube root, 5e-4, is where the
 * truncation and the rounding error of a central difference balance, and within a factor 2 of it they still do), lambda0 1e-2,
 * lambda_up 10, lambda_down 0.1, tol_step 1e-6 (max |step| in ln theta), tol_phi 1e-9 (relative decrease of phi) */
int ucf_fit_default_options(ucf_fit_options* opt);

/* host arithmetic only, no GPU: */
/* *out = *base with the fields named by ids[0..npar) set to theta[0..npar) and no other byte changed.  UCF_ERR_BAD_ARGUMENT:
 * npar outside 1..UCF_FIT_MAX_PAR, a duplicate id, an id that base->model does not read (kappa for Theis; Sy for models 0..2;
 * ak outside model 6; ac, usL outside model 6 / MNtype 2; a Moench alpha outside model 3 or beyond MoenchM) */
int ucf_fit_perturb(const ucf_params* base, int npar, const int* ids, const double* theta, ucf_params* out);
/* (A + lambda diag A) step = g by a Cholesky factorisation, A [npar][npar] symmetric; UCF_ERR_SINGULAR (step = 0, never a
 * NaN) where the matrix is not positive definite */
int ucf_fit_solve_step(int npar, const double* A, const double* g, double lambda, double* step);

/* Validation comes first and needs no GPU -- UCF_ERR_BAD_ARGUMENT, ucf_last_error names the offender: the checks of
 * ucf_fit_perturb, nobs < npar, iz outside 0..nz-1, a negative or non-finite weight, a non-finite obs, t, r or z, t or r <= 0;
 * base itself is checked as by ucf_plan_create (with its statuses).  Then UCF_ERR_NO_DEVICE as for every compute entry. */
int ucf_fit_create(const ucf_params* base, int npar, const int* ids,
                   int nobs, const double* t, const double* r, const int* iz, int nz, const double* z,
                   const double* obs, const double* weight, int device, ucf_fit** out);
void ucf_fit_destroy(ucf_fit* fit);
/* nsets parameter sets theta[nsets][npar] at once: nsets (1 + 2 npar) plans in one launch sequence (plan by plan on a pool of
 * streams for the models that have no shared launch, see ucf_drawdown_multi).  phi[nsets], g[nsets][npar],
 * A[nsets][npar][npar], nbad[nsets]; J [nsets][nobs][npar] and sim_all [nsets][1 + 2 npar][nobs] (row 0 the base values, row
 * 1 + 2j parameter j up, row 2 + 2j parameter j down) only when asked for; any output may be NULL.
 * A theta that is not positive and finite: UCF_ERR_BAD_ARGUMENT; a parameter set that fails the checks of ucf_plan_update:
 * that status, with the set and the parameter in ucf_last_error. */
int ucf_fit_evaluate(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/, double dlog,
                     double* phi, double* g, double* A, int* nbad,
                     double* J /*NULL ok, [nsets][nobs][npar]*/, double* sim_all /*NULL ok, [nsets][1+2npar][nobs]*/);
/* Levenberg-Marquardt from nstarts starting points theta0[nstarts][npar], all advancing together: per iteration one
 * ucf_fit_evaluate over the starts that moved and one base-values-only evaluation of the trial points.  Per start: step from
 * ucf_fit_solve_step with Marquardt's damping, accepted if the trial has nbad = 0 and phi did not grow (lambda x
 * lambda_down), rejected otherwise (lambda x lambda_up); converged when max |step| <= tol_step or an accepted step lowers
 * phi by no more than tol_phi x phi; starts that are finished drop out of the batch.  theta[nstarts][npar], phi[nstarts],
 * iters[nstarts], status[nstarts] (UCF_FIT_*); cov [nstarts][npar][npar] = phi / (nobs - npar) A^-1 at the final point, in
 * ln theta (NaN where it does not exist), costs one more evaluation. */
int ucf_fit_lm(ucf_fit* fit, int nstarts, const double* theta0, const ucf_fit_options* opt /*NULL = defaults*/,
               double* theta, double* phi, int* iters, int* status, double* cov /*NULL ok*/);
/* device allocations made so far by the fit and its plans (a repeated call of the same size makes none) */
long long ucf_fit_alloc_count(const ucf_fit* fit);

/* An observation network: nwell wells, well w at radius well_r[w] with well_nz[w] depths (1..UCF_MAX_NZ) stored
 * consecutively in well_z (z up from the aquifer base, dimensional).  Observation i: time t[i] at well well[i];
 * iz[i] >= 0 selects depth iz[i] OF THAT WELL, iz[i] == UCF_FIT_SCREEN (-1) is the screen average of all of the
 * well's depths by the rule of ucf_screen_average.  Only the depths of its own well are evaluated at a point.
 *   launch       wells are grouped by their number of depths, one launch sequence of ucf_drawdown_multi per distinct number.
 *                Inside a group the distinct times of every (parameter set, well) are cut into blocks of 64 points (the last
 *                block of a well repeats its last time; those results are never read), wells in order of radius, and every
 *                block carries the parameter block of its plan with the depths of its well: the kernels are those of
 *                ucf_drawdown_multi, unchanged.  Models without a shared launch run plan by plan and well by well through
 *                ucf_drawdown_batch_device on the stream pool.  Each plan's split vector is taken over all the launched times
 *                of the network, so a value does not depend on how the wells fall into groups.
 *   reduction    fit_reduce_kernel over network_source: as above, but an observation finds its value through (offset, count):
 *                count 1 reads one double per plan; count n > 1 forms s = v[1]; s = s + v[j], j = 2..n-1;
 *                ((v[0] + 2 s) + v[n-1]) / (2 n) on the dimensionless h, then x Hc -- the operations of ucf_screen_average.
 * A well that no observation names is never launched; observations that share a (well, time) share one evaluation.  J and
 * sim_all come back in the caller's observation order.  ucf_fit_evaluate, ucf_fit_lm, ucf_fit_destroy and
 * ucf_fit_alloc_count work on the object as on one made by ucf_fit_create.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_fit_create
 * checks, nwell < 1, well_nz outside 1..UCF_MAX_NZ, well[i] outside 0..nwell-1, iz[i] outside -1..well_nz[w]-1, a well_r that
 * is not finite and positive, a well_z that is not finite. */
#define UCF_FIT_SCREEN (-1)
int ucf_fit_create_network(const ucf_params* base, int npar, const int* ids,
                           int nwell, const double* well_r, const int* well_nz, const double* well_z,
                           int nobs, const double* t, const int* well, const int* iz,
                           const double* obs, const double* weight, int device, ucf_fit** out);
/* (point, depth) evaluations per parameter set that this fit launches (padding included) and that the dense form
 * -- every depth of the network at every (well, time) -- would launch.  Host arithmetic, no launch.  For a fit made by
 * ucf_fit_create launched == dense. */
int ucf_fit_eval_counts(const ucf_fit* fit, long long* launched, long long* dense);
/* the same two numbers from the network alone (no fit object, no GPU); checks well_nz, well[i] and t[i] as above */
int ucf_fit_network_eval_counts(int nwell, const int* well_nz, int nobs, const double* t, const int* well,
                                long long* launched, long long* dense);
/* diagnostic: the dimensionless h behind observation i under plan `plan` (set * (1 + 2 npar) + row) as the LAST
 * ucf_fit_evaluate left it in device memory: n = 1 value for a point observation, the n depths of the well for a screen
 * average (what its average was formed from).  cap < n: UCF_ERR_BAD_ARGUMENT.  On a fit made by ucf_fit_create_field i is a
 * TERM index (ucf_fit_field_terms): the h behind that term, at its own time and distance. */
int ucf_fit_debug_h(ucf_fit* fit, int plan, int i, int cap, double* h, int* n);

/* A field fit: the observations of an interference test -- several pumping wells, wells that start at different times, image
 * wells for a river or an outcrop -- fitted against the superposition that ucf_field_* maps.  npump pumping wells (xw, yw, qw,
 * t0w) with the meaning of ucf_field_create (qw a factor on the plan's Q, never 0; t0w >= 0); an image well is a plain entry,
 * so the output of ucf_field_images can be passed as it is.  nwell observation wells at (well_x, well_y) with depths well_nz /
 * well_z as in ucf_fit_create_network.  Observation i: dimensional drawdown at time t[i] in well well[i], at depth iz[i] of
 * that well or, with iz[i] == UCF_FIT_SCREEN, its screen average.
 *   value        acc = +0.0;  for j = 0..npump-1 in the caller's order, only where t[i] > t0w[j]:
 *                    v = the plan's dimensionless h at time t[i] - t0w[j] and distance |well - pumping well j|, at the
 *                        observation's depth or averaged over the well's depths by the rule of ucf_screen_average (what
 *                        a network observation is before x Hc);   acc = acc + qw[j] * v;
 *                sim = acc * Hc.  Every operation is rounded on its own.  An observation that no well's start precedes has
 *                sim = +0.0 and is legal.  Nothing is scrubbed: a term that is not finite makes sim not finite and the
 *                observation is counted in nbad.
 *   layout       host arithmetic, stated by ucf_fit_field_terms.  dist = sqrt(dx dx + dy dy), dimensional, as in ucf_field_group.
 *                One VIRTUAL WELL per (observation well, distinct distance): pairs of one observation well whose distances
 *                are equal bit for bit share it; it carries the depths of its observation well; virtual wells are ordered by
 *                observation well, then by ascending distance.  One TERM per (observation i, pumping well j with t[i] >
 *                t0w[j]): time t[i] - t0w[j] (one rounding), its virtual well, qw[j]; the terms of an observation keep the
 *                caller's order of pumping wells.
 *   launch       the virtual wells with the term times as their observation times are the network of
 *                ucf_fit_create_network, launched as stated there: distinct times per virtual well in blocks of 64, groups
 *                by number of depths, one split vector per plan over all launched term times, the shared launch where the
 *                plans have one and plan by plan, virtual well by virtual well otherwise.  Terms that land on the same
 *                (virtual well, time) share one evaluation.  A map of ucf_field_drawdown takes one split vector per
 *                group of wells, this fit one over all term times: where wells start at different times the two differ by
 *                that choice, not by rounding alone.
 *   reduction    fit_reduce_kernel over field_source: as for a network, the value of an observation being the sum above.
 * ucf_fit_evaluate, ucf_fit_lm, ucf_fit_destroy and ucf_fit_alloc_count work on the object unchanged; J and sim_all come back
 * in the caller's observation order; ucf_fit_eval_counts reports launched and dense of the network of virtual wells (every
 * virtual well's depths count in dense); ucf_fit_debug_h takes a term index.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything
 * ucf_fit_create_network checks, with well_x / well_y (finite) in place of well_r; what ucf_field_create checks on the pumping
 * wells (npump < 1, NULL, a number that is not finite, t0w < 0, qw == 0); a distance that is not finite or below base->rw --
 * the observation well is inside a bore -- naming the (observation well, pumping well) pair; more than 2^24 pairs or terms;
 * no term at all.  Then UCF_ERR_NO_DEVICE. */
int ucf_fit_create_field(const ucf_params* base, int npar, const int* ids,
                         int npump, const double* xw, const double* yw, const double* qw, const double* t0w,
                         int nwell, const double* well_x, const double* well_y, const int* well_nz, const double* well_z,
                         int nobs, const double* t, const int* well, const int* iz,
                         const double* obs, const double* weight, int device, ucf_fit** out);
/* host only: what the fit above launches and sums -- nvirt virtual wells (virt_well: the observation well, virt_r: the
 * distance), term_first[i] .. term_first[i + 1] the terms of observation i, per term its pumping well, its virtual well and
 * its time.  Arrays sized for the worst case; any output may be NULL.  The checks of ucf_fit_create_field that concern these
 * arguments (base as by ucf_plan_create). */
int ucf_fit_field_terms(const ucf_params* base,
                        int npump, const double* xw, const double* yw, const double* qw, const double* t0w,
                        int nwell, const double* well_x, const double* well_y,
                        int nobs, const double* t, const int* well,
                        int* nvirt, int* virt_well /*[nwell*npump]*/, double* virt_r /*[nwell*npump], dimensional*/,
                        int* term_first /*[nobs+1]*/, int* term_pump, int* term_virt, double* term_t /*[nobs*npump] each*/);

/* Derivative data: the log-time derivative t ds/dt of the drawdown, fitted jointly with the drawdown itself.  The evaluators
 * write dh = t dh/dt beside every h; a fit keeps it in device memory in the layout of h, and a fit that has derivative data
 * reads it in the reduction.  No evaluator launch is added.
 *   dobs[i]      the observed DIMENSIONAL derivative t ds/dt of observation i (a length: what a deck with dimensionless = F
 *                prints in its derivative column), dweight[i] >= 0 its weight.  dweight[i] == 0: observation i has no
 *                derivative datum and dobs[i] may be anything, NaN included.  nd = number of i with dweight[i] > 0.
 *   simd_i       the simulated derivative of observation i under a plan, every operation rounded on its own:
 *                  ucf_fit_create          dh[plan][place of i] * Hc[plan];
 *                  ucf_fit_create_network  what the reduction of that entry forms from h, formed from dh: one value, or the
 *                                          screen average over the well's depths by the rule of ucf_screen_average; then x Hc;
 *                  ucf_fit_create_field    acc = +0.0; over the terms of i in the caller's order of pumping wells
 *                                          acc = acc + q * (tfac * v), v as for a network on the term's dh and
 *                                          tfac = t[i] / term_t (one division of the observation's own time by the term time
 *                                          that ucf_fit_field_terms states: the factor tfac of ucf_field_group; exactly 1
 *                                          for a well that starts at 0); acc * Hc.  The operation order of ds in
 *                                          field_superpose_kernel.
 *   Jd[i][j]     (simd_i(theta e^{+dlog e_j}) - simd_i(theta e^{-dlog e_j})) / (2 dlog).
 *   reduction    fit_joint_reduce_kernel, fit_network_joint_reduce_kernel, fit_field_joint_reduce_kernel: per observation, in
 *                the lane order and with the fixed reduction order of the kernels without derivative data,
 *                  1. s[k] and sd[k] of every plan of the set; sim, simd, J, Jd are written where asked, finite or not;
 *                  2. the observation counts when every s[k] is finite AND (dweight[i] == 0 OR every sd[k] is finite);
 *                     otherwise it adds 1 to nbad and nothing to the sums.  With all dweight == 0 that is the rule of a fit
 *                     without derivative data, and phi, g, A, nbad have the same bits;
 *                  3. the drawdown term, operation for operation as without derivative data;
 *                  4. where dweight[i] > 0 (skipped otherwise, not added as zero), into the same sums:
 *                       wr = wd_i * (dobs_i - sd[0]);   phi = phi + wr*wr;   phi_d = phi_d + wr*wr;
 *                       dd_j = (sd[1+2j] - sd[2+2j]) / (2 dlog);   wdd_j = wd_i * dd_j;
 *                       g_j = g_j + wdd_j * wr;   A_jk = A_jk + wdd_j * wdd_k  (j <= k).
 *                No floating-point atomics: a call repeated gives the same bits. */
/* host only, no GPU.  UCF_ERR_BAD_ARGUMENT, the offender in ucf_last_error: a NULL array, a dweight[i] that is negative or not
 * finite, a dobs[i] that is not finite where dweight[i] > 0.  *nd = number of i with dweight[i] > 0. */
int ucf_fit_derivative_check(int nobs, const double* dobs /*[nobs]*/, const double* dweight /*[nobs]*/, int* nd);
/* attaches dobs, dweight [nobs of the fit, in the caller's observation order] to a fit made by any of the three constructors
 * (ucf_fit_derivative_check first; then two device buffers of the fit, counted in ucf_fit_alloc_count the first time, and for
 * a field fit a third with tfac per term); NULL for both arrays detaches them again (the buffers stay with the fit). */
int ucf_fit_set_derivative(ucf_fit* fit, const double* dobs, const double* dweight);
/* On a fit WITH derivative data ucf_fit_evaluate and ucf_fit_lm return the joint phi, g, A and nbad, so that ucf_fit_lm fits
 * both curves, and cov = phi / (nobs + nd - npar) A^-1; on a fit without, both run what they ran before these entries existed.
 * ucf_fit_evaluate_joint is ucf_fit_evaluate plus phi_d[nsets], the derivative terms' share of phi, Jd [nsets][nobs][npar] and
 * simd_all [nsets][1 + 2 npar][nobs] (rows as in sim_all); any output may be NULL.  UCF_ERR_BAD_ARGUMENT on a fit without
 * derivative data. */
int ucf_fit_evaluate_joint(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/, double dlog,
                           double* phi, double* g, double* A, int* nbad, double* J, double* sim_all,
                           double* phi_d, double* Jd, double* simd_all);
/* diagnostic: as ucf_fit_debug_h, the dimensionless dh behind observation (field fit: term) i of the last evaluation */
int ucf_fit_debug_dh(ucf_fit* fit, int plan, int i, int cap, double* dh, int* n);
/* The objective of many parameter sets without a Jacobian: what ucf_fit_lm runs at its trial points.  Only the base plan of
 * every set is evaluated (nsets plans, not nsets (1 + 2 npar)) and the reduction is the npar = 0 instantiation of
 * fit_reduce_kernel, in the order of sums stated with ucf_debug_fit_reduce.  Every kind of fit (ucf_fit_create,
 * ucf_fit_create_network, ucf_fit_create_field).  phi [nsets], nbad [nsets]; sim [nsets][nobs] the simulated value of EVERY
 * observation, counted or not (NULL ok).  On a fit with derivative data phi is the joint sum, and phi_d [nsets], the derivative
 * terms' share of it, and simd [nsets][nobs] may be asked for; without derivative data either of them is UCF_ERR_BAD_ARGUMENT.
 * The checks of ucf_fit_evaluate except dlog, which is not an argument; nsets up to 2^20.  A repeated call of the same size
 * allocates nothing (ucf_fit_alloc_count). */
int ucf_fit_objective(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/,
                      double* phi, int* nbad, double* sim /*NULL ok*/, double* phi_d /*NULL ok*/, double* simd /*NULL ok*/);

/* Robust losses.  A loss is a property of a fit, like derivative data: once set, every entry that reduces residuals uses it.
 * The residuals exist only inside fit_reduce_kernel, so the loss is applied there: no evaluator launch and no traffic is added.
 *   kinds        UCF_LOSS_L2 (plain least squares, the default), UCF_LOSS_HUBER, UCF_LOSS_TUKEY (the biweight);
 *   c            the tuning constant, positive and finite, in units of the WEIGHTED residual: sigmas where weight = 1 / sigma.
 * A weighted residual x -- the drawdown term wr with its weighted derivatives wd_j, or the derivative term wrd with wdd_j; the
 * same rule and the same c for both -- gives rho(x) and the factor b(x), every operation rounded on its own:
 *     a = fabs(x)
 *     HUBER:  a <= c :  b = 1.0;            rho = x * x
 *             else   :  b = c / a;          rho = c * (2.0 * a - c)
 *     TUKEY:  c2 = c * c;  u = x / c
 *             a <  c :  v = 1.0 - u * u;  b = v * v;  rho = (c2 * (1.0 - b * v)) / 3.0
 *             else   :  b = 0.0;            rho = c2 / 3.0
 * and the sums, in place of the least-squares ones, in the same order and over the same counted observations:
 *     phi   = phi   + rho            (derivative term: also phi_d = phi_d + rho)
 *     phi_w = phi_w + b * (x * x)    (new, the last entry of a set's sums: phi | g | A | [phi_d] | phi_w)
 *     bw_j  = b * wd_j;   g_j = g_j + bw_j * x;   A_jk = A_jk + bw_j * wd_k   (j <= k)
 *     ndown[set] = number of counted residual terms (drawdown and derivative) with b < 1.0
 * This is the IRLS / Gauss-Newton form: the term of the loss's second derivative is dropped, so A stays positive
 * semidefinite.  Unchanged: the rule that decides whether an observation counts, nbad, "the derivative term is skipped where
 * dweight == 0", the lane / butterfly / wave order of the sums, the absence of floating-point atomics.  Consequences:
 *   - Huber with c >= every |x| gives the bits of least squares in phi, g, A, phi_d and nbad, and phi_w has the bits of phi;
 *   - at a == c both branches of Tukey give the same rho (b = 0 * 0, rho = (c2 * 1.0) / 3.0 = c2 / 3.0);
 *   - an infinite x gives b = 0 and rho = +inf under Huber. */
enum { UCF_LOSS_L2 = 0, UCF_LOSS_HUBER = 1, UCF_LOSS_TUKEY = 2 };
/* host only, no GPU, compiled without contraction: the arithmetic above on x[n] -> rho[n], b[n]; UCF_LOSS_L2 gives rho = x * x,
 * b = 1.0 and does not read c.  UCF_ERR_BAD_ARGUMENT: a kind outside the enum, a c that is not positive and finite (Huber,
 * Tukey), n < 0, a NULL array. */
int ucf_fit_loss_terms(int kind, double c, int n, const double* x, double* rho, double* b);
/* host only, no GPU: *scale = 1.4826 * m, m the median of fabs(x[i]) over the finite x[i]: the k of them sorted ascending
 * into a[0..k), m = a[k / 2] for odd k and (a[k / 2 - 1] + a[k / 2]) / 2.0 for even k (the textbook median); one product.  The
 * usual estimate of sigma from residuals that hold outliers; a multiple of it (4.685 for 95 % efficiency under Tukey, 1.345
 * under Huber) is the usual c.  UCF_ERR_BAD_ARGUMENT: n < 1, a NULL argument, no finite entry. */
int ucf_fit_robust_scale(int n, const double* x, double* scale);
/* sets the loss of a fit made by any of the three constructors; UCF_LOSS_L2 detaches it (c is then not read).  The argument
 * checks come before anything else (NULL fit, a kind outside the enum, c not positive and finite); the call allocates nothing.
 * From here on ucf_fit_evaluate, ucf_fit_evaluate_joint, ucf_fit_objective and ucf_fit_lm reduce with the loss: their phi and
 * phi_d are the robust sums, g and A the reweighted ones above, and ucf_fit_lm accepts and rejects on the robust phi.
 *   cov          of ucf_fit_lm = phi_w / (nobs + nd - npar) A^-1 with the IRLS A at the final point: the covariance of the
 *                WEIGHTED LEAST-SQUARES problem that the final factors define.  It is NOT a sandwich estimator: it ignores
 *                that the factors depend on the data, and understates the variance when many observations are down-weighted.
 * On a fit whose loss is UCF_LOSS_L2 every one of these entries returns the bits it returned before a loss existed. */
int ucf_fit_set_loss(ucf_fit* fit, int kind, double c);
int ucf_fit_get_loss(const ucf_fit* fit, int* kind, double* c /*0.0 under UCF_LOSS_L2*/);
/* The factors at given parameter sets: how a caller flags outliers at a fitted theta.  Evaluates the base plans only, through the
 * npar = 0 reduction, as ucf_fit_objective does, on every kind of fit, with the fit's loss.  phi, phi_w [nsets], nbad, ndown
 * [nsets], b, bd [nsets][nobs] in the caller's observation order: the factor of observation i's drawdown residual and of its
 * derivative residual, NaN where the observation does not count (bd: or has dweight == 0).  Any output may be NULL; bd on a fit
 * without derivative data is UCF_ERR_BAD_ARGUMENT.  On a fit whose loss is UCF_LOSS_L2 b is 1.0 where the observation counts,
 * phi_w has the bits of phi and ndown is 0.  The checks of ucf_fit_objective.  A repeated call of the same size allocates
 * nothing (ucf_fit_alloc_count). */
int ucf_fit_loss_report(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/,
                        double* phi, double* phi_w, int* nbad, int* ndown, double* b, double* bd);

/* Resampled fits.  cov of ucf_fit_lm is linearised and model-based; the honest spread of a fit comes from refitting on bootstrap or
 * jackknife replicates of the data.  A replicate is a vector of integer multiplicities on the observations, and like a loss it is
 * applied where the residuals are, inside fit_reduce_kernel: no evaluator launch is added per replicate, and several replicates
 * reduced at the same parameter set read one evaluation.
 *   mult         [nrep][nobs] unsigned short, in the caller's observation order; m = mult[rep][i] copies of observation i;
 *   reduction r  one workgroup: the plans of parameter set set_of[r] (set_of NULL: r) under the multiplicities of replicate rep[r];
 *                rep[r] == -1 (or rep NULL): every m = 1.  Every output is indexed by r.
 * Per observation i, on top of the arithmetic of ucf_fit_set_loss (least squares runs as Huber with c = +inf, every factor 1.0),
 * every operation rounded on its own, in the lane / butterfly / wave order of ucf_debug_fit_reduce, no floating-point atomics;
 * `ok` is the counting rule stated there:
 *     m == 0 (held out) and ok:  phi_out = phi_out + wr * wr;  where dweight_i > 0 also  phi_out = phi_out + wrd * wrd;  nheld++.
 *              A held-out observation adds nothing else and is never counted in nbad; one that is not ok is in no count at all.
 *     m > 0 and not ok:          nbad++          (once, not m times)
 *     m > 0 and ok:              fm = (double)m;  (rho, b) of x = wr;  fb = fm * b;
 *              phi = phi + fm * rho;  phi_w = phi_w + fb * (x * x);  bw_j = fb * wd_j;  g_j = g_j + bw_j * x;
 *              A_jk = A_jk + bw_j * wd_k (j <= k);  ndown++ where b < 1.0 (once);  nuse += m;
 *              then, where dweight_i > 0, the derivative term x = wrd with its own b by the same rules, also
 *              phi_d = phi_d + fm * rho, and nuse_d += m.
 *     sums per reduction:  phi | g | upper A | [phi_d] | phi_w | phi_out;   counts per reduction: nuse, nuse_d, nheld, ndown.
 * Consequence: with every m = 1, fm * x == x exactly, so phi, g, A, phi_d, phi_w, nbad and ndown have the bits of the reduction
 * under the fit's loss (ucf_fit_set_loss), and under least squares the bits of the plain one.
 *
 * ucf_fit_set_resample attaches mult to a fit made by any of the three constructors; NULL detaches (nrep is then not read).  The
 * device buffer stays with the fit and is counted in ucf_fit_alloc_count when it grows.  A row with no positive entry is legal.
 * Every existing entry (ucf_fit_evaluate, _joint, _objective, _lm, _loss_report) ignores the multiplicities and returns the bits it
 * returns without them.  UCF_ERR_BAD_ARGUMENT before any GPU work: a NULL fit, nrep outside 1..65536, a row whose entries sum
 * beyond 2^31 - 1 (the counts are int; the row is named). */
int ucf_fit_set_resample(ucf_fit* fit, int nrep, const unsigned short* mult /*[nrep][nobs]; NULL: detach*/);
/* One evaluation of the nsets (1 + 2 npar) plans that ucf_fit_evaluate makes of theta, then ONE reduction launch of nred workgroups.
 * phi, phi_d, phi_w, phi_out [nred], g [nred][npar], A [nred][npar][npar] (full, symmetric), nbad [nred], counts [nred][4] = nuse,
 * nuse_d, nheld, ndown.  Any output may be NULL.  On a fit without derivative data nuse_d is 0 and phi_d is refused.  A repeated
 * call of the same size allocates nothing (ucf_fit_alloc_count).  UCF_ERR_BAD_ARGUMENT before any GPU work: the checks of
 * ucf_fit_evaluate; nred outside 1..2^20; set_of NULL with nred > nsets; a set_of[r] outside 0..nsets-1; a rep[r] outside
 * -1..nrep-1; a rep[r] != -1 on a fit without attached multiplicities; phi_d on a fit without derivative data. */
int ucf_fit_evaluate_resampled(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/, double dlog,
                               int nred, const int* set_of /*[nred]; NULL: r*/, const int* rep /*[nred]; NULL: all -1*/,
                               double* phi, double* g, double* A, int* nbad, double* phi_d, double* phi_w, double* phi_out,
                               int* counts /*[nred][4]*/);
/* the same on the base plans only, through the npar = 0 instantiations (no dlog, g or A): what ucf_fit_lm_resampled runs at its
 * trial points, and the cross-validation score phi_out of many replicates at one theta.  The same checks. */
int ucf_fit_objective_resampled(ucf_fit* fit, int nsets, const double* theta /*[nsets][npar]*/,
                                int nred, const int* set_of, const int* rep,
                                double* phi, int* nbad, double* phi_d, double* phi_w, double* phi_out, int* counts);
/* ucf_fit_lm with start s reduced under replicate rep[s] (set_of the identity): the same loop, not a copy -- the same steps,
 * damping, stopping rules and status; accept and reject decisions use the replicate's phi; a start is UCF_FIT_NONFINITE_START
 * where an observation with m > 0 is not finite at theta0.  From one more evaluation at the final point:
 *   cov          = phi_w / (nuse + nuse_d - npar) A^-1 per start, NaN where the denominator is <= 0, A is singular, nbad > 0 or
 *                the start was not finite: ucf_fit_lm's cov of the replicate's own weighted problem.  The spread that resampling
 *                is for comes from the thetas over the replicates (ucf_fit_resample_cov), not from this matrix;
 *   phi_out      [nstarts] the held-out sum of squares (the cross-validation score of a jackknife replicate), NaN for a start
 *                that was not finite;  counts [nstarts][4], 0 there.
 * cov, phi_out, counts: NULL ok.  With rep all -1 (or NULL) theta, phi, iters, status and cov have the bytes of ucf_fit_lm.  The
 * checks of ucf_fit_lm, and a rep[s] outside -1..nrep-1 or != -1 without attached multiplicities, before any GPU work. */
int ucf_fit_lm_resampled(ucf_fit* fit, int nstarts, const double* theta0, const int* rep /*[nstarts]; NULL: all -1*/,
                         const ucf_fit_options* opt /*NULL = defaults*/,
                         double* theta, double* phi, int* iters, int* status, double* cov, double* phi_out, int* counts);
/* host only, no GPU, compiled without contraction: the block bootstrap.  block[i] is the block (well, time window) of observation i,
 * in 0..nb-1 with every id used, nb = the largest id + 1; block NULL: block i = i (nb = nobs), the iid bootstrap.  Replicates in
 * ascending order, each with nb draws; a draw is one step of the splitmix64 stream stated at ucf_field_ensemble_draw (state = seed,
 * one stream for the whole call), then  k = (x * nb) >> 64  as a 128-bit unsigned product, and every observation of block k gains
 * 1.  mult [nrep][nobs] (NULL: only *nblock is set);  *nblock = nb (NULL ok).  UCF_ERR_BAD_ARGUMENT: nobs outside 1..2^24, nrep
 * outside 1..65536, a block id that is negative or >= nobs, an id below the largest that no observation has, a count beyond 65535
 * (the replicate is named). */
int ucf_fit_resample_blocks(int nobs, const int* block /*[nobs]; NULL: iid*/, int nrep, unsigned long long seed,
                            unsigned short* mult /*[nrep][nobs]*/, int* nblock);
/* host only, no GPU: delete-one-block.  Row b of mult [nb][nobs] is 0 on the observations of block b and 1 elsewhere: leave one
 * well out, or k-fold cross-validation with fold ids as blocks.  block NULL: block i = i.  The checks of ucf_fit_resample_blocks on
 * nobs and block; a NULL mult. */
int ucf_fit_resample_jackknife(int nobs, const int* block /*[nobs]; NULL: i*/, unsigned short* mult /*[nb][nobs]*/);
/* host only, no GPU, compiled without contraction: mean and covariance in ln theta over the n replicates r with use[r] != 0 (use
 * NULL: all), every operation rounded on its own, every sum from +0.0 in ascending r:
 *     x_rj = log(theta[r][j]);   s_j = s_j + x_rj;   mean_j = s_j / (double)n;
 *     c_jk = c_jk + (x_rj - mean_j) * (x_rk - mean_k)   for j <= k, mirrored;
 *     UCF_RESAMPLE_BOOTSTRAP:  cov_jk = c_jk / (double)(n - 1);     UCF_RESAMPLE_JACKKNIFE:  cov_jk = c_jk * ((double)(n - 1) / (double)n)
 * mean [npar], cov [npar][npar], *nused = n; each NULL ok.  UCF_ERR_BAD_ARGUMENT: a kind outside the enum, nrep < 1, npar outside
 * 1..UCF_FIT_MAX_PAR, a NULL theta, n < 2, a used theta that is not positive and finite (replicate and parameter named). */
enum { UCF_RESAMPLE_BOOTSTRAP = 0, UCF_RESAMPLE_JACKKNIFE = 1 };
int ucf_fit_resample_cov(int kind, int nrep, int npar, const double* theta /*[nrep][npar]*/, const int* use /*[nrep]; NULL: all*/,
                         double* mean, double* cov, int* nused);

/* ---- well fields: the drawdown of several pumping wells -- wells that start at different times, image wells for a river or an
 * outcrop -- is the sum over wells of q_j h(t - t0_j, |x - x_j|, z).  All wells share the plan's aquifer, well geometry and
 * time behaviour; they differ in position (xw, yw), rate factor qw (times the plan's Q; negative: injection or a constant-head
 * image; never 0) and start time t0w >= 0.  A map of a field is a product grid per group of wells that share a start time:
 * times after the start x distinct distances, which is what ucf_drawdown_grid_device is built for.  A field object owns the
 * geometry and the device buffers; h and dh of the groups stay in device memory, one small kernel forms the sums, and only the
 * superposed s, ds cross the bus.  All inputs are dimensional as for ucf_drawdown_multi, z up from the aquifer base.
 *   groups       wells with bitwise-equal t0w form a group; groups in ascending t0, wells inside a group in the caller's order.
 *   launch       per group g ONE call of the grid path in the plan's current flavour with exactly the arrays that
 *                ucf_field_group states:  k0 = first k with t[k] > t0_g, nt_g = nt - k0;  tD[i] = (t[k0+i] - t0_g) / Tc;
 *                sv = ucf_split_vector(tD), checked as ucf_drawdown_grid checks it;  rD = the distinct values (bitwise) of
 *                sqrt(dx dx + dy dy) / Lc over (location, well of g), ascending;  col[i][j] = index into rD (-1: well j is not
 *                in g);  tfac[i] = t[k0+i] / (t[k0+i] - t0_g).  Host code is compiled without FMA contraction: every
 *                operation above is rounded on its own.
 *   superposition field_superpose_kernel, one thread per output (k, i, z), z fastest; acc = +0.0, then for j = 0..nwell-1 in the
 *                caller's order, skipping wells whose group has k < k0:
 *                    s :  acc = acc + qw[j] * h_g[k-k0][col][z]        ds :  acc = acc + qw[j] * (tfac[k-k0] * dh_g[k-k0][col][z])
 *                (the library's dh is t dh/dt in the well's OWN time, so the second sum is t ds/dt), both times Hc at the end
 *                unless dimensionless != 0.  No scrubbing: non-finite values and the Wynn sentinel propagate as the plan
 *                produced them.  No atomics, fixed order: a call repeated gives the same bits.
 * A field is used by one host thread at a time; its buffers live on the device of the plan of its first ucf_field_drawdown. */
typedef struct ucf_field ucf_field;
/* Host arithmetic, no GPU.  UCF_ERR_BAD_ARGUMENT (ucf_last_error names the offender): a size < 1, a NULL array, a number that is
 * not finite, t not strictly increasing or not > 0, t0w < 0, qw == 0. */
int ucf_field_create(int nwell, const double* xw, const double* yw, const double* qw, const double* t0w,
                     int nloc, const double* x, const double* y, int nt, const double* t, ucf_field** out);
void ucf_field_destroy(ucf_field* field);
int ucf_field_group_count(const ucf_field* field, int* ngroups);
/* Host only: what group g launches under `plan` (arrays sized for the worst case; any output may be NULL).  nt_g may be 0
 * (no time of the field lies after the group's start: nothing is launched, nr_g, rD and col are still stated).
 * UCF_ERR_BAD_ARGUMENT: g outside 0..ngroups-1; a distance below the plan's rw -- the location is inside a well bore --
 * naming the (location, well) pair; nt_g * nr_g > 2^31 - 1; a split index the grid entry would refuse. */
int ucf_field_group(const ucf_field* field, const ucf_plan* plan, int g, int* k0, int* nt_g, double* tD /*[nt]*/, int* sv /*[nt]*/,
                    int* nr_g, double* rD /*[nloc*nwell]*/, int* col /*[nloc][nwell], -1 = well not in g*/,
                    double* tfac /*[nt]*/);
/* the same from a parameter set alone (no plan, no GPU): P is checked and non-dimensionalised as by ucf_nondimensionalise,
 * with its statuses; a plan made from P states the same arrays bit for bit */
int ucf_field_group_from_params(const ucf_field* field, const ucf_params* P, int g, int* k0, int* nt_g, double* tD, int* sv,
                                int* nr_g, double* rD, int* col, double* tfac);
/* s, ds [nt][nloc][nz]: drawdown and its logarithmic time derivative t ds/dt, dimensional (x Hc) unless dimensionless != 0;
 * an output at a time that no well's start precedes is +0.0.  zD = z / Lc and zLay are formed as in ucf_drawdown_multi.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT: NULL field, s, ds or z, nz < 1, a z that is not finite, what
 * ucf_field_group refuses for any group), then UCF_ERR_NO_DEVICE as for every compute entry.  h_g, dh_g [nt_g][nr_g][nz] of
 * every group live in buffers of the field that grow when needed and are kept: a repeated call of the same size allocates
 * nothing.  stats: summed over the groups. */
int ucf_field_drawdown(ucf_field* field, ucf_plan* plan, int nz, const double* z, int dimensionless,
                       double* s, double* ds /*[nt][nloc][nz]*/, ucf_stats* stats /*NULL ok*/);
/* device allocations made so far by the field (the plan's own workspaces count in ucf_plan_alloc_count; the scratch plan of
 * ucf_field_forecast counts once when it is made) */
long long ucf_field_alloc_count(const ucf_field* field);

/* ---- forecasts: what a fitted well field will do, how sure that is and which parameter it is sensitive to.  theta and cov are
 * those of ucf_fit_lm, passed as they are (cov in ln theta).  One call maps the field under the base parameter set and its
 * 2 npar log-perturbed neighbours, keeps all 1 + 2 npar superposed maps in device memory and forms there the central-difference
 * sensitivities d s / d ln theta_j and the first-order standard error sqrt(j' C j), for the drawdown and for its log-time
 * derivative; only the maps that are asked for cross the bus.
 *   sets         ucf_field_forecast_sets(&plan->P, ...): set 0 the base, set 1 + 2j / 2 + 2j parameter j up / down.
 *   plan         supplies the base parameters, the device, the numerical settings and the flavour; it is never modified.  The
 *                field owns ONE scratch plan on the plan's device (ucf_plan_create_on from set 0, the plan's mode, timing off),
 *                refreshed with ucf_plan_update for every set, kept for later calls, rebuilt only when ucf_plan_update refuses
 *                set 0 because the model or the numerical settings changed, destroyed with the field.
 *   per set      for k = 0 .. 2 npar in this order exactly what ucf_field_drawdown(field, plan of set k, nz, z, 0, ...) runs: the
 *                launch arrays that ucf_field_group_from_params(field, &sets[k], g, ...) states, one grid call per group, then
 *                field_superpose_kernel with that set's Hc into slot k of two device buffers [1 + 2 npar][nout],
 *                nout = nt nloc nz.  Slot k has the bits of ucf_field_drawdown on a fresh field and a fresh plan of sets[k].
 *                Outputs are always dimensional (Hc depends on Kr: a dimensionless sensitivity would be another quantity).
 *   combination  field_forecast_kernel, one thread per output e = (k, i, z), once on the s slots (a = s_all) and once on the ds
 *                slots (a = ds_all), every operation rounded on its own:
 *                    J_j = (a[1+2j][e] - a[2+2j][e]) / two_dlog,   two_dlog = 2.0 * dlog formed once on the host;
 *                    sens[j][e] = J_j;
 *                    var = +0.0;  for j = 0..npar-1:  inner = +0.0;  for k = 0..npar-1: inner = inner + cov[j][k] * J_k;
 *                                                     var = var + J_j * inner;
 *                    se[e] = (var < 0) ? +0.0 : sqrt(var)   (a NaN var stays NaN).
 *                nbad[0] (s) and nbad[1] (ds) count the outputs e for which any of the 1 + 2 npar slot values is not finite (a
 *                ballot per wave, one integer atomic per wave, no floating-point atomics: a call repeated gives the same bits).
 *                Nothing is scrubbed: non-finite values and the Wynn sentinel propagate as ucf_field_drawdown states.
 *   outputs      s, ds are slot 0, copied, not recomputed.  stats: summed over all sets and groups.
 * The slot buffers, the staging of sens / se and cov are buffers of the field, grown on demand and kept: a repeated call of the
 * same size allocates nothing.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_drawdown
 * checks; NULL ids, theta, s or ds; npar outside 1..UCF_FIT_MAX_PAR; dlog not positive and finite; se or dse without cov; a cov
 * entry that is not finite, cov[j][k] != cov[k][j], a negative cov[j][j]; (1 + 2 npar) nout beyond what one buffer may hold.
 * With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan", as in ucf_field_drawdown; with a plan the checks of
 * ucf_field_forecast_sets on plan->P run before any launch.  A set that ucf_plan_update refuses: that status, with the set and
 * the parameter moved in ucf_last_error. */
/* host only, no GPU: the 1 + 2 npar parameter sets a forecast evaluates.  sets[0] = ucf_fit_perturb(base, ids, theta);
 * sets[1 + 2j] / sets[2 + 2j] = the same with theta[j] * exp(+dlog) / theta[j] * exp(-dlog) (one product each; exactly the
 * sets ucf_fit_evaluate makes for one theta).  Checks: those of ucf_fit_perturb; theta positive and finite; dlog positive
 * and finite; every set valid as by ucf_nondimensionalise (its status, set and parameter named in ucf_last_error). */
int ucf_field_forecast_sets(const ucf_params* base, int npar, const int* ids, const double* theta, double dlog,
                            ucf_params* sets /*[1 + 2 npar]*/);
int ucf_field_forecast(ucf_field* field, ucf_plan* plan, int npar, const int* ids, const double* theta /*[npar]*/, double dlog,
                       const double* cov /*[npar][npar], in ln theta as ucf_fit_lm returns it; NULL: no standard error*/,
                       int nz, const double* z,
                       double* s, double* ds            /*[nt][nloc][nz], the base set; required*/,
                       double* sens, double* dsens      /*[npar][nt][nloc][nz]; NULL ok*/,
                       double* se, double* dse          /*[nt][nloc][nz]; NULL ok; not NULL needs cov*/,
                       double* s_all, double* ds_all    /*[1 + 2 npar][nt][nloc][nz]; NULL ok*/,
                       long long* nbad /*[2]: s, ds; NULL ok*/, ucf_stats* stats /*NULL ok*/);

/* ---- ensembles: a forecast linearises in ln theta around one point; over the width of a real posterior the drawdown of an
 * unconfined aquifer is not linear in ln Sy, ln kappa or ln Ss.  An ensemble call maps the field under nens parameter sets --
 * draws from cov (ucf_field_ensemble_draw), a Latin hypercube, the theta rows of a multi-start ucf_fit_lm: any source is legal
 * -- keeps all member maps of s and of ds in device memory and reduces them there over the member axis: per output the number of
 * finite members, their mean, standard deviation, extremes, order statistics (the 5 % / 50 % / 95 % maps) and the fraction of
 * members above a drawdown limit.  Only the maps that are asked for cross the bus.
 *   members      member m is ucf_fit_perturb(&plan->P, npar, ids, thetas[m]), m = 0 .. nens-1.
 *   plan         as in ucf_field_forecast: it supplies the base parameters, the device, the numerical settings and the flavour
 *                and is never modified; the members run on the field's ONE scratch plan (made from member 0 where the field
 *                has none that ucf_plan_update can refresh), refreshed with ucf_plan_update for every member.
 *   per member   for m = 0 .. nens-1 in this order exactly what ucf_field_forecast runs per set: the launch arrays that
 *                ucf_field_group_from_params(field, member m, g, ...) states, one grid call per group, then
 *                field_superpose_kernel with that member's Hc into slot m of two device buffers [nens][nout],
 *                nout = nt nloc nz.  Slot m has the bits of ucf_field_drawdown on a fresh field and a fresh plan of member m.
 *                Outputs are always dimensional.  Every member is validated, and the launch arrays of every member are formed
 *                and checked once, before the first launch (a refused member: that status, ucf_last_error names the member and
 *                its parameter values); they are formed again member by member for the launches, so that the host never holds
 *                the arrays of more than one member.
 *   reduction    two kernels, once on the s slots (a = the s slots) and once on the ds slots, every operation rounded on its
 *                own (no FMA contraction).  For output e: F = the members m with a[m][e] finite, in member order, n = |F|;
 *                members that are not finite take part in nothing below; the Wynn sentinel is finite and takes part.
 *                field_ensemble_moments_kernel, one thread per output:
 *                    nfin[e] = n;
 *                    acc = +0.0;  for m in F:  acc = acc + a[m][e];        mean[e] = acc / (double)n          (n = 0: NaN)
 *                    ss = +0.0;   for m in F:  d = a[m][e] - mean[e];  ss = ss + d * d;
 *                    sd[e] = sqrt(ss / (double)(n - 1))                                                      (n < 2: NaN)
 *                    min[e]: the first member of F, then replaced by every later v with v < min;              (n = 0: NaN)
 *                    max[e]: the first member of F, then replaced by every later v with v >= max;             (n = 0: NaN)
 *                            -- so min is x_0 and max is x_{n-1} of the order below, signs of zero included (the level 0
 *                            is x_0 + 0 * (x_1 - x_0): min in value, but a -0.0 becomes +0.0; the level 1 is max bit for bit);
 *                    pexc[l][e] = (double)#{m in F : a[m][e] > limit[l]} / (double)n, the comparison strict   (n = 0: NaN)
 *                field_ensemble_quantile_kernel: x_0 .. x_{n-1} are the values of F in ascending order, ties broken by member
 *                index: the value of member m has rank #{m' in F : v' < v or (v' == v and m' < m)} -- a stable sort; -0.0 and
 *                +0.0 are equal and keep their member order.  For level p = q[i]:
 *                    pos = p * (double)(n - 1);   k = floor(pos);
 *                    quant[i][e] = x_{n-1}                        where k >= n - 1,
 *                                  x_k + g * (x_{k+1} - x_k)      with g = pos - (double)k otherwise               (n = 0: NaN)
 *                (the `linear` rule of the textbooks, in one fixed operation order).
 *                nbad[0] (s) and nbad[1] (ds) count the outputs with n < nens (a ballot per wave, one integer atomic per wave, no
 *                floating-point atomics: a call repeated gives the same bits).  The payload of a NaN is not part of the contract.
 *   outputs      per map one ucf_ensemble_maps; every pointer may be NULL, and a NULL struct asks for nothing of that map (a
 *                NULL ds still evaluates the same members: the evaluators write dh beside every h).  pexc is formed from s.
 *                `all` [nens][nout] are the member maps as they stand.  stats: summed over all members and groups.
 * The slots, the statistics' staging and the levels / limits are buffers of the field, grown on demand, kept and counted in
 * ucf_field_alloc_count: a repeated call of the same or a smaller size allocates nothing.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_drawdown
 * checks (its s, ds aside); NULL ids or thetas; npar outside 1..UCF_FIT_MAX_PAR; nens outside 1..UCF_ENSEMBLE_MAX; a theta that
 * is not positive and finite (the member is named); nq or nlim outside 0..UCF_ENSEMBLE_MAX_Q, or positive with a NULL q /
 * limit; a q outside [0,1] or not finite; a limit that is not finite; quant asked for with nq = 0; pexc asked for with nlim = 0;
 * nens nout beyond what one buffer may hold.  With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan"; with a plan the
 * checks of ucf_fit_perturb and of every member run before any launch. */
#define UCF_ENSEMBLE_MAX 1024      /* members of one ensemble call */
#define UCF_ENSEMBLE_MAX_Q 16      /* quantile levels, and drawdown limits, per call */
/* per map (one for s, one for ds); every pointer may be NULL */
typedef struct ucf_ensemble_maps {
    double* mean;  double* sd;  double* min;  double* max;   /* [nout] */
    double* quant;                                           /* [nq][nout] */
    double* all;                                             /* [nens][nout]: the member maps */
    int*    nfin;                                            /* [nout]: members finite there */
} ucf_ensemble_maps;
int ucf_field_ensemble(ucf_field* field, ucf_plan* plan, int npar, const int* ids,
                       int nens, const double* thetas /*[nens][npar]*/,
                       int nz, const double* z,
                       int nq, const double* q /*[nq], each in [0,1]*/,
                       int nlim, const double* limit /*[nlim], dimensional drawdowns*/,
                       const ucf_ensemble_maps* s, const ucf_ensemble_maps* ds /*either may be NULL*/,
                       double* pexc /*[nlim][nout], of s; NULL ok*/,
                       long long* nbad /*[2]: s, ds; NULL ok*/, ucf_stats* stats /*NULL ok*/);
/* host only, no GPU: nens members drawn from the log-normal distribution that a fit states with theta and cov (in ln theta).
 *   member m     thetas[m][j] = theta[j] * exp(sum_{k<=j} L[j][k] zeta[m][k]),  the sum from +0.0 in ascending k, one product and
 *                one exp per value;
 *   L            the lower Cholesky factor of cov, L L' = cov, by the factorisation of ucf_fit_solve_step without damping: for
 *                j = 0 .. npar-1:  d = c_jj;  d = d - L_jk * L_jk, k = 0 .. j-1;  L_jj = sqrt(d);  then for i > j:  v = c_ij;
 *                v = v - L_ik * L_jk, k = 0 .. j-1;  L_ij = v / L_jj.  UCF_ERR_SINGULAR where a d is not positive and finite;
 *   zeta         standard normal deviates.  One splitmix64 stream for the whole call: state = seed; every draw is
 *                    state += 0x9E3779B97F4A7C15;  x = state;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                    x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  x = x ^ (x >> 31)           (64-bit unsigned, wrapping)
 *                and the uniform of a draw is u = ((double)(x >> 11) + 0.5) * 2^-53, in (0, 1).  Draws are taken in (member,
 *                parameter pair) order: for m = 0 .. nens-1, for i = 0, 2, 4 .. < npar: u1, then u2;
 *                    rad = sqrt(-2.0 * log(u1));   ang = 6.283185307179586 * u2   (the double nearest 2 pi);
 *                    zeta[m][i] = rad * cos(ang);   zeta[m][i+1] = rad * sin(ang), discarded where i + 1 = npar.
 * The checks are those of ucf_field_forecast on theta and cov (npar, NULL, theta positive and finite, cov finite, symmetric,
 * no negative variance) and nens >= 1. */
int ucf_field_ensemble_draw(int npar, const double* theta, const double* cov /*[npar][npar], ln theta*/,
                            int nens, unsigned long long seed, double* thetas /*[nens][npar]*/);
/* the two reduction kernels exactly as ucf_field_ensemble launches them (the same launchers, the same choice of tile), on caller
 * data a[nens][nout]: a is uploaded, the statistics that `out` asks for (out->all is ignored; out may be NULL), pexc [nlim][nout]
 * and nbad[0] are copied back.  The checks of ucf_field_ensemble on nens, nq, q, nlim, limit, quant and pexc, nout >= 1, then
 * UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_ensemble(int nens, long long nout, const double* a, int nq, const double* q,
                       int nlim, const double* limit, const ucf_ensemble_maps* out /*all ignored*/,
                       double* pexc, long long* nbad /*[1]*/);
/* ---- weighted ensembles.  The members of ucf_field_ensemble count equally, which is right for draws from a distribution and
 * wrong for a Latin hypercube or the rows of a multi-start fit: there every member is weighted by its likelihood against the
 * observations (importance sampling; GLUE with a formal likelihood).  Three host functions and one call:
 * ucf_fit_objective -> ucf_ensemble_likelihood_weights -> ucf_field_ensemble_weighted (which calls ucf_ensemble_quantise).
 *
 * host only, no GPU: integer weights.  wmax = the largest weight[m];
 *     r = weight[m] / wmax;   u[m] = (unsigned long long)floor(r * 4294967296.0 + 0.5)            (0 .. 2^32, u of wmax is 2^32)
 *     U = sum of u[m] (integer);   U2 = +0.0;  U2 = U2 + (double)u[m] * (double)u[m], m ascending;   *ess = (double)U * (double)U / U2
 * (Kish's effective sample size; ess NULL ok).  Why integers: every cumulative weight on the device is then a 64-bit integer sum
 * of at most 2^42 -- exact and independent of the order of summation -- so exactly one member is selected per quantile level
 * and a repeated call gives the same bits.  A member with u[m] = 0 (a weight below 2^-33 of the largest) IS NOT IN THE ENSEMBLE:
 * it takes part in no statistic and in no count.  With all weights equal every u is 2^32, and mean, sd and pexc below have the
 * bits of the unweighted ones.  UCF_ERR_BAD_ARGUMENT (the member named in ucf_last_error): nens outside 1..UCF_ENSEMBLE_MAX, a
 * NULL array, a weight that is negative or not finite, all weights 0. */
int ucf_ensemble_quantise(int nens, const double* weight, unsigned long long* u /*[nens]*/, double* ess /*NULL ok*/);
/* host only, no GPU: likelihood weights from the objectives of ucf_fit_objective.  Member m is admissible when phi[m] is finite
 * and nbad[m] == 0 (nbad NULL: the first test alone); best = the admissible member of least phi, the lowest index on a tie;
 *     weight[m] = exp(-0.5 * ((phi[m] - phi[best]) / s2))   each operation rounded on its own;   0 where m is not admissible;
 * weight[best] is exactly 1.  s2 is the variance factor: 1 where the fit's weights are true 1 / sigma, else an estimate such as
 * phi[best] / (nobs + nd - npar), the factor of cov in ucf_fit_lm.  best, nadmissible: NULL ok.  UCF_ERR_BAD_ARGUMENT: nens
 * outside 1..UCF_ENSEMBLE_MAX, NULL phi or weight, s2 not positive and finite, no admissible member. */
int ucf_ensemble_likelihood_weights(int nens, const double* phi, const int* nbad /*NULL ok*/, double s2,
                                    double* weight /*[nens]*/, int* best, int* nadmissible);
/* ucf_field_ensemble with a weight per member.  Everything is as stated there -- members, plan, per member, outputs, buffers,
 * validation of every member before the first launch -- except:
 *   weights      u = ucf_ensemble_quantise(weight), with its checks, after the other argument checks and before any GPU work;
 *                u [nens], *ess and *nlaunched (each NULL ok) are written then, with or without a device.
 *   per member   a member with u[m] = 0 is validated but NOT LAUNCHED; its slot in both buffers is filled with NaN bytes (0xff), so
 *                `all` is defined.  *nlaunched = the number of members with u > 0; stats sums over them.  The scratch plan is
 *                made from, or refreshed to, the first launched member.  A launched slot has the bits of ucf_field_drawdown on
 *                a fresh field and a fresh plan of that member.
 *   reduction    u [nens] is a buffer of the field (grown on demand, kept, counted in ucf_field_alloc_count), read by the kernels
 *                at wave-uniform addresses.  For output e: F = the members m with a[m][e] finite AND u[m] > 0, in member order;
 *                n = |F|;  U = sum_F u[m], a 64-bit integer sum.  Every operation is rounded on its own.
 *                field_ensemble_wmoments_kernel, one thread per output:
 *                    nfin[e] = n;
 *                    acc = +0.0;  for m in F:  acc = acc + (double)u[m] * a[m][e];     mean[e] = acc / (double)U      (n = 0: NaN)
 *                    U2 = +0.0;   for m in F:  U2 = U2 + (double)u[m] * (double)u[m];
 *                    ss = +0.0;   for m in F:  d = a[m][e] - mean[e];  ss = ss + (double)u[m] * (d * d);
 *                    den = (double)U - U2 / (double)U;
 *                    sd[e] = sqrt(ss / den)      (NaN where n < 2 or den is not positive) -- the reliability-weights estimator;
 *                            with equal weights den = (n - 1) 2^32 exactly;
 *                    min[e], max[e]: the compare-and-replace rules of ucf_field_ensemble, over F;
 *                    pexc[l][e] = (double)(sum of u[m] over the m in F with a[m][e] > limit[l]) / (double)U, an integer sum, the
 *                            comparison strict                                                                    (n = 0: NaN)
 *                field_ensemble_wquantile_kernel: the inverse of the weighted empirical distribution function (the rule of
 *                numpy's quantile(weights=, method="inverted_cdf"); the cumulative-likelihood rule of GLUE).  In the stable
 *                order of ucf_field_ensemble (ascending, ties in member order) member m has in front of it the weight
 *                    E_m = sum of u[m'] over the m' in F with v' < v or (v' == v and m' < m)                  (an integer sum)
 *                and for level p = q[i]:   tgt = p * (double)U   (one rounded product);
 *                    quant[i][e] = the value of the member with (double)E_m < tgt && tgt <= (double)(E_m + u[m]);
 *                                  where tgt == 0 the member with E_m == 0                                        (n = 0: NaN)
 *                No interpolation.  The intervals (E_m, E_m + u[m]] partition (0, U]: exactly one member matches.  Tied members
 *                have one value, so the order among them only decides which of -0.0 and +0.0 is returned.  With equal weights
 *                the result is the order statistic of index ceil(p n) - 1 (index 0 at p = 0).
 *                nbad[0] (s), nbad[1] (ds) count the outputs with n < the number of members with u > 0.
 * ucf_field_ensemble itself runs what it ran before: its kernels take no weights. */
int ucf_field_ensemble_weighted(ucf_field* field, ucf_plan* plan, int npar, const int* ids,
                                int nens, const double* thetas /*[nens][npar]*/, const double* weight /*[nens]*/,
                                int nz, const double* z, int nq, const double* q, int nlim, const double* limit,
                                const ucf_ensemble_maps* s, const ucf_ensemble_maps* ds, double* pexc,
                                long long* nbad /*[2]*/, ucf_stats* stats,
                                unsigned long long* u /*[nens]; NULL ok*/, double* ess /*NULL ok*/, int* nlaunched /*NULL ok*/);
/* the two weighted reduction kernels exactly as ucf_field_ensemble_weighted launches them, on caller data a[nens][nout] and
 * caller weights: the twin of ucf_debug_ensemble.  Its checks, then those of ucf_ensemble_quantise, then UCF_ERR_NO_DEVICE
 * without a device. */
int ucf_debug_ensemble_weighted(int nens, long long nout, const double* a, const double* weight /*[nens]*/,
                                int nq, const double* q, int nlim, const double* limit,
                                const ucf_ensemble_maps* out /*all ignored*/, double* pexc, long long* nbad /*[1]*/);
/* ---- data worth: where the next observation well has to go, and how long it has to be read, so that a forecast becomes sure
 * (first-order data-worth analysis, the PREDUNC family of PEST).  One call evaluates the slots of ucf_field_forecast and keeps
 * them on the device; field_worth_kernel conditions the fit's covariance on the readings that a candidate well at (location i,
 * depth z) would deliver and reports the variance left on up to UCF_WORTH_MAX_TGT forecast targets; a greedy loop picks a
 * network of up to UCF_WORTH_MAX_PICK wells on the resident slots, one small launch per pick and no evaluation again.
 *   notation     nout = nt nloc nz, output e = (k nloc + i) nz + z; candidate c = i nz + z, ncand = nloc nz, so e = k ncand + c.
 *                a_s, a_d [1 + 2 npar][nout]: the slots of s and of ds exactly as ucf_field_forecast forms them (the same sets,
 *                plan, scratch plan and launch sequence), dimensional.  two_dlog = 2.0 * dlog, formed once on the host.  Every
 *                operation below is rounded on its own (no FMA contraction), on the device and on the host.
 *   data         a candidate well records the drawdown at every time k with tsel[k] != 0 (NULL tsel: every time), each reading
 *                with standard deviation sigma_s: ws = 1.0 / sigma_s; where sigma_d > 0 also the log-time derivative, wd =
 *                1.0 / sigma_d.  sigma_d == 0: no derivative data, wd = 0, and a_d is read for targets only.
 *   prior        cov in ln theta as ucf_fit_lm returns it, factorised once on the host: cov = F F', F the lower Cholesky factor
 *                that ucf_field_ensemble_draw states, its upper triangle +0.0 (UCF_ERR_SINGULAR where a pivot is not positive
 *                and finite).  After a pick F is a general square matrix: the kernel takes a general F [npar][npar].
 *   kernel       field_worth_kernel<npar>, one thread per candidate c:
 *                    B_jj = 1.0, B_ij = +0.0 (i > j; the lower triangle only);  nused = 0
 *                    for k = 0 .. nt-1 ascending with tsel[k] != 0:
 *                      for (a, w) = (a_s, ws), then (a_d, wd), only where w > 0:
 *                        J_j = (a[1+2j][e] - a[2+2j][e]) / two_dlog,  j = 0 .. npar-1
 *                        if any of these 2 npar slot values is not finite: the datum is skipped
 *                        nused = nused + 1
 *                        g_j = +0.0;  g_j = g_j + F[i][j] * J_i,  i = 0 .. npar-1 ascending                      (g = F' J)
 *                        wg_j = w * g_j;      B_ij = B_ij + wg_i * wg_j,  i >= j
 *                    B = L D L' without square roots, for j = 0 .. npar-1:
 *                        v = B_jj;  v = v - (l_jk * l_jk) * d_k, k = 0 .. j-1;   d_j = v
 *                        for i > j:  v = B_ij;  v = v - (l_ik * l_jk) * d_k, k = 0 .. j-1;   l_ij = v / d_j
 *                    per target t = 0 .. ntgt-1:
 *                        v = +0.0;  for j ascending:  y_j = A[t][j];  y_j = y_j - l_jk * y_k, k = 0 .. j-1;  v = v + (y_j * y_j) / d_j
 *                        post[t][c] = v, NaN where a d_j is not positive and finite (in exact arithmetic every d_j >= 1; overflow
 *                        breaks that, and rounding where kappa_2(B) exceeds 2^53, as with a Wynn sentinel among the readings)
 *                    crit[c] = +0.0;  crit[c] = crit[c] + tw[t] * post[t][c],  t ascending;       nused_out[c] = nused
 *                post[t][c] is the variance of target t after the candidate's data, j_t' (C^-1 + sum w^2 j j')^-1 j_t, formed as
 *                a_t' B^-1 a_t with B = I + sum (w F'j)(w F'j)': cov is never inverted and B has no eigenvalue below 1.  Slot 0 is
 *                not read.  The Wynn sentinel is finite and takes part, as everywhere else.  No atomics: a call repeated gives the
 *                same bits.
 *   targets      target t is tgt[t] = (kind 0 = s | 1 = ds, k, i, z), an output of the same map.  Per call its 2 npar slot values
 *                are fetched once (field_gather_kernel, out[n] = a[idx[n]]), J as above; per round on the host
 *                    A[t][j] = +0.0;  A[t][j] = A[t][j] + F[i][j] * J_i, i ascending;
 *                    prior[t] = +0.0;  prior[t] = prior[t] + A[t][j] * A[t][j], j ascending.
 *                A target with a slot value that is not finite: A[t][.] = NaN, so its prior, its post and crit are NaN; the call
 *                still returns UCF_OK.  tw NULL: every weight 1.
 *   pick         round r copies crit back; pick[r] = the candidate of least crit among those with cmask[c] != 0 (NULL cmask: all),
 *                not picked in an earlier round, crit finite; the lowest index on a tie.  None: pick[r] = -1, the later rounds
 *                are not run, their rows of prior / post / crit are NaN and their pick entries -1.
 *   conditioning after a pick the column of the picked candidate -- 2 npar nt slot values per map, through the same gather --
 *                gives the rows (J, w) of its used data in kernel order, F = ucf_worth_condition(F, rows), and the next round
 *                runs the kernel with that F.  cov_post = F F' of the last factor: after the last pick made (of the prior's factor
 *                where no pick was made).  nused does not depend on the round.
 * post, crit, nused and the small arrays are buffers of the field, grown on demand, kept and counted in ucf_field_alloc_count: a
 * repeated call of the same size allocates nothing.  Every output may be NULL.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_forecast
 * checks on field, nz, z, npar, ids, theta, dlog and the size of the slots; a NULL cov, and what the forecast checks on cov; a cov
 * that is not positive definite (UCF_ERR_SINGULAR); sigma_s not positive and finite; sigma_d negative or not finite; ntgt outside
 * 1..UCF_WORTH_MAX_TGT; a NULL tgt; a target kind, k, i or z out of range; a tw that is negative or not finite; npick outside
 * 1..UCF_WORTH_MAX_PICK; a tsel that selects no time.  With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan". */
#define UCF_WORTH_MAX_TGT 16
#define UCF_WORTH_MAX_PICK 16
int ucf_field_worth(ucf_field* field, ucf_plan* plan, int npar, const int* ids, const double* theta, double dlog,
                    const double* cov /*[npar][npar], ln theta; required*/, int nz, const double* z,
                    double sigma_s, double sigma_d, const int* tsel /*[nt], NULL ok*/,
                    int ntgt, const int* tgt /*[ntgt][4]: kind, k, i, z*/, const double* tw /*[ntgt], NULL = 1*/,
                    int npick, const int* cmask /*[ncand], NULL ok*/,
                    double* prior /*[npick][ntgt]*/, double* post /*[npick][ntgt][ncand]*/,
                    double* crit /*[npick][ncand]*/, int* nused /*[ncand]*/, int* pick /*[npick]*/,
                    double* cov_post /*[npar][npar]: after the last pick made*/, ucf_stats* stats);
/* host only, no GPU: the factor of the covariance after nrow readings, row r with sensitivities J[r][.] (in ln theta) and weight
 * w[r] = 1 / sigma.  B, l and d are formed from the rows, in the order given, by the statements of the kernel above (every row is
 * used); then per entry
 *     X[i][j] = F[i][j];  X[i][j] = X[i][j] - X[i][k] * l[j][k], k = 0 .. j-1 ascending     (X L' = F);
 *     F_out[i][j] = X[i][j] / sqrt(d_j);
 *     cov_out[i][j] = +0.0;  cov_out[i][j] = cov_out[i][j] + F_out[i][k] * F_out[j][k], k ascending          (cov_out NULL ok)
 * so that F_out F_out' = F B^-1 F' = (C^-1 + sum w^2 j j')^-1 with C = F F'.  F general [npar][npar]; F_out may be F.  nrow = 0 is
 * legal and returns F (J, w may then be NULL).  UCF_ERR_BAD_ARGUMENT: npar outside 1..UCF_FIT_MAX_PAR, a NULL array, nrow < 0, a
 * number that is not finite, a negative w; UCF_ERR_SINGULAR where a d_j is not positive and finite (as in the kernel). */
int ucf_worth_condition(int npar, const double* F /*[npar][npar]*/, int nrow, const double* J /*[nrow][npar]*/,
                        const double* w /*[nrow]*/, double* F_out /*[npar][npar]*/, double* cov_out /*[npar][npar]; NULL ok*/);
/* field_worth_kernel exactly as ucf_field_worth launches it (the same launcher), once, on caller data a_s, a_d
 * [1 + 2 npar][nt][ncand] (a_d NULL ok where wd == 0), F [npar][npar], A [ntgt][npar], tw [ntgt] (NULL = 1), tsel [nt] (NULL = all):
 * the twin of ucf_debug_ensemble.  post [ntgt][ncand], crit [ncand], nused [ncand]: each NULL ok.  The slot values and A may hold
 * anything.  UCF_ERR_BAD_ARGUMENT: npar outside 1..UCF_FIT_MAX_PAR, nt or ncand < 1, (1 + 2 npar) nt ncand beyond 2^31-1 values, a
 * NULL a_s, F or A, a NULL a_d with wd > 0, two_dlog not positive and finite, an F entry that is not finite, ws not positive and
 * finite, wd negative or not finite, ntgt outside 1..UCF_WORTH_MAX_TGT, a tw that is negative or not finite, a tsel that selects
 * no time.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_field_worth(int npar, int nt, int ncand, const double* a_s, const double* a_d, double two_dlog, const double* F,
                          double ws, double wd, const int* tsel, int ntgt, const double* A, const double* tw,
                          double* post, double* crit, int* nused);
/* ---- well-field yield: how much may these wells pump before a permitted drawdown is exceeded somewhere, and how sure is that
 * under the posterior.  Drawdown is linear in the rates: with the group results of a member on the device its map is an affine
 * function of any rate multipliers, and the largest admissible multiplier is a ratio test over the constrained outputs.  One
 * ensemble's worth of evaluator launches answers every rate pattern at once.
 *   controls     a control is a set of wells whose rates move together (a real well with its images).  ctl[j], one per well of the
 *                field, in -1 .. nctl-1: -1 = the well is fixed and is not scaled; every control 0 .. nctl-1 owns at least one well;
 *                nctl in 1..UCF_YIELD_MAX_CTL.
 *   patterns     x [npat][nctl]: multipliers on the wells' qw, every entry finite (negative and zero are legal), npat in
 *                1..UCF_YIELD_MAX_PAT.  Pattern p at scale lam pumps well j of control c at lam * x[p][c] * qw[j] (in units of the
 *                plan's Q); a fixed well pumps qw[j].
 *   limits       limit [nt][nloc][nz]: dimensional drawdowns; +inf = the output is unconstrained; NaN and -inf are refused.  con =
 *                the ascending list of the output indices e = (k nloc + iloc) nz + z with a finite limit, ncon >= 1 of them.
 *   smax         the largest scale of interest (the pump capacity), positive and finite: it keeps every result finite.
 *   members      those of ucf_field_ensemble; with weight != NULL u = ucf_ensemble_quantise(weight) as in
 *                ucf_field_ensemble_weighted: a member with u[m] = 0 is validated but not launched, its rows of R are NaN bytes
 *                (0xff) and through R its rows of y, fe, hi, lo are NaN; u, *ess, *nlaunched are written with or without a device.
 *   response     per member m exactly what ucf_field_ensemble runs per member up to the superposition -- the same launch arrays,
 *                group calls, scratch plan and order -- then, in place of field_superpose_kernel, field_response_kernel: one thread
 *                per (slot c = 0 .. nctl, constrained output i), e = con[i] = (k, iloc, z):
 *                    acc = +0.0
 *                    for j = 0 .. nwell-1 in the caller's order, only the wells with ctl[j] == c (slot nctl: ctl[j] == -1) and
 *                        k >= k0_j:   acc = acc + q_j * h[at]                     (the index `at` of field_superpose_kernel)
 *                    R[m][c][i] = acc * Hc_m
 *                every operation rounded on its own; the drawdown only (dh is not read).  With one control that holds every well
 *                R[m][0][i] has the bits of the member map of ucf_field_ensemble at con[i].
 *   ratio test   field_yield_kernel<nctl>, for member m and pattern p over i = 0 .. ncon-1, with b = R[m][nctl][i], r_c = R[m][c][i]:
 *                    hi = smax;  lo = +0.0;  dead = 0;  bind = -1
 *                    room = limit[con[i]] - b
 *                    D = +0.0;  D = D + x[p][c] * r_c,  c ascending                  (one product, one sum, each rounded)
 *                    D > 0:   cand = room / D;  if cand < hi, or (cand == hi and bind == -1):  hi = cand, bind = con[i]
 *                    D < 0:   cand = room / D;  if cand > lo:  lo = cand
 *                    D == 0:  if room < 0:  dead = 1
 *                  after the loop:
 *                    feas = (dead == 0 && lo <= hi);    y[m][p] = feas ? hi : +0.0;    fe[m][p] = feas ? 1.0 : 0.0
 *                The result is defined without order: hi is the least candidate (smax where none is below it), lo the greatest, bind
 *                the lowest con[i] among the outputs whose candidate equals hi under ==, -1 where no candidate is <= smax.  A
 *                candidate or a D that is NaN passes no comparison and changes nothing.  The sign of a zero in hi, lo and y is not
 *                part of the contract.  A negative hi (room < 0 with D > 0) is below lo: not feasible.  Member m is valid when
 *                every one of its (nctl + 1) ncon slot values is finite (the Wynn sentinel is finite and takes part, as everywhere);
 *                for an invalid member y, fe, hi, lo are NaN, bind is -1 and dead is 0 for every pattern.  *nbad = the launched
 *                members that are invalid, each counted once (one integer atomic per member).  No floating-point atomics: a call
 *                repeated gives the same bits.
 *   reduction    no kernel of its own: the reduction of ucf_field_ensemble (of ucf_field_ensemble_weighted with weights) with
 *                nout = npat, on y for ystat (mean, sd, min, max, quant at q, nfin; all = y) and for pexc [nlev][npat], the share
 *                of members whose admissible scale exceeds level[l]; on fe with the single limit 0.5 for pfeas [npat], the share of
 *                valid members that admit any scale.  Reading a quantile: quant at level q is the scale that a share 1 - q of the
 *                ensemble admits -- the yield at reliability 1 - q; the 5 % map is the scale that 95 % of the members admit.
 *   outputs      hi, lo (double), bind, dead (int) [nens][npat]; resp [nens][nctl + 1][ncon] = R; con [nout] with its first *ncon
 *                entries filled, and *ncon: written by the checks, with or without a device; stats summed over the launched
 *                members and groups.  Every output may be NULL.
 * R, y, fe, hi, lo, bind, dead, con, ctl, x and the limits are buffers of the field, grown on demand, kept and counted in
 * ucf_field_alloc_count: a repeated call of the same or a smaller size allocates nothing.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything
 * ucf_field_ensemble_weighted checks on field, nz, z, npar, ids, nens, thetas, nq, q, nlev, level (as its nlim, limit), quant and
 * pexc, and on weight where it is not NULL; nctl outside 1..UCF_YIELD_MAX_CTL; a NULL ctl, x or limit; a ctl outside -1 .. nctl-1;
 * a control without a well; npat outside 1..UCF_YIELD_MAX_PAT; an x that is not finite; a limit that is NaN or -inf; no finite
 * limit at all; nt nloc nz beyond 2^31-1 (con and bind are ints); smax not positive and finite; nens (nctl + 1) ncon beyond what
 * one buffer may hold.  With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan". */
#define UCF_YIELD_MAX_CTL 8        /* controls of one ucf_field_yield */
#define UCF_YIELD_MAX_PAT 4096     /* rate patterns of one ucf_field_yield */
#define UCF_YIELD_PAT_TILE 8       /* patterns per workgroup of field_yield_kernel */
int ucf_field_yield(ucf_field* field, ucf_plan* plan, int npar, const int* ids,
                    int nens, const double* thetas /*[nens][npar]*/, const double* weight /*[nens]; NULL ok: unweighted*/,
                    int nz, const double* z,
                    int nctl, const int* ctl /*[nwell]*/, int npat, const double* x /*[npat][nctl]*/,
                    const double* limit /*[nt][nloc][nz]*/, double smax,
                    int nq, const double* q /*[nq]*/, int nlev, const double* level /*[nlev], scales*/,
                    const ucf_ensemble_maps* ystat /*of y, nout = npat*/, double* pexc /*[nlev][npat]*/, double* pfeas /*[npat]*/,
                    double* hi, double* lo, int* bind, int* dead /*[nens][npat] each*/,
                    double* resp /*[nens][nctl+1][ncon]*/, int* con /*[nout], first *ncon filled*/, int* ncon,
                    long long* nbad /*[1]*/, ucf_stats* stats,
                    unsigned long long* u /*[nens]*/, double* ess, int* nlaunched);
/* field_yield_kernel exactly as ucf_field_yield launches it (the same launcher), once, on caller data R [nens][nctl + 1][ncon], x
 * [npat][nctl], limit_con [ncon] (the limit of constrained output i) and con [ncon]: the twin of ucf_debug_field_worth.  y, fe,
 * hi, lo, bind, dead [nens][npat] and nbad [1] (every invalid member): each NULL ok.  R may hold anything.
 * UCF_ERR_BAD_ARGUMENT: nctl outside 1..UCF_YIELD_MAX_CTL, nens outside 1..UCF_ENSEMBLE_MAX, ncon < 1, npat outside
 * 1..UCF_YIELD_MAX_PAT, nens (nctl + 1) ncon beyond 2^31-1 values, a NULL R, x, limit_con or con, an x or a limit_con that is not
 * finite, a con that is negative or does not ascend strictly, smax not positive and finite.  Then UCF_ERR_NO_DEVICE without a
 * device. */
int ucf_debug_field_yield(int nctl, int nens, int ncon, int npat, const double* R, const double* x, const double* limit_con,
                          const int* con, double smax, double* y, double* fe, double* hi, double* lo, int* bind, int* dead,
                          long long* nbad /*[1]*/);
/* ---- well-field allocation: HOW should the abstraction be distributed over the wells so that the total is largest and every
 * receptor stays within its limit, which receptors limit that optimum, what would relaxing a limit buy, and how sure is that
 * under the posterior (the response-matrix method, Gorelick 1983).  Drawdown is linear in the rates, so per member the question is a
 * linear programme in at most UCF_YIELD_MAX_CTL unknowns; its data are the response slots R that the member loop of
 * ucf_field_yield leaves on the device.  Controls, ctl, the fixed-well slot, con, limit and R are exactly those of ucf_field_yield.
 *   programme    per member m and objective o, in the multipliers x_c (c = 0 .. nctl-1) on the qw of the wells of control c -- what
 *                a pattern of ucf_field_yield is at scale 1:
 *                    maximise    g = sum_c w[o][c] x_c
 *                    subject to  R[m][nctl][i] + sum_c x_c R[m][c][i] <= limit[con[i]]      i = 0 .. ncon-1
 *                                0 <= x_c <= xmax[c]
 *                w [nobj][nctl] finite (negative and zero are legal), nobj in 1..UCF_ALLOC_MAX_OBJ; xmax [nctl] positive and finite:
 *                the pump capacities, which keep every programme bounded.
 *   constraints  every constraint is a row a . x <= beta with an id, used for every tie-break and in every output:
 *                    id c          (c = 0 .. nctl-1)   lower bound   a = -e_c (-1.0 at c, +0.0 elsewhere),  beta = +0.0
 *                    id nctl + c                       upper bound   a = +e_c (1.0 at c, +0.0 elsewhere),   beta = xmax[c]
 *                    id 2 nctl + i (i = 0 .. ncon-1)   output row    a_c = R[m][c][i],   beta = room_i = limit[con[i]] - R[m][nctl][i]
 *   solve(A, b)  the nctl x nctl systems: Gaussian elimination with partial pivoting on copies of A and b, n = nctl:
 *                    for col = 0 .. n-1:
 *                        piv = the row r in col .. n-1 with the largest |A[r][col]|, the lowest r among equals (a later row wins only
 *                              with a magnitude that is greater under >)
 *                        a pivot magnitude that is zero, NaN or infinite ends the programme: status NUMERIC
 *                        rows piv and col of A and b are exchanged
 *                        for r = col+1 .. n-1:   f = A[r][col] / A[col][col]
 *                                                A[r][c] = A[r][c] - f * A[col][c],  c = col+1 .. n-1;     b[r] = b[r] - f * b[col]
 *                    for r = n-1 .. 0:   s = b[r];   s = s - A[r][c] * y[c],  c = r+1 .. n-1 ascending;   y[r] = s / A[r][r]
 *                every product, difference and quotient rounded on its own.
 *   algorithm    a primal active-set simplex from the vertex x = +0.0, working set W[s] = s (the lower bounds), s = 0 .. nctl-1:
 *                    valid:   every one of the (nctl + 1) ncon slot values of the member is finite; else status INVALID
 *                    start:   if any room_i < 0 the fixed wells alone exceed a limit: status INFEASIBLE_AT_ZERO, nothing is solved
 *                             (injection, a negative x, as a repair is out of scope)
 *                    iters = 0;  repeat at most maxit times (maxit in 1..UCF_ALLOC_MAX_ITER):
 *                      1. B = the rows of W, row s = a of W[s].  lambda = solve(B', w[o]).  No lambda_s < 0: status OPTIMAL, stop.
 *                      2. k = the slot s with the lowest id W[s] among those with lambda_s < 0 (Bland's rule).
 *                      3. d = solve(B, -e_k), the right-hand side -1.0 at k and +0.0 elsewhere.
 *                      4. over every constraint j that is not in W:
 *                             output row:   D = +0.0, S = +0.0, ax = +0.0;  for c ascending:  p = a_c * d_c;  D = D + p;
 *                                           S = S + |p|;  ax = ax + a_c * x_c;            slack = room_i - ax
 *                             lower bound:  D = -d_c, slack = x_c;       upper bound:  D = d_c, slack = xmax[c] - x_c;
 *                                           S = dmax = the largest |d_c| (any order: it is a maximum)
 *                             D > UCF_ALLOC_DTOL * S:  if slack < 0 (rounding):  slack = +0.0;     cand = slack / D
 *                         (step, enter) = the lexicographic minimum of (cand, id j) over the constraints that pass the test on D,
 *                         defined without order as hi and bind of the ratio test are: the least cand, the lowest id among those
 *                         that attain it under ==.  A cand, a D or an S that is NaN passes no comparison.  No candidate: status
 *                         NUMERIC, stop.  Why D > 0 alone does not do: the twin of a working row (the same drawdown at two depths
 *                         of a fully penetrating well) and a row through the vertex along the edge have D = 0 exactly, computed as
 *                         rounding noise of either sign; a positive one has slack 0, wins the test and makes B singular.  The
 *                         rounding of D is at most nctl 2^-53 S (nctl products and sums of terms bounded by S), the error that d
 *                         inherits from its solve is of the order of cond(B) 2^-53 S; UCF_ALLOC_DTOL = 2^-40 lies 2^10 above the
 *                         first and still far below any D that moves the vertex by a representable amount.  With S = 0 the test is
 *                         D > 0.
 *                      5. W[k] = enter;  x = solve(B, beta) on the rows and right-hand sides of the new W (never x + step d);
 *                         iters = iters + 1.
 *                    the maxit pivots are spent and step 1 has not said OPTIMAL: status ITERATION_CAP (a programme that needs
 *                    exactly maxit pivots ends so: optimality is tested before a pivot, not after the last)
 *   polish       at OPTIMAL, before anything is written: x and g in double-double (a value is hi + lo), so that what is returned
 *                is the vertex of the final working set and its value rounded once and not the sum of the roundings of one
 *                elimination.  two_sum(a, b) = (s, err):  s = a + b;  bb = s - a;  err = (a - (s - bb)) + (b - bb)   (exact).
 *                add((h, l), (p, e)):  (s, t) = two_sum(h, p);  low = l + (t + e);  h = s + low;  l = low - (h - s).
 *                addprod((h, l), sign, a, (xh, xl)):  p = a * xh;  e = fma(a, xh, -p) (the exact error of p; the one fused
 *                operation of the contract);  add((h, l), (sign * p, sign * (e + a * xl))).
 *                    xl = +0.0;  twice:
 *                        per slot s:  (h, l) = (beta, +0.0) of a bound, two_sum(limit[con[i]], -R[m][nctl][i]) of an output row;
 *                                     addprod((h, l), -1.0, B[s][c], (x_c, xl_c)), c ascending;     r_s = h
 *                        e = solve(B, r);     (x_c, xl_c) = add((x_c, xl_c), (e_c, +0.0))
 *                    (g, gl) = (+0.0, +0.0);  addprod((g, gl), 1.0, w[o][c], (x_c, xl_c)), c ascending
 *                x (the high parts) and g are what is returned, and x is what the reliability stage scales.
 *   outputs      per (m, o), [nens][nobj] leading: x [nctl] and g, both as polished; status (UCF_ALLOC_*) and
 *                iters, the pivots made; work [nctl], the ids of W at the optimum, ascending -- the receptors (and capacities) that
 *                limit the well field --, and lam [nctl], the lambda of step 1 of the same constraints: the shadow prices, the gain
 *                in g per unit of relaxed limit.  With a status other than OPTIMAL x, g and lam are NaN and work is -1; for an
 *                invalid member iters is 0.  *nbad = the launched members that are invalid, each counted once (one integer atomic
 *                per member).  A member of weight 0 is not launched (its R is NaN bytes): its outputs are those of an invalid member
 *                and it is not counted.  No floating-point atomics: a call repeated gives the same bits.
 *   kernel       field_allocate_kernel<nctl>, one workgroup of 256 threads per (m, o).  Steps 1 to 3 and 5 are done by one thread
 *                on LDS; step 4 is shared by the 256 threads, combined by a wave butterfly on (cand, id) and through LDS.  A
 *                member's R is reread once per iteration.  ucf_allocate_solve is the same arithmetic on the host, bit for bit.
 *   reliability  optional, in the same call, while R is on the device; skipped when quant, value, best and best_x are all NULL;
 *                needs nq >= 1 and nens nobj <= UCF_YIELD_MAX_PAT.  The optima become rate patterns: pattern p = m nobj + o is
 *                x of (m, o), all +0.0 where the status is not OPTIMAL.  They run through field_yield_kernel as in
 *                ucf_field_yield with smax = 1 (candidates are only ever scaled DOWN and stay within xmax); the member reduction
 *                of ucf_field_ensemble (weighted with weights) on y [nens][npat] gives quant [nq][npat]: quant[q][p] is the scale
 *                of candidate p that a share 1 - q of the members admits.  On the host (ucf_allocate_select):
 *                    value[q][p] = quant[q][p] * g[p]                                   (one product; NaN propagates)
 *                    best[q][o]  = the p = m nobj + o with the largest value[q][p] under >, m ascending: the lowest p wins ties,
 *                                  a NaN value is never chosen, -1 where none is
 *                    best_x[q][o][c] = quant[q][best] * x[best][c]                      (NaN where best is -1)
 *                What this is: a FEASIBLE allocation at reliability 1 - q, chosen among the nens scenario optima and scaled down
 *                -- a lower bound on the chance-constrained optimum, not that optimum.  gquant [nq][nobj], the quantiles of the
 *                per-member g (the same reduction on g, members without an optimum left out), is the wait-and-see figure above it:
 *                what a manager who knew the member could pump.
 * x, g, lam, status, iters and work are buffers of the field like those of ucf_field_yield, and so are the y, hi, lo, bind, dead
 * of the reliability stage: a repeated call of the same or a smaller size allocates nothing.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_yield checks on
 * field, nz, z, npar, ids, nens, thetas, nq, q, weight, nctl, ctl and limit (nq may be 0 unless the reliability stage or gquant is
 * asked for); nobj outside 1..UCF_ALLOC_MAX_OBJ; a NULL w or xmax; a w that is not finite; an xmax that is not positive and finite;
 * maxit outside 1..UCF_ALLOC_MAX_ITER; the reliability stage with nens nobj > UCF_YIELD_MAX_PAT. */
#define UCF_ALLOC_MAX_OBJ 8        /* objectives of one ucf_field_allocate */
#define UCF_ALLOC_MAX_ITER 256     /* the largest maxit */
#define UCF_ALLOC_DTOL 0x1p-40     /* step 4: a D that is not above this times its scale S is zero up to rounding */
#define UCF_ALLOC_INVALID (-1)
#define UCF_ALLOC_OPTIMAL 0
#define UCF_ALLOC_ITERATION_CAP 1
#define UCF_ALLOC_INFEASIBLE_AT_ZERO 2
#define UCF_ALLOC_NUMERIC 3
int ucf_field_allocate(ucf_field* field, ucf_plan* plan, int npar, const int* ids,
                       int nens, const double* thetas /*[nens][npar]*/, const double* weight /*[nens]; NULL ok: unweighted*/,
                       int nz, const double* z,
                       int nctl, const int* ctl /*[nwell]*/,
                       int nobj, const double* w /*[nobj][nctl]*/, const double* xmax /*[nctl]*/, int maxit,
                       const double* limit /*[nt][nloc][nz]*/,
                       double* x /*[nens][nobj][nctl]*/, double* g /*[nens][nobj]*/, int* status, int* iters /*[nens][nobj]*/,
                       int* work /*[nens][nobj][nctl]*/, double* lam /*[nens][nobj][nctl]*/,
                       int nq, const double* q /*[nq]*/,
                       double* quant /*[nq][nens nobj]*/, double* value /*[nq][nens nobj]*/, int* best /*[nq][nobj]*/,
                       double* best_x /*[nq][nobj][nctl]*/, double* gquant /*[nq][nobj]*/,
                       double* resp /*[nens][nctl+1][ncon]*/, int* con /*[nout], first *ncon filled*/, int* ncon,
                       long long* nbad /*[1]*/, ucf_stats* stats,
                       unsigned long long* u /*[nens]*/, double* ess, int* nlaunched);
/* The arithmetic of field_allocate_kernel for ONE member on host arrays, no GPU: R_m [nctl + 1][ncon] (may hold anything),
 * limit_con [ncon] (the limit of constrained output i), w [nobj][nctl], xmax [nctl]; x, lam [nobj][nctl], g [nobj], status, iters
 * [nobj], work [nobj][nctl]: each NULL ok.  The kernel is held to it bit for bit.  UCF_ERR_BAD_ARGUMENT as ucf_debug_field_allocate
 * on the arguments the two share. */
int ucf_allocate_solve(int nctl, int ncon, const double* R_m, const double* limit_con, int nobj, const double* w, const double* xmax,
                       int maxit, double* x, double* g, int* status, int* iters, int* work, double* lam);
/* The host step of the reliability stage, no GPU: value, best and best_x as stated above from quant [nq][nens nobj], g
 * [nens][nobj] and x [nens][nobj][nctl] (any values).  value, best, best_x: each NULL ok.  UCF_ERR_BAD_ARGUMENT: nq outside
 * 1..UCF_ENSEMBLE_MAX_Q, nens outside 1..UCF_ENSEMBLE_MAX, nobj outside 1..UCF_ALLOC_MAX_OBJ, nctl outside 1..UCF_YIELD_MAX_CTL, a
 * NULL quant, g or x. */
int ucf_allocate_select(int nq, int nens, int nobj, int nctl, const double* quant, const double* g, const double* x, double* value,
                        int* best, double* best_x);
/* field_allocate_kernel exactly as ucf_field_allocate launches it (the same launcher), once, on caller data R
 * [nens][nctl + 1][ncon], limit_con [ncon], con [ncon], w [nobj][nctl], xmax [nctl]: the twin of ucf_debug_field_yield.  x, g,
 * status, iters, work, lam as in ucf_field_allocate and nbad [1] (every invalid member): each NULL ok.  R may hold anything.
 * UCF_ERR_BAD_ARGUMENT: nctl outside 1..UCF_YIELD_MAX_CTL, nens outside 1..UCF_ENSEMBLE_MAX, ncon < 1, nobj outside
 * 1..UCF_ALLOC_MAX_OBJ, maxit outside 1..UCF_ALLOC_MAX_ITER, nens (nctl + 1) ncon beyond 2^31-1 values, a NULL R, limit_con, con, w
 * or xmax, a w or a limit_con that is not finite, an xmax that is not positive and finite, a con that is negative or does not
 * ascend strictly.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_field_allocate(int nctl, int nens, int ncon, int nobj, const double* R, const double* limit_con, const int* con,
                             const double* w, const double* xmax, int maxit, double* x, double* g, int* status, int* iters, int* work,
                             double* lam, long long* nbad /*[1]*/);
/* ---- well-field times: WHEN does the drawdown at a receptor first pass a permitted value, from when on does it stay below one
 * after the pumps have stopped, and how sure is either under the posterior.  The member maps of an ensemble are on the device when
 * its member loop ends; field_times_kernel turns every member's time series at every (location, depth) into a time per limit,
 * and the member reduction of ucf_field_ensemble runs on those times.  Only the maps that are asked for cross the bus.
 *   notation     nsite = nloc nz, site e = iloc nz + z; a = the s slots [nens][nt][nsite] of ucf_field_ensemble (the dimensional
 *                drawdown; ds takes no part); T [nens][nlim][nsite]; nout = nlim nsite for everything the reduction writes.
 *   abscissa     tau [nt], strictly increasing and finite: what the answer is expressed in and interpolated in.  NULL: the field's
 *                t.  (ln t is the usual other choice: drawdown is close to linear in it.)  tau_never, finite and above tau[nt-1]:
 *                the censoring value for "not within the horizon of the map".
 *   limits       limit [nlim] dimensional drawdowns, finite, with kind [nlim], nlim in 1..UCF_ENSEMBLE_MAX_Q.
 *   members      those of ucf_field_ensemble; with weight != NULL those of ucf_field_ensemble_weighted: u =
 *                ucf_ensemble_quantise(weight) after the other argument checks, a member with u[m] = 0 is validated but not
 *                launched and its slots are NaN bytes; u, *ess, *nlaunched are written before any GPU work, with or without a
 *                device.  The plan, the validation of every member before the first launch and what runs per member are exactly
 *                those of ucf_field_ensemble: slot m of a has the bits of its member map.
 *   times        field_times_kernel, one thread per (member m, limit l, site e), e fastest; the thread walks k = 0 .. nt-1 once;
 *                every operation rounded on its own (no FMA contraction); L = limit[l]; no atomics.
 *                kind[l] == UCF_TIME_FIRST_ABOVE, the first up-crossing: for k ascending, v = a[m][k][e]:
 *                    v not finite:   T = NaN, stop
 *                    v > L (strict, as in pexc), stop with
 *                        k == 0:     T = tau[0]
 *                        otherwise   v0 = a[m][k-1][e];   f = (L - v0) / (v - v0);   T = tau[k-1] + f * (tau[k] - tau[k-1])
 *                    no k stops:     T = tau_never
 *                  Values behind the crossing are not read: a NaN there does not matter.  v0 <= L < v, so f is in [0, 1).
 *                kind[l] == UCF_TIME_LAST_ABOVE, the abscissa from which the value stays at or below L (the recovery time): all
 *                nt values are read and any that is not finite gives T = NaN.  Otherwise, with k* the last k with a[m][k][e] > L:
 *                    there is none:  T = tau[0]
 *                    k* == nt-1:     T = tau_never
 *                    otherwise       v0 = a[m][k*][e];  v1 = a[m][k*+1][e];   f = (v0 - L) / (v0 - v1);
 *                                    T = tau[k*] + f * (tau[k*+1] - tau[k*])                       (v1 <= L < v0: f is in (0, 1])
 *                The Wynn sentinel is finite and takes part, as everywhere.  A slot of NaN bytes (a member that was not launched)
 *                gives NaN.  The NaN written is the quiet NaN 0x7ff8000000000000.
 *   reduction    no kernel of its own and none edited: the reduction of ucf_field_ensemble (of ucf_field_ensemble_weighted with
 *                weights), through its launcher, once, on T as [nens][nout], with horizon [nhor] in the place of its limit: T-> mean,
 *                sd, min, max, nfin [nout], quant [nq][nout], all = T itself; plater [nhor][nout] is its pexc, the share of the
 *                finite members with T > horizon[h] -- the chance of crossing by H is 1 - plater, the chance of never crossing
 *                within the map is plater at H = tau[nt-1]; nbad[0] is its count (the outputs where a member that counts has
 *                T = NaN).  Row l of every array belongs to limit l.  A censored member takes part with T = tau_never: quantiles
 *                below the censored share are exact, mean and sd are those of the censored values.
 * T is a buffer of the field (grown on demand, kept, counted in ucf_field_alloc_count) beside those of ucf_field_ensemble, which
 * the call shares: a repeated call of the same or a smaller size allocates nothing, and ucf_field_ensemble before and after it
 * gives the same bits.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_ensemble (with
 * weight: _weighted) checks on field, nz, z, npar, ids, nens, thetas, nq, q, quant and, as its nlim and limit, on nhor and horizon
 * (nhor outside 0..UCF_ENSEMBLE_MAX_Q, or positive with a NULL horizon; a horizon that is not finite); a NULL T; plater with
 * nhor = 0; nlim outside 1..UCF_ENSEMBLE_MAX_Q; a NULL limit or kind; a limit that is not finite; a kind outside the enum; a tau
 * that is not finite or does not increase strictly; tau_never not finite or not above tau[nt-1]; nens nlim nsite beyond what one
 * buffer may hold.  With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan". */
enum { UCF_TIME_FIRST_ABOVE = 0, UCF_TIME_LAST_ABOVE = 1 };
int ucf_field_ensemble_times(ucf_field* field, ucf_plan* plan, int npar, const int* ids,
                             int nens, const double* thetas /*[nens][npar]*/,
                             const double* weight /*[nens]; NULL: every member counts equally*/,
                             int nz, const double* z,
                             const double* tau /*[nt]; NULL: the field's t*/, double tau_never,
                             int nlim, const double* limit /*[nlim]*/, const int* kind /*[nlim]*/,
                             int nq, const double* q /*[nq]*/, int nhor, const double* horizon /*[nhor], in units of tau*/,
                             const ucf_ensemble_maps* T /*every array over nlim nloc nz outputs; all: [nens][nlim][nloc][nz]*/,
                             double* plater /*[nhor][nlim nloc nz]; NULL ok*/,
                             long long* nbad /*[1]; NULL ok*/, ucf_stats* stats /*NULL ok*/,
                             unsigned long long* u /*[nens]; NULL ok*/, double* ess /*NULL ok*/, int* nlaunched /*NULL ok*/);
/* field_times_kernel exactly as ucf_field_ensemble_times launches it (the same launcher), once, on caller data a [nens][nt][nsite]:
 * a, tau, limit and kind are uploaded, T [nens][nlim][nsite] is copied back.  a may hold anything.  UCF_ERR_BAD_ARGUMENT: nens
 * outside 1..UCF_ENSEMBLE_MAX, nt or nsite < 1, a NULL a, tau or T, what ucf_field_ensemble_times checks on nlim, limit, kind, tau
 * and tau_never, nens nsite max(nt, nlim) beyond 2^31-1 values.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_field_times(int nens, int nt, long long nsite, const double* a, const double* tau, double tau_never,
                          int nlim, const double* limit, const int* kind, double* T);
/* ---- well-field Sobol indices: WHICH parameter causes the spread of a forecast where the posterior is too wide to linearise.
 * The sensitivities of ucf_field_forecast are derivatives at one point; over the width of a real posterior the drawdown is not
 * linear in ln Sy, ln kappa or ln Ss (see the ensembles above), and a parameter may matter only through an interaction, which a
 * one-at-a-time derivative never sees.  Variance-based global sensitivity analysis answers per output with the first-order index
 * S_j, the share of the variance that parameter j explains alone, the total index ST_j, its share including every interaction,
 * and a standard error of each.  A Saltelli design is an ensemble of (npar + 2) nbase members; its member maps stay on the device
 * and are reduced there over the member axis.  Only the maps that are asked for cross the bus.
 *   design       ucf_sobol_design, host only, pure copies, no arithmetic.  With N = nbase and draws [2 N][npar]:
 *                    block 0, rows 0 .. N-1 of thetas:       A = draws[0 .. N)
 *                    block 1, rows N .. 2N-1:                B = draws[N .. 2N)
 *                    block 2 + j, j = 0 .. npar-1:           A with column j taken from B
 *                thetas [(npar + 2) N][npar], row (block) N + r.  Any source of the 2 N draws is legal: ucf_field_ensemble_draw
 *                with one seed, a Latin hypercube, anything else.  The variance decomposition PRESUPPOSES INDEPENDENT
 *                PARAMETERS, so a design drawn with a diagonal cov.  With correlated draws the numbers are still computed and
 *                still repeatable, but S and ST lose that meaning.  UCF_ERR_BAD_ARGUMENT: npar outside 1..UCF_FIT_MAX_PAR,
 *                nbase outside 2..UCF_SOBOL_MAX_BASE, a NULL array, a draw that is not positive and finite (row and parameter
 *                are named).
 *   members      ucf_field_sobol does with the (npar + 2) N members exactly what ucf_field_ensemble does with its nens: the
 *                same plan rules, the same scratch plan, every member validated and its launch arrays checked before the first
 *                launch, the same launch sequence per member, the same slots.  Slot m has the bits of ucf_field_drawdown on a
 *                fresh field and a fresh plan of member m.  No member is skipped or deduplicated.
 *   reduction    field_sobol_kernel<npar>, one thread per output e, once on the s slots (a = the s slots) and once on the ds
 *                slots, every operation rounded on its own (no FMA contraction).  fa = a[r][e], fb = a[N + r][e],
 *                fj = a[(2 + j) N + r][e].  Base row r is COMPLETE at e where all npar + 2 of these values are finite; the Wynn
 *                sentinel is finite and takes part, as everywhere.  C = the complete rows in ascending r, n = |C|; rows that
 *                are not complete take part in nothing.
 *                    nrow[e] = n
 *                    sA = +0.0; sB = +0.0;   for r in C:  sA = sA + fa;  sB = sB + fb
 *                    mean[e] = (sA + sB) / (double)(2 n)                                (n = 0: NaN, and everything below NaN)
 *                    qA = +0.0; qB = +0.0;   for r in C:  d = fa - mean; qA = qA + d*d;  d = fb - mean; qB = qB + d*d
 *                    var[e] = (qA + qB) / (double)(2 n - 1)
 *                    per j:  v1 = q1 = vt = qt = +0.0;  for r in C:
 *                                p  = (fb - mean) * (fj - fa);   v1 = v1 + p;    q1 = q1 + p*p
 *                                dt = fa - fj;  pt = dt*dt;      vt = vt + pt;   qt = qt + pt*pt
 *                            m1 = v1 / (double)n;   mt = vt / (double)n
 *                            S[j][e]  = m1 / var              ST[j][e] = (0.5 * mt) / var               (NaN unless var > 0)
 *                            w1 = q1/(double)n - m1*m1;   wt = qt/(double)n - mt*mt            (a negative w counts as +0.0)
 *                            seS[j][e]  = sqrt(w1/(double)(n-1)) / var
 *                            seST[j][e] = (0.5 * sqrt(wt/(double)(n-1))) / var               (n < 2 or not var > 0: NaN)
 *                The estimators are Saltelli's of 2010 for the first-order index, with f(B) centred, and Jansen's for the total
 *                index, both normalised by the pooled sample variance of A u B; seS and seST are the standard errors of the row
 *                means m1 and mt, taking var as given.  Every NaN written is the quiet NaN 0x7ff8000000000000.
 *                nbad[0] (s) and nbad[1] (ds) count the outputs with n < nbase (a ballot per wave, one integer atomic per wave,
 *                no floating-point atomics: a call repeated gives the same bits).
 *                What the statement implies: a parameter that the map does not depend on has fj bitwise equal to fa in every
 *                row; its ST and seST are then exactly +0.0, and so are its S and seS, because every p is +-0 and the sums
 *                start from +0.0 (where var > 0, and for the errors n >= 2).  A constant column has var = 0: all four are NaN.
 *   outputs      per map one ucf_sobol_maps; every pointer may be NULL, and a NULL struct asks for nothing of that map.  `all`
 *                [(npar + 2) N][nout] are the member maps as they stand.  stats: summed over all members and groups.
 * The slots are those of ucf_field_ensemble; the statistics' staging is one more buffer of the field, grown on demand, kept and
 * counted in ucf_field_alloc_count: a repeated call of the same or a smaller size allocates nothing, and ucf_field_ensemble before
 * and after it gives the same bits.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): everything ucf_field_drawdown
 * checks (its s, ds aside); NULL ids or thetas; npar outside 1..UCF_FIT_MAX_PAR; nbase outside 2..UCF_SOBOL_MAX_BASE; a theta that
 * is not positive and finite (the member is named); thetas that do not have the design's structure bit for bit --
 * thetas[(2 + j) N + r][k] is B[r][k] where k == j and A[r][k] otherwise -- (block, row and parameter are named); (npar + 2) N nout
 * beyond what one buffer may hold.  With a NULL plan UCF_ERR_NO_DEVICE comes before "NULL plan"; with a plan the checks of
 * ucf_fit_perturb and of every member run before any launch. */
#define UCF_SOBOL_MAX_BASE 1024     /* base rows N of one design; members = (npar + 2) N */
typedef struct ucf_sobol_maps {     /* per map (one for s, one for ds); every pointer may be NULL */
    double *S, *ST, *seS, *seST;    /* [npar][nout] */
    double *mean, *var;             /* [nout] */
    double *all;                    /* [(npar + 2) nbase][nout]: the member maps */
    int    *nrow;                   /* [nout]: complete base rows there */
} ucf_sobol_maps;
int ucf_sobol_design(int npar, int nbase, const double* draws /*[2 nbase][npar]*/, double* thetas /*[(npar+2) nbase][npar]*/);
int ucf_field_sobol(ucf_field* field, ucf_plan* plan, int npar, const int* ids, int nbase, const double* thetas,
                    int nz, const double* z, const ucf_sobol_maps* s, const ucf_sobol_maps* ds /*either may be NULL*/,
                    long long* nbad /*[2]: s, ds; NULL ok*/, ucf_stats* stats /*NULL ok*/);
/* field_sobol_kernel exactly as ucf_field_sobol launches it (the same launcher, and through it the same instantiation), once, on
 * caller data a [(npar + 2) nbase][nout]: a is uploaded, the maps that `out` asks for (out->all is ignored; out may be NULL) and
 * nbad[0] are copied back.  a may hold anything.  UCF_ERR_BAD_ARGUMENT: npar or nbase out of range, nout < 1, a NULL a,
 * (npar + 2) nbase nout beyond what one buffer may hold.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_sobol(int npar, int nbase, long long nout, const double* a /*[(npar+2) nbase][nout]*/,
                    const ucf_sobol_maps* out /*all ignored*/, long long* nbad /*[1]*/);
/* The reduction kernel of ucf_fit_evaluate exactly as a fit launches it (the same launcher, and through it the same choice among the
 * instantiations: npar 0..UCF_FIT_MAX_PAR x source x with / without derivative data), on caller data.  One 256-thread workgroup
 * per parameter set; set s owns the plans s (1 + 2 npar) + (0 base | 1 + 2j: parameter j up | 2 + 2j: parameter j down);
 * nplans = nsets (1 + 2 npar).  h [nh] is the dimensionless drawdown, dh [nh] its log-time derivative in the same layout (NULL: a
 * fit without derivative data; then dobs, wd, tfac are not read and the sums have no phi_d), Hc [nplans] the scale of each plan.
 *   source 0     slots: the value of observation i under a plan is h[plan * plan_stride + slot[i]];
 *   source 1     network: observation i reads count[i] consecutive doubles at prefix[i] * nplans + plan * stride[i] + at[i] (nref =
 *                nobs): count 1 is the value itself; otherwise, with v the n = count doubles, the screen average of
 *                ucf_screen_average:  s = v[1];  s = s + v[j], j = 2 .. n-1;  ((v[0] + 2.0 * s) + v[n-1]) / (double)(2 n);
 *   source 2     field: observation i is the sum of the terms first[i] .. first[i+1]-1 (nref terms; prefix, stride, at, count, q and,
 *                with dh, tfac per term):  acc = +0.0;  acc = acc + q * (value at the term's ref);  on dh
 *                acc = acc + q * (tfac * (value at the ref)).  An observation without terms is +0.0.
 * The arrays of the other sources are not read and may be NULL.  Every operation is rounded on its own (no FMA contraction):
 *   s[k] = value * Hc[plan0 + k], k = 0 .. 2 npar (sd[k] the same from dh);   d[j] = (s[1+2j] - s[2+2j]) / two_dlog (dd[j] from sd);
 *   wr = w[i] * (obs[i] - s[0]);  wd_[j] = w[i] * d[j];   wrd = wd[i] * (dobs[i] - sd[0]);  wdd[j] = wd[i] * dd[j];
 *   observation i counts where every s[k] is finite and (dh is NULL or wd[i] == 0 or every sd[k] is finite); nbad[set] is the number
 *   that do not.  One that counts adds, in this order:  phi += wr * wr;  g[j] += wd_[j] * wr;  A[q] += wd_[j] * wd_[k], j <= k row by
 *   row;  then, only where wd[i] > 0 (skipped, not added as zero; dobs[i] is read only there):  phi += wrd * wrd;
 *   phi_d += wrd * wrd;  g[j] += wdd[j] * wrd;  A[q] += wdd[j] * wdd[k].
 *   Order of the sums: lane l of 256 takes the observations l, l + 256, ... ascending, each accumulator from +0.0; per wave of 64
 *   lanes the butterfly v = v + v[lane ^ m], m = 32, 16, 8, 4, 2, 1; then wave 0 + wave 1 + wave 2 + wave 3 in that order.  No
 *   floating-point atomics: a repeated call gives the same bits.
 * Outputs: sums [nsets][1 + npar + npar (npar+1) / 2 (+ 1 with dh)] = phi | g | upper A | phi_d;  nbad [nsets];  J, Jd
 * [nsets][nobs][npar] = d, dd and sim, simd [nplans][nobs] = s, sd of EVERY observation, counted or not; each of the four may be
 * NULL.
 * Validation comes first and needs no GPU (UCF_ERR_BAD_ARGUMENT, offender in ucf_last_error): source outside 0..2, npar outside
 * 0..UCF_FIT_MAX_PAR, nsets outside 1..2^16, nobs outside 1..2^24, nh outside 1..2^28, a NULL array that the call would read or
 * must write, Jd or simd without dh, and every element the kernel could read under any plan lying outside [0, nh): plan_stride < 1
 * or nplans plan_stride
 * > nh, a slot outside 0 .. plan_stride - 1; a ref or term with a negative prefix, stride or at, a count outside 1..UCF_MAX_NZ, or
 * prefix nplans + (nplans - 1) stride + at + count - 1 >= nh; nref != nobs for a network; first[0] < 0, first not ascending, or
 * first[nobs] != nref.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_fit_reduce(int source, int npar, int nsets, int nobs, double two_dlog,
                         long long nh, const double* h, const double* dh /*NULL ok*/, const double* Hc /*[nplans]*/,
                         const double* obs, const double* w, const double* dobs, const double* wd /*[nobs]*/,
                         const int* slot /*[nobs]*/, long long plan_stride,
                         int nref, const long long* prefix, const long long* stride, const int* at, const int* count /*[nref]*/,
                         const double* q, const double* tfac /*[nref]*/, const int* first /*[nobs + 1]*/,
                         double* sums, int* nbad, double* J, double* sim, double* Jd, double* simd);
/* ucf_debug_fit_reduce under a robust loss (ucf_fit_set_loss states the arithmetic): the production launcher on caller data with
 * kind = UCF_LOSS_HUBER or UCF_LOSS_TUKEY and the constant c, through the ROBUST instantiations of the kernel.  sums is one entry
 * longer per set, phi | g | upper A | [phi_d] | phi_w.  ndown [nsets] = counted residual terms with a factor below 1.0; b, bd
 * [nsets][nobs] = the factor of observation i's drawdown residual and of its derivative residual under the set's base plan, NaN
 * where the observation does not count (bd: or has wd[i] == 0); each of the three may be NULL, bd needs dh.  The validation of
 * ucf_debug_fit_reduce, which needs no GPU, and: kind outside 1..2 (least squares is ucf_debug_fit_reduce), c not positive and
 * finite, bd without dh.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_fit_reduce_loss(int kind, double c, int source, int npar, int nsets, int nobs, double two_dlog,
                              long long nh, const double* h, const double* dh /*NULL ok*/, const double* Hc /*[nplans]*/,
                              const double* obs, const double* w, const double* dobs, const double* wd /*[nobs]*/,
                              const int* slot /*[nobs]*/, long long plan_stride,
                              int nref, const long long* prefix, const long long* stride, const int* at, const int* count /*[nref]*/,
                              const double* q, const double* tfac /*[nref]*/, const int* first /*[nobs + 1]*/,
                              double* sums, int* nbad, double* J, double* sim, double* Jd, double* simd,
                              int* ndown, double* b, double* bd);
/* The RESAMPLE instantiations of the kernel (ucf_fit_set_resample states the arithmetic) through the production launcher on caller
 * data: the arguments of ucf_debug_fit_reduce_loss -- kind 0 (UCF_LOSS_L2) is allowed here and runs as Huber with c = +inf, c is
 * then not read -- without J, sim, Jd, simd, b and bd, which belong to a parameter set and not to a reduction, plus mult
 * [nrep][nobs], nred, set_of [nred] (NULL: r) and rep [nred] (NULL: all -1).  One workgroup per reduction.  sums
 * [nred][1 + npar + npar (npar+1) / 2 (+ 1 with dh) + 2] = phi | g | upper A | [phi_d] | phi_w | phi_out;  nbad [nred];  counts
 * [nred][4] = nuse, nuse_d, nheld, ndown.  The validation of ucf_debug_fit_reduce, which needs no GPU, and: kind outside 0..2, c not
 * positive and finite under kinds 1 and 2, nrep outside 0..65536 (0: no mult), a NULL mult with nrep > 0, a row of mult that sums
 * beyond 2^31 - 1, nred outside 1..2^16, set_of NULL with nred > nsets, a set_of[r] outside 0..nsets-1, a rep[r] outside
 * -1..nrep-1, a NULL sums, nbad or counts.  Then UCF_ERR_NO_DEVICE without a device. */
int ucf_debug_fit_reduce_resampled(int kind, double c, int source, int npar, int nsets, int nobs, double two_dlog,
                                   long long nh, const double* h, const double* dh /*NULL ok*/, const double* Hc /*[nplans]*/,
                                   const double* obs, const double* w, const double* dobs, const double* wd /*[nobs]*/,
                                   const int* slot /*[nobs]*/, long long plan_stride,
                                   int nref, const long long* prefix, const long long* stride, const int* at, const int* count /*[nref]*/,
                                   const double* q, const double* tfac /*[nref]*/, const int* first /*[nobs + 1]*/,
                                   int nrep, const unsigned short* mult, int nred, const int* set_of, const int* rep,
                                   double* sums, int* nbad, int* counts);
/* Host only: the nwell real wells followed by their mirror images in the straight line a x + b y = c (xo, yo, qo, t0o
 * [2 nwell]).  An image has q = +q for a no-flow boundary (kind 0), -q for a constant-head boundary (kind 1), and the t0 of its
 * real well.  One boundary only (two parallel boundaries need an infinite image series).  UCF_ERR_BAD_ARGUMENT: a = b = 0, a
 * number that is not finite, kind outside 0..1, a well on the line. */
int ucf_field_images(int nwell, const double* xw, const double* yw, const double* qw, const double* t0w,
                     double a, double b, double c, int kind /*0 no-flow, 1 constant head*/,
                     double* xo, double* yo, double* qo, double* t0o /*[2*nwell]*/);

/* driver.f90:234-243 (quirk Q2: not a textbook trapezoid) */
int ucf_screen_average(int npts, int zOrd, const double* h, double* havg);

/* ---- stage hooks (device implementations of the imported procedures; used by the
 * parity tests to compare each stage with the oracle) ---- */
/* lap_hank_soln, laplace_hankel_solutions.f90:30-120: fp[n_a][nz][np] complex */
int ucf_eval_samples(ucf_plan* plan, int n_a, const double* a, double rD,
                     int np, const double* p_re_im, int nz, const double* zD, const int* zLay,
                     double* fp_re_im);
/* deHoog_pvalues, invlap.f90:154-172 */
int ucf_pvalues(const ucf_plan* plan, double tee, double* p_re_im);
/* deHoog_invlap (scalar t), invlap.f90:143-152 -> 46-141; n independent problems */
int ucf_dehoog(int n, int M, double alpha, double tol, const double* t, const double* tee,
               const double* fp_re_im /*[n][2M+1]*/, double* ft);
/* wynn_epsilon, integration.f90:125-189; status: 0 ok, 1 truncated, 2 sentinel, 3 early exit */
int ucf_wynn_epsilon(int n, int nterms, const double* series_re_im /*[n][nterms]*/,
                     double* acc_re_im, int* status);
/* extraptozero, integration.f90:192-237 */
int ucf_extraptozero(int n, int R, const double* x /*[R]*/, const double* y_re_im /*[n][R]*/,
                     double* out_re_im);

/* The intermediate stages (driver.f90:129-216) of the PRODUCTION launch sequence: the call runs exactly what
 * ucf_drawdown_grid (grid != 0: nt times x nr radii) or ucf_drawdown_batch on a list already ordered by radius (grid == 0:
 * nt = nr = number of points, rD per point) would run for these sizes -- the same lane layout, kernel instantiations and
 * launch bounds -- and then reads back what those kernels left in the plan's workspace:
 *   state [npts][2M+1][(R+1+nacc)*nz] complex: per Laplace sample the level sums [R][nz] of the tanh-sinh part (WITHOUT the
 *         factor arg/2 of driver.f90:135,154, which the finishing kernel applies), the area of the interval in progress
 *         [nz], the finished J0-interval areas [nacc][nz] (driver.f90:201-203); zeros where the launch sequence keeps no
 *         state (info[1] = 0: the monolithic kernel);
 *   ndone [npts][2M+1]: abscissae the fast evaluators integrated (< nabs: the item was finished by the reference-order
 *         evaluator, whose accumulators never leave the kernel: its state entries are what the hand-over was);
 *   totlap [npts][nz][2M+1] complex: finint + infint (driver.f90:216);   h, dh [npts][nz].
 * info[0..3] = lane layout used (0 sample, 1 time, 3 point), slots per sample, 2M+1, npts.  Needs nz <= the depths of
 * one launch and sizes that make one launch sequence (UCF_ERR_UNSUPPORTED otherwise). */
int ucf_debug_stages(ucf_plan* plan, int grid, int nt, const double* tD, const int* sv, int nr, const double* rD,
                     int nz, const double* zD, const int* zLay, double* state, int* ndone, double* totlap,
                     double* h, double* dh, int* info);
/* wynn_epsilon as the finishing kernel runs it -- both epsilon columns in registers, at most 12 terms -- in flavour
 * `mode` (0 faithful, 1 fast); same conventions as ucf_wynn_epsilon */
int ucf_debug_wynn(int mode, int n, int nterms, const double* series_re_im, double* acc_re_im, int* status);
/* deHoog_invlap as every grid call and long point list runs it (the tiled kernel: cooperative quotient-difference rhombus,
 * continued fraction per lane): n transforms fp[n][2M+1] at times t[n], T = 2 t (driver.f90:106); h[n] = f(t),
 * dh[n] = t * (inverse of p F(p)) (driver.f90:219-230) */
int ucf_debug_dehoog_tiles(int mode, int n, int M, double alpha, double tol, const double* t, const double* fp_re_im,
                           double* h, double* dh);

/* K0(z), K1(z), Re z >= 0: cbesk(z, fnu=0, kode=1, n=2), cbessel.f90:877 -> cbknu :5036 (model 2);
 * k_re_im[n][2][2] = (K0, K1), ierr[n] as cbesk's IERR */
int ucf_bessel_k01(int n, const double* z_re_im, double* k_re_im, int* ierr);

/* the (sin, cos)(k pi / 128), k = 0..255, table that every plan uploads for the fast flavour's evaluators (host code, no
 * GPU needed; tab[256][2]) */
int ucf_sincos_table(double* tab);
/* and the 2^(j/128), j = 0..127, table behind it (exp of the fast flavour's evaluators; tab[128][2] = (hi, lo)) */
int ucf_exp2_table(double* tab);

/* ---- measurement helper: sustained fp64 FMA rate of the device ---- */
int ucf_fp64_fma_peak(double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* UCF_H */
