// ucf_field.h -- launchers of the well-field kernels: the superposition, called by ucf_field_drawdown, ucf_field_forecast and
// ucf_field_ensemble (ucf_field.cpp), the response slots of ucf_field_yield, the combination of a forecast (all three
// ucf_field.hip), the reduction of an ensemble (ucf_field_ensemble.hip), the data worth of candidate wells
// (ucf_field_worth.hip), the ratio test of ucf_field_yield (ucf_field_yield.hip), the linear programme of ucf_field_allocate
// (ucf_field_allocate.hip; its serial steps, shared with the host twin, are ucf_field_allocate.h), the time kernel of
// ucf_field_ensemble_times (ucf_field_times.hip) and the reduction of a Saltelli design (ucf_field_sobol.hip).
#pragma once
#include <cstddef>

// What the kernel needs of well j: its rate factor and where its group's results lie.  The groups' h (and dh) share one
// buffer, group g at `off` doubles, [nt_g][nr][nz]; tfac of all groups one array, group g at `toff`.
struct ucf_field_well {
    double q;
    long long off;
    int k0, nr, toff, _pad;
};

// One thread per output (k, i, z) of s, ds [nt][nloc][nz], z fastest:
//   acc = +0.0;  for j = 0..nwell-1 with k >= k0_j:  at = off_j + ((k - k0_j) nr_j + col[i][j]) nz + z
//     s :  acc = acc + q_j * h[at]        ds :  acc = acc + q_j * (tfac[toff_j + k - k0_j] * dh[at])
//   both times `scale` unless scaled == 0.
// d_wells [nwell], d_col [nloc][nwell] (column of location i in the group of well j), d_tfac, d_h, d_dh as above.
int ucf_field_launch_superpose(int nt, int nloc, int nz, int nwell, const ucf_field_well* d_wells, const int* d_col,
                               const double* d_tfac, const double* d_h, const double* d_dh, int scaled, double scale,
                               double* d_s, double* d_ds, void* stream);

// The response slots of ucf_field_yield, field_response_kernel, in place of the superposition: one thread per (slot c,
// constrained output i) of d_R [nctl + 1][ncon], output e = d_con[i] = (k, iloc, z) of the map:
//   acc = +0.0;  for j = 0..nwell-1 with d_ctl[j] == c (slot nctl: d_ctl[j] == -1) and k >= k0_j:  acc = acc + q_j * h[at]
//   d_R[c][i] = acc * scale                                       (`at` as in the superposition; dh is not read)
// d_ctl [nwell] in -1 .. nctl-1, d_con [ncon] each in 0 .. nt nloc nz - 1 (the caller has checked both).
int ucf_field_launch_response(int ncon, int nctl, int nloc, int nz, int nwell, const ucf_field_well* d_wells, const int* d_col,
                              const int* d_ctl, const int* d_con, const double* d_h, double scale, double* d_R, void* stream);

// The ratio test of ucf_field_yield (ucf_field_yield.hip), field_yield_kernel<nctl>: a workgroup of 256 threads per (member,
// tile of UCF_YIELD_PAT_TILE patterns); the arithmetic is stated with ucf_field_yield in include/ucf.h.  Device memory throughout.
struct ucf_yield_args {
    int nctl, nens, ncon, npat;            // 1..UCF_YIELD_MAX_CTL, 1..UCF_ENSEMBLE_MAX, >= 1, 1..UCF_YIELD_MAX_PAT
    const double* d_R;                     // [nens][nctl + 1][ncon]
    const double* d_x;                     // [npat][nctl]
    const double* d_lim;                   // [ncon] the limit of constrained output i
    const int* d_con;                      // [ncon] ascending, not negative
    double smax;
    double *d_y, *d_fe, *d_hi, *d_lo;      // [nens][npat]
    int *d_bind, *d_dead;                  // [nens][npat]
    long long* d_nbad;                     // += the members with a slot value that is not finite; the caller zeroes it
};
// UCF_ERR_BAD_ARGUMENT for what the comments above exclude and for a NULL array
int ucf_field_launch_yield(const ucf_yield_args* a, void* stream);

// The linear programme of ucf_field_allocate (ucf_field_allocate.hip), field_allocate_kernel<nctl>: a workgroup of 256 threads
// per (member, objective); the arithmetic is stated with ucf_field_allocate in include/ucf.h.  Device memory throughout.
struct ucf_allocate_args {
    int nctl, nens, ncon, nobj, maxit;     // 1..UCF_YIELD_MAX_CTL, 1..UCF_ENSEMBLE_MAX, >= 1, 1..UCF_ALLOC_MAX_OBJ, 1..UCF_ALLOC_MAX_ITER
    const double* d_R;                     // [nens][nctl + 1][ncon]
    const double* d_lim;                   // [ncon] the limit of constrained output i
    const double* d_w;                     // [nobj][nctl]
    const double* d_xmax;                  // [nctl]
    double *d_x, *d_g, *d_lam;             // [nens][nobj][nctl], [nens][nobj], [nens][nobj][nctl]
    int *d_status, *d_iters, *d_work;      // [nens][nobj], [nens][nobj], [nens][nobj][nctl]
    double* d_xpat;                        // NULL ok: [nens nobj][nctl], x where the status is 0 and +0.0 elsewhere
    long long* d_nbad;                     // += the members with a slot value that is not finite; the caller zeroes it
};
// UCF_ERR_BAD_ARGUMENT for what the comments above exclude and for a NULL array
int ucf_field_launch_allocate(const ucf_allocate_args* a, void* stream);

// The time kernel of ucf_field_ensemble_times (ucf_field_times.hip), field_times_kernel: one thread per (member m, limit l, site
// e) of d_T [nens][nlim][nsite], e fastest, a workgroup of 256 threads per (tile of sites, l, m); the arithmetic is stated with
// ucf_field_ensemble_times in include/ucf.h.  Device memory throughout.
struct ucf_times_args {
    int nens, nt;                          // 1..UCF_ENSEMBLE_MAX, >= 1
    long long nsite;                       // >= 1, below 2^32 - 256
    const double* d_a;                     // [nens][nt][nsite] the series, site fastest
    const double* d_tau;                   // [nt] strictly increasing and finite
    double tau_never;                      // finite, above d_tau[nt - 1]
    int nlim;                              // 1..UCF_ENSEMBLE_MAX_Q
    const double* d_limit;                 // [nlim] finite
    const int* d_kind;                     // [nlim] UCF_TIME_FIRST_ABOVE or UCF_TIME_LAST_ABOVE
    double* d_T;                           // [nens][nlim][nsite]
};
// UCF_ERR_BAD_ARGUMENT for what the comments above exclude and for a NULL array (the caller has checked tau, the limits and the kinds)
int ucf_field_launch_times(const ucf_times_args* a, void* stream);

// The reduction of a Saltelli design over its member axis (ucf_field_sobol.hip), field_sobol_kernel<npar>: one thread per output
// e of the member maps d_a [(npar + 2) nbase][nout] -- block 0 the rows of A, block 1 those of B, block 2 + j those of A with
// column j from B --, a workgroup of 256 threads; the arithmetic is stated with ucf_field_sobol in include/ucf.h.  Device memory
// throughout.
struct ucf_sobol_args {
    int npar, nbase;                       // 1..UCF_FIT_MAX_PAR, 2..UCF_SOBOL_MAX_BASE
    long long nout;                        // >= 1
    const double* d_a;                     // [(npar + 2) nbase][nout]
    double *d_S, *d_ST, *d_seS, *d_seST;   // [npar][nout]; these, d_mean, d_var and d_nrow may each be NULL (not written)
    double *d_mean, *d_var;                // [nout]
    int* d_nrow;                           // [nout] the complete base rows
    long long* d_nbad;                     // += the outputs with fewer than nbase complete rows; the caller zeroes it
};
// UCF_ERR_BAD_ARGUMENT for what the comments above exclude and for a grid beyond 2^31 - 1 workgroups
int ucf_field_launch_sobol(const ucf_sobol_args* a, void* stream);

// The combination of a forecast, field_forecast_kernel<npar>: one thread per output e of the slots d_a [1 + 2 npar][nout]
// (slot 0 the base set, slot 1 + 2j / 2 + 2j parameter j up / down), every operation rounded on its own:
//   J_j = (a[1+2j][e] - a[2+2j][e]) / two_dlog;   d_sens[j][e] = J_j   (d_sens NULL: not stored)
//   var = +0.0;  for j = 0..npar-1:  inner = +0.0;  for k = 0..npar-1: inner = inner + cov[j][k] * J_k;   var = var + J_j * inner
//   d_se[e] = (var < 0) ? +0.0 : sqrt(var), a NaN var stays NaN   (d_se NULL: not formed; not NULL needs d_cov [npar][npar])
//   *d_nbad += the number of outputs e for which any of the 1 + 2 npar values a[.][e] is not finite (the caller zeroes it).
// UCF_ERR_BAD_ARGUMENT for npar outside 1..UCF_FIT_MAX_PAR.
int ucf_field_launch_forecast(int npar, long long nout, double two_dlog, const double* d_a, const double* d_cov, double* d_sens,
                              double* d_se, long long* d_nbad, void* stream);

// The reduction of an ensemble over its member axis (ucf_field_ensemble.hip), on the member maps d_a [nens][nout]; the
// arithmetic is stated with ucf_field_ensemble and ucf_field_ensemble_weighted in include/ucf.h.  F(e) = the members m with
// a[m][e] finite, in member order, each of mass 1; with weights d_u only those with u[m] > 0, each of mass u[m].
// field_ensemble_moments_kernel / _wmoments_kernel, one thread per output e, then, where d_quant is not NULL,
// field_ensemble_quantile_kernel<T> / _wquantile_kernel<T>: a workgroup of 256 threads ranks the members of T =
// ucf_field_ensemble_tile(nens) neighbouring outputs against each other in LDS, (nens + 2 UCF_ENSEMBLE_MAX_Q) T doubles, at
// most 144 KB; weighted (nens + UCF_ENSEMBLE_MAX_Q) T, at most 136 KB.  Device memory throughout.
struct ucf_ensemble_reduce_args {
    int nens;                              // 1..UCF_ENSEMBLE_MAX
    long long nout;
    const double* d_a;
    const unsigned long long* d_u;         // [nens] the integers of ucf_ensemble_quantise, each 0 .. 2^32; NULL: unweighted
    int nq, nlim;                          // 1..UCF_ENSEMBLE_MAX_Q with d_quant, 0..UCF_ENSEMBLE_MAX_Q (>= 1 with d_pexc)
    const double *d_q, *d_limit;           // [nq] levels, read with d_quant; [nlim] limits, read with d_pexc
    double *d_mean, *d_sd, *d_min, *d_max; // [nout]; these, d_nfin, d_quant and d_pexc may each be NULL (not formed)
    int* d_nfin;                           // [nout] |F|
    double* d_quant;                       // [nq][nout] the order statistics of F at d_q, linearly interpolated; weighted the
                                           // inverse of the weighted empirical distribution function
    double* d_pexc;                        // [nlim][nout] the mass of F above d_limit[l] over the mass of F
    long long* d_nbad;                     // += the outputs with |F| < nens, weighted < the members with u > 0; the caller zeroes it
};
// UCF_ERR_BAD_ARGUMENT for what the comments above exclude and for a grid beyond 2^31 - 1 workgroups
int ucf_field_launch_ensemble_reduce(const ucf_ensemble_reduce_args* a, void* stream);
// outputs per workgroup of the quantile kernels: 64 / 32 / 16 for nens <= 256 / 512 / 1024
int ucf_field_ensemble_tile(int nens);

// Data worth (ucf_field_worth.hip), field_worth_kernel<npar>: one thread per candidate c of the slots d_as, d_ad
// [1 + 2 npar][nt][ncand], one wave per workgroup; the arithmetic is stated with ucf_field_worth in include/ucf.h.  d_F
// [npar][npar] (general, row-major), d_tsel [nt] (never NULL here: all ones where the caller selects every time), d_A
// [ntgt][npar], d_tw [ntgt]; d_post [ntgt][ncand], d_crit [ncand], d_nused [ncand].  d_ad is read only where wd > 0 (NULL ok
// otherwise).  Device memory throughout.  UCF_ERR_BAD_ARGUMENT for npar outside 1..UCF_FIT_MAX_PAR, ntgt outside
// 1..UCF_WORTH_MAX_TGT, nt or ncand < 1, a NULL array that the kernel would read or write.
int ucf_field_launch_worth(int npar, int nt, int ncand, const double* d_as, const double* d_ad, double two_dlog, const double* d_F,
                           double ws, double wd, const int* d_tsel, int ntgt, const double* d_A, const double* d_tw, double* d_post,
                           double* d_crit, int* d_nused, void* stream);
// field_gather_kernel: d_out[i] = d_a[d_idx[i]], i = 0 .. n-1 -- the few slot values that the host needs (targets, the column
// of a picked candidate) of maps that stay on the device.  The caller has checked every index against the length of d_a.
int ucf_field_launch_gather(int n, const long long* d_idx, const double* d_a, double* d_out, void* stream);
