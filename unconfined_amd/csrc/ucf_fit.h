// ucf_fit.h -- launcher of the fit reduction (ucf_fit.hip), called by ucf_fit_evaluate (ucf_fit.cpp).
#pragma once

#include <cstddef>

// The sums of one parameter set (of one reduction, when resampled) in d_sums, stated once: the kernel places them, the host
// sizes its buffers and reads them through this.  phi | g[npar] | upper triangle of A, row by row (j <= k) | [phi_d] the
// derivative terms' share of phi, with derivative data | [phi_w] under a robust or resampled reduction | [phi_out] the held-out
// observations' squares, resampled only.  -1: the launch has no such sum; count = doubles per set.
struct ucf_fit_sums_layout {
    int phi, g, A, phi_d, phi_w, phi_out, count;
};
constexpr ucf_fit_sums_layout ucf_fit_sums(int npar, bool deriv, bool robust, bool resampled)
{
    const int nA = npar * (npar + 1) / 2, tail = 1 + npar + nA, d = deriv ? 1 : 0, w = (robust || resampled) ? 1 : 0;
    return {0, 1, 1 + npar, deriv ? tail : -1, w ? tail + d : -1, resampled ? tail + d + w : -1, tail + d + w + (resampled ? 1 : 0)};
}

// Where an observation of a network fit (ucf_fit_create_network) finds its simulated value.  The h of a network is ragged:
// one region per group of wells with the same number of depths, group g at nplans * prefix_g doubles, plan k of it at
// k * stride_g (stride_g = points per plan x depths of the group, prefix_g = sum of the strides before it).  The
// observation reads `count` consecutive doubles at  prefix * nplans + plan * stride + at:  1 = that depth of its point,
// n > 1 = all n depths of its well, averaged by the rule of ucf_screen_average.
struct ucf_fit_obs_ref {
    long long prefix, stride;
    int at, count;
};

// One term of an observation of a field fit (ucf_fit_create_field): the value that `ref` finds in the h of the network of
// virtual wells, times the rate factor q of its pumping well.
struct ucf_fit_term {
    ucf_fit_obs_ref ref;
    double q;
};

// how observation i finds its simulated value in d_h and, with derivative data, its simulated log-time derivative in d_dh
enum ucf_fit_source {
    UCF_FIT_SLOTS = 0,     // ucf_fit_create: d_h[plan * plan_stride + d_slot[i]]
    UCF_FIT_NETWORK = 1,   // ucf_fit_create_network: through d_ref[i]; a screen is averaged, in d_dh by the same rule
    UCF_FIT_FIELD = 2      // ucf_fit_create_field: the sum of its terms d_term[d_first[i] .. d_first[i + 1]) in that order,
                           // acc = +0.0; acc = acc + q * (value at ref); in d_dh acc = acc + q * (tfac * (value at ref))
};

// One reduction: one 256-thread workgroup per parameter set.  Every simulated value is formed on the dimensionless array
// and then scaled by d_Hc[plan].
struct ucf_fit_reduce_args {
    // npar >= 1: set s owns plans s*(1+2 npar) + (0 base | 1+2j: parameter j up | 2+2j: parameter j down); npar == 0: one
    // plan per set, phi (phi_d) and nbad only.  nplans = nsets * (1 + 2 npar); two_dlog = the step of the central difference
    int npar, nsets, nobs;
    size_t nplans, plan_stride;            // plan_stride: doubles per plan of d_h (UCF_FIT_SLOTS only)
    double two_dlog;
    // dimensionless drawdown as the evaluators left it ([nplans][plan_stride], or ragged: ucf_fit_obs_ref), its log-time
    // derivative in the same layout (NULL: a fit without derivative data), and the scale [nplans]
    const double *d_h, *d_dh, *d_Hc;
    ucf_fit_source source;                 // the pointers of the other sources are not read
    const int* d_slot;                     // [nobs] place of observation i inside one plan's block
    const ucf_fit_obs_ref* d_ref;          // [nobs]
    const ucf_fit_term* d_term;            // [terms]
    const int* d_first;                    // [nobs + 1] ascending; an observation without terms is +0.0
    const double* d_tfac;                  // [terms] t_i / (t_i - t0) of each term; read with derivative data only
    const double *d_obs, *d_w;             // [nobs]
    const double *d_dobs, *d_wd;           // [nobs], with derivative data; d_dobs[i] is read only where d_wd[i] > 0
    double* d_sums;                        // [nsets][ucf_fit_sums_of(this).count], resampled [nred][..]: ucf_fit_sums_layout
    int* d_nbad;                           // [nsets]
    double *d_J, *d_sim;                   // [nsets][nobs][npar], [nsets][1+2 npar][nobs]; each may be NULL
    double *d_Jd, *d_simd;                 // the same of the derivative; each may be NULL
    // The loss (include/ucf.h, ucf_fit_set_loss).  All zero: least squares, the reduction and the sums as above.  Otherwise
    // -- a loss other than UCF_LOSS_L2, or one of the three outputs asked for -- the robust instantiation runs and every set
    // of d_sums is one entry longer (phi_w).  Least squares with an output asked for runs as Huber with c = +inf: every factor
    // is 1.0 and phi, g, A, phi_d, nbad have the bits of the plain reduction.
    int loss;                              // UCF_LOSS_*
    double loss_c;                         // positive and finite; not read under UCF_LOSS_L2
    int* d_ndown;                          // [nsets] counted residual terms with a factor below 1.0; may be NULL
    double *d_b, *d_bd;                    // [nsets][nobs] factor of the drawdown / derivative residual under the base plan, NaN
                                           // where the observation does not count (d_bd: or has wd == 0); each may be NULL;
                                           // d_bd needs d_dh
    // Resampling (include/ucf.h, ucf_fit_set_resample).  nred == 0: none, everything as above.  nred >= 1: the RESAMPLE
    // instantiation runs, one workgroup per REDUCTION r = 0 .. nred-1, which reads the plans of set d_set_of[r] (NULL: r, then
    // nred <= nsets) under the multiplicities d_mult[d_rep[r]][.] (d_rep NULL or d_rep[r] == -1: every m = 1), with the loss above
    // (least squares: Huber with c = +inf).  d_sums [nred][.. | phi_w | phi_out] is two entries longer than the plain one, d_nbad
    // is [nred].  d_J, d_sim, d_Jd, d_simd, d_ndown, d_b, d_bd belong to the set, not to the reduction: the launcher refuses them.
    int nred;
    const unsigned short* d_mult;          // [nrep][nobs]; NULL where every d_rep[r] is -1
    const int *d_set_of, *d_rep;           // [nred]; each may be NULL
    int* d_counts;                         // [nred][4]: nuse, nuse_d, nheld, ndown
};
static inline int ucf_fit_reduce_is_resampled(const ucf_fit_reduce_args* a) { return a->nred > 0; }
static inline int ucf_fit_reduce_is_robust(const ucf_fit_reduce_args* a) { return a->loss != 0 || a->d_ndown || a->d_b || a->d_bd; }
// where the launch of `a` writes its sums: by the predicates that choose its instantiation (launch_source, ucf_fit.hip)
static inline ucf_fit_sums_layout ucf_fit_sums_of(const ucf_fit_reduce_args* a)
{
    return ucf_fit_sums(a->npar, a->d_dh != NULL, ucf_fit_reduce_is_robust(a) != 0, ucf_fit_reduce_is_resampled(a) != 0);
}

int ucf_fit_launch_reduce(const ucf_fit_reduce_args* a, void* stream);
