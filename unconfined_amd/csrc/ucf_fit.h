// ucf_fit.h -- launcher of the fit reduction (ucf_fit.hip), called by ucf_fit_evaluate (ucf_fit.cpp).
#pragma once

// sums per parameter set: phi | g[npar] | upper triangle of A, row by row (j <= k)
static inline int ucf_fit_nsums(int npar) { return 1 + npar + npar * (npar + 1) / 2; }

// One 256-thread workgroup per parameter set.  npar >= 1: set s owns plans s*(1+2 npar) + (0 base | 1+2j: parameter j up |
// 2+2j: parameter j down); npar == 0: one plan per set, phi and nbad only.
//   d_h [nplans][plan_stride] dimensionless drawdown as the evaluators left it, d_Hc [nplans], d_slot [nobs] = place of
//   observation i inside one plan's block, d_obs, d_w [nobs];
//   d_sums [nsets][ucf_fit_nsums(npar)], d_nbad [nsets]; d_J [nsets][nobs][npar] and d_sim [nsets][1+2 npar][nobs] may be NULL.
int ucf_fit_launch_reduce(int npar, int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_Hc,
                          const int* d_slot, const double* d_obs, const double* d_w, double* d_sums, int* d_nbad, double* d_J,
                          double* d_sim, void* stream);

// Where an observation of a network fit (ucf_fit_create_network) finds its simulated value.  The h of a network is ragged:
// one region per group of wells with the same number of depths, group g at nplans * prefix_g doubles, plan k of it at
// k * stride_g (stride_g = points per plan x depths of the group, prefix_g = sum of the strides before it).  The
// observation reads `count` consecutive doubles at  prefix * nplans + plan * stride + at:  1 = that depth of its point,
// n > 1 = all n depths of its well, averaged by the rule of ucf_screen_average.
struct ucf_fit_obs_ref {
    long long prefix, stride;
    int at, count;
};

// as ucf_fit_launch_reduce (same sums, same order), observation i found through d_ref[i]; nplans = nsets * (1 + 2 npar)
int ucf_fit_launch_network_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc,
                                  const ucf_fit_obs_ref* d_ref, const double* d_obs, const double* d_w, double* d_sums, int* d_nbad,
                                  double* d_J, double* d_sim, void* stream);

// One term of an observation of a field fit (ucf_fit_create_field): the value that `ref` finds in the h of the network of
// virtual wells, times the rate factor q of its pumping well.
struct ucf_fit_term {
    ucf_fit_obs_ref ref;
    double q;
};

// as ucf_fit_launch_network_reduce, the simulated value of observation i being the sum of its terms
// d_term[d_first[i] .. d_first[i + 1]) in that order: acc = +0.0; acc = acc + q * (value at ref, dimensionless); acc x Hc.
// d_first [nobs + 1] ascending; an observation without terms is +0.0.
int ucf_fit_launch_field_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc,
                                const ucf_fit_term* d_term, const int* d_first, const double* d_obs, const double* d_w, double* d_sums,
                                int* d_nbad, double* d_J, double* d_sim, void* stream);

// ---- a fit with derivative data (ucf_fit_set_derivative): the joint reduction.  The kernels above and their launchers are
// what a fit without derivative data runs; these read the evaluators' dh (d_dh, laid out exactly as d_h) as well.
// sums per parameter set: phi | g[npar] | upper triangle of A | phi_d (the derivative terms' share of phi)
static inline int ucf_fit_joint_nsums(int npar) { return ucf_fit_nsums(npar) + 1; }

// what the three joint launchers share: d_obs, d_w, d_dobs, d_wd [nobs] (d_dobs[i] is read only where d_wd[i] > 0);
// d_sums [nsets][ucf_fit_joint_nsums(npar)], d_nbad [nsets]; d_J, d_Jd [nsets][nobs][npar] and d_sim, d_simd
// [nsets][1+2 npar][nobs] may each be NULL
struct ucf_fit_joint_io {
    const double *d_obs, *d_w, *d_dobs, *d_wd;
    double* d_sums;
    int* d_nbad;
    double *d_J, *d_sim, *d_Jd, *d_simd;
};

// as ucf_fit_launch_reduce; the simulated derivative of observation i is d_dh[plan * plan_stride + d_slot[i]] * d_Hc[plan]
int ucf_fit_launch_joint_reduce(int npar, int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_dh,
                                const double* d_Hc, const int* d_slot, const ucf_fit_joint_io* io, void* stream);
// as ucf_fit_launch_network_reduce; the derivative is found through the same d_ref[i] in d_dh (a screen is averaged by the same rule)
int ucf_fit_launch_network_joint_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh,
                                        const double* d_Hc, const ucf_fit_obs_ref* d_ref, const ucf_fit_joint_io* io, void* stream);
// as ucf_fit_launch_field_reduce; d_tfac [terms]: t_i / (t_i - t0) of each term; the derivative of observation i is
// acc = +0.0; acc = acc + q * (tfac * (value at ref in d_dh)); acc x Hc
int ucf_fit_launch_field_joint_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh,
                                      const double* d_Hc, const ucf_fit_term* d_term, const double* d_tfac, const int* d_first,
                                      const ucf_fit_joint_io* io, void* stream);
