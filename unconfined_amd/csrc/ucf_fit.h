// ucf_fit.h -- launcher of the fit reduction (ucf_fit.hip), called by ucf_fit_evaluate (ucf_api.cpp).
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
