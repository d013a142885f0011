// ucf_fit.hip -- residuals, objective, central-difference Jacobian and normal equations of a least-squares fit, from the
// drawdowns that the evaluators left in device memory (ucf_fit_evaluate, include/ucf.h).  Three kernels over one body:
// fit_reduce_kernel (ucf_fit_create: one double per observation and plan), fit_network_reduce_kernel
// (ucf_fit_create_network: ragged per-group h, point observations and screen averages) and fit_field_reduce_kernel
// (ucf_fit_create_field: an observation is the sum over pumping wells of rate factor x such a value).
//
// Tiny and HBM-bound: (1 + 2 NPAR) x nobs doubles per parameter set are read once.  Built with -ffp-contract=off: every
// product and sum below is rounded on its own, so that the result is the arithmetic written here.  The sums are reduced in
// a FIXED order -- per lane over its observations in ascending order, a butterfly over the 64 lanes of a wave, the four
// waves in wave order from LDS, one lane writes -- and without floating-point atomics: a repeated call gives the same bits.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_fit.h"

namespace {
constexpr int FIT_THREADS = 256;
constexpr int FIT_WAVES = FIT_THREADS / 64;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);     // every lane ends with the same bits
    return v;
}

// Everything after the simulated values: value(i, plan) is the dimensional simulated value of observation i under plan
// `plan`; the two kernels below differ only in it.
template <int NPAR, class VALUE>
__device__ __forceinline__ void fit_reduce_body(int nobs, double two_dlog, const VALUE& value, const double* __restrict__ obs,
                                                const double* __restrict__ w, double* __restrict__ sums, int* __restrict__ nbad,
                                                double* __restrict__ J, double* __restrict__ sim)
{
    constexpr int NP = NPAR > 0 ? NPAR : 1;                  // array extents (NPAR = 0: objective only)
    constexpr int NPLANS = 1 + 2 * NPAR;
    constexpr int NSUMS = 1 + NPAR + NPAR * (NPAR + 1) / 2;
    __shared__ double part[FIT_WAVES][NSUMS];
    __shared__ int part_bad[FIT_WAVES];
    const int set = blockIdx.x, lane = threadIdx.x;
    const size_t plan0 = (size_t)set * NPLANS;
    double phi = 0.0, g[NP], A[NP * (NP + 1) / 2];
#pragma unroll
    for (int j = 0; j < NP; j++) g[j] = 0.0;
#pragma unroll
    for (int j = 0; j < NP * (NP + 1) / 2; j++) A[j] = 0.0;
    int bad = 0;
    for (int i = lane; i < nobs; i += FIT_THREADS) {
        double s[NPLANS];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NPLANS; k++) {
            s[k] = value(i, plan0 + k);
            ok = ok && isfinite(s[k]);
        }
        if (sim) {
#pragma unroll
            for (int k = 0; k < NPLANS; k++) sim[(plan0 + k) * (size_t)nobs + i] = s[k];
        }
        double d[NP];
#pragma unroll
        for (int j = 0; j < NPAR; j++) d[j] = (s[1 + 2 * j] - s[2 + 2 * j]) / two_dlog;
        if (J) {
#pragma unroll
            for (int j = 0; j < NPAR; j++) J[((size_t)set * nobs + i) * NPAR + j] = d[j];
        }
        if (!ok) { bad++; continue; }
        const double wi = w[i];
        const double wr = wi * (obs[i] - s[0]);
        phi = phi + wr * wr;
        double wd[NP];
#pragma unroll
        for (int j = 0; j < NPAR; j++) { wd[j] = wi * d[j]; g[j] = g[j] + wd[j] * wr; }
        int q = 0;
#pragma unroll
        for (int j = 0; j < NPAR; j++)
#pragma unroll
            for (int k = j; k < NPAR; k++) { A[q] = A[q] + wd[j] * wd[k]; q++; }
    }
    // wave butterfly, then the waves in order
    const int wave = lane >> 6;
    phi = wave_sum(phi);
#pragma unroll
    for (int j = 0; j < NPAR; j++) g[j] = wave_sum(g[j]);
#pragma unroll
    for (int j = 0; j < NPAR * (NPAR + 1) / 2; j++) A[j] = wave_sum(A[j]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if ((lane & 63) == 0) {
        part[wave][0] = phi;
#pragma unroll
        for (int j = 0; j < NPAR; j++) part[wave][1 + j] = g[j];
#pragma unroll
        for (int j = 0; j < NPAR * (NPAR + 1) / 2; j++) part[wave][1 + NPAR + j] = A[j];
        part_bad[wave] = bad;
    }
    __syncthreads();
    if (lane == 0) {
        for (int j = 0; j < NSUMS; j++) {
            double v = part[0][j];
            for (int k = 1; k < FIT_WAVES; k++) v = v + part[k][j];
            sums[(size_t)set * NSUMS + j] = v;
        }
        int b = 0;
        for (int k = 0; k < FIT_WAVES; k++) b += part_bad[k];
        nbad[set] = b;
    }
}

// observation i = one double per plan, at slot[i] of the plan's block
struct slot_value {
    const double* __restrict__ h;
    const double* __restrict__ Hc;
    const int* __restrict__ slot;
    size_t plan_stride;
    __device__ __forceinline__ double operator()(int i, size_t plan) const
    {
        return h[plan * plan_stride + slot[i]] * Hc[plan];      // dimensional, as ucf_drawdown_multi scales it
    }
};

// `o.count` consecutive depths of one point in the ragged per-group h of a network: one value, or the screen average over
// the well's depths in the operation order of ucf_screen_average (driver.f90:234-243, quirk Q2); dimensionless
__device__ __forceinline__ double network_h(const double* __restrict__ h, const ucf_fit_obs_ref o, size_t nplans, size_t plan)
{
    const double* v = h + ((size_t)o.prefix * nplans + plan * (size_t)o.stride + (size_t)o.at);
    const int n = o.count;
    if (n == 1) return v[0];
    double s = v[1];
    for (int j = 2; j < n; j++) s = s + v[j];
    return ((v[0] + 2.0 * s) + v[n - 1]) / (2 * n);
}

// observation i of a network = network_h at ref[i], formed on the dimensionless h and then scaled
struct network_value {
    const double* __restrict__ h;
    const double* __restrict__ Hc;
    const ucf_fit_obs_ref* __restrict__ ref;
    size_t nplans;
    __device__ __forceinline__ double operator()(int i, size_t plan) const
    {
        return network_h(h, ref[i], nplans, plan) * Hc[plan];
    }
};

// observation i of a field fit = the terms first[i] .. first[i + 1], one per pumping well that has started, in the
// caller's order of pumping wells: acc = +0.0; acc = acc + q * network_h(term); then x Hc.  Every operation is rounded on
// its own; nothing is scrubbed, so a term that is not finite makes the observation not finite.
struct field_value {
    const double* __restrict__ h;
    const double* __restrict__ Hc;
    const ucf_fit_term* __restrict__ term;
    const int* __restrict__ first;
    size_t nplans;
    __device__ __forceinline__ double operator()(int i, size_t plan) const
    {
        double acc = 0.0;
        const int end = first[i + 1];
        for (int k = first[i]; k < end; k++) acc = acc + term[k].q * network_h(h, term[k].ref, nplans, plan);
        return acc * Hc[plan];
    }
};

template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_reduce_kernel(int nobs, size_t plan_stride, double two_dlog, const double* __restrict__ h,
                                                                 const double* __restrict__ Hc, const int* __restrict__ slot,
                                                                 const double* __restrict__ obs, const double* __restrict__ w,
                                                                 double* __restrict__ sums, int* __restrict__ nbad, double* __restrict__ J,
                                                                 double* __restrict__ sim)
{
    fit_reduce_body<NPAR>(nobs, two_dlog, slot_value{h, Hc, slot, plan_stride}, obs, w, sums, nbad, J, sim);
}

template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_network_reduce_kernel(int nobs, size_t nplans, double two_dlog, const double* __restrict__ h,
                                                                         const double* __restrict__ Hc,
                                                                         const ucf_fit_obs_ref* __restrict__ ref,
                                                                         const double* __restrict__ obs, const double* __restrict__ w,
                                                                         double* __restrict__ sums, int* __restrict__ nbad,
                                                                         double* __restrict__ J, double* __restrict__ sim)
{
    fit_reduce_body<NPAR>(nobs, two_dlog, network_value{h, Hc, ref, nplans}, obs, w, sums, nbad, J, sim);
}

template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_field_reduce_kernel(int nobs, size_t nplans, double two_dlog, const double* __restrict__ h,
                                                                       const double* __restrict__ Hc,
                                                                       const ucf_fit_term* __restrict__ term,
                                                                       const int* __restrict__ first, const double* __restrict__ obs,
                                                                       const double* __restrict__ w, double* __restrict__ sums,
                                                                       int* __restrict__ nbad, double* __restrict__ J,
                                                                       double* __restrict__ sim)
{
    fit_reduce_body<NPAR>(nobs, two_dlog, field_value{h, Hc, term, first, nplans}, obs, w, sums, nbad, J, sim);
}

template <int NPAR>
int launch_field(int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc, const ucf_fit_term* d_term,
                 const int* d_first, const double* d_obs, const double* d_w, double* d_sums, int* d_nbad, double* d_J, double* d_sim,
                 hipStream_t stream)
{
    hipLaunchKernelGGL(fit_field_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, nplans, two_dlog, d_h, d_Hc, d_term,
                       d_first, d_obs, d_w, d_sums, d_nbad, d_J, d_sim);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

template <int NPAR>
int launch_network(int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc, const ucf_fit_obs_ref* d_ref,
                   const double* d_obs, const double* d_w, double* d_sums, int* d_nbad, double* d_J, double* d_sim, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_network_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, nplans, two_dlog, d_h, d_Hc, d_ref,
                       d_obs, d_w, d_sums, d_nbad, d_J, d_sim);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

template <int NPAR>
int launch(int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_Hc, const int* d_slot,
           const double* d_obs, const double* d_w, double* d_sums, int* d_nbad, double* d_J, double* d_sim, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, plan_stride, two_dlog, d_h, d_Hc, d_slot,
                       d_obs, d_w, d_sums, d_nbad, d_J, d_sim);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
}  // namespace

int ucf_fit_launch_reduce(int npar, int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_Hc,
                          const int* d_slot, const double* d_obs, const double* d_w, double* d_sums, int* d_nbad, double* d_J,
                          double* d_sim, void* stream)
{
    if (nsets < 1 || nobs < 1) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch<N>(nsets, nobs, plan_stride, two_dlog, d_h, d_Hc, d_slot, d_obs, d_w, d_sums, d_nbad, d_J, d_sim, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}

int ucf_fit_launch_network_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc,
                                  const ucf_fit_obs_ref* d_ref, const double* d_obs, const double* d_w, double* d_sums, int* d_nbad,
                                  double* d_J, double* d_sim, void* stream)
{
    if (nsets < 1 || nobs < 1) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch_network<N>(nsets, nobs, nplans, two_dlog, d_h, d_Hc, d_ref, d_obs, d_w, d_sums, d_nbad, d_J, d_sim, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}

int ucf_fit_launch_field_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_Hc,
                                const ucf_fit_term* d_term, const int* d_first, const double* d_obs, const double* d_w, double* d_sums,
                                int* d_nbad, double* d_J, double* d_sim, void* stream)
{
    if (nsets < 1 || nobs < 1) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch_field<N>(nsets, nobs, nplans, two_dlog, d_h, d_Hc, d_term, d_first, d_obs, d_w, d_sums, d_nbad, d_J, d_sim, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}
