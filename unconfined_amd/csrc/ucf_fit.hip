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
//
// A fit with derivative data (ucf_fit_set_derivative) runs a second body, fit_reduce_joint_body, in three kernels of its
// own (fit_joint_reduce_kernel, fit_network_joint_reduce_kernel, fit_field_joint_reduce_kernel): it reads the dh array
// that the evaluators wrote beside h, in the same layout, and adds the terms of the log-time derivative to the same sums.
// The body above it and its kernels are what a fit without derivative data launches, unchanged.
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

// The joint body: the drawdown term of fit_reduce_body, operation for operation, then -- where the derivative weight wd_i
// is positive -- the same term formed from the simulated log-time derivative dvalue(i, plan) against dobs_i, added to the
// same accumulators (phi_d keeps the derivative's share of phi).  One rule decides whether an observation counts: every
// s[k] finite AND (wd_i == 0 OR every sd[k] finite); with all wd = 0 it is the rule above and the sums have the same bits.
// sums per set: phi | g | upper A | phi_d.  The weighted drawdown residual and derivatives are formed before sd is read,
// so that s[] is dead by then.
template <int NPAR, class VALUE, class DVALUE>
__device__ __forceinline__ void fit_reduce_joint_body(int nobs, double two_dlog, const VALUE& value, const DVALUE& dvalue,
                                                      const double* __restrict__ obs, const double* __restrict__ w,
                                                      const double* __restrict__ dobs, const double* __restrict__ wdv,
                                                      double* __restrict__ sums, int* __restrict__ nbad, double* __restrict__ J,
                                                      double* __restrict__ sim, double* __restrict__ Jd, double* __restrict__ simd)
{
    constexpr int NP = NPAR > 0 ? NPAR : 1;                  // array extents (NPAR = 0: objective only)
    constexpr int NPLANS = 1 + 2 * NPAR;
    constexpr int NA = NPAR * (NPAR + 1) / 2;
    constexpr int NSUMS = 1 + NPAR + NA + 1;
    __shared__ double part[FIT_WAVES][NSUMS];
    __shared__ int part_bad[FIT_WAVES];
    const int set = blockIdx.x, lane = threadIdx.x;
    const size_t plan0 = (size_t)set * NPLANS;
    double phi = 0.0, phi_d = 0.0, g[NP], A[NP * (NP + 1) / 2];
#pragma unroll
    for (int j = 0; j < NP; j++) g[j] = 0.0;
#pragma unroll
    for (int j = 0; j < NP * (NP + 1) / 2; j++) A[j] = 0.0;
    int bad = 0;
    for (int i = lane; i < nobs; i += FIT_THREADS) {
        bool ok = true;
        double wr, wd[NP];
        {
            double s[NPLANS];
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
            const double wi = w[i];
            wr = wi * (obs[i] - s[0]);
#pragma unroll
            for (int j = 0; j < NPAR; j++) wd[j] = wi * d[j];
        }
        const double wdi = wdv[i];
        double sd0, dd[NP];
        {
            double sd[NPLANS];
            bool okd = true;
#pragma unroll
            for (int k = 0; k < NPLANS; k++) {
                sd[k] = dvalue(i, plan0 + k);
                okd = okd && isfinite(sd[k]);
            }
            if (simd) {
#pragma unroll
                for (int k = 0; k < NPLANS; k++) simd[(plan0 + k) * (size_t)nobs + i] = sd[k];
            }
#pragma unroll
            for (int j = 0; j < NPAR; j++) dd[j] = (sd[1 + 2 * j] - sd[2 + 2 * j]) / two_dlog;
            if (Jd) {
#pragma unroll
                for (int j = 0; j < NPAR; j++) Jd[((size_t)set * nobs + i) * NPAR + j] = dd[j];
            }
            sd0 = sd[0];
            ok = ok && (wdi == 0.0 || okd);
        }
        if (!ok) { bad++; continue; }
        // the drawdown term
        phi = phi + wr * wr;
#pragma unroll
        for (int j = 0; j < NPAR; j++) g[j] = g[j] + wd[j] * wr;
        int q = 0;
#pragma unroll
        for (int j = 0; j < NPAR; j++)
#pragma unroll
            for (int k = j; k < NPAR; k++) { A[q] = A[q] + wd[j] * wd[k]; q++; }
        // the derivative term: skipped, not added as zero, where it has no weight
        if (wdi > 0.0) {
            const double wrd = wdi * (dobs[i] - sd0);
            phi = phi + wrd * wrd;
            phi_d = phi_d + wrd * wrd;
            double wdd[NP];
#pragma unroll
            for (int j = 0; j < NPAR; j++) { wdd[j] = wdi * dd[j]; g[j] = g[j] + wdd[j] * wrd; }
            q = 0;
#pragma unroll
            for (int j = 0; j < NPAR; j++)
#pragma unroll
                for (int k = j; k < NPAR; k++) { A[q] = A[q] + wdd[j] * wdd[k]; q++; }
        }
    }
    // wave butterfly, then the waves in order
    const int wave = lane >> 6;
    phi = wave_sum(phi);
    phi_d = wave_sum(phi_d);
#pragma unroll
    for (int j = 0; j < NPAR; j++) g[j] = wave_sum(g[j]);
#pragma unroll
    for (int j = 0; j < NA; j++) A[j] = wave_sum(A[j]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if ((lane & 63) == 0) {
        part[wave][0] = phi;
#pragma unroll
        for (int j = 0; j < NPAR; j++) part[wave][1 + j] = g[j];
#pragma unroll
        for (int j = 0; j < NA; j++) part[wave][1 + NPAR + j] = A[j];
        part[wave][1 + NPAR + NA] = phi_d;
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

// the log-time derivative of a field observation: the terms of field_value on the dh array, each scaled by its tfac =
// t_i / (t_i - t0 of its pumping well) -- dh is t dh/dt in the well's OWN time -- in the operation order of
// field_superpose_kernel's ds: acc = +0.0; acc = acc + q * (tfac * v); then x Hc
struct field_dvalue {
    const double* __restrict__ dh;
    const double* __restrict__ Hc;
    const ucf_fit_term* __restrict__ term;
    const double* __restrict__ tfac;
    const int* __restrict__ first;
    size_t nplans;
    __device__ __forceinline__ double operator()(int i, size_t plan) const
    {
        double acc = 0.0;
        const int end = first[i + 1];
        for (int k = first[i]; k < end; k++) acc = acc + term[k].q * (tfac[k] * network_h(dh, term[k].ref, nplans, plan));
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

// the joint kernels: d_dh is the evaluators' dh, laid out as d_h
#define UCF_FIT_JOINT_IN const double* __restrict__ obs, const double* __restrict__ w, const double* __restrict__ dobs, const double* __restrict__ wd
#define UCF_FIT_JOINT_OUT double* __restrict__ sums, int* __restrict__ nbad, double* __restrict__ J, double* __restrict__ sim, double* __restrict__ Jd, double* __restrict__ simd
template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_joint_reduce_kernel(int nobs, size_t plan_stride, double two_dlog, const double* __restrict__ h,
                                                                       const double* __restrict__ dh, const double* __restrict__ Hc,
                                                                       const int* __restrict__ slot, UCF_FIT_JOINT_IN, UCF_FIT_JOINT_OUT)
{
    fit_reduce_joint_body<NPAR>(nobs, two_dlog, slot_value{h, Hc, slot, plan_stride}, slot_value{dh, Hc, slot, plan_stride}, obs, w, dobs, wd,
                                sums, nbad, J, sim, Jd, simd);
}

template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_network_joint_reduce_kernel(int nobs, size_t nplans, double two_dlog, const double* __restrict__ h,
                                                                               const double* __restrict__ dh, const double* __restrict__ Hc,
                                                                               const ucf_fit_obs_ref* __restrict__ ref, UCF_FIT_JOINT_IN,
                                                                               UCF_FIT_JOINT_OUT)
{
    fit_reduce_joint_body<NPAR>(nobs, two_dlog, network_value{h, Hc, ref, nplans}, network_value{dh, Hc, ref, nplans}, obs, w, dobs, wd, sums,
                                nbad, J, sim, Jd, simd);
}

template <int NPAR>
__global__ void __launch_bounds__(FIT_THREADS) fit_field_joint_reduce_kernel(int nobs, size_t nplans, double two_dlog, const double* __restrict__ h,
                                                                             const double* __restrict__ dh, const double* __restrict__ Hc,
                                                                             const ucf_fit_term* __restrict__ term,
                                                                             const double* __restrict__ tfac, const int* __restrict__ first,
                                                                             UCF_FIT_JOINT_IN, UCF_FIT_JOINT_OUT)
{
    fit_reduce_joint_body<NPAR>(nobs, two_dlog, field_value{h, Hc, term, first, nplans}, field_dvalue{dh, Hc, term, tfac, first, nplans}, obs, w,
                                dobs, wd, sums, nbad, J, sim, Jd, simd);
}
#undef UCF_FIT_JOINT_IN
#undef UCF_FIT_JOINT_OUT

template <int NPAR>
int launch_joint(int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_dh, const double* d_Hc,
                 const int* d_slot, const ucf_fit_joint_io& io, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_joint_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, plan_stride, two_dlog, d_h, d_dh, d_Hc,
                       d_slot, io.d_obs, io.d_w, io.d_dobs, io.d_wd, io.d_sums, io.d_nbad, io.d_J, io.d_sim, io.d_Jd, io.d_simd);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

template <int NPAR>
int launch_network_joint(int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh, const double* d_Hc,
                         const ucf_fit_obs_ref* d_ref, const ucf_fit_joint_io& io, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_network_joint_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, nplans, two_dlog, d_h, d_dh,
                       d_Hc, d_ref, io.d_obs, io.d_w, io.d_dobs, io.d_wd, io.d_sums, io.d_nbad, io.d_J, io.d_sim, io.d_Jd, io.d_simd);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

template <int NPAR>
int launch_field_joint(int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh, const double* d_Hc,
                       const ucf_fit_term* d_term, const double* d_tfac, const int* d_first, const ucf_fit_joint_io& io, hipStream_t stream)
{
    hipLaunchKernelGGL(fit_field_joint_reduce_kernel<NPAR>, dim3(nsets), dim3(FIT_THREADS), 0, stream, nobs, nplans, two_dlog, d_h, d_dh, d_Hc,
                       d_term, d_tfac, d_first, io.d_obs, io.d_w, io.d_dobs, io.d_wd, io.d_sums, io.d_nbad, io.d_J, io.d_sim, io.d_Jd,
                       io.d_simd);
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

int ucf_fit_launch_joint_reduce(int npar, int nsets, int nobs, size_t plan_stride, double two_dlog, const double* d_h, const double* d_dh,
                                const double* d_Hc, const int* d_slot, const ucf_fit_joint_io* io, void* stream)
{
    if (nsets < 1 || nobs < 1 || !io) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch_joint<N>(nsets, nobs, plan_stride, two_dlog, d_h, d_dh, d_Hc, d_slot, *io, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}

int ucf_fit_launch_network_joint_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh,
                                        const double* d_Hc, const ucf_fit_obs_ref* d_ref, const ucf_fit_joint_io* io, void* stream)
{
    if (nsets < 1 || nobs < 1 || !io) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch_network_joint<N>(nsets, nobs, nplans, two_dlog, d_h, d_dh, d_Hc, d_ref, *io, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}

int ucf_fit_launch_field_joint_reduce(int npar, int nsets, int nobs, size_t nplans, double two_dlog, const double* d_h, const double* d_dh,
                                      const double* d_Hc, const ucf_fit_term* d_term, const double* d_tfac, const int* d_first,
                                      const ucf_fit_joint_io* io, void* stream)
{
    if (nsets < 1 || nobs < 1 || !io) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
#define UCF_FIT_CASE(N) case N: return launch_field_joint<N>(nsets, nobs, nplans, two_dlog, d_h, d_dh, d_Hc, d_term, d_tfac, d_first, *io, s)
    switch (npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}
