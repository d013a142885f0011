// ucf_fit.hip -- residuals, objective, central-difference Jacobian and normal equations of a least-squares fit, from the
// drawdowns that the evaluators left in device memory (ucf_fit_evaluate, include/ucf.h).  One kernel template over one
// body, fit_reduce_kernel<NPAR, SOURCE, DERIV, MODE>, behind one launcher (ucf_fit_launch_reduce, ucf_fit.h):
//   SOURCE  how observation i finds its simulated value in h and its log-time derivative in dh: slot_source
//           (ucf_fit_create: one double per observation and plan), network_source (ucf_fit_create_network: ragged per-group
//           h, point observations and screen averages) or field_source (ucf_fit_create_field: an observation is the sum
//           over pumping wells of rate factor x such a value);
//   DERIV   whether the fit has derivative data (ucf_fit_set_derivative).  It is a template parameter so that a fit
//           without them has no load of dh, no phi_d and no register for either;
//   MODE    FIT_L2, FIT_ROBUST or FIT_RESAMPLE.  ROBUST (the last two): a robust loss (ucf_fit_set_loss: Huber or Tukey, the
//           kind a wave-uniform argument) reweights the terms.  It is a template parameter so that a plain least-squares fit
//           has the arithmetic, the registers and the sums it had before a loss existed; the kind is an argument because the
//           two losses differ by one short branch that every lane of a launch takes alike, and a further template axis would
//           double the robust instantiations for nothing.  FIT_RESAMPLE (ucf_fit_set_resample) is the robust arithmetic
//           under integer multiplicities: a workgroup is a REDUCTION -- a parameter set and a replicate, both wave-uniform
//           -- and least squares runs as Huber with c = +inf, so that one mode serves every loss.  It is a mode of its own so
//           that the other two keep their arithmetic, registers and sums: every line it adds sits under `if constexpr`.
//
// Tiny and HBM-bound: (1 + 2 NPAR) x nobs doubles per parameter set are read once (twice with derivative data).  Built with
// -ffp-contract=off: every product and sum below is rounded on its own, so that the result is the arithmetic written here.
// The sums are reduced in a FIXED order -- per lane over its observations in ascending order, a butterfly over the 64 lanes
// of a wave, the four waves in wave order from LDS, one lane writes -- and without floating-point atomics: a repeated call
// gives the same bits.
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

// The robust loss of a launch and where its per-observation factors go (ROBUST instantiations only; passed by value)
struct fit_loss {
    int kind;                              // UCF_LOSS_HUBER or UCF_LOSS_TUKEY: the same in every lane
    double c;                              // > 0; +inf under Huber: every factor 1.0, the bits of least squares
    int* __restrict__ ndown;               // [nsets] counted residual terms with b < 1.0, or NULL
    double* __restrict__ b;                // [nsets][nobs] factor of the drawdown residual, NaN where not counted, or NULL
    double* __restrict__ bd;               // [nsets][nobs] the same of the derivative residual (NaN also where wd == 0), or NULL
};

// The replicates of a launch (FIT_RESAMPLE instantiations only; passed by value).  Reduction r = blockIdx.x
struct fit_resample {
    int nobs_row;                                  // entries per row of mult (= nobs)
    const unsigned short* __restrict__ mult;       // [nrep][nobs_row], or NULL: no reduction names a replicate
    const int* __restrict__ set_of;                // [nred] the parameter set whose plans r reads, or NULL: r
    const int* __restrict__ rep;                   // [nred] its replicate, -1: every multiplicity 1; or NULL: all -1
    int* __restrict__ counts;                      // [nred][4] nuse, nuse_d, nheld, ndown
};

// rho(x) and the IRLS factor b(x) of include/ucf.h (ucf_fit_loss_terms), every operation rounded on its own
__device__ __forceinline__ void loss_terms(int kind, double c, double x, double& rho, double& b)
{
    const double a = fabs(x);
    if (kind == UCF_LOSS_HUBER) {
        if (a <= c) { b = 1.0; rho = x * x; }
        else { b = c / a; rho = c * (2.0 * a - c); }
    } else {
        const double c2 = c * c, u = x / c;
        if (a < c) { const double v = 1.0 - u * u; b = v * v; rho = (c2 * (1.0 - b * v)) / 3.0; }
        else { b = 0.0; rho = c2 / 3.0; }
    }
}

// Everything after the simulated values.  src.value(h, i, plan) is the dimensionless simulated value of observation i
// under plan `plan`, src.dvalue(dh, i, plan) its log-time derivative; the kernels differ only in them.  Either is scaled
// by Hc[plan] here, as ucf_drawdown_multi scales it.  First the drawdown term; then, with DERIV and where the derivative
// weight wd_i is positive, the same term formed from dvalue against dobs_i, added to the same accumulators (phi_d keeps
// the derivative's share of phi).  One rule decides whether an observation counts: every s[k] finite AND (no DERIV OR
// wd_i == 0 OR every sd[k] finite); with all wd = 0 the sums have the bits of the reduction without DERIV.  sums per set:
// phi | g | upper A, with DERIV ... | phi_d.  The weighted drawdown residual and derivatives are formed before sd is read,
// so that s[] is dead by then.
// With ROBUST a residual term x (wr, wrd) with weighted derivatives wd_j adds rho(x) to phi (phi_d), b (x x) to phi_w,
// (b wd_j) x to g_j and (b wd_j) wd_k to A_jk: the Gauss-Newton / IRLS form, A stays positive semidefinite.  Same counting
// rule, same order; sums per set: phi | g | upper A | [phi_d] | phi_w.
// With RESAMPLE observation i has the multiplicity m of the reduction's replicate (include/ucf.h, ucf_fit_set_resample).  m == 0:
// held out -- where it counts, its squared residuals go to phi_out and it is one of nheld; nothing else.  m > 0: the robust
// term with rho and b scaled by fm = (double)m, which is exact for m == 1: the bits of the ROBUST instantiation.  nbad counts
// only observations with m > 0.  Outputs are indexed by the reduction; sums: phi | g | upper A | [phi_d] | phi_w | phi_out.
enum fit_mode { FIT_L2 = 0, FIT_ROBUST = 1, FIT_RESAMPLE = 2 };

template <int NPAR, class SOURCE, bool DERIV, int MODE>
__device__ __forceinline__ void fit_reduce_body(int nobs, double two_dlog, const SOURCE& src, const double* __restrict__ h,
                                                const double* __restrict__ dh, const double* __restrict__ Hc,
                                                const double* __restrict__ obs, const double* __restrict__ w,
                                                const double* __restrict__ dobs, const double* __restrict__ wdv,
                                                double* __restrict__ sums, int* __restrict__ nbad, double* __restrict__ J,
                                                double* __restrict__ sim, double* __restrict__ Jd, double* __restrict__ simd,
                                                const fit_loss& loss, const fit_resample& rs)
{
    constexpr bool ROBUST = MODE != FIT_L2, RESAMPLE = MODE == FIT_RESAMPLE;
    constexpr int NP = NPAR > 0 ? NPAR : 1;                  // array extents (NPAR = 0: objective only)
    constexpr int NPLANS = 1 + 2 * NPAR;
    constexpr int NA = NPAR * (NPAR + 1) / 2;
    constexpr ucf_fit_sums_layout AT = ucf_fit_sums(NPAR, DERIV, ROBUST, RESAMPLE);      // where the sums of a set go
    constexpr int NSUMS = AT.count;
    __shared__ double part[FIT_WAVES][NSUMS];
    __shared__ int part_bad[FIT_WAVES], part_down[FIT_WAVES];
    const int lane = threadIdx.x;
    // the workgroup's outputs go to `set`; its plans are those of `pset` (the same without RESAMPLE)
    const int set = blockIdx.x;
    int pset = set;
    const unsigned short* __restrict__ mrow = nullptr;       // NULL: every multiplicity 1
    if constexpr (RESAMPLE) {
        if (rs.set_of) pset = rs.set_of[set];
        const int r = rs.rep ? rs.rep[set] : -1;
        if (r >= 0 && rs.mult) mrow =rs.mult + (size_t)r * (size_t)rs.nobs_row;
    }
    const size_t plan0 = (size_t)pset * NPLANS;
    double phi = 0.0, phi_d = 0.0, phi_w = 0.0, phi_out = 0.0, g[NP], A[NP * (NP + 1) / 2];
    [[maybe_unused]] int nuse = 0, nuse_d = 0, nheld = 0;
#pragma unroll
    for (int j = 0; j < NP; j++) g[j] = 0.0;
#pragma unroll
    for (int j = 0; j < NP * (NP + 1) / 2; j++) A[j] = 0.0;
    int bad = 0, down = 0;
    for (int i = lane; i < nobs; i += FIT_THREADS) {
        bool ok = true;
        double wr, wd[NP];
        {
            double s[NPLANS];
#pragma unroll
            for (int k = 0; k < NPLANS; k++) {
                s[k] = src.value(h, i, plan0 + k) * Hc[plan0 + k];
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
        double wdi = 0.0, sd0 = 0.0, dd[NP];
        if constexpr (DERIV) {
            wdi = wdv[i];
            double sd[NPLANS];
            bool okd = true;
#pragma unroll
            for (int k = 0; k < NPLANS; k++) {
                sd[k] = src.dvalue(dh, i, plan0 + k) * Hc[plan0 + k];
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
        [[maybe_unused]] double fm = 1.0;
        if constexpr (RESAMPLE) {
            const int m = mrow ? (int)mrow[i] : 1;
            if (m == 0) {                  // held out: a cross-validation term where it counts, and nothing else
                if (ok) {
                    phi_out = phi_out + wr * wr;
                    if (DERIV && wdi > 0.0) { const double wrd = wdi * (dobs[i] - sd0); phi_out = phi_out + wrd * wrd; }
                    nheld++;
                }
                continue;
            }
            if (ok) { nuse += m; if (DERIV && wdi > 0.0) nuse_d += m; }
            fm = (double)m;
        }
        if (!ok) {
            bad++;
            if constexpr (ROBUST && !RESAMPLE) {
                if (loss.b) loss.b[(size_t)set * nobs + i] = __builtin_nan("");
                if (loss.bd) loss.bd[(size_t)set * nobs + i] = __builtin_nan("");
            }
            continue;
        }
        // Without DERIV the compiler sinks the loads of w[i] and obs[i] to here and, left alone, asks for one after the other
        // has arrived: both first (2 VMEM reads), then the arithmetic.  One memory round trip of a pass that has three.
        if constexpr (!DERIV) { __builtin_amdgcn_sched_group_barrier(0x20, 2, 0); __builtin_amdgcn_sched_group_barrier(0x2, 256, 0); }
        // the drawdown term
        int q = 0;
        if constexpr (ROBUST) {
            double rho, b;
            loss_terms(loss.kind, loss.c, wr, rho, b);
            if constexpr (RESAMPLE) { if (b < 1.0) down++; rho = fm * rho; b = fm * b; }      // counted once; fb = fm * b
            phi = phi + rho;
            phi_w = phi_w + b * (wr * wr);
            if constexpr (!RESAMPLE) {
                if (b < 1.0) down++;
                if (loss.b) loss.b[(size_t)set * nobs + i] = b;
            }
#pragma unroll
            for (int j = 0; j < NPAR; j++) {
                const double bw = b * wd[j];
                g[j] = g[j] + bw * wr;
#pragma unroll
                for (int k = j; k < NPAR; k++) { A[q] = A[q] + bw * wd[k]; q++; }
            }
        } else {
            phi = phi + wr * wr;
#pragma unroll
            for (int j = 0; j < NPAR; j++) g[j] = g[j] + wd[j] * wr;
#pragma unroll
            for (int j = 0; j < NPAR; j++)
#pragma unroll
                for (int k = j; k < NPAR; k++) { A[q] = A[q] + wd[j] * wd[k]; q++; }
        }
        // the derivative term: skipped, not added as zero, where it has no weight
        if (DERIV && wdi > 0.0) {
            const double wrd = wdi * (dobs[i] - sd0);
            double wdd[NP];
            q = 0;
            if constexpr (ROBUST) {
                double rho, b;
                loss_terms(loss.kind, loss.c, wrd, rho, b);
                if constexpr (RESAMPLE) { if (b < 1.0) down++; rho = fm * rho; b = fm * b; }
                phi = phi + rho;
                phi_d = phi_d + rho;
                phi_w = phi_w + b * (wrd * wrd);
                if constexpr (!RESAMPLE) {
                    if (b < 1.0) down++;
                    if (loss.bd) loss.bd[(size_t)set * nobs + i] = b;
                }
#pragma unroll
                for (int j = 0; j < NPAR; j++) wdd[j] = wdi * dd[j];
#pragma unroll
                for (int j = 0; j < NPAR; j++) {
                    const double bw = b * wdd[j];
                    g[j] = g[j] + bw * wrd;
#pragma unroll
                    for (int k = j; k < NPAR; k++) { A[q] = A[q] + bw * wdd[k]; q++; }
                }
            } else {
                phi = phi + wrd * wrd;
                phi_d = phi_d + wrd * wrd;
#pragma unroll
                for (int j = 0; j < NPAR; j++) { wdd[j] = wdi * dd[j]; g[j] = g[j] + wdd[j] * wrd; }
#pragma unroll
                for (int j = 0; j < NPAR; j++)
#pragma unroll
                    for (int k = j; k < NPAR; k++) { A[q] = A[q] + wdd[j] * wdd[k]; q++; }
            }
        } else if constexpr (ROBUST && !RESAMPLE) {
            if (loss.bd) loss.bd[(size_t)set * nobs + i] = __builtin_nan("");
        }
    }
    // wave butterfly, then the waves in order
    const int wave = lane >> 6;
    phi = wave_sum(phi);
    if constexpr (DERIV) phi_d = wave_sum(phi_d);
    if constexpr (ROBUST) phi_w = wave_sum(phi_w);
    if constexpr (RESAMPLE) phi_out = wave_sum(phi_out);
#pragma unroll
    for (int j = 0; j < NPAR; j++) g[j] = wave_sum(g[j]);
#pragma unroll
    for (int j = 0; j < NA; j++) A[j] = wave_sum(A[j]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if constexpr (ROBUST) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) down += __shfl_xor(down, m, 64);
    }
    if constexpr (RESAMPLE) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            nuse += __shfl_xor(nuse, m, 64); nuse_d += __shfl_xor(nuse_d, m, 64); nheld += __shfl_xor(nheld, m, 64);
        }
    }
    [[maybe_unused]] __shared__ int part_cnt[RESAMPLE ? FIT_WAVES : 1][3];
    if ((lane & 63) == 0) {
        part[wave][AT.phi] = phi;
#pragma unroll
        for (int j = 0; j < NPAR; j++) part[wave][AT.g + j] = g[j];
#pragma unroll
        for (int j = 0; j < NA; j++) part[wave][AT.A + j] = A[j];
        if constexpr (DERIV) part[wave][AT.phi_d] = phi_d;
        if constexpr (ROBUST) { part[wave][AT.phi_w] = phi_w; part_down[wave] = down; }
        if constexpr (RESAMPLE) {
            part[wave][AT.phi_out] = phi_out;
            part_cnt[wave][0] = nuse; part_cnt[wave][1] = nuse_d; part_cnt[wave][2] = nheld;
        }
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
        if constexpr (RESAMPLE) {
            int c[4] = {0, 0, 0, 0};
            for (int k = 0; k < FIT_WAVES; k++) { c[0] += part_cnt[k][0]; c[1] += part_cnt[k][1]; c[2] += part_cnt[k][2]; c[3] += part_down[k]; }
            for (int k = 0; k < 4; k++) rs.counts[(size_t)set * 4 + k] = c[k];
        } else if constexpr (ROBUST) {
            if (loss.ndown) {
                int d = 0;
                for (int k = 0; k < FIT_WAVES; k++) d += part_down[k];
                loss.ndown[set] = d;
            }
        }
    }
}

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

// The three sources.  Each is passed to the kernel by value and yields the dimensionless value of observation i under a
// plan from h and its log-time derivative from dh.

// ucf_fit_create: one double per plan, at slot[i] of the plan's block; the derivative by the same rule
struct slot_source {
    const int* __restrict__ slot;
    size_t plan_stride;
    __device__ __forceinline__ double value(const double* __restrict__ h, int i, size_t plan) const { return h[plan * plan_stride + slot[i]]; }
    __device__ __forceinline__ double dvalue(const double* __restrict__ dh, int i, size_t plan) const { return value(dh, i, plan); }
};

// ucf_fit_create_network: network_h at ref[i]; the derivative by the same rule
struct network_source {
    const ucf_fit_obs_ref* __restrict__ ref;
    size_t nplans;
    __device__ __forceinline__ double value(const double* __restrict__ h, int i, size_t plan) const { return network_h(h, ref[i], nplans, plan); }
    __device__ __forceinline__ double dvalue(const double* __restrict__ dh, int i, size_t plan) const { return value(dh, i, plan); }
};

// ucf_fit_create_field: the terms first[i] .. first[i + 1], one per pumping well that has started, in the caller's order of
// pumping wells: acc = +0.0; acc = acc + q * network_h(term).  Every operation is rounded on its own; nothing is scrubbed,
// so a term that is not finite makes the observation not finite.  The derivative takes the same terms on dh, each scaled by
// its tfac = t_i / (t_i - t0 of its pumping well) -- dh is t dh/dt in the well's OWN time -- in the operation order of
// field_superpose_kernel's ds: acc = +0.0; acc = acc + q * (tfac * v).
struct field_source {
    const ucf_fit_term* __restrict__ term;
    const double* __restrict__ tfac;       // not read without derivative data
    const int* __restrict__ first;
    size_t nplans;
    __device__ __forceinline__ double value(const double* __restrict__ h, int i, size_t plan) const
    {
        double acc = 0.0;
        const int end = first[i + 1];
        for (int k = first[i]; k < end; k++) acc = acc + term[k].q * network_h(h, term[k].ref, nplans, plan);
        return acc;
    }
    __device__ __forceinline__ double dvalue(const double* __restrict__ dh, int i, size_t plan) const
    {
        double acc = 0.0;
        const int end = first[i + 1];
        for (int k = first[i]; k < end; k++) acc = acc + term[k].q * (tfac[k] * network_h(dh, term[k].ref, nplans, plan));
        return acc;
    }
};

template <int NPAR, class SOURCE, bool DERIV, int MODE>
__global__ void __launch_bounds__(FIT_THREADS) fit_reduce_kernel(int nobs, double two_dlog, SOURCE src, const double* __restrict__ h,
                                                                 const double* __restrict__ dh, const double* __restrict__ Hc,
                                                                 const double* __restrict__ obs, const double* __restrict__ w,
                                                                 const double* __restrict__ dobs,
                                                                 const double* __restrict__ wd, double* __restrict__ sums,
                                                                 int* __restrict__ nbad, double* __restrict__ J, double* __restrict__ sim,
                                                                 double* __restrict__ Jd, double* __restrict__ simd, fit_loss loss,
                                                                 fit_resample rs)
{
    fit_reduce_body<NPAR, SOURCE, DERIV, MODE>(nobs, two_dlog, src, h, dh, Hc, obs, w, dobs, wd, sums, nbad, J, sim, Jd, simd, loss, rs);
}

template <int NPAR, class SOURCE, bool DERIV, int MODE>
int launch(const ucf_fit_reduce_args& a, const SOURCE& src, hipStream_t stream)
{
    // least squares with a factor asked for: Huber with c = +inf, whose every factor is 1.0 and whose sums have the bits of L2
    const fit_loss loss = {a.loss == UCF_LOSS_L2 ? (int)UCF_LOSS_HUBER : a.loss, a.loss == UCF_LOSS_L2 ? (double)INFINITY : a.loss_c, a.d_ndown,
                           a.d_b, a.d_bd};
    // one workgroup per parameter set, or with resampling per reduction (the struct is not read by the other modes)
    const fit_resample rs = {a.nobs, a.d_mult, a.d_set_of, a.d_rep, a.d_counts};
    hipLaunchKernelGGL((fit_reduce_kernel<NPAR, SOURCE, DERIV, MODE>), dim3(MODE == FIT_RESAMPLE ? a.nred : a.nsets), dim3(FIT_THREADS), 0, stream,
                       a.nobs, a.two_dlog, src, a.d_h, a.d_dh, a.d_Hc, a.d_obs, a.d_w, a.d_dobs, a.d_wd, a.d_sums, a.d_nbad, a.d_J, a.d_sim, a.d_Jd,
                       a.d_simd, loss, rs);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

template <class SOURCE, bool DERIV, int MODE>
int launch_npar(const ucf_fit_reduce_args& a, const SOURCE& src, hipStream_t stream)
{
#define UCF_FIT_CASE(N) case N: return launch<N, SOURCE, DERIV, MODE>(a, src, stream)
    switch (a.npar) {
        UCF_FIT_CASE(0); UCF_FIT_CASE(1); UCF_FIT_CASE(2); UCF_FIT_CASE(3); UCF_FIT_CASE(4);
        UCF_FIT_CASE(5); UCF_FIT_CASE(6); UCF_FIT_CASE(7); UCF_FIT_CASE(8);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_FIT_CASE
}

template <class SOURCE>
int launch_source(const ucf_fit_reduce_args& a, const SOURCE& src, hipStream_t stream)
{
    if (ucf_fit_reduce_is_resampled(&a))
        return a.d_dh ? launch_npar<SOURCE, true, FIT_RESAMPLE>(a, src, stream) : launch_npar<SOURCE, false, FIT_RESAMPLE>(a, src, stream);
    if (ucf_fit_reduce_is_robust(&a))
        return a.d_dh ? launch_npar<SOURCE, true, FIT_ROBUST>(a, src, stream) : launch_npar<SOURCE, false, FIT_ROBUST>(a, src, stream);
    return a.d_dh ? launch_npar<SOURCE, true, FIT_L2>(a, src, stream) : launch_npar<SOURCE, false, FIT_L2>(a, src, stream);
}
}  // namespace

int ucf_fit_launch_reduce(const ucf_fit_reduce_args* a, void* stream)
{
    if (!a || a->nsets < 1 || a->nobs < 1) return UCF_ERR_BAD_ARGUMENT;
    if (a->loss != UCF_LOSS_L2 && a->loss != UCF_LOSS_HUBER && a->loss != UCF_LOSS_TUKEY) return UCF_ERR_BAD_ARGUMENT;
    if (a->loss != UCF_LOSS_L2 && !(a->loss_c > 0.0 && a->loss_c < (double)INFINITY)) return UCF_ERR_BAD_ARGUMENT;
    if (a->d_bd && !a->d_dh) return UCF_ERR_BAD_ARGUMENT;
    if (a->nred < 0) return UCF_ERR_BAD_ARGUMENT;
    if (a->nred > 0) {
        // what belongs to a parameter set is not written per reduction; the counts are; identity set_of needs a set per reduction
        if (a->d_J || a->d_sim || a->d_Jd || a->d_simd || a->d_ndown || a->d_b || a->d_bd || !a->d_counts) return UCF_ERR_BAD_ARGUMENT;
        if (!a->d_set_of && a->nred > a->nsets) return UCF_ERR_BAD_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (a->source) {
    case UCF_FIT_SLOTS: return launch_source(*a, slot_source{a->d_slot, a->plan_stride}, s);
    case UCF_FIT_NETWORK: return launch_source(*a, network_source{a->d_ref, a->nplans}, s);
    case UCF_FIT_FIELD: return launch_source(*a, field_source{a->d_term, a->d_tfac, a->d_first, a->nplans}, s);
    default: return UCF_ERR_BAD_ARGUMENT;
    }
}
