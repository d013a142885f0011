// ucf_field_ensemble.hip -- the reduction of an ensemble of well-field maps over its member axis (ucf_field_ensemble and
// ucf_field_ensemble_weighted, include/ucf.h): per output e of a [nens][nout] the number of members in F(e), their mean,
// standard deviation, extremes, exceedance fractions (moments_body) and quantiles (quantile_body), each written once for
// both forms.  WEIGHTED = false: every member has mass 1, and masses add up in an int.  WEIGHTED = true: member m has mass
// u[m], the integer weights of ucf_ensemble_quantise, 0 .. 2^32, and u = 0 means not in the ensemble; u[m] is read at a
// wave-uniform address (m is a loop counter): scalar loads, no LDS.  Every sum of weights is a 64-bit integer of at most
// 1024 * 2^32 = 2^42: exact, whatever the order, and exact again as a double.
//
// Built with -ffp-contract=off like ucf_field.hip: every sum, product and quotient below is rounded on its own, so the
// result is the arithmetic that include/ucf.h states.  One thread (moments) or one group of threads that meet only through
// LDS and barriers (quantiles) owns an output; members are taken in member order: no floating-point atomics, a call repeated
// gives the same bits.  Members that are not finite are left out; the Wynn sentinel is finite and takes part.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int ENS_THREADS = 256;
constexpr int ENS_OWN = 4;                  // members a thread of the quantile kernels takes per pass over the tile

typedef unsigned long long u64;
template <bool WEIGHTED>
using ens_mass = std::conditional_t<WEIGHTED, u64, int>;
// the mass of member m: 1, or its weight (an int and no read of u, or a 64-bit integer: so are all sums of masses)
template <bool WEIGHTED>
__device__ __forceinline__ ens_mass<WEIGHTED> mass_of(const u64* __restrict__ u, int m)
{
    if constexpr (WEIGHTED) return u[m]; else return 1;
}

// One thread per output e; neighbouring threads read neighbouring doubles of one member row.  Two passes over the nens
// values of the output (the second one finds them in the cache): sum, mass, extremes and exceedance masses, then the squared
// deviations.  The exceedance masses live in registers: the loop over UCF_ENSEMBLE_MAX_Q unrolls, limits beyond nlim are
// never read.  limit is read at wave-uniform addresses.  WEIGHTED: a member with u = 0 is skipped by a wave-uniform branch,
// its value is not loaded.  The unweighted instantiation holds no weight arithmetic and does not read u.
template <bool WEIGHTED>
__device__ __forceinline__ void moments_body(int nens, long long nout, const double* __restrict__ a, const u64* __restrict__ u, int nlim,
                                             const double* __restrict__ limit, double* __restrict__ mean, double* __restrict__ sd,
                                             double* __restrict__ mn, double* __restrict__ mx, int* __restrict__ nfin,
                                             double* __restrict__ pexc, u64* __restrict__ nbad)
{
    const long long e = (long long)blockIdx.x * ENS_THREADS + threadIdx.x;
    bool bad = false;
    if (e < nout) {
        const size_t no = (size_t)nout;
        double lim[UCF_ENSEMBLE_MAX_Q];
        ens_mass<WEIGHTED> over[UCF_ENSEMBLE_MAX_Q];
#pragma unroll
        for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) {
            lim[l] = (pexc && l < nlim) ? limit[l] : 0.0;
            over[l] = 0;
        }
        const double nan = __builtin_nan("");
        double acc = 0.0, U2 = 0.0, lo = nan, hi = nan;
        u64 U = 0;
        int n = 0, nmem = 0;                             // nmem: the members of the ensemble (u > 0), the same in every thread
        for (int m = 0; m < nens; m++) {
            const ens_mass<WEIGHTED> um = mass_of<WEIGHTED>(u, m);
            if constexpr (WEIGHTED) {
                if (um == 0) continue;
                nmem++;
            }
            const double v = a[(size_t)m * no + e];
            if (!isfinite(v)) continue;
            if constexpr (WEIGHTED) {
                const double du = (double)um;
                acc = acc + du * v;
                U2 = U2 + du * du;
                U += um;
            } else
                acc = acc + v;
            n++;
            if (!(v >= lo)) lo = v;                      // the first member of F, then v < lo
            if (!(v < hi)) hi = v;                       // the first member of F, then v >= hi
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) over[l] += (v > lim[l]) ? um : 0;
        }
        double dU;                                       // the mass of F: n, or U
        if constexpr (WEIGHTED) dU = (double)U; else dU = (double)n;
        const double mu = acc / dU;                      // n = 0: +0.0 / +0.0 = NaN
        bad = n < (WEIGHTED ? nmem : nens);
        if (mean) mean[e] = mu;
        if (mn) mn[e] = lo;
        if (mx) mx[e] = hi;
        if (nfin) nfin[e] = n;
        if (sd) {
            double ss = 0.0;
            for (int m = 0; m < nens; m++) {
                const ens_mass<WEIGHTED> um = mass_of<WEIGHTED>(u, m);
                if (um == 0) continue;
                const double v = a[(size_t)m * no + e];
                if (!isfinite(v)) continue;
                const double d = v - mu;
                if constexpr (WEIGHTED) ss = ss + (double)um * (d * d); else ss = ss + d * d;
            }
            if constexpr (WEIGHTED) {
                const double den = dU - U2 / dU;         // the reliability-weights estimator
                sd[e] = (n < 2 || !(den > 0.0)) ? nan : sqrt(ss / den);
            } else
                sd[e] = (n < 2) ? nan : sqrt(ss / (double)(n - 1));
        }
        if (pexc) {
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++)
                if (l < nlim) pexc[(size_t)l * no + e] = (double)over[l] / dU;
        }
    }
    // every lane of every wave arrives here (no early return above)
    const u64 b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(nbad, (u64)__popcll(b));
}

__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_moments_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                              int nlim, const double* __restrict__ limit,
                                                                              double* __restrict__ mean, double* __restrict__ sd,
                                                                              double* __restrict__ mn, double* __restrict__ mx,
                                                                              int* __restrict__ nfin, double* __restrict__ pexc,
                                                                              unsigned long long* __restrict__ nbad)
{
    moments_body<false>(nens, nout, a, nullptr, nlim, limit, mean, sd, mn, mx, nfin, pexc, nbad);
}

__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_wmoments_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                               const unsigned long long* __restrict__ u, int nlim,
                                                                               const double* __restrict__ limit, double* __restrict__ mean,
                                                                               double* __restrict__ sd, double* __restrict__ mn,
                                                                               double* __restrict__ mx, int* __restrict__ nfin,
                                                                               double* __restrict__ pexc, unsigned long long* __restrict__ nbad)
{
    moments_body<true>(nens, nout, a, u, nlim, limit, mean, sd, mn, mx, nfin, pexc, nbad);
}

// The unweighted result of a level at pos = p (n - 1), from the landing places land [2][UCF_ENSEMBLE_MAX_Q][T] of x_k and
// x_{k+1}: x_k + g (x_{k+1} - x_k), or x_(n-1) where k >= n - 1
template <int T>
__device__ __forceinline__ double interpolate_ranks(const double* land, int j, int l, int n, double pos)
{
    double out = __builtin_nan("");
    if (n > 0) {
        const double fl = floor(pos);
        const int k = (int)fl;
        const double x0 = land[l * T + j];
        if (k >= n - 1) out = x0;
        else {
            const double gq = pos - fl;
            out = x0 + gq * (land[(UCF_ENSEMBLE_MAX_Q + l) * T + j] - x0);
        }
    }
    return out;
}

// Quantiles.  A workgroup stages the tile [nens][T] of T neighbouring outputs in LDS (coalesced reads of T doubles per
// member row; a member that is not in F(e) -- not finite, or u = 0 -- and an output beyond nout is staged as NaN, which
// compares false with everything and so drops out of every sum below).  Thread tid works on output tid % T -- neighbouring
// lanes, neighbouring doubles of a tile row: 8-byte LDS reads on distinct banks, lanes of the same output (T < 64) read one
// address -- and, with the ENS_THREADS / T threads of that output, shares its members: ENS_OWN consecutive members per thread
// and pass.  Every pass walks all rows of the tile at wave-uniform row addresses and accumulates, without a branch,
// E(m) = the mass of the m' with v' < v or (v' == v and m' < m): what lies in front of member m in the stable order, its
// rank where masses are 1.  Level p lies at pos = p (n - 1), weighted at p U, and the members that the form's rule selects
// leave their values in the landing places behind the tile; after a barrier one thread per (level, output) forms the result.
// Unweighted (the `linear` rule on the stable order): the members of rank k = floor(pos) and k + 1 land in two places per
// level, the result interpolates between them.  Weighted (the inverse of the weighted empirical distribution function): the
// intervals (E(m), E(m) + u[m]] of the staged members partition (0, U], so exactly one member has E < pos <= E + u (E == 0
// where pos == 0); it lands in the one place of the level, and that value is the result -- no interpolation; ties have one
// value, so the stable order only decides which of -0.0 and +0.0 a tie returns.
// LDS, dynamic: (nens + 2 UCF_ENSEMBLE_MAX_Q) T doubles, weighted (nens + UCF_ENSEMBLE_MAX_Q) T.
template <int T, bool WEIGHTED>
__device__ __forceinline__ void quantile_body(int nens, long long nout, const double* __restrict__ a, const u64* __restrict__ u, int nq,
                                              const double* __restrict__ q, double* __restrict__ quant)
{
    extern __shared__ double ens_lds[];
    constexpr int G = ENS_THREADS / T;                   // threads per output
    double* tile = ens_lds;                              // [nens][T]
    double* land = ens_lds + (size_t)nens * T;           // [2][UCF_ENSEMBLE_MAX_Q][T]: x_k and x_{k+1} of every level; weighted [1]
    const int j = threadIdx.x % T, g = threadIdx.x / T;
    const long long e0 = (long long)blockIdx.x * T;
    const long long e = e0 + j;
    const size_t no = (size_t)nout;
    const double nan = __builtin_nan("");
    for (int m = g; m < nens; m += G) {
        double v = nan;
        if (e < nout && mass_of<WEIGHTED>(u, m) != 0) v = a[(size_t)m * no + e];
        tile[m * T + j] = isfinite(v) ? v : nan;
    }
    __syncthreads();
    // the mass of F of this thread's output (n, or U): every thread of the output adds the same rows, an integer sum
    ens_mass<WEIGHTED> tot = 0;
    for (int m = 0; m < nens; m++) tot += (tile[m * T + j] == tile[m * T + j]) ? mass_of<WEIGHTED>(u, m) : 0;
    const double span = WEIGHTED ? (double)tot : (double)(tot - 1);      // level p lies at p * span
    for (int base = g * ENS_OWN; base < nens; base += G * ENS_OWN) {
        double v[ENS_OWN];
        ens_mass<WEIGHTED> E[ENS_OWN], uo[ENS_OWN];      // uo: the masses of the thread's own members (the weighted rule reads them)
#pragma unroll
        for (int i = 0; i < ENS_OWN; i++) {
            v[i] = (base + i < nens) ? tile[(base + i) * T + j] : nan;
            uo[i] = 1;
            if constexpr (WEIGHTED) uo[i] = (base + i < nens) ? u[base + i] : 0ULL;
            E[i] = 0;
        }
        for (int m = 0; m < nens; m++) {
            const double w = tile[m * T + j];
            const ens_mass<WEIGHTED> um = mass_of<WEIGHTED>(u, m);
#pragma unroll
            for (int i = 0; i < ENS_OWN; i++) E[i] += ((w < v[i]) | ((w == v[i]) & (m < base + i))) ? um : 0;
        }
        for (int l = 0; l < nq; l++) {
            const double pos = q[l] * span;
            if constexpr (WEIGHTED) {
#pragma unroll
                for (int i = 0; i < ENS_OWN; i++) {
                    const bool in = ((double)E[i] < pos) & (pos <= (double)(E[i] + uo[i]));
                    const bool first = (pos == 0.0) & (E[i] == 0);
                    if (v[i] == v[i] && (in | first)) land[l * T + j] = v[i];
                }
            } else {
                int k = (int)floor(pos);
                if (k >= tot - 1) k = tot - 1;
#pragma unroll
                for (int i = 0; i < ENS_OWN; i++)
                    if (v[i] == v[i]) {
                        if (E[i] == k) land[l * T + j] = v[i];
                        if (E[i] == k + 1) land[(UCF_ENSEMBLE_MAX_Q + l) * T + j] = v[i];
                    }
            }
        }
    }
    __syncthreads();
    if (e >= nout) return;
    for (int l = g; l < nq; l += G) {
        if constexpr (WEIGHTED) quant[(size_t)l * no + e] = (tot > 0) ? land[l * T + j] : nan;
        else quant[(size_t)l * no + e] = interpolate_ranks<T>(land, j, l, tot, q[l] * span);
    }
}

template <int T>
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_quantile_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                               int nq, const double* __restrict__ q,
                                                                               double* __restrict__ quant)
{
    quantile_body<T, false>(nens, nout, a, nullptr, nq, q, quant);
}

template <int T>
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_wquantile_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                                const unsigned long long* __restrict__ u, int nq,
                                                                                const double* __restrict__ q, double* __restrict__ quant)
{
    quantile_body<T, true>(nens, nout, a, u, nq, q, quant);
}

template <int T>
void quantile_launch(const ucf_ensemble_reduce_args* a, hipStream_t st)
{
    const size_t lds = sizeof(double) * ((size_t)a->nens + (a->d_u ? 1 : 2) * UCF_ENSEMBLE_MAX_Q) * T;
    const void* kernel = a->d_u ? (const void*)field_ensemble_wquantile_kernel<T> : (const void*)field_ensemble_quantile_kernel<T>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 blocks((unsigned)((a->nout + T - 1) / T));
    if (a->d_u)
        hipLaunchKernelGGL(field_ensemble_wquantile_kernel<T>, blocks, dim3(ENS_THREADS), lds, st, a->nens, a->nout, a->d_a, a->d_u, a->nq, a->d_q, a->d_quant);
    else
        hipLaunchKernelGGL(field_ensemble_quantile_kernel<T>, blocks, dim3(ENS_THREADS), lds, st, a->nens, a->nout, a->d_a, a->nq, a->d_q, a->d_quant);
}
}  // namespace

int ucf_field_ensemble_tile(int nens) { return nens <= 256 ? 64 : nens <= 512 ? 32 : 16; }

int ucf_field_launch_ensemble_reduce(const ucf_ensemble_reduce_args* a, void* stream)
{
    if (!a || a->nens < 1 || a->nens > UCF_ENSEMBLE_MAX || a->nout < 1 || !a->d_a || !a->d_nbad || a->nlim < 0 || a->nlim > UCF_ENSEMBLE_MAX_Q ||
        (a->d_pexc && (a->nlim < 1 || !a->d_limit)) || (a->d_quant && (a->nq < 1 || a->nq > UCF_ENSEMBLE_MAX_Q || !a->d_q))) return UCF_ERR_BAD_ARGUMENT;
    // the grids: the quantile kernel's is the larger one (T <= 64 < ENS_THREADS)
    const int T = a->d_quant ? ucf_field_ensemble_tile(a->nens) : ENS_THREADS;
    if ((a->nout + T - 1) / T > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    const dim3 blocks((unsigned)((a->nout + ENS_THREADS - 1) / ENS_THREADS));
    if (a->d_u)
        hipLaunchKernelGGL(field_ensemble_wmoments_kernel, blocks, dim3(ENS_THREADS), 0, st, a->nens, a->nout, a->d_a, a->d_u, a->nlim, a->d_limit,
                           a->d_mean, a->d_sd, a->d_min, a->d_max, a->d_nfin, a->d_pexc, (u64*)a->d_nbad);
    else
        hipLaunchKernelGGL(field_ensemble_moments_kernel, blocks, dim3(ENS_THREADS), 0, st, a->nens, a->nout, a->d_a, a->nlim, a->d_limit,
                           a->d_mean, a->d_sd, a->d_min, a->d_max, a->d_nfin, a->d_pexc, (u64*)a->d_nbad);
    if (hipGetLastError() != hipSuccess) return UCF_ERR_HIP;
    if (!a->d_quant) return UCF_OK;
    switch (T) {
    case 64: quantile_launch<64>(a, st); break;
    case 32: quantile_launch<32>(a, st); break;
    default: quantile_launch<16>(a, st); break;
    }
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
