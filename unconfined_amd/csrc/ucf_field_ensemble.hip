// ucf_field_ensemble.hip -- the reduction of an ensemble of well-field maps over its member axis (ucf_field_ensemble,
// include/ucf.h): per output e of a [nens][nout] the number of finite members, their mean, standard deviation, extremes,
// exceedance fractions (field_ensemble_moments_kernel) and order statistics (field_ensemble_quantile_kernel).
//
// Built with -ffp-contract=off like ucf_field.hip: every sum, product and quotient below is rounded on its own, so the
// result is the arithmetic that include/ucf.h states.  One thread (moments) or one group of threads that meet only through
// LDS and barriers (quantiles) owns an output; members are taken in member order: no floating-point atomics, a call repeated
// gives the same bits.  Members that are not finite are left out; the Wynn sentinel is finite and takes part.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int ENS_THREADS = 256;
constexpr int ENS_OWN = 4;                  // members a thread of the quantile kernel ranks per pass over the tile

// One thread per output e; neighbouring threads read neighbouring doubles of one member row.  Two passes over the nens
// values of the output (the second one finds them in the cache): sum, count, extremes and exceedance counts, then the squared
// deviations.  The exceedance counters live in registers: the loop over UCF_ENSEMBLE_MAX_Q unrolls, limits beyond nlim are
// never read.  limit is read at wave-uniform addresses.
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_moments_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                              int nlim, const double* __restrict__ limit,
                                                                              double* __restrict__ mean, double* __restrict__ sd,
                                                                              double* __restrict__ mn, double* __restrict__ mx,
                                                                              int* __restrict__ nfin, double* __restrict__ pexc,
                                                                              unsigned long long* __restrict__ nbad)
{
    const long long e = (long long)blockIdx.x * ENS_THREADS + threadIdx.x;
    bool bad = false;
    if (e < nout) {
        const size_t no = (size_t)nout;
        double lim[UCF_ENSEMBLE_MAX_Q];
        int over[UCF_ENSEMBLE_MAX_Q];
#pragma unroll
        for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) {
            lim[l] = (pexc && l < nlim) ? limit[l] : 0.0;
            over[l] = 0;
        }
        const double nan = __builtin_nan("");
        double acc = 0.0, lo = nan, hi = nan;
        int n = 0;
        for (int m = 0; m < nens; m++) {
            const double v = a[(size_t)m * no + e];
            if (!isfinite(v)) continue;
            acc = acc + v;
            n++;
            if (!(v >= lo)) lo = v;                      // the first member of F, then v < lo
            if (!(v < hi)) hi = v;                       // the first member of F, then v >= hi
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) over[l] += (v > lim[l]) ? 1 : 0;
        }
        const double dn = (double)n;
        const double mu = acc / dn;                      // n = 0: +0.0 / +0.0 = NaN
        bad = n < nens;
        if (mean) mean[e] = mu;
        if (mn) mn[e] = lo;
        if (mx) mx[e] = hi;
        if (nfin) nfin[e] = n;
        if (sd) {
            double ss = 0.0;
            for (int m = 0; m < nens; m++) {
                const double v = a[(size_t)m * no + e];
                if (!isfinite(v)) continue;
                const double d = v - mu;
                ss = ss + d * d;
            }
            sd[e] = (n < 2) ? nan : sqrt(ss / (double)(n - 1));
        }
        if (pexc) {
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++)
                if (l < nlim) pexc[(size_t)l * no + e] = (double)over[l] / dn;
        }
    }
    // every lane of every wave arrives here (no early return above)
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(nbad, (unsigned long long)__popcll(b));
}

// Order statistics.  A workgroup stages the tile [nens][T] of T neighbouring outputs in LDS (coalesced reads of T doubles per
// member row; a member that is not finite, and an output beyond nout, is staged as NaN, which compares false with everything
// and so drops out of every count below).  Thread tid works on output tid % T -- neighbouring lanes, neighbouring doubles of a
// tile row: 8-byte LDS reads on distinct banks, lanes of the same output (T < 64) read one address -- and, with the
// ENS_THREADS / T threads of that output, shares its members: ENS_OWN consecutive members per thread and pass.  Every pass
// walks all rows of the tile at wave-uniform row addresses and counts, without a branch, rank(m) = #{m' : v' < v or (v' == v
// and m' < m)}; then, per level, the member whose rank is k or k + 1 leaves its value in LDS.  After a barrier one thread per
// (level, output) interpolates and writes.  LDS: (nens + 2 UCF_ENSEMBLE_MAX_Q) T doubles, dynamic.
template <int T>
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_quantile_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                               int nq, const double* __restrict__ q,
                                                                               double* __restrict__ quant)
{
    extern __shared__ double ens_lds[];
    constexpr int G = ENS_THREADS / T;                   // threads per output
    double* tile = ens_lds;                              // [nens][T]
    double* xk = ens_lds + (size_t)nens * T;             // [UCF_ENSEMBLE_MAX_Q][T]: x_k of every level
    double* xk1 = xk + UCF_ENSEMBLE_MAX_Q * T;           // ... and x_{k+1}
    const int j = threadIdx.x % T, g = threadIdx.x / T;
    const long long e0 = (long long)blockIdx.x * T;
    const long long e = e0 + j;
    const size_t no = (size_t)nout;
    const double nan = __builtin_nan("");
    for (int m = g; m < nens; m += G) {
        double v = nan;
        if (e < nout) v = a[(size_t)m * no + e];
        tile[m * T + j] = isfinite(v) ? v : nan;
    }
    __syncthreads();
    // n of this thread's output: every thread of the output counts the same rows
    int n = 0;
    for (int m = 0; m < nens; m++) n += (tile[m * T + j] == tile[m * T + j]) ? 1 : 0;
    const double dn1 = (double)(n - 1);
    for (int base = g * ENS_OWN; base < nens; base += G * ENS_OWN) {
        double v[ENS_OWN];
        int r[ENS_OWN];
#pragma unroll
        for (int i = 0; i < ENS_OWN; i++) {
            v[i] = (base + i < nens) ? tile[(base + i) * T + j] : nan;
            r[i] = 0;
        }
        for (int m = 0; m < nens; m++) {
            const double w = tile[m * T + j];
#pragma unroll
            for (int i = 0; i < ENS_OWN; i++) r[i] += ((w < v[i]) | ((w == v[i]) & (m < base + i))) ? 1 : 0;
        }
        for (int l = 0; l < nq; l++) {
            const double pos = q[l] * dn1;
            int k = (int)floor(pos);
            if (k >= n - 1) k = n - 1;
#pragma unroll
            for (int i = 0; i < ENS_OWN; i++) {
                if (v[i] == v[i] && r[i] == k) xk[l * T + j] = v[i];
                if (v[i] == v[i] && r[i] == k + 1) xk1[l * T + j] = v[i];
            }
        }
    }
    __syncthreads();
    if (e >= nout) return;
    for (int l = g; l < nq; l += G) {
        double out = nan;
        if (n > 0) {
            const double pos = q[l] * dn1;
            const double fl = floor(pos);
            const int k = (int)fl;
            const double x0 = xk[l * T + j];
            if (k >= n - 1) out = x0;
            else {
                const double gq = pos - fl;
                out = x0 + gq * (xk1[l * T + j] - x0);
            }
        }
        quant[(size_t)l * no + e] = out;
    }
}

template <int T>
void quantile_launch(int nens, long long nout, const double* d_a, int nq, const double* d_q, double* d_quant, hipStream_t st)
{
    const size_t lds = sizeof(double) * ((size_t)nens + 2 * UCF_ENSEMBLE_MAX_Q) * T;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)field_ensemble_quantile_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long blocks = (nout + T - 1) / T;
    hipLaunchKernelGGL(field_ensemble_quantile_kernel<T>, dim3((unsigned)blocks), dim3(ENS_THREADS), lds, st, nens, nout, d_a, nq, d_q, d_quant);
}

// ---- the weighted reduction (ucf_field_ensemble_weighted).  u [nens] are the integer weights of ucf_ensemble_quantise, 0 .. 2^32; a
// member with u = 0 is not in the ensemble.  u[m] is read at a wave-uniform address (m is a loop counter): scalar loads, no
// LDS.  Every cumulative weight is a 64-bit integer sum of at most 1024 * 2^32 = 2^42: exact, whatever the order, and exact
// again as a double.

// field_ensemble_moments_kernel with weights: F = the members with u > 0 and a finite value.  The exceedance sums are
// 64-bit integers in registers.  A member with u = 0 is skipped by a wave-uniform branch, its value is not loaded.
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_wmoments_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                               const unsigned long long* __restrict__ u, int nlim,
                                                                               const double* __restrict__ limit, double* __restrict__ mean,
                                                                               double* __restrict__ sd, double* __restrict__ mn,
                                                                               double* __restrict__ mx, int* __restrict__ nfin,
                                                                               double* __restrict__ pexc, unsigned long long* __restrict__ nbad)
{
    const long long e = (long long)blockIdx.x * ENS_THREADS + threadIdx.x;
    bool bad = false;
    if (e < nout) {
        const size_t no = (size_t)nout;
        double lim[UCF_ENSEMBLE_MAX_Q];
        unsigned long long over[UCF_ENSEMBLE_MAX_Q];
#pragma unroll
        for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) {
            lim[l] = (pexc && l < nlim) ? limit[l] : 0.0;
            over[l] = 0;
        }
        const double nan = __builtin_nan("");
        double acc = 0.0, U2 = 0.0, lo = nan, hi = nan;
        unsigned long long U = 0;
        int n = 0, nmem = 0;                             // nmem: the members of the ensemble (u > 0), the same in every thread
        for (int m = 0; m < nens; m++) {
            const unsigned long long um = u[m];
            if (um == 0) continue;
            nmem++;
            const double v = a[(size_t)m * no + e];
            if (!isfinite(v)) continue;
            const double du = (double)um;
            acc = acc + du * v;
            U2 = U2 + du * du;
            U += um;
            n++;
            if (!(v >= lo)) lo = v;
            if (!(v < hi)) hi = v;
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++) over[l] += (v > lim[l]) ? um : 0ULL;
        }
        const double dU = (double)U;
        const double mu = acc / dU;                      // n = 0: +0.0 / +0.0 = NaN
        bad = n < nmem;
        if (mean) mean[e] = mu;
        if (mn) mn[e] = lo;
        if (mx) mx[e] = hi;
        if (nfin) nfin[e] = n;
        if (sd) {
            double ss = 0.0;
            for (int m = 0; m < nens; m++) {
                const unsigned long long um = u[m];
                if (um == 0) continue;
                const double v = a[(size_t)m * no + e];
                if (!isfinite(v)) continue;
                const double d = v - mu;
                ss = ss + (double)um * (d * d);
            }
            const double den = dU - U2 / dU;
            sd[e] = (n < 2 || !(den > 0.0)) ? nan : sqrt(ss / den);
        }
        if (pexc) {
#pragma unroll
            for (int l = 0; l < UCF_ENSEMBLE_MAX_Q; l++)
                if (l < nlim) pexc[(size_t)l * no + e] = (double)over[l] / dU;
        }
    }
    // every lane of every wave arrives here (no early return above)
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(nbad, (unsigned long long)__popcll(b));
}

// The inverse of the weighted empirical distribution function: the tiles, the threads and the ENS_OWN scheme of
// field_ensemble_quantile_kernel.  A member that is not finite or has u = 0 is staged as NaN and drops out of every comparison.
// In place of a rank a thread accumulates, without a branch, E(m) = the sum of u[m'] over the m' with v' < v or (v' == v and
// m' < m): the weight in front of member m in the stable order (ties have one value, so that order only decides which of -0.0
// and +0.0 a tie returns).  The intervals (E(m), E(m) + u[m]] of the staged members partition (0, U], so for a level p exactly
// one member has E < p U <= E + u (E == 0 where p U == 0): it leaves its value in LDS, and that value is the result -- no
// interpolation.  LDS: (nens + UCF_ENSEMBLE_MAX_Q) T doubles, dynamic.
template <int T>
__global__ __launch_bounds__(ENS_THREADS) void field_ensemble_wquantile_kernel(int nens, long long nout, const double* __restrict__ a,
                                                                                const unsigned long long* __restrict__ u, int nq,
                                                                                const double* __restrict__ q, double* __restrict__ quant)
{
    extern __shared__ double ens_lds[];
    constexpr int G = ENS_THREADS / T;                   // threads per output
    double* tile = ens_lds;                              // [nens][T]
    double* xq = ens_lds + (size_t)nens * T;             // [UCF_ENSEMBLE_MAX_Q][T]: the selected value of every level
    const int j = threadIdx.x % T, g = threadIdx.x / T;
    const long long e0 = (long long)blockIdx.x * T;
    const long long e = e0 + j;
    const size_t no = (size_t)nout;
    const double nan = __builtin_nan("");
    for (int m = g; m < nens; m += G) {
        double v = nan;
        if (e < nout && u[m] != 0) v = a[(size_t)m * no + e];
        tile[m * T + j] = isfinite(v) ? v : nan;
    }
    __syncthreads();
    // U of this thread's output: every thread of the output adds the same rows, an integer sum
    unsigned long long U = 0;
    for (int m = 0; m < nens; m++) U += (tile[m * T + j] == tile[m * T + j]) ? u[m] : 0ULL;
    const double dU = (double)U;
    for (int base = g * ENS_OWN; base < nens; base += G * ENS_OWN) {
        double v[ENS_OWN];
        unsigned long long E[ENS_OWN], uo[ENS_OWN];
#pragma unroll
        for (int i = 0; i < ENS_OWN; i++) {
            v[i] = (base + i < nens) ? tile[(base + i) * T + j] : nan;
            uo[i] = (base + i < nens) ? u[base + i] : 0ULL;
            E[i] = 0;
        }
        for (int m = 0; m < nens; m++) {
            const double w = tile[m * T + j];
            const unsigned long long um = u[m];
#pragma unroll
            for (int i = 0; i < ENS_OWN; i++) E[i] += ((w < v[i]) | ((w == v[i]) & (m < base + i))) ? um : 0ULL;
        }
        for (int l = 0; l < nq; l++) {
            const double tgt = q[l] * dU;
#pragma unroll
            for (int i = 0; i < ENS_OWN; i++) {
                const bool in = ((double)E[i] < tgt) & (tgt <= (double)(E[i] + uo[i]));
                const bool first = (tgt == 0.0) & (E[i] == 0);
                if (v[i] == v[i] && (in | first)) xq[l * T + j] = v[i];
            }
        }
    }
    __syncthreads();
    if (e >= nout) return;
    for (int l = g; l < nq; l += G) quant[(size_t)l * no + e] = (U > 0) ? xq[l * T + j] : nan;
}

template <int T>
void wquantile_launch(int nens, long long nout, const double* d_a, const unsigned long long* d_u, int nq, const double* d_q, double* d_quant,
                      hipStream_t st)
{
    const size_t lds = sizeof(double) * ((size_t)nens + UCF_ENSEMBLE_MAX_Q) * T;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)field_ensemble_wquantile_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long blocks = (nout + T - 1) / T;
    hipLaunchKernelGGL(field_ensemble_wquantile_kernel<T>, dim3((unsigned)blocks), dim3(ENS_THREADS), lds, st, nens, nout, d_a, d_u, nq, d_q, d_quant);
}
}  // namespace

int ucf_field_ensemble_tile(int nens) { return nens <= 256 ? 64 : nens <= 512 ? 32 : 16; }

int ucf_field_launch_ensemble_moments(int nens, long long nout, const double* d_a, int nlim, const double* d_limit, double* d_mean,
                                      double* d_sd, double* d_min, double* d_max, int* d_nfin, double* d_pexc, long long* d_nbad,
                                      void* stream)
{
    const long long blocks = (nout + ENS_THREADS - 1) / ENS_THREADS;
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX || nout < 1 || blocks > 0x7fffffffLL || !d_a || !d_nbad || nlim < 0 || nlim > UCF_ENSEMBLE_MAX_Q ||
        (d_pexc && (nlim < 1 || !d_limit))) return UCF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(field_ensemble_moments_kernel, dim3((unsigned)blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, nens, nout, d_a,
                       nlim, d_limit, d_mean, d_sd, d_min, d_max, d_nfin, d_pexc, (unsigned long long*)d_nbad);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_ensemble_quantile(int nens, long long nout, const double* d_a, int nq, const double* d_q, double* d_quant,
                                       void* stream)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX || nout < 1 || nq < 1 || nq > UCF_ENSEMBLE_MAX_Q || !d_a || !d_q || !d_quant) return UCF_ERR_BAD_ARGUMENT;
    const int T = ucf_field_ensemble_tile(nens);
    if ((nout + T - 1) / T > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    switch (T) {
    case 64: quantile_launch<64>(nens, nout, d_a, nq, d_q, d_quant, st); break;
    case 32: quantile_launch<32>(nens, nout, d_a, nq, d_q, d_quant, st); break;
    default: quantile_launch<16>(nens, nout, d_a, nq, d_q, d_quant, st); break;
    }
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_ensemble_wmoments(int nens, long long nout, const double* d_a, const unsigned long long* d_u, int nlim,
                                       const double* d_limit, double* d_mean, double* d_sd, double* d_min, double* d_max, int* d_nfin,
                                       double* d_pexc, long long* d_nbad, void* stream)
{
    const long long blocks = (nout + ENS_THREADS - 1) / ENS_THREADS;
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX || nout < 1 || blocks > 0x7fffffffLL || !d_a || !d_u || !d_nbad || nlim < 0 || nlim > UCF_ENSEMBLE_MAX_Q ||
        (d_pexc && (nlim < 1 || !d_limit))) return UCF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(field_ensemble_wmoments_kernel, dim3((unsigned)blocks), dim3(ENS_THREADS), 0, (hipStream_t)stream, nens, nout, d_a, d_u,
                       nlim, d_limit, d_mean, d_sd, d_min, d_max, d_nfin, d_pexc, (unsigned long long*)d_nbad);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_ensemble_wquantile(int nens, long long nout, const double* d_a, const unsigned long long* d_u, int nq, const double* d_q,
                                        double* d_quant, void* stream)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX || nout < 1 || nq < 1 || nq > UCF_ENSEMBLE_MAX_Q || !d_a || !d_u || !d_q || !d_quant) return UCF_ERR_BAD_ARGUMENT;
    const int T = ucf_field_ensemble_tile(nens);
    if ((nout + T - 1) / T > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    switch (T) {
    case 64: wquantile_launch<64>(nens, nout, d_a, d_u, nq, d_q, d_quant, st); break;
    case 32: wquantile_launch<32>(nens, nout, d_a, d_u, nq, d_q, d_quant, st); break;
    default: wquantile_launch<16>(nens, nout, d_a, d_u, nq, d_q, d_quant, st); break;
    }
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
