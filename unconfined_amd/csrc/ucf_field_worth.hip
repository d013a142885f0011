// ucf_field_worth.hip -- data worth on the slots of a forecast (ucf_field_worth, include/ucf.h): per candidate observation well
// c = (location, depth) the variance that its readings would leave on up to UCF_WORTH_MAX_TGT forecast targets.  The prior is
// cov = F F' in ln theta; the readings of c add sum (w j)(w j)' to its inverse, and with g = F' j the posterior variance of a
// target with a = F' j_t is a' B^-1 a, B = I + sum (w g)(w g)': cov is never inverted and B has no eigenvalue below 1.
//
// One thread per candidate.  The slots are a [1 + 2 NPAR][nt][ncand]: neighbouring lanes are neighbouring candidates of one slot
// row, so every load is coalesced.  B (lower triangle), its LDL' factors, J, g and y live in registers: NPAR is a template
// argument and every loop over parameters unrolls, so every index is a compile-time constant (no scratch).  F, A, tw and tsel
// are read at wave-uniform addresses.  A map has few candidates (thousands), each with a long dependent chain of arithmetic,
// so a workgroup is ONE wave: ncand / 64 workgroups spread over the compute units instead of filling a few of them.
//
// Built with -ffp-contract=off like ucf_field.hip: every sum, product and quotient below is rounded on its own, so the result
// is the arithmetic that include/ucf.h states.  A thread owns its outputs: no atomics, a call repeated gives the same bits.
// Nothing is scrubbed but what the header states: a datum with a slot value that is not finite is skipped and not counted.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int WORTH_THREADS = 64;           // one wave
constexpr int GATHER_THREADS = 256;

// g = F' J, then B_ij += (w g_i)(w g_j) on the lower triangle; J of the datum at a[.][e]; false: a slot value is not finite
template <int NPAR>
__device__ __forceinline__ bool worth_add_datum(const double* __restrict__ a, size_t slot, size_t e, double two_dlog,
                                                const double* __restrict__ F, double w, double (&B)[NPAR][NPAR])
{
    double J[NPAR];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NPAR; j++) {
        const double up = a[(size_t)(1 + 2 * j) * slot + e], down = a[(size_t)(2 + 2 * j) * slot + e];
        ok = ok && isfinite(up) && isfinite(down);
        J[j] = (up - down) / two_dlog;
    }
    if (!ok) return false;
    double wg[NPAR];
#pragma unroll
    for (int j = 0; j < NPAR; j++) {
        double g = 0.0;
#pragma unroll
        for (int i = 0; i < NPAR; i++) g = g + F[i * NPAR + j] * J[i];
        wg[j] = w * g;
    }
#pragma unroll
    for (int i = 0; i < NPAR; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) B[i][j] = B[i][j] + wg[i] * wg[j];
    return true;
}

template <int NPAR>
__global__ __launch_bounds__(WORTH_THREADS) void field_worth_kernel(int nt, int ncand, const double* __restrict__ a_s,
                                                                    const double* __restrict__ a_d, double two_dlog,
                                                                    const double* __restrict__ F, double ws, double wd,
                                                                    const int* __restrict__ tsel, int ntgt, const double* __restrict__ A,
                                                                    const double* __restrict__ tw, double* __restrict__ post,
                                                                    double* __restrict__ crit, int* __restrict__ nused)
{
    const long long c = (long long)blockIdx.x * WORTH_THREADS + threadIdx.x;
    if (c >= ncand) return;
    const size_t nc = (size_t)ncand, slot = (size_t)nt * nc;
    double B[NPAR][NPAR];                                // the lower triangle; the rest is never touched
#pragma unroll
    for (int i = 0; i < NPAR; i++)
#pragma unroll
        for (int j = 0; j <= i; j++) B[i][j] = (i == j) ? 1.0 : 0.0;
    int used = 0;
    for (int k = 0; k < nt; k++) {
        if (tsel[k] == 0) continue;                      // wave-uniform
        const size_t e = (size_t)k * nc + c;
        if (ws > 0.0 && worth_add_datum<NPAR>(a_s, slot, e, two_dlog, F, ws, B)) used++;
        if (wd > 0.0 && worth_add_datum<NPAR>(a_d, slot, e, two_dlog, F, wd, B)) used++;
    }
    // B = L D L' without square roots: l in the strict lower triangle of B, d apart
    double d[NPAR];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NPAR; j++) {
        double v = B[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) v = v - (B[j][k] * B[j][k]) * d[k];
        d[j] = v;
        ok = ok && v > 0.0 && isfinite(v);
#pragma unroll
        for (int i = j + 1; i < NPAR; i++) {
            double u = B[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) u = u - (B[i][k] * B[j][k]) * d[k];
            B[i][j] = u / d[j];
        }
    }
    double cr = 0.0;
    for (int t = 0; t < ntgt; t++) {
        double y[NPAR];
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < NPAR; j++) {
            double yj = A[t * NPAR + j];
#pragma unroll
            for (int k = 0; k < j; k++) yj = yj - B[j][k] * y[k];
            y[j] = yj;
            v = v + (yj * yj) / d[j];
        }
        if (!ok) v = __builtin_nan("");
        post[(size_t)t * nc + c] = v;
        cr = cr + tw[t] * v;
    }
    crit[c] = cr;
    nused[c] = used;
}

template <int NPAR>
void worth_launch(unsigned blocks, int nt, int ncand, const double* a_s, const double* a_d, double two_dlog, const double* F, double ws,
                  double wd, const int* tsel, int ntgt, const double* A, const double* tw, double* post, double* crit, int* nused,
                  hipStream_t st)
{
    hipLaunchKernelGGL(field_worth_kernel<NPAR>, dim3(blocks), dim3(WORTH_THREADS), 0, st, nt, ncand, a_s, a_d, two_dlog, F, ws, wd, tsel,
                       ntgt, A, tw, post, crit, nused);
}

// out[n] = a[idx[n]]: the few slot values that the host needs of a map that stays on the device
__global__ __launch_bounds__(GATHER_THREADS) void field_gather_kernel(int n, const long long* __restrict__ idx, const double* __restrict__ a,
                                                                      double* __restrict__ out)
{
    const int i = (int)(blockIdx.x * (unsigned)GATHER_THREADS + threadIdx.x);
    if (i < n) out[i] = a[idx[i]];
}
}  // namespace

int ucf_field_launch_worth(int npar, int nt, int ncand, const double* d_as, const double* d_ad, double two_dlog, const double* d_F,
                           double ws, double wd, const int* d_tsel, int ntgt, const double* d_A, const double* d_tw, double* d_post,
                           double* d_crit, int* d_nused, void* stream)
{
    if (nt < 1 || ncand < 1 || ntgt < 1 || ntgt > UCF_WORTH_MAX_TGT || !d_as || (wd > 0.0 && !d_ad) || !d_F || !d_tsel || !d_A || !d_tw ||
        !d_post || !d_crit || !d_nused)
        return UCF_ERR_BAD_ARGUMENT;
    const unsigned blocks = (unsigned)(((long long)ncand + WORTH_THREADS - 1) / WORTH_THREADS);
    hipStream_t st = (hipStream_t)stream;
#define UCF_WORTH_CASE(N) \
    case N: worth_launch<N>(blocks, nt, ncand, d_as, d_ad, two_dlog, d_F, ws, wd, d_tsel, ntgt, d_A, d_tw, d_post, d_crit, d_nused, st); break;
    switch (npar) {
        UCF_WORTH_CASE(1) UCF_WORTH_CASE(2) UCF_WORTH_CASE(3) UCF_WORTH_CASE(4)
        UCF_WORTH_CASE(5) UCF_WORTH_CASE(6) UCF_WORTH_CASE(7) UCF_WORTH_CASE(8)
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_WORTH_CASE
    static_assert(UCF_FIT_MAX_PAR == 8, "one case per parameter count");
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_gather(int n, const long long* d_idx, const double* d_a, double* d_out, void* stream)
{
    if (n < 1 || !d_idx || !d_a || !d_out) return UCF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(field_gather_kernel, dim3((unsigned)((n + GATHER_THREADS - 1) / GATHER_THREADS)), dim3(GATHER_THREADS), 0,
                       (hipStream_t)stream, n, d_idx, d_a, d_out);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
