// ucf_field.hip -- superposition of a well field (ucf_field_drawdown, include/ucf.h): the drawdown at (time k, location i,
// depth z) is the sum over the wells of q_j times the group result at (k - k0_j, column of the distance |x_i - x_j|, z).
//
// Tiny and gather-bound: per output nwell pairs of doubles, neighbours in z (the fastest index of the outputs and of the
// group results) read neighbours.  Built with -ffp-contract=off: every product and sum below is rounded on its own, so the
// result is the arithmetic written here.  One thread owns one output and adds the wells in the caller's order: no atomics,
// a repeated call gives the same bits.  Nothing is scrubbed: non-finite values and the Wynn sentinel propagate.
// field_forecast_kernel (ucf_field_forecast) combines the 1 + 2 npar superposed maps of a forecast under the same rules;
// field_response_kernel (ucf_field_yield) forms the same sums control by control at the constrained outputs.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int FIELD_THREADS = 256;

__global__ __launch_bounds__(FIELD_THREADS) void field_superpose_kernel(long long nout, int nloc, int nz, int nwell,
                                                                        const ucf_field_well* __restrict__ wells,
                                                                        const int* __restrict__ col, const double* __restrict__ tfac,
                                                                        const double* __restrict__ h, const double* __restrict__ dh,
                                                                        int scaled, double scale, double* __restrict__ s,
                                                                        double* __restrict__ ds)
{
    const long long e = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (e >= nout) return;
    const int z = (int)(e % nz);
    const long long p = e / nz;
    const int i = (int)(p % nloc), k = (int)(p / nloc);
    double acc = 0.0, dacc = 0.0;
    for (int j = 0; j < nwell; j++) {
        const ucf_field_well w = wells[j];
        if (k < w.k0) continue;                      // the well has not started
        const int kk = k - w.k0;
        const size_t at = (size_t)w.off + ((size_t)kk * w.nr + col[(size_t)i * nwell + j]) * nz + z;
        acc = acc + w.q * h[at];
        dacc = dacc + w.q * (tfac[w.toff + kk] * dh[at]);
    }
    if (scaled) { acc = acc * scale; dacc = dacc * scale; }
    s[e] = acc;
    ds[e] = dacc;
}

// The response slots of ucf_field_yield, in place of the superposition: one thread per (slot c, constrained output i).  Slot c
// sums the wells of control c, slot nctl the fixed wells (ctl == -1), in the caller's order and with the statements of
// field_superpose_kernel, so that the slots of a member add up to its map; the drawdown only, dh is not read.  Neighbouring
// threads are neighbouring constrained outputs of one slot: the stores are coalesced, the gathers as near as con allows.
__global__ __launch_bounds__(FIELD_THREADS) void field_response_kernel(int ncon, int nctl, int nloc, int nz, int nwell,
                                                                       const ucf_field_well* __restrict__ wells,
                                                                       const int* __restrict__ col, const int* __restrict__ ctl,
                                                                       const int* __restrict__ con, const double* __restrict__ h,
                                                                       double scale, double* __restrict__ R)
{
    const long long q = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (q >= (long long)(nctl + 1) * ncon) return;
    const int c = (int)(q / ncon), i = (int)(q % ncon);
    const int mine = (c == nctl) ? -1 : c;
    const long long e = con[i];
    const int z = (int)(e % nz);
    const long long p = e / nz;
    const int iloc = (int)(p % nloc), k = (int)(p / nloc);
    double acc = 0.0;
    for (int j = 0; j < nwell; j++) {
        const ucf_field_well w = wells[j];
        if (ctl[j] != mine || k < w.k0) continue;
        const size_t at = (size_t)w.off + ((size_t)(k - w.k0) * w.nr + col[(size_t)iloc * nwell + j]) * nz + z;
        acc = acc + w.q * h[at];
    }
    R[q] = acc * scale;
}

// The combination of a forecast (ucf_field_forecast): one thread per output e of the slots a [1 + 2 NPAR][nout], launched once
// on the s slots and once on the ds slots.  HBM-bound: 1 + 2 NPAR coalesced reads (neighbouring threads read neighbouring
// doubles of one slot) and up to NPAR + 1 writes per output.  The J of a thread live in registers (NPAR is a template
// argument, every loop unrolls: no scratch); cov is read at wave-uniform addresses.  The count of outputs with a value that
// is not finite is a ballot per wave and one integer atomic per wave: the order of the additions does not change the sum.
template <int NPAR>
__global__ __launch_bounds__(FIELD_THREADS) void field_forecast_kernel(long long nout, double two_dlog, const double* __restrict__ a,
                                                                        const double* __restrict__ cov, double* __restrict__ sens,
                                                                        double* __restrict__ se, unsigned long long* __restrict__ nbad)
{
    const long long e = (long long)blockIdx.x * FIELD_THREADS + threadIdx.x;
    bool bad = false;
    if (e < nout) {
        const size_t n = (size_t)nout;
        bool ok = isfinite(a[e]);
        double J[NPAR];
#pragma unroll
        for (int j = 0; j < NPAR; j++) {
            const double up = a[(size_t)(1 + 2 * j) * n + e], down = a[(size_t)(2 + 2 * j) * n + e];
            ok = ok && isfinite(up) && isfinite(down);
            J[j] = (up - down) / two_dlog;
        }
        bad = !ok;
        if (sens) {
#pragma unroll
            for (int j = 0; j < NPAR; j++) sens[(size_t)j * n + e] = J[j];
        }
        if (se) {
            double var = 0.0;
#pragma unroll
            for (int j = 0; j < NPAR; j++) {
                double inner = 0.0;
#pragma unroll
                for (int k = 0; k < NPAR; k++) inner = inner + cov[j * NPAR + k] * J[k];
                var = var + J[j] * inner;
            }
            se[e] = (var < 0.0) ? 0.0 : sqrt(var);       // a NaN var is not < 0: it stays NaN
        }
    }
    // every lane of every wave arrives here (no early return above)
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(nbad, (unsigned long long)__popcll(m));
}

template <int NPAR>
void forecast_launch(long long nout, unsigned blocks, double two_dlog, const double* d_a, const double* d_cov, double* d_sens,
                     double* d_se, long long* d_nbad, hipStream_t st)
{
    hipLaunchKernelGGL(field_forecast_kernel<NPAR>, dim3(blocks), dim3(FIELD_THREADS), 0, st, nout, two_dlog, d_a, d_cov, d_sens, d_se,
                       (unsigned long long*)d_nbad);
}
}  // namespace

int ucf_field_launch_superpose(int nt, int nloc, int nz, int nwell, const ucf_field_well* d_wells, const int* d_col,
                               const double* d_tfac, const double* d_h, const double* d_dh, int scaled, double scale,
                               double* d_s, double* d_ds, void* stream)
{
    const long long nout = (long long)nt * nloc * nz;
    const long long blocks = (nout + FIELD_THREADS - 1) / FIELD_THREADS;
    if (nout < 1 || blocks > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(field_superpose_kernel, dim3((unsigned)blocks), dim3(FIELD_THREADS), 0, (hipStream_t)stream, nout, nloc, nz,
                       nwell, d_wells, d_col, d_tfac, d_h, d_dh, scaled, scale, d_s, d_ds);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_response(int ncon, int nctl, int nloc, int nz, int nwell, const ucf_field_well* d_wells, const int* d_col,
                              const int* d_ctl, const int* d_con, const double* d_h, double scale, double* d_R, void* stream)
{
    const long long n = (long long)(nctl + 1) * ncon, blocks = (n + FIELD_THREADS - 1) / FIELD_THREADS;
    if (ncon < 1 || nctl < 1 || nctl > UCF_YIELD_MAX_CTL || blocks > 0x7fffffffLL || !d_wells || !d_col || !d_ctl || !d_con || !d_h || !d_R)
        return UCF_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(field_response_kernel, dim3((unsigned)blocks), dim3(FIELD_THREADS), 0, (hipStream_t)stream, ncon, nctl, nloc, nz,
                       nwell, d_wells, d_col, d_ctl, d_con, d_h, scale, d_R);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}

int ucf_field_launch_forecast(int npar, long long nout, double two_dlog, const double* d_a, const double* d_cov, double* d_sens,
                              double* d_se, long long* d_nbad, void* stream)
{
    const long long blocks = (nout + FIELD_THREADS - 1) / FIELD_THREADS;
    if (nout < 1 || blocks > 0x7fffffffLL || !d_a || !d_nbad || (d_se && !d_cov)) return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    switch (npar) {
    case 1: forecast_launch<1>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 2: forecast_launch<2>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 3: forecast_launch<3>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 4: forecast_launch<4>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 5: forecast_launch<5>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 6: forecast_launch<6>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 7: forecast_launch<7>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    case 8: forecast_launch<8>(nout, (unsigned)blocks, two_dlog, d_a, d_cov, d_sens, d_se, d_nbad, st); break;
    default: return UCF_ERR_BAD_ARGUMENT;
    }
    static_assert(UCF_FIT_MAX_PAR == 8, "one case per parameter count");
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
