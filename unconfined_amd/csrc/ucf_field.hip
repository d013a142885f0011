// ucf_field.hip -- superposition of a well field (ucf_field_drawdown, include/ucf.h): the drawdown at (time k, location i,
// depth z) is the sum over the wells of q_j times the group result at (k - k0_j, column of the distance |x_i - x_j|, z).
//
// Tiny and gather-bound: per output nwell pairs of doubles, neighbours in z (the fastest index of the outputs and of the
// group results) read neighbours.  Built with -ffp-contract=off: every product and sum below is rounded on its own, so the
// result is the arithmetic written here.  One thread owns one output and adds the wells in the caller's order: no atomics,
// a repeated call gives the same bits.  Nothing is scrubbed: non-finite values and the Wynn sentinel propagate.
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
