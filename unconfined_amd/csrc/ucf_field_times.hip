// ucf_field_times.hip -- the time kernel of ucf_field_ensemble_times (include/ucf.h): per member m, limit l and site e the
// abscissa at which the member's series a[m][.][e] first passes limit[l] (UCF_TIME_FIRST_ABOVE) or from which it stays at or
// below it (UCF_TIME_LAST_ABOVE), linearly interpolated in tau between the two samples that bracket the crossing.
//
// One thread per (m, l, e), e fastest: a workgroup of 256 threads takes 256 neighbouring sites of ONE member and ONE limit
// (blockIdx.x the tile of sites, .y the limit, .z the member), so limit[l], kind[l] and -- in the forward walk -- tau[k] are
// read at wave-uniform addresses, and at every k neighbouring lanes read neighbouring doubles of the row a[m][k][.]: every
// load of the series is coalesced.  A thread walks k = 0 .. nt-1 once and keeps what it needs of the series (the previous
// value; for LAST_ABOVE the last value above and its successor) in registers.  No atomics, no LDS, no scratch: a call
// repeated gives the same bits.  FIRST_ABOVE stops reading at the crossing; a wave goes on until its last lane has crossed.
//
// Built with -ffp-contract=off like ucf_field.hip: every difference, quotient, product and sum is rounded on its own.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int TIMES_THREADS = 256;

__global__ __launch_bounds__(TIMES_THREADS) void field_times_kernel(int nt, long long nsite, const double* __restrict__ a,
                                                                    const double* __restrict__ tau, double tau_never,
                                                                    const double* __restrict__ limit, const int* __restrict__ kind,
                                                                    double* __restrict__ T)
{
    const long long e = (long long)blockIdx.x * TIMES_THREADS + threadIdx.x;
    if (e >= nsite) return;
    const int l = blockIdx.y, m = blockIdx.z, nlim = gridDim.y;
    const size_t ns = (size_t)nsite;
    const double L = limit[l];
    const double* col = a + (size_t)m * nt * ns + e;
    const double nan = __builtin_nan("");
    double out;
    if (kind[l] == UCF_TIME_FIRST_ABOVE) {
        out = tau_never;
        double v0 = 0.0;
        for (int k = 0; k < nt; k++) {
            const double v = col[(size_t)k * ns];
            if (!isfinite(v)) { out = nan; break; }
            if (v > L) {
                if (k == 0) {
                    out = tau[0];
                } else {
                    const double f = (L - v0) / (v - v0);
                    out = tau[k - 1] + f * (tau[k] - tau[k - 1]);
                }
                break;
            }
            v0 = v;
        }
    } else {
        // ks: the last k with a[k] > L so far, v0 = a[ks], v1 = a[ks + 1] once it has been read
        bool bad = false;
        int ks = -1;
        double v0 = 0.0, v1 = 0.0;
        for (int k = 0; k < nt; k++) {
            const double v = col[(size_t)k * ns];
            bad = bad || !isfinite(v);
            if (ks == k - 1) v1 = v;
            if (v > L) { ks = k; v0 = v; }
        }
        if (bad) {
            out = nan;
        } else if (ks < 0) {
            out = tau[0];
        } else if (ks == nt - 1) {
            out = tau_never;
        } else {
            const double f = (v0 - L) / (v0 - v1);
            out = tau[ks] + f * (tau[ks + 1] - tau[ks]);
        }
    }
    T[((size_t)m * nlim + l) * ns + e] = out;
}
}  // namespace

int ucf_field_launch_times(const ucf_times_args* a, void* stream)
{
    if (!a || a->nens < 1 || a->nens > UCF_ENSEMBLE_MAX || a->nt < 1 || a->nsite < 1 || a->nlim < 1 || a->nlim > UCF_ENSEMBLE_MAX_Q ||
        !a->d_a || !a->d_tau || !a->d_limit || !a->d_kind || !a->d_T)
        return UCF_ERR_BAD_ARGUMENT;
    const long long tiles = (a->nsite + TIMES_THREADS - 1) / TIMES_THREADS;
    if (tiles * TIMES_THREADS > 0xffffffffLL) return UCF_ERR_BAD_ARGUMENT;       // threads along x: below 2^32
    const dim3 grid((unsigned)tiles, (unsigned)a->nlim, (unsigned)a->nens);
    hipLaunchKernelGGL(field_times_kernel, grid, dim3(TIMES_THREADS), 0, (hipStream_t)stream, a->nt, a->nsite, a->d_a, a->d_tau,
                       a->tau_never, a->d_limit, a->d_kind, a->d_T);
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
