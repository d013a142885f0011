// ucf_field_sobol.hip -- the reduction of a Saltelli design over its member axis (ucf_field_sobol, include/ucf.h): per output e
// of the member maps a [(npar + 2) nbase][nout] the first-order Sobol index S_j and the total index ST_j of every parameter, their
// standard errors, the pooled mean and variance of A u B and the number of complete base rows.
//
// One thread per output e, field_sobol_kernel<NPAR>.  The layout is member-major: at every (block, r) neighbouring lanes read
// neighbouring doubles of one member row, so every load is coalesced, and the slots are read as they lie.  The NPAR + 2 loads
// of a base row are independent of each other and are issued together, before the first of them is used.  Two sweeps over r,
// because the estimators are centred: sweep 1 finds which rows are complete, and sA, sB, hence the mean; sweep 2 finds
// completeness again (the second sweep finds the values in the cache) and forms qA, qB and the 4 NPAR sums of the indices about
// that mean.  Every accumulator lives in a register (the loops over j unroll): no LDS, no scratch.  The only atomic is the
// integer count of nbad, one per wave after a ballot: a call repeated gives the same bits.
//
// Built with -ffp-contract=off like ucf_field.hip: every sum, difference, product and quotient below is rounded on its own, so
// the result is the arithmetic that include/ucf.h states.  Every NaN written is the quiet NaN 0x7ff8000000000000.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int SOBOL_THREADS = 256;

// x, or the one NaN that the statement writes
__device__ __forceinline__ double sobol_out(double x) { return x == x ? x : __builtin_nan(""); }

template <int NPAR>
__global__ __launch_bounds__(SOBOL_THREADS) void field_sobol_kernel(int nbase, long long nout, const double* __restrict__ a,
                                                                    double* __restrict__ S, double* __restrict__ ST,
                                                                    double* __restrict__ seS, double* __restrict__ seST,
                                                                    double* __restrict__ mean, double* __restrict__ var,
                                                                    int* __restrict__ nrow, unsigned long long* __restrict__ nbad)
{
    const long long e = (long long)blockIdx.x * SOBOL_THREADS + threadIdx.x;
    bool bad = false;
    if (e < nout) {
        const size_t no = (size_t)nout, blk = (size_t)nbase * no;          // a block of the design: nbase member rows
        const double* col = a + e;
        const double nan = __builtin_nan("");
        // sweep 1: the complete rows, sA, sB
        double sA = 0.0, sB = 0.0;
        int n = 0;
        for (int r = 0; r < nbase; r++) {
            const double* row = col + (size_t)r * no;
            const double fa = row[0], fb = row[blk];
            double fj[NPAR];
#pragma unroll
            for (int j = 0; j < NPAR; j++) fj[j] = row[(size_t)(2 + j) * blk];
            bool c = isfinite(fa) && isfinite(fb);
#pragma unroll
            for (int j = 0; j < NPAR; j++) c = c && isfinite(fj[j]);
            if (c) {
                sA = sA + fa;
                sB = sB + fb;
                n++;
            }
        }
        bad = n < nbase;
        const double dn = (double)n;
        const double mu = (sA + sB) / (double)(2 * n);                     // n = 0: +0.0 / +0.0 = NaN
        // sweep 2: the squared deviations of A and B and the sums of the two estimators, about mu
        double qA = 0.0, qB = 0.0, v1[NPAR], q1[NPAR], vt[NPAR], qt[NPAR];
#pragma unroll
        for (int j = 0; j < NPAR; j++) v1[j] = q1[j] = vt[j] = qt[j] = 0.0;
        for (int r = 0; r < nbase; r++) {
            const double* row = col + (size_t)r * no;
            const double fa = row[0], fb = row[blk];
            double fj[NPAR];
#pragma unroll
            for (int j = 0; j < NPAR; j++) fj[j] = row[(size_t)(2 + j) * blk];
            bool c = isfinite(fa) && isfinite(fb);
#pragma unroll
            for (int j = 0; j < NPAR; j++) c = c && isfinite(fj[j]);
            if (c) {
                const double da = fa - mu, db = fb - mu;
                qA = qA + da * da;
                qB = qB + db * db;
#pragma unroll
                for (int j = 0; j < NPAR; j++) {
                    const double p = db * (fj[j] - fa);
                    v1[j] = v1[j] + p;
                    q1[j] = q1[j] + p * p;
                    const double dt = fa - fj[j], pt = dt * dt;
                    vt[j] = vt[j] + pt;
                    qt[j] = qt[j] + pt * pt;
                }
            }
        }
        const double vr = n == 0 ? nan : (qA + qB) / (double)(2 * n - 1);
        const bool pos = vr > 0.0, two = n >= 2 && pos;
        if (nrow) nrow[e] = n;
        if (mean) mean[e] = sobol_out(mu);
        if (var) var[e] = sobol_out(vr);
        const double dn1 = (double)(n - 1);
#pragma unroll
        for (int j = 0; j < NPAR; j++) {
            const size_t at = (size_t)j * no + e;
            const double m1 = v1[j] / dn, mt = vt[j] / dn;
            if (S) S[at] = pos ? sobol_out(m1 / vr) : nan;
            if (ST) ST[at] = pos ? sobol_out((0.5 * mt) / vr) : nan;
            if (seS) {
                double w1 = q1[j] / dn - m1 * m1;
                if (w1 < 0.0) w1 = 0.0;
                seS[at] = two ? sobol_out(sqrt(w1 / dn1) / vr) : nan;
            }
            if (seST) {
                double wt = qt[j] / dn - mt * mt;
                if (wt < 0.0) wt = 0.0;
                seST[at] = two ? sobol_out((0.5 * sqrt(wt / dn1)) / vr) : nan;
            }
        }
    }
    // every lane of every wave arrives here (no early return above)
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(nbad, (unsigned long long)__popcll(b));
}

template <int NPAR>
void sobol_launch(const ucf_sobol_args* a, hipStream_t st)
{
    const dim3 blocks((unsigned)((a->nout + SOBOL_THREADS - 1) / SOBOL_THREADS));
    hipLaunchKernelGGL(field_sobol_kernel<NPAR>, blocks, dim3(SOBOL_THREADS), 0, st, a->nbase, a->nout, a->d_a, a->d_S, a->d_ST, a->d_seS,
                       a->d_seST, a->d_mean, a->d_var, a->d_nrow, (unsigned long long*)a->d_nbad);
}
}  // namespace

int ucf_field_launch_sobol(const ucf_sobol_args* a, void* stream)
{
    if (!a || a->npar < 1 || a->npar > UCF_FIT_MAX_PAR || a->nbase < 2 || a->nbase > UCF_SOBOL_MAX_BASE || a->nout < 1 || !a->d_a || !a->d_nbad)
        return UCF_ERR_BAD_ARGUMENT;
    if ((a->nout + SOBOL_THREADS - 1) / SOBOL_THREADS > 0x7fffffffLL) return UCF_ERR_BAD_ARGUMENT;
    static_assert(UCF_FIT_MAX_PAR == 8, "one instantiation per npar");
    hipStream_t st = (hipStream_t)stream;
    switch (a->npar) {
    case 1: sobol_launch<1>(a, st); break;
    case 2: sobol_launch<2>(a, st); break;
    case 3: sobol_launch<3>(a, st); break;
    case 4: sobol_launch<4>(a, st); break;
    case 5: sobol_launch<5>(a, st); break;
    case 6: sobol_launch<6>(a, st); break;
    case 7: sobol_launch<7>(a, st); break;
    default: sobol_launch<8>(a, st); break;
    }
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
