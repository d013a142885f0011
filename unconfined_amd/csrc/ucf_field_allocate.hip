// ucf_field_allocate.hip -- the linear programme of ucf_field_allocate (include/ucf.h): per member m and objective o the rates
// x in [0, xmax] that maximise w[o] . x while the drawdown b + sum_c x_c r_c stays at or below its limit on every constrained
// output.  b and r_c are the response slots R [nens][NCTL + 1][ncon] that field_response_kernel left on the device.
//
// A workgroup of four waves takes ONE (member, objective) and runs the primal active-set simplex of the header from x = 0.
// The small solves (NCTL <= 8) are serial: thread 0 does them on B, x, d, lambda and the working set in LDS, with the statements
// of ucf_field_allocate.h that the host twin ucf_allocate_solve runs too.  The ratio test is the parallel step: threads 0 ..
// 2 NCTL - 1 take a bound each, then all lanes walk the constrained outputs i with stride 256 -- neighbouring lanes read
// neighbouring doubles of one slot row, every load is coalesced --, and the lane partials (cand, id) are combined by a wave
// butterfly, lexicographic, the four waves through LDS: the pattern of field_yield_kernel.  A member's R is reread once per
// iteration.  No floating-point atomics: a call repeated gives the same bits.
//
// The kernel cannot hang.  Every loop has a compile-time bound, ncon / 256 or maxit as its bound.  Whether to go on is written
// to LDS by thread 0 only, in a phase of its own between two barriers, and read by every thread after the barrier that ends the
// phase: s_after_A is written between barrier 3 (or the start) and barrier 1 and read between barriers 1 and 2, s_after_C is
// written between barriers 2 and 3 and read between barrier 3 and the next barrier 1.  So every break below is taken by all 256
// threads or by none, all of them reach every __syncthreads(), and there is no return before the last barrier.
//
// Built with -ffp-contract=off like ucf_field_yield.hip: every product, sum, difference and quotient is rounded on its own; the
// one fused operation is the fma that the polish of the optimum asks for by name (the exact error of a product).
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"
#include "ucf_field_allocate.h"

namespace {
constexpr int ALLOC_THREADS = 256, ALLOC_WAVES = ALLOC_THREADS / 64;
using namespace ucf_alloc;

template <int NCTL>
__global__ __launch_bounds__(ALLOC_THREADS) void field_allocate_kernel(int ncon, int nobj, int maxit, const double* __restrict__ R,
                                                                       const double* __restrict__ lim, const double* __restrict__ w,
                                                                       const double* __restrict__ xmax, double* __restrict__ x_out,
                                                                       double* __restrict__ g_out, int* __restrict__ status_out,
                                                                       int* __restrict__ iters_out, int* __restrict__ work_out,
                                                                       double* __restrict__ lam_out, double* __restrict__ xpat_out,
                                                                       unsigned long long* __restrict__ nbad)
{
    __shared__ double s_B[NCTL * NCTL], s_A[NCTL * NCTL], s_b[NCTL], s_beta[NCTL], s_x[NCTL], s_xl[NCTL], s_d[NCTL], s_lam[NCTL];
    __shared__ int s_W[NCTL];
    __shared__ int s_bad, s_neg, s_start, s_after_A, s_after_C, s_k, s_status, s_iters;
    __shared__ double s_cand[ALLOC_WAVES];
    __shared__ unsigned s_id[ALLOC_WAVES];
    const int o = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const size_t nc = (size_t)ncon;
    const problem P = {R + (size_t)m * (NCTL + 1) * nc, lim, w + (size_t)o * NCTL, xmax, nc};

    if (tid == 0) { s_bad = 0; s_neg = 0; }
    if (tid < NCTL) { s_x[tid] = 0.0; s_lam[tid] = 0.0; s_W[tid] = tid; }
    __syncthreads();
    // validity and the start: any slot value that is not finite; any room below zero
    bool bad = false, neg = false;
    for (int i = tid; i < ncon; i += ALLOC_THREADS) {
#pragma unroll
        for (int c = 0; c < NCTL; c++) bad = bad || !isfinite(P.Rm[(size_t)c * nc + i]);
        const double b = P.Rm[(size_t)NCTL * nc + i];
        bad = bad || !isfinite(b);
        neg = neg || (lim[i] - b < 0.0);
    }
    if (bad) s_bad = 1;                        // every writer writes the same value
    if (neg) s_neg = 1;
    __syncthreads();
    if (tid == 0) {
        const int st = s_bad ? UCF_ALLOC_INVALID : s_neg ? UCF_ALLOC_INFEASIBLE_AT_ZERO : UCF_ALLOC_ITERATION_CAP;
        s_status = st;
        s_iters = 0;
        s_start = st == UCF_ALLOC_ITERATION_CAP ? 1 : 0;
        if (st == UCF_ALLOC_ITERATION_CAP) working_rows<NCTL>(P, s_W, s_B, s_beta);
    }
    __syncthreads();
    const int start = s_start;                 // written once, before the barrier above
    for (int it = 0; it < maxit; it++) {
        if (!start) break;
        // steps 1 to 3
        if (tid == 0) {
            int k = 0;
            const step what = multipliers_and_direction<NCTL>(P, s_W, s_B, s_A, s_b, s_lam, s_d, &k);
            s_k = k;
            if (what == STEP_OPTIMAL) s_status = UCF_ALLOC_OPTIMAL;
            if (what == STEP_NUMERIC) s_status = UCF_ALLOC_NUMERIC;
            s_after_A = what == STEP_PIVOT ? 1 : 0;
        }
        __syncthreads();                       // barrier 1
        if (!s_after_A) break;
        // step 4
        double best = __builtin_inf();
        unsigned bid = NO_ID;
        if (tid < 2 * NCTL && !in_working_set<NCTL>(s_W, tid)) candidate_bound<NCTL>(P, tid, s_x, s_d, best, bid);
        for (int i = tid; i < ncon; i += ALLOC_THREADS)
            if (!in_working_set<NCTL>(s_W, 2 * NCTL + i)) candidate_output<NCTL>(P, (size_t)i, s_x, s_d, best, bid);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ob = __shfl_xor(best, off);
            const unsigned oi = (unsigned)__shfl_xor((int)bid, off);
            take_min(best, bid, ob, oi);
        }
        if (lane == 0) { s_cand[wave] = best; s_id[wave] = bid; }
        __syncthreads();                       // barrier 2
        // step 5
        if (tid == 0) {
            double h = s_cand[0];
            unsigned id = s_id[0];
#pragma unroll
            for (int v = 1; v < ALLOC_WAVES; v++) take_min(h, id, s_cand[v], s_id[v]);
            bool ok = id != NO_ID;
            if (ok) ok = enter_and_vertex<NCTL>(P, s_W, s_k, (int)id, s_B, s_beta, s_A, s_b, s_x);
            if (ok) s_iters = s_iters + 1;
            else s_status = UCF_ALLOC_NUMERIC;
            s_after_C = ok ? 1 : 0;
        }
        __syncthreads();                       // barrier 3
        if (!s_after_C) break;
    }
    // thread 0 wrote everything it reads here itself
    if (tid == 0) {
        const size_t mo = (size_t)m * nobj + o;
        const result out = {x_out + mo * NCTL, g_out + mo, status_out + mo, iters_out + mo, work_out + mo * NCTL, lam_out + mo * NCTL,
                            xpat_out ? xpat_out + mo * NCTL : nullptr};
        write_result<NCTL>(P, out, s_status, s_iters, s_W, s_B, s_A, s_b, s_d, s_x, s_xl, s_lam);
        // an invalid member is counted once: by the workgroup of its first objective
        if (s_status == UCF_ALLOC_INVALID && o == 0) atomicAdd(nbad, 1ull);
    }
}

template <int NCTL>
void allocate_launch(const ucf_allocate_args* a, hipStream_t st)
{
    const dim3 grid((unsigned)a->nobj, (unsigned)a->nens);
    hipLaunchKernelGGL(field_allocate_kernel<NCTL>, grid, dim3(ALLOC_THREADS), 0, st, a->ncon, a->nobj, a->maxit, a->d_R, a->d_lim, a->d_w, a->d_xmax,
                       a->d_x, a->d_g, a->d_status, a->d_iters, a->d_work, a->d_lam, a->d_xpat, (unsigned long long*)a->d_nbad);
}
}  // namespace

int ucf_field_launch_allocate(const ucf_allocate_args* a, void* stream)
{
    if (!a || a->nens < 1 || a->nens > UCF_ENSEMBLE_MAX || a->ncon < 1 || a->nobj < 1 || a->nobj > UCF_ALLOC_MAX_OBJ || a->maxit < 1 ||
        a->maxit > UCF_ALLOC_MAX_ITER || !a->d_R || !a->d_lim || !a->d_w || !a->d_xmax || !a->d_x || !a->d_g || !a->d_status || !a->d_iters ||
        !a->d_work || !a->d_lam || !a->d_nbad)
        return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
#define UCF_ALLOC_CASE(N) \
    case N: allocate_launch<N>(a, st); break;
    switch (a->nctl) {
        UCF_ALLOC_CASE(1) UCF_ALLOC_CASE(2) UCF_ALLOC_CASE(3) UCF_ALLOC_CASE(4)
        UCF_ALLOC_CASE(5) UCF_ALLOC_CASE(6) UCF_ALLOC_CASE(7) UCF_ALLOC_CASE(8)
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_ALLOC_CASE
    static_assert(UCF_YIELD_MAX_CTL == 8, "one case per number of controls");
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
