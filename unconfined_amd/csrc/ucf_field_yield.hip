// ucf_field_yield.hip -- the ratio test of ucf_field_yield (include/ucf.h): per member m and rate pattern p the largest scale
// lam in [0, smax] for which the drawdown b + lam sum_c x[p][c] r_c stays at or below its limit on every constrained output.
// b and r_c are the response slots R [nens][NCTL + 1][ncon] that field_response_kernel left on the device.
//
// A workgroup of four waves takes ONE member and a tile of UCF_YIELD_PAT_TILE patterns; its lanes walk the constrained outputs
// i with stride 256.  Per i a lane loads its NCTL + 1 slot values once -- neighbouring lanes read neighbouring doubles of one
// slot row, every load is coalesced -- and uses them for every pattern of the tile.  r_c and the tile's partial results (hi,
// lo, bind per pattern, dead as one bit per pattern) live in registers: NCTL and the tile are compile-time constants and
// every loop over them unrolls, so every index is a constant (no scratch).  x[p][.] is read at wave-uniform addresses.  One
// fp64 division per (m, p, i) is the stated arithmetic and most of the work.
//
// The result is defined without order: hi is the least candidate, bind the lowest con among the outputs that attain it, lo
// the greatest candidate, dead and the non-finite flag are ORs.  So the lane partials are combined by a wave butterfly on the
// pairs (cand, con), lexicographic (con unsigned, so that "none" = -1 is the largest), plain max for lo and a ballot for the
// flags; the four waves meet in LDS.  No floating-point atomics: a call repeated gives the same bits.
//
// Built with -ffp-contract=off like ucf_field.hip: every product, sum, difference and quotient is rounded on its own.
#include <hip/hip_runtime.h>
#include "../../include/ucf.h"
#include "ucf_field.h"

namespace {
constexpr int YIELD_THREADS = 256, YIELD_WAVES = YIELD_THREADS / 64, PT = UCF_YIELD_PAT_TILE;
constexpr unsigned NO_BIND = 0xffffffffu;

// (hi, bind) <- the lexicographically smaller of it and (cand, con)
__device__ __forceinline__ void yield_take_min(double& hi, unsigned& bind, double cand, unsigned con)
{
    if (cand < hi || (cand == hi && con < bind)) { hi = cand; bind = con; }
}

template <int NCTL>
__global__ __launch_bounds__(YIELD_THREADS) void field_yield_kernel(int ncon, int npat, const double* __restrict__ R,
                                                                    const double* __restrict__ x, const double* __restrict__ lim,
                                                                    const int* __restrict__ con, double smax, double* __restrict__ y,
                                                                    double* __restrict__ fe, double* __restrict__ hi_out,
                                                                    double* __restrict__ lo_out, int* __restrict__ bind_out,
                                                                    int* __restrict__ dead_out, unsigned long long* __restrict__ nbad)
{
    __shared__ double s_hi[YIELD_WAVES][PT], s_lo[YIELD_WAVES][PT];
    __shared__ unsigned s_bind[YIELD_WAVES][PT], s_dead[YIELD_WAVES], s_bad[YIELD_WAVES];
    const int m = blockIdx.y, p0 = blockIdx.x * PT;
    const size_t nc = (size_t)ncon;
    const double* Rm = R + (size_t)m * (NCTL + 1) * nc;
    double hi[PT], lo[PT];
    unsigned bind[PT], dead = 0;
    bool bad = false;
#pragma unroll
    for (int t = 0; t < PT; t++) { hi[t] = smax; lo[t] = 0.0; bind[t] = NO_BIND; }
    for (int i = threadIdx.x; i < ncon; i += YIELD_THREADS) {
        double r[NCTL];
#pragma unroll
        for (int c = 0; c < NCTL; c++) {
            r[c] = Rm[(size_t)c * nc + i];
            bad = bad || !isfinite(r[c]);
        }
        const double b = Rm[(size_t)NCTL * nc + i];
        bad = bad || !isfinite(b);
        const double room = lim[i] - b;
        const unsigned ci = (unsigned)con[i];
#pragma unroll
        for (int t = 0; t < PT; t++) {
            // a tile that reaches past the last pattern works on the last one again and stores nothing for it
            const double* xp = x + (size_t)min(p0 + t, npat - 1) * NCTL;
            double D = 0.0;
#pragma unroll
            for (int c = 0; c < NCTL; c++) D = D + xp[c] * r[c];
            const double cand = room / D;                // used only where D != 0
            if (D > 0.0) yield_take_min(hi[t], bind[t], cand, ci);
            if (D < 0.0 && cand > lo[t]) lo[t] = cand;
            if (D == 0.0 && room < 0.0) dead |= 1u << t;
        }
    }
    // every lane of every wave arrives here
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned wave_dead = 0;
#pragma unroll
    for (int t = 0; t < PT; t++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ohi = __shfl_xor(hi[t], off), olo = __shfl_xor(lo[t], off);
            const unsigned ob = (unsigned)__shfl_xor((int)bind[t], off);
            yield_take_min(hi[t], bind[t], ohi, ob);
            if (olo > lo[t]) lo[t] = olo;
        }
        if (__ballot((dead >> t) & 1u) != 0) wave_dead |= 1u << t;
        if (lane == 0) {
            s_hi[wave][t] = hi[t];
            s_lo[wave][t] = lo[t];
            s_bind[wave][t] = bind[t];
        }
    }
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0) {
        s_dead[wave] = wave_dead;
        s_bad[wave] = any_bad ? 1u : 0u;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < PT && p0 + t < npat) {
        double h = s_hi[0][t], l = s_lo[0][t];
        unsigned bd = s_bind[0][t], dd = s_dead[0], invalid = s_bad[0];
#pragma unroll
        for (int w = 1; w < YIELD_WAVES; w++) {
            yield_take_min(h, bd, s_hi[w][t], s_bind[w][t]);
            if (s_lo[w][t] > l) l = s_lo[w][t];
            dd |= s_dead[w];
            invalid |= s_bad[w];
        }
        const int is_dead = (int)((dd >> t) & 1u);
        const bool feas = is_dead == 0 && l <= h;
        const double nan = __builtin_nan("");
        const size_t o = (size_t)m * npat + (p0 + t);
        y[o] = invalid ? nan : (feas ? h : 0.0);
        fe[o] = invalid ? nan : (feas ? 1.0 : 0.0);
        hi_out[o] = invalid ? nan : h;
        lo_out[o] = invalid ? nan : l;
        bind_out[o] = invalid ? -1 : (int)bd;
        dead_out[o] = invalid ? 0 : is_dead;
        // an invalid member is counted once: by the workgroup of its first tile
        if (invalid && p0 + t == 0) atomicAdd(nbad, 1ull);
    }
}

template <int NCTL>
void yield_launch(const ucf_yield_args* a, hipStream_t st)
{
    const dim3 grid((unsigned)((a->npat + PT - 1) / PT), (unsigned)a->nens);
    hipLaunchKernelGGL(field_yield_kernel<NCTL>, grid, dim3(YIELD_THREADS), 0, st, a->ncon, a->npat, a->d_R, a->d_x, a->d_lim, a->d_con, a->smax,
                       a->d_y, a->d_fe, a->d_hi, a->d_lo, a->d_bind, a->d_dead, (unsigned long long*)a->d_nbad);
}
}  // namespace

int ucf_field_launch_yield(const ucf_yield_args* a, void* stream)
{
    if (!a || a->nens < 1 || a->nens > UCF_ENSEMBLE_MAX || a->ncon < 1 || a->npat < 1 || a->npat > UCF_YIELD_MAX_PAT || !a->d_R || !a->d_x ||
        !a->d_lim || !a->d_con || !a->d_y || !a->d_fe || !a->d_hi || !a->d_lo || !a->d_bind || !a->d_dead || !a->d_nbad)
        return UCF_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
#define UCF_YIELD_CASE(N) \
    case N: yield_launch<N>(a, st); break;
    switch (a->nctl) {
        UCF_YIELD_CASE(1) UCF_YIELD_CASE(2) UCF_YIELD_CASE(3) UCF_YIELD_CASE(4)
        UCF_YIELD_CASE(5) UCF_YIELD_CASE(6) UCF_YIELD_CASE(7) UCF_YIELD_CASE(8)
    default: return UCF_ERR_BAD_ARGUMENT;
    }
#undef UCF_YIELD_CASE
    static_assert(UCF_YIELD_MAX_CTL == 8, "one case per number of controls");
    return hipGetLastError() == hipSuccess ? UCF_OK : UCF_ERR_HIP;
}
