// ucf_allocate.cpp -- the host half of ucf_field_allocate (include/ucf.h): ucf_allocate_solve, the linear programme of one member
// with the statements that field_allocate_kernel runs (ucf_field_allocate.h), ucf_allocate_select, the host step of the
// reliability stage, and the checks that the entries share.  No GPU is touched here.  Built without contraction, like every host
// source: the kernel is held to ucf_allocate_solve bit for bit.
#include <cmath>
#include <vector>

#include "ucf_host.h"
#include "ucf_field_allocate.h"

using namespace ucf_host;

int ucf_host::allocate_check_programme(int nctl, int nobj, const double* w, const double* xmax, int maxit)
{
    if (nctl < 1 || nctl > UCF_YIELD_MAX_CTL) return fail(UCF_ERR_BAD_ARGUMENT, "nctl=%d outside 1..%d", nctl, UCF_YIELD_MAX_CTL);
    if (nobj < 1 || nobj > UCF_ALLOC_MAX_OBJ) return fail(UCF_ERR_BAD_ARGUMENT, "nobj=%d outside 1..%d", nobj, UCF_ALLOC_MAX_OBJ);
    if (!w || !xmax) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !w ? "w" : "xmax");
    int rc = field_check_finite("w", nobj * nctl, w);
    if (rc) return rc;
    for (int c = 0; c < nctl; c++)
        if (!(xmax[c] > 0.0) || !std::isfinite(xmax[c])) return fail(UCF_ERR_BAD_ARGUMENT, "xmax[%d]=%g must be positive and finite", c, xmax[c]);
    if (maxit < 1 || maxit > UCF_ALLOC_MAX_ITER) return fail(UCF_ERR_BAD_ARGUMENT, "maxit=%d outside 1..%d", maxit, UCF_ALLOC_MAX_ITER);
    return UCF_OK;
}

int ucf_host::allocate_check_slots(int nctl, int nens, int ncon, const double* R, const double* limit_con)
{
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (ncon < 1) return fail(UCF_ERR_BAD_ARGUMENT, "ncon=%d: at least one constrained output", ncon);
    if ((long long)nens * (nctl + 1) * ncon > 0x7fffffffLL)
        return fail(UCF_ERR_BAD_ARGUMENT, "%d members x %d slots x %d constrained outputs: more than 2^31-1 values", nens, nctl + 1, ncon);
    if (!R || !limit_con) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !R ? "R" : "limit_con");
    return field_check_finite("limit_con", ncon, limit_con);
}

namespace {
using namespace ucf_alloc;

// one (member, objective): the walk of field_allocate_kernel with the ratio test in ascending id
template <int N>
void solve_one(const problem& P, int maxit, const result& out)
{
    double B[N * N], A[N * N], b[N], beta[N], x[N], xl[N], d[N], lam[N];
    int W[N];
    const int ncon = (int)P.ncon;
    bool bad = false, neg = false;
    for (int i = 0; i < ncon; i++) {
        for (int c = 0; c <= N; c++) bad = bad || !std::isfinite(P.Rm[(size_t)c * P.ncon + i]);
        neg = neg || (P.lim[i] - P.Rm[(size_t)N * P.ncon + i] < 0.0);
    }
    for (int c = 0; c < N; c++) { x[c] = 0.0; lam[c] = 0.0; W[c] = c; }
    int status = bad ? UCF_ALLOC_INVALID : neg ? UCF_ALLOC_INFEASIBLE_AT_ZERO : UCF_ALLOC_ITERATION_CAP, iters = 0;
    if (status == UCF_ALLOC_ITERATION_CAP) {
        working_rows<N>(P, W, B, beta);
        for (int it = 0; it < maxit; it++) {
            int k = 0;
            const step what = multipliers_and_direction<N>(P, W, B, A, b, lam, d, &k);
            if (what == STEP_OPTIMAL) status = UCF_ALLOC_OPTIMAL;
            if (what == STEP_NUMERIC) status = UCF_ALLOC_NUMERIC;
            if (what != STEP_PIVOT) break;
            double best = INFINITY;
            unsigned id = NO_ID;
            for (int j = 0; j < 2 * N; j++)
                if (!in_working_set<N>(W, j)) candidate_bound<N>(P, j, x, d, best, id);
            for (int i = 0; i < ncon; i++)
                if (!in_working_set<N>(W, 2 * N + i)) candidate_output<N>(P, (size_t)i, x, d, best, id);
            if (id == NO_ID || !enter_and_vertex<N>(P, W, k, (int)id, B, beta, A, b, x)) {
                status = UCF_ALLOC_NUMERIC;
                break;
            }
            iters++;
        }
    }
    write_result<N>(P, out, status, iters, W, B, A, b, d, x, xl, lam);
}
}  // namespace

extern "C" {

int ucf_allocate_solve(int nctl, int ncon, const double* R_m, const double* limit_con, int nobj, const double* w, const double* xmax, int maxit,
                       double* x, double* g, int* status, int* iters, int* work, double* lam)
{
    int rc = allocate_check_programme(nctl, nobj, w, xmax, maxit);
    if (rc || (rc = allocate_check_slots(nctl, 1, ncon, R_m, limit_con))) return rc;
    // every output may be NULL: the programme writes into staging of its own
    std::vector<double> hx((size_t)nobj * nctl), hg(nobj), hl((size_t)nobj * nctl);
    std::vector<int> hs(nobj), hi(nobj), hw((size_t)nobj * nctl);
    for (int o = 0; o < nobj; o++) {
        const problem P = {R_m, limit_con, w + (size_t)o * nctl, xmax, (size_t)ncon};
        const size_t at = (size_t)o * nctl;
        const result out = {hx.data() + at, hg.data() + o, hs.data() + o, hi.data() + o, hw.data() + at, hl.data() + at, nullptr};
#define UCF_ALLOC_CASE(N) \
    case N: solve_one<N>(P, maxit, out); break;
        switch (nctl) {
            UCF_ALLOC_CASE(1) UCF_ALLOC_CASE(2) UCF_ALLOC_CASE(3) UCF_ALLOC_CASE(4)
            UCF_ALLOC_CASE(5) UCF_ALLOC_CASE(6) UCF_ALLOC_CASE(7) UCF_ALLOC_CASE(8)
        }
#undef UCF_ALLOC_CASE
        static_assert(UCF_YIELD_MAX_CTL == 8, "one case per number of controls");
    }
    if (x) std::copy(hx.begin(), hx.end(), x);
    if (g) std::copy(hg.begin(), hg.end(), g);
    if (lam) std::copy(hl.begin(), hl.end(), lam);
    if (status) std::copy(hs.begin(), hs.end(), status);
    if (iters) std::copy(hi.begin(), hi.end(), iters);
    if (work) std::copy(hw.begin(), hw.end(), work);
    return UCF_OK;
}

int ucf_allocate_select(int nq, int nens, int nobj, int nctl, const double* quant, const double* g, const double* x, double* value, int* best,
                        double* best_x)
{
    if (nq < 1 || nq > UCF_ENSEMBLE_MAX_Q) return fail(UCF_ERR_BAD_ARGUMENT, "nq=%d outside 1..%d", nq, UCF_ENSEMBLE_MAX_Q);
    if (nens < 1 || nens > UCF_ENSEMBLE_MAX) return fail(UCF_ERR_BAD_ARGUMENT, "nens=%d outside 1..%d", nens, UCF_ENSEMBLE_MAX);
    if (nobj < 1 || nobj > UCF_ALLOC_MAX_OBJ) return fail(UCF_ERR_BAD_ARGUMENT, "nobj=%d outside 1..%d", nobj, UCF_ALLOC_MAX_OBJ);
    if (nctl < 1 || nctl > UCF_YIELD_MAX_CTL) return fail(UCF_ERR_BAD_ARGUMENT, "nctl=%d outside 1..%d", nctl, UCF_YIELD_MAX_CTL);
    if (!quant || !g || !x) return fail(UCF_ERR_BAD_ARGUMENT, "NULL %s", !quant ? "quant" : !g ? "g" : "x");
    const size_t npat = (size_t)nens * nobj;
    for (int iq = 0; iq < nq; iq++) {
        const double* qrow = quant + (size_t)iq * npat;
        for (size_t p = 0; value && p < npat; p++) value[(size_t)iq * npat + p] = qrow[p] * g[p];
        for (int o = 0; o < nobj; o++) {
            long long at = -1;
            double top = 0.0;
            for (int m = 0; m < nens; m++) {
                const size_t p = (size_t)m * nobj + o;
                const double v = qrow[p] * g[p];
                if (v == v && (at < 0 || v > top)) { top = v; at = (long long)p; }
            }
            if (best) best[(size_t)iq * nobj + o] = (int)at;
            for (int c = 0; best_x && c < nctl; c++)
                best_x[((size_t)iq * nobj + o) * nctl + c] = at < 0 ? std::nan("") : qrow[at] * x[(size_t)at * nctl + c];
        }
    }
    return UCF_OK;
}

}  // extern "C"
