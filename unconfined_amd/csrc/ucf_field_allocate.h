// ucf_field_allocate.h -- the serial steps of the active-set simplex of ucf_field_allocate (include/ucf.h), written once for
// field_allocate_kernel (ucf_field_allocate.hip) and for its host twin ucf_allocate_solve (ucf_allocate.cpp): both translation
// units are built with -ffp-contract=off, so the same statements give the same bits on either side.  The ratio test, the one
// parallel step, is stated here per constraint (candidate_bound, candidate_output) and combined with take_min, which is defined
// without order; how the constraints are walked is each side's own business.
//
// N = nctl is a template argument: every loop below has a compile-time bound.
#pragma once
#include <cmath>

#include "../../include/ucf.h"

#if defined(__HIPCC__)
#define UCF_ALLOC_HD __host__ __device__ __forceinline__
#else
#define UCF_ALLOC_HD inline
#endif

namespace ucf_alloc {
constexpr unsigned NO_ID = 0xffffffffu;        // "no constraint": above every id
enum step { STEP_PIVOT = 0, STEP_OPTIMAL = 1, STEP_NUMERIC = 2 };

// One member's slots R_m [N + 1][ncon] and what else a programme reads
struct problem {
    const double* Rm;      // [N + 1][ncon]
    const double* lim;     // [ncon]
    const double* w;       // [N] the objective
    const double* xmax;    // [N]
    size_t ncon;
};

// A x = b by Gaussian elimination with partial pivoting: the pivot of column `col` is the entry of largest magnitude among the
// rows col .. N-1, the lowest row among equals.  A [N][N] and b [N] are destroyed.  false: a pivot is zero or not finite.
template <int N>
UCF_ALLOC_HD bool solve(double* A, double* b, double* x)
{
    for (int col = 0; col < N; col++) {
        int piv = col;
        double best = fabs(A[col * N + col]);
        for (int r = col + 1; r < N; r++) {
            const double v = fabs(A[r * N + col]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 0.0) || !(best <= 1.7976931348623157e308)) return false;
        if (piv != col) {
            for (int c = 0; c < N; c++) { const double t = A[col * N + c]; A[col * N + c] = A[piv * N + c]; A[piv * N + c] = t; }
            const double t = b[col]; b[col] = b[piv]; b[piv] = t;
        }
        for (int r = col + 1; r < N; r++) {
            const double f = A[r * N + col] / A[col * N + col];
            for (int c = col + 1; c < N; c++) A[r * N + c] = A[r * N + c] - f * A[col * N + c];
            b[r] = b[r] - f * b[col];
        }
    }
    for (int r = N - 1; r >= 0; r--) {
        double s = b[r];
        for (int c = r + 1; c < N; c++) s = s - A[r * N + c] * x[c];
        x[r] = s / A[r * N + r];
    }
    return true;
}

// row a [N] and right-hand side of constraint `id`: a . x <= beta
template <int N>
UCF_ALLOC_HD double row_of(const problem& P, int id, double* a)
{
    if (id < 2 * N) {
        const int own = id < N ? id : id - N;
        for (int c = 0; c < N; c++) a[c] = 0.0;
        a[own] = id < N ? -1.0 : 1.0;
        return id < N ? 0.0 : P.xmax[own];
    }
    const size_t i = (size_t)(id - 2 * N);
    for (int c = 0; c < N; c++) a[c] = P.Rm[(size_t)c * P.ncon + i];
    return P.lim[i] - P.Rm[(size_t)N * P.ncon + i];
}

// B [N][N] = the rows of the working set W, beta [N] their right-hand sides
template <int N>
UCF_ALLOC_HD void working_rows(const problem& P, const int* W, double* B, double* beta)
{
    for (int s = 0; s < N; s++) beta[s] = row_of<N>(P, W[s], B + s * N);
}

// Steps 1 to 3.  B [N][N] holds the working rows (working_rows); A [N][N] and b [N] are scratch.  lam [N] is written; with
// STEP_PIVOT *k is the leaving slot and d [N] the direction.
template <int N>
UCF_ALLOC_HD step multipliers_and_direction(const problem& P, const int* W, const double* B, double* A, double* b, double* lam, double* d, int* k)
{
    for (int r = 0; r < N; r++) {
        for (int c = 0; c < N; c++) A[r * N + c] = B[c * N + r];
        b[r] = P.w[r];
    }
    if (!solve<N>(A, b, lam)) return STEP_NUMERIC;
    int slot = -1;
    unsigned lowest = NO_ID;
    for (int s = 0; s < N; s++)
        if (lam[s] < 0.0 && (unsigned)W[s] < lowest) { lowest = (unsigned)W[s]; slot = s; }
    if (slot < 0) return STEP_OPTIMAL;
    for (int r = 0; r < N; r++) {
        for (int c = 0; c < N; c++) A[r * N + c] = B[r * N + c];
        b[r] = r == slot ? -1.0 : 0.0;
    }
    if (!solve<N>(A, b, d)) return STEP_NUMERIC;
    *k = slot;
    return STEP_PIVOT;
}

// Step 5: slot k takes `enter`; B and beta are rebuilt, x is solved for on the new working set.  false: NUMERIC.
template <int N>
UCF_ALLOC_HD bool enter_and_vertex(const problem& P, int* W, int k, int enter, double* B, double* beta, double* A, double* b, double* x)
{
    W[k] = enter;
    working_rows<N>(P, W, B, beta);
    for (int r = 0; r < N; r++) {
        for (int c = 0; c < N; c++) A[r * N + c] = B[r * N + c];
        b[r] = beta[r];
    }
    return solve<N>(A, b, x);
}

template <int N>
UCF_ALLOC_HD bool in_working_set(const int* W, int id)
{
    bool in = false;
    for (int s = 0; s < N; s++) in = in || W[s] == id;
    return in;
}

// (best, id) <- the lexicographically smaller of it and (cand, cid); a NaN cand passes no comparison
UCF_ALLOC_HD void take_min(double& best, unsigned& id, double cand, unsigned cid)
{
    if (cand < best || (cand == best && cid < id)) { best = cand; id = cid; }
}

// Step 4 for one constraint outside the working set: D = a . d, slack = beta - a . x
// and S the scale that D's rounding is measured against: a D that is not above UCF_ALLOC_DTOL S is zero up to rounding (the
// twin of a row of the working set, a row through the vertex along an edge) and must not enter -- B would be singular
UCF_ALLOC_HD void candidate(double D, double S, double slack, unsigned cid, double& best, unsigned& id)
{
    if (D > UCF_ALLOC_DTOL * S) {
        if (slack < 0.0) slack = 0.0;
        take_min(best, id, slack / D, cid);
    }
}
template <int N>
UCF_ALLOC_HD void candidate_bound(const problem& P, int id, const double* x, const double* d, double& best, unsigned& bid)
{
    const int own = id < N ? id : id - N;
    const double D = id < N ? -d[own] : d[own];
    const double slack = id < N ? x[own] : P.xmax[own] - x[own];
    double dmax = 0.0;
    for (int c = 0; c < N; c++) dmax = fabs(d[c]) > dmax ? fabs(d[c]) : dmax;
    candidate(D, dmax, slack, (unsigned)id, best, bid);
}
template <int N>
UCF_ALLOC_HD void candidate_output(const problem& P, size_t i, const double* x, const double* d, double& best, unsigned& bid)
{
    double D = 0.0, S = 0.0, ax = 0.0;
    for (int c = 0; c < N; c++) {
        const double r = P.Rm[(size_t)c * P.ncon + i];
        const double rd = r * d[c];
        D = D + rd;
        S = S + fabs(rd);
        ax = ax + r * x[c];
    }
    const double beta = P.lim[i] - P.Rm[(size_t)N * P.ncon + i];
    candidate(D, S, beta - ax, (unsigned)(2 * N) + (unsigned)i, best, bid);
}

// What one (member, objective) returns: x, lam [N], work [N]
struct result {
    double* x;
    double* g;
    int* status;
    int* iters;
    int* work;
    double* lam;
    double* xpat;          // NULL ok: the pattern of the reliability stage, x where status is 0 and +0.0 elsewhere
};

// ---- the polish of the optimum: x and g in double-double (a value is hi + lo, |lo| <= ulp(hi) / 2), so that what is returned is
// the vertex of the final working set and its value rounded once, not the sum of the roundings of one elimination.
// s + err = a + b exactly (Knuth)
UCF_ALLOC_HD void two_sum(double a, double b, double& s, double& err)
{
    s = a + b;
    const double bb = s - a;
    err = (a - (s - bb)) + (b - bb);
}
// (h, l) <- (h, l) + (p, e), renormalised
UCF_ALLOC_HD void dd_add(double& h, double& l, double p, double e)
{
    double s, t;
    two_sum(h, p, s, t);
    const double low = l + (t + e);
    h = s + low;
    l = low - (h - s);
}
// (h, l) <- (h, l) + sign * a * (xh + xl): the product a * xh exactly (one fma), a * xl rounded
UCF_ALLOC_HD void dd_add_product(double& h, double& l, double sign, double a, double xh, double xl)
{
    const double p = a * xh;
    const double e = fma(a, xh, -p);
    dd_add(h, l, sign * p, sign * (e + a * xl));
}
// Two steps of iterative refinement of x on the rows B of the final working set: the residual beta - B x in double-double (beta
// of an output row = limit - b exactly, by two_sum), the correction from the same elimination.  x [N] becomes the high part, xl
// [N] the low part.  A [N][N], b [N], e [N] are scratch.  The elimination succeeded on this B in step 5 (or B is -I): it succeeds.
template <int N>
UCF_ALLOC_HD void polish_vertex(const problem& P, const int* W, const double* B, double* A, double* b, double* e, double* x, double* xl)
{
    for (int c = 0; c < N; c++) xl[c] = 0.0;
    for (int pass = 0; pass < 2; pass++) {
        for (int s = 0; s < N; s++) {
            double h, l = 0.0;
            if (W[s] < 2 * N) h = W[s] < N ? 0.0 : P.xmax[W[s] - N];
            else two_sum(P.lim[W[s] - 2 * N], -P.Rm[(size_t)N * P.ncon + (size_t)(W[s] - 2 * N)], h, l);
            for (int c = 0; c < N; c++) dd_add_product(h, l, -1.0, B[s * N + c], x[c], xl[c]);
            b[s] = h;
            for (int c = 0; c < N; c++) A[s * N + c] = B[s * N + c];
        }
        if (!solve<N>(A, b, e)) return;
        for (int c = 0; c < N; c++) dd_add(x[c], xl[c], e[c], 0.0);
    }
}

// the outputs of a programme that ended with `status` after `iters` pivots; W, B (the rows of W), x, lam are read where status
// is UCF_ALLOC_OPTIMAL, and x is polished in place; A [N][N], b, e, xl [N] are scratch
template <int N>
UCF_ALLOC_HD void write_result(const problem& P, const result& out, int status, int iters, const int* W, const double* B, double* A, double* b,
                               double* e, double* x, double* xl, const double* lam)
{
    const double nan = __builtin_nan("");
    *out.status = status;
    *out.iters = iters;
    if (status != UCF_ALLOC_OPTIMAL) {
        *out.g = nan;
        for (int c = 0; c < N; c++) {
            out.x[c] = nan;
            out.lam[c] = nan;
            out.work[c] = -1;
            if (out.xpat) out.xpat[c] = 0.0;
        }
        return;
    }
    polish_vertex<N>(P, W, B, A, b, e, x, xl);
    double g = 0.0, gl = 0.0;
    for (int c = 0; c < N; c++) {
        dd_add_product(g, gl, 1.0, P.w[c], x[c], xl[c]);
        out.x[c] = x[c];
        if (out.xpat) out.xpat[c] = x[c];
    }
    *out.g = g;
    // work ascending, lam with it: insertion into the output (the ids of a working set are distinct)
    for (int s = 0; s < N; s++) {
        out.work[s] = W[s];
        out.lam[s] = lam[s];
        for (int j = s; j > 0; j--)
            if (out.work[j - 1] > out.work[j]) {
                const int ti = out.work[j]; out.work[j] = out.work[j - 1]; out.work[j - 1] = ti;
                const double tl = out.lam[j]; out.lam[j] = out.lam[j - 1]; out.lam[j - 1] = tl;
            }
    }
}
}  // namespace ucf_alloc
