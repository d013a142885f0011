// ucf_plan.cpp -- plans: input validation, non-dimensionalisation, the quadrature tables, create / update / destroy and
// the accessors.
//
// Plan creation restates the numerical half of the reference's read_input and the
// driver's `first`-time setup (reference driver_io.f90:159-186,531-567,628-647;
// driver.f90:79-91,121-126,138-151,179-183; integration.f90:31-120) on the host:
// these run once, their results (J0 zeros, tanh-sinh weights, Gauss-Lobatto nodes)
// are uploaded once and stay resident.
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ucf_host.h"

using namespace ucf_host;

namespace {

// ---- driver_io.f90:628-647: Newton on J0 from the asymptotic guess (i+3/4)*pi
void j0_zeros(int n, double* z)
{
    const double PI = 4.0 * std::atan(1.0);
    for (int i = 0; i < n; i++) {
        double x = (i + 0.75) * PI;
        for (int it = 0; it < 100; it++) {
            const double dx = j0(x) / j1(x);
            x = x + dx;
            if (std::fabs(dx) < std::nextafter(std::fabs(x), INFINITY) - std::fabs(x)) break;   // spacing(x)
        }
        z[i] = x;
    }
}

// ---- integration.f90:31-67: weights of a 2^k-1 point rule (sum normalised to 2) and, on
// request, tanh(u2)+1 (the abscissa on [0,s] is (that)*s/2, applied per point on the device)
void tanh_sinh_level(int k, double* w, double* x_unit)
{
    const double PIOV2 = 2.0 * std::atan(1.0);
    const int N = (1 << k) - 1, r = (N - 1) / 2;
    const double h = 4.0 / (double)(1 << k);
    std::vector<double> u2(N);
    for (int i = -r; i <= r; i++) {
        const double u1 = PIOV2 * std::cosh(h * i);
        u2[i + r] = PIOV2 * std::sinh(h * i);
        const double c = std::cosh(u2[i + r]);
        w[i + r] = u1 / (c * c);
    }
    double sum = 0.0;
    for (int i = 0; i < N; i++) sum = sum + w[i];
    for (int i = 0; i < N; i++) w[i] = 2.0 * w[i] / sum;
    if (x_unit)
        for (int i = 0; i < N; i++) x_unit[i] = std::tanh(u2[i]) + 1.0;
}

// ---- integration.f90:70-120: Newton on the Legendre recurrence; interior nodes only
void gauss_lobatto(int ord, double* xo, double* wo)
{
    const int N = ord - 1, N1 = N + 1;
    const double PI = 4.0 * std::atan(1.0);
    std::vector<double> Pm((size_t)ord * ord, 0.0), x(ord), xold(ord, 2.0);
    auto PP = [&](int i, int k) -> double& { return Pm[(size_t)(k - 1) * ord + i]; };
    for (int i = 0; i <= N; i++) x[i] = std::cos(PI * i / N);
    for (int it = 0; it < 1000; it++) {
        double mx = 0.0;
        for (int i = 0; i < ord; i++) mx = std::fmax(mx, std::fabs(x[i] - xold[i]));
        if (!(mx > DBL_EPSILON)) break;
        for (int i = 0; i < ord; i++) { xold[i] = x[i]; PP(i, 1) = 1.0; PP(i, 2) = x[i]; }
        for (int k = 2; k <= N; k++)
            for (int i = 0; i < ord; i++) PP(i, k + 1) = ((2 * k - 1) * x[i] * PP(i, k) - (k - 1) * PP(i, k - 1)) / k;
        for (int i = 0; i < ord; i++) x[i] = xold[i] - (x[i] * PP(i, N1) - PP(i, N)) / (N1 * PP(i, N1));
    }
    for (int i = 1; i <= ord - 2; i++) {
        xo[i - 1] = x[i];
        wo[i - 1] = 2.0 / ((N * N1) * (PP(i, N1) * PP(i, N1)));
    }
}

// (sin, cos)(k pi / 128), k = 0..255, correctly rounded (80-bit evaluation of the first octant) and exactly symmetric:
// the zeros and ones of the table are exact, every other entry appears with the same bits wherever symmetry repeats it
void sincos_table(double* tab /* [256][2] */)
{
    const long double a = 3.14159265358979323846264338327950288L / 128.0L;
    double s64[65], c64[65];
    for (int j = 0; j <= 32; j++) { s64[j] = (double)sinl(j * a); c64[j] = (double)cosl(j * a); }
    s64[0] = 0.0; c64[0] = 1.0;
    s64[32] = c64[32] = (double)sqrtl(0.5L);
    for (int j = 33; j <= 64; j++) { s64[j] = c64[64 - j]; c64[j] = s64[64 - j]; }
    for (int k = 0; k < 256; k++) {
        const int q = k / 64, j = k % 64;
        double sn, cs;
        switch (q) {
        case 0: sn = s64[j]; cs = c64[j]; break;
        case 1: sn = c64[j]; cs = -s64[j]; break;
        case 2: sn = -s64[j]; cs = -c64[j]; break;
        default: sn = -c64[j]; cs = s64[j]; break;
        }
        tab[2 * k] = sn;
        tab[2 * k + 1] = (cs == 0.0) ? 0.0 : cs;      // (no negative zero)
    }
}

// 2^(j/128), j = 0..127, as (hi, lo): hi correctly rounded, hi + lo good to the 64 bits of the 80-bit evaluation
void exp2_table(double* tab /* [128][2] */)
{
    for (int j = 0; j < 128; j++) {
        const long double v = exp2l((long double)j / 128.0L);
        tab[2 * j] = (double)v;
        tab[2 * j + 1] = (double)(v - (long double)tab[2 * j]);
    }
}

// Everything of a plan that depends on the parameters.  create: also the quadrature tables (which depend only on the
// numerical settings k, R, ord, nacc, the J0 split) and the device allocation.  !create (ucf_plan_update): the new set
// must leave those settings and the model alone; only the parameter-dependent table segments (finite-difference
// exponentials, pumping schedule) are uploaded again.
int plan_set_params(ucf_plan* pl, const ucf_params& Pin, bool create)
{
    ucf_params Pn = Pin;
    if (Pn.tol < DBL_EPSILON) Pn.tol = DBL_EPSILON;                  // driver_io.f90:311-314
    if (!create) {
        const ucf_params& O = pl->P;
        const bool same = O.model == Pn.model && O.MNtype == Pn.MNtype && O.order == Pn.order && O.timeType == Pn.timeType &&
                          O.MoenchM == Pn.MoenchM && O.M == Pn.M && O.k == Pn.k && O.R == Pn.R && O.nacc == Pn.nacc && O.ord == Pn.ord &&
                          O.j0s[0] == Pn.j0s[0] && O.j0s[1] == Pn.j0s[1];
        if (!same)
            return fail(UCF_ERR_BAD_ARGUMENT, "ucf_plan_update: the model and the numerical settings (M, k, R, nacc, ord, J0 split, "
                                              "schedule length, FD order, number of Moench terms) must stay as they are; create a new plan");
    }
    pl->P = Pn;
    const ucf_params& P = pl->P;
    nondimensionalise(P, pl->D);
    const ucf_derived& D = pl->D;
    const int N = D.N, R = P.R, ngl = P.ord - 2;
    ucf_dev_params& dp = pl->dev;
    if (create) {
        (void)hipGetDevice(&pl->device);
        pl->h_j0z = (double*)std::malloc(sizeof(double) * D.nj0z);
        pl->h_ts_x = (double*)std::malloc(sizeof(double) * N);
        pl->h_ts_w = (double*)std::calloc((size_t)R * N, sizeof(double));
        pl->h_gl_x = (double*)std::malloc(sizeof(double) * ngl);
        pl->h_gl_w = (double*)std::malloc(sizeof(double) * ngl);
        j0_zeros(D.nj0z, pl->h_j0z);
        for (int j = 1; j <= R; j++) {                                    // driver.f90:86-91
            const int kv = P.k - R + j;
            pl->Nv[j - 1] = (1 << kv) - 1;
            dp.hv[j - 1] = 4.0 / (double)(1 << kv);
            tanh_sinh_level(kv, pl->h_ts_w + (size_t)(j - 1) * N, (j == R) ? pl->h_ts_x : nullptr);
        }
        gauss_lobatto(P.ord, pl->h_gl_x, pl->h_gl_w);
    }

    // FD table exp(-beta1*(j-1)*h)  (laplace_hankel_solutions.f90:494)
    std::vector<double> fd_e;
    if (P.model == 6 && P.MNtype == 2) {
        const double h = D.usLD / (double)(P.order - 1);
        const double beta1 = -D.lambdaD;
        fd_e.resize(P.order);
        for (int j = 1; j <= P.order; j++) fd_e[j - 1] = std::exp(-(beta1 * (double)(j - 1) * h));
        dp.fd_h = h;
        dp.fd_invhsq = 1.0 / (h * h);
        dp.fd_beta0 = D.ac_eff * P.Sy / P.Ss;
        dp.fd_beta3 = D.akD;
        dp.fd_expmb2 = std::exp(-(P.ak * D.b1));
        {   // constants of the unit-coefficient form of the elimination recurrence (fd_inverse_B2, ucf_device.h)
            const double K = (dp.fd_invhsq - dp.fd_beta3 / h) * dp.fd_invhsq;
            dp.fd_isk = (K > 0.0 && std::isfinite(K)) ? 1.0 / std::sqrt(K) : 0.0;
            dp.fd_gmax = std::exp2(500.0 / (double)P.order) - 1.0;
        }
    }
    if (P.model == 2) {                                               // laplace_hankel_solutions.f90:250-253
        const double PI = 4.0 * std::atan(1.0);
        dp.hs_rDw = D.rDw;
        dp.hs_CDw = D.rDw * D.rDw / (2.0 * (D.l_eff - D.d_eff) * P.Ss);
        dp.hs_tDb = PI * (D.rDwobs * D.rDwobs) / (P.sF * P.Ss);
    }
    if (P.model == 6 && P.MNtype == 1) {                              // :420-427
        const double beta0 = P.ak * P.b;
        const double phiDa = P.psia / P.b, phiDk = P.psik / P.b;
        dp.mn_vartheta = beta0 * P.Sy / (P.Ss * P.b) * std::exp(-(beta0 * (phiDa - phiDk)));
        dp.mn_u0 = beta0 / 2.0;
        dp.mn_c3 = 1.0 / (P.kappa * dp.mn_u0 * dp.mn_u0);
    }

    // pumping schedules: increments and their sum, once.  Piecewise constant (time.f90:81-95): rate increments
    // Q_k - Q_{k-1}; piecewise linear (time.f90:97-122): slope increments W_k - W_{k-1}, W_k = (y_{k+1} - y_k) /
    // (t_{k+1} - t_k) with y_1 = 0 at t_1 and the n given rates at t_2..t_n, t_f (see ucf.h on the reading)
    std::vector<double> sched;
    if (P.timeType < 0) {
        const bool linear = P.timeType <= -101;
        const int n = linear ? -P.timeType - 100 : -P.timeType;
        sched.resize(2 * n + 2);
        double prev = 0.0, sum = 0.0, yprev = 0.0;
        for (int k = 0; k < n; k++) {
            double cur = P.timeParExt[n + 1 + k];
            if (linear) {
                const double denom = P.timeParExt[k + 1] - P.timeParExt[k];
                const double w = (cur - yprev) / denom;       // rise / run                        (:113)
                yprev = cur;
                cur = w;
            }
            const double dq = cur - prev;
            prev = cur;
            sched[k] = P.timeParExt[k];
            sched[n + k] = dq;
            sum = (k == 0) ? dq : sum + dq;
        }
        sched[2 * n] = P.timeParExt[n];
        sched[2 * n + 1] = sum;
    }
    if (create) {
        // one device allocation for all tables
        const size_t n_tab = (size_t)N + (size_t)R * N + 2 * (size_t)ngl + D.nj0z + fd_e.size() + sched.size() + 1 + 2 * UCF_SC_ENTRIES;
        std::vector<double> host(n_tab);
        size_t o = 0;
        pl->o_tsx = o; std::memcpy(&host[o], pl->h_ts_x, sizeof(double) * N); o += N;
        pl->o_tsw = o; std::memcpy(&host[o], pl->h_ts_w, sizeof(double) * (size_t)R * N); o += (size_t)R * N;
        pl->o_glx = o; std::memcpy(&host[o], pl->h_gl_x, sizeof(double) * ngl); o += ngl;
        pl->o_glw = o; std::memcpy(&host[o], pl->h_gl_w, sizeof(double) * ngl); o += ngl;
        pl->o_j0z = o; std::memcpy(&host[o], pl->h_j0z, sizeof(double) * D.nj0z); o += D.nj0z;
        pl->o_fde = o; if (!fd_e.empty()) std::memcpy(&host[o], fd_e.data(), sizeof(double) * fd_e.size());
        o += fd_e.size();
        pl->o_sched = o; if (!sched.empty()) std::memcpy(&host[o], sched.data(), sizeof(double) * sched.size());
        o += sched.size();
        o += (o & 1);                                    // 16-byte alignment: the kernels read the table as double2
        pl->o_sct = o; sincos_table(&host[o]); exp2_table(&host[o + 512]);
        pl->tables_bytes = n_tab * sizeof(double);
        if (hipMalloc((void**)&pl->d_tables, pl->tables_bytes) != hipSuccess)
            return fail(UCF_ERR_NOMEM, "hipMalloc of %zu table bytes failed", pl->tables_bytes);
        if (hipMemcpy(pl->d_tables, host.data(), pl->tables_bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(UCF_ERR_HIP, "table upload failed");
    } else if (!fd_e.empty() || !sched.empty()) {
        {   // launches of the old parameter set may still read them: wait for the plan's own streams (not the device)
            std::lock_guard<std::mutex> g(pl->mu);
            for (ucf_workspace* w : pl->ws) (void)hipStreamSynchronize((hipStream_t)w->stream);
        }
        if (!fd_e.empty() && hipMemcpy(pl->d_tables + pl->o_fde, fd_e.data(), sizeof(double) * fd_e.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(UCF_ERR_HIP, "table upload failed");
        if (!sched.empty() && hipMemcpy(pl->d_tables + pl->o_sched, sched.data(), sizeof(double) * sched.size(), hipMemcpyHostToDevice) != hipSuccess)
            return fail(UCF_ERR_HIP, "table upload failed");
    }

    dp.model = P.model; dp.MNtype = P.MNtype; dp.order = P.order; dp.timeType = P.timeType; dp.MoenchM = P.MoenchM;
    dp.M = P.M; dp.np = D.np; dp.k = P.k; dp.N = N; dp.R = R; dp.nacc = P.nacc; dp.ngl = ngl; dp.nz = 0;
    dp.nj0z = D.nj0z;
    dp.timePar[0] = P.timePar[0]; dp.timePar[1] = P.timePar[1];
    dp.kappa = P.kappa; dp.alphaD = D.alphaD; dp.beta = P.beta;
    dp.lD = D.lD; dp.dD = D.dD; dp.bD = D.bD; dp.dD1 = 1.0 - D.dD; dp.lD1 = 1.0 - D.lD;
    for (int m = 0; m < P.MoenchM; m++) dp.MoenchInvGamma[m] = 1.0 / D.MoenchGamma[m];
    dp.alpha = P.alpha; dp.logtol = std::log(P.tol); dp.maxexp = -std::log(DBL_EPSILON) / 3.0;   // constants.f90:66
    dp.inv_kappa = 1.0 / P.kappa;
    dp.half_inv_kappa = 0.5 * dp.inv_kappa;
    dp.inv_bD = 1.0 / D.bD;
    dp.fold_dD = (D.dD == 0.0);                       // sinh(eta*0) == 0 exactly
    dp.fold_lD1 = (dp.lD1 == 0.0);
    // cosh(eta (dD1 - 1)) of the water-table value (:175 at zD = 1) next to sinh(eta dD) (:176): dD1 - 1 = -(dD - delta)
    // with |delta| <= 2^-53 (the rounding of 1 - dD), delta = (dD1 - 1) + dD exactly.  delta = 0: the same number bit for
    // bit (1); else cosh(eta dD) - eta delta sinh(eta dD), exact to (eta delta)^2 < 1e-26 (2): no primitive of its own
    dp.g1_delta = (dp.dD1 - 1.0) + D.dD;
    dp.share_g1top = (dp.g1_delta == 0.0) ? 1 : (std::fabs(dp.g1_delta) < 1.0e-15 ? 2 : 0);
    // the fast path is only used where the REFERENCE's own intermediates stay finite (beyond that its results are
    // shaped by Inf/NaN and the in-band rules, which the generic evaluator reproduces): no cosh/sinh (<= e^{Re eta})
    // and none of the products of two of them that the reference forms may overflow.  Refined per call in
    // fill_call_params (the products depend on the depths).
    dp.fast_eta_max = (dp.fold_dD && dp.fold_lD1) ? 700.0 : 350.0;      // (refined per call from the depths, fill_call_params)
    dp.ts_x = pl->d_tables + pl->o_tsx;
    dp.ts_w = pl->d_tables + pl->o_tsw;
    dp.gl_x = pl->d_tables + pl->o_glx;
    dp.gl_w = pl->d_tables + pl->o_glw;
    dp.j0z = pl->d_tables + pl->o_j0z;
    dp.fd_e = pl->d_tables + pl->o_fde;
    dp.sched = pl->d_tables + pl->o_sched;
    dp.sc_tab = pl->d_tables + pl->o_sct;
    return UCF_OK;
}

// distinct kernel names of the last timed call (pointers into the timer set)
const char** names_scratch(ucf_workspace* ws) { return ws->tm_names; }
}  // namespace

namespace ucf_host {

// ---- driver_io.f90:88-333: the checks read_input performs before stopping
int validate(const ucf_params& P)
{
    if (P.model < 0 || P.model > 6) return fail(UCF_ERR_INVALID_MODEL, "invalid model choice %d (valid: 0..6)", P.model);
    if (P.model == 3 && P.MoenchM < 1) return fail(UCF_ERR_MOENCH, "number of Moench alphas must be >= 1 for model 3");
    if (P.MoenchM > UCF_MAX_MOENCH) return fail(UCF_ERR_MOENCH, "more than %d Moench alphas", UCF_MAX_MOENCH);
    if (P.model > 0 && (P.gammaSkin < 0.0 || P.d < 0.0 || P.l < 0.0))
        return fail(UCF_ERR_GEOMETRY, "negative geometry parameters (gamma, d, l)");
    if (P.b <= 0.0 || P.Kr <= 0.0 || P.Ss <= 0.0) return fail(UCF_ERR_AQUIFER, "zero or negative aquifer parameters (b, Kr, Ss)");
    if (P.model > 2 && (P.kappa <= 0.0 || P.Sy <= 0.0))
        return fail(UCF_ERR_AQUIFER, "zero or negative unconfined aquifer parameters (kappa, Sy)");
    double l = P.l, d = P.d;
    if (P.MNtype == 1) {                     // overrides happen before the check in the reference (:159-186)
        if (std::fabs(l - P.b) > FLT_EPSILON) l = P.b;
        if (d > FLT_EPSILON) d = 0.0;
    }
    if (P.model > 0 && d >= l) return fail(UCF_ERR_GEOMETRY, "screen top/bottom: l must be > d (l=%g d=%g)", l, d);
    if (P.model == 6) {
        if (P.ac < 0.0 || P.ak < 0.0 || P.usL < 0.0 || P.psia < 0.0 || P.psik < 0.0)
            return fail(UCF_ERR_MISHRA_NEUMAN, "invalid Mishra/Neuman parameters (a_c, a_k, L, psi_a, psi_k)");
        if (P.MNtype == 2 && P.order < 3) return fail(UCF_ERR_MISHRA_NEUMAN, "Mishra/Neuman finite difference order must be >= 3");
        if (P.MNtype == 0)
            return fail(UCF_ERR_UNSUPPORTED, "Mishra/Neuman type 0 is the quad-precision ARB path, excluded from this build");
        if (P.MNtype < 0 || P.MNtype > 2) return fail(UCF_ERR_MISHRA_NEUMAN, "invalid Mishra/Neuman solution type %d", P.MNtype);
    }
    if ((P.model == 4 || P.model == 5) && P.beta < 0.0) return fail(UCF_ERR_MALAMA_BETA, "Malama beta cannot be negative");
    if (P.model == 3)
        for (int i = 0; i < P.MoenchM; i++)
            if (P.MoenchAlpha[i] < 0.0) return fail(UCF_ERR_MOENCH, "Moench alphas cannot be negative");
    if (P.M < 2) return fail(UCF_ERR_DEHOOG, "de Hoog M must be >= 2 (M=%d)", P.M);
    if (P.M > UCF_MAX_LAP_M) return fail(UCF_ERR_UNSUPPORTED, "de Hoog M=%d: the wave-cooperative inversion holds at most four Laplace samples per lane (M <= %d)", P.M, UCF_MAX_LAP_M);
    if (P.k - P.R < 2) return fail(UCF_ERR_TANH_SINH, "tanh-sinh k (%d) too low for %d Richardson levels", P.k, P.R);
    if (P.R < 1) return fail(UCF_ERR_TANH_SINH, "Richardson extrapolation level must be >= 1");
    if (P.R > UCF_MAX_R || P.k > 20) return fail(UCF_ERR_UNSUPPORTED, "tanh-sinh k=%d R=%d beyond build limits", P.k, P.R);
    if (P.j0s[0] < 1 || P.j0s[1] < 1 || P.nacc < 1 || P.k < 1)
        return fail(UCF_ERR_GAUSS_LOBATTO, "min/max split, # accelerated terms and k must be >= 1");
    if (P.ord < 3) return fail(UCF_ERR_GAUSS_LOBATTO, "Gauss-Lobatto order must be >= 3");
    if (P.model == 2 && (P.rwobs <= 0.0 || P.sF <= 0.0))
        return fail(UCF_ERR_OBSERVATION, "model 2 needs a positive observation-well radius and shape factor");   // driver_io.f90:374-383
    if (P.timeType == 0 || P.timeType > 8 || P.timeType < -(100 + UCF_MAX_SCHEDULE))
        return fail(UCF_ERR_UNSUPPORTED, "time behaviour %d does not exist (1..8, -1..-100 piecewise constant, -101..-%d piecewise linear)", P.timeType, 100 + UCF_MAX_SCHEDULE);
    if (P.timeType <= -101) {                          // time.f90:109-112
        const int n = -P.timeType - 100;
        for (int k = 0; k < n; k++) {
            const double denom = P.timeParExt[k + 1] - P.timeParExt[k];      // [t_2..t_n, t_f] - t_1..t_n
            if (std::fabs(denom) < (double)FLT_EPSILON)
                return fail(UCF_ERR_BAD_ARGUMENT, "no vertical sloped lines in piecewise linear pumping rate (knots %d and %d coincide)", k + 1, k + 2);
        }
    }
    return UCF_OK;
}

// ---- driver_io.f90:159-186, 531-567
void nondimensionalise(const ucf_params& P, ucf_derived& D)
{
    const double PI = 4.0 * std::atan(1.0);
    std::memset(&D, 0, sizeof(D));
    double l = P.l, d = P.d, ac = P.ac;
    if (P.MNtype == 1) {
        if (std::fabs(P.ac - P.ak) > FLT_EPSILON) ac = P.ak;
        if (std::fabs(l - P.b) > FLT_EPSILON) l = P.b;
        if (d > FLT_EPSILON) d = 0.0;
    }
    D.l_eff = l; D.d_eff = d; D.ac_eff = ac;
    D.Lc = P.b;
    D.Tc = D.Lc * D.Lc / (P.Kr / P.Ss);
    D.Hc = P.Q / (4 * PI * P.Kr * P.b);
    D.sigma = P.Sy / (P.Ss * P.b);
    D.alphaD = P.kappa / D.sigma;
    D.betaD = P.beta / D.Lc;
    D.lD = l / D.Lc;
    D.dD = d / D.Lc;
    D.bD = D.lD - D.dD;
    D.rDw = P.rw / D.Lc;
    D.rDwobs = P.rwobs / D.Lc;
    for (int m = 0; m < P.MoenchM && m < UCF_MAX_MOENCH; m++)
        D.MoenchGamma[m] = P.MoenchAlpha[m] * D.Lc * P.Sy / (P.kappa * P.Kr);
    D.acD = ac * D.Lc;
    D.akD = P.ak * D.Lc;
    D.lambdaD = (P.ak - ac) * D.Lc;
    D.psiaD = P.psia / D.Lc;
    D.psikD = P.psik / D.Lc;
    D.usLD = P.usL / D.Lc;
    D.b1 = P.psia - P.psik;
    D.PsiD = D.b1 / D.Lc;
    D.np = 2 * P.M + 1;
    D.N = (1 << P.k) - 1;
    D.nj0z = (P.j0s[0] > P.j0s[1] ? P.j0s[0] : P.j0s[1]) + P.nacc + 1;
    D.nabs = D.N + P.nacc * (P.ord - 2);
}

// depths per launch.  The integrate kernels keep (R+1) KB of accumulators per depth in LDS and share the
// z-independent half of every sample among the depths of a launch: ~12 KB (2 depths at R = 4) balances occupancy
// against that sharing (measured: 21 depths of the C2 settings take 54 / 44 / 49 / 51 / 66 ms at 1 / 2 / 3 / 4 / 7
// depths per launch).  The monolithic point_kernel (faithful finite-difference closure) takes as many as keep its
// footprint <= 40 KB.  At most UCF_MAX_NZ; UCF_Z_CHUNK overrides (diagnostic).
int z_chunk(const ucf_plan* plan)
{
    const int R = plan->P.R, nacc = plan->P.nacc;
    ucf_dev_params one = plan->dev;
    one.nz = 1;
    const bool split = state_item_bytes(plan, one) != 0;
    int n;
    if (split) {
        n = (int)(((size_t)12 * 1024) / ((size_t)(R + 1) * UCF_WAVE * 16));
    } else {
        const size_t scr = (size_t)(2 * nacc > R ? 2 * nacc : R) * 16 * 16;
        n = (int)(((size_t)40 * 1024 - scr) / ((size_t)(R + 1) * UCF_WAVE * 16));
    }
    if (ucf_env_get().z_chunk > 0) n = ucf_env_get().z_chunk;
    if (n < 1) n = 1;
    if (n > UCF_MAX_NZ) n = UCF_MAX_NZ;
    return n;
}

int fill_call_params(const ucf_plan* plan, int nz, const double* zD, const int* zLay, ucf_dev_params& dp, int nz_out, int z_off)
{
    if (nz < 1 || nz > UCF_MAX_NZ) return fail(UCF_ERR_BAD_ARGUMENT, "nz=%d out of range 1..%d", nz, UCF_MAX_NZ);
    if (!zD || !zLay) return fail(UCF_ERR_BAD_ARGUMENT, "zD / zLay must not be NULL");
    dp = plan->dev;
    dp.nz = nz;
    dp.nz_out = nz_out > 0 ? nz_out : nz;
    dp.z_off = z_off;
    for (int i = 0; i < nz; i++) {
        if (zLay[i] < 1 || zLay[i] > 3) return fail(UCF_ERR_BAD_ARGUMENT, "zLay[%d]=%d not in 1..3", i, zLay[i]);
        dp.zD[i] = zD[i];
        dp.zLay[i] = zLay[i];
    }
    dp.any_lay3 = dp.any_lay1 = 0;
    for (int i = 0; i < nz; i++) { dp.any_lay3 |= (zLay[i] == 3); dp.any_lay1 |= (zLay[i] == 1); }
    dp.any_fold = (dp.fold_dD || dp.fold_lD1 || dp.model == 4) ? 1 : 0;      // (model 4 has no screen terms at all: not a NOFOLD plan)
    dp.tab_premul = (plan->mode == 1);      // fast flavour: a J0(a rD) w_m in the table's Gauss-Lobatto entries (abscissa_kernel)
    // the fast evaluators take sin/cos of Im(eta)*c for c in {1, dD, 1-lD, dD1-1, zD, 1-zD, dD1-zD}:
    // the largest |c| bounds the argument (two-stage Cody-Waite reduction is good below 1e6)
    double cmax = 1.0;
    const double cs[] = {dp.dD, dp.lD1, dp.dD1 - 1.0};
    for (double c : cs) cmax = std::fmax(cmax, std::fabs(c));
    for (int i = 0; i < nz; i++) {
        cmax = std::fmax(cmax, std::fabs(zD[i]));
        cmax = std::fmax(cmax, std::fabs(1.0 - zD[i]));
        cmax = std::fmax(cmax, std::fabs(dp.dD1 - zD[i]));
    }
    dp.fast_im_max = 1.0e6 / cmax;
    if (!(dp.fold_dD && dp.fold_lD1)) {
        // products the reference forms (laplace_hankel_solutions.f90:179-180 and the zD = 1 evaluation of :81):
        // sinh(eta dD) cosh(eta zD), sinh(eta lD1) cosh(eta (1-zD)), sinh(eta dD) cosh(eta): exponents eta*(c1 + c2)
        double cprod = 1.0 + std::fabs(dp.dD);
        for (int i = 0; i < nz; i++) {
            if (zLay[i] == 1) continue;                       // below the screen: g(3) cosh(eta zD), no such product
            cprod = std::fmax(cprod, std::fabs(dp.dD) + std::fabs(zD[i]));
            cprod = std::fmax(cprod, std::fabs(dp.lD1) + std::fabs(1.0 - zD[i]));
        }
        dp.fast_eta_max = 700.0 / cprod;
    }
    // FD closure: its largest intermediate is cosh(eta) / h^2 (b(1), a(2): laplace_hankel_solutions.f90:499-509), finite in the
    // reference up to Re(eta) = 709 - ln(1/h^2); the fast form scales its one division (cinv_scaled)
    if (dp.model == 6 && dp.MNtype == 2) {
        const double lim = 700.0 - std::log(std::fmax(dp.fd_invhsq, 1.0));
        if (dp.fast_eta_max > lim) dp.fast_eta_max = lim;
    }
    // Malama's closed form of the Mishra-Neuman solution: u cosh(eta) with |u| up to ~1e4 u0 must stay finite
    if (dp.model == 6 && dp.MNtype == 1 && dp.fast_eta_max > 680.0) dp.fast_eta_max = 680.0;
    // depths outside the aquifer (the reference evaluates them all the same: growing exponentials): the fast
    // evaluators assume 0 <= zD <= 1, so the generic evaluator takes every abscissa of such a call
    for (int i = 0; i < nz; i++)
        if (!(zD[i] >= 0.0 && zD[i] <= 1.0)) dp.fast_eta_max = -1.0;
    // (the closure's denominator is inverted without exponent scaling: 1 + beta eta xi must stay far from overflow)
    if (!(std::fabs(dp.beta) < 1.0e20)) dp.fast_eta_max = -1.0;
    const double eta_cap = ucf_env_get().fast_eta_max;
    if (eta_cap > 0.0 && dp.fast_eta_max > eta_cap) dp.fast_eta_max = eta_cap;      // diagnostic: hand more of the range to the generic evaluator
    return UCF_OK;
}

// ---- driver_io.f90:654-664
void split_vector(const int* j0s, int nt, const double* tD, int* sv)
{
    const int mx = j0s[0] > j0s[1] ? j0s[0] : j0s[1], mn = j0s[0] < j0s[1] ? j0s[0] : j0s[1];
    const int zrange = mx - mn;
    double lmin = INFINITY, lmax = -INFINITY;
    for (int i = 0; i < nt; i++) {
        const double lg = std::log10(tD[i]);
        lmin = std::fmin(lmin, lg);
        lmax = std::fmax(lmax, lg);
    }
    const int minlsp = (int)std::floor(lmin), maxlsp = (int)std::ceil(lmax);
    const int sprange = maxlsp - minlsp + 1;
    for (int i = 0; i < nt; i++) sv[i] = mn + (int)(zrange * ((maxlsp - std::log10(tD[i])) / sprange));
}

}  // namespace ucf_host

extern "C" {

int ucf_plan_create(const ucf_params* Pin, ucf_plan** out)
{
    if (!Pin || !out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *out = nullptr;
    int rc = validate(*Pin);
    if (rc) return rc;
    rc = require_device();
    if (rc) return rc;
    ucf_plan* pl = new (std::nothrow) ucf_plan();
    if (!pl) return fail(UCF_ERR_NOMEM, "host allocation failed");
    rc = plan_set_params(pl, *Pin, true);
    if (rc) { ucf_plan_destroy(pl); return rc; }
    pl->mode = 0;
    *out = pl;
    return UCF_OK;
}

int ucf_sincos_table(double* tab)
{
    if (!tab) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    sincos_table(tab);
    return UCF_OK;
}

int ucf_exp2_table(double* tab)
{
    if (!tab) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    exp2_table(tab);
    return UCF_OK;
}

int ucf_nondimensionalise(const ucf_params* Pin, ucf_derived* out)
{
    if (!Pin || !out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = validate(*Pin);
    if (rc) return rc;
    nondimensionalise(*Pin, *out);
    return UCF_OK;
}

int ucf_device_count(int* n)
{
    if (!n) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *n = 0;
    int rc = require_device();
    if (rc) return rc;
    (void)hipGetDeviceCount(n);
    return UCF_OK;
}

int ucf_plan_create_on(const ucf_params* Pin, int device, ucf_plan** out)
{
    if (out) *out = nullptr;
    int n = 0;
    int rc = ucf_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return fail(UCF_ERR_BAD_ARGUMENT, "device %d does not exist (%d visible)", device, n);
    device_switch sw(device);
    return ucf_plan_create(Pin, out);
}

int ucf_plan_update(ucf_plan* pl, const ucf_params* Pin)
{
    if (!pl || !Pin) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    int rc = validate(*Pin);
    if (rc) return rc;
    return plan_set_params(pl, *Pin, false);
}

void ucf_plan_destroy(ucf_plan* pl)
{
    if (!pl) return;
    {
        device_switch sw(pl->device);      // the device that owns the memory
        if (pl->d_tables) (void)hipFree(pl->d_tables);
        if (pl->own_stream) { (void)hipStreamSynchronize((hipStream_t)pl->own_stream); (void)hipStreamDestroy((hipStream_t)pl->own_stream); }
        for (ucf_workspace* w : pl->ws) ws_destroy(w);
    }
    std::free(pl->h_j0z); std::free(pl->h_ts_x); std::free(pl->h_ts_w); std::free(pl->h_gl_x); std::free(pl->h_gl_w);
    delete pl;
}

int ucf_plan_derived(const ucf_plan* pl, ucf_derived* out)
{
    if (!pl || !out) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    *out = pl->D;
    return UCF_OK;
}

int ucf_plan_j0z(const ucf_plan* pl, int n, double* j0z)
{
    if (!pl || !j0z || n > pl->D.nj0z) return fail(UCF_ERR_BAD_ARGUMENT, "bad j0z request");
    std::memcpy(j0z, pl->h_j0z, sizeof(double) * n);
    return UCF_OK;
}

int ucf_plan_tanh_sinh(const ucf_plan* pl, int level, int n, double* w, double* x_unit)
{
    if (!pl || !w || level < 1 || level > pl->P.R) return fail(UCF_ERR_BAD_ARGUMENT, "bad tanh-sinh level");
    if (n != pl->Nv[level - 1]) return fail(UCF_ERR_BAD_ARGUMENT, "level %d has %d abscissae", level, pl->Nv[level - 1]);
    std::memcpy(w, pl->h_ts_w + (size_t)(level - 1) * pl->D.N, sizeof(double) * n);
    if (x_unit) {
        if (level != pl->P.R) return fail(UCF_ERR_BAD_ARGUMENT, "abscissae exist for the densest level only");
        std::memcpy(x_unit, pl->h_ts_x, sizeof(double) * n);
    }
    return UCF_OK;
}

int ucf_plan_gauss_lobatto(const ucf_plan* pl, int n, double* x, double* w)
{
    if (!pl || !x || !w || n != pl->P.ord - 2) return fail(UCF_ERR_BAD_ARGUMENT, "bad Gauss-Lobatto request");
    std::memcpy(x, pl->h_gl_x, sizeof(double) * n);
    std::memcpy(w, pl->h_gl_w, sizeof(double) * n);
    return UCF_OK;
}

int ucf_plan_set_timing(ucf_plan* pl, int enable)
{
    if (!pl) return fail(UCF_ERR_BAD_ARGUMENT, "NULL plan");
    std::lock_guard<std::mutex> g(pl->mu);
    pl->timing = enable ? 1 : 0;
    pl->last_timed = nullptr;
    return UCF_OK;
}

int ucf_plan_kernel_times(ucf_plan* pl, int cap, double* ms, int* launches, const char** names, int* n)
{
    if (!pl || !ms || !n || cap < 1) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    ucf_workspace* ws;
    {
        std::lock_guard<std::mutex> g(pl->mu);
        ws = pl->last_timed;
    }
    if (!ws || !ws->tm_valid || ws->tm.n < 1)
        return fail(UCF_ERR_BAD_ARGUMENT, "no timed launch: enable timing (ucf_plan_set_timing) and run a grid call in the lane = time layout first");
    std::lock_guard<std::mutex> g(ws->mu);
    const ucf_timers& tm = ws->tm;
    // one row per kernel, in order of first launch: total duration and number of launches (a call that walks the radii
    // in chunks launches every kernel once per chunk)
    int rows = 0;
    for (int i = 0; i < tm.n; i++) {
        HIP_TRY(hipEventSynchronize((hipEvent_t)tm.ev[2 * i + 1]));
        float f = 0.f;
        HIP_TRY(hipEventElapsedTime(&f, (hipEvent_t)tm.ev[2 * i], (hipEvent_t)tm.ev[2 * i + 1]));
        int r = 0;
        while (r < rows && std::strcmp(names_scratch(ws)[r], tm.name[i]) != 0) r++;
        if (r == rows) {
            if (rows == cap) continue;
            names_scratch(ws)[rows] = tm.name[i];
            ms[rows] = 0.0;
            if (launches) launches[rows] = 0;
            rows++;
        }
        ms[r] += (double)f;
        if (launches) launches[r]++;
    }
    for (int r = 0; r < rows; r++) if (names) names[r] = names_scratch(ws)[r];
    *n = rows;
    return UCF_OK;
}

int ucf_plan_kernel_ms(ucf_plan* pl, double* ms, const char** kernel_name)
{
    if (!pl || !ms) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    double t[16];
    int cnt[16];
    const char* nm[16];
    int n = 0;
    const int rc = ucf_plan_kernel_times(pl, 16, t, cnt, nm, &n);
    if (rc) return rc;
    int best = 0;
    for (int i = 1; i < n; i++) if (t[i] > t[best]) best = i;
    *ms = t[best] / (cnt[best] > 0 ? cnt[best] : 1);            // per launch
    if (kernel_name) *kernel_name = nm[best];
    return UCF_OK;
}

long long ucf_plan_alloc_count(const ucf_plan* pl)
{
    if (!pl) return -1;
    std::lock_guard<std::mutex> g(const_cast<ucf_plan*>(pl)->mu);
    return pl->n_alloc;
}

int ucf_plan_set_mode(ucf_plan* pl, int mode)
{
    // bit 0: 0 faithful / 1 fast;  bit 1 (diagnostic): force the lane = Laplace-sample layout for grids
    if (!pl || mode < 0 || mode > 3) return fail(UCF_ERR_BAD_ARGUMENT, "mode must be 0 (faithful) or 1 (fast) [+2: lane=sample layout]");
    pl->mode = mode & 1;
    pl->force_layout0 = (mode >> 1) & 1;
    return UCF_OK;
}

// ---- driver_io.f90:575-586
int ucf_zlay(const ucf_plan* pl, int nz, const double* zD, int* zLay)
{
    if (!pl || !zD || !zLay) return fail(UCF_ERR_BAD_ARGUMENT, "NULL argument");
    for (int i = 0; i < nz; i++) {
        if (zD[i] <= 0.0 || zD[i] < (1.0 - pl->D.lD)) zLay[i] = 1;
        else if ((zD[i] - 1.0) >= 0.0 || zD[i] < (1.0 - pl->D.dD)) zLay[i] = 2;
        else zLay[i] = 3;
    }
    return UCF_OK;
}

int ucf_split_vector(const ucf_plan* pl, int nt, const double* tD, int* sv)
{
    if (!pl || !tD || !sv || nt < 1) return fail(UCF_ERR_BAD_ARGUMENT, "bad split-vector request");
    split_vector(pl->P.j0s, nt, tD, sv);
    return UCF_OK;
}

}  // extern "C"
