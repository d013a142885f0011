#!/usr/bin/env python3
"""Where the (wave, abscissa) pairs of the folded one-depth water-table kernel lie for a grid, from a binary64 CPU evaluation
of eta = sqrt((p + a^2) / kappa): the form the wave is on (cosh/sinh below Re eta = maxexp in every lane, exponential above,
both), whether the wave is on the short sin/cos form there (sincos_small_: every lane's argument below UCF_SC_SMALL at an
abscissa where the kernel may set the bit, and from then on), and the transitions along an item.
No GPU: the oracle's J0 zeros, tanh-sinh and Gauss-Lobatto nodes, split vector and de Hoog p-values.  A wave is 64
consecutive times of one split index, one radius and one Laplace index; whole items (the kernel cuts them into parts).

Everything the model reads lives in a Model: the deck with its overrides (kappa, the boundary, the numerics), what follows
from it (P, D, M, N, nacc, ngl, the J0 zeros, the tanh-sinh and Gauss-Lobatto nodes) and the limits of the fast evaluators
(maxexp, fast_eta_max, fast_im_max).  Every function below is a method of it.  DEFAULT is the model of the C2 deck; the
module-level names (P, N, row, waves, bound_class_v, ...) are DEFAULT's, for the command line and the tests that read S.P, S.N.
Other configurations: Model(kappa=0.03), Model(kappa=4.0, model=4, beta=2.0), ... (tests/folded_configs.py).

usage: tools/folded_loop_phase_shares.py            the grids of tests/test_gpu_folded_loop_phases.py, one line per depth
       tools/folded_loop_phase_shares.py bench      the C2 sweep of bench.py (1024 times x 256 radii, every 8th radius)
       tools/folded_loop_phase_shares.py intervals [bench]
            the Gauss-Lobatto pairs by the class that eta at the two ends of their J0 interval proves for the whole interval
            (zpair_interval_class, ucf_fastpath.h; interval_class() below is its restatement): the grids of
            tests/test_gpu_folded_loop_intervals.py, or the bench sweep
       tools/folded_loop_phase_shares.py units
            the bench sweep's quadrature units (J0 intervals, the tanh-sinh part in 1 / 2 / 4 runs, 12-node runs of unproven
            intervals) by what the bounds alone decide (zpair_unit_bounds; bound_class_v() below) and what the exact
            classifier behind them still proves
       tools/folded_loop_phase_shares.py sh [bench]
            UCF_PH_SH (Re eta zD >= 0.35 in every lane from here on: sinh without its series test): the share of the proven
            cosh/sinh Gauss-Lobatto pairs that run with the bit, and where in a part it is set -- the grids of
            tests/test_gpu_folded_loop_drops.py, or the bench sweep"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from golden_util import load_deck
from oracle_lib import Oracle
from unconfined_amd.abi import params_from_deck
import test_gpu_folded_loop_phases as T

SMALL, FAST_ETA_MAX, FAST_IM_MAX = 0.012, 700.0, 1.0e6
# whole J0 intervals (zpair_interval_class, ucf_fastpath.h): what eta at an interval's two ends proves for all of its nodes
CLASSES = ("cs_tab", "cs_short", "ex_tab", "ex_short", "unproven")
# the same decision from bounds, without eta (zpair_unit_bounds): the class decided, or UNDECIDED
UNDECIDED = -1
# UCF_PH_SH: "Re eta zD >= 0.35 in every lane from here on", so that sinh(eta zD) and sinh(eta) never take their series
# again (prim_from_e).  Set by the units' classifiers, from the lower end of a unit proven on the cosh/sinh form: by the
# bounds (kappa (Re eta)^2 >= Re p + lob^2 against zb[UCF_ZB_SH]) or, where they did not decide the unit, from Re eta at lob.
# A proven cosh/sinh J0 interval of a part that has the bit runs the loop without the series test.
SINH_SERIES = 0.35
O = Oracle()


def first(mask):
    i = np.flatnonzero(mask)
    return i[0] if i.size else mask.size


class Model:
    """the kernel's view of one plan: the deck `deck` with `overrides` (Deck.replace), and the limits of the fast evaluators
    as fill_call_params sets them for a fully penetrating well and a depth in [0, 1]"""
    SMALL, CLASSES, UNDECIDED, SINH_SERIES = SMALL, CLASSES, UNDECIDED, SINH_SERIES

    def __init__(self, deck=T.DECK, fast_eta_max=FAST_ETA_MAX, fast_im_max=FAST_IM_MAX, **overrides):
        self.deck, self.overrides = deck, dict(overrides)
        dk, ts, P = load_deck(deck)
        if overrides:
            dk = dk.replace(**overrides)
            P = params_from_deck(dk)
        self.dk, self.P, self.D = dk, P, O.nondim(P)
        self.kappa = float(P.kappa)
        self.M, self.N, self.nacc, self.ngl = P.M, self.D.N, P.nacc, P.ord - 2
        self.nabs = self.N + self.nacc * self.ngl
        self.maxexp = -np.log(np.finfo(float).eps) / 3.0
        self.fast_eta_max = self.FAST_ETA_MAX = fast_eta_max
        self.fast_im_max = self.FAST_IM_MAX = fast_im_max
        self.j0z = O.j0_zeros(self.D.nj0z)
        _, self.tsx = O.tanh_sinh(P.k, 0.0)
        self.glx, _ = O.gauss_lobatto(P.ord)
        # where the kernel may set a bit: any tanh-sinh node, the last (smallest) Gauss-Lobatto node of a J0 interval
        self.MAY = np.zeros(self.nabs, bool)
        self.MAY[:self.N] = True
        self.MAY[self.N + self.ngl - 1::self.ngl] = True

    def row(self, rD, sv):
        P, N, nacc, ngl, j0z = self.P, self.N, self.nacc, self.ngl, self.j0z
        a = np.empty(N + nacc * ngl)
        a[:N] = O.tanh_sinh(P.k, j0z[sv - 1] / rD)[1]
        for jj in range(nacc):
            lob, hib = j0z[sv + jj - 1] / rD, j0z[sv + jj] / rD
            a[N + jj * ngl:N + (jj + 1) * ngl] = ((hib - lob) * self.glx + (hib + lob)) / 2.0
        return a

    def split_vector(self, tD):
        return O.split_vector(self.P.j0s, tD)

    def waves(self, tD):
        """(split index, the lanes' p [lane][m]) of every wave of a lane = time grid"""
        P = self.P
        sv = self.split_vector(tD)
        for s in np.unique(sv):
            idx = np.flatnonzero(sv == s)
            for w0 in range(0, len(idx), 64):
                pv = np.stack([O.pvalues(2.0 * x, self.M, P.alpha, P.tol) for x in tD[idx[w0:w0 + 64]]])
                yield int(s), pv[..., 0] + 1j * pv[..., 1]

    def shares(self, tD, radii, zD):
        P, M, N, nacc, ngl, maxexp = self.P, self.M, self.N, self.nacc, self.ngl, self.maxexp
        MAY = self.MAY
        sv = self.split_vector(tD)
        cnt = dict(cs_tab=0, cs_short=0, mixed=0, ex_tab=0, ex_short=0, out=0)
        tr = dict(waves=0, to_exp=0, cs_to_short=0, ex_to_short=0, short_at_start=0, could=0)
        nabs = N + nacc * ngl
        for s in np.unique(sv):
            idx = np.flatnonzero(sv == s)
            for w0 in range(0, len(idx), 64):
                t = tD[idx[w0:w0 + 64]]
                pv = np.stack([O.pvalues(2.0 * x, M, P.alpha, P.tol) for x in t])      # [lane][m][re, im]
                p = pv[..., 0] + 1j * pv[..., 1]
                for rD in radii:
                    a = self.row(rD, int(s))
                    for m in range(2 * M + 1):
                        eta = np.sqrt((p[:, m, None] + a[None, :] ** 2) / self.kappa)      # [lane][abscissa]
                        ok = (eta.real <= self.fast_eta_max).all(0) & (np.abs(eta.imag) < self.fast_im_max).all(0) & ((p[:, m].real > 0).all())
                        ok = np.cumprod(ok).astype(bool)                                 # the fast evaluators are left for good
                        small = eta.real < maxexp
                        f0, f2 = ok & small.all(0), ok & (~small).all(0)
                        ys = (np.abs(eta.imag) < SMALL).all(0)
                        yl = (np.abs(eta.imag) * (1.0 - zD) < SMALL).all(0)
                        i_ys = first(MAY & f0 & ys)
                        i_yl = min(i_ys, first(MAY & f2 & yl))
                        pos = np.arange(nabs)
                        cs_short, ex_short = f0 & (pos >= i_ys), f2 & (pos >= i_yl)
                        cnt["out"] += int((~ok).sum())
                        cnt["cs_short"] += int(cs_short.sum()); cnt["cs_tab"] += int((f0 & ~cs_short).sum())
                        cnt["ex_short"] += int(ex_short.sum()); cnt["ex_tab"] += int((f2 & ~ex_short).sum())
                        cnt["mixed"] += int((ok & ~f0 & ~f2).sum())
                        tr["could"] += int((f0 & ys).sum() + (f2 & yl).sum())
                        tr["waves"] += 1
                        tr["to_exp"] += int(f0.any() and f2.any())
                        tr["cs_to_short"] += int(cs_short.any() and (f0 & ~cs_short).any())
                        tr["ex_to_short"] += int(ex_short.any() and (f2 & ~ex_short).any())
                        tr["short_at_start"] += int(cs_short[0] or ex_short[0])
        return cnt, tr

    # ---- whole J0 intervals
    def interval_class(self, p, lob, hib, zD):
        """the kernel's classifier for one wave (p: the lanes' Laplace parameters) and one J0 interval [lob, hib], restated in
        binary64 with its margins; returns one of CLASSES"""
        kappa, maxexp = self.kappa, self.maxexp
        with np.errstate(all="ignore"):
            eta_hi, eta_lo = np.sqrt((p + hib * hib) / kappa), np.sqrt((p + lob * lob) / kappa)
        re_hi, re_lo, im_lo = eta_hi.real, eta_lo.real, np.abs(eta_lo.imag)
        if not np.all((p.real > 0.0) & (re_hi * 1.01 <= self.fast_eta_max) & (im_lo * 2.0 < self.fast_im_max)):
            return "unproven"
        ys = bool(np.all(im_lo < SMALL))
        yl = ys or bool(np.all(im_lo * (1.0 - zD) < SMALL))
        if np.all(re_hi * (1.0 + 2.0 ** -20) < maxexp):
            return "cs_short" if ys else "cs_tab"
        if np.all(re_lo * (1.0 - 2.0 ** -20) > maxexp):
            return "ex_short" if yl else "ex_tab"
        return "unproven"

    def interval_class_v(self, p, lob, hib, zD):
        """interval_class for waves p[lane][m]: the index into CLASSES per m"""
        kappa, maxexp = self.kappa, self.maxexp
        with np.errstate(all="ignore"):
            eta_hi, eta_lo = np.sqrt((p + hib * hib) / kappa), np.sqrt((p + lob * lob) / kappa)
            re_hi, re_lo, im_lo = eta_hi.real, eta_lo.real, np.abs(eta_lo.imag)
            ok = np.all((p.real > 0.0) & (re_hi * 1.01 <= self.fast_eta_max) & (im_lo * 2.0 < self.fast_im_max), axis=0)
            ys = np.all(im_lo < SMALL, axis=0)
            yl = ys | np.all(im_lo * (1.0 - zD) < SMALL, axis=0)
            cs = np.all(re_hi * (1.0 + 2.0 ** -20) < maxexp, axis=0)
            ex = ~cs & np.all(re_lo * (1.0 - 2.0 ** -20) > maxexp, axis=0)
        out = np.full(ok.shape, CLASSES.index("unproven"))
        out[ok & cs & ys] = CLASSES.index("cs_short")
        out[ok & cs & ~ys] = CLASSES.index("cs_tab")
        out[ok & ex & yl] = CLASSES.index("ex_short")
        out[ok & ex & ~yl] = CLASSES.index("ex_tab")
        return out

    def interval_shares(self, tD, radii, zD):
        """Gauss-Lobatto (wave, abscissa) pairs by the class of their J0 interval, and the transitions along an item"""
        M, nacc, ngl, j0z = self.M, self.nacc, self.ngl, self.j0z
        cnt = dict.fromkeys(CLASSES, 0)
        tr = dict(items=0, straddle=0, cs_to_short=0, ex_to_short=0, after_proven=0)
        for s, p in self.waves(tD):
            for rD in radii:
                for m in range(2 * M + 1):
                    seq = [self.interval_class(p[:, m], j0z[s + jj - 1] / rD, j0z[s + jj] / rD, zD) for jj in range(nacc)]
                    for c in seq:
                        cnt[c] += ngl
                    tr["items"] += 1
                    pairs = list(zip(seq, seq[1:]))
                    tr["straddle"] += int(any(a.startswith("cs") and b == "unproven" and c.startswith("ex") for a, b, c in zip(seq, seq[1:], seq[2:])))
                    tr["cs_to_short"] += int(("cs_tab", "cs_short") in pairs)
                    tr["ex_to_short"] += int(("ex_tab", "ex_short") in pairs)
                    tr["after_proven"] += int(seq[-1] == "unproven" and any(c != "unproven" for c in seq))
        return cnt, tr

    # ---- the bounds (zpair_unit_bounds, ucf_fastpath.h; the limits: zpair_bound_limit, ucf_launch_plan.h).  A unit is a J0
    # interval, a run of tanh-sinh nodes or a run of Gauss-Lobatto nodes: [lob, hib] holds every abscissa of it.
    def bound_limits(self, zD, fast_eta_max=None, fast_im_max=None):
        kappa, maxexp = self.kappa, self.maxexp
        fast_eta_max = self.fast_eta_max if fast_eta_max is None else fast_eta_max
        fast_im_max = self.fast_im_max if fast_im_max is None else fast_im_max
        lim, me2, c = 0.99 * fast_eta_max, kappa * (maxexp * maxexp), 1.0 - zD
        ys = 4.0 * kappa * (SMALL * SMALL)
        with np.errstate(divide="ignore"):
            yl = np.float64(ys) / np.float64(c * c)
        return dict(range=kappa * (lim * lim) if lim > 0.0 else 0.0, im=kappa * (fast_im_max * fast_im_max),
                    cs=me2 / (1.0 + 2.0 ** -19), ex=me2 / (1.0 - 2.0 ** -19), ys=ys, yl=float(yl))

    def bound_class_v(self, p, lob, hib, zD, lim=None):
        """the kernel's bound classifier for waves p[lane, ...] (the lanes' Laplace parameters; every trailing index is a wave
        of its own) and one unit [lob, hib], restated in binary64: an int array over the trailing indices, the index into
        CLASSES of the class decided or UNDECIDED.  (A comparison with a NaN is false, as on the device.)"""
        Z = self.bound_limits(zD) if lim is None else lim
        with np.errstate(all="ignore"):
            u = np.abs(p.imag) * 0.5 + p.real
            i2 = p.imag * p.imag
            up_hi, lo_lo, up_lo = hib * hib + u, lob * lob + p.real, lob * lob + u
            in_range = np.all((p.real > 0.0) & (up_hi < Z["range"]) & (i2 < Z["im"] * lo_lo), axis=0)
            ys = np.all(i2 < Z["ys"] * lo_lo, axis=0)
            yl = ys | np.all(i2 < Z["yl"] * lo_lo, axis=0)
            not_ys = np.any(i2 >= Z["ys"] * up_lo, axis=0)
            not_yl = np.any(i2 >= Z["yl"] * up_lo, axis=0)
            cs = np.all(up_hi < Z["cs"], axis=0)
            ex = ~cs & np.all(lo_lo > Z["ex"], axis=0)
        out = np.full(in_range.shape, UNDECIDED)
        out[in_range & cs & ys] = CLASSES.index("cs_short")
        out[in_range & cs & ~ys & not_ys] = CLASSES.index("cs_tab")
        out[in_range & ex & yl] = CLASSES.index("ex_short")
        out[in_range & ex & ~yl & not_yl] = CLASSES.index("ex_tab")
        return out

    def bound_class(self, p, lob, hib, zD):
        """one wave p[lane]: the class name, or None where the bounds do not decide"""
        c = int(self.bound_class_v(np.asarray(p), lob, hib, zD))
        return None if c == UNDECIDED else CLASSES[c]

    def ts_runs(self, runs):
        """[first node, end node) of the tanh-sinh part's runs, as integrate_kernel cuts them"""
        cuts = [k * self.N // runs for k in range(runs + 1)]
        return [(b, e) for b, e in zip(cuts, cuts[1:]) if e > b]

    def unit_shares(self, tD, radii, zD):
        """share of the units that the bounds alone decide, and that bounds + exact classifier prove: J0 intervals, the
        tanh-sinh part in 1 / 2 / 4 runs, the 12-node runs of the intervals that neither proves"""
        N, nacc, ngl, j0z = self.N, self.nacc, self.ngl, self.j0z
        lim = self.bound_limits(zD)
        cnt = {k: [0, 0, 0] for k in ("intervals", "ts1", "ts2", "ts4", "gl12")}      # units, decided by the bounds, proven
        cls_pairs = dict.fromkeys(CLASSES, 0)
        stronger = 0

        def exact_v(p, lob, hib):
            return np.array([CLASSES.index(self.interval_class(p[:, m], lob, hib, zD)) for m in range(p.shape[1])])

        def tally(key, p, lob, hib, w=1):      # w: the unit's nodes (runs differ in length)
            b = self.bound_class_v(p, lob, hib, zD, lim=lim)
            e = exact_v(p, lob, hib)
            final = np.where(b != UNDECIDED, b, e)
            cnt[key][0] += w * b.size
            cnt[key][1] += w * int((b != UNDECIDED).sum())
            cnt[key][2] += w * int((final != CLASSES.index("unproven")).sum())
            return b, e, final

        for s, p in self.waves(tD):
            for rD in radii:
                a = self.row(rD, s)
                for jj in range(nacc):
                    b, e, final = tally("intervals", p, j0z[s + jj - 1] / rD, j0z[s + jj] / rD)
                    stronger += int(((b != UNDECIDED) & (b != e)).sum())
                    for c in final:
                        cls_pairs[CLASSES[c]] += ngl
                    g = a[N + jj * ngl:N + (jj + 1) * ngl]
                    open_ = final == CLASSES.index("unproven")
                    if open_.any():
                        for r0 in range(0, ngl, 12):                     # (the nodes descend: first node = upper end)
                            tally("gl12", p[:, open_], g[min(r0 + 11, ngl - 1)], g[r0], min(12, ngl - r0))
                for runs in (1, 2, 4):
                    for b0, e0 in self.ts_runs(runs):
                        tally(f"ts{runs}", p, 0.0 if b0 == 0 else a[b0], a[e0 - 1], e0 - b0)
        return cnt, cls_pairs, stronger

    # ---- UCF_PH_SH
    def sh_limit(self, zD):
        with np.errstate(divide="ignore"):
            s = np.float64(SINH_SERIES) / np.float64(zD)
            return float(self.kappa * (s * s) / (1.0 - 2.0 ** -19))

    def sh_bound_v(self, p, lob, zD):
        """the bounds' test for waves p[lane, ...]: a bool array over the trailing indices"""
        with np.errstate(all="ignore"):
            return np.all(lob * lob + p.real > self.sh_limit(zD), axis=0)

    def sh_exact_v(self, p, lob, zD):
        """the exact classifier's test"""
        with np.errstate(all="ignore"):
            re_lo = np.sqrt((p + lob * lob) / self.kappa).real
            return np.all(re_lo * (1.0 - 2.0 ** -20) * zD >= SINH_SERIES, axis=0)

    def part_cuts(self, nsplit):
        """the abscissae at which integrate_kernel cuts an item into nsplit parts (part_bound)"""
        N, nacc, ngl = self.N, self.nacc, self.ngl
        nabs = N + nacc * ngl
        cuts = [0]
        for k in range(1, nsplit):
            j = (k * nabs // nsplit - N + ngl // 2) // ngl
            cuts.append(N + min(max(j, 0), nacc) * ngl)
        return cuts + [nabs]

    def sh_walk(self, p, a, s, rD, zD, nsplit=1, ts_runs_n=2):
        """One wave's items (p[lane][m], every m an item) through the units as the kernel classifies them, part by part (the
        bits are cleared at the start of a part).  Returns a list of (kind, first node, end node, class index [m], the unit's
        own classification set the bit [m], the part has the bit when the unit runs [m], part index, lob, hib)."""
        N, nacc, ngl, j0z = self.N, self.nacc, self.ngl, self.j0z
        cuts = self.part_cuts(nsplit)
        units = [("ts", b, e, 0.0 if b == 0 else a[b], a[e - 1]) for b, e in self.ts_runs(ts_runs_n)]
        units += [("interval", N + jj * ngl, N + (jj + 1) * ngl, j0z[s + jj - 1] / rD, j0z[s + jj] / rD) for jj in range(nacc)]
        out = []
        nm = p.shape[1]
        CS = (CLASSES.index("cs_tab"), CLASSES.index("cs_short"))
        for ip, (c0, c1) in enumerate(zip(cuts, cuts[1:])):
            have = np.zeros(nm, bool)
            for kind, b, e, lob, hib in units:
                if not (c0 <= b < c1):
                    continue
                bc = self.bound_class_v(p, lob, hib, zD)
                ec = self.interval_class_v(p, lob, hib, zD)
                cls = np.where(bc != UNDECIDED, bc, ec)
                is_cs = (cls == CS[0]) | (cls == CS[1])
                sets = is_cs & np.where(bc != UNDECIDED, self.sh_bound_v(p, lob, zD), self.sh_exact_v(p, lob, zD))
                have = have | sets
                out.append((kind, b, e, cls, sets, have.copy(), ip, lob, hib))
        return out

    def sh_shares(self, tD, radii, zD, nsplit=1):
        """(wave, abscissa) pairs of proven cosh/sinh J0 intervals with and without the bit; parts by what happens to the bit"""
        ngl = self.ngl
        cnt = dict(cs_sh=0, cs_plain=0, ts_cs=0, other=0)
        ev = dict(parts=0, never=0, from_start=0, inside=0, lanes_split=0, ts_sets=0, first_of_part_after_none=0)
        CS = (CLASSES.index("cs_tab"), CLASSES.index("cs_short"))
        for s, p in self.waves(tD):
            for rD in radii:
                a = self.row(rD, s)
                walk = self.sh_walk(p, a, s, rD, zD, nsplit)
                nparts = walk[-1][6] + 1
                prev_had = None
                for ip in range(nparts):
                    us = [u for u in walk if u[6] == ip]
                    had_end = us[-1][5]
                    iv = [u for u in us if u[0] == "interval"]
                    ev["parts"] += had_end.size
                    ev["never"] += int((~had_end).sum())
                    ev["from_start"] += int(us[0][4].sum())
                    for i, u in enumerate(us):
                        new = u[4] & ~(us[i - 1][5] if i else np.zeros(had_end.size, bool))
                        if i:
                            ev["inside"] += int(new.sum())
                        if u[0] == "ts":
                            ev["ts_sets"] += int(new.sum())
                        # some lanes past the limit at the unit's lower end, others not: the wave waits for the last of them
                        is_cs = (u[3] == CS[0]) | (u[3] == CS[1])
                        with np.errstate(all="ignore"):
                            past = np.sqrt((p + u[7] * u[7]) / self.kappa).real * zD >= SINH_SERIES
                        ev["lanes_split"] += int((is_cs & past.any(0) & ~past.all(0)).sum())
                    if prev_had is not None:
                        ev["first_of_part_after_none"] += int((us[0][4] & ~prev_had).sum())
                    prev_had = had_end
                    for u in iv:
                        is_cs = (u[3] == CS[0]) | (u[3] == CS[1])
                        cnt["cs_sh"] += ngl * int((is_cs & u[5]).sum())
                        cnt["cs_plain"] += ngl * int((is_cs & ~u[5]).sum())
                        cnt["other"] += ngl * int((~is_cs).sum())
                    for u in us:
                        if u[0] == "ts":
                            cnt["ts_cs"] += (u[2] - u[1]) * int(((u[3] == CS[0]) | (u[3] == CS[1])).sum())
        return cnt, ev

    def bench_grid(self):
        D = self.D
        return O.logspace(-1, 8, 1024) / D.Tc, np.logspace(-1, 1, 256)[::8], 145.7 / D.Lc      # (bench.py's radii span rD = 0.1 ... 10)


def line(tag, cnt, tr):
    n = sum(cnt.values())
    pc = {k: 100.0 * v / n for k, v in cnt.items()}
    print(f"{tag:14s} pairs {n:9d}  cosh/sinh table {pc['cs_tab']:5.1f} % short {pc['cs_short']:5.1f} %  both {pc['mixed']:4.1f} %  "
          f"exponential table {pc['ex_tab']:5.1f} % short {pc['ex_short']:5.1f} %  out of the fast range {pc['out']:4.1f} %")
    w = tr["waves"]
    print(f"{'':14s} items {w}: cosh/sinh -> exponential {100.0 * tr['to_exp'] / w:.1f} %, table -> short on cosh/sinh {100.0 * tr['cs_to_short'] / w:.1f} %, "
          f"on exponential {100.0 * tr['ex_to_short'] / w:.1f} %, short from the first abscissa {100.0 * tr['short_at_start'] / w:.1f} %; "
          f"pairs with every argument below {SMALL}: {100.0 * tr['could'] / n:.1f} %")


def interval_line(tag, cnt, tr):
    n = sum(cnt.values())
    pc = {k: 100.0 * v / n for k, v in cnt.items()}
    print(f"{tag:14s} Gauss-Lobatto pairs {n:9d}  cosh/sinh table {pc['cs_tab']:5.1f} % short {pc['cs_short']:5.1f} %  "
          f"exponential table {pc['ex_tab']:5.1f} % short {pc['ex_short']:5.1f} %  unproven {pc['unproven']:5.1f} %  (proven {100.0 - pc['unproven']:.1f} %)")
    w = tr["items"]
    print(f"{'':14s} items {w}: cosh/sinh -> unproven -> exponential {100.0 * tr['straddle'] / w:.1f} %, table -> short at an interval boundary on "
          f"cosh/sinh {100.0 * tr['cs_to_short'] / w:.1f} %, on exponential {100.0 * tr['ex_to_short'] / w:.1f} %, "
          f"unproven last interval after proven ones {100.0 * tr['after_proven'] / w:.1f} %")


# ---- the model of the C2 deck, and its members under the names the module has always had
DEFAULT = Model()
dk, P, D = DEFAULT.dk, DEFAULT.P, DEFAULT.D
M, N, nacc, ngl = DEFAULT.M, DEFAULT.N, DEFAULT.nacc, DEFAULT.ngl
maxexp, j0z, tsx, glx, MAY = DEFAULT.maxexp, DEFAULT.j0z, DEFAULT.tsx, DEFAULT.glx, DEFAULT.MAY
row, waves, shares = DEFAULT.row, DEFAULT.waves, DEFAULT.shares
interval_class, interval_class_v, interval_shares = DEFAULT.interval_class, DEFAULT.interval_class_v, DEFAULT.interval_shares
bound_limits, bound_class_v, bound_class = DEFAULT.bound_limits, DEFAULT.bound_class_v, DEFAULT.bound_class
ts_runs, unit_shares = DEFAULT.ts_runs, DEFAULT.unit_shares
sh_limit, sh_bound_v, sh_exact_v = DEFAULT.sh_limit, DEFAULT.sh_bound_v, DEFAULT.sh_exact_v
part_cuts, sh_walk, sh_shares, bench_grid = DEFAULT.part_cuts, DEFAULT.sh_walk, DEFAULT.sh_shares, DEFAULT.bench_grid


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["intervals"]:
        if args[1:2] == ["bench"]:
            tD, rD, zD = bench_grid()
            interval_line("bench C2", *interval_shares(tD, rD, zD))
        else:
            import test_gpu_folded_loop_intervals as TI
            tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in TI.TD_CLUSTERS])
            for zD in sorted({c[2] for c in TI.CALLS}, reverse=True):
                interval_line(f"zD = {zD}", *interval_shares(tD, np.array(TI.RD), zD))
    elif args[:1] == ["units"]:
        tD, rD, zD = bench_grid()
        cnt, cls_pairs, stronger = unit_shares(tD, rD, zD)
        for k, (n, d, pr) in cnt.items():
            print(f"{k:10s} nodes-weighted units {n:9d}  decided by the bounds alone {100.0 * d / n:5.1f} %  proven with the exact classifier behind them {100.0 * pr / n:5.1f} %")
        n = sum(cls_pairs.values())
        print("Gauss-Lobatto pairs by class, bounds first:", {k: round(100.0 * v / n, 1) for k, v in cls_pairs.items()},
              "; intervals where the bounds decide another class than the exact classifier:", stronger)
    elif args[:1] == ["sh"]:
        def sh_line(tag, cnt, ev):
            cs = cnt["cs_sh"] + cnt["cs_plain"]
            print(f"{tag:22s} proven cosh/sinh Gauss-Lobatto pairs {cs:9d} ({100.0 * cs / max(cs + cnt['other'], 1):5.1f} % of all), "
                  f"with UCF_PH_SH {100.0 * cnt['cs_sh'] / max(cs, 1):5.1f} %; cosh/sinh tanh-sinh pairs {cnt['ts_cs']}")
            print(f"{'':22s} parts {ev['parts']}: never set {ev['never']}, set by the part's first unit {ev['from_start']} "
                  f"(the part before ended without it: {ev['first_of_part_after_none']}), set by a later unit {ev['inside']}, "
                  f"by a tanh-sinh run {ev['ts_sets']}; cosh/sinh units with lanes on both sides of the limit at their lower end {ev['lanes_split']}")
        if args[1:2] == ["bench"]:
            tD, rD, zD = bench_grid()
            sh_line("bench C2", *sh_shares(tD, rD, zD))
        else:
            import test_gpu_folded_loop_drops as TD
            for tag, beta, zD, cut, clusters, radii in TD.CALLS:
                tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in clusters])
                sh_line(tag, *sh_shares(tD, np.array(radii), zD, int(cut.get("UCF_NSPLIT", 1))))
    elif args[:1] == ["bench"]:
        tD, rD, zD = bench_grid()
        line("bench C2", *shares(tD, rD, zD))
    else:
        tD = np.concatenate([np.logspace(c, c + 0.5, 64) for c in T.TD_CLUSTERS])
        for zD in sorted({c[2] for c in T.CALLS}, reverse=True):
            line(f"zD = {zD}", *shares(tD, np.array(T.RD), zD))
