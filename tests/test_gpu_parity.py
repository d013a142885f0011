"""Parity of the HIP path (through the C ABI) against the oracle and the golden fixtures.

Bars (the reference is fp64; see DESIGN.md "Parity"):
  * integer/table work (non-dimensionalisation, J0 zeros, split vector, layers, quadrature
    tables) and the stages built only from IEEE +,-,*,/ (Wynn-epsilon, Neville): BIT-EXACT;
  * stages that call elementary functions (sample evaluators, de Hoog): within a few ulp
    of the oracle -- tolerance written at each test;
  * end to end: Wynn-epsilon + de Hoog amplify last-bit differences of the samples by
    1e5..1e7, so the reference is not reproducible with itself below ~1e-10 (its -O2 and
    -O3 -march=native builds differ by up to 1.7e-10 in h and 4e-8 in dh on C2, far more on
    ill-conditioned decks).  Two gates, both relative with the SURVEY floor
    max(|ref|, 1e-3):
      (1) against the binary128 evaluation of the same algorithm (tests/golden/truth_*.npz,
          oracle/gen_truth.py): the device's error must be statistically the reference's own:
              max err_gpu <= max(1e-10, 10 x max err_ref),  median err_gpu <= max(2e-12, 20 x median err_ref)
              (50 x for the finite-difference Mishra-Neuman model, whose Thomas recursion amplifies);
      (2) against every row of the reference binary's .out:
              |gpu - ref| <= max(1e-10, 20 x noise, 64 u c(row)), noise = the larger of the reference's
              build-to-build spread (running max over +-8 times) and its error against (1); c(row) = the
              conditioning of the last stage at that time: the first-order amplification, by de Hoog's inversion,
              of a perturbation of the 2M+1 Laplace-space values by epsilon x the largest of them
              (tests/golden/conditioning.npz, oracle/gen_conditioning.py) -- a device whose Laplace-space values are
              good to 64 u cannot be asked for more than 64 u c(row).  EVERY row, no exception clause;
          for the headline C2 configuration additionally >= 95 % of all points within 1e-10 in h.
    Both gates run through the point-list entry (lane = point / lane = Laplace sample) for every deck and, for the four
    BASELINE decks, through the GRID entry as well (lane = time: the layout bench.py measures).
"""
import os

import numpy as np
import pytest

from golden_util import (COND_K, GOLD, bits_equal, conditioning, crel, deck_names, load_deck, load_e2e, load_stages, rel_err, ulps)

pytestmark = pytest.mark.gpu

NAMES = deck_names()
MODES = ["faithful", "fast"]
# how much of every gate's slack is used: worst err / bound per deck x flavour, written to
# gpurun_out/parity_r03.json when the session ends (tests/conftest.py) and kept under profiles/
PARITY = {}


def _record(gate, name, mode, label, ratio, **extra):
    ent = PARITY.setdefault(gate, {}).setdefault(name, {}).setdefault(mode, {})
    ent[label] = max(ent.get(label, 0.0), float(ratio))
    for k, v in extra.items():
        ent[f"{label}_{k}"] = max(ent.get(f"{label}_{k}", 0.0), float(v))


@pytest.fixture(scope="module")
def engine():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("GPU tests need a GPU (run with -m gpu on the MI355X box)")
    from unconfined_amd import engine as e
    return e


@pytest.mark.parametrize("name", NAMES)
def test_plan_tables_bit_exact(engine, oracle, name):
    """a18, a11, a12: everything the plan builds once equals the oracle's (hence the reference's) bits"""
    dk, ts, P = load_deck(name)
    meta, z = load_stages(name)
    plan = engine.Plan(P)
    D, Do = plan.derived, oracle.nondim(P)
    for f, _ in type(D)._fields_:
        if f == "MoenchGamma":
            assert list(D.MoenchGamma) == list(Do.MoenchGamma)
        else:
            assert getattr(D, f) == getattr(Do, f), f
    assert bits_equal(plan.j0z(), z["par_j0z"])
    assert np.array_equal(plan.split_vector(z["par_tD"]), z["par_sv"])
    assert np.array_equal(plan.zlay(z["par_zD"]), z["par_zLay"])
    assert bits_equal(engine.logspace(ts.min_log, ts.max_log, ts.n), z["par_t"])
    arg = float(z["ts_arg"][0])
    for j in range(1, dk.R + 1):
        w, x = plan.tanh_sinh(j)
        assert bits_equal(w, z[f"ts_w{j}"])
        if x is not None:
            assert bits_equal(x * arg / 2.0, z[f"ts_a{j}"])        # integration.f90:62
    gx, gw = plan.gauss_lobatto()
    assert bits_equal(gx, z["gl_x"]) and bits_equal(gw, z["gl_w"])
    for tee, pref in zip(z["pv_tee"], z["pv_p"]):
        assert bits_equal(plan.pvalues(tee), pref)


def test_wynn_epsilon_bit_exact(engine):
    """a14 incl. truncation at the first non-finite term, the -999999.9 sentinel and the
    absolute-epsilon early exit"""
    z = np.load(os.path.join(GOLD, "stages_generic.npz"))
    nw = int(z["counts"][0])
    by_n = {}
    for i in range(nw):
        by_n.setdefault(len(z[f"wynn_in_{i}"]), []).append(i)
    seen = set()
    for n, idx in by_n.items():
        acc, st = engine.wynn_epsilon(np.stack([z[f"wynn_in_{i}"] for i in idx]))
        seen |= set(int(s) for s in st)
        for k, i in enumerate(idx):
            assert bits_equal(acc[k], z[f"wynn_out_{i}"]), ("wynn", i)
    assert seen == {0, 1, 2, 3}


def test_extraptozero_bit_exact(engine):
    """a13"""
    z = np.load(os.path.join(GOLD, "stages_generic.npz"))
    ne = int(z["counts"][1])
    for i in range(ne):
        out = engine.extraptozero(z[f"extrap_x_{i}"], z[f"extrap_y_{i}"][None])
        assert bits_equal(out[0], z[f"extrap_out_{i}"]), ("extrap", i)


def test_bessel_k0_k1(engine):
    """a9: Amos K0/K1 (series and Miller branches) on the device against the reference's cbesk"""
    z = np.load(os.path.join(GOLD, "stages_generic.npz"))
    k, ierr = engine.bessel_k01(z["cbesk_z"])
    ref, ref_err = z["cbesk_k"], z["cbesk_nz_ierr"][:, 1]
    ok = ref_err == 0
    assert np.array_equal(ierr[ok], np.zeros(ok.sum(), np.int32))
    assert np.all(ierr[~ok] != 0)
    zr = ref[..., 0] + 1j * ref[..., 1]
    zg = k[..., 0] + 1j * k[..., 1]
    rel = np.abs(zg - zr)[ok] / np.abs(zr)[ok]
    assert rel.max() < 5e-15, float(rel.max())


def test_dehoog_few_ulp(engine):
    """a15: QD table + continued fraction across lanes; cexp/csqrt/exp are device libm -> 1e-13 relative"""
    z = np.load(os.path.join(GOLD, "stages_generic.npz"))
    nd = int(z["counts"][2])
    for i in range(nd):
        M, alpha, tol, t, tee = z[f"dehoog_par_{i}"]
        out = engine.dehoog(int(M), alpha, tol, t, tee, z[f"dehoog_fp_{i}"])[0]
        ref = float(z[f"dehoog_out_{i}"][0])
        if np.isnan(ref):
            assert np.isnan(out)
        elif ref == 0.0:
            assert out == 0.0
        else:
            assert abs(out - ref) <= 1e-13 * abs(ref), (i, out, ref)


# decks whose sample formula is free of catastrophic cancellation / ill-conditioned recursions
# (excluded: depths above the screen, g1 - g2; the 30/64-node Thomas recursion of the FD model; the
#  piecewise schedules, whose multiplier sum(dQ_k exp(-t_k p)) - sum(dQ) exp(-tf p) cancels at late time)
WELL_CONDITIONED = [n for n in NAMES if n not in ("hantush_lay3", "hantush_screen", "c4_malama_partpen", "malama_fullpen",
                                                  "c5_mishra_fd64", "mishra_fd30", "neuman_sched2", "theis_sched3")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_samples_vs_oracle(engine, oracle, oracle_quad, name, mode):
    """a3-a10: lap_hank_soln on the device against the bit-pinned oracle.  Inf/NaN must appear
    exactly where the CPU produces them.  Where the reference formula is well conditioned the
    device is within 1e-12 of the oracle; everywhere it must be as close to the binary128
    evaluation of the same formula as the binary64 oracle is (factor 32 + 1e-13)."""
    dk, ts, P = load_deck(name)
    meta, z = load_stages(name)
    plan = engine.Plan(P, mode=mode)
    D = oracle.nondim(P)
    zD, zl = z["par_zD"], z["par_zLay"]
    for i, (tD, a, rD) in enumerate(zip(z["soln_tD"], z["soln_a"], z["soln_rD"])):
        p = oracle.pvalues(2 * tD, dk.M, dk.alpha, dk.tol)
        fp = plan.lap_hank_soln([a], rD, p, zD, zl)[0]
        ref = z["soln_fp"][i]
        assert np.array_equal(np.isnan(fp), np.isnan(ref)), (name, i, "NaN pattern")
        assert np.array_equal(np.isinf(fp), np.isinf(ref)), (name, i, "Inf pattern")
        fin = np.isfinite(ref).all(axis=-1)
        if not fin.any():
            continue
        truth = oracle_quad.soln(P, D, a, rD, p, zD, zl)
        zt = truth[..., 0] + 1j * truth[..., 1]
        zr = ref[..., 0] + 1j * ref[..., 1]
        zg = fp[..., 0] + 1j * fp[..., 1]
        ok = fin & np.isfinite(zt)
        # errors against the binary128 evaluation, as 2-norms over the sample vector (all p, all z):
        # where the reference formula cancels catastrophically (g1 - g2 above the screen) single
        # entries are pure rounding noise for the CPU and the GPU alike, only the norm is meaningful
        e_ref = np.linalg.norm((zr - zt)[ok])
        e_gpu = np.linalg.norm((zg - zt)[ok])
        scale = np.linalg.norm(zt[ok])
        assert e_gpu <= 32.0 * e_ref + 1e-13 * scale + 1e-300, (name, i, a, tD, float(e_gpu / max(scale, 1e-300)), float(e_ref / max(scale, 1e-300)))
        if name in WELL_CONDITIONED:
            r = np.abs(zg - zr)[ok] / np.maximum(np.abs(zr)[ok], 1e-300)
            assert r.max() <= 1e-12, (name, i, a, tD, float(r.max()))


def _grid(oracle, name, ir, e2e):
    dk, ts, P = load_deck(name)
    D = oracle.nondim(P)
    t = oracle.logspace(ts.min_log, ts.max_log, ts.n)
    tD = t / D.Tc
    sv = oracle.split_vector(list(dk.j0s), tD)
    zz = oracle.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd)
    zD = zz / D.Lc
    return dk, P, D, t, tD, np.full_like(tD, float(e2e["radii"][ir]) / D.Lc), sv, zD, oracle.zlay(D, zD)


def _truth(name):
    p = os.path.join(GOLD, f"truth_{name}.npz")
    return np.load(p) if os.path.exists(p) else None


BASELINE_DECKS = ["c2_neuman74_fullpen", "c3_moench", "c4_malama_partpen", "c5_mishra_fd64"]


def gate1_bounds(mode, finite_differences, er):
    """(bound on the largest, bound on the median) error of the device against binary128 under gate (1), from the errors `er`
    of the binary64 oracle at the same points"""
    fmed = 50.0 if finite_differences else 20.0      # FD: Thomas recursion amplifies
    # the max over ~100 points of a 1e5..1e7x amplified rounding error is heavy-tailed: the fast flavour
    # (different roundings in exp/sincos/sqrt) gets 20x the reference's own worst point, the faithful one 10x
    fmax = 10.0 if mode == "faithful" else 20.0
    return max(1e-10, fmax * er.max()), max(2e-12, fmed * np.median(er))
ENTRIES = [(n, "list") for n in NAMES] + [(n, "grid") for n in BASELINE_DECKS]


def _layout_of_last_timed_call(plan):
    """lane layout of the transform kernel of the last grid call (second template argument of its name)"""
    import re
    for name, ms, cnt in plan.kernel_times():
        m = re.search(r"integrate(?:_generic)?_kernel<\d+, (\d+)", name) or re.search(r"point_kernel<\d+, (\d+)", name)
        if m:
            return int(m.group(1))
    return -1


def _through_grid(plan, tD, sv, rDs, zD, zl, with_stats=False):
    """all times x all radii of a fixture through the GRID entry in the lane = time layout (LAYOUT 1): the time vector is
    padded to a multiple of 64 (the padding rows are dropped), which is what makes the library pick that layout for the
    100- to 256-row fixtures as it does for the 1024-row sweeps; the layout that ran is read back from the kernel names"""
    nt = len(tD)
    pad = (-nt) % 64
    tDp = np.concatenate([tD, np.full(pad, tD[-1])])
    svp = np.concatenate([sv, np.full(pad, sv[-1], sv.dtype)])
    plan.set_timing(True)
    out = plan.drawdown_grid(tDp, svp, rDs, zD, zl, with_stats=with_stats)
    assert _layout_of_last_timed_call(plan) == 1, "the grid entry did not run the lane = time layout"
    plan.set_timing(False)
    return (out[0][:nt], out[1][:nt]) + tuple(out[2:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,entry", ENTRIES)
def test_end_to_end_vs_binary128_truth(engine, oracle, name, entry, mode):
    """gate (1): the device result is as close to the exact-arithmetic evaluation of the reference
    algorithm as the (bit-pinned) binary64 oracle, i.e. the reference, is"""
    e2e, tr = load_e2e(name), _truth(name)
    assert e2e is not None and tr is not None
    idx = tr["idx"]
    grid_res = None
    if entry == "grid":
        dk, P, D, t, tD, rD, sv, zD, zl = _grid(oracle, name, 0, e2e)
        grid_res = _through_grid(engine.Plan(P, mode=mode), tD, sv, e2e["radii"] / D.Lc, zD, zl)
    for ir in range(len(e2e["radii"])):
        dk, P, D, t, tD, rD, sv, zD, zl = _grid(oracle, name, ir, e2e)
        if entry == "grid":
            h, dh = grid_res[0][idx, ir, :], grid_res[1][idx, ir, :]
        else:
            plan = engine.Plan(P, mode=mode)
            h, dh = plan.drawdown(tD[idx], rD[idx], sv[idx], zD, zl)
        ho, dho = oracle.batch(P, tD[idx], rD[idx], sv[idx], zD, zl)
        floor = 1e-3 / (1.0 if dk.dimless else D.Hc)
        for got, ref, truth, label in ((h, ho, tr[f"h_r{ir}"], "h"), (dh, dho, tr[f"dh_r{ir}"], "dh")):
            eg, er = rel_err(got, truth, floor), rel_err(ref, truth, floor)
            bound_max, bound_med = gate1_bounds(mode, dk.model == 6 and dk.MNtype == 2, er)
            _record("vs_binary128_truth", name + ("" if entry == "list" else "@grid"), mode, label + "_max", eg.max() / bound_max, err=eg.max(), ref_err=er.max())
            _record("vs_binary128_truth", name + ("" if entry == "list" else "@grid"), mode, label + "_median", np.median(eg) / bound_med, err=np.median(eg))
            assert eg.max() <= bound_max, (name, mode, ir, label, float(eg.max()), float(er.max()))
            assert np.median(eg) <= bound_med, (name, mode, ir, label, float(np.median(eg)), float(np.median(er)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,entry", ENTRIES)
def test_end_to_end_vs_reference_outputs(engine, oracle, name, entry, mode):
    """gate (2): the whole loop body (a1) against every row of the reference binary's own .out"""
    from unconfined_amd.host import screen_average_np
    e2e, tr = load_e2e(name), _truth(name)
    assert e2e is not None
    frac_ok = []
    grid_res = None
    if entry == "grid":
        dk, P, D, t, tD, rD, sv, zD, zl = _grid(oracle, name, 0, e2e)
        grid_res = _through_grid(engine.Plan(P, mode=mode), tD, sv, e2e["radii"] / D.Lc, zD, zl)
    for ir in range(len(e2e["radii"])):
        dk, P, D, t, tD, rD, sv, zD, zl = _grid(oracle, name, ir, e2e)
        if entry == "grid":
            h, dh = grid_res[0][:, ir, :], grid_res[1][:, ir, :]
        else:
            plan = engine.Plan(P, mode=mode)
            h, dh, st = plan.drawdown(tD, rD, sv, zD, zl, with_stats=True)
        sc = 1.0 if dk.dimless else D.Hc
        hobs, dobs = screen_average_np(h, dk) * sc, screen_average_np(dh, dk) * sc
        ref, alt = e2e[f"O2_r{ir}"], e2e[f"O3native_r{ir}"]
        floor = 1e-3
        # the reference's own error against the binary128 truth on the truth subsample
        idx = tr["idx"]
        ho, dho = oracle.batch(P, tD[idx], rD[idx], sv[idx], zD, zl)
        fl_raw = 1e-3 / sc
        noise_t = {"h": float(rel_err(ho, tr[f"h_r{ir}"], fl_raw).max()), "dh": float(rel_err(dho, tr[f"dh_r{ir}"], fl_raw).max())}
        cond = dict(zip(("h", "dh"), conditioning(name, ir)))
        for col, got, label in ((1, hobs, "h"), (2, dobs, "dh")):
            err = rel_err(got, ref[:, col], floor)
            spread = rel_err(alt[:, col], ref[:, col], floor)
            k = 8
            sp = np.array([spread[max(0, i - k): i + k + 1].max() for i in range(len(spread))])
            # per row: the reference's own noise around that time, or what the conditioning of the inversion at that time makes
            # of Laplace-space values that are good to COND_K u (of the largest of them) -- whichever is larger.  Every row.
            bound = np.maximum(np.maximum(1e-10, 20.0 * np.maximum(sp, noise_t[label])), COND_K * 2.220446049250313e-16 * cond[label])
            bad = err > bound
            _record("vs_reference_out", name + ("" if entry == "list" else "@grid"), mode, label, (err / bound).max(), err=err.max(),
                    frac_within_1e_10=np.mean(err <= 1e-10), n_over=int(bad.sum()),
                    rows_ruled_by_conditioning=int((COND_K * 2.220446049250313e-16 * cond[label] > np.maximum(1e-10, 20.0 * np.maximum(sp, noise_t[label]))).sum()))
            assert not bad.any(), (name, entry, mode, ir, label, float(err.max()), float((err / bound).max()), int(np.argmax(err / bound)), int(bad.sum()))
            if label == "h":
                frac_ok.append(float(np.mean(err <= 1e-10)))
    if name == "c2_neuman74_fullpen":
        assert min(frac_ok) >= 0.95, frac_ok


@pytest.mark.parametrize("name", ["c2_neuman74_fullpen", "c3_moench", "neuman74_partpen", "hantush_lay1", "mishra_malama"])
def test_end_to_end_vs_oracle_tight(engine, oracle, name):
    """faithful mode against the oracle on a strided subsample: well below the 1e-10 target in h"""
    e2e = load_e2e(name)
    dk, P, D, t, tD, rD, sv, zD, zl = _grid(oracle, name, 0, e2e)
    idx = np.unique(np.linspace(0, len(t) - 1, 32).astype(int))
    plan = engine.Plan(P, mode="faithful")
    h, dh = plan.drawdown(tD[idx], rD[idx], sv[idx], zD, zl)
    ho, dho = oracle.batch(P, tD[idx], rD[idx], sv[idx], zD, zl)
    floor = 1e-3 / (1.0 if dk.dimless else D.Hc)
    assert rel_err(h, ho, floor).max() < 2e-10
    assert rel_err(dh, dho, floor).max() < 5e-7


@pytest.mark.parametrize("which", ["top", "bottom"])
@pytest.mark.parametrize("name", ["hantush_lay2", "neuman74_partpen", "c3_moench", "hstorage_partpen_lay2", "mishra_fd30"])
def test_wells_that_fold_exactly_one_screen_term(engine, oracle, name, which):
    """A well screened from the very top of the aquifer (d = 0, l < b) or down to its very bottom (l = b, d > 0) folds exactly ONE
    of the two screen terms: neither the fully penetrating instantiation of the unfolded kernels nor the NOFOLD one takes it, and
    of the fixtures only hantush_fullpen is such a well.  Every Hantush-based family against the ORACLE, both flavours, a list
    (lane = point) and a grid (lane = time), depths beside and beyond the screen"""
    dk, ts, P0 = load_deck(name)
    from unconfined_amd.abi import params_from_deck
    dk = dk.replace(d=0.0) if which == "top" else dk.replace(l=dk.b)
    P = params_from_deck(dk)
    D = oracle.nondim(P)
    zmid = 0.5 * (dk.d + dk.l)                                   # (depths below the top of the aquifer, like d and l)
    zD = np.array([zmid, 0.03 * dk.b if which == "bottom" else 0.97 * dk.b]) / D.Lc
    zl = oracle.zlay(D, zD)
    keep = np.asarray(zl) != 3          # (above the screen top the reference's own digits are noise, DESIGN.md section 2: the
    zD, zl = zD[keep], np.asarray(zl)[keep]      #  fuzz net arbitrates that regime against binary128, not this test)
    assert len(zD) >= 1
    rng = np.random.default_rng(17)
    n = 320
    tD = 10.0 ** rng.uniform(-1, 4, n); rD = 10.0 ** rng.uniform(-0.5, 0.7, n)
    sv = oracle.split_vector(list(dk.j0s), tD)
    ho, dho = oracle.batch(P, tD, rD, sv, zD, zl)
    floor = 1e-3 * np.nanmax(np.abs(ho))
    # Bounds on the DISTRIBUTION over 320 random points (the reference is not reproducible with itself below ~1e-10 at isolated
    # points; measured with tools/dbg_mixed_fold.py: medians 5e-15 ... 2e-13, 99th percentiles <= 1.3e-9,
    # maxima <= 2e-8 in h, in BOTH flavours): median, 99th percentile, maximum of h / of dh
    worst = {}
    for mode in ("faithful", "fast"):
        plan = engine.Plan(P, mode=mode)
        h, dh = plan.drawdown(tD, rD, sv, zD, zl)
        assert np.array_equal(np.isnan(h), np.isnan(ho)), (mode, "NaN pattern")
        e, ed = rel_err(h, ho, floor).ravel(), rel_err(dh, dho, floor).ravel()
        assert np.median(e) < 1e-12 and np.quantile(e, 0.99) < 5e-9 and e.max() < 1e-7, (mode, "list h", np.median(e), np.quantile(e, 0.99), e.max())
        assert np.median(ed) < 1e-10 and np.quantile(ed, 0.99) < 5e-7 and ed.max() < 5e-5, (mode, "list dh", np.median(ed), np.quantile(ed, 0.99), ed.max())
        worst[mode] = (e.max(), ed.max())
        tg = np.logspace(-1, 4, 64); rg = np.array([0.4, 1.3, 4.0])
        svg = oracle.split_vector(list(dk.j0s), tg)
        hg, dhg = plan.drawdown_grid(tg, svg, rg, zD, zl)
        hog, dhog = oracle.batch(P, np.repeat(tg, len(rg)), np.tile(rg, len(tg)), np.repeat(svg, len(rg)), zD, zl)
        eg, edg = rel_err(hg.reshape(hog.shape), hog, floor).ravel(), rel_err(dhg.reshape(dhog.shape), dhog, floor).ravel()
        assert np.median(eg) < 1e-12 and eg.max() < 1e-7, (mode, "grid h", np.median(eg), eg.max())
        assert np.median(edg) < 1e-10 and edg.max() < 5e-5, (mode, "grid dh", np.median(edg), edg.max())
        plan.close()
    # the fast flavour is no further from the oracle at its worst point than the reference-order one (x 30, the fuzz net's bar)
    assert worst["fast"][0] <= max(30.0 * worst["faithful"][0], 1e-9) and worst["fast"][1] <= max(30.0 * worst["faithful"][1], 1e-7), worst


def test_full_size_properties(engine, oracle):
    """BASELINE.json's full C2 size (1024 x 256 points) through size-independent properties:
    (1) finite everywhere; (2) h is non-decreasing in time at fixed radius and non-increasing in
    radius at fixed time (drawdown of a constant-rate test), up to the inversion's own accuracy;
    (3) linearity of the path in the Laplace domain: the step response equals the pulse
    decomposition  step(t0=0) - step(t0=T) == pulse(0,T)  after the switch-off;
    (4) a strided 1-in-4096 subsample agrees with the oracle."""
    dk, ts, P = load_deck("c2_neuman74_fullpen")
    plan = engine.Plan(P, mode="fast")
    D = plan.derived
    nt, nr = 1024, 256
    tD = engine.logspace(-1, 8, nt) / D.Tc
    rD = 10.0 ** engine.linspace(-1.0, 1.0, nr)
    TT, RR = np.meshgrid(tD, rD, indexing="ij")
    sv = np.ones(nt * nr, np.int32)
    zD = np.array([145.7 / D.Lc]); zl = plan.zlay(zD)
    hg, dhg, st = plan.drawdown_grid(tD, np.ones(nt, np.int32), rD, zD, zl, with_stats=True)
    h, dh = hg.reshape(nt * nr, 1), dhg.reshape(nt * nr, 1)
    H = h.reshape(nt, nr)
    # the grid entry point runs the lane = time layout, the per-point entry point the lane = Laplace-sample
    # layout: same per-lane arithmetic.  Bit-for-bit in the faithful flavour (no contraction); in the fast
    # flavour the compiler contracts the two instantiations differently, i.e. agreement at the noise floor
    sub0 = np.arange(0, nt * nr, 1013)
    hb, dhb = plan.drawdown(TT.ravel()[sub0], RR.ravel()[sub0], sv[sub0], zD, zl)
    assert rel_err(hb, h[sub0], 1e-3 / D.Hc).max() < 1e-9 and rel_err(dhb, dh[sub0], 1e-3 / D.Hc).max() < 1e-7
    pf = engine.Plan(P, mode="faithful")
    sub1 = np.arange(0, nt, 37)
    hgf, dgf = pf.drawdown_grid(tD[sub1], np.ones(len(sub1), np.int32), rD[::16], zD, zl)
    TTf, RRf = np.meshgrid(tD[sub1], rD[::16], indexing="ij")
    hbf, dbf = pf.drawdown(TTf.ravel(), RRf.ravel(), np.ones(TTf.size, np.int32), zD, zl)
    assert np.array_equal(hgf.ravel(), hbf.ravel()) and np.array_equal(dgf.ravel(), dbf.ravel())
    pf2 = engine.Plan(P, mode="faithful", layout="sample")
    hgs, dgs = pf2.drawdown_grid(tD[sub1], np.ones(len(sub1), np.int32), rD[::16], zD, zl)
    assert np.array_equal(hgs, hgf) and np.array_equal(dgs, dgf)
    assert np.isfinite(h).all() and np.isfinite(dh).all()
    assert st["wynn_sentinel"] == 0 and st["nan_scrubbed"] == 0
    # the de Hoog inversion itself is only good to ~1e-6 absolute where h ~ 0 (early time, far away)
    tol = 2e-6 * np.maximum(np.abs(H), 5.0)
    # ... and erratic at the 1e-5 level where the true drawdown is below it: test where h is resolved
    resolved = (H[1:] > 1e-3) & (H[:-1] > 1e-3)
    dt_viol = np.argwhere((np.diff(H, axis=0) < -tol[1:]) & resolved)
    assert len(dt_viol) == 0, ("h must not decrease in time", len(dt_viol), dt_viol[:5].tolist(),
                               [(float(H[i, j]), float(H[i + 1, j])) for i, j in dt_viol[:5]])
    resolved_r = (H[:, 1:] > 1e-3) & (H[:, :-1] > 1e-3)
    assert not np.any((np.diff(H, axis=1) > tol[:, 1:]) & resolved_r), "h must not increase with radius"
    idx = np.arange(0, nt * nr, 4099)
    ho, dho = oracle.batch(P, TT.ravel()[idx], RR.ravel()[idx], sv[idx], zD, zl)
    assert rel_err(h[idx], ho, 1e-3 / D.Hc).max() < 5e-10
    # (dh: the inversion of p F(p) is 100 x worse conditioned than that of F(p), tests/golden/conditioning.npz)
    assert rel_err(dh[idx], dho, 1e-3 / D.Hc).max() < 5e-8
    # linearity / superposition through the time-behaviour multiplier (time.f90:47-52)
    T = 50.0
    from unconfined_amd.abi import params_from_deck
    sub = np.arange(0, nt * nr, 97)
    P2 = params_from_deck(dk.replace(timeType=2, timePar=[0.0, T]))
    P1b = params_from_deck(dk.replace(timeType=1, timePar=[T, 1.0]))
    h_pulse, _ = engine.Plan(P2, mode="fast").drawdown(TT.ravel()[sub], RR.ravel()[sub], sv[sub], zD, zl)
    h_late, _ = engine.Plan(P1b, mode="fast").drawdown(TT.ravel()[sub], RR.ravel()[sub], sv[sub], zD, zl)
    lhs = h[sub] - h_late
    # the Laplace-domain samples are exactly linear in the schedule; Wynn-epsilon and the de Hoog Pade
    # step are not, so the identity holds to the accuracy of the inversion, and only after the switch-off
    late = TT.ravel()[sub] > 4.0 * T
    dev = np.abs(lhs - h_pulse)[late] / np.maximum(np.abs(h[sub][late]), 1e-3 / D.Hc)
    assert dev.max() < 1e-4, float(dev.max())


@pytest.mark.parametrize("name,nt,nr", [("c3_moench", 2048, 512), ("c4_malama_partpen", 4096, 1024), ("c5_mishra_fd64", 1024, 256)])
def test_full_size_properties_other_configs(engine, oracle, oracle_quad, name, nt, nr):
    """BASELINE.json's configs 3-5 at FULL size through the grid entry (lane = time, radii in chunks: what bench.py
    --workload c3|c4|c5 runs), fast flavour, through size-independent properties: (1) finite everywhere, no in-band rule
    fired; (2) drawdown does not decrease in time at fixed radius nor increase with radius at fixed time where it is
    resolved -- EXCEPT at the isolated points where the reference's own algorithm breaks that (its series acceleration
    produces blips in exact arithmetic too, e.g. C3 at tD = 0.335, rD = 0.634: 0.2286 between 0.3056 and 0.3073): there are
    few of them (< 1e-4 of the sweep) and at every one the device reproduces the ORACLE's value; (3) the chunking of the
    radii does not change a bit (a column block computed on its own); (4) a strided subsample against the oracle, h and dh;
    (5) the faithful flavour on a sub-grid agrees with the fast one."""
    dk, ts, P = load_deck(name)
    plan = engine.Plan(P, mode="fast")
    D = plan.derived
    tD = engine.logspace(-1, 8, nt) / D.Tc
    rD = 10.0 ** engine.linspace(-1.0, 1.0, nr)
    sv = plan.split_vector(tD)
    zD = engine.linspace(dk.zBot, dk.zTop, 1 if dk.piezometer else dk.zOrd) / D.Lc
    zl = plan.zlay(zD)
    hg, dhg, st = plan.drawdown_grid(tD, sv, rD, zD, zl, with_stats=True)
    assert np.isfinite(hg).all() and np.isfinite(dhg).all()
    assert st["wynn_sentinel"] == 0 and st["nan_scrubbed"] == 0 and st["wynn_truncated"] == 0
    floor = 1e-3 / D.Hc
    suspects = set()
    for z in range(len(zD)):
        H = hg[:, :, z]
        tol = 2e-6 * np.maximum(np.abs(H), 5.0)
        resolved = (H[1:] > 1e-3) & (H[:-1] > 1e-3)
        for i, j in np.argwhere((np.diff(H, axis=0) < -tol[1:]) & resolved):
            suspects |= {(int(i), int(j)), (int(i) + 1, int(j))}
        resolved_r = (H[:, 1:] > 1e-3) & (H[:, :-1] > 1e-3)
        for i, j in np.argwhere((np.diff(H, axis=1) > tol[:, 1:]) & resolved_r):
            suspects |= {(int(i), int(j)), (int(i), int(j) + 1)}
    assert len(suspects) <= max(4, 1e-4 * nt * nr), ("too many non-monotone points", name, len(suspects))
    if suspects:
        sp = np.array(sorted(suspects))[:160]
        ho, dho = oracle.batch(P, tD[sp[:, 0]], rD[sp[:, 1]], sv[sp[:, 0]], zD, zl)
        hq, dhq = oracle_quad.batch(P, tD[sp[:, 0]], rD[sp[:, 1]], sv[sp[:, 0]], zD, zl, threads=8)
        e_dev = rel_err(hg[sp[:, 0], sp[:, 1]], ho, floor).max(axis=1)
        e_ref = rel_err(ho, hq, floor).max(axis=1)
        # (the blips are where the series acceleration is at its worst conditioned: the reference's own distance from exact
        #  arithmetic there is 1e-9 ... 1e-5)
        assert (e_dev <= np.maximum(1e-8, 30.0 * e_ref)).all(), (name, float((e_dev / np.maximum(1e-8, 30.0 * e_ref)).max()), sp[np.argmax(e_dev)].tolist())
    # a block of radii on its own (another chunking of the same columns): same bits
    c0 = nr // 3
    hb, db = plan.drawdown_grid(tD, sv, rD[c0:c0 + 7], zD, zl)
    assert np.array_equal(hb, hg[:, c0:c0 + 7]) and np.array_equal(db, dhg[:, c0:c0 + 7])
    # oracle on a strided subsample (48 points across the sweep)
    idx = np.arange(0, nt * nr, (nt * nr) // 48 + 1)
    it, ir = idx // nr, idx % nr
    ho, dho = oracle.batch(P, tD[it], rD[ir], sv[it], zD, zl)
    # (against the reference's own distance from exact arithmetic on those points: the sweeps reach far-field corners where
    #  that is 1e-8)
    hq, dhq = oracle_quad.batch(P, tD[it], rD[ir], sv[it], zD, zl, threads=8)
    e_h, r_h = rel_err(hg[it, ir], hq, floor), rel_err(ho, hq, floor)
    e_d, r_d = rel_err(dhg[it, ir], dhq, floor), rel_err(dho, dhq, floor)
    assert e_h.max() <= max(2e-9, 20.0 * r_h.max()), (float(e_h.max()), float(r_h.max()))
    assert e_d.max() <= max(2e-6, 20.0 * r_d.max()), (float(e_d.max()), float(r_d.max()))
    assert np.median(e_h) <= max(1e-11, 20.0 * np.median(r_h)) and np.median(e_d) <= max(1e-9, 20.0 * np.median(r_d))
    # the faithful flavour on a sub-grid of the same sweep (64 times x 6 radii: lane = time as well)
    pf = engine.Plan(P, mode="faithful")
    ts_, rs_ = np.arange(0, nt, nt // 64)[:64], np.arange(0, nr, nr // 6)[:6]
    hf, df = pf.drawdown_grid(tD[ts_], sv[ts_], rD[rs_], zD, zl)
    assert np.median(rel_err(hg[np.ix_(ts_, rs_)], hf, floor)) < 1e-11 and rel_err(hg[np.ix_(ts_, rs_)], hf, floor).max() < 1e-6
    assert np.median(rel_err(dhg[np.ix_(ts_, rs_)], df, floor)) < 1e-9 and rel_err(dhg[np.ix_(ts_, rs_)], df, floor).max() < 1e-4


def test_edge_cases(engine, oracle, oracle_quad):
    """empty batch, a single point, ragged (non multiple of 64) batch, nz > 1, maximum M, the
    overflow regime rD = 0.02 (NaN scrub / Wynn truncation rules) and bad arguments"""
    from unconfined_amd.lib import UcfError
    dk, ts, P = load_deck("neuman74_partpen")
    plan = engine.Plan(P)
    D = plan.derived
    zD = np.array([0.3, 0.7, 0.95]); zl = plan.zlay(zD)
    h, dh = plan.drawdown(np.zeros(0), np.zeros(0), np.zeros(0, np.int32), zD, zl)
    assert h.shape == (0, 3)
    tD = np.array([0.5]); rD = np.array([0.7]); sv = np.array([1], np.int32)
    h1, dh1 = plan.drawdown(tD, rD, sv, zD, zl)
    ho, dho = oracle.batch(P, tD, rD, sv, zD, zl)
    assert rel_err(h1, ho, 1e-6).max() < 1e-9 and h1.shape == (1, 3)
    n = 67
    tD = 10.0 ** np.linspace(-3, 3, n); rD = np.full(n, 0.4); sv = np.ones(n, np.int32)
    h, dh = plan.drawdown(tD, rD, sv, zD, zl)
    ho, dho = oracle.batch(P, tD, rD, sv, zD, zl)
    assert rel_err(h, ho, 1e-6).max() < 1e-7
    # overflow regime: eta > 709 for the outer abscissae -> Inf/NaN samples -> in-band rules
    tD = 10.0 ** np.linspace(-3, 2, 16); rD = np.full(16, 0.02); sv = np.ones(16, np.int32)
    hg, dhg, st = plan.drawdown(tD, rD, sv, zD, zl, with_stats=True)
    ho, dho = oracle.batch(P, tD, rD, sv, zD, zl)
    assert np.array_equal(np.isnan(hg), np.isnan(ho))
    assert st["wynn_truncated"] + st["wynn_sentinel"] + st["nan_scrubbed"] > 0
    # (values in this regime are the product of the in-band rules acting on overflowed samples;
    #  what must agree is where they are NaN and that the rules fired)
    with pytest.raises(UcfError):
        plan.drawdown(np.array([1.0]), np.array([1.0]), np.array([99], np.int32), zD, zl)     # sv beyond the J0 table
    with pytest.raises(UcfError):
        plan.drawdown(np.array([1.0]), np.array([1.0]), np.array([1], np.int32), zD, np.array([1, 2, 7], np.int32))
    # many depths (contour maps): the API walks them in LDS-sized chunks; every depth equals its own single call
    zmany = np.linspace(0.02, 0.98, 23); zlm = plan.zlay(zmany)
    tq = np.array([0.3, 30.0]); rq = np.array([0.2, 0.9, 4.0])
    hm, dhm = plan.drawdown_grid(tq, np.ones(2, np.int32), rq, zmany, zlm)
    assert hm.shape == (2, 3, 23) and np.isfinite(hm).all()
    for iz in (0, 6, 7, 13, 22):
        h1, d1 = plan.drawdown_grid(tq, np.ones(2, np.int32), rq, zmany[iz:iz + 1], zlm[iz:iz + 1])
        assert np.array_equal(h1[..., 0], hm[..., iz]) and np.array_equal(d1[..., 0], dhm[..., iz]), iz
    TTq, RRq = np.meshgrid(tq, rq, indexing="ij")
    hbq, dbq = plan.drawdown(TTq.ravel(), RRq.ravel(), np.ones(6, np.int32), zmany, zlm)
    assert np.array_equal(hbq.reshape(2, 3, 23), hm)
    hoq, doq = oracle.batch(P, TTq.ravel(), RRq.ravel(), np.ones(6, np.int32), zmany, zlm)
    assert rel_err(hbq, hoq, 1e-6).max() < 1e-7
    # a depth outside the aquifer (zD > 1): not physical, but the reference evaluates it; the fast flavour hands
    # such calls to the generic evaluator
    zo = np.array([0.5, 1.2]); zlo = plan.zlay(zo)
    hx, dhx = plan.drawdown(tD[:4], np.full(4, 0.4), sv[:4], zo, zlo)
    hox, dhox = oracle.batch(P, tD[:4], np.full(4, 0.4), sv[:4], zo, zlo)
    assert np.array_equal(np.isnan(hx), np.isnan(hox))
    assert rel_err(hx[:, 0], hox[:, 0], 1e-6).max() < 1e-7      # the depth inside the aquifer; the other one is
    # ill-conditioned beyond comparison (the reference's own values reach 1e15 there)
    # Laplace sample counts around the wave width: 2M+1 = 63 (one per lane), 65 and 127 (two per lane), 129 and 255 (four)
    tDm = np.array([0.05, 1.0, 40.0]); rDm = np.array([0.5, 0.5, 0.5]); svm = np.ones(3, np.int32)
    for M in (31, 32, 63, 64, 127):
        Pm = type(P).from_buffer_copy(P); Pm.M = M
        pm = engine.Plan(Pm)
        h, dh = pm.drawdown(tDm, rDm, svm, zD[:2], zl[:2])
        ho, dho = oracle.batch(Pm, tDm, rDm, svm, zD[:2], zl[:2])
        if M < 63:
            assert rel_err(h, ho, 1e-6).max() < 1e-7, M
        else:
            # >= 127 Laplace samples: the QD table amplifies rounding so much that only the comparison with
            # exact arithmetic is meaningful -- the device must be as close to it as the binary64 oracle is
            ht, dht = oracle_quad.batch(Pm, tDm, rDm, svm, zD[:2], zl[:2], threads=8)
            assert rel_err(h, ht, 1e-6).max() <= max(1e-9, 10.0 * rel_err(ho, ht, 1e-6).max()), (M, rel_err(h, ht, 1e-6).max(), rel_err(ho, ht, 1e-6).max())
        hg, dg = pm.drawdown_grid(tDm, svm, rDm[:1], zD[:2], zl[:2])
        assert np.array_equal(hg[:, 0, :], h), M            # grid (lane = time) and per-point entries: same bits
        # the de Hoog stage hook at this M against the oracle's (binary128 where the binary64 table is void)
        rng = np.random.default_rng(M)
        fp = np.stack([1.0 / (1.0 + np.arange(2 * M + 1)) ** 1.5 * (1 + 0.1 * rng.standard_normal(2 * M + 1)),
                       -0.3 / (1.0 + np.arange(2 * M + 1)) * (1 + 0.1 * rng.standard_normal(2 * M + 1))], axis=1)
        got = engine.dehoog(M, 1e-8, 1e-9, 1.3, 2.6, fp[None])[0]
        r64 = oracle.dehoog(M, 1e-8, 1e-9, 1.3, 2.6, fp); r128 = oracle_quad.dehoog(M, 1e-8, 1e-9, 1.3, 2.6, fp)
        assert abs(got - r128) <= max(1e-12 * abs(r128), 10.0 * abs(r64 - r128)), (M, got, r64, r128)


_PIPE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
out = {}
for name in ("c2_neuman74_fullpen", "neuman74_partpen"):
    dk, ts, P = load_deck(name)
    plan = engine.Plan(P, mode="fast")
    zD = np.array([0.3, 0.91]); zl = plan.zlay(zD)
    tD = 10.0 ** np.linspace(-2, 4, 150); sv = plan.split_vector(tD)
    rD = np.array([0.02, 0.1, 0.7, 3.0, 9.0])          # 0.02: overflow regime -> unfinished items -> point_kernel
    h, dh = plan.drawdown_grid(tD, sv, rD, zD, zl)
    TT, RR = np.meshgrid(tD[::2], rD, indexing="ij")          # 375 points: enough for the lane = point layout
    hb, dhb = plan.drawdown(TT.ravel(), RR.ravel(), np.repeat(sv[::2], len(rD)), zD, zl)
    out[name + "_h"], out[name + "_dh"], out[name + "_hb"], out[name + "_dhb"] = h, dh, hb, dhb
    # a short time vector against many radii: the library expands such a grid into its point list (lane = point)
    ts_, rs_ = tD[::20], 10.0 ** np.linspace(-1, 1, 80)
    hs, dhs = plan.drawdown_grid(ts_, sv[::20], rs_, zD, zl)
    T2, R2 = np.meshgrid(ts_, rs_, indexing="ij")
    hp, dhp = plan.drawdown(T2.ravel(), R2.ravel(), np.repeat(sv[::20], len(rs_)), zD, zl)
    out[name + "_hs"], out[name + "_hp"] = hs, hp.reshape(hs.shape)
    out[name + "_dhs"], out[name + "_dhp"] = dhs, dhp.reshape(dhs.shape)
# a parameter batch: 5 sets x 300 observation points, against the same sets one by one
from unconfined_amd.abi import params_from_deck
dk, ts, P = load_deck("neuman74_partpen")
plans = [engine.Plan(params_from_deck(dk.replace(Kr=dk.Kr * (0.6 + 0.2 * i), kappa=dk.kappa * (0.5 + 0.3 * i))), mode="fast") for i in range(5)]
rng = np.random.default_rng(3)
t = 10.0 ** rng.uniform(-1, 4, 300); r = rng.choice([30.0, 85.1, 400.0], 300); z = np.array([145.7, 60.0])
hm, dhm = engine.drawdown_multi(plans, t, r, z)
out["multi_h"], out["multi_dh"] = hm, dhm
for k, pl in enumerate(plans):
    D = pl.derived
    tDk, rDk, zDk = t / D.Tc, r / D.Lc, z / D.Lc
    h1, dh1 = pl.drawdown(tDk, rDk, pl.split_vector(tDk), zDk, pl.zlay(zDk))
    out[f"single_h{k}"], out[f"single_dh{k}"] = h1 * D.Hc, dh1 * D.Hc
np.savez(sys.argv[2], **out)
"""


# 2M+1 = 65 samples > 64 lanes: (point, 64-sample chunk) work items, launch_points_chunked.  8 points, one depth: two items
# of (R + 1 + nacc) x 1 KiB = 15 KiB of state per point, so a 64 KiB state budget cuts the list into launches of 2 points
_CHUNKED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
dk, ts, P = load_deck("c2_neuman74_fullpen")
Pm = type(P).from_buffer_copy(P); Pm.M = 32
out = {}
for mode in ("fast", "faithful"):
    plan = engine.Plan(Pm, mode=mode)
    zD = np.array([0.91]); tD = 10.0 ** np.linspace(-2, 3, 8); rD = np.array([0.02, 0.1, 0.5, 3.0] * 2)
    out[mode + "_h"], out[mode + "_dh"] = plan.drawdown(tD, rD, plan.split_vector(tD), zD, plan.zlay(zD))
np.savez(sys.argv[2], **out)
"""


def test_pipeline_knobs_do_not_change_results(tmp_path):
    """the fast flavour's kernel pipeline (integrate -> finish -> resume of unfinished items): cutting the work
    into small state-budget chunks and every scratch-part width of finish_kernel give the same bits"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, env in (("default", {}), ("chunks", {"UCF_STATE_BYTES": str(3 << 20)}), ("part16", {"UCF_FINISH_PART": "16"}),
                     ("part32", {"UCF_FINISH_PART": "32"}), ("tables", {"UCF_TABLE_BYTES": str(3 << 20)}),
                     ("lane_sample", {"UCF_BATCH_LAYOUT": "0"})):
        out = str(tmp_path / f"{tag}.npz")
        e = dict(os.environ); e.update(env)
        subprocess.run([sys.executable, "-c", _PIPE_SCRIPT, root, out], check=True, env=e, timeout=600)
        res[tag] = np.load(out)
    ck = {}
    for tag, env in (("default", {}), ("chunks", {"UCF_STATE_BYTES": str(64 << 10)})):
        out = str(tmp_path / f"chunked_{tag}.npz")
        e = dict(os.environ); e.update(env)
        subprocess.run([sys.executable, "-c", _CHUNKED_SCRIPT, root, out], check=True, env=e, timeout=600)
        ck[tag] = np.load(out)
    for k in ck["default"].files:
        assert np.isfinite(ck["default"][k]).any(), k
        assert np.array_equal(ck["default"][k], ck["chunks"][k], equal_nan=True), ("chunked layout", k)
    ref = res["default"]
    for tag in ("chunks", "part16", "part32", "tables"):
        for k in ref.files:
            assert np.array_equal(ref[k], res[tag][k], equal_nan=True), (tag, k)
    # a short-time-vector grid equals the point list it stands for
    for tag in ("default", "chunks", "tables"):
        for name in ("c2_neuman74_fullpen", "neuman74_partpen"):
            assert np.array_equal(res[tag][name + "_hs"], res[tag][name + "_hp"], equal_nan=True), (tag, name)
            assert np.array_equal(res[tag][name + "_dhs"], res[tag][name + "_dhp"], equal_nan=True), (tag, name)
    # the parameter batch equals its plans one by one, whatever the chunking
    for tag in ("default", "chunks", "tables", "lane_sample"):
        for k in range(5):
            assert np.array_equal(res[tag]["multi_h"][k], res[tag][f"single_h{k}"], equal_nan=True), (tag, k)
            assert np.array_equal(res[tag]["multi_dh"][k], res[tag][f"single_dh{k}"], equal_nan=True), (tag, k)
    # lane = point and lane = Laplace sample layouts of a point list: same per-lane arithmetic
    for k in ref.files:
        a, b = ref[k], res["lane_sample"][k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        if k.endswith("_hb") or k.startswith("multi_h") or k.startswith("single_h"):
            fin = np.isfinite(a)
            scale = np.abs(b[fin]).max()
            assert (np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-4 * scale)).max() < 1e-6, k
    # grid (lane = time) and batch (lane = Laplace sample) agree to rounding of the fast flavour's contractions
    for name in ("c2_neuman74_fullpen", "neuman74_partpen"):
        hg = ref[name + "_h"][::2]; hb = ref[name + "_hb"].reshape(hg.shape)
        assert np.array_equal(np.isnan(hg), np.isnan(hb))
        a_, b_ = hg[:, 1:], hb[:, 1:]                                        # (column 0 is the overflow regime)
        assert (np.abs(a_ - b_) / np.maximum(np.abs(b_), 1e-4 * np.abs(b_).max())).max() < 1e-6, name


_LAYOUT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
out = {}
for name in ("c2_neuman74_fullpen", "neuman74_partpen", "hantush_lay3", "hstorage_partpen_lay1", "c1_theis", "mishra_fd30"):
    dk, ts, P = load_deck(name)
    plan = engine.Plan(P, mode="faithful")
    rng = np.random.default_rng(5)
    tD = 10.0 ** rng.uniform(-2, 4, 400); rD = 10.0 ** rng.uniform(-1, 1, 400); sv = plan.split_vector(tD)
    zD = np.array([0.3, 0.95]); zl = plan.zlay(zD)
    h, dh = plan.drawdown(tD, rD, sv, zD, zl)
    out[name + "_h"], out[name + "_dh"] = h, dh
np.savez(sys.argv[2], **out)
"""


def test_general_instantiation_stays_under_the_gates(tmp_path):
    """A plan that folds neither screen term (d > 0, l < b) runs the NOFOLD instantiations of the unfolded kernels since the last
    pass of round 3; the GENERAL instantiation is left with plans that fold exactly one term and with mixed parameter batches.
    It must not drop out of the parity net: the end-to-end gates of the partially penetrating decks (point list and grid
    entry, fast flavour) once more in a child process with UCF_NOFOLD=0, and one deck of each family general against NOFOLD"""
    import subprocess, sys
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, UCF_NOFOLD="0", UCF_PARITY_OUT=str(tmp_path / "parity_general.json"))
    sel = ("(end_to_end_vs_reference_outputs or end_to_end_vs_binary128_truth) and fast and "
           "(neuman74_partpen or c4_malama_partpen or c3_moench or hantush_lay2 or hstorage_partpen_lay2 or mishra_fd30 or c5_mishra_fd64)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-q", "-x", "-m", "gpu",
                        "-p", "no:cacheprovider", "--no-header", "-k", sel], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
    # the two instantiations against each other: same formulas, other contractions -- the fast flavour's rounding noise
    res = {}
    for tag, e in (("nofold", {}), ("general", {"UCF_NOFOLD": "0"})):
        out = str(tmp_path / f"{tag}.npz")
        ee = {k: v for k, v in os.environ.items() if k != "UCF_NOFOLD"}
        ee.update(e)
        subprocess.run([sys.executable, "-c", _NOFOLD_SCRIPT, root, out], check=True, env=ee, timeout=600)
        res[tag] = np.load(out)
    ran = {str(x) for x in res["nofold"]["kernels"]} | {str(x) for x in res["general"]["kernels"]}
    assert any(k.endswith(", true>") for k in ran if "integrate_kernel" in k), ran        # NOFOLD did run ...
    assert all(not k.endswith(", true>") for k in (str(x) for x in res["general"]["kernels"]) if "integrate_kernel" in k)     # ... and not under UCF_NOFOLD=0
    for k in res["nofold"].files:
        if k == "kernels":
            continue
        a, b = res["nofold"][k], res["general"][k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        fin = np.isfinite(a)
        scale = np.abs(b[fin]).max()
        # (h to 1e-6; the log-derivative, whose inversion amplifies the Laplace-space rounding 1e2 x more -- DESIGN.md section 2,
        #  c(row) -- to 1e-4: both instantiations pass the gates against the reference in their own right, above)
        assert (np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-4 * scale)).max() < (1e-4 if k.endswith("_dh") else 1e-6), k


_NOFOLD_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
out = {}; kernels = set()
for name in ("hantush_lay2", "neuman74_partpen", "c4_malama_partpen", "hstorage_partpen_lay2", "mishra_fd30"):
    dk, ts, P = load_deck(name)
    pl = engine.Plan(P, mode="fast")
    pl.set_timing(True)
    for nz, zD in ((1, np.array([0.6])), (2, np.array([0.3, 0.93]))):
        zl = pl.zlay(zD)
        tD = np.logspace(-1, 4, 128); rD = np.array([0.11, 0.7, 3.0, 9.0])
        h, dh = pl.drawdown_grid(tD, pl.split_vector(tD), rD, zD, zl)
        kernels |= {n for n, ms, cnt in pl.kernel_times()}
        out["%s_nz%d_h" % (name, nz)] = h; out["%s_nz%d_dh" % (name, nz)] = dh
    pl.close()
out["kernels"] = np.array(sorted(kernels))
np.savez(sys.argv[2], **out)
"""


def test_point_list_layouts_same_bits_faithful(tmp_path):
    """a list of 400 arbitrary points in the lane = point and in the lane = Laplace-sample layout: the faithful
    flavour gives the same bits (six models, all layers)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, env in (("point", {}), ("sample", {"UCF_BATCH_LAYOUT": "0"})):
        out = str(tmp_path / f"{tag}.npz")
        e = dict(os.environ); e.update(env)
        subprocess.run([sys.executable, "-c", _LAYOUT_SCRIPT, root, out], check=True, env=e, timeout=600)
        res[tag] = np.load(out)
    for k in res["point"].files:
        assert np.isfinite(res["point"][k]).any()
        assert np.array_equal(res["point"][k], res["sample"][k], equal_nan=True), k


def test_plan_update_equals_fresh_plan(engine):
    """ucf_plan_update: an existing plan given new parameters computes what a fresh plan computes, bit for bit
    (water-table model, the finite-difference closure with its parameter-dependent table, a pumping schedule); a
    change of the numerical settings is refused"""
    from unconfined_amd.abi import params_from_deck
    from unconfined_amd.lib import UcfError
    t = 10.0 ** np.linspace(-1, 4, 40); r = np.full(40, 85.1); r[::4] = 20.0
    for name in ("neuman74_partpen", "mishra_fd30", "neuman_sched2"):
        dk, ts, P0 = load_deck(name)
        for mode in MODES:
            plan = engine.Plan(P0, mode=mode)
            for i in range(3):
                d = dk.replace(Kr=dk.Kr * (0.5 + 0.4 * i), Sy=dk.Sy * (0.7 + 0.1 * i), kappa=dk.kappa * (0.6 + 0.3 * i),
                               ak=dk.ak * (1.0 + 0.2 * i), Q=dk.Q * (1 + i))
                Pn = params_from_deck(d)
                plan.update(Pn)
                fresh = engine.Plan(Pn, mode=mode)
                D = fresh.derived
                assert plan.derived.Tc == D.Tc and plan.derived.Hc == D.Hc
                tD, rD = t / D.Tc, r / D.Lc
                zD = np.array([145.7]) / D.Lc
                a = plan.drawdown(tD, rD, plan.split_vector(tD), zD, plan.zlay(zD))
                b = fresh.drawdown(tD, rD, fresh.split_vector(tD), zD, fresh.zlay(zD))
                assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True), (name, mode, i)
    dk, ts, P0 = load_deck("neuman74_partpen")
    plan = engine.Plan(P0)
    with pytest.raises(UcfError):
        plan.update(params_from_deck(dk.replace(M=dk.M + 2)))
    with pytest.raises(UcfError):
        plan.update(params_from_deck(dk.replace(model=4)))


def test_device_entry_orders_by_radius(engine):
    """ucf_drawdown_batch_device on device-resident, unordered points (radii from the overflow regime up): the library
    orders them by radius on the device; same bits as the host entry, which orders them on the host"""
    import torch
    dk, ts, P = load_deck("neuman74_partpen")
    plan = engine.Plan(P, mode="fast")
    rng = np.random.default_rng(9)
    n = 1500
    tD = 10.0 ** rng.uniform(-1, 4, n); rD = 10.0 ** rng.uniform(np.log10(0.03), 1, n); sv = plan.split_vector(tD)
    zD = np.array([0.4, 0.93]); zl = plan.zlay(zD)
    h0, dh0 = plan.drawdown(tD, rD, sv, zD, zl)
    dev = torch.device("cuda:0")
    d_t = torch.tensor(tD, device=dev); d_r = torch.tensor(rD, device=dev); d_s = torch.tensor(sv, dtype=torch.int32, device=dev)
    d_h = torch.zeros(n, 2, dtype=torch.float64, device=dev); d_dh = torch.zeros_like(d_h)
    plan.drawdown_device(n, d_t.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), zD, zl, d_h.data_ptr(), d_dh.data_ptr(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_h.cpu().numpy(), h0, equal_nan=True)
    assert np.array_equal(d_dh.cpu().numpy(), dh0, equal_nan=True)
    assert np.isfinite(h0).mean() > 0.9


def test_parameter_batched_sweep(engine):
    """f4: the same observation points under 12 parameter sets in one call == 12 single-plan calls"""
    from unconfined_amd.abi import params_from_deck
    dk, ts, P0 = load_deck("neuman74_partpen")
    plans = []
    for i in range(12):
        d = dk.replace(Kr=dk.Kr * (0.5 + 0.1 * i), Sy=dk.Sy * (0.8 + 0.03 * i), kappa=dk.kappa * (0.7 + 0.05 * i))
        plans.append(engine.Plan(params_from_deck(d), mode="fast"))
    t = 10.0 ** np.linspace(-1, 4, 37); r = np.full(37, 85.1); r[::3] = 30.0
    z = np.array([145.7, 100.0])
    h, dh = engine.drawdown_multi(plans, t, r, z)
    assert h.shape == (12, 37, 2) and np.isfinite(h).all()
    for k, pl in enumerate(plans):
        D = pl.derived
        tD, rD, zD = t / D.Tc, r / D.Lc, z / D.Lc
        h1, dh1 = pl.drawdown(tD, rD, pl.split_vector(tD), zD, pl.zlay(zD))
        assert np.array_equal(h[k], h1 * D.Hc) and np.array_equal(dh[k], dh1 * D.Hc), k
    assert np.abs(h[0] - h[11]).max() > 1e-3        # the parameter sets do differ
    # geometry varies too (the depths fall into different layers from plan to plan), still one launch sequence;
    # and a batch that cannot share one (different M) goes plan by plan -- same results either way
    geo = [engine.Plan(params_from_deck(dk.replace(l=dk.l * f, d=dk.d * g, Kr=dk.Kr * (1 + 0.1 * i))), mode="fast")
           for i, (f, g) in enumerate([(1.0, 1.0), (0.55, 1.0), (1.0, 4.5), (0.9, 0.2), (2.2, 0.5)])]
    zg = np.array([145.7, 100.0, 20.0])
    lays = {tuple(pl.zlay(zg / pl.derived.Lc)) for pl in geo}
    assert len(lays) > 1, lays
    mixed = [engine.Plan(params_from_deck(dk.replace(M=20 + 3 * i, Kr=dk.Kr * (1 + 0.2 * i))), mode="fast") for i in range(3)]
    for group in (geo, mixed):
        hg, dhg = engine.drawdown_multi(group, t, r, zg)
        for k, pl in enumerate(group):
            D = pl.derived
            tD, rD, zD = t / D.Tc, r / D.Lc, zg / D.Lc
            h1, dh1 = pl.drawdown(tD, rD, pl.split_vector(tD), zD, pl.zlay(zD))
            assert np.array_equal(hg[k], h1 * D.Hc, equal_nan=True) and np.array_equal(dhg[k], dh1 * D.Hc, equal_nan=True), k


def test_random_parameter_sets_fast_vs_faithful():
    """a broad net over the parameter space (models 1, 3, 4, 5, 6-FD; full and partial penetration, all three
    layers, kappa over two decades, radii down to the overflow regime): the two flavours agree to 1e-7 of the
    solution's scale, and where they do not, the reference itself is that far from exact arithmetic (cancellation above
    the screen at large eta, Inf/NaN regime): the fast flavour must then be no further from the binary128
    evaluation than 30x the reference's own distance"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_flavours
    worst, judged = fuzz_flavours.run(nsets=40, seed=11, verbose=False, judge_above=1e-7, max_judged=12)
    assert len(worst) >= 30
    assert all(w[-1] for w in worst), ("NaN patterns differ (beyond the documented overflow-regime limit: kappa < 0.05, <= 3 % of a set)",
                                       [w for w in worst if not w[-1]])
    arb = {j[0]: j for j in judged}
    for w in worst:
        if w[0] > 1e-7:
            assert w[1] in arb, w
            _, e_fast, e_faithful, e_ref = arb[w[1]]
            assert e_fast <= 30.0 * max(e_ref, 1e-10), (w, arb[w[1]])


def test_random_parameter_sets_round3_evaluators():
    """the same net over the families whose fast evaluators are new in round 3: Theis (model 0), Hantush with wellbore
    storage (model 2: partially and fully penetrating, well / casing / observation-well radii and the shape factor moved),
    Mishra-Neuman in Malama's closed form (model 6, MNtype 1: sorptive numbers and the unsaturated thickness moved)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_flavours
    # (above the screen the reference's Hantush factor cancels -- up to O(1) errors against exact arithmetic, as for model 1 --
    #  so that many model-2 sets are judged against the binary128 evaluation: the fast flavour is the accurate one there)
    worst, judged = fuzz_flavours.run(nsets=40, seed=23, verbose=False, judge_above=1e-7, max_judged=40, models=(0, 2, 12, 16))
    assert len(worst) >= 30
    assert {w[2] for w in worst} == {0, 2, 6}
    assert all(w[-1] for w in worst), [w for w in worst if not w[-1]]
    arb = {j[0]: j for j in judged}
    for w in worst:
        if w[0] > 1e-7:
            assert w[1] in arb, w
            _, e_fast, e_faithful, e_ref = arb[w[1]]
            assert e_fast <= 30.0 * max(e_ref, 1e-10), (w, arb[w[1]])


def test_random_shapes_fast_vs_faithful():
    """the index arithmetic of every lane layout rather than the formulas (tools/fuzz_shapes.py): random numerical settings
    (de Hoog M 3 ... 70 -- more Laplace samples than lanes included --, tanh-sinh k / R, 2 ... 16 accelerated zeros, 4 ... 81
    Gauss-Lobatto nodes, J0 split ranges), 1 ... 4 depths in any layers, lists of 1 ... 700 points and grids of 1 ... 200 x
    1 ... 9, every family.  Many of these settings resolve the integrals badly and the accelerations amplify that: where the
    flavours are further apart than 1e-6 the reference itself is that far from the binary128 evaluation, and the fast
    flavour must be no further than 30 x the reference's distance (depths above the screen of the Hantush models are left
    out: known cancellation of the reference, tested elsewhere)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_shapes
    worst, judged = fuzz_shapes.run(nsets=150, seed=5, verbose=False, max_judged=16)
    assert len(worst) >= 90
    arb = {j[0]: j for j in judged}
    for w in worst:
        assert w[5] <= 0.03 * w[6], w               # NaN patterns (overflow regime only)
        if w[0] > 1e-6:
            assert w[1] in arb, w
            _, e_fast, e_faithful, e_ref = arb[w[1]]
            assert e_fast <= 30.0 * max(e_ref, 1e-10), (w, arb[w[1]])


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_analytic_identities(engine):
    """known answers of the reference's own formulation, at points where the inversion resolves them:
    (1) model 0 is the Theis solution: h = E1(rD^2 / 4 tD) (dimensionless head, 4 pi T s / Q convention of the reference), to 1e-3;
    (2) Hantush (model 1) with a fully penetrating well (d = 0, l = b) is Theis at every depth;
    (3) model 4 (Malama, fully penetrating by construction) is model 5 with d = 0, l = b."""
    from scipy.special import exp1
    from unconfined_amd.abi import params_from_deck
    dk, ts, P0 = load_deck("c1_theis")
    tD = np.array([0.5, 2.0, 10.0, 50.0, 300.0]); rD = np.array([0.5, 1.0, 2.0, 1.0, 3.0])
    for mode in MODES:
        pl = engine.Plan(P0, mode=mode)
        zD = np.array([0.5]); zl = pl.zlay(zD)
        h0, _ = pl.drawdown(tD, rD, pl.split_vector(tD), zD, zl)
        want = exp1(rD * rD / (4.0 * tD))
        ratio = h0[:, 0] / want
        # (to the accuracy of the reference's own scheme -- ten J0 intervals accelerated by Wynn-epsilon: ~1e-3)
        assert np.abs(ratio - 1.0).max() < 1e-3, (mode, ratio)
        dh = load_deck("hantush_fullpen")[0]
        dh = dh.replace(d=0.0, l=dh.b)
        ph = engine.Plan(params_from_deck(dh), mode=mode)
        pt = engine.Plan(params_from_deck(dh.replace(model=0)), mode=mode)
        zz = np.array([0.1, 0.5, 0.9]); zlh = ph.zlay(zz)
        hh, _ = ph.drawdown(tD, rD, ph.split_vector(tD), zz, zlh)
        ht, _ = pt.drawdown(tD, rD, pt.split_vector(tD), zz, pt.zlay(zz))
        assert rel_err(hh, ht, 1e-6).max() < 1e-9, (mode, float(rel_err(hh, ht, 1e-6).max()))
        dm = load_deck("malama_fullpen")[0]
        p4 = engine.Plan(params_from_deck(dm.replace(model=4)), mode=mode)
        p5 = engine.Plan(params_from_deck(dm.replace(model=5, d=0.0, l=dm.b)), mode=mode)
        h4, d4 = p4.drawdown(tD, rD, p4.split_vector(tD), zz, p4.zlay(zz))
        h5, d5 = p5.drawdown(tD, rD, p5.split_vector(tD), zz, p5.zlay(zz))
        assert rel_err(h4, h5, 1e-6).max() < 1e-9 and rel_err(d4, d5, 1e-6).max() < 1e-7, (mode, float(rel_err(h4, h5, 1e-6).max()))
