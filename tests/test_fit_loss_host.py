"""The host side of robust losses in a fit (ucf_fit_loss_terms, ucf_fit_robust_scale, the refusals of ucf_fit_set_loss,
ucf_fit_get_loss, ucf_fit_loss_report and ucf_debug_fit_reduce_loss) and the CPU tests of tests/fit_loss_restate.py, the numpy
restatement that tests/test_gpu_fit_loss_edges.py and tests/test_gpu_fit_loss.py hold the device to bit for bit.  No GPU.

The contract is the text of include/ucf.h at ucf_fit_set_loss:

    a = fabs(x)
    HUBER:  a <= c :  b = 1.0;            rho = x * x
            else   :  b = c / a;          rho = c * (2.0 * a - c)
    TUKEY:  c2 = c * c;  u = x / c
            a <  c :  v = 1.0 - u * u;  b = v * v;  rho = (c2 * (1.0 - b * v)) / 3.0
            else   :  b = 0.0;            rho = c2 / 3.0

Bounds on the rounded rho and b against the loss itself (u = 2^-53, first order, the constants rounded up):
  Huber  a <= c: b exact, rho one product: |rho - x^2| <= u x^2.  a > c: b one quotient: u b; rho = c * (2a - c): 2a is exact,
         the difference (no cancellation: 2a - c > a) and the product round once each: 2 u rho.  Held to 2.01 u, relative.
  Tukey  a < c: u_ = x / c carries 1 rounding, u_ * u_ 3 (relative, the value <= 1), v = 1 - u_u_ then 4 u ABSOLUTE (v <= 1),
         b = v * v: 2 v (4 u) + u b <= 9 u absolute.  Relative it is unbounded as a -> c (v -> 0 by cancellation), so the bound
         on b is absolute: 10 u.  b * v: v (9 u) + b (4 u) + u <= 14 u; 1 - b v: 15 u absolute; times c2 (1 rounding in c2, 1 in
         the product) and / 3.0: (15 + 2 + 1) u / 3 = 6 u, in units of c^2.  rho cancels as a -> 0 (1 - b v -> 3 (a / c)^2), so
         its bound is absolute too: |rho - exact| <= 7 u c^2.  a >= c: b exact, rho = c2 / 3.0: 2 u relative."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
from unconfined_amd import abi
from unconfined_amd import fit as ufit
from unconfined_amd import lib as ucflib

U = 2.0 ** -53
SOURCE_NAMES = sorted(fr.SOURCES, key=fr.SOURCES.get)
KIND_NAMES = sorted(fl.KINDS, key=fl.KINDS.get)


def loss_cases_of(npar):
    """(nobs, nsets) of tests/test_gpu_fit_loss_edges.py for this NPAR"""
    out = [(1, 3), (64, 3), (257, 3)]
    if npar in (0, 1, 4, 8):
        out += [(n, 2) for n in (63, 65, 256, 513)]
    return out


def edge_values(c):
    """mixed signs, +-0, +-c exactly, the doubles adjacent to +-c, +-inf, and magnitudes over twelve decades"""
    rng = np.random.default_rng(20)
    near = [c, -c, np.nextafter(c, 0.0), np.nextafter(c, np.inf), -np.nextafter(c, 0.0), -np.nextafter(c, np.inf)]
    decades = c * 10.0 ** np.linspace(-6.0, 6.0, 49) * np.where(np.arange(49) % 2 == 0, 1.0, -1.0)
    return np.concatenate([[0.0, -0.0, np.inf, -np.inf], near, decades, c * rng.uniform(-3.0, 3.0, 200)])


@pytest.mark.parametrize("c", [2.0, 1.345, 4.685 * 0.37, 3.0e-5, 7.0e11])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_loss_terms_are_the_restatement_bit_for_bit(kind, c):
    x = edge_values(c)
    rho, b = ufit.loss_terms(kind, c, x)
    want_rho, want_b = fl.loss_terms(fl.KINDS[kind], c, x)
    assert rho.tobytes() == want_rho.tobytes() and b.tobytes() == want_b.tobytes(), (kind, c)
    # least squares through the same entry: rho = x * x, b = 1.0, c not read
    rho, b = ufit.loss_terms("l2", -1.0, x)
    assert rho.tobytes() == (x * x).tobytes() and (b == 1.0).all()


@pytest.mark.parametrize("c", [2.0, 1.345, 4.685 * 0.37])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_rho_and_b_against_exact_rational_arithmetic(kind, c):
    """the bounds of the module's docstring, on the finite edge values and 200 random ones"""
    x = edge_values(c)
    x = x[np.isfinite(x)]
    rho, b = fl.loss_terms(fl.KINDS[kind], c, x)
    c2 = Fraction(c) ** 2
    worst = [0.0, 0.0]
    for xi, ri, bi in zip(x, rho, b):
        er, eb = fl.exact_terms(fl.KINDS[kind], c, xi)
        dr, db = abs(Fraction(float(ri)) - er), abs(Fraction(float(bi)) - eb)
        if kind == "huber":
            lim_r, lim_b = Fraction(2.01 * U) * er, Fraction(1.01 * U) * eb
        else:
            lim_r, lim_b = Fraction(7 * U) * c2, Fraction(10 * U)       # absolute: in units of c^2, and of 1
        assert dr <= lim_r and db <= lim_b, (kind, c, xi, float(dr), float(lim_r), float(db), float(lim_b))
        if lim_r:
            worst[0] = max(worst[0], float(dr / lim_r))
        worst[1] = max(worst[1], float(db / lim_b))
    print(f"[fit loss {kind} c={c:g}] worst error / bound: rho {worst[0]:.3f}, b {worst[1]:.3f}")


def test_the_three_stated_consequences():
    c = 2.0
    x = edge_values(c)
    # Tukey is continuous at a == c: the inner branch, evaluated there, gives the rho of the outer one
    for s in (c, -c):
        v = 1.0 - (s / c) * (s / c)
        assert v == 0.0 and ((c * c) * (1.0 - (v * v) * v)) / 3.0 == (c * c) / 3.0
    rho, b = ufit.loss_terms("tukey", c, np.array([c, -c, np.nextafter(c, np.inf)]))
    assert (rho == (c * c) / 3.0).all() and (b == 0.0).all()
    # an infinite x under Huber: b = 0, rho = +inf
    rho, b = ufit.loss_terms("huber", c, np.array([np.inf, -np.inf]))
    assert (b == 0.0).all() and (rho == np.inf).all()
    # Huber with c >= every |x|: the bits of least squares, term by term ...
    fin = x[np.isfinite(x)]
    rho, b = ufit.loss_terms("huber", 1.0e300, fin)
    assert rho.tobytes() == (fin * fin).tobytes() and (b == 1.0).all()
    # ... and sum by sum: phi, g, A, phi_d, nbad of the plain restatement, phi_w the bits of phi, nothing down-weighted
    for source in fr.SOURCES.values():
        for deriv in (False, True):
            for npar, nobs in ((0, 257), (1, 65), (4, 513), (8, 257)):
                inp, _ = fr.synthetic(source, npar, deriv, nobs, 2)
                plain, big = fr.restate(inp), fl.restate(inp, fl.HUBER, 1.0e300)
                n = fr.nsums(npar, deriv)
                assert big["sums"][:, :n].tobytes() == plain["sums"].tobytes(), (source, deriv, npar, nobs)
                assert big["sums"][:, -1].tobytes() == plain["sums"][:, 0].tobytes()
                assert (big["nbad"] == plain["nbad"]).all() and (big["ndown"] == 0).all()
                assert (big["b"][big["counted"]] == 1.0).all() and np.isnan(big["b"][~big["counted"]]).all()


@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_restated_sums_against_longdouble(kind, source, deriv):
    """every restated sum of every case of the GPU module against np.longdouble, formed from the residuals x, the factors b and
    the Jacobian that fp64 holds (b is held to the loss itself above).  A sum of n terms with at most 3 roundings inside a term
    lies within (n + 4) u sum|terms|, n = nobs without and 2 nobs with derivative data.  phi and phi_d are sums of rho, formed
    here from x in np.longdouble: Huber's rho carries 2 roundings (inside the bound), Tukey's an ABSOLUTE 7 u c^2 per term
    (module docstring), which is added for those two sums."""
    k, c = fl.KINDS[kind], fl.C_GPU
    worst = 0.0
    for npar in range(9):
        for nobs, nsets in loss_cases_of(npar):
            inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, nsets)
            res = fl.restate(inp, k, c)
            NS = fl.nsums(npar, deriv)
            for s in range(nsets):
                assert np.isfinite(res["sums"][s]).all()
                ref, mag = fl.longdouble_sums(inp, res, k, c, s)
                lim = ((2 if deriv else 1) * nobs + 4) * U * mag
                if kind == "tukey":
                    lim[0] += 7 * U * c * c * (res["counted"][s].sum() + res["weighted"][s].sum())
                    if deriv:
                        lim[NS - 2] += 7 * U * c * c * res["weighted"][s].sum()
                err = np.abs(res["sums"][s].astype(np.longdouble) - ref)
                assert (err <= lim).all(), (kind, source, deriv, npar, nobs, s, err, lim)
                if (lim > 0).any():
                    worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print(f"[fit loss restate {kind} {source} deriv={deriv}] worst |sum - longdouble| / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_the_gpu_inputs_lie_on_both_sides_of_c(kind):
    """a condition on the inputs of the GPU module: with c = C_GPU at least 10 % of the counted residual terms (drawdown and
    derivative) of every case lie on each side of c, so that both branches of the loss carry weight in every sum.  A case of
    nobs = 1 has one or two terms per set and cannot meet a share: those cases are held to it pooled per source, which is what
    their purpose (one lane of one wave) needs."""
    c = fl.C_GPU
    low = 1.0
    for source in SOURCE_NAMES:
        pooled = []
        for deriv in (False, True):
            for npar in range(9):
                for nobs, nsets in loss_cases_of(npar):
                    inp, _ = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, nsets)
                    res = fl.restate(inp, fl.KINDS[kind], c)
                    for s in range(nsets):
                        a = np.abs(np.concatenate([res["x"][s][res["counted"][s]], res["xd"][s][res["weighted"][s]]]))
                        if nobs == 1:
                            pooled.append(a)
                            continue
                        inside = float((a < c).mean())
                        low = min(low, inside, 1.0 - inside)
                        assert 0.1 <= inside <= 0.9, (source, deriv, npar, nobs, s, inside)
        a = np.concatenate(pooled)
        assert 0.1 <= float((a < c).mean()) <= 0.9, (source, float((a < c).mean()), len(a))
    print(f"[fit loss inputs {kind}] smallest share on one side of c = {c}: {low:.3f}")


def test_robust_scale_is_the_textbook_median():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 4, 7, 64, 1001):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)
        assert ufit.robust_scale(x) == 1.4826 * np.median(np.abs(x)), n
        y = np.concatenate([x, [np.nan, np.inf, -np.inf]])
        assert ufit.robust_scale(rng.permutation(y)) == 1.4826 * np.median(np.abs(x)), n      # the entries that are not finite are left out
    assert ufit.robust_scale([3.0, -1.0]) == 1.4826 * ((1.0 + 3.0) / 2.0)
    assert ufit.robust_scale([0.0, -0.0, 0.0]) == 0.0


# ---- refusals, none of which needs a device

def status_of(call):
    with pytest.raises(ucflib.UcfError) as err:
        call()
    return err.value.status, err.value.message


def bad(call, word):
    status, message = status_of(call)
    assert status == abi.UCF_ERR_BAD_ARGUMENT and word in message, (status, message)


def test_host_entries_refuse_bad_arguments():
    so = ucflib.load()
    x = np.array([1.0, -2.0])
    for c in (0.0, -1.0, np.nan, np.inf):
        for kind in ("huber", "tukey"):
            bad(lambda: ufit.loss_terms(kind, c, x), "c=")
    bad(lambda: ufit.loss_terms(3, 1.0, x), "kind=3")
    bad(lambda: ufit.loss_terms(-1, 1.0, x), "kind=-1")
    out = np.zeros(2)
    assert so.ucf_fit_loss_terms(1, 1.0, -1, x.ctypes.data, out.ctypes.data, out.ctypes.data) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_loss_terms(1, 1.0, 2, None, out.ctypes.data, out.ctypes.data) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_loss_terms(1, 1.0, 2, x.ctypes.data, None, out.ctypes.data) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_loss_terms(1, 1.0, 2, x.ctypes.data, out.ctypes.data, None) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_loss_terms(2, 1.0, 0, x.ctypes.data, out.ctypes.data, out.ctypes.data) == 0          # an empty array is legal
    bad(lambda: ufit.robust_scale([]), "n=0")
    bad(lambda: ufit.robust_scale([np.nan, np.inf]), "finite")
    s = C.c_double()
    assert so.ucf_fit_robust_scale(2, None, C.addressof(s)) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_robust_scale(2, x.ctypes.data, None) == abi.UCF_ERR_BAD_ARGUMENT
    # ucf_fit_set_loss: kind and c are checked before the fit is looked at
    for kind, c, word in ((3, 1.0, "kind=3"), (-1, 1.0, "kind=-1"), (1, 0.0, "c="), (2, np.nan, "c="), (1, np.inf, "c="), (2, -2.0, "c="),
                          (1, 1.0, "NULL"), (0, np.nan, "NULL")):
        assert so.ucf_fit_set_loss(None, kind, c) == abi.UCF_ERR_BAD_ARGUMENT, (kind, c)
        assert word in so.ucf_last_error().decode(), (kind, c, so.ucf_last_error())
    k, c = C.c_int(), C.c_double()
    assert so.ucf_fit_get_loss(None, C.byref(k), C.byref(c)) == abi.UCF_ERR_BAD_ARGUMENT
    assert so.ucf_fit_loss_report(None, 1, x.ctypes.data, None, None, None, None, None, None) == abi.UCF_ERR_BAD_ARGUMENT


def accepted(inp, kind, c):
    """passes every check: without a GPU the answer is UCF_ERR_NO_DEVICE, with one the call succeeds"""
    import torch
    if torch.cuda.is_available():
        assert (fl.debug_fit_reduce_loss(inp, kind, c)["nbad"] >= 0).all()
        return
    status, message = status_of(lambda: fl.debug_fit_reduce_loss(inp, kind, c))
    assert status == abi.UCF_ERR_NO_DEVICE, message


def test_the_debug_entry_refuses_before_it_needs_a_device():
    slots, _ = fr.synthetic(fr.SLOTS, 2, True, 65, 2)
    net, _ = fr.synthetic(fr.NETWORK, 2, True, 65, 2)
    field, _ = fr.synthetic(fr.FIELD, 2, True, 65, 2)
    edit = lambda inp, **kw: {**inp, **{k: (v(inp[k].copy()) if callable(v) else v) for k, v in kw.items()}}
    no = lambda inp, word, kind=fl.TUKEY, c=2.0: bad(lambda: fl.debug_fit_reduce_loss(inp, kind, c), word)

    def at(i, v):
        def put(a):
            a[i] = v
            return a
        return put
    # kind and c
    no(slots, "kind=0", kind=abi.LOSS_L2)
    no(slots, "kind=3", kind=3)
    for c in (0.0, -2.0, np.nan, np.inf, -np.inf):
        no(slots, "c=", kind=fl.HUBER, c=c)
        no(net, "c=", kind=fl.TUKEY, c=c)
    no({**edit(slots, dh=None, dobs=None, wd=None), "force_bd": True}, "bd")
    # the checks of ucf_debug_fit_reduce, inherited
    no(edit(slots, slot=at(7, slots["plan_stride"])), "slot[7]")
    no(edit(slots, slot=at(64, -1)), "slot[64]")
    no(edit(slots, nh=len(slots["h"]) - 1), "plan_stride")
    no(edit(slots, plan_stride=0), "plan_stride")
    no(edit(net, count=at(3, 0)), "ref 3")
    no(edit(net, count=at(3, 33)), "ref 3")
    no(edit(net, stride=at(5, -1)), "ref 5")
    no(edit(net, prefix=at(5, 2 ** 62)), "ref 5")
    no(edit(net, nref=64), "nref")
    no(edit(net, nh=1), "beyond h")
    no(edit(field, prefix=at(11, len(field["h"]))), "term 11")
    no(edit(field, first=at(9, field["first"][8] - 1)), "not ascending")
    no(edit(field, first=at(65, field["first"][65] - 1)), "number of terms")
    no(edit(field, first=at(0, -1)), "first[0]")
    no(edit(field, tfac=None), "tfac")
    no(edit(slots, npar=9), "npar=9")
    no(edit(slots, npar=-1), "npar=-1")
    no(edit(slots, nobs=0), "nobs=0")
    no(edit(slots, nsets=0), "nsets=0")
    no(edit(slots, source=3), "source=3")
    no(edit(slots, dobs=None), "dobs")
    no(edit(slots, Hc=None), "NULL")
    # the same inputs unedited pass every check, under both kinds and without derivative data too
    for inp in (slots, net, field, edit(slots, dh=None, dobs=None, wd=None)):
        for kind in fl.KINDS.values():
            accepted(inp, kind, 2.0)
