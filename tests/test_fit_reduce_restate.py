"""CPU tests of tests/fit_reduce_restate.py, the numpy restatement that tests/test_gpu_fit_reduce_edges.py holds the fit
reduction kernel to bit for bit, and of the refusals of ucf_debug_fit_reduce, which need no GPU.

  * the restatement computes the right quantity: on the synthetic inputs of the GPU module every restated sum lies within
    (nobs + 4) u sum|terms| of its np.longdouble value, the bound of tests/test_gpu_fit.py::check_sums;
  * the data tell the orders apart: for the inputs with nobs >= 257 the documented order and three changed ones (a plain
    ascending sum, the waves added in reverse, a butterfly m = 1 .. 32) differ in the bits of phi and of at least one entry of A.
    Without this "bit for bit" would say nothing about the order;
  * nbad of the restatement is the number of observations that the pattern of kinds excludes, counted from the pattern alone;
  * a mistake in a test becomes a refusal, not a read out of bounds: UCF_ERR_BAD_ARGUMENT before any allocation or launch."""
import numpy as np
import pytest

import fit_reduce_restate as fr

U = 2.0 ** -53
SOURCE_NAMES = sorted(fr.SOURCES, key=fr.SOURCES.get)


def cases_of(npar):
    """(nobs, nsets) of the GPU module for this NPAR"""
    out = [(1, 3), (64, 3), (257, 3)]
    if npar in (0, 1, 4, 8):
        out += [(n, 2) for n in (63, 65, 255, 256, 300, 513, 1025)]
    return out


@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
def test_restatement_against_longdouble(source, deriv):
    """every restated sum of every case of the GPU module within (nobs + 4) u sum|terms| of its np.longdouble evaluation, twice:
    from the sim rows, as check_sums of tests/test_gpu_fit.py forms it, and from the residual and the Jacobian that fp64 holds,
    with every entry of J within 2 roundings (2.001 u) of its np.longdouble value.

    Why twice: (nobs + 4) u is (nobs - 1) u for the summation and 5 u for the roundings inside a term.  A term w d_j w d_k formed
    from sim carries up to 7 (a difference, a quotient and a weighting per factor, the product) and with derivative data one
    more addition, so from the sim rows the bound is no theorem at nobs = 1, though the data meet it (worst case printed).  From
    r and J a term carries 3 (+ 1): there it is a theorem at every nobs, and what J carries is held on its own."""
    worst = worst_sim = worst_j = 0.0
    for npar in range(9):
        for nobs, nsets in cases_of(npar):
            inp, nterm = fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, nsets)
            res = fr.restate(inp)
            bad = fr.expected_bad(fr.SOURCES[source], npar, deriv, nobs, nterm)
            assert (res["nbad"] == bad.sum()).all() and (res["counted"] == ~bad).all(), (source, deriv, npar, nobs, res["nbad"], int(bad.sum()))
            for s in range(nsets):
                assert np.isfinite(res["sums"][s]).all()
                ref, mag = fr.longdouble_sums(inp, res, s)
                err = np.abs(res["sums"][s].astype(np.longdouble) - ref)
                lim = (nobs + 4) * U * mag
                assert (err <= lim).all(), (source, deriv, npar, nobs, s, err, lim)
                worst = max(worst, float((err[mag > 0] / lim[mag > 0]).max()))
                ref, mag = fr.longdouble_sums(inp, res, s, start="sim")
                err = np.abs(res["sums"][s].astype(np.longdouble) - ref)
                assert (err <= (nobs + 4) * U * mag).all(), (source, deriv, npar, nobs, s, "from the sim rows", err, mag)
                worst_sim = max(worst_sim, float((err[mag > 0] / ((nobs + 4) * U * mag[mag > 0])).max()))
                worst_j = max(worst_j, fr.jacobian_error(inp, res, s))
    print(f"[fit restate {source} deriv={deriv}] worst |sum - longdouble| / ((nobs + 4) u sum|terms|) = {worst:.3f} (from the sim rows: {worst_sim:.3f}); "
          f"worst |J - longdouble| = {worst_j:.3f} u |J|")
    assert worst_j <= 2.001


@pytest.mark.parametrize("deriv", [False, True])
@pytest.mark.parametrize("source", SOURCE_NAMES)
def test_the_data_tell_the_orders_apart(source, deriv):
    """every GPU case with a second pass: under each changed order the bytes of phi differ from those of the documented order,
    and so do those of the upper triangle of A where there is one (fit_reduce_restate.orders_differ; DRAWS)"""
    n = 0
    for npar in range(9):
        for nobs, nsets in cases_of(npar):
            if nobs >= 257:
                assert fr.orders_differ(fr.synthetic(fr.SOURCES[source], npar, deriv, nobs, nsets)[0]), (source, deriv, npar, nobs)
                n += 1
    assert n == 21


def test_every_kind_of_observation_occurs():
    """what the synthetic inputs were built for, read from an input set"""
    inp, nterm = fr.synthetic(fr.FIELD, 8, True, 257, 3)
    assert set(nterm) == {0, 1, 2, 3, 7} and (inp["q"] < 0).any() and (inp["tfac"] == 1.0).any() and (inp["tfac"] > 1.0).any()
    assert set(inp["count"]) == set(fr.COUNTS) and len(set(inp["prefix"])) == 3 and len(set(inp["stride"])) == 3 and (inp["at"] > 0).all()
    assert len(set(inp["Hc"])) == len(inp["Hc"]) and (inp["Hc"] != 1.0).all() and (inp["w"] != 1.0).all()
    mag = np.abs(inp["h"][np.isfinite(inp["h"])])
    assert mag.max() / mag.min() > 1e5 and (inp["h"] < 0).any() and (inp["h"] > 0).any()
    res = fr.restate(inp)
    kind = np.arange(257) % 12
    has = nterm > 0
    assert np.isnan(res["sim"][0][has & (kind == 1)]).all() and (res["sim"][0][~has] == 0.0).all() and not np.signbit(res["sim"][0][~has]).any()
    inf = np.isinf(res["sim"][:17])                 # +Inf in h; a negative q makes it -Inf
    assert (inf.sum(axis=0)[has & (kind == 2)] == 1).all() and not inf[0].any()
    assert inf[1:, kind == 2].any(axis=1).all(), "every perturbed plan is hit"
    assert np.isnan(res["simd"][:17][:, has & (kind == 4)]).all() and res["counted"][0][kind == 4].all()
    assert (~np.isfinite(res["simd"][:17][:, has & (kind == 5)])).sum(axis=0).min() == 1 and not res["counted"][0][has & (kind == 5)].any()
    assert (inp["wd"][kind == 6] > 0).all() and (inp["w"][kind == 6] == 0).all() and (res["terms"][0][:, kind == 6] == 0).all()
    assert (res["terms_d"][0][0, has & (kind == 6)] > 0).all()
    slots, _ = fr.synthetic(fr.SLOTS, 2, False, 64, 3)
    assert (fr.restate(slots)["sim"][0][kind[:64] == 7] == fr.SENTINEL * slots["Hc"][0]).all()


# ---- the refusals of the hook

def refused(inp, word):
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    with pytest.raises(ucflib.UcfError) as err:
        fr.debug_fit_reduce(inp)
    assert err.value.status == abi.UCF_ERR_BAD_ARGUMENT and word in err.value.message, (err.value.status, err.value.message)


def accepted(inp):
    """passes every check: without a GPU the answer is UCF_ERR_NO_DEVICE, with one the call succeeds"""
    import torch
    from unconfined_amd import abi
    from unconfined_amd import lib as ucflib
    if torch.cuda.is_available():
        assert (fr.debug_fit_reduce(inp)["nbad"] >= 0).all()
        return
    with pytest.raises(ucflib.UcfError) as err:
        fr.debug_fit_reduce(inp)
    assert err.value.status == abi.UCF_ERR_NO_DEVICE, err.value.message


def test_refusals_need_no_device():
    slots, _ = fr.synthetic(fr.SLOTS, 2, True, 65, 2)
    net, _ = fr.synthetic(fr.NETWORK, 2, True, 65, 2)
    field, _ = fr.synthetic(fr.FIELD, 2, True, 65, 2)
    edit = lambda inp, **kw: {**inp, **{k: (v(inp[k].copy()) if callable(v) else v) for k, v in kw.items()}}

    def at(i, v):
        def put(a):
            a[i] = v
            return a
        return put
    # a slot beyond plan_stride, and below zero; plans that do not fit in h
    refused(edit(slots, slot=at(7, slots["plan_stride"])), "slot[7]")
    refused(edit(slots, slot=at(64, -1)), "slot[64]")
    refused(edit(slots, nh=len(slots["h"]) - 1), "plan_stride")
    refused(edit(slots, plan_stride=0), "plan_stride")
    # a ref whose last depth lies beyond h: the largest plan decides
    last = int(np.argmax(net["prefix"] * 10 + 9 * net["stride"] + net["at"] + net["count"]))
    assert net["prefix"][last] * 10 + 9 * net["stride"][last] + net["at"][last] + net["count"][last] <= len(net["h"])
    slack = int(len(net["h"]) - (net["prefix"][last] * 10 + 9 * net["stride"][last] + net["at"][last] + net["count"][last]))
    accepted(edit(net, at=at(last, net["at"][last] + slack)))
    refused(edit(net, at=at(last, net["at"][last] + slack + 1)), f"ref {last}")
    accepted(edit(net, nh=len(net["h"]) - slack))
    refused(edit(net, nh=len(net["h"]) - slack - 1), "beyond h")
    refused(edit(net, count=at(3, 0)), "ref 3")
    refused(edit(net, count=at(3, 33)), "ref 3")
    refused(edit(net, stride=at(5, -1)), "ref 5")
    refused(edit(net, prefix=at(5, 2 ** 62)), "ref 5")
    refused(edit(net, nref=64), "nref")
    # a term beyond h; a descending first; a first that does not end at the number of terms
    refused(edit(field, prefix=at(11, len(field["h"]))), "term 11")
    refused(edit(field, first=at(9, field["first"][8] - 1)), "not ascending")
    refused(edit(field, first=at(65, field["first"][65] - 1)), "number of terms")
    refused(edit(field, first=at(0, -1)), "first[0]")
    refused(edit(field, tfac=None), "tfac")
    # sizes and what must be there
    refused(edit(slots, npar=9), "npar=9")
    refused(edit(slots, npar=-1), "npar=-1")
    refused(edit(slots, nobs=0), "nobs=0")
    refused(edit(slots, nsets=0), "nsets=0")
    refused(edit(slots, source=3), "source=3")
    refused(edit(slots, dobs=None), "dobs")
    refused(edit(slots, Hc=None), "NULL")


def test_a_valid_request_reaches_the_device_check():
    """the same inputs unedited pass every check"""
    for source in fr.SOURCES.values():
        accepted(fr.synthetic(source, 2, True, 65, 2)[0])
