"""The host half of the field fit (ucf_fit_create_field, ucf_fit_field_terms of include/ucf.h), no GPU needed: header /
exports, the validation of ucf_fit_create_field, which comes before the device check, the layout rules -- virtual wells and
terms -- on a case written out by hand and on the fixture (tools/gen_fit_field_fixture.py forms them in numpy), the
evaluation counts of the network of virtual wells, and the packing of the arguments in Python."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ucf_fit_create_field", "ucf_fit_field_terms"]
PPP = 64            # points per block of a network launch


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(ucflib.LIB_PATH):
        ucflib.build()
    return ucflib.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "fit_field_neuman74.npz"))


def obs_wells_of(fx):
    out, at = [], 0
    for x, y, n in zip(fx["well_x"], fx["well_y"], fx["well_nz"]):
        out.append((float(x), float(y), fx["well_z"][at:at + n].copy()))
        at += n
    return out


def test_header_and_exports(so):
    text = open(os.path.join(ROOT, "include", "ucf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    assert "UCF_VERSION 100" in code


def field(fx):
    """the arguments of ucf_fit_create_field after (base, npar, ids), as a dict that a case may damage"""
    p = fx["pump"]
    return dict(npump=len(p), xw=p[:, 0].copy(), yw=p[:, 1].copy(), qw=p[:, 2].copy(), t0w=p[:, 3].copy(),
                nwell=len(fx["well_x"]), well_x=fx["well_x"].copy(), well_y=fx["well_y"].copy(), well_nz=fx["well_nz"].copy(),
                well_z=fx["well_z"].copy(), nobs=len(fx["t"]), t=fx["t"].copy(), well=fx["well"].copy(), iz=fx["iz"].copy(),
                obs=fx["obs"].copy(), weight=np.ones(len(fx["t"])))


def create(so, P, ids, a):
    h = C.c_void_p(1)
    ids = np.ascontiguousarray(ids, np.int32)
    rc = so.ucf_fit_create_field(C.byref(P), len(ids), ids, a["npump"], a["xw"], a["yw"], a["qw"], a["t0w"], a["nwell"], a["well_x"],
                                 a["well_y"], a["well_nz"], a["well_z"], a["nobs"], a["t"], a["well"], a["iz"], a["obs"], a["weight"], 0,
                                 C.byref(h))
    return rc, h, so.ucf_last_error()


def _set(key, i, v):
    def f(a):
        a[key][i] = v
    return f


def _count(key, n):
    def f(a):
        a[key] = n
    return f


def _into_the_bore_of_p1(a):
    """D, which no observation names, 0.1 from P1 (both decks have rw > 0.02; neuman74_partpen: 0.3333)"""
    a["well_x"][3], a["well_y"][3] = a["xw"][1] + 0.1, a["yw"][1]


def _onto_p0(a):
    a["well_x"][0], a["well_y"][0] = a["xw"][0], a["yw"][0]


# (what is damaged, words that ucf_last_error must hold)
CASES = [
    # the pumping wells, as ucf_field_create checks them
    (_set("qw", 1, 0.0), [b"qw[1]"]), (_set("t0w", 2, -1.0), [b"t0w[2]"]), (_set("t0w", 0, math.nan), [b"t0w[0]"]),
    (_set("xw", 1, math.nan), [b"xw[1]"]), (_set("yw", 0, math.inf), [b"yw[0]"]), (_set("qw", 2, math.nan), [b"qw[2]"]),
    (_count("npump", 0), [b"npump"]), (_count("npump", -2), [b"npump"]),
    # the observation wells
    (_set("well_x", 2, math.nan), [b"well_x[2]"]), (_set("well_y", 3, math.inf), [b"well_y[3]"]),
    (_into_the_bore_of_p1, [b"observation well 3", b"pumping well 1", b"bore"]),
    (_onto_p0, [b"observation well 0", b"pumping well 0", b"bore"]),
    (_count("nwell", 0), [b"nwell"]),
    (_set("well_nz", 1, 0), [b"well_nz[1]"]), (_set("well_nz", 3, abi.UCF_MAX_NZ + 1), [b"well_nz[3]"]),
    (_set("well_z", 2, math.nan), [b"well_z[2]"]),
    # the observations
    (_set("well", 5, 4), [b"well[5]"]), (_set("well", 0, -1), [b"well[0]"]),
    (_count("nobs", 1), [b"fewer observations"]),
    (_set("weight", 3, -1.0), [b"weight[3]"]), (_set("obs", 7, math.inf), [b"obs[7]"]),
    (_set("t", 2, 0.0), [b"t[2]"]), (_set("t", 9, math.nan), [b"t[9]"]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_validation_comes_before_the_device(so, fx, case):
    """every damaged argument set is refused with UCF_ERR_BAD_ARGUMENT and the offender named"""
    _, _, P = load_deck(str(fx["deck"]))
    a = field(fx)
    damage, words = CASES[case]
    damage(a)
    rc, h, msg = create(so, P, [abi.PAR_KR, abi.PAR_SY], a)
    assert rc == abi.UCF_ERR_BAD_ARGUMENT, (rc, msg)
    for word in words:
        assert word in msg, msg
    assert not h.value


def test_the_untouched_arguments_reach_the_device_check(so, fx):
    """on a machine without a GPU the intact argument set gets as far as the device check (UCF_ERR_NO_DEVICE), so the
    refusals above came first; with a GPU it makes a fit"""
    _, _, P = load_deck(str(fx["deck"]))
    rc, h, msg = create(so, P, [abi.PAR_KR, abi.PAR_SY], field(fx))
    ndev = C.c_int()
    if so.ucf_device_count(C.byref(ndev)) == 0 and ndev.value > 0:
        assert rc == 0, msg
        so.ucf_fit_destroy(h)
    else:
        assert rc == abi.UCF_ERR_NO_DEVICE and not h.value, (rc, msg)


def test_iz_is_checked_against_its_own_well(so, fx):
    _, _, P = load_deck(str(fx["deck"]))
    ids = [abi.PAR_KR, abi.PAR_SY]
    piezo = int(np.flatnonzero(fx["well_nz"][fx["well"]] == 1)[0])
    screened = int(np.flatnonzero(fx["well_nz"][fx["well"]] == 3)[0])
    for i, v in ((piezo, 1), (screened, 3), (piezo, -2)):
        a = field(fx)
        a["iz"][i] = v
        rc, h, msg = create(so, P, ids, a)
        assert rc == abi.UCF_ERR_BAD_ARGUMENT and (b"iz[%d]" % i) in msg and not h.value, (i, v, rc, msg)
    for i, v in ((screened, 2), (piezo, -1)):
        a = field(fx)
        a["iz"][i] = v
        rc, h, msg = create(so, P, ids, a)
        assert rc != abi.UCF_ERR_BAD_ARGUMENT, (i, v, msg)
        if rc == 0:
            so.ucf_fit_destroy(h)


def test_parameter_checks_and_a_field_without_terms(so, fx):
    _, _, P = load_deck(str(fx["deck"]))
    a = field(fx)
    for ids, word in (([abi.PAR_KR, abi.PAR_KR], b"duplicate"), ([99], b"no parameter id"), ([abi.PAR_AK], b"not read")):
        rc, h, msg = create(so, P, ids, a)
        assert rc == abi.UCF_ERR_BAD_ARGUMENT and word in msg and not h.value, (ids, msg)
    a["t0w"][:] = 1.0e6                              # every well starts after the last observation
    rc, h, msg = create(so, P, [abi.PAR_KR, abi.PAR_SY], a)
    assert rc == abi.UCF_ERR_BAD_ARGUMENT and b"nothing to fit" in msg and not h.value, msg


def test_terms_of_a_case_written_out_by_hand():
    """pumping wells at (-3, 0) and (+3, 0), starting at t = 1 and t = 2; observation well 0 at (0, 4) lies 5 from both: ONE
    virtual well; observation well 1 at (3, 4) lies sqrt(52) from the first and 4 from the second: two virtual wells, the
    nearer one first.  t == t0 gives no term, an observation before every start has none at all, the terms of an
    observation follow the pumping wells' order, and term_t is t - t0 bit for bit"""
    from unconfined_amd import fit as ufit
    _, _, P = load_deck("neuman74_partpen")
    wells = [(-3.0, 0.0, 1.0, 1.0), (3.0, 0.0, -1.0, 2.0)]
    obs_wells = [(0.0, 4.0), (3.0, 4.0)]
    t = np.array([2.0, 0.5, 5.5, 2.3])
    well = np.array([0, 1, 0, 1], np.int32)
    got = ufit.field_terms(P, wells, obs_wells, t, well)
    assert got["virt_well"].tolist() == [0, 1, 1] and got["virt_well"].dtype == np.int32
    assert got["virt_r"].tobytes() == np.array([5.0, 4.0, np.sqrt(np.float64(52.0))]).tobytes()
    assert got["term_first"].tolist() == [0, 1, 1, 3, 5]
    assert got["term_pump"].tolist() == [0, 0, 1, 0, 1]
    assert got["term_virt"].tolist() == [0, 0, 0, 2, 1]
    want_t = np.array([t[0] - 1.0, t[2] - 1.0, t[2] - 2.0, t[3] - 1.0, t[3] - 2.0])
    assert got["term_t"].tobytes() == want_t.tobytes()
    assert got["term_t"][3] != 1.3                   # one rounding of the difference, not the decimal number
    # swapped pumping wells: the terms of an observation swap with them
    got = ufit.field_terms(P, wells[::-1], obs_wells, t, well)
    assert got["term_first"].tolist() == [0, 1, 1, 3, 5] and got["term_pump"].tolist() == [1, 0, 1, 0, 1]
    assert got["term_virt"].tolist() == [0, 0, 0, 1, 2] and got["virt_r"][0] == 5.0


def test_terms_refuse_what_create_refuses(so):
    from unconfined_amd import fit as ufit
    _, _, P = load_deck("neuman74_partpen")
    for wells, obs_wells, t, well, words in (
            ([(0, 0, 0.0, 0)], [(5, 0)], [1.0], [0], ["qw[0]"]),
            ([(0, 0, 1.0, -1.0)], [(5, 0)], [1.0], [0], ["t0w[0]"]),
            ([(0, 0, 1.0, 0), (5.2, 0, 1.0, 0)], [(9, 0), (5, 0)], [1.0], [0], ["observation well 1", "pumping well 1"]),
            ([(0, 0, 1.0, 0)], [(5, 0)], [1.0], [1], ["well[0]"]),
            ([(0, 0, 1.0, 0)], [(5, 0)], [-1.0], [0], ["t[0]"])):
        with pytest.raises(ucflib.UcfError) as e:
            ufit.field_terms(P, wells, obs_wells, t, well)
        assert e.value.status == abi.UCF_ERR_BAD_ARGUMENT
        for w in words:
            assert w in e.value.message, e.value.message


@pytest.mark.parametrize("key", ["neuman74", "theis"])
def test_terms_of_the_fixture(key):
    """the library's layout equals the generator's numpy statement of the rules, bit for bit; and the field is the one the
    fixture is meant to be"""
    from unconfined_amd import fit as ufit
    fx = np.load(os.path.join(GOLD, f"fit_field_{key}.npz"))
    _, _, P = load_deck(str(fx["deck"]))
    got = ufit.field_terms(P, fx["pump"], obs_wells_of(fx), fx["t"], fx["well"])
    for k in ("virt_well", "virt_r", "term_first", "term_pump", "term_virt", "term_t"):
        assert got[k].dtype == fx[k].dtype and got[k].tobytes() == fx[k].tobytes(), k
    per_obs = np.diff(fx["term_first"])
    assert set(per_obs[fx["well"] == 2]) == {2} and set(per_obs[fx["well"] == 0]) == {2, 3}      # C never sees P1, A sometimes
    assert 3 not in fx["well"] and 3 in fx["virt_well"]                                          # D: virtual wells, no term
    assert len(fx["virt_well"]) == 12                 # four observation wells x three distinct distances
    assert fx["pump"][2].tolist()[2:] == [-1.0, 0.0]  # the constant-head image of P0


def expected_counts(virt_nz, term_t, term_virt):
    """launched = whole blocks of 64 distinct times per used virtual well x its depths; dense = distinct (virtual well, time)
    points x the depths of all virtual wells"""
    used = sorted(set(int(v) for v in term_virt))
    nt = {v: len(set(float(x) for x in term_t[term_virt == v])) for v in used}
    return sum(math.ceil(nt[v] / PPP) * PPP * int(virt_nz[v]) for v in used), sum(nt.values()) * int(np.sum(virt_nz))


def test_eval_counts_are_those_of_the_network_of_virtual_wells(so, fx):
    virt_nz = np.ascontiguousarray(fx["well_nz"][fx["virt_well"]], np.int32)
    a, b = C.c_longlong(), C.c_longlong()
    ucflib.check(so.ucf_fit_network_eval_counts(len(virt_nz), virt_nz, len(fx["term_t"]), fx["term_t"], fx["term_virt"], C.byref(a), C.byref(b)))
    launched, dense = expected_counts(virt_nz, fx["term_t"], fx["term_virt"])
    assert (a.value, b.value) == (launched, dense)
    # A towards P0 and towards the image: 66 times = two blocks each; towards P1 fewer times, one block; B: one block of
    # three depths per pumping well; C: one block each towards P0 and the image, none towards P1
    n_a1 = int(np.sum((fx["t"] > 20.0) & (fx["well"] == 0)))
    assert 0 < n_a1 < 64
    assert launched == (2 + 2 + 1) * PPP + 3 * PPP * 3 + 2 * PPP
    assert dense == (66 + 66 + n_a1 + 6 + 6 + 4 + 4 + 4) * (3 * (1 + 3 + 1 + 3))


def test_python_packs_the_field(monkeypatch):
    """Fit.field hands ucf_fit_create_field the columns of the pumping wells, the positions, the depth counts and the
    depths one after the other"""
    from unconfined_amd import fit as ufit
    wells = [(0, 0, 1, 0), (40.0, 30.0, 0.6, 20.0), (200.0, 0.0, -1.0, 0.0)]
    obs_wells = [(10.0, 5.0, [150.0]), (25, -8, np.array([105.0, 123.0, 141.0])), (7, 1, 2.5)]
    x, y, nz, z = ufit.pack_obs_wells(obs_wells)
    assert x.dtype == y.dtype == z.dtype == np.float64 and nz.dtype == np.int32
    assert x.tolist() == [10.0, 25.0, 7.0] and y.tolist() == [5.0, -8.0, 1.0] and nz.tolist() == [1, 3, 1]
    assert z.tolist() == [150.0, 105.0, 123.0, 141.0, 2.5]
    seen = {}

    class FakeLib:
        def ucf_fit_create_field(self, base, npar, ids, npump, xw, yw, qw, t0w, nwell, well_x, well_y, well_nz, well_z, nobs, t, well, iz,
                                 obs, weight, device, out):
            seen.update(npar=npar, ids=ids.tolist(), npump=npump, xw=xw.tolist(), yw=yw.tolist(), qw=qw.tolist(), t0w=t0w.tolist(),
                        nwell=nwell, well_x=well_x.tolist(), well_y=well_y.tolist(), well_nz=well_nz.tolist(), well_z=well_z.tolist(),
                        nobs=nobs, t=t.tolist(), well=well.tolist(), iz=iz.tolist(), obs=obs.tolist(), weight=weight.tolist(),
                        device=device, dtypes=(xw.dtype, t0w.dtype, well_nz.dtype, well.dtype, iz.dtype, t.dtype),
                        contiguous=all(v.flags["C_CONTIGUOUS"] for v in (xw, yw, qw, t0w)))
            return 0

        def ucf_fit_destroy(self, h):
            pass

    monkeypatch.setattr(ufit._libmod, "load", lambda: FakeLib())
    _, _, P = load_deck("neuman74_partpen")
    f = ufit.Fit.field(P, ["Kr", "Sy"], wells, obs_wells, t=[1, 2, 30], well=[0, 1, 1], iz=[0, -1, 2], obs=[0.1, 0.2, 0.3], device=0)
    assert isinstance(f, ufit.Fit) and f.nobs == 3 and f.npar == 2
    assert seen["ids"] == [abi.PAR_KR, abi.PAR_SY] and seen["npump"] == 3 and seen["nwell"] == 3 and seen["nobs"] == 3
    assert seen["xw"] == [0.0, 40.0, 200.0] and seen["yw"] == [0.0, 30.0, 0.0] and seen["qw"] == [1.0, 0.6, -1.0]
    assert seen["t0w"] == [0.0, 20.0, 0.0] and seen["contiguous"]
    assert seen["well_x"] == [10.0, 25.0, 7.0] and seen["well_y"] == [5.0, -8.0, 1.0] and seen["well_nz"] == [1, 3, 1]
    assert seen["well_z"] == [150.0, 105.0, 123.0, 141.0, 2.5]
    assert seen["t"] == [1.0, 2.0, 30.0] and seen["well"] == [0, 1, 1] and seen["iz"] == [0, -1, 2] and seen["weight"] == [1.0, 1.0, 1.0]
    assert seen["dtypes"] == (np.float64, np.float64, np.int32, np.int32, np.int32, np.float64)
    with pytest.raises(ValueError):
        ufit.Fit.field(P, ["Kr", "Sy"], wells, obs_wells, t=[1, 2, 30], well=[0, 1], iz=[0, -1, 2], obs=[0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        ufit.Fit.field(P, ["Kr", "Sy"], [(0, 0, 1)], obs_wells, t=[1, 2, 30], well=[0, 1, 1], iz=[0, -1, 2], obs=[0.1, 0.2, 0.3])
