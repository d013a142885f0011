"""The host half of the observation-network fit (ucf_fit_create_network, ucf_fit_eval_counts of include/ucf.h), no GPU
needed: header / exports, the validation of ucf_fit_create_network, which comes before the device check, the arithmetic of
the evaluation counts on the fixture's network (tools/gen_fit_network_fixture.py), and the packing of ``wells`` in Python."""
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
SYMBOLS = ["ucf_fit_create_network", "ucf_fit_eval_counts", "ucf_fit_network_eval_counts", "ucf_fit_debug_h"]
PPP = 64            # points per block of a network launch: one tile of the lane = point layout


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(ucflib.LIB_PATH):
        ucflib.build()
    return ucflib.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "fit_network_neuman74.npz"))


def test_header_and_exports(so):
    text = open(os.path.join(ROOT, "include", "ucf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"ucf.h does not declare {s}"
        assert s in ucflib.EXPORTS and hasattr(so, s), s
    assert re.search(r"#define\s+UCF_FIT_SCREEN\s+\(-1\)", code) and abi.FIT_SCREEN == -1
    assert "UCF_VERSION 100" in code
    assert "not built)" not in text.split("parameter fitting")[1].split("UCF_FIT_MAX_PAR")[0]


def network(fx):
    """the arguments of ucf_fit_create_network after (base, npar, ids), as a dict that a case may damage"""
    return dict(nwell=len(fx["well_r"]), well_r=fx["well_r"].copy(), well_nz=fx["well_nz"].copy(), well_z=fx["well_z"].copy(),
                nobs=len(fx["t"]), t=fx["t"].copy(), well=fx["well"].copy(), iz=fx["iz"].copy(), obs=fx["obs"].copy(),
                weight=np.ones(len(fx["t"])))


def create(so, P, ids, a):
    h = C.c_void_p(1)
    ids = np.ascontiguousarray(ids, np.int32)
    rc = so.ucf_fit_create_network(C.byref(P), len(ids), ids, a["nwell"], a["well_r"], a["well_nz"], a["well_z"], a["nobs"], a["t"],
                                   a["well"], a["iz"], a["obs"], a["weight"], 0, C.byref(h))
    return rc, h, so.ucf_last_error()


def _set(key, i, v):
    def f(a):
        a[key][i] = v
    return f


def _nobs(n):
    def f(a):
        a["nobs"] = n
    return f


def _nwell(n):
    def f(a):
        a["nwell"] = n
    return f


# (what is damaged, a word that ucf_last_error must hold)
CASES = [
    (_nwell(0), b"nwell"), (_nwell(-3), b"nwell"),
    (_set("well_nz", 2, 0), b"well_nz[2]"), (_set("well_nz", 3, abi.UCF_MAX_NZ + 1), b"well_nz[3]"),
    (_set("well", 5, 4), b"well[5]"), (_set("well", 0, -1), b"well[0]"),
    (_set("well_r", 1, 0.0), b"well_r[1]"), (_set("well_r", 2, -4.0), b"well_r[2]"), (_set("well_r", 0, math.inf), b"well_r[0]"),
    (_set("well_r", 3, math.nan), b"well_r[3]"),                  # a well that no observation names is checked all the same
    (_set("well_z", 4, math.nan), b"well_z[4]"), (_set("well_z", 0, math.inf), b"well_z[0]"),
    # what ucf_fit_create checks
    (_nobs(1), b"fewer observations"),
    (_set("weight", 3, -1.0), b"weight[3]"), (_set("weight", 0, math.nan), b"weight[0]"),
    (_set("obs", 7, math.inf), b"obs[7]"),
    (_set("t", 2, 0.0), b"t[2]"), (_set("t", 9, math.nan), b"t[9]"), (_set("t", 1, -1.0), b"t[1]"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_validation_comes_before_the_device(so, fx, case):
    """every damaged network is refused with UCF_ERR_BAD_ARGUMENT and the offender named; on a machine without a GPU the
    intact one gets as far as the device check (UCF_ERR_NO_DEVICE), so the refusals above came first"""
    _, _, P = load_deck(str(fx["deck"]))
    ids = [abi.PAR_KR, abi.PAR_SY]
    a = network(fx)
    damage, word = CASES[case]
    damage(a)
    rc, h, msg = create(so, P, ids, a)
    assert rc == abi.UCF_ERR_BAD_ARGUMENT, (rc, msg)
    assert word in msg, msg
    assert not h.value


def test_iz_is_checked_against_its_own_well(so, fx):
    _, _, P = load_deck(str(fx["deck"]))
    ids = [abi.PAR_KR, abi.PAR_SY]
    piezo = int(np.flatnonzero(fx["well_nz"][fx["well"]] == 1)[0])
    screened = int(np.flatnonzero(fx["well_nz"][fx["well"]] == 3)[0])
    for i, v in ((piezo, 1), (screened, 3), (piezo, -2), (screened, -2)):
        a = network(fx)
        a["iz"][i] = v
        rc, h, msg = create(so, P, ids, a)
        assert rc == abi.UCF_ERR_BAD_ARGUMENT and (b"iz[%d]" % i) in msg and not h.value, (i, v, rc, msg)
    # in range for their well: iz = 2 of a three-depth well and the screen average of a piezometer pass validation
    for i, v in ((screened, 2), (piezo, -1)):
        a = network(fx)
        a["iz"][i] = v
        rc, h, msg = create(so, P, ids, a)
        assert rc != abi.UCF_ERR_BAD_ARGUMENT, (i, v, msg)
        if rc == 0:
            so.ucf_fit_destroy(h)


def test_the_checks_of_ucf_fit_create_on_the_parameters(so, fx):
    _, _, P = load_deck(str(fx["deck"]))
    a = network(fx)
    for ids, word in (([abi.PAR_KR, abi.PAR_KR], b"duplicate"), ([99], b"no parameter id"), ([abi.PAR_AK], b"not read")):
        rc, h, msg = create(so, P, ids, a)
        assert rc == abi.UCF_ERR_BAD_ARGUMENT and word in msg and not h.value, (ids, msg)
    _, _, T = load_deck("c1_theis")
    rc, h, msg = create(so, T, [abi.PAR_KR, abi.PAR_SY], a)
    assert rc == abi.UCF_ERR_BAD_ARGUMENT and b"Sy" in msg


def expected_counts(well_nz, t, well):
    """(launched bound, dense) from the network alone"""
    used = sorted(set(int(w) for w in well))
    nt = {w: len(set(float(x) for x in t[well == w])) for w in used}
    dense = sum(nt.values()) * int(np.sum(well_nz))
    bound = sum(math.ceil(nt[w] / PPP) * PPP * int(well_nz[w]) for w in used)
    return bound, dense


def test_eval_counts_of_the_fixture_network(fx):
    """dense = distinct (well, time) points x all depths of the network; launched = whole blocks of 64 points per used well
    x that well's depths; the network form launches less"""
    from unconfined_amd import fit as ufit
    wells = []
    at = 0
    for r, n in zip(fx["well_r"], fx["well_nz"]):
        wells.append((r, fx["well_z"][at:at + n]))
        at += n
    launched, dense = ufit.network_eval_counts(wells, fx["t"], fx["well"])
    bound, want_dense = expected_counts(fx["well_nz"], fx["t"], fx["well"])
    # 5 + 70 + 9 distinct points (the extra observation of C shares one), 1 + 1 + 3 + 3 depths
    assert want_dense == (5 + 70 + 9) * 8
    assert dense == want_dense
    assert 0 < launched <= bound
    assert launched == bound                   # blocks of exactly 64 points
    assert launched < dense
    # an unused well costs nothing; one more observation at an existing (well, time) neither
    t2, w2 = np.append(fx["t"], fx["t"][0]), np.append(fx["well"], fx["well"][0])
    assert ufit.network_eval_counts(wells, t2, w2) == (launched, dense)
    # a new time in the piezometer with 5 times stays inside its block: launched unchanged, dense grows by all depths
    first_a = fx["t"][fx["well"] == 0][0]
    t3, w3 = np.append(fx["t"], first_a * 1.5), np.append(fx["well"], 0)
    assert ufit.network_eval_counts(wells, t3, w3) == (launched, dense + 8)


def test_eval_counts_refuses_a_bad_network(so):
    a, b = C.c_longlong(), C.c_longlong()
    nz = np.array([1, 40], np.int32)
    t, w = np.array([1.0, 2.0]), np.array([0, 1], np.int32)
    assert so.ucf_fit_network_eval_counts(2, nz, 2, t, w, C.byref(a), C.byref(b)) == abi.UCF_ERR_BAD_ARGUMENT
    assert b"well_nz[1]" in so.ucf_last_error()
    nz[1] = 2
    w[1] = 2
    assert so.ucf_fit_network_eval_counts(2, nz, 2, t, w, C.byref(a), C.byref(b)) == abi.UCF_ERR_BAD_ARGUMENT
    assert b"well[1]" in so.ucf_last_error()


def test_python_packs_the_wells(monkeypatch):
    """Fit.network hands ucf_fit_create_network the radii, the depth counts and the depths one after the other"""
    from unconfined_amd import fit as ufit
    wells = [(30.0, [150.0]), (85.1, np.array([105.0, 123.0, 141.0])), (7, 2.5)]
    r, nz, z = ufit.pack_wells(wells)
    assert r.dtype == np.float64 and nz.dtype == np.int32 and z.dtype == np.float64
    assert r.tolist() == [30.0, 85.1, 7.0] and nz.tolist() == [1, 3, 1] and z.tolist() == [150.0, 105.0, 123.0, 141.0, 2.5]
    seen = {}

    class FakeLib:
        def ucf_fit_create_network(self, base, npar, ids, nwell, well_r, well_nz, well_z, nobs, t, well, iz, obs, weight, device, out):
            seen.update(npar=npar, ids=ids.tolist(), nwell=nwell, well_r=well_r.tolist(), well_nz=well_nz.tolist(), well_z=well_z.tolist(),
                        nobs=nobs, t=t.tolist(), well=well.tolist(), iz=iz.tolist(), obs=obs.tolist(), weight=weight.tolist(), device=device,
                        dtypes=(well_nz.dtype, well.dtype, iz.dtype, t.dtype))
            return 0

        def ucf_fit_destroy(self, h):
            pass

    monkeypatch.setattr(ufit._libmod, "load", lambda: FakeLib())
    _, _, P = load_deck("neuman74_partpen")
    f = ufit.Fit.network(P, ["Kr", "Sy"], wells, t=[1, 2, 3], well=[0, 1, 1], iz=[0, -1, 2], obs=[0.1, 0.2, 0.3])
    assert isinstance(f, ufit.Fit) and f.nobs == 3 and f.npar == 2
    assert seen["ids"] == [abi.PAR_KR, abi.PAR_SY] and seen["nwell"] == 3 and seen["nobs"] == 3
    assert seen["well_r"] == [30.0, 85.1, 7.0] and seen["well_nz"] == [1, 3, 1] and seen["well_z"] == [150.0, 105.0, 123.0, 141.0, 2.5]
    assert seen["t"] == [1.0, 2.0, 3.0] and seen["well"] == [0, 1, 1] and seen["iz"] == [0, -1, 2] and seen["weight"] == [1.0, 1.0, 1.0]
    assert seen["dtypes"] == (np.int32, np.int32, np.int32, np.float64)
    with pytest.raises(ValueError):
        ufit.Fit.network(P, ["Kr", "Sy"], wells, t=[1, 2, 3], well=[0, 1], iz=[0, -1, 2], obs=[0.1, 0.2, 0.3])
