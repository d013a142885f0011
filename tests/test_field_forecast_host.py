"""The host half of ucf_field_forecast (include/ucf.h): the parameter sets of a forecast against numpy, and every refusal of
the argument checks with its offender named.  No GPU is needed: the checks come before the call asks for a device.  That the
fit's sums did not move when its parameter-set loop became the helper that ucf_field_forecast_sets shares is what
tests/test_fit_host.py and the GPU fit tests judge, unchanged."""
import ctypes as C

import numpy as np
import pytest

from golden_util import load_deck
from unconfined_amd import abi
from unconfined_amd import lib as ucflib
from unconfined_amd.fit import par_id

BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def col(a, j):
    return np.ascontiguousarray(np.asarray(a, float)[:, j])


def create(so, wells=WELLS, loc=LOCATIONS, t=TIMES):
    h = C.c_void_p()
    assert so.ucf_field_create(len(wells), col(wells, 0), col(wells, 1), col(wells, 2), col(wells, 3), len(loc), col(loc, 0), col(loc, 1),
                               len(t), np.ascontiguousarray(t, dtype=float), C.byref(h)) == 0
    return h


def addr(a):
    return a.ctypes.data if a is not None else None


def moench4():
    """deck c3_moench with a fourth alpha"""
    _, _, P = load_deck("c3_moench")
    P.MoenchM = 4
    P.MoenchAlpha[3] = 2.5
    return P


def problems():
    _, _, theis = load_deck("c1_theis")
    _, _, neuman = load_deck("neuman74_partpen")
    return [(theis, ["Kr", "Ss"]), (neuman, ["Kr", "kappa", "Ss", "Sy"]),
            (moench4(), ["Kr", "kappa", "Ss", "Sy"] + [f"MoenchAlpha[{i}]" for i in range(4)])]


def sets_of(so, P, ids, theta, dlog):
    ids, theta = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(theta, dtype=float)
    out = (abi.UcfParams * (1 + 2 * len(ids)))()
    rc = so.ucf_field_forecast_sets(C.byref(P), len(ids), addr(ids), addr(theta), dlog, out)
    return rc, out, (so.ucf_last_error() or b"").decode()


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("dlog", [1e-3, 0.25])
def test_sets_are_perturb_and_one_product(so, case, dlog):
    P, free = problems()[case]
    ids = np.array([par_id(n) for n in free], np.int32)
    rng = np.random.default_rng(case)
    base = np.array([P.MoenchAlpha[i - abi.PAR_MOENCH_ALPHA0] if i >= abi.PAR_MOENCH_ALPHA0 else getattr(P, n) for i, n in zip(ids, free)])
    theta = base * np.exp(rng.uniform(-0.3, 0.3, len(ids)))
    rc, got, msg = sets_of(so, P, ids, theta, dlog)
    assert rc == 0, msg
    assert len(got) == 1 + 2 * len(ids) == (5, 9, 17)[case]
    up, down = np.exp(np.float64(dlog)), np.exp(-np.float64(dlog))
    for k in range(len(got)):
        th = theta.copy()
        if k > 0:
            j = (k - 1) // 2
            th[j] = th[j] * (up if k & 1 else down)
        want = abi.UcfParams()
        assert so.ucf_fit_perturb(C.byref(P), len(ids), ids, th, C.byref(want)) == 0
        assert bytes(got[k]) == bytes(want), (case, k)
    assert bytes(got[1]) != bytes(got[0]) != bytes(got[2])


def test_sets_refusals_name_the_offender(so):
    _, _, P = load_deck("neuman74_partpen")
    ids = [par_id(n) for n in ("Kr", "kappa", "Ss", "Sy")]
    theta = [P.Kr, P.kappa, P.Ss, P.Sy]
    cases = [
        (dict(ids=ids + ids + [0]), "npar"), (dict(ids=[0, 1, 0, 3]), "duplicate"), (dict(ids=[0, 1, 2, abi.PAR_IDS["ak"]]), "ak"),
        (dict(theta=[P.Kr, -1.0, P.Ss, P.Sy]), "kappa"), (dict(theta=[P.Kr, P.kappa, np.inf, P.Sy]), "Ss"),
        (dict(theta=[P.Kr, P.kappa, P.Ss, 0.0]), "Sy"),
        (dict(dlog=0.0), "dlog"), (dict(dlog=-1e-3), "dlog"), (dict(dlog=np.nan), "dlog"), (dict(dlog=np.inf), "dlog"),
    ]
    for kw, offender in cases:
        a = dict(ids=ids, theta=theta, dlog=1e-3)
        a.update(kw)
        if len(a["ids"]) != len(a["theta"]):
            a["theta"] = [1.0] * len(a["ids"])
        rc, _, msg = sets_of(so, P, a["ids"], a["theta"], a["dlog"])
        assert rc == BAD and offender in msg, (kw, rc, msg)
    out = (abi.UcfParams * 9)()
    th = np.array(theta)
    assert so.ucf_field_forecast_sets(C.byref(P), 4, None, addr(th), 1e-3, out) == BAD and b"ids" in so.ucf_last_error()
    assert so.ucf_field_forecast_sets(C.byref(P), 4, addr(np.array(ids, np.int32)), None, 1e-3, out) == BAD
    assert so.ucf_field_forecast_sets(None, 4, addr(np.array(ids, np.int32)), addr(th), 1e-3, out) == BAD
    # a set that the plan builder would refuse keeps its status and is named: the base set ...
    _, _, Pbad = load_deck("neuman74_partpen")
    Pbad.b = -1.0
    rc, _, msg = sets_of(so, Pbad, ids, theta, 1e-3)
    assert rc == -3 and "set 0" in msg, (rc, msg)
    # ... and a perturbed one: Kr exp(-dlog) underflows to 0 in set 2
    rc, _, msg = sets_of(so, P, ids, [1e-300, P.kappa, P.Ss, P.Sy], 700.0)
    assert rc == -3 and "set 2" in msg and "Kr" in msg and "-700" in msg, (rc, msg)


def forecast(so, h, plan=None, npar=2, ids=(0, 2), theta=(1.0, 1e-4), dlog=1e-3, cov=None, nz=2, z=(145.7, 100.0), shape=(6, 5, 2),
             want=("s", "ds", "sens", "dsens"), null=()):
    """one call with small host arrays; `want`: the outputs that are passed, `null`: required arguments passed as NULL"""
    arrs = dict(ids=np.ascontiguousarray(ids, dtype=np.int32), theta=np.ascontiguousarray(theta, dtype=float),
                z=np.ascontiguousarray(z, dtype=float), cov=None if cov is None else np.ascontiguousarray(cov, dtype=float))
    n = int(np.prod(shape))
    sizes = dict(s=n, ds=n, sens=npar * n, dsens=npar * n, se=n, dse=n, s_all=(1 + 2 * npar) * n, ds_all=(1 + 2 * npar) * n)
    out = {k: (np.zeros(max(sizes[k], 1)) if k in want else None) for k in sizes}
    for k in null:
        if k in arrs:
            arrs[k] = None
        else:
            out[k] = None
    nbad = np.zeros(2, np.int64)
    rc = so.ucf_field_forecast(h, plan, npar, addr(arrs["ids"]), addr(arrs["theta"]), dlog, addr(arrs["cov"]), nz, addr(arrs["z"]),
                               *(addr(out[k]) for k in ("s", "ds", "sens", "dsens", "se", "dse", "s_all", "ds_all")), addr(nbad), None)
    return rc, (so.ucf_last_error() or b"").decode()


def test_forecast_refusals_name_the_offender(so):
    import torch
    h = create(so)
    good = np.array([[0.01, 0.002], [0.002, 0.03]])
    cases = [
        # what ucf_field_drawdown checks
        (dict(nz=0), "nz"), (dict(z=(145.7, np.nan)), "z[1]"), (dict(null=("z",)), "NULL z"),
        # NULL ids, theta, s, ds
        (dict(null=("ids",)), "NULL ids"), (dict(null=("theta",)), "NULL theta"), (dict(null=("s",)), "NULL s"), (dict(null=("ds",)), "NULL ds"),
        # npar, dlog
        (dict(npar=0, ids=(0,), theta=(1.0,)), "npar=0"), (dict(npar=abi.UCF_FIT_MAX_PAR + 1, ids=range(9), theta=[1.0] * 9), "npar=9"),
        (dict(dlog=0.0), "dlog"), (dict(dlog=-1e-3), "dlog"), (dict(dlog=np.nan), "dlog"), (dict(dlog=np.inf), "dlog"),
        # a standard error without a covariance
        (dict(want=("s", "ds", "se")), "se is asked for without cov"), (dict(want=("s", "ds", "dse")), "dse is asked for without cov"),
        # the covariance
        (dict(cov=[[0.01, np.nan], [np.nan, 0.03]]), "cov[0][1]"), (dict(cov=[[0.01, 0.002], [0.002, np.inf]]), "cov[1][1]"),
        (dict(cov=[[0.01, 0.002], [0.0021, 0.03]]), "cov[0][1]"), (dict(cov=[[0.01, 0.002], [0.002, -0.03]]), "cov[1][1]"),
    ]
    for kw, offender in cases:
        rc, msg = forecast(so, h, **kw)
        assert rc == BAD and offender in msg, (kw, rc, msg)
    rc, msg = forecast(so, h, cov=[[0.01, 0.002], [0.0021, 0.03]])
    assert "cov[1][0]" in msg and "symmetric" in msg, msg
    rc, msg = forecast(so, None)
    assert rc == BAD and "field" in msg
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device
    for kw in (dict(), dict(cov=good, want=("s", "ds", "se", "dse", "s_all", "ds_all")), dict(cov=good, want=("s", "ds"))):
        rc, msg = forecast(so, h, **kw)
        if torch.cuda.is_available():
            assert rc == BAD and "plan" in msg, (kw, msg)
        else:
            assert rc == NO_DEVICE and "no CPU fallback" in msg, (kw, msg)
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def test_forecast_refuses_more_values_than_a_buffer_holds(so):
    """70000 times x 40000 locations x 12 depths: a map that ucf_field_drawdown accepts (3.4e10 outputs, below 2^31-1 blocks
    of 256), but not the 17 maps of 8 parameters"""
    loc = np.stack([np.linspace(10.0, 5000.0, 40000), np.zeros(40000)], axis=1)
    h = create(so, np.array([[0.0, 0.0, 1.0, 0.0]]), loc, np.linspace(1.0, 1000.0, 70000))
    z = np.linspace(1.0, 12.0, 12)
    small = np.zeros(4)
    assert 70000 * 40000 * 12 <= (2 ** 31 - 1) * 256 < 17 * 70000 * 40000 * 12
    rc, msg = forecast(so, h, npar=8, ids=range(8), theta=[1.0] * 8, nz=12, z=z, shape=(1,), want=("s", "ds"))
    assert rc == BAD and "17 parameter sets" in msg and "too many" in msg, (rc, msg)
    # one parameter: 3 maps fit, the call goes on to ask for a plan
    rc, msg = forecast(so, h, npar=1, ids=(0,), theta=(1.0,), nz=12, z=z, shape=(1,), want=("s", "ds"))
    assert rc in (NO_DEVICE, BAD) and "too many" not in msg, (rc, msg)
    assert so.ucf_field_alloc_count(h) == 0 and small.sum() == 0.0
    so.ucf_field_destroy(h)


def test_python_front_end_without_a_gpu():
    from unconfined_amd import forecast_sets
    _, _, P = load_deck("c1_theis")
    sets = forecast_sets(P, ["Kr", "Ss"], [P.Kr, P.Ss], 1e-3)
    assert len(sets) == 5 and bytes(sets[0]) == bytes(P)
    assert sets[1].Kr == P.Kr * np.exp(1e-3) and sets[2].Kr == P.Kr * np.exp(-1e-3) and sets[1].Ss == P.Ss
    assert sets[3].Ss == P.Ss * np.exp(1e-3) and sets[4].Ss == P.Ss * np.exp(-1e-3) and sets[3].Kr == P.Kr
    with pytest.raises(ucflib.UcfError) as e:
        forecast_sets(P, ["Kr", "Sy"], [P.Kr, 0.1], 1e-3)
    assert e.value.status == BAD and "Sy" in e.value.message
    with pytest.raises(ValueError):
        forecast_sets(P, ["Kr", "Ss"], [P.Kr], 1e-3)
