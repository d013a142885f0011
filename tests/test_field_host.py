"""The host half of the well-field entry points (ucf_field_* of include/ucf.h): argument checks, the launch arrays of a group
against a numpy restatement of the arithmetic that the header states, and the image wells.  No GPU is needed: a plan cannot
exist without a device, so the launch arrays are taken from ucf_field_group_from_params -- the same code as ucf_field_group
behind a parameter set instead of a plan (tests/test_gpu_field.py compares the two on the GPU)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from golden_util import load_deck
from unconfined_amd import abi
from unconfined_amd import lib as ucflib

U = 2.0 ** -53
BAD, NO_DEVICE = abi.UCF_ERR_BAD_ARGUMENT, abi.UCF_ERR_NO_DEVICE
# 4 wells (x, y, q, t0) in 2 start-time groups; 5 locations, the first equidistant from wells 0 and 1; 6 times, 2 before t0 = 5
WELLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.6, 0.0], [0.0, 1.5, -0.5, 5.0], [1.0, -1.0, 0.8, 5.0]])
LOCATIONS = np.array([[1.0, 0.7], [0.4, 0.3], [1.5, -0.4], [-0.6, 0.5], [2.5, 1.2]])
TIMES = np.array([0.5, 2.0, 7.0, 150.0, 1000.0, 3000.0])


@pytest.fixture(scope="module")
def so():
    return ucflib.load()


def col(a, j):
    return np.ascontiguousarray(np.asarray(a, float)[:, j])


def create(so, wells=WELLS, loc=LOCATIONS, t=TIMES, nwell=None, nloc=None, nt=None):
    wells, loc, t = np.atleast_2d(np.asarray(wells, float)), np.atleast_2d(np.asarray(loc, float)), np.asarray(t, float)
    h = C.c_void_p()
    rc = so.ucf_field_create(len(wells) if nwell is None else nwell, col(wells, 0), col(wells, 1), col(wells, 2), col(wells, 3),
                             len(loc) if nloc is None else nloc, col(loc, 0), col(loc, 1), len(t) if nt is None else nt,
                             np.ascontiguousarray(t), C.byref(h))
    return rc, h, (so.ucf_last_error() or b"").decode()


def changed(a, i, j, v):
    a = np.array(a, float)
    a[i, j] = v
    return a


def test_create_names_the_offender(so):
    cases = [
        (dict(nwell=0), "nwell"), (dict(nloc=0), "nloc"), (dict(nt=0), "nt"),
        (dict(wells=changed(WELLS, 1, 0, np.nan)), "xw[1]"), (dict(wells=changed(WELLS, 2, 1, np.inf)), "yw[2]"),
        (dict(wells=changed(WELLS, 3, 2, np.nan)), "qw[3]"), (dict(wells=changed(WELLS, 0, 3, np.inf)), "t0w[0]"),
        (dict(loc=changed(LOCATIONS, 4, 0, -np.inf)), "x[4]"), (dict(loc=changed(LOCATIONS, 2, 1, np.nan)), "y[2]"),
        (dict(t=[0.5, np.nan, 10.0]), "t[1]"),
        (dict(t=[0.5, 2.0, 2.0]), "t[2]"), (dict(t=[0.5, 2.0, 1.0]), "t[2]"), (dict(t=[0.0, 2.0]), "t[0]"), (dict(t=[-1.0, 2.0]), "t[0]"),
        (dict(wells=changed(WELLS, 2, 3, -1.0)), "t0w[2]"),
        (dict(wells=changed(WELLS, 1, 2, 0.0)), "qw[1]"),
    ]
    for kw, offender in cases:
        rc, h, msg = create(so, **kw)
        assert rc == BAD and not h.value, (kw, rc)
        assert offender in msg, (kw, msg)
    rc, h, _ = create(so)
    assert rc == 0 and h.value
    n = C.c_int()
    assert so.ucf_field_group_count(h, C.byref(n)) == 0 and n.value == 2
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)
    so.ucf_field_destroy(None)


def group(so, h, P, g, nwell, nloc, nt):
    k0, nt_g, nr_g = C.c_int(), C.c_int(), C.c_int()
    tD, tfac, sv = np.zeros(nt), np.zeros(nt), np.zeros(nt, np.int32)
    rD, cl = np.zeros(nloc * nwell), np.zeros((nloc, nwell), np.int32)
    rc = so.ucf_field_group_from_params(h, C.byref(P), g, C.byref(k0), C.byref(nt_g), tD, sv, C.byref(nr_g), rD, cl, tfac)
    return rc, dict(k0=k0.value, tD=tD[:nt_g.value], sv=sv[:nt_g.value], rD=rD[:nr_g.value], col=cl, tfac=tfac[:nt_g.value])


def restated(wells, loc, t, Tc, Lc):
    """the arithmetic of ucf_field_group as include/ucf.h states it, in numpy (every operation rounded on its own)"""
    out = []
    for t0 in sorted(set(wells[:, 3])):
        members = [j for j in range(len(wells)) if wells[j, 3] == t0]
        k0 = int(np.argmax(t > t0)) if (t > t0).any() else len(t)
        dt = t[k0:] - t0
        dx = loc[:, None, 0] - wells[None, members, 0]
        dy = loc[:, None, 1] - wells[None, members, 1]
        r = np.sqrt(dx * dx + dy * dy) / Lc
        rD = np.unique(r)
        cl = np.full((len(loc), len(wells)), -1, np.int32)
        cl[:, members] = np.searchsorted(rD, r)
        out.append(dict(k0=k0, tD=dt / Tc, rD=rD, col=cl, tfac=t[k0:] / dt))
    return out


@pytest.mark.parametrize("deck,unit", [("neuman74_partpen", 100.0), ("c2_neuman74_fullpen", 100.0), ("c1_theis", 3.0)])
def test_group_is_the_stated_arithmetic(so, oracle, deck, unit):
    dk, _, P = load_deck(deck)
    D = abi.UcfDerived()
    assert so.ucf_nondimensionalise(C.byref(P), C.byref(D)) == 0
    wells = WELLS.copy(); wells[:, :2] *= unit
    loc = LOCATIONS * unit
    rc, h, msg = create(so, wells, loc)
    assert rc == 0, msg
    want = restated(wells, loc, TIMES, D.Tc, D.Lc)
    assert [w["k0"] for w in want] == [0, 2]
    assert len(want[0]["rD"]) == 9 and len(want[1]["rD"]) == 10            # one shared column in group 0
    assert want[0]["col"][0, 0] == want[0]["col"][0, 1]
    for g, w in enumerate(want):
        rc, got = group(so, h, P, g, 4, 5, 6)
        assert rc == 0, so.ucf_last_error()
        assert got["k0"] == w["k0"]
        for key in ("tD", "rD", "tfac", "col"):
            assert got[key].tobytes() == w[key].tobytes(), (deck, g, key, got[key], w[key])
        assert (got["sv"] == oracle.split_vector(list(dk.j0s), w["tD"])).all()
    rc, _ = group(so, h, P, 2, 4, 5, 6)
    assert rc == BAD and b"group 2" in so.ucf_last_error()
    so.ucf_field_destroy(h)


def test_group_refuses_what_cannot_be_launched(so):
    _, _, P = load_deck("neuman74_partpen")
    # a location inside the bore of well 1 (rw = 0.3333)
    loc = np.array([[50.0, 0.0], [200.1, 0.2]])
    rc, h, _ = create(so, WELLS * [100.0, 100.0, 1.0, 1.0], loc)
    assert rc == 0
    rc, _ = group(so, h, P, 0, 4, 2, 6)
    msg = so.ucf_last_error()
    assert rc == BAD and b"location 1" in msg and b"well 1" in msg, msg
    rc, _ = group(so, h, P, 1, 4, 2, 6)                               # the wells of the other group are far away
    assert rc == 0
    so.ucf_field_destroy(h)
    # 70000 times x 40000 distinct distances: more than 2^31 - 1 grid points
    loc = np.stack([np.linspace(10.0, 5000.0, 40000), np.zeros(40000)], axis=1)
    rc, h, _ = create(so, [[0.0, 0.0, 1.0, 0.0]], loc, np.linspace(1.0, 1000.0, 70000))
    assert rc == 0
    rc, _ = group(so, h, P, 0, 1, 40000, 70000)
    assert rc == BAD and b"2^31-1" in so.ucf_last_error(), so.ucf_last_error()
    # a parameter set that the plan builder refuses keeps its own status
    _, _, Pbad = load_deck("neuman74_partpen")
    Pbad.b = -1.0
    rc, _ = group(so, h, Pbad, 0, 1, 40000, 70000)
    assert rc == -3
    so.ucf_field_destroy(h)


def test_drawdown_validates_before_it_asks_for_a_device(so):
    import torch
    rc, h, _ = create(so)
    assert rc == 0
    s, ds = np.zeros((6, 5, 2)), np.zeros((6, 5, 2))
    z = np.array([145.7, 100.0])
    assert so.ucf_field_drawdown(None, None, 2, z, 0, s, ds, None) == BAD and b"field" in so.ucf_last_error()
    assert so.ucf_field_drawdown(h, None, 0, z, 0, s, ds, None) == BAD and b"nz" in so.ucf_last_error()
    assert so.ucf_field_drawdown(h, None, 2, np.array([145.7, np.nan]), 0, s, ds, None) == BAD and b"z[1]" in so.ucf_last_error()
    # every argument that can be checked without a plan is in order: a plan cannot exist without a device, so that is the answer
    rc = so.ucf_field_drawdown(h, None, 2, z, 0, s, ds, None)
    if torch.cuda.is_available():
        assert rc == BAD and b"plan" in so.ucf_last_error()
    else:
        assert rc == NO_DEVICE and b"no CPU fallback" in so.ucf_last_error()
    assert so.ucf_field_alloc_count(h) == 0
    so.ucf_field_destroy(h)


def images(so, wells, a, b, c, kind):
    wells = np.atleast_2d(np.asarray(wells, float))
    n = len(wells)
    out = [np.zeros(2 * n) for _ in range(4)]
    rc = so.ucf_field_images(n, col(wells, 0), col(wells, 1), col(wells, 2), col(wells, 3), a, b, c, kind, *out)
    return rc, np.stack(out, axis=1)


def test_images(so):
    wells = np.array([[0.0, 0.0, 1.0, 0.0], [0.75, -3.0, 0.6, 2.5], [5.5, 1.25, -0.5, 7.0]])
    # x = 2 and y = -1.5: exact mirror coordinates; signs for both kinds; t0 copied
    for kind, sign in ((0, 1.0), (1, -1.0)):
        rc, o = images(so, wells, 1.0, 0.0, 2.0, kind)
        assert rc == 0
        assert np.array_equal(o[:3], wells)
        assert np.array_equal(o[3:, 0], 4.0 - wells[:, 0]) and np.array_equal(o[3:, 1], wells[:, 1])
        assert np.array_equal(o[3:, 2], sign * wells[:, 2]) and np.array_equal(o[3:, 3], wells[:, 3])
        rc, o = images(so, wells, 0.0, 1.0, -1.5, kind)
        assert rc == 0
        assert np.array_equal(o[3:, 0], wells[:, 0]) and np.array_equal(o[3:, 1], -3.0 - wells[:, 1])
        assert np.array_equal(o[3:, 2], sign * wells[:, 2]) and np.array_equal(o[3:, 3], wells[:, 3])
    # a skew line: within 4 u (|x| + |y| + |c|) of the exact mirror point (rational arithmetic)
    a, b, c = 0.6, 0.8, 1.3
    rc, o = images(so, wells, a, b, c, 0)
    assert rc == 0
    A, B, Cc = Fraction(a), Fraction(b), Fraction(c)
    for j, (x, y) in enumerate(wells[:, :2]):
        d = (A * Fraction(x) + B * Fraction(y) - Cc) / (A * A + B * B)
        mx, my = Fraction(x) - 2 * A * d, Fraction(y) - 2 * B * d
        tol = 4 * U * (abs(x) + abs(y) + abs(c))
        assert abs(Fraction(o[3 + j, 0]) - mx) <= tol and abs(Fraction(o[3 + j, 1]) - my) <= tol, (j, o[3 + j])
    # refusals
    rc, _ = images(so, wells, 0.0, 0.0, 1.0, 0)
    assert rc == BAD and b"a = b = 0" in so.ucf_last_error()
    rc, _ = images(so, [[2.0, 7.0, 1.0, 0.0]], 1.0, 0.0, 2.0, 1)
    assert rc == BAD and b"well 0" in so.ucf_last_error()
    rc, _ = images(so, wells, 1.0, 0.0, 2.0, 2)
    assert rc == BAD and b"kind" in so.ucf_last_error()


def test_python_front_end_without_a_gpu():
    from unconfined_amd import WellField, images as py_images
    w = py_images([(0.0, 0.0, 1.0, 0.0)], (1.0, 0.0, 2.0), "constant_head")
    assert w.tolist() == [[0.0, 0.0, 1.0, 0.0], [4.0, 0.0, -1.0, 0.0]]
    _, _, P = load_deck("c1_theis")
    f = WellField(w, [(2.0, 0.0), (2.0, 3.0), (1.0, 0.0)], [1.0, 10.0])
    (g,) = f.groups(P)
    # both locations on the line are equidistant from the well and its image: one column each
    assert g["k0"] == 0 and (g["col"][0] == g["col"][0, 0]).all() and (g["col"][1] == g["col"][1, 0]).all()
    assert g["col"][2, 0] != g["col"][2, 1] and len(g["rD"]) == 4
    assert f.alloc_count() == 0
    with pytest.raises(ucflib.UcfError) as e:
        WellField(w, [(2.0, 0.0)], [1.0, 1.0])
    assert e.value.status == BAD and "t[1]" in e.value.message
    f.close()
