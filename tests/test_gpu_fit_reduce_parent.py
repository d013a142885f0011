"""The fit reduction (fit_reduce_kernel of ucf_fit.hip: one body for every observation source, with and without derivative
data), bit for bit against the parent build that had two bodies, six kernel templates and six launchers.

tests/golden/fit_reduce_parent.npz holds what the parent (commit and build id inside the file) gave on an MI355X for the calls
of run_calls below, through the public API unconfined_amd.fit alone; tools/gen_fit_reduce_parent_fixture.py wrote it and this
module replays the same calls on the build under test.  The inputs travel in the fixture, so that both builds see the same
bits.

The other fit fixtures have about 20 observations: only wave 0 of the 256-thread workgroup holds a partial sum that is not
zero, the lane loop never takes a second pass, and there is one workgroup that matters.  Here every problem has 300
observations (> 256 and no multiple of 64: a second pass that fills only part of wave 0, four waves with partial sums) and
every evaluation 2 parameter sets (workgroup 1), all on neuman74_partpen in the fast flavour:

  plain    20 times x 15 radii at 2 depths, observation i at depth i % 2, through the slot list;
  network  the wells A, B and the screened C of fit_deriv_network.npz, 100 times each: count == 1 and count > 1;
  field    the pumping wells of fit_deriv_field.npz (P0, P1 that starts at 20, the image of P0) seen from its wells A and
           screened B, 150 times each: observations of 2 and of 3 terms, tfac > 1 on the terms of P1.

Observations are the parent's own sim_all / simd_all row 0 at theta_star times 1 + 0.01 cos i; weights are some_weights() of
tests/test_gpu_fit_deriv.py (not 1 on either curve, every fourth derivative weight 0 with NaN in dobs there).  Per kind, for
npar = 1 .. len(free) over prefixes of the free list: evaluate(jacobian, sim_all) without derivative data, then with them
(derivative=True); then one lm from two perturbed starts with max_iter = 3 on the largest npar, without and with derivative
data -- its trial points run the NPAR = 0 kernels.  phi, g, A, nbad, phi_d and the lm results are stored in full, J, Jd,
sim_all and simd_all as the SHA-256 of their bytes.

Not covered here: the instantiations with NPAR above the number of free parameters of a problem (plain: 5..8; network and
field: 3..8) are not reached by this fixture, and recorded bits say "as the parent", not "right".  Both gaps are closed by
tests/test_gpu_fit_reduce_edges.py, which launches all 54 instantiations on synthetic data through ucf_debug_fit_reduce and
holds every output bit for bit to the documented arithmetic, and by problem moench8 of tests/test_gpu_fit.py, a real call at
NPAR = 8."""
import hashlib
import os

import numpy as np
import pytest

from golden_util import GOLD, load_deck
from test_gpu_fit_deriv import some_weights, with_gaps
from test_gpu_fit_field import obs_wells_of
from test_gpu_fit_network import wells_of

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLD, "fit_reduce_parent.npz")
KINDS = ("plain", "network", "field")
SOURCE = {"plain": "fit_deriv_neuman74.npz", "network": "fit_deriv_network.npz", "field": "fit_deriv_field.npz"}
NOBS, NSETS, LM_ITER = 300, 2, 3
HASHED = ("J", "Jd", "sim_all", "simd_all")


def geometry(kind):
    """the fixture of tests/test_gpu_fit_deriv.py that gives this kind its deck, free list, wells and parameter sets"""
    fx = np.load(os.path.join(GOLD, SOURCE[kind]))
    return {k: fx[k] for k in fx.files}


def layout(kind):
    """t, place (r of a plain fit, the well otherwise) and iz of the 300 observations"""
    i = np.arange(NOBS)
    if kind == "plain":
        t, r = 10.0 ** np.linspace(-1.0, 4.0, 20), 10.0 ** np.linspace(np.log10(30.0), np.log10(300.0), 15)
        return t[i // 15], r[i % 15], (i % 2).astype(np.int32)
    if kind == "network":
        return (10.0 ** np.linspace(-1.0, 4.0, 100))[i // 3], (i % 3).astype(np.int32), np.where(i % 3 == 2, -1, 0).astype(np.int32)
    return (10.0 ** np.linspace(-1.0, 3.5, 150))[i // 2], (i % 2).astype(np.int32), np.where(i % 2 == 1, -1, 0).astype(np.int32)


def make(ufit, kind, geo, npar, t, place, iz, obs, weight):
    P = load_deck(str(geo["deck"]))[2]
    free = [str(n) for n in geo["free"]][:npar]
    if kind == "plain":
        return ufit.Fit(P, free, t, place, geo["z"], iz, obs, weight=weight)
    if kind == "network":
        return ufit.Fit.network(P, free, wells_of(geo), t, place, iz, obs, weight=weight)
    return ufit.Fit.field(P, free, geo["pump"], obs_wells_of(geo), t, place, iz, obs, weight=weight)


def thetas(geo, npar):
    return np.ascontiguousarray(geo["eval_theta"][:NSETS, :npar])


def starts(geo):
    """two starts off theta_star, parameter j moved by 25 % up or 20 % down in turn"""
    up = np.where(np.arange(len(geo["theta_star"])) % 2 == 0, 1.25, 0.8)
    return np.stack([geo["theta_star"] * up, geo["theta_star"] / up])


def parent_observations(ufit, kind):
    """obs and dobs of the fixture: sim_all and simd_all of row 0 at theta_star from the library that is loaded, x (1 + 0.01 cos i)"""
    geo = geometry(kind)
    t, place, iz = layout(kind)
    npar = len(geo["free"])
    assert np.array_equal(geo["eval_theta"][0], geo["theta_star"])
    f = make(ufit, kind, geo, npar, t, place, iz, np.ones(NOBS), None)
    f.set_derivative(np.ones(NOBS))
    out = f.evaluate(thetas(geo, npar), float(geo["eval_dlog"]), sim_all=True, derivative=True)
    f.close()
    wiggle = 1.0 + 0.01 * np.cos(np.arange(NOBS))
    return out["sim_all"][0, 0] * wiggle, out["simd_all"][0, 0] * wiggle


def run_calls(ufit, kind, t, place, iz, obs, dobs):
    """{name: array} of every call on the library that is loaded; big arrays as the SHA-256 of their bytes"""
    geo = geometry(kind)
    dlog = float(geo["eval_dlog"])
    w, wd = some_weights(NOBS)
    dobs = with_gaps(dobs, wd)
    res = {}

    def keep(tag, out):
        for k, v in out.items():
            res[f"{tag}_{k}"] = np.array(hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()) if k in HASHED else v

    nfree = len(geo["free"])
    for npar in range(1, nfree + 1):
        f = make(ufit, kind, geo, npar, t, place, iz, obs, w)
        keep(f"p{npar}_plain", f.evaluate(thetas(geo, npar), dlog, jacobian=True, sim_all=True))
        if npar == nfree:
            keep("lm_plain", f.lm(starts(geo), max_iter=LM_ITER))
        f.set_derivative(dobs, wd)
        keep(f"p{npar}_joint", f.evaluate(thetas(geo, npar), dlog, jacobian=True, sim_all=True, derivative=True))
        if npar == nfree:
            keep("lm_joint", f.lm(starts(geo), max_iter=LM_ITER))
        f.close()
    return res


def inputs(parent, kind):
    """t, place, iz, obs, dobs as the fixture carries them"""
    return tuple(parent[f"{kind}_in_{k}"] for k in ("t", "place", "iz", "obs", "dobs"))


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


@pytest.fixture(scope="module")
def parent():
    want = np.load(FIXTURE)
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    return want


def test_shapes_reach_every_wave_a_second_pass_and_a_second_block(ufit, parent):
    """what the problems were chosen for, read from the inputs that the fixture carries"""
    assert NOBS > 256 and NOBS % 64 != 0 and NSETS == 2
    w, wd = some_weights(NOBS)
    assert (w > 0).all() and (w != 1).any() and (wd[1::4] == 0).all() and (np.delete(wd, np.arange(1, NOBS, 4)) > 0).all()
    for kind in KINDS:
        t, place, iz, obs, dobs = inputs(parent, kind)
        assert len(t) == len(place) == len(iz) == len(obs) == len(dobs) == NOBS
        for a, b in zip((t, place, iz), layout(kind)):
            assert np.allclose(a, b, rtol=1e-12, atol=0)
        assert np.isfinite(obs).all() and np.isfinite(dobs).all()
    t, r, iz, _, _ = inputs(parent, "plain")
    assert len(set(t)) == 20 and len(set(r)) == 15 and set(iz) == {0, 1}
    t, well, iz, _, _ = inputs(parent, "network")
    count = np.where(iz < 0, geometry("network")["well_nz"][well], 1)
    assert (count == 1).sum() == 200 and (count == 3).sum() == 100
    assert all(len(set(t[well == k])) == 100 for k in range(3))
    t, well, iz, _, _ = inputs(parent, "field")
    geo = geometry("field")
    tm = ufit.field_terms(load_deck(str(geo["deck"]))[2], geo["pump"], obs_wells_of(geo), t, well)
    nterm = np.diff(tm["term_first"])
    tfac = np.repeat(t, nterm) / tm["term_t"]
    assert set(nterm) == {2, 3} and (nterm[iz < 0] == 3).any() and (nterm[iz == 0] == 3).any()
    assert (tfac[tm["term_pump"] == 1] > 1.0).all() and (tfac[tm["term_pump"] != 1] == 1.0).all() and (tm["term_pump"] == 1).any()
    assert all(len(set(t[well == k])) == 150 for k in range(2))


@pytest.mark.parametrize("kind", KINDS)
def test_every_result_has_the_bytes_of_the_parent(ufit, parent, kind):
    got = run_calls(ufit, kind, *inputs(parent, kind))
    names = sorted(n[len(kind) + 5:] for n in parent.files if n.startswith(kind + "_out_"))
    assert names == sorted(got), (names, sorted(got))
    nfree = len(geometry(kind)["free"])
    assert len(names) == nfree * (6 + 9) + 2 * 5
    bad = []
    for n in names:
        a, ref = np.asarray(got[n]), parent[f"{kind}_out_{n}"]
        assert a.shape == ref.shape and a.dtype == ref.dtype, (n, a.shape, ref.shape, a.dtype, ref.dtype)
        if a.tobytes() != ref.tobytes():
            bad.append((n, a.ravel()[:4].tolist(), ref.ravel()[:4].tolist()))
    print(f"[fit reduce parent {kind}] {len(bad)} of {len(names)} results differ from the parent in a bit")
    assert not bad, bad[:6]
    # the content: every observation counted, both curves in the sums, lm asked for trial points
    for npar in range(1, nfree + 1):
        for mode in ("plain", "joint"):
            assert (got[f"p{npar}_{mode}_nbad"] == 0).all() and (got[f"p{npar}_{mode}_phi"] > 0).all()
            assert np.isfinite(got[f"p{npar}_{mode}_A"]).all() and (got[f"p{npar}_{mode}_g"] != 0).any()
        assert (got[f"p{npar}_joint_phi_d"] > 0).all() and (got[f"p{npar}_joint_phi_d"] < got[f"p{npar}_joint_phi"]).all()
        assert (got[f"p{npar}_joint_phi"] > got[f"p{npar}_plain_phi"]).all()
    for mode in ("plain", "joint"):
        assert (got[f"lm_{mode}_iters"] >= 1).all() and np.isfinite(got[f"lm_{mode}_phi"]).all()
