"""ucf_fit_objective on the GPU, on the fixtures of the fit tests and with their own parameter sets: the simulated values lie within
the per-value gate of tests/test_gpu_fit.py of the oracle, phi is bit for bit the documented fixed-order sum over the returned
values (lane l takes observations l, l + 256, ...; the butterfly; the four waves: reduce_lanes of tests/fit_reduce_restate.py),
nbad is 0 -- on a plain, a network and a field fit, and jointly with derivative data.  One test runs the whole chain, objective
-> likelihood weights -> weighted ensemble, and asserts structure only."""
import os

import numpy as np
import pytest

import test_gpu_fit_field as tfield
import test_gpu_fit_network as tnet
from fit_reduce_restate import LANES, reduce_lanes
from golden_util import GOLD
from test_gpu_fit import PROBLEMS, gate, problem
from test_gpu_fit_deriv import make, references

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ufit():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from unconfined_amd import fit
    return fit


def phi_restated(sim, obs, w, simd=None, dobs=None, wd=None):
    """(phi, phi_d) of one parameter set from its simulated values, in the order of sums that include/ucf.h states with
    ucf_debug_fit_reduce: wr = w (obs - sim); phi += wr wr; then, where wd > 0, wrd = wd (dobs - simd); phi += wrd wrd; phi_d += wrd wrd"""
    acc = np.zeros((2, LANES))
    for i0 in range(0, len(obs), LANES):
        sl = slice(i0, min(i0 + LANES, len(obs)))
        n = sl.stop - sl.start
        ok = np.isfinite(sim[sl])                       # the observation counts ...
        if simd is not None:
            ok = ok & ((wd[sl] == 0.0) | np.isfinite(simd[sl]))
        wr = w[sl] * (obs[sl] - sim[sl])
        acc[0, :n] = np.where(ok, acc[0, :n] + wr * wr, acc[0, :n])
        if simd is not None:
            ok = ok & (wd[sl] > 0.0)                    # ... and has a derivative datum
            with np.errstate(invalid="ignore"):
                wrd = wd[sl] * (dobs[sl] - simd[sl])
            acc[0, :n] = np.where(ok, acc[0, :n] + wrd * wrd, acc[0, :n])
            acc[1, :n] = np.where(ok, acc[1, :n] + wrd * wrd, acc[1, :n])
    return reduce_lanes(acc, "documented")


def check(f, thetas, obs, ref, bound, what):
    """one objective call with sim: the two statements, and nbad = 0; a repeated call allocates nothing and gives the same bytes"""
    out = f.objective(thetas, sim=True)
    n0 = f.alloc_count()
    again = f.objective(thetas, sim=True)
    assert f.alloc_count() == n0 and sorted(out) == sorted(again) == ["nbad", "phi", "sim"]
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
    assert out["sim"].shape == ref.shape and (out["nbad"] == 0).all()
    err = np.abs(out["sim"] - ref)
    print(f"[objective {what}] worst |sim - oracle| / b = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), (what, float((err / bound).max()))
    w = np.ones(len(obs))
    for s in range(len(thetas)):
        assert out["phi"][s].tobytes() == phi_restated(out["sim"][s], obs, w)[0].tobytes(), (what, s)
    # without sim: the same phi and nbad
    bare = f.objective(thetas)
    assert sorted(bare) == ["nbad", "phi"] and bare["phi"].tobytes() == out["phi"].tobytes() and f.alloc_count() == n0
    return out


@pytest.mark.parametrize("key", PROBLEMS)
def test_plain_fit(ufit, key):
    fx, _, f = problem(ufit, key)
    out = check(f, fx["eval_theta"], fx["obs"], fx["eval_ref"][0][:, 0], gate(fx["eval_ref"][0][:, 0], fx["eval_noise"][0][:, 0]), key)
    # the observations are the oracle's values at theta_star = set 0: its objective is a sum of squared evaluation errors
    assert out["phi"][0] < 1e-12 * out["phi"][1:].min()
    # one set, and many: set s of a larger call is the call of that set alone
    one = f.objective(fx["eval_theta"][1])
    assert one["phi"].tobytes() == out["phi"][1:2].tobytes()
    many = f.objective(np.tile(fx["eval_theta"], (7, 1)))
    assert many["phi"].tobytes() == np.tile(out["phi"], 7).tobytes() and (many["nbad"] == 0).all()


@pytest.mark.parametrize("key", tnet.PROBLEMS)
def test_network_fit(ufit, key):
    fx, _, f, ref, bound = tnet.problem(ufit, key)
    check(f, fx["eval_theta"], fx["obs"], ref[:, 0], bound[:, 0], f"network {key}")


def test_field_fit(ufit):
    fx, _, f, ref, bound = tfield.problem(ufit, "theis")
    check(f, fx["eval_theta"], fx["obs"], ref[:, 0], bound[:, 0], "field theis")


def test_joint_with_derivative_data(ufit):
    fx, _, f = make(ufit, "plain", key="neuman74")
    thetas, n = fx["eval_theta"], len(fx["obs"])
    plain = f.objective(thetas, sim=True)
    # phi_d or simd without derivative data is refused
    phi_d = np.zeros(len(thetas))
    rc = f._lib.ucf_fit_objective(f._h, len(thetas), np.ascontiguousarray(thetas).ctypes.data, None, None, None, phi_d.ctypes.data, None)
    assert rc == -11 and b"no derivative data" in f._lib.ucf_last_error()
    wd = 0.7 + 0.4 * np.cos(np.arange(n))
    wd[1::4] = 0.0                                          # every fourth observation has no derivative datum
    f.set_derivative(np.where(wd > 0, fx["dobs"], np.nan), wd)
    out = f.objective(thetas, sim=True)
    n0 = f.alloc_count()
    again = f.objective(thetas, sim=True)
    assert f.alloc_count() == n0 and sorted(out) == ["nbad", "phi", "phi_d", "sim", "simd"]
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k
    assert (out["nbad"] == 0).all() and out["sim"].tobytes() == plain["sim"].tobytes()
    ref, b, dref, bd = references("plain", "neuman74")
    assert (np.abs(out["sim"] - ref[:, 0]) <= b[:, 0]).all() and (np.abs(out["simd"] - dref[:, 0]) <= bd[:, 0]).all()
    w = np.ones(n)
    for s in range(len(thetas)):
        phi, phid = phi_restated(out["sim"][s], fx["obs"], w, out["simd"][s], fx["dobs"], wd)
        assert out["phi"][s].tobytes() == phi.tobytes() and out["phi_d"][s].tobytes() == phid.tobytes(), s
        assert 0.0 <= out["phi_d"][s] <= out["phi"][s] and out["phi"][s] >= plain["phi"][s]
    assert (out["phi_d"][1:] > 0.0).all()
    f.clear_derivative()
    back = f.objective(thetas, sim=True)
    assert sorted(back) == ["nbad", "phi", "sim"] and back["phi"].tobytes() == plain["phi"].tobytes()
    f.close()


def chain_members(fx):
    """16 members whose oracle values the fixture holds: rows of eval_ref as (set, row, step); member 5 is theta_star itself.
    Returns thetas [16][npar] and the oracle's values [16][nobs]"""
    npar = len(fx["free"])
    rows = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    rows += [(0, r, d) for d in (1, 0) for r in range(1, 1 + 2 * npar)]
    rows += [(s, r, 1) for s in (1, 2) for r in range(1, 1 + 2 * npar)]
    rows = rows[:16]
    rows[0], rows[5] = rows[5], rows[0]
    thetas, ref, noise = [], [], []
    for s, r, d in rows:
        th = np.array(fx["eval_theta"][s])
        if r > 0:
            j, dlog = (r - 1) // 2, float(fx["eval_dlogs"][d])
            th[j] = th[j] * (np.exp(dlog) if r & 1 else np.exp(-dlog))
        thetas.append(th)
        ref.append(fx["eval_ref"][d][s][r])
        noise.append(fx["eval_noise"][d][s][r])
    return np.array(thetas), np.array(ref), np.array(noise)


@pytest.mark.parametrize("key", PROBLEMS)
def test_the_whole_chain(ufit, key):
    """members in the +-0.5 box in ln theta around theta_star -> objective -> likelihood weights (s2 = 1) -> weighted ensemble on the
    60-output field of the forecast fixture.  Structure only: the best member is theta_star, which the oracle's own objective
    ranks first by more than the evaluation error can move any member; ess lies in [1, 16]; the weighted median map lies between
    the weighted extremes."""
    from unconfined_amd import WellField, engine, likelihood_weights
    fx, P, f = problem(ufit, key)
    thetas, ref, noise = chain_members(fx)
    assert thetas.shape == (16, f.npar) and (np.abs(np.log(thetas / fx["theta_star"])) <= 0.5).all()
    # the oracle's objective and how far |sim - ref| <= b can move it: sum of (2 |r| b + b b)
    r, b = fx["obs"] - ref, gate(ref, noise)
    phi_or, move = (r * r).sum(axis=1), (2.0 * np.abs(r) * b + b * b).sum(axis=1)
    assert phi_or[5] == 0.0 and (np.delete(phi_or - move, 5) > move[5]).all()
    obj = f.objective(thetas)
    lw = likelihood_weights(obj["phi"], obj["nbad"], s2=1.0)
    assert lw["best"] == 5 and lw["nadmissible"] == 16 and lw["weight"][5] == 1.0 and (lw["weight"] > 0).all()
    ff = np.load(os.path.join(GOLD, f"field_forecast_{str(fx['deck'])}.npz"))
    assert [str(n) for n in ff["free"]] == f.free
    plan = engine.Plan(P, mode="fast")
    field = WellField(ff["wells"], ff["locations"], ff["times"])
    out = field.ensemble(plan, f.free, thetas, ff["z"], quantiles=(0.05, 0.5, 0.95), limits=[0.02], weights=lw["weight"])
    assert out["mean"].size == 60 and 1.0 <= out["ess"] <= 16.0 and 1 <= out["nlaunched"] <= 16
    assert out["nbad"].tolist() == [0, 0] and (out["nfin"] == out["nlaunched"]).all()
    for pre in ("", "d"):
        assert (out[pre + "min"] <= out[pre + "quant"][0]).all() and (out[pre + "quant"][0] <= out[pre + "quant"][1]).all()
        assert (out[pre + "quant"][1] <= out[pre + "quant"][2]).all() and (out[pre + "quant"][2] <= out[pre + "max"]).all()
        assert (out[pre + "min"] <= out[pre + "mean"]).all() and (out[pre + "mean"] <= out[pre + "max"]).all()
    assert ((out["pexc"] >= 0.0) & (out["pexc"] <= 1.0)).all()
    field.close(); plan.close()
