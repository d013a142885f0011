"""Measurement of ucf_fit_evaluate on a field fit (ucf_fit_create_field); recorded in DESIGN.md, not gated.

The problem is made up here, in the shape of an interference test beside a river: three production wells that start at
t = 0, 30 and 300, each with its constant-head image in the line x = 250 (six pumping entries), and the observation
network of tools/bench_fit_network.py placed around them -- 20 wells with 60 times each, 16 piezometers and 4 screened wells
of 5 depths -- deck neuman74_partpen, free = Kr, kappa, Ss, Sy, 64 parameter sets = 576 plans.  Every (observation well,
pumping well) pair is a virtual well of its own here, so the fit launches about six times the points of the network alone;
short virtual wells are padded to blocks of 64 points, which `launched` shows.

    python tools/bench_fit_field.py [OUT.json] [--sets N] [--reps N]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from golden_util import load_deck                       # noqa: E402
from bench_fit_network import DLOG, FREE, NT, arg, network   # noqa: E402
from unconfined_amd import engine, field as ufield, fit as ufit   # noqa: E402


def interference_test():
    """pumping wells [(x, y, q, t0)], observation wells [(x, y, z)], and per observation t, well, iz"""
    real = [(0.0, 0.0, 1.0, 0.0), (-120.0, 80.0, 0.7, 30.0), (60.0, -150.0, 0.5, 300.0)]
    pump = ufield.images(real, line=(1.0, 0.0, 250.0), kind="constant_head")
    wells, t, well, iz = network()
    ang = np.random.default_rng(21).uniform(0.5 * np.pi, 1.5 * np.pi, len(wells))      # on the land side of the river
    obs_wells = [(r * np.cos(a), r * np.sin(a), z) for (r, z), a in zip(wells, ang)]
    return pump, obs_wells, t, well, iz


def main():
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
    nsets, reps = arg("--sets", 64), arg("--reps", 5)
    _, _, P = load_deck("neuman74_partpen")
    pump, obs_wells, t, well, iz = interference_test()
    theta_star = np.array([getattr(P, n) for n in FREE])
    theta = theta_star * np.exp(np.random.default_rng(5).uniform(np.log(0.7), np.log(1.4), (nsets, len(FREE))))
    f = ufit.Fit.field(P, FREE, pump, obs_wells, t, well, iz, np.ones(len(t)))
    launched, dense = f.eval_counts()
    terms = ufit.field_terms(P, pump, obs_wells, t, well)

    def timed():                                         # evaluate ends with its streams drained and the sums on the host
        t0 = time.perf_counter()
        o = f.evaluate(theta, DLOG)
        return time.perf_counter() - t0, o

    _, o = timed()                                       # warm-ups, discarded
    timed()
    ms = [1e3 * timed()[0] for _ in range(reps)]
    rep = {"build_id": engine.build_id(),
           "what": f"ucf_fit_evaluate on a field fit, {nsets} sets x 4 parameters = {nsets * 9} plans, deck neuman74_partpen, 6 pumping "
                   f"entries (3 wells + constant-head images, starts 0 / 30 / 300), 20 observation wells x {NT} times; two warm-ups, then "
                   f"{reps} calls, wall clock [ms] around evaluate; recorded, not gated",
           "launched": launched, "dense": dense, "virtual_wells": int(len(terms["virt_well"])), "terms": int(len(terms["term_t"])),
           "observations": int(len(t)), "evaluate_ms": {"median": float(np.median(ms)), "min": min(ms), "max": max(ms), "all": ms},
           "nbad": int(o["nbad"].sum())}
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(rep, fh, indent=1, sort_keys=True)
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
