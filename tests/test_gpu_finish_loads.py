"""finish_kernel with an item's state fetched a group of loads at a time: every result bit for bit what the parent build gave.

finish_kernel (the tail of every work item the integrate kernels completed: level sums -> Richardson/Neville, J0-interval
areas -> Wynn-epsilon, the transform to the workspace or straight through de Hoog) used to read the slots of an item's state
one by one, each load waited for before the next was issued.  It now issues them in groups (load_group / pin_group /
stage_group in ucf_device.h): the lane's time and the first four level sums, further level sums in groups of 4 or 8, the
areas of a depth in one group (epsilon table in registers) or in groups of 4 (table in LDS); an index past the end of a
group repeats the last slot of the same run, and the first group is issued before ndone[pt] is known.  No floating-point
operation changed, so h and dh must be the SAME BITS as before, in both flavours.  tests/golden/finish_loads_parent.npz
holds what the parent build (commit and build id inside the file) gave on an MI355X for the calls below;
tools/gen_finish_loads_fixture.py wrote it.

Calls (CALLS; C2 = the deck c2_neuman74_fullpen at the bench's depth zD = 0.9106, 128 times x 4 radii unless said otherwise):
  * c2, c2_faithful: R = 4 level sums and nacc = 10 areas, table in registers, lane = time -- what bench.py times
    (fast: the pass with the unguarded table and the pass over what it deferred; faithful: one pass);
  * r1n1, r2n2, r5n12, r4n13: (R, nacc) = (1, 1), (2, 2), (5, 12) with k = 7 -- the full register table and a second group
    of level sums -- and (4, 13), the first nacc that takes the table in LDS: the edges of the padded groups;
  * nz2, c3_nz2: two depths (piezometer = F; the C3 deck as it stands): 8 level-sum slots, one group of areas per depth;
    nz3: three depths, which a call at R = 4 runs as two launches of 2 and 1 depths (z_chunk); nz3_one_launch: the same under
    UCF_Z_CHUNK=3, 12 slots in one launch; r3_nz3: R = 3, whose three depths (9 slots: 4, then 5 of a group of 8) share a launch;
  * nt120: a partial last wave of the lane = time layout, lanes that are not live; nt70: 70 times fill the lane = time waves
    worse than the Laplace samples do, so the grid runs as the list of its 280 points (lane = point, a partial last tile);
  * list300: 300 points in random order (lane = point); pts5: 5 points (lane = Laplace sample, finish straight into de Hoog);
  * part32, part16 (+ their nz2): UCF_FINISH_PART, the scratch-part paths, in processes of their own;
  * guard: the first grid of GUARD_GRIDS on which the parent build counted all-zero series, early exits or truncated series
    (ucf_stats; the fixture names the grid and holds the counts) -- the unguarded pass defers, the guarded one runs;
  * handover: rD = 0.02 and 0.07 at tD from 1e-4: items that integrate_kernel leaves to point_kernel, which finish_kernel
    must skip AFTER it has issued their loads.
Every call must have run a finish_kernel instantiation of the expected lane layout and table placement: the grid calls say
so through Plan.kernel_times(); a point list and a call of several launch sequences keep no timers, so list300, pts5, nt70
and nz3 run under UCF_TRACE_LAUNCHES=1 and the names are read from the trace."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "finish_loads_parent.npz")
KERNEL = re.compile(r"finish_kernel<(\d), (\d+), (true|false), (\d)>")
C2, C3 = "c2_neuman74_fullpen", "c3_moench"
ZBENCH = 0.9106
KNOBS = ("UCF_FINISH_PART", "UCF_TRACE_LAUNCHES", "UCF_NSPLIT", "UCF_TAIL_LSPLIT", "UCF_TAIL_ITEMS", "UCF_PERSIST", "UCF_Z_CHUNK",
         "UCF_BATCH_LAYOUT")
TD = (-2.0, 4.0, 128)                   # log10 of the first and last time, count
RD = (0.2, 1.5, 4.0, 30.0)
# candidates for `guard`, tried in this order by the fixture tool: (log10 tD range and count, radii)
GUARD_GRIDS = (((-2.0, 4.0, 128), (10.0, 100.0, 300.0, 1000.0)),
               ((-3.0, 5.0, 128), (1.5, 10.0, 30.0, 100.0)),
               ((-4.0, -1.0, 128), (0.2, 0.6, 1.5, 4.0)))
GUARD_COUNTERS = ("wynn_all_zero", "wynn_early_exit", "wynn_truncated")

# tag: (process, deck, flavour, deck overrides, tD, rD, depths [None = zD 0.9106; n = n points from zBot to zTop], kind,
#       expected (layout, table in registers))
PART32, PART16, TRACE, ZCHUNK3 = {"UCF_FINISH_PART": "32"}, {"UCF_FINISH_PART": "16"}, {"UCF_TRACE_LAUNCHES": "1"}, {"UCF_Z_CHUNK": "3"}
CALLS = {
    "c2": ({}, C2, "fast", {}, TD, RD, None, "grid", (1, True)),
    "c2_faithful": ({}, C2, "faithful", {}, TD, RD, None, "grid", (1, True)),
    "r1n1": ({}, C2, "fast", {"R": 1, "nacc": 1}, TD, RD, None, "grid", (1, True)),
    "r2n2": ({}, C2, "fast", {"R": 2, "nacc": 2}, TD, RD, None, "grid", (1, True)),
    "r5n12": ({}, C2, "fast", {"R": 5, "nacc": 12, "k": 7}, TD, RD, None, "grid", (1, True)),
    "r4n13": ({}, C2, "fast", {"nacc": 13}, TD, RD, None, "grid", (1, False)),
    "r4n13_faithful": ({}, C2, "faithful", {"nacc": 13}, TD, RD, None, "grid", (1, False)),
    "nz2": ({}, C2, "fast", {}, TD, RD, 2, "grid", (1, True)),
    "nz3": (TRACE, C2, "fast", {}, TD, RD, 3, "grid", (1, True)),
    "nz3_one_launch": (ZCHUNK3, C2, "fast", {}, TD, RD, 3, "grid", (1, True)),
    "r3_nz3": ({}, C2, "fast", {"R": 3}, TD, RD, 3, "grid", (1, True)),
    "c3_nz2": ({}, C3, "fast", {}, TD, RD, 2, "grid", (1, True)),
    "nt120": ({}, C2, "fast", {}, (-2.0, 4.0, 120), RD, None, "grid", (1, True)),
    "nt70": (TRACE, C2, "fast", {}, (-2.0, 4.0, 70), RD, None, "grid", (3, True)),
    "guard": ({}, C2, "fast", {}, None, None, None, "grid", (1, True)),
    "handover": ({}, C2, "fast", {}, ((-4.0, -3.5, 64), (-1.0, -0.5, 64)), (0.02, 0.07, 0.6, 4.0), None, "grid", (1, True)),
    "list300": (TRACE, C2, "fast", {}, 300, None, None, "list", (3, True)),
    "pts5": (TRACE, C2, "fast", {}, 5, None, None, "list", (0, True)),
    "part32": (PART32, C2, "fast", {}, TD, RD, None, "grid", (1, False)),
    "part32_nz2": (PART32, C2, "fast", {}, TD, RD, 2, "grid", (1, False)),
    "part16": (PART16, C2, "fast", {}, TD, RD, None, "grid", (1, False)),
    "part16_nz2": (PART16, C2, "fast", {}, TD, RD, 2, "grid", (1, False)),
}
PART_OF = {"part32": 32, "part32_nz2": 32, "part16": 16, "part16_nz2": 16}


def times(spec):
    """the times of a grid: one (lo, hi, n) range of log10 tD, or several one after the other"""
    ranges = spec if isinstance(spec[0], tuple) else (spec,)
    return np.concatenate([np.logspace(lo, hi, n) for lo, hi, n in ranges])


def list_points(n):
    """n points in no order: log-uniform times in 1e-2 .. 1e4 and radii in 0.05 .. 30 (fixed seed)"""
    rng = np.random.default_rng(20240611 + n)
    return 10.0 ** rng.uniform(-2.0, 4.0, n), 10.0 ** rng.uniform(np.log10(0.05), np.log10(30.0), n)


# every call of one process; argv: root, out.npz, tags, guard grid index
_CALL_SCRIPT = r"""
import os, sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck
import test_gpu_finish_loads as T
out = {"build_id": np.array(engine.build_id())}
for tag in sys.argv[3].split(","):
    _, deck, flavour, over, tsp, rsp, depths, kind, _ = T.CALLS[tag]
    dk, ts, P = load_deck(deck)
    if depths is not None:
        dk.piezometer, dk.zOrd = False, depths
    for key, val in over.items():
        setattr(dk, key, val)
    pl = engine.Plan(params_from_deck(dk), mode=flavour)
    zD = np.array([T.ZBENCH]) if depths is None else engine.linspace(dk.zBot, dk.zTop, depths) / pl.derived.Lc
    print("[call] " + tag, file=sys.stderr, flush=True)
    if kind == "list":
        tD, rD = T.list_points(tsp)
        h, dh = pl.drawdown(tD, rD, pl.split_vector(tD), zD, pl.zlay(zD))
        names = []
    else:
        if tag == "guard":
            tsp, rsp = T.GUARD_GRIDS[int(sys.argv[4])]
        tD, rD = T.times(tsp), np.array(rsp)
        timed = not os.environ.get("UCF_TRACE_LAUNCHES")
        pl.set_timing(timed)
        r = pl.drawdown_grid(tD, pl.split_vector(tD), rD, zD, pl.zlay(zD), with_stats=(tag == "guard"))
        h, dh = r[0], r[1]
        names = [k[0] for k in pl.kernel_times()] if timed else []
        if tag == "guard":
            out[tag + "_stats"] = np.array([r[2][c] for c in T.GUARD_COUNTERS], np.int64)
    pl.close()
    out[tag + "_h"], out[tag + "_dh"], out[tag + "_kernels"] = h, dh, np.array(names, dtype=str)
np.savez(sys.argv[2], **out)
"""


def run_calls(outdir, guard_grid, tags=None):
    """{tag: (h, dh, kernel names, build id, guard counters or None)} of the calls `tags` (all of CALLS), one child process
    per environment; `guard_grid`: index into GUARD_GRIDS"""
    tags = list(CALLS) if tags is None else list(tags)
    res = {}
    envs = []
    for t in tags:
        if CALLS[t][0] not in envs:
            envs.append(CALLS[t][0])
    for i, env in enumerate(envs):
        mine = [t for t in tags if CALLS[t][0] == env]
        out = os.path.join(str(outdir), f"proc{i}.npz")
        e = {k: v for k, v in os.environ.items() if k not in KNOBS}
        e.update(env)
        p = subprocess.run([sys.executable, "-c", _CALL_SCRIPT, ROOT, out, ",".join(mine), str(guard_grid)], env=e, timeout=600,
                           stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        traced = {}
        cur = None
        for line in p.stderr.split("\n"):
            if line.startswith("[call] "):
                cur = line[7:].strip()
            elif cur and "next: " in line:
                traced.setdefault(cur, []).append(line.split("next: ", 1)[1].strip())
        with np.load(out) as d:
            for t in mine:
                names = [str(k) for k in d[t + "_kernels"]] or traced.get(t, [])
                res[t] = (d[t + "_h"], d[t + "_dh"], names, str(d["build_id"]), d[t + "_stats"] if t + "_stats" in d else None)
    return res


def finish_kernels(names):
    """[(layout, part, table in registers, mode)] of the finish_kernel instantiations among `names`"""
    return [(int(m.group(1)), int(m.group(2)), m.group(3) == "true", int(m.group(4))) for m in map(KERNEL.search, names) if m]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    want = np.load(FIXTURE)
    return want, run_calls(tmp_path_factory.mktemp("finish_loads"), int(want["guard_grid"]))


def test_fixture_names_its_parent_and_a_grid_that_needs_the_guarded_table(results):
    want, got = results
    assert len(str(want["parent_commit"])) == 40 and len(str(want["parent_build_id"])) == 16
    assert set(got) == set(CALLS)
    assert 0 <= int(want["guard_grid"]) < len(GUARD_GRIDS)
    assert want["guard_stats"].shape == (len(GUARD_COUNTERS),) and int(want["guard_stats"].sum()) > 0
    # (counted by integer atomics: the new build must count what the parent counted)
    assert np.array_equal(got["guard"][4], want["guard_stats"]), (got["guard"][4], want["guard_stats"])


@pytest.mark.parametrize("tag", list(CALLS))
def test_finish_kernel_with_grouped_state_loads_keeps_every_bit(results, tag):
    want, got = results
    h, dh, names, _, _ = got[tag]
    fk = finish_kernels(names)
    layout, wreg = CALLS[tag][8]
    flavour = CALLS[tag][2]
    print(tag, fk)
    assert fk, (tag, names)
    assert all(k[0] == layout and k[2] == wreg for k in fk), (tag, fk)
    # fast flavour, table in registers: the unguarded pass, then the guarded one; else one pass
    assert {k[3] for k in fk} == ({1, 2} if flavour == "fast" and wreg else {0}), (tag, fk)
    if tag in PART_OF:
        assert all(k[1] == PART_OF[tag] for k in fk), (tag, fk)
    for name, a in (("h", h), ("dh", dh)):
        ref = want[f"{tag}_{name}"]
        assert a.shape == ref.shape and a.dtype == ref.dtype == np.float64 and a.size > 0
        diff = np.flatnonzero(a.view(np.uint64).ravel() != ref.view(np.uint64).ravel())
        print(f"{tag} {name}: {diff.size} of {a.size} values differ in a bit")
        assert diff.size == 0, (tag, name, diff.size, diff[:8], a.ravel()[diff[:8]], ref.ravel()[diff[:8]])
