"""Which kernels a call launches, name for name and in order, against the commit before the launch plan
(tests/golden/launch_names_parent.json, recorded there by tools/gen_launch_names_fixture.py).

plan_transform (unconfined_amd/csrc/ucf_launch_plan.h) decides the instantiations and launch_transform_ only maps its plan
onto template arguments; the names it passes to ucf_tm_mark are built from those template arguments.  UCF_TRACE_LAUNCHES=1
prints every one of them on stderr ("... next: <name>").  One fresh child process per environment setting (the library
reads its environment once) runs every case below -- 12 decks x 2 flavours x 1, 2, 3 depths x (a 128 x 2 grid: lane = time;
a 4 x 3 grid and a 40-point list: lane = Laplace sample; a 256-point list: lane = point), a plan with 2M+1 > 64 (chunked
samples) and two parameter batches -- with a marker line between the cases, and the lists must be the recorded ones.
"""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_names_parent.json")

SETTINGS = ["", "UCF_NZC2=0", "UCF_NOFOLD=0", "UCF_FOLD_WAVES_RT=4", "UCF_FOLD_WAVES_RT=6", "UCF_UNFOLD_WAVES_RT=3", "UCF_FINISH_PART=32",
            "UCF_PERSIST=0", "UCF_NSPLIT=8", "UCF_TAIL_LSPLIT=0", "UCF_BATCH_LAYOUT=0"]

CHILD = r"""
import os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from golden_util import load_deck
from unconfined_amd import engine
from unconfined_amd.abi import params_from_deck

DECKS = ["c1_theis", "hantush_lay1", "hantush_lay2", "hantush_lay3", "c2_neuman74_fullpen", "neuman74_partpen", "c3_moench",
         "c4_malama_partpen", "mishra_malama", "mishra_fd30", "hstorage_fullpen_lay1", "hstorage_partpen_lay2"]
DEPTHS = {1: [0.91], 2: [0.3, 0.91], 3: [0.2, 0.6, 0.97]}
MODES = ("faithful", "fast")

def case(name):
    sys.stderr.write("[case] %s\n" % name); sys.stderr.flush()

def grid(plan, nt, nr, zD, zl):
    tD = 10.0 ** np.linspace(-1.0, 3.0, nt)
    plan.drawdown_grid(tD, plan.split_vector(tD), 10.0 ** np.linspace(-1.0, 0.9, nr), zD, zl)

def points(plan, n, zD, zl):
    tD = 10.0 ** np.linspace(-1.0, 3.0, n)
    rD = 10.0 ** np.linspace(-1.0, 0.9, 7)[np.arange(n) % 7]
    plan.drawdown(tD, rD, plan.split_vector(tD), zD, zl)

for name in DECKS:
    dk, ts, P = load_deck(name)
    for mode in MODES:
        plan = engine.Plan(P, mode=mode)
        for nz, z in DEPTHS.items():
            zD = np.array(z); zl = plan.zlay(zD)
            tag = "%s/%s/nz%d/" % (name, mode, nz)
            case(tag + "grid128x2"); grid(plan, 128, 2, zD, zl)
            case(tag + "grid4x3"); grid(plan, 4, 3, zD, zl)
            case(tag + "list256"); points(plan, 256, zD, zl)
            case(tag + "list40"); points(plan, 40, zD, zl)
        plan.close()
# more Laplace samples than lanes: (point, 64-sample chunk) work items
dk, ts, P = load_deck("neuman74_partpen")
for mode in MODES:
    plan = engine.Plan(params_from_deck(dk.replace(M=40)), mode=mode)
    for nz, z in DEPTHS.items():
        zD = np.array(z); zl = plan.zlay(zD)
        case("neuman74_partpen_M40/%s/nz%d/list8" % (mode, nz)); points(plan, 8, zD, zl)
    plan.close()
# parameter batches: 4 sets x 64 points
for name in ("hantush_lay1", "neuman74_partpen"):
    dk, ts, P = load_deck(name)
    for mode in MODES:
        plans = [engine.Plan(params_from_deck(dk.replace(Kr=dk.Kr * (0.6 + 0.2 * i), kappa=dk.kappa * (0.5 + 0.2 * i))), mode=mode) for i in range(4)]
        t = 10.0 ** np.linspace(-1.0, 3.0, 64)
        r = np.array([0.3, 1.0, 2.5, 6.0])[np.arange(64) % 4] * dk.b
        for nz, z in DEPTHS.items():
            case("%s/%s/nz%d/multi4x64" % (name, mode, nz)); engine.drawdown_multi(plans, t, r, np.array(z) * dk.b)
        for p in plans: p.close()
case("end")
"""

_ABORTED = []


def run_setting(setting, tmpdir):
    """{case: [kernel names in launch order]} of a fresh child with `setting` (NAME=VALUE or "") in its environment"""
    script = os.path.join(str(tmpdir), "launch_names_child.py")
    with open(script, "w") as f:
        f.write(CHILD)
    env = dict(os.environ, UCF_TRACE_LAUNCHES="1")
    for s in SETTINGS:
        env.pop(s.split("=")[0], None)
    if setting:
        k, v = setting.split("=")
        env[k] = v
    r = subprocess.run([sys.executable, script, ROOT], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        if r.returncode != 1:       # not a Python exception: the device may be in trouble, start nothing more on it
            _ABORTED.append(setting)
        raise RuntimeError(f"child of setting {setting!r} ended with {r.returncode}:\n{r.stderr[-3000:]}")
    cases, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:]
            assert cur not in cases, cur
            cases[cur] = []
            continue
        m = re.search(r"next: (.*)$", line)
        if m and line.startswith("[ucf] stream"):
            assert line.startswith("[ucf] stream clean;"), line
            cases[cur].append(m.group(1))
    assert cases.pop("end") == []
    return cases


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    names = fx["names"]
    return {s: {c: [names[i] for i in idx] for c, idx in cases.items()} for s, cases in fx["settings"].items()}


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=[s or "none" for s in SETTINGS])
def test_same_kernels_in_the_same_order_as_before_the_launch_plan(setting, recorded, tmp_path):
    assert not _ABORTED, f"a child process died ({_ABORTED}): nothing more is started on the device"
    assert sorted(recorded) == sorted(SETTINGS)
    want = recorded[setting]
    got = run_setting(setting, tmp_path)
    assert sorted(got) == sorted(want)
    assert len(want) == 12 * 2 * 3 * 4 + 2 * 3 + 2 * 2 * 3
    diff = {c: (want[c], got[c]) for c in want if got[c] != want[c]}
    assert not diff, (len(diff), sorted(diff.items())[:3])
    assert all(len(v) > 0 for v in got.values())
