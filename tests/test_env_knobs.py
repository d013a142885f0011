"""The environment knobs of the library (unconfined_amd/csrc/ucf_env.h): names, defaults and parse rules.

A stand-alone program includes only ucf_env.h and calls ucf_env_read with a fake environment (its arguments).  The
expectations below were written from the getenv lambdas that ucf_env.h replaced (each sat beside the code it steered:
launch_transform_, z_chunk, fill_call_params, guarded_malloc, the table / state budgets, batch_layout, ucf_drawdown_multi,
ucf_debug_stages, ucf_tm_mark and the two global initialisers), not from the new reader:

    atoi knobs      e ? atoi(e) : default                       (so "" reads as 0, whatever the default is)
    UCF_GRID_SLOTS  atoi, then <= 0 -> 8192;   UCF_DEBUG_REPS  atoi, then < 1 -> 1
    byte budgets    atoll, then <= 0 -> default
    PERSIST / NZC2 / NOFOLD          !e || *e != '0'            (on unless the value starts with '0'; "" is on)
    GUARD / TRACE_LAUNCHES           e && *e && *e != '0'       (off unless set, non-empty, not starting with '0')
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unconfined_amd", "csrc")

PROGRAM = r"""
#include "ucf_env.h"
#include <stdio.h>
#include <string.h>
static int g_n;
static char** g_kv;      /* NAME=VALUE */
static const char* fake_get(const char* name)
{
    const size_t n = strlen(name);
    for (int i = 0; i < g_n; i++)
        if (!strncmp(g_kv[i], name, n) && g_kv[i][n] == '=') return g_kv[i] + n + 1;
    return NULL;
}
int main(int argc, char** argv)
{
    g_n = argc - 1;
    g_kv = argv + 1;
    const ucf_env e = ucf_env_read(fake_get);
    printf("nsplit %d\ntail_lsplit %d\ntail_items %d\npersist %d\nnzc2 %d\nnofold %d\nfold_waves_rt %d\nunfold_waves_rt %d\n",
           e.nsplit, e.tail_lsplit, e.tail_items, (int)e.persist, (int)e.nzc2, (int)e.nofold, e.fold_waves_rt, e.unfold_waves_rt);
    printf("finish_part %d\ngrid_slots %d\nz_chunk %d\nfast_eta_max %.17g\nguard %d\ntable_bytes %zu\nstate_bytes %zu\n",
           e.finish_part, e.grid_slots, e.z_chunk, e.fast_eta_max, (int)e.guard, e.table_bytes, e.state_bytes);
    printf("batch_layout %d\nmulti_groups %d\ndebug_reps %d\ntrace_launches %d\n", e.batch_layout, e.multi_groups, e.debug_reps,
           (int)e.trace_launches);
    return 0;
}
"""

MiB, GiB = 1 << 20, 1 << 30
# knob -> (field, default with nothing set, [(value, what the replaced lambda gives)])
KNOBS = {
    "UCF_NSPLIT": ("nsplit", 0, [("4", 4), ("8", 8), ("0", 0), ("", 0), ("-3", -3)]),
    "UCF_TAIL_LSPLIT": ("tail_lsplit", -1, [("2", 2), ("0", 0), ("", 0)]),
    "UCF_TAIL_ITEMS": ("tail_items", -1, [("10240", 10240), ("0", 0), ("", 0)]),
    "UCF_PERSIST": ("persist", 1, [("0", 0), ("", 1), ("1", 1), ("01", 0), ("off", 1)]),
    "UCF_NZC2": ("nzc2", 1, [("0", 0), ("", 1), ("1", 1), ("00", 0)]),
    "UCF_NOFOLD": ("nofold", 1, [("0", 0), ("", 1), ("1", 1), ("0x", 0)]),
    "UCF_FOLD_WAVES_RT": ("fold_waves_rt", 0, [("4", 4), ("6", 6), ("", 0)]),
    "UCF_UNFOLD_WAVES_RT": ("unfold_waves_rt", 0, [("3", 3), ("4", 4), ("", 0)]),
    "UCF_FINISH_PART": ("finish_part", 0, [("16", 16), ("32", 32), ("64", 64), ("0", 0), ("", 0)]),
    "UCF_GRID_SLOTS": ("grid_slots", 8192, [("4096", 4096), ("1", 1), ("0", 8192), ("", 8192), ("-5", 8192)]),
    "UCF_Z_CHUNK": ("z_chunk", 0, [("3", 3), ("0", 0), ("", 0), ("-1", -1)]),
    "UCF_FAST_ETA_MAX": ("fast_eta_max", 0.0, [("50.5", 50.5), ("1e2", 100.0), ("0", 0.0), ("", 0.0), ("-2", -2.0)]),
    "UCF_GUARD": ("guard", 0, [("1", 1), ("0", 0), ("", 0), ("yes", 1), ("01", 0)]),
    "UCF_TABLE_BYTES": ("table_bytes", 256 * MiB, [("1048576", MiB), ("0", 256 * MiB), ("", 256 * MiB), ("-1", 256 * MiB)]),
    "UCF_STATE_BYTES": ("state_bytes", 8 * GiB, [("33554432", 32 * MiB), (str(16 * GiB), 16 * GiB), ("0", 8 * GiB), ("", 8 * GiB),
                                                 ("-4096", 8 * GiB)]),
    "UCF_BATCH_LAYOUT": ("batch_layout", 3, [("0", 0), ("3", 3), ("2", 2), ("", 0)]),
    "UCF_MULTI_GROUPS": ("multi_groups", 0, [("3", 3), ("1", 1), ("", 0)]),
    "UCF_DEBUG_REPS": ("debug_reps", 1, [("5", 5), ("1", 1), ("0", 1), ("", 1), ("-2", 1)]),
    "UCF_TRACE_LAUNCHES": ("trace_launches", 0, [("1", 1), ("0", 0), ("", 0), ("on", 1), ("0n", 0)]),
}
DEFAULTS = {field: dflt for field, dflt, _ in KNOBS.values()}


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_knobs")
    src = d / "env_knobs.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "env_knobs")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)

    def read(*settings):
        out = subprocess.run([exe, *settings], capture_output=True, text=True, check=True).stdout
        return {k: float(v) for k, v in (line.split() for line in out.splitlines())}
    return read


def test_nothing_set_gives_the_defaults(reader):
    got = reader()
    assert len(DEFAULTS) == 19 and set(got) == set(DEFAULTS)
    assert got == {k: float(v) for k, v in DEFAULTS.items()}
    # (spelled out: the values the documents quote)
    assert got["grid_slots"] == 8192 and got["table_bytes"] == 268435456 and got["state_bytes"] == 8589934592
    assert got["batch_layout"] == 3 and got["persist"] == got["nzc2"] == got["nofold"] == 1
    assert got["guard"] == got["trace_launches"] == 0 and got["tail_lsplit"] == got["tail_items"] == -1
    assert got["debug_reps"] == 1


def test_every_knob_sets_its_own_field_and_no_other(reader):
    for knob, (field, _, cases) in KNOBS.items():
        for value, want in cases:
            got = reader(f"{knob}={value}")
            expect = dict(DEFAULTS, **{field: want})
            assert got == {k: float(v) for k, v in expect.items()}, (knob, value)


def test_all_knobs_at_once(reader):
    got = reader(*[f"{knob}={cases[0][0]}" for knob, (_, _, cases) in KNOBS.items()])
    assert got == {field: float(cases[0][1]) for field, _, cases in KNOBS.values()}


def test_the_library_reads_its_environment_in_one_place():
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                hits += [(name, i + 1) for i, line in enumerate(f) if "getenv" in line]
    assert len(hits) == 1 and hits[0][0] == "ucf_api.cpp", hits
