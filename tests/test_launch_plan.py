"""The launch plan of the transform stage (unconfined_amd/csrc/ucf_launch_plan.h): which kernel instantiations run, how the
work items are cut, how the shared buffers are laid out -- decided in plain C++, so it is looked at here without a GPU.

A stand-alone program includes only ucf_launch_plan.h, builds a ucf_dev_params and an environment from its arguments, calls
plan_transform and prints the plan.  The expectations were written from the launch_transform_ that the header replaced (the
macro cascade UCF_LAUNCH_I4 <- I3 <- UNF_ <- UNF / FOLD <- switch (fam), the cuts above it and the finish choice below
it), not from the new function.  Sizes in its terms: an LDS complex is 16 B, a wave 64 lanes, UCF_IWPB = 4 waves share the
sin/cos table of 384 entries; the defaults below are R = 4, nacc = 8, one depth, 2M+1 = 21.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unconfined_amd", "csrc")
NEW_HEADER = "ucf_launch_plan.h"

PROGRAM = r"""
#include "ucf_launch_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
static int g_n;
static char** g_kv;      /* name=value: UCF_* are the environment, the rest the call */
static const char* fake_get(const char* name)
{
    const size_t n = strlen(name);
    for (int i = 0; i < g_n; i++)
        if (!strncmp(g_kv[i], name, n) && g_kv[i][n] == '=') return g_kv[i] + n + 1;
    return NULL;
}
static int arg(const char* name, int dflt) { const char* v = fake_get(name); return v ? atoi(v) : dflt; }
int main(int argc, char** argv)
{
    g_n = argc - 1;
    g_kv = argv + 1;
    const ucf_env env = ucf_env_read(fake_get);
    ucf_dev_params dp;
    memset(&dp, 0, sizeof(dp));
    dp.model = arg("model", 3); dp.MNtype = arg("MNtype", 0); dp.order = arg("order", 0);
    dp.R = arg("R", 4); dp.nacc = arg("nacc", 8); dp.nz = arg("nz", 1); dp.np = arg("np", 21); dp.M = (dp.np - 1) / 2;
    dp.N = arg("N", 100); dp.ngl = arg("ngl", 10);
    dp.fold_dD = arg("fold_dD", 0); dp.fold_lD1 = arg("fold_lD1", 0); dp.any_fold = arg("any_fold", 0);
    dp.any_lay1 = arg("any_lay1", 0); dp.any_lay3 = arg("any_lay3", 0);
    const bool fast = arg("fast", 1) != 0;
    const int nwork = arg("nwork", 1000);
    printf("UNSUPPORTED %d\nMAX_NZ %d\n", (int)UCF_ERR_UNSUPPORTED, (int)UCF_MAX_NZ);
    const ucf_transform_buffers b = transform_buffers(dp, fast, (size_t)nwork, (size_t)arg("lt_rows", 0));
    printf("b_ndone %zu\nb_todo %zu\nb_defer %zu\nb_wcount %zu\nb_ints %zu\nb_item %zu\nb_ltab %zu\nb_state %zu\n", b.ndone, b.todo, b.defer, b.wcount,
           b.ints, b.state_item_bytes, b.ltab, b.state_bytes);
    printf("family %d\nsplit_kind %d\npoint_lds_fresh %zu\nsamples_lds %zu\n", family_of(dp), split_kind(dp, fast), point_lds_bytes(dp, fast), samples_lds_bytes(dp, fast));
    ucf_transform_plan P;
    memset(&P, 0xff, sizeof(P));
    const int rc = plan_transform(dp, env, fast, arg("layout", 1), arg("multi", 0) != 0, nwork, arg("per_point", 0), arg("nr", 1), arg("nt", 64), &P);
    printf("rc %d\n", rc);
    if (rc) return 0;
    printf("fam %d\nkind %d\npoint_lds %zu\npoint_grid %u\nglobal_areas %d\n", P.fam, P.kind, P.point_lds, P.point_grid, (int)P.global_areas);
    printf("lsplit %d\nltail %d\nntail %d\nnhead %d\nnworkw %lld\npersist %d\nintegrate_grid %u\nnrows %d\nlaptime_grid %u\n", P.lsplit, P.ltail, P.ntail,
           P.nhead, P.nworkw, (int)P.persist, P.integrate_grid, P.nrows, P.laptime_grid);
    printf("waves %d\nfold %d\nlay3 %d\nnzc %d\nlay1 %d\nnofold %d\nintegrate_lds %zu\ngeneric_lds %zu\n", P.ik.waves, (int)P.ik.fold, (int)P.ik.lay3, P.ik.nzc,
           (int)P.ik.lay1, (int)P.ik.nofold, P.integrate_lds, P.generic_lds);
    printf("part %d\nwreg %d\ntwo_pass %d\nfinish_lds %zu\nfinish_grid2 %u\n", P.fin.part, (int)P.fin.wreg, (int)P.fin.two_pass, P.finish_lds, P.finish_grid2);
    printf("p_todo %zu\np_defer %zu\np_wcount %zu\np_ints %zu\np_item %zu\np_ltab %zu\np_state %zu\n", P.buf.todo, P.buf.defer, P.buf.wcount, P.buf.ints,
           P.buf.state_item_bytes, P.buf.ltab, P.buf.state_bytes);
    return 0;
}
"""

SC = 384 * 16          # the sin/cos table of a workgroup of integrate_kernel


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    src = d / "launch_plan.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "launch_plan")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)

    def run(**kw):
        out = subprocess.run([exe, *[f"{k}={v}" for k, v in kw.items()]], capture_output=True, text=True, check=True).stdout
        return {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    return run


def choice(p):
    return {k: p[k] for k in ("waves", "fold", "lay3", "nzc", "lay1", "nofold")}


# model -> family (family_of): 0 Theis, 1 Hantush, 2 -> 5 Hantush with storage, 3 / 4 / 5 -> 2 water table,
# 6 -> 3 (MNtype 1) or 4 (MNtype 2, finite differences)
FAMILY = {0: dict(model=0), 1: dict(model=1), 2: dict(model=3), 3: dict(model=6, MNtype=1), 4: dict(model=6, MNtype=2, order=8),
          5: dict(model=2)}
FOLDED2 = dict(model=3, fold_dD=1, fold_lD1=1, any_fold=1, layout=1)
FOLD = dict(waves=5, fold=1, lay3=0, nzc=1, lay1=1, nofold=0)
UNFOLDED2 = dict(model=4, any_fold=0, layout=1)


def test_families(plan):
    assert [plan(model=m)["family"] for m in range(6)] == [0, 1, 5, 2, 2, 2]
    assert plan(model=6, MNtype=1)["family"] == 3 and plan(model=6, MNtype=2)["family"] == 4
    for bad in (dict(model=6, MNtype=0), dict(model=7), dict(model=-1)):
        p = plan(**bad)
        assert p["family"] == -1 and p["rc"] == p["UNSUPPORTED"]
    for f, kw in FAMILY.items():
        assert plan(**kw)["fam"] == f and plan(**kw)["kind"] == 1


def test_folded_water_table_choice(plan):
    p = plan(**FOLDED2)
    assert p["rc"] == 0 and p["fam"] == 2 and choice(p) == FOLD
    assert p["integrate_lds"] == 4 * (4 * 64 * 16) + SC           # NZC: R level sums, no running area
    assert choice(plan(**FOLDED2, UCF_FOLD_WAVES_RT=4)) == dict(FOLD, waves=4)
    assert choice(plan(**FOLDED2, UCF_FOLD_WAVES_RT=6)) == dict(FOLD, waves=6)
    assert choice(plan(**FOLDED2, UCF_FOLD_WAVES_RT=5)) == FOLD
    p = plan(**FOLDED2, nz=2)
    assert p["nzc"] == 2 and p["fold"] == 1 and p["integrate_lds"] == 4 * (4 * 2 * 64 * 16) + SC
    # (two depths: 4 * 2 KB + 1.5 KB per wave, 20 of them are more than 160 KB: four waves per SIMD)
    assert p["waves"] == 4
    p = plan(**FOLDED2, nz=2, UCF_NZC2=0)
    assert p["nzc"] == 0 and p["integrate_lds"] == 4 * (5 * 2 * 64 * 16) + SC
    assert plan(**FOLDED2, nz=3)["nzc"] == 0
    # the sixth wave only where 24 waves' footprints fit: R = 6 -> 6 KB + 1.5 KB per wave
    assert plan(**FOLDED2, R=6, UCF_FOLD_WAVES_RT=6)["waves"] == 5      # 24 x 7.5 KB = 180 KB do not fit, 20 do: the built-in five
    assert plan(**FOLDED2, R=6)["waves"] == 5 and plan(**FOLDED2, R=7)["waves"] == 4      # 20 x 8.5 KB = 170 KB
    for layout in (0, 2, 3):
        for nz in (1, 2, 3):
            p = plan(**dict(FOLDED2, layout=layout), nz=nz, per_point=1)
            assert p["nzc"] == (2 if (layout == 3 and nz == 2) else 0), (layout, nz)
    for nz in (1, 2, 3):
        assert plan(**dict(FOLDED2, layout=0), nz=nz, per_point=1)["nzc"] == 0
        assert plan(**dict(UNFOLDED2, layout=0), nz=nz, per_point=1)["nzc"] == 0


def test_unfolded_water_table_choice(plan):
    unf = dict(waves=4, fold=0, lay3=0, nzc=0, lay1=0, nofold=1)
    assert choice(plan(**UNFOLDED2)) == unf
    assert choice(plan(**UNFOLDED2, UCF_NOFOLD=0)) == dict(unf, nofold=0)
    assert choice(plan(**dict(UNFOLDED2, any_fold=1))) == dict(unf, nofold=0)
    assert choice(plan(**dict(UNFOLDED2, fold_dD=1, any_fold=1))) == dict(unf, nofold=0)      # one term folds: the general one
    assert choice(plan(**UNFOLDED2, any_lay3=1)) == dict(unf, lay3=1, lay1=1)
    assert choice(plan(**UNFOLDED2, any_lay3=1, any_lay1=1)) == dict(unf, lay3=1, lay1=1)
    assert choice(plan(**UNFOLDED2, any_lay1=1)) == dict(unf, lay3=0, lay1=1)
    assert plan(**UNFOLDED2)["integrate_lds"] == 4 * (5 * 64 * 16) + SC
    # depth counts: two depths in the lane = time / lane = point layouts run NZC = 2 at 4 waves, anything else with >= 2 depths 3 waves
    assert choice(plan(**UNFOLDED2, nz=2)) == dict(unf, nzc=2)
    assert choice(plan(**UNFOLDED2, nz=2, UCF_NZC2=0)) == dict(unf, nzc=0, waves=3)
    assert choice(plan(**UNFOLDED2, nz=3)) == dict(unf, waves=3)
    assert choice(plan(**dict(UNFOLDED2, layout=0), nz=3, per_point=1)) == dict(unf, waves=3)
    assert choice(plan(**dict(UNFOLDED2, layout=0), nz=2, per_point=1)) == dict(unf, waves=3)
    assert choice(plan(**dict(UNFOLDED2, layout=0), nz=3, per_point=1, UCF_UNFOLD_WAVES_RT=4)) == dict(unf, waves=4)
    assert choice(plan(**UNFOLDED2, UCF_UNFOLD_WAVES_RT=3)) == dict(unf, waves=3)


def test_other_families_choice(plan):
    folded = dict(waves=4, fold=1, lay3=0, nzc=0, lay1=1, nofold=0)
    # Theis: six waves while 24 x ((R+1) nz KB + 1.5 KB) <= 160 KB
    assert choice(plan(model=0)) == dict(folded, waves=6)                 # 24 x 6.5 KB = 156 KB
    assert choice(plan(model=0, nz=2, UCF_NZC2=0)) == folded              # 24 x 11.5 KB
    assert choice(plan(model=0, nz=2)) == dict(folded, nzc=2)
    assert choice(plan(model=0, R=5)) == folded                           # 24 x 7.5 KB = 180 KB
    # (the folded form whatever the plan's fold flags say)
    assert choice(plan(model=0, any_lay3=1, any_lay1=1)) == dict(folded, waves=6)
    assert choice(plan(**FAMILY[3])) == folded
    for f in (1, 4, 5):
        assert choice(plan(**FAMILY[f], fold_dD=1, fold_lD1=1, any_fold=1)) == folded, f
        assert choice(plan(**FAMILY[f])) == dict(waves=4, fold=0, lay3=0, nzc=0, lay1=0, nofold=1), f
        assert choice(plan(**FAMILY[f], nz=3, any_lay3=1, any_fold=1)) == dict(waves=4, fold=0, lay3=1, nzc=0, lay1=1, nofold=0), f
        assert choice(plan(**FAMILY[f], nz=2))["nzc"] == 2 and choice(plan(**FAMILY[f], nz=2))["waves"] == 4, f
        assert choice(plan(**FAMILY[f], nz=1))["nzc"] == 0, f


def test_parameter_batches(plan):
    for f in (0, 3, 5):
        for layout in (0, 2, 3):
            p = plan(**FAMILY[f], multi=1, layout=layout, per_point=1)
            assert p["rc"] == p["UNSUPPORTED"] == -10, f
    # no batch runs a folded kernel: every plan of it would have to be fully penetrating
    for f in (1, 2, 4):
        p = plan(**FAMILY[f], fold_dD=1, fold_lD1=1, any_fold=1, multi=1, layout=3, per_point=1)
        assert p["rc"] == 0 and choice(p) == dict(waves=4, fold=0, lay3=0, nzc=0, lay1=0, nofold=0), f
    p = plan(**dict(FOLDED2, layout=3), multi=1, per_point=1, nz=2)
    assert choice(p) == dict(waves=4, fold=0, lay3=0, nzc=2, lay1=0, nofold=0)
    p = plan(**dict(FOLDED2, layout=0), multi=1, per_point=1, nz=2, any_lay1=1)
    assert choice(p) == dict(waves=3, fold=0, lay3=0, nzc=0, lay1=1, nofold=0)


def test_cutting(plan):
    for nacc in (7, 8, 12):
        p = plan(**FOLDED2, nacc=nacc, nwork=27136)
        assert (p["lsplit"], p["ltail"], p["ntail"], p["nhead"]) == (1, 3, 5120, 22016)
        assert p["nworkw"] == (22016 << 1) + (5120 << 3)
        assert p["persist"] == 1 and p["integrate_grid"] == 2048
        p = plan(**FOLDED2, nacc=nacc, nwork=27136, UCF_PERSIST=0)
        assert p["persist"] == 0 and p["integrate_grid"] == ((22016 << 1) + (5120 << 3) + 3) // 4
        p = plan(**FOLDED2, nacc=nacc, nwork=49152)
        assert (p["lsplit"], p["ltail"], p["nhead"]) == (0, 3, 49152 - 5120)
        assert plan(**FOLDED2, nacc=nacc, nwork=49151)["lsplit"] == 1
        p = plan(**FOLDED2, nacc=nacc, nwork=27136, UCF_NSPLIT=8)
        assert (p["lsplit"], p["ltail"], p["nhead"], p["nworkw"]) == (3, 3, 27136, 27136 << 3)
        assert plan(**FOLDED2, nacc=nacc, nwork=49152, UCF_NSPLIT=4)["lsplit"] == 2
        assert plan(**FOLDED2, nacc=nacc, nwork=1000, UCF_NSPLIT=1)["lsplit"] == 0
        p = plan(**FOLDED2, nacc=nacc, nwork=27136, UCF_TAIL_LSPLIT=0)
        assert (p["lsplit"], p["ltail"], p["nhead"], p["nworkw"]) == (1, 1, 27136, 27136 << 1)
        p = plan(**FOLDED2, nacc=nacc, nwork=27136, UCF_TAIL_LSPLIT=2, UCF_TAIL_ITEMS=10240)
        assert (p["ltail"], p["ntail"], p["nhead"]) == (2, 10240, 27136 - 10240)
        assert plan(**FOLDED2, nacc=nacc, nwork=27136, UCF_TAIL_LSPLIT=7)["ltail"] == 3
    # few interval areas: no more parts than nacc + 1 of them
    p = plan(**FOLDED2, nacc=1, nwork=27136)
    assert (p["lsplit"], p["ltail"], p["nhead"]) == (1, 1, 27136)
    p = plan(**FOLDED2, nacc=1, nwork=49152)
    assert (p["lsplit"], p["ltail"], p["nhead"]) == (0, 1, 49152 - 5120)
    p = plan(**FOLDED2, nacc=2, nwork=27136, UCF_NSPLIT=8)
    assert (p["lsplit"], p["ltail"]) == (0, 1)
    p = plan(**FOLDED2, nacc=3, nwork=49152)
    assert (p["lsplit"], p["ltail"]) == (0, 2)
    # a launch smaller than the tail is all tail
    p = plan(**FOLDED2, nwork=3000)
    assert (p["lsplit"], p["ltail"], p["ntail"], p["nhead"], p["nworkw"]) == (1, 3, 3000, 0, 3000 << 3)
    assert p["integrate_grid"] == 2048
    p = plan(**FOLDED2, nwork=100)
    assert p["integrate_grid"] == 200 and p["point_grid"] == 100 and p["finish_grid2"] == 100
    p = plan(**FOLDED2, nwork=27136)
    assert p["point_grid"] == 2048 and p["finish_grid2"] == 12288 and p["global_areas"] == 0
    # 2^31 work units and more: no launch
    assert plan(**FOLDED2, nwork=(1 << 28) - 1, UCF_NSPLIT=8)["nworkw"] == (1 << 31) - 8
    p = plan(**FOLDED2, nwork=1 << 28, UCF_NSPLIT=8)
    assert p["rc"] == p["UNSUPPORTED"]


def test_laptime_rows(plan):
    p = plan(**FOLDED2, nwork=27136, nt=500, nr=7)
    assert p["nrows"] == 500 and p["laptime_grid"] == (500 * 21 + 255) // 256
    assert plan(**dict(FOLDED2, layout=3), nwork=210, nt=640, per_point=1)["nrows"] == 640
    assert plan(**dict(FOLDED2, layout=0), nwork=40, nt=0, per_point=1)["nrows"] == 40
    assert plan(**dict(FOLDED2, layout=0), nwork=12, nt=0, nr=3, per_point=0)["nrows"] == 4
    assert plan(**dict(FOLDED2, layout=0), nwork=13, nt=0, nr=3, per_point=0)["nrows"] == 5
    p = plan(**dict(FOLDED2, layout=2), nwork=24, np=161, per_point=1)          # 3 chunks of 64 samples per point
    assert p["nrows"] == 8 and p["laptime_grid"] == (8 * 161 + 255) // 256


def test_finish(plan):
    for nacc in (1, 8, 12):
        p = plan(**FOLDED2, nacc=nacc)
        assert (p["part"], p["wreg"], p["two_pass"]) == (64, 1, 1)
        assert p["finish_lds"] == (4 * 64 + 4 * 64) * 16
        p = plan(**FOLDED2, nacc=nacc, fast=0)
        assert (p["kind"], p["part"], p["wreg"], p["two_pass"]) == (2, 64, 1, 0)
    # the epsilon table in LDS: max(2 nacc, R) scratch columns; the widest part within 40 KB
    p = plan(**FOLDED2, nacc=13)
    assert (p["part"], p["wreg"], p["two_pass"]) == (64, 0, 0) and p["finish_lds"] == (4 * 64 + 26 * 64) * 16
    p = plan(**FOLDED2, nacc=13, nz=4)          # 16 + 26 KB > 40 KB; 16 + 13 KB
    assert (p["part"], p["wreg"]) == (32, 0) and p["finish_lds"] == (4 * 4 * 64 + 26 * 32) * 16
    p = plan(**FOLDED2, nacc=13, nz=7)          # 28 + 13 KB > 40 KB
    assert (p["part"], p["wreg"]) == (16, 0) and p["finish_lds"] == (4 * 7 * 64 + 26 * 16) * 16
    # in registers the scratch is the Neville column alone
    assert plan(**FOLDED2, nacc=12, nz=9)["part"] == 64              # 36 + 4 KB
    assert plan(**FOLDED2, nacc=12, nz=10)["part"] == 16             # 40 KB of level sums: no part fits, the narrowest
    for part in (16, 32, 64):
        p = plan(**FOLDED2, UCF_FINISH_PART=part)
        assert (p["part"], p["wreg"], p["two_pass"]) == (part, 0, 0)
        assert p["finish_lds"] == (4 * 64 + 16 * part) * 16
    p = plan(**FOLDED2, UCF_FINISH_PART=8)      # not a part width: the 40 KB rule, and the table stays in LDS
    assert (p["part"], p["wreg"]) == (64, 0)


def test_faithful_flavour(plan):
    # reference-order evaluators in integrate_generic_kernel, unless the finite-difference Thomas buffer (2 x order x 1 KB) is > 16 KB
    for f, kw in FAMILY.items():
        p = plan(**kw, fast=0, nwork=10000, layout=0, per_point=1)
        assert (p["kind"], p["fam"]) == (2, f)
        assert p["generic_lds"] == 5 * 64 * 16 + (2 * 8 * 64 * 16 if f == 4 else 0)
        assert p["b_item"] == p["p_item"] == (4 + 1 + 8) * 64 * 16 and p["p_state"] == 10000 * p["p_item"]
    p = plan(**dict(FAMILY[4], order=9), fast=0, nwork=10000, layout=0, per_point=1)
    assert p["kind"] == 0 and p["b_item"] == 0 and p["b_state"] == 0
    # point_kernel does everything: level sums, running area and (while 8 workgroups fit a CU, 20 KB) the interval areas in LDS
    assert p["point_lds"] == ((4 + 1 + 8) * 64 + 16 * 16) * 16 + 2 * 9 * 64 * 16
    assert p["global_areas"] == 0 and p["point_grid"] == 10000
    p = plan(**dict(FAMILY[4], order=9), fast=0, nwork=10000, layout=0, per_point=1, nz=2)
    assert p["point_lds"] == (5 * 2 * 64 + 16 * 16) * 16 + 2 * 9 * 64 * 16
    assert p["global_areas"] == 1 and p["point_grid"] == 8192
    p = plan(**dict(FAMILY[4], order=9), fast=0, nwork=10000, layout=0, per_point=1, nz=2, UCF_GRID_SLOTS=512)
    assert p["point_grid"] == 512
    assert plan(**dict(FAMILY[4], order=9), fast=0, nwork=100, layout=0, per_point=1, nz=2)["point_grid"] == 100
    assert plan(**dict(FAMILY[4], order=8), fast=0)["kind"] == 2
    assert plan(**dict(FAMILY[4], order=80), fast=1)["kind"] == 1
    # samples_kernel
    assert plan(**FAMILY[4], fast=0)["samples_lds"] == 2 * 8 * 64 * 16 and plan(**FAMILY[2], fast=0)["samples_lds"] == 16
    assert plan(**FAMILY[4], fast=1)["samples_lds"] == SC
    # more LDS than a CU has: no kernel
    p = plan(**FAMILY[2], fast=0, R=16, nz=32)
    assert p["rc"] == p["UNSUPPORTED"]


def test_point_kernel_resumes_with_level_sums_only(plan):
    p = plan(**FOLDED2, nz=2)
    assert p["point_lds"] == (5 * 2 * 64 + 16 * 16) * 16
    assert p["point_lds_fresh"] == (5 * 2 * 64 + 16 * 16) * 16            # 2 depths: the areas would not fit 20 KB anyway
    p = plan(**FOLDED2)
    assert p["point_lds"] == (5 * 64 + 16 * 16) * 16 and p["point_lds_fresh"] == (13 * 64 + 16 * 16) * 16


def test_buffers(plan):
    max_nz = plan()["MAX_NZ"]
    assert max_nz == 32
    for fast in (0, 1):
        for nwork in (1, 2, 1000):
            for nz in (1, 2, max_nz):
                p = plan(**FOLDED2, fast=fast, nwork=nwork, nz=nz, nt=77, lt_rows=77, R=2, nacc=3)
                regions = [(p["b_ndone"], nwork), (p["b_todo"], 1 + nwork), (p["b_defer"], 1 + nwork * nz), (p["b_wcount"], 1)]
                assert regions[0][0] == 0
                for (o0, n0), (o1, _) in zip(regions, regions[1:]):
                    assert o0 + n0 <= o1, (nwork, nz)
                assert regions[-1][0] + regions[-1][1] <= p["b_ints"]
                assert p["b_ints"] == 2 * nwork + 2 + nwork * nz + 2
                # ... and as the launcher wrote them out
                assert (p["b_todo"], p["b_defer"], p["b_wcount"]) == (nwork, 2 * nwork + 1, 2 * nwork + 2 + nwork * nz)
                assert p["b_item"] == (2 + 1 + 3) * nz * 64 * 16
                assert p["b_ltab"] == nwork * p["b_item"]
                assert p["b_state"] == p["b_ltab"] + (77 * 21 * 16 if fast else 0)
                # the plan carries the same description, for the rows its laptime_kernel writes
                assert p["rc"] == 0 and (not fast or p["nrows"] == 77)
                assert [p[k] for k in ("p_todo", "p_defer", "p_wcount", "p_ints", "p_item", "p_ltab", "p_state")] == \
                       [p[k] for k in ("b_todo", "b_defer", "b_wcount", "b_ints", "b_item", "b_ltab", "b_state")]


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip", ".cpp")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read().splitlines()


def test_the_shared_buffers_are_laid_out_in_one_place():
    """in the style of test_the_library_reads_its_environment_in_one_place: the offsets that launcher and host used to write out
    twice (d_ndone + 2 * (size_t)nwork + ..., (2 * items + 2 + ...) * sizeof(int), the table behind nwork x slots of state)"""
    pat = re.compile(r"2 \* \(size_t\)nwork|2 \* items|2 \* nwork|ndone \+ nwork|state \+ \(size_t\)nwork|items \* \(size_t\)dp\.nz")
    hits = [(name, i + 1) for name, lines in _sources() if name != NEW_HEADER for i, line in enumerate(lines) if pat.search(line)]
    assert hits == [], hits
    own = [name for name, lines in _sources() if any("ucf_transform_buffers transform_buffers(" in line for line in lines)]
    assert own == [NEW_HEADER]


def test_lds_budgets_are_compared_in_one_place():
    pat = re.compile(r"(<=|>=|<|>)\s*(\(size_t\))?(160|40) \* 1024")
    hits = [(name, i + 1) for name, lines in _sources() if name != NEW_HEADER for i, line in enumerate(lines) if pat.search(line)]
    assert hits == [], hits
    with open(os.path.join(CSRC, NEW_HEADER)) as f:
        assert len(pat.findall(f.read())) >= 6
