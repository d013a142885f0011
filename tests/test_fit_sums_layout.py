"""The layout of the sums of the fit reduction (unconfined_amd/csrc/ucf_fit.h: ucf_fit_sums, ucf_fit_sums_of): where the kernel
places phi, g, A, phi_d, phi_w and phi_out of a parameter set, where the host reads them and how it sizes its buffers -- one
constexpr description in plain C++, so it is looked at here without a GPU.

A stand-alone program includes only ucf_fit.h and prints the layout of every instantiation of the kernel (npar 0..8, with and
without derivative data, plain / robust / resampled), then the layout of a few filled ucf_fit_reduce_args.  The expectations
are the layout as the kernel has always written it,

    phi | g[npar] | upper triangle of A, row by row | [phi_d] | [phi_w] | [phi_out]

phi_d with derivative data, phi_w under a robust or a resampled reduction, phi_out under a resampled one -- spelled out below
as that row of names, not taken from the header; the number of sums is also held to nsums of the three restatements of the
kernel (fit_reduce_restate, fit_loss_restate, fit_resample_restate), which know nothing of the header.
"""
import os
import subprocess

import pytest

import fit_loss_restate as fl
import fit_reduce_restate as fr
import fit_resample_restate as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unconfined_amd", "csrc")

PROGRAM = r"""
#include "ucf_fit.h"
#include <stdio.h>
static void row(const char* tag, int npar, int deriv, const char* what, const ucf_fit_sums_layout& L)
{
    printf("%s %d %d %s %d %d %d %d %d %d %d\n", tag, npar, deriv, what, L.phi, L.g, L.A, L.phi_d, L.phi_w, L.phi_out, L.count);
}
/* usable where a constant is needed: the kernel takes its array extent from it */
static_assert(ucf_fit_sums(2, true, true, true).count == 9, "constexpr");
static double sized_by_layout[ucf_fit_sums(8, true, false, true).count];
int main()
{
    for (int npar = 0; npar <= 8; npar++)
        for (int deriv = 0; deriv < 2; deriv++) {
            row("T", npar, deriv, "plain", ucf_fit_sums(npar, deriv != 0, false, false));
            row("T", npar, deriv, "robust", ucf_fit_sums(npar, deriv != 0, true, false));
            row("T", npar, deriv, "resampled", ucf_fit_sums(npar, deriv != 0, false, true));
        }
    /* robust and resampled at once (a resampled launch under Huber or Tukey): the resampled layout */
    row("B", 3, 1, "resampled", ucf_fit_sums(3, true, true, true));
    printf("S %d\n", (int)(sizeof(sized_by_layout) / sizeof(double)));
    /* filled arguments: the layout follows the predicates that choose the launcher's instantiation */
    static double some;
    static int some_int;
    for (int deriv = 0; deriv < 2; deriv++) {
        ucf_fit_reduce_args a = {};
        a.npar = 3; a.nsets = 2; a.nobs = 5;
        a.d_dh = deriv ? &some : NULL;
        row("A", 3, deriv, "l2_nothing_asked", ucf_fit_sums_of(&a));
        printf("P %d %d\n", ucf_fit_reduce_is_robust(&a) != 0, ucf_fit_reduce_is_resampled(&a) != 0);
        ucf_fit_reduce_args b = a;
        b.d_b = &some;
        row("A", 3, deriv, "l2_with_b", ucf_fit_sums_of(&b));
        printf("P %d %d\n", ucf_fit_reduce_is_robust(&b) != 0, ucf_fit_reduce_is_resampled(&b) != 0);
        ucf_fit_reduce_args n = a;
        n.d_ndown = &some_int;
        row("A", 3, deriv, "l2_with_ndown", ucf_fit_sums_of(&n));
        ucf_fit_reduce_args h = a;
        h.loss = 1; h.loss_c = 1.5;                  /* UCF_LOSS_HUBER */
        row("A", 3, deriv, "huber", ucf_fit_sums_of(&h));
        printf("P %d %d\n", ucf_fit_reduce_is_robust(&h) != 0, ucf_fit_reduce_is_resampled(&h) != 0);
        ucf_fit_reduce_args r = a;
        r.nred = 4;
        row("A", 3, deriv, "l2_resampled", ucf_fit_sums_of(&r));
        printf("P %d %d\n", ucf_fit_reduce_is_robust(&r) != 0, ucf_fit_reduce_is_resampled(&r) != 0);
        ucf_fit_reduce_args z = a;
        z.npar = 0;                                  /* the trial points: objective only */
        row("A", 0, deriv, "l2_nothing_asked", ucf_fit_sums_of(&z));
    }
    return 0;
}
"""

FIELDS = ("phi", "g", "A", "phi_d", "phi_w", "phi_out")


def expected(npar, deriv, mode):
    """positions in the row of names above; -1 where the launch has no such sum"""
    names = ["phi"] + ["g"] * npar + ["A"] * (npar * (npar + 1) // 2)
    names += ["phi_d"] if deriv else []
    names += ["phi_w"] if mode in ("robust", "resampled") else []
    names += ["phi_out"] if mode == "resampled" else []
    at = {k: (names.index(k) if k in names else -1) for k in FIELDS}
    if npar == 0:
        at["g"] = at["A"] = 1      # empty, but with a place: where they would start
    at["count"] = len(names)
    return at


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("fit_sums_layout")
    src = d / "fit_sums_layout.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "fit_sums_layout")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.splitlines()]


def rows(lines, tag):
    return [(int(t[1]), int(t[2]), t[3], dict(zip(FIELDS + ("count",), map(int, t[4:])))) for t in lines if t[0] == tag]


def test_every_instantiation(lines):
    table = rows(lines, "T")
    assert len(table) == 54
    assert sorted((n, d, m) for n, d, m, _ in table) == sorted((n, d, m) for n in range(9) for d in (0, 1) for m in ("plain", "robust", "resampled"))
    for npar, deriv, mode, got in table:
        assert got == expected(npar, deriv, mode), (npar, deriv, mode)


def test_some_rows_by_hand(lines):
    table = {(n, d, m): got for n, d, m, got in rows(lines, "T")}
    assert table[(0, 0, "plain")] == dict(phi=0, g=1, A=1, phi_d=-1, phi_w=-1, phi_out=-1, count=1)
    assert table[(0, 1, "robust")] == dict(phi=0, g=1, A=1, phi_d=1, phi_w=2, phi_out=-1, count=3)
    assert table[(2, 1, "resampled")] == dict(phi=0, g=1, A=3, phi_d=6, phi_w=7, phi_out=8, count=9)
    assert table[(4, 0, "plain")] == dict(phi=0, g=1, A=5, phi_d=-1, phi_w=-1, phi_out=-1, count=15)
    assert table[(8, 0, "robust")] == dict(phi=0, g=1, A=9, phi_d=-1, phi_w=45, phi_out=-1, count=46)
    assert table[(8, 1, "resampled")] == dict(phi=0, g=1, A=9, phi_d=45, phi_w=46, phi_out=47, count=48)
    (_, _, _, both), = rows(lines, "B")
    assert both == table[(3, 1, "resampled")]
    assert [t for t in lines if t[0] == "S"] == [["S", "48"]]      # an array sized by the layout of (8, deriv, resampled)


def test_count_is_nsums_of_the_restatements(lines):
    nsums = {"plain": fr.nsums, "robust": fl.nsums, "resampled": fs.nsums}
    for npar, deriv, mode, got in rows(lines, "T"):
        assert got["count"] == nsums[mode](npar, bool(deriv)), (npar, deriv, mode)


def test_layout_of_filled_arguments_follows_the_launcher(lines):
    mode_of = {"l2_nothing_asked": "plain", "l2_with_b": "robust", "l2_with_ndown": "robust", "huber": "robust", "l2_resampled": "resampled"}
    got = rows(lines, "A")
    assert len(got) == 12
    for npar, deriv, case, at in got:
        assert at == expected(npar, deriv, mode_of[case]), (npar, deriv, case)
    # (robust, resampled) as the launcher's predicates see the cases, in the program's order, without and with derivative data
    preds = [(int(t[1]), int(t[2])) for t in lines if t[0] == "P"]
    assert preds == [(0, 0), (1, 0), (1, 0), (0, 1)] * 2


def test_the_layout_is_written_in_one_place():
    """in the style of test_launch_plan: no host file holds a position into a row of sums, and the counting helpers that the
    layout replaced are gone"""
    for name in ("ucf_fit.cpp", "ucf_debug.cpp", "ucf_fit.hip", "ucf_fit.h"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for gone in ("ucf_fit_nsums", "ucf_fit_joint_nsums", "ucf_fit_reduce_nsums", "nsum - 1", "nsum - 2", "NSUMS - 1"):
            assert gone not in text, (name, gone)
    own = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip", ".cpp"))
           and "ucf_fit_sums_layout ucf_fit_sums(" in open(os.path.join(CSRC, name)).read()]
    assert own == ["ucf_fit.h"]
