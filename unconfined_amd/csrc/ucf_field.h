// ucf_field.h -- launcher of the well-field superposition (ucf_field.hip), called by ucf_field_drawdown (ucf_field.cpp).
#pragma once
#include <cstddef>

// What the kernel needs of well j: its rate factor and where its group's results lie.  The groups' h (and dh) share one
// buffer, group g at `off` doubles, [nt_g][nr][nz]; tfac of all groups one array, group g at `toff`.
struct ucf_field_well {
    double q;
    long long off;
    int k0, nr, toff, _pad;
};

// One thread per output (k, i, z) of s, ds [nt][nloc][nz], z fastest:
//   acc = +0.0;  for j = 0..nwell-1 with k >= k0_j:  at = off_j + ((k - k0_j) nr_j + col[i][j]) nz + z
//     s :  acc = acc + q_j * h[at]        ds :  acc = acc + q_j * (tfac[toff_j + k - k0_j] * dh[at])
//   both times `scale` unless scaled == 0.
// d_wells [nwell], d_col [nloc][nwell] (column of location i in the group of well j), d_tfac, d_h, d_dh as above.
int ucf_field_launch_superpose(int nt, int nloc, int nz, int nwell, const ucf_field_well* d_wells, const int* d_col,
                               const double* d_tfac, const double* d_h, const double* d_dh, int scaled, double scale,
                               double* d_s, double* d_ds, void* stream);
