// Which eigen-directions of a Gramian carry a mode, stated once for the POD build (eigh.hip: select_modes_kernel; eigh_topk.hip:
// build_w_kernel, scale_cols_kernel; mor/pod.py: modes_from_gramian states the same on the host).  An eigenvalue that has cancelled
// to nothing -- w_i <= floor w_max, or w_i <= 0 -- has no singular value to divide by: its direction gets a zero row / column
// instead of inf or NaN.  floor = 1e-28 (a singular value below 1e-14 of the largest) where the caller knows nothing more;
// mode_floor(n) where the eigenvalues come from srom_eigh_dev on a formed n x n Gramian: its eigenvalues are good to n eps w_max
// in absolute terms, so below that floor a positive w_i is rounding noise of either sign (rom_dim beyond the numerical rank).
#pragma once
#include <cstdint>

__device__ inline bool mode_is_live(double wi, double wmax, double floor = 1e-28) { return wi > floor * wmax && wi > 0.0; }
__device__ inline double mode_floor(int64_t n) { return fmax(1e-28, (double)n * 2.220446049250313e-16); }
