// What the SSM horizon error (ssm_horizon.hip) needs of the SSM closed loops' sub-step (gusto_ssm_loop.hip) beyond the staged evaluator of
// ssm_dev.h: the affine sum of the plant step (SSM/ssm.py:331-333), which both units call from here, and THE ESTIMATE of the reference's
// SSMObserver (SSM/controllers.py:302-310).
#pragma once
#include "ssm_dev.h"

// THE ESTIMATE for units other than gusto_ssm_loop.hip: x_hat = V phi_s(yd), yd = y - z_ref of the observer's model (no entries, LDS).
// gusto_ssm_loop.hip states THE ESTIMATE itself (ssm_loop_estimate: the unit's own surface test keeps that definition in its file); this is
// the same statement, token for token behind the name (tests/test_ssm_horizon_surface_cpu.py compares the two bodies) and bit for bit
// (tests/test_ssm_horizon_gpu.py: x_obs of the loop's measurement record is the loop's Xhat record).
// ps / vs: parent and variable of every monomial of its ssm basis, lv: first index of every degree, Vl: its v_coeff (n x ns) in LDS,
// phi: ns doubles of work.  The monomials degree by degree (ssm::basis_l without a derivative table: only parent / variable are read),
// then row o by eight lanes, lane g summing the columns g, g + 8, ... by fma from 0.0, and wg::group_sum<8> -- as ssm::observe_l.
// Writes xh (LDS) and, unless null, the record row XHr.  All nt threads; ends with a sync.
__device__ __forceinline__ void ssm_step_estimate(liptr ps, liptr vs, const int *lv, int order_s, int ns, int no, int n, clptr yd, lptr phi,
                                                  clptr Vl, lptr xh, gptr XHr, int tid, int nt) {
    ssm::basis_l(ps, ps, vs, ps, lv, order_s, ns, no, yd, phi, (lptr) nullptr);
    const int g8 = tid & 7;
    for (int o0 = 0; o0 < n; o0 += nt / 8) {
        const int o = o0 + (tid >> 3);
        double acc = 0.0;
        if (o < n) for (int k = g8; k < ns; k += 8) acc = fma(Vl[(size_t)o * ns + k], phi[k], acc);
        acc = wg::group_sum<8>(acc);
        if (g8 == 0 && o < n) {
            xh[o] = acc;
            if (XHr != nullptr) XHr[o] = acc;
        }
    }
    __syncthreads();
}

// THE AFFINE SUM of the plant step, row i: (A_d x)_i and (B_d u)_i each by fma from 0.0 in column order, then (ax + bu) + d_i.
// Al (n x n), Bl (n x m), dl (n): the discretised linearisation at (x, u) (ssm::jacobians_l, ssm::discretize), all in LDS.
__device__ __forceinline__ double ssm_step_affine_row(clptr Al, clptr Bl, clptr dl, clptr xs, clptr us, int n, int m, int i) {
    double ax = 0.0, bu = 0.0;
    for (int j = 0; j < n; ++j) ax = fma(Al[i * n + j], xs[j], ax);
    for (int j = 0; j < m; ++j) bu = fma(Bl[i * m + j], us[j], bu);
    return ax + bu + dl[i];
}
