// Host-side iLQR buffers and the resident plan handle (owns every buffer of a solve) shared by lqr.hip / ilqr_loop.hip.
#pragma once
#include "tpwl_host.h"

// Every device buffer of one ilqr_kernel launch: the inputs, the policy (x, u, K), cost / iters, and the kernel's work space.
// silqr_solve / silqr_solve_ssm make one per call; a plan keeps one.
struct IlqrBufs {
    srh::DevBuf x0, z, uw, ul, Q, R, Qf, x, u, K, cost, iters, work, iwork, lin;
    size_t stride = 0;                   // doubles of `work` per problem
};

// `batch` problems of horizon N on one pre-discretised TPWL model.  x (batch x (N+1) x n), u (batch x N x m), K (batch x N x m x n)
// are the policy of the last solve and stay on the device; x0 / uw / ul are where the host-pointer solve puts its inputs.
struct silqr_plan : IlqrBufs {
    stpwl *model = nullptr;
    int N = 0, n = 0, m = 0, nz = 0;
    int64_t batch = 0;
    silqr_params par;
    bool has_target = false, has_ul = false, solved = false;
    const double *x_dev() const { return x.as<double>(); }
    const double *u_dev() const { return u.as<double>(); }
    const double *K_dev() const { return K.as<double>(); }
};

// One solve of every problem of the plan on `stream` from device inputs: one launch, no copy, no wait.  x0_dev (batch x n);
// u_warm_dev (batch x N x m) or NULL; u_last is the one silqr_plan_set_u_last installed (none: zeros, as a NULL u_last of silqr_solve).
extern "C" int silqr_plan_solve_dev(silqr_plan *p, const double *x0_dev, const double *u_warm_dev, hipStream_t stream);
