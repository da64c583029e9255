// Host-side EKF handle (owns the filters' HBM state) shared by observer.hip / gusto_loop.hip.
#pragma once
#include "tpwl_host.h"

// `batch` filters over one model, one launch per step: workgroup b is filter b.  C, y_ref, W, V and the model tables are shared;
// x, Sigma and the status word are per filter.  The single filter (sekf) is this at batch = 1.
struct EkfFilters {
    stpwl *model = nullptr;
    int n = 0, m = 0, ny = 0, batch = 0;
    // xs: [x (batch x n) | status (batch int32)]: one copy back; uy: [u (batch x m) | y (batch x ny)]: the host step's inputs;
    // Sigma0, pick (sekf_batch only): the covariance the loop's reset re-installs, the table point of each filter's last predictor
    srh::DevBuf C, y_ref, W, V, Sigma0, Sigma, xs, uy, pick;
    size_t lds = 0;
    int path = 0, gain_form = 0;          // the kernel of these filters: ekf_plan (EKF_VALU .. EKF_WIDE)
    double *pin_in = nullptr, *pin_out = nullptr;               // pinned mirrors of uy and xs: one copy each way per step
    double *x_dev() const { return xs.as<double>(); }
    int *status_dev() const { return (int *)(x_dev() + (size_t)batch * n); }
    const double *yref_dev() const { return y_ref.p ? y_ref.as<double>() : nullptr; }
    size_t xs_bytes() const { return sizeof(double) * (size_t)batch * n + sizeof(int) * (size_t)batch; }
    ~EkfFilters() {
        if (pin_in) (void)hipHostFree(pin_in);
        if (pin_out) (void)hipHostFree(pin_out);
    }
};

struct sekf_batch : EkfFilters {};

struct sekf : EkfFilters {
    srh::DevBuf ext;                     // explicit [A_d (n x n) | B_d (n x m) | d_d (n)] of sekf_step
    hipStream_t side = nullptr;          // sekf_step_projected: the projection runs beside the filter kernel
    hipEvent_t side_gate = nullptr;      // orders the side stream behind earlier work of stream 0 on the same rom
    ~sekf() {
        if (side) (void)hipStreamDestroy(side);
        if (side_gate) (void)hipEventDestroy(side_gate);
    }
};

// One step of every filter of the batch on `stream`, from device inputs: one launch, no copy, no wait (gusto_loop.hip chains it behind
// its advance kernel).  u_dev / y_dev: filter b reads u_dev + b su (n_u entries) and y_dev + b sy (n_y entries); NULL: no predictor / no
// update.  pick_dev (optional): the table point filter b's predictor took goes to pick_dev[b sp].
int sekf_batch_step_dev(sekf_batch *h, const double *u_dev, int64_t su, const double *y_dev, int64_t sy, int32_t *pick_dev, int64_t sp,
                        hipStream_t stream);
// Sigma0 into every filter (device copies on stream 0, waited for)
int sekf_batch_install_sigma0(sekf_batch *h);
