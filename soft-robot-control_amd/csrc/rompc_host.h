// Host-side ROMPC handle (owns the estimate and the folded constants in HBM) shared by rompc.hip / rompc_loop.hip.
#pragma once
#include "common.h"

struct srompc {
    int64_t batch = 0;
    int n = 0, m = 0, ny = 0, nz = 0;
    bool has_H = false;
    std::vector<double> A, B, d, C, yref, H, zref, K, L;     // host copies: the fold is redone when the gains change
    int n4 = 0, m4 = 0, ny4 = 0, ld1 = 0, ldk = 0, nconst = 0;
    size_t lds = 0;
    srh::DevBuf consts, in, res, xfull;
    size_t in_doubles = 0, res_doubles = 0, xfull_doubles = 0;
    double *pin_in = nullptr, *pin_out = nullptr, *pin_xf = nullptr;
    hipStream_t stream = nullptr;
    int64_t steps = 0, step_waits = 0;
    bool timing = false;
    hipEvent_t ev[2] = {nullptr, nullptr};      // first enqueue .. last copy of a call, when timing is on
    double last_ms = -1.0;
    double *est() const { return res.as<double>() + (size_t)batch * m; }            // res = [u | x_hat | z]
    double *zres() const { return res.as<double>() + (size_t)batch * (m + n); }
    // F = A - L C, entry (i, j): the sum rompc.hip's packed constants and rompc_loop.hip's transposed ones both hold (k = 0, 1, ...)
    double fold(int i, int j) const {
        double f = A[(size_t)i * n + j];
        for (int k = 0; k < ny; ++k) f -= L[(size_t)i * ny + k] * C[(size_t)k * n + j];
        return f;
    }
};
