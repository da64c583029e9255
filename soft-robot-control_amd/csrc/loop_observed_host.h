// The observed sub-step chain of the two loops whose law reads a batched filter's estimate (gusto_loop.hip, ilqr_loop.hip), stated once:
// what an attached observer must match, the shapes of the blocks it adds to a run, the kernel that records a filter step, and the
// order of the chain's launches.  Included by those two units only: each gets its own instance of the kernel (anonymous namespace).
#pragma once
#include "observer_host.h"
#include "gusto_loop_host.h"

namespace {

// After a batched filter step: the estimates into row `row` of the record (B x rows x n), and the filters' status words into the
// status record E (B) -- assigned at the chain's first sub-step, or-ed at the others.  64 threads per member.
__global__ __launch_bounds__(64) void loop_estimate_record_kernel(const double *xhat, const int *status, double *Xhat, int32_t *E, int n,
                                                                  int64_t rows, int64_t row, int first) {
    const size_t b = blockIdx.x;
    for (int e = SRH_TID; e < n; e += 64) ((gptr)Xhat)[(b * (size_t)rows + row) * n + e] = ((cgptr)xhat)[b * n + e];
    if (SRH_TID == 0) E[b] = first ? status[b] : (E[b] | status[b]);
}

// what a loop of B members with n states and m inputs refuses of an observer
int loop_check_observer(const char *who, const sekf_batch *observer, int64_t B, int n, int m) {
    SRH_REQUIRE(observer->batch == B, "%s: the observer has batch = %lld filters, the loop %lld members", who, (long long)observer->batch,
                (long long)B);
    SRH_REQUIRE(observer->n == n && observer->m == m, "%s: the observer's model has n_x = %d, n_u = %d, the loop n_x = %d, n_u = %d", who,
                observer->n, observer->m, n, m);
    SRH_REQUIRE(observer->model->has_discrete, "%s: the observer's model has not been pre-discretised (at dt_sim)", who);
    return SRH_OK;
}

// the blocks an observer of n states and ny measurements adds to a run: estimates (B x (S + 1) x n), measurements (B x S x ny), the
// filters' status (per period), the measurement noise (S x B x ny)
void loop_shape_observed(LoopRec &XH, LoopRec &Y, LoopRec &E, LoopRec &V, int n, int ny) {
    const size_t D = sizeof(double);
    XH.shape(D * n, 1); Y.shape(D * ny, 0); E.shape(sizeof(int32_t), 0, true); V.shape(D * ny, 0);
    (void)V.d.alloc(0);                 // (the noise block of another n_y is given back: the first run with noise allocates this one's)
}

// where the chain reads and writes: rows row0_u + s of the records U (m wide) and Y (ny wide), rows_u rows per member; row xh_row0 + s
// of the estimate record XH (xh_rows rows per member); the status entry E (B); the filters' region record pick with its member
// stride sp, or null
struct ObsRecs {
    const double *U, *Y;
    int64_t rows_u, row0_u;
    double *XH;
    int64_t xh_rows, xh_row0;
    int32_t *E, *pick;
    int64_t sp;
};

// The observed chain on the handle's stream, steps x (advance(s): the unit's launch of sub-step s under the law at the estimate, with
// its measurement -> one step of every filter from the recorded u and y -> the estimates and the status into their records)
template <class Advance>
int loop_observed_chain(const LoopStage *h, sekf_batch *obs, int64_t steps, const ObsRecs &r, Advance advance) {
    const int n = obs->n, m = obs->m, ny = obs->ny;
    int rc;
    for (int64_t s = 0; s < steps; ++s) {
        if ((rc = advance(s))) return rc;
        if ((rc = sekf_batch_step_dev(obs, r.U + (size_t)(r.row0_u + s) * m, r.rows_u * m, r.Y + (size_t)(r.row0_u + s) * ny, r.rows_u * ny,
                                      r.pick ? r.pick + s : nullptr, r.sp, h->stream)))
            return rc;
        loop_estimate_record_kernel<<<(unsigned)h->B, 64, 0, h->stream>>>(obs->x_dev(), obs->status_dev(), r.XH, r.E, n, r.xh_rows, r.xh_row0 + s,
                                                                          s == 0 ? 1 : 0);
        SRH_CHECK_HIP(hipGetLastError());
    }
    return SRH_OK;
}

}  // namespace
