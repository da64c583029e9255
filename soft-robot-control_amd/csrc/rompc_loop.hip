// Batched closed loop of the ROMPC baseline: every problem of an srompc_t handle's batch is its own loop of the reference's controller --
// solve the linear reduced-order MPC from the END of the stitched nominal trajectory, track that trajectory with u = ubar + K (x_hat -
// xbar) while a Luenberger observer follows the plant's measurements -- and a whole run of periods is one launch sequence on the handle's
// stream with one host wait.  Reference: sofacontrol/baselines/rompc/rompc.py:57-141 (evaluate, solve_OCP, get_OCP_solution),
// rompc/observer.py:37-40 (update), baselines/ros.py:202-235 (the MPC node and its failure shift), baselines/mpc.py (get_target).
//
// THE POLICY.  B members, controller step dt_sim, QP horizon N at dt_mpc, n_replan sub-steps per period, n_replan dt_sim <= N dt_mpc.
// Period p starts at t_p = t_start + p n_replan dt_sim.
//   request   x0_p = x_hat0 of the reset (p = 0), else the previous plan's states interpolated at tau = n_replan dt_sim: interval
//             j = min(int(tau / dt_mpc), N - 1), theta = (tau - j dt_mpc) / dt_mpc (theta == 1 at the largest n_replan).  Targets: the
//             window at (t_p + phase_b) + dt_mpc k; zf its last row when the cost has Qf; u_des N rows (loop_prepare_kernel).
//   solve     the trust-region-free QP with constant (A_mpc, B_mpc, d_mpc), all members in one launch (slocp_plan_solve_dev_resident:
//             the tiled horizon goes through the plan's transposes once).
//   chain     row 0 of the plan's states is set to x0_p; a member whose QP reports a non-zero status gets the previous plan moved up one
//             row with its last row held (ros.py:223-227), in period 0 x0_0 in every state row and zero inputs; the status is recorded
//             either way.  The next request's x0 is read off the plan as it stands after this (THE PLAN SHIFT of mpc_loop_host.h with
//             row 0 pinned, no idle input and x0_next).
//   sub-steps s = 0..n_replan-1 at tau = s dt_sim, (j_s, theta_s) of sgusto_loop_schedule, ubar_s / xbar_s = lo + theta (hi - lo) with
//             the input held over the last interval (rompc_loop_advance_kernel):
//               1. y_s = (C x_s + y_ref) + v_s                      the measurement of the current plant state
//               2. u_s = ubar_s + K (x_hat_s - xbar_s)              (rompc.py:79: the law reads the estimate before the update)
//               3. x_hat_{s+1} = [F | B | L] [x_hat_s ; u_s ; y_s - y_ref] + d, F = A - L C     (the folded form of rompc.hip)
//               4. x_{s+1} = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s (tpwl::nearest_wave), or
//                  x_{s+1} read from the given plant record.
// Not offered: the start-up phase before t_delay, the full-order state and its projection per step, input clipping, dU rows,
// input_nullspace.  The host shell of a handle and of a run is gusto_loop_host.h, the constant-horizon QP and the plan shift
// mpc_loop_host.h, the target window gusto_loop_prep.h.
#include "rompc_host.h"
#include "tpwl_host.h"
#include "mpc_loop_host.h"

#include <algorithm>

namespace {

struct RlAdvArgs {
    int N, n_keep, n, m, ny, nz;
    int plant;                          // 1: the TPWL plant is stepped; 0: x_{s+1} is read from Xp
    int z0;                             // 1: H x_in goes to row row0_x - 1 of Z first (the first period of a run)
    const double *xopt, *uopt;          // the plans (B x (N+1) x n), (B x N x m)
    const double *Mt;                   // ((n + m + ny) x n) [F B L]^T: row q holds column q of [F B L]
    const double *dv, *K, *C, *yref, *Hz;       // (n), (m x n), (ny x n), (ny), (nz x n)
    const double *W, *Vn;               // (steps x B x n), (steps x B x ny) or null; this launch reads steps w_step0 ..
    const double *Xp;                   // (B x rows_x x n) the recorded plant (rows as X), or null
    const int32_t *js;                  // (n_keep) plan interval of every sub-step
    const double *theta;                // (n_keep) position inside it
    const double *x_in, *xh_in;         // (B x n) plant states and estimates
    const double *x0_next;              // (B x n) the plan at the period's end: the row of Xbar behind the last sub-step, or null
    double *x_out, *xh_out;             // (B x n) or null (may be the inputs)
    double *X, *XH, *Z, *Xbar;          // records (B x rows_x x .): row row0_x + s holds what sub-step s ends with; Xbar row row0_x - 1 + s
    double *Y, *U, *Ubar;               // records (B x rows_u x .): row row0_u + s
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
};

// LDS of the launch in doubles: x, x_bar | v = [x_hat ; u ; y - y_ref] | u_bar (16) | partial sums of A x, B u, [F B L] v (256 each) |
// the point (2) | the plant's panel A^T, B^T, d (plant only).  n, m, n + m + ny are padded to even so that the panel is 16-byte aligned.
__host__ __device__ inline int rl_even(int v) { return (v + 1) & ~1; }
size_t rl_advance_lds_bytes(int n, int m, int ny, bool plant) {
    const size_t d = 2 * (size_t)rl_even(n) + rl_even(n + m + ny) + 16 + 256 + 2;
    return srh::lds_request(sizeof(double) * (d + (plant ? tpwl::step_doubles(n, m, 256) : 2 * 256)));
}

// One workgroup of 256 threads per member, all n_keep sub-steps of a period.  The plant's region panel [A_d^T | B_d^T | d_d] sits in LDS
// and is reloaded only when the plant's nearest point changes (as loop_advance_kernel, gusto_loop.hip); x, x_bar and the observer's
// operand v = [x_hat ; u ; y - y_ref] stay in LDS for the whole launch (x_hat - x_bar is formed where K reads it).  The controller's
// constants -- [F B L]^T, K, C, H -- are read from global memory through L2: every workgroup reads the same 59 KB at the Diamond shape.
// Fixed summation orders:
//   y_e    = measure_row (gusto_loop_prep.h): (C x)_e + y_ref[e], then + v_e; v's last block holds y_e - y_ref[e]
//   u_e    = ubar_e + wave_sum over lanes of (sum over c = lane, lane + 64, ... of K[e][c] (x_hat[c] - x_bar[c]) by fma from 0.0)
//   x'     = THE STEP RULE of tpwl_dev.h (+ w)
//   x_hat' = d + (partials of [F B L] v in slice order), the step rule's slices over the n + m + ny rows of [F B L]^T
//   z_e    = out_row (gusto_loop_prep.h) of H x'
__global__ __launch_bounds__(256) void rompc_loop_advance_kernel(TpwlDev TL, RlAdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = a.n, m = a.m, ny = a.ny, nz = a.nz, N = a.N, nv = n + m + ny;
    lptr xc = (lptr)smem;                                // n      plant state
    lptr xb = xc + rl_even(n);                           // n      x_bar
    lptr vh = xb + rl_even(n);                           // nv     [x_hat ; u ; y - y_ref]
    lptr ub = vh + rl_even(nv);                          // 16     u_bar
    tpwl::StepLds L;                                     //        partial sums of A x, B u | ph, ip | the panel of region `cur`
    tpwl::step_carve(L, ub + 16, n, m, 256, 256 + 2);
    lptr ph = L.pb + 256;                                // 256    partial sums of [F B L] v
    liptr ip = (liptr)(ph + 256);                        // (two doubles) plant point
    lptr xh = vh, uc = vh + n, yd = vh + n + m;
    const size_t b = blockIdx.x;
    const int tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int S = max(1, 256 / n), j = tid % n, sl = tid / n;
    cgptr xo = (cgptr)a.xopt + b * (size_t)(N + 1) * n, uo = (cgptr)a.uopt + b * (size_t)N * m;
    cgptr Mt = (cgptr)a.Mt, dv = (cgptr)a.dv, Kg = (cgptr)a.K, Cg = (cgptr)a.C, yr = (cgptr)a.yref, Hz = (cgptr)a.Hz;
    cgptr Wd = (cgptr)a.W, Vd = (cgptr)a.Vn, Xp = (cgptr)a.Xp, thg = (cgptr)a.theta;
    cgiptr jsg = (cgiptr)a.js;
    for (int e = tid; e < n; e += 256) {
        xc[e] = ((cgptr)a.x_in)[b * n + e];
        xh[e] = ((cgptr)a.xh_in)[b * n + e];
    }
    __syncthreads();
    if (a.z0 && a.Z)
        for (int e = tid; e < nz; e += 256) ((gptr)a.Z)[(b * (size_t)a.rows_x + a.row0_x - 1) * nz + e] = out_row(Hz, e, n, xc);
    int cur = -1;
    for (int s = 0; s < a.n_keep; ++s) {
        const int js = jsg[s];
        const double th = thg[s];
        const size_t rx = b * (size_t)a.rows_x + a.row0_x + s, ru = b * (size_t)a.rows_u + a.row0_u + s;
        if (tid < n) {                                   // (n <= 128: waves 0 and 1)
            const double v = plan_at(xo, n, js, js + 1, th, tid);
            xb[tid] = v;
            if (a.Xbar) ((gptr)a.Xbar)[(rx - 1) * n + tid] = v;
        } else if (tid >= 128 && tid < 128 + m) {        // the input is held over the last interval
            const int e = tid - 128;
            const double v = plan_at(uo, m, js, min(js + 1, N - 1), th, e);
            ub[e] = v;
            if (a.Ubar) ((gptr)a.Ubar)[ru * m + e] = v;
        }
        if (a.plant && wave == 3) {                      // (the wave with neither plan rows nor input rows)
            const int i = tpwl::nearest_wave(TL, xc);
            if (lane == 0) ip[0] = (unsigned)i < (unsigned)TL.P ? i : 0;           // (a state that is not a number: no minimum)
        }
        for (int e = tid; e < ny; e += 256) {            // 1. the measurement of the current plant state
            __builtin_assume(yr != nullptr);             // (a controller always has its y_ref: no test of it in measure_row)
            const double v = measure_row(Cg, e, n, xc, yr, Vd, ((size_t)(a.w_step0 + s) * a.B + b) * ny + e);
            yd[e] = v - yr[e];
            if (a.Y) ((gptr)a.Y)[ru * ny + e] = v;
        }
        __syncthreads();
        int p = 0;
        if (a.plant) {
            p = ip[0];
            tpwl::panel_load(L, TL, p, cur, n, m, SRH_TID, 256);           // (the same for every thread; the barrier below covers the copies)
        }
        for (int e = wave; e < m; e += 4) {              // 2. u = ubar + K (x_hat - xbar)
            double acc = 0.0;
            for (int c = lane; c < n; c += 64) acc = fma(Kg[e * n + c], xh[c] - xb[c], acc);
            acc = wg::wave_sum(acc);
            if (lane == 0) {
                const double u = ub[e] + acc;
                uc[e] = u;
                if (a.U) ((gptr)a.U)[ru * m + e] = u;
            }
        }
        __syncthreads();
        if (sl < S) {                                    // 3. and 4.: the slices of both products
            double vh_ = 0.0;
#pragma unroll 4
            for (int q = sl; q < nv; q += S) vh_ = fma(Mt[(size_t)q * n + j], vh[q], vh_);
            ph[sl * n + j] = vh_;
            if (a.plant) tpwl::step_slices(L, xc, uc, n, m, S, j, sl);
        }
        __syncthreads();
        if (tid < n) {
            double v;
            if (a.plant) {
                v = tpwl::step_sum(L, n, S, tid);
                if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * n + tid];
            } else {
                v = Xp[(rx)*n + tid];
            }
            xc[tid] = v;
            if (a.X) ((gptr)a.X)[rx * n + tid] = v;
            double h = dv[tid];
            for (int q = 0; q < S; ++q) h += ph[q * n + tid];
            xh[tid] = h;
            if (a.XH) ((gptr)a.XH)[rx * n + tid] = h;
        }
        __syncthreads();
        // z = H x'.  x is next written behind three barriers of the next sub-step.
        if (a.Z)
            for (int e = tid; e < nz; e += 256) ((gptr)a.Z)[rx * nz + e] = out_row(Hz, e, n, xc);
    }
    for (int e = tid; e < n; e += 256) {
        if (a.x_out) ((gptr)a.x_out)[b * n + e] = xc[e];
        if (a.xh_out) ((gptr)a.xh_out)[b * n + e] = xh[e];
        if (a.Xbar && a.x0_next)
            ((gptr)a.Xbar)[(b * (size_t)a.rows_x + a.row0_x - 1 + a.n_keep) * n + e] = ((cgptr)a.x0_next)[b * n + e];
    }
}

}  // namespace

struct srompc_loop : MpcLoopCore {
    srompc *ctrl = nullptr;
    stpwl *plant = nullptr;
    int ny = 0, nzc = 0;                // the controller's measurement width and the width of its output map (the Z record)
    int j_end = 0;
    double th_end = 0.0;
    // cst: [F B L]^T | d | K | C | y_ref | H (re-formed from the controller's host copies at every reset); xreq: the next request's state
    srh::DevBuf cst, xreq;
    LoopRec UBrec, XBrec, XPd;          // records u_bar (B x S x m), x_bar (B x (S + 1) x n); input: the recorded plant (B x (S + 1) x n)
    __attribute__((always_inline)) srompc_loop() {            // (inlined: no constructor among the library's dynamic symbols)
        recs.push_back(&XBrec); recs.push_back(&UBrec);
        ins.push_back(&XPd);
    }
    ~srompc_loop() { drain(); }
    size_t cst_doubles() const { return (size_t)(n + m + ny) * n + n + (size_t)m * n + (size_t)ny * n + ny + (size_t)nzc * n; }
    // [F B L]^T and the rest from the controller's host copies, as they stand now (blocking: reset path)
    int upload_consts() {
        std::vector<double> c(cst_doubles(), 0.0);
        double *Mt = c.data(), *dv = Mt + (size_t)(n + m + ny) * n, *K = dv + n, *Cm = K + (size_t)m * n, *yr = Cm + (size_t)ny * n, *Hz = yr + ny;
        for (int i = 0; i < n; ++i) {
            for (int q = 0; q < n; ++q) Mt[(size_t)q * n + i] = ctrl->fold(i, q);
            for (int q = 0; q < m; ++q) Mt[(size_t)(n + q) * n + i] = ctrl->B[(size_t)i * m + q];
            for (int q = 0; q < ny; ++q) Mt[(size_t)(n + m + q) * n + i] = ctrl->L[(size_t)i * ny + q];
        }
        std::copy(ctrl->d.begin(), ctrl->d.end(), dv);
        std::copy(ctrl->K.begin(), ctrl->K.end(), K);
        std::copy(ctrl->C.begin(), ctrl->C.end(), Cm);
        std::copy(ctrl->yref.begin(), ctrl->yref.end(), yr);
        const std::vector<double> &Ho = ctrl->has_H ? ctrl->H : ctrl->C;
        std::copy(Ho.begin(), Ho.end(), Hz);
        SRH_CHECK_HIP(hipMemcpy(cst.p, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice));
        return SRH_OK;
    }
    RlAdvArgs adv_args() const {
        RlAdvArgs a{};
        a.N = N; a.n_keep = n_keep; a.n = n; a.m = m; a.ny = ny; a.nz = nzc;
        a.Mt = cst.as<double>();
        a.dv = a.Mt + (size_t)(n + m + ny) * n; a.K = a.dv + n; a.C = a.K + (size_t)m * n; a.yref = a.C + (size_t)ny * n; a.Hz = a.yref + ny;
        a.js = js.as<int32_t>(); a.theta = theta.as<double>();
        a.B = B;
        return a;
    }
    // the chain: row 0 pinned to the request, zero inputs behind a failed first solve, the next request read off the plan
    ShiftArgs shift_args() const {
        ShiftArgs c{};
        c.N = N; c.n = n; c.m = m; c.pin_row0 = 1; c.j_end = j_end; c.th_end = th_end;
        return c;
    }
    int launch_advance(const RlAdvArgs &a) const {
        rompc_loop_advance_kernel<<<(unsigned)B, 256, lds, stream>>>(a.plant ? plant->view() : TpwlDev{}, a);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
};

extern "C" {

int srompc_loop_create(srompc_loop_t **out, srompc_t *ctrl, const slocp_problem *prob, const double *A_mpc, const double *B_mpc,
                       const double *d_mpc, double dt_mpc, stpwl_t *plant, double dt_sim, int n_replan, int64_t max_steps_per_run) {
    SRH_REQUIRE(out && ctrl && prob && A_mpc && B_mpc && d_mpc, "srompc_loop_create: null argument");
    *out = nullptr;
    const int N = prob->N, n = ctrl->n, m = ctrl->m, ny = ctrl->ny;
    const int64_t B = ctrl->batch;
    SRH_REQUIRE(N >= 1 && dt_mpc > 0.0, "srompc_loop_create: need a horizon N >= 1 and dt_mpc > 0");
    SRH_REQUIRE(prob->n_x == n && prob->n_u == m, "srompc_loop_create: the QP has n_x = %d, n_u = %d, the controller n_x = %d, n_u = %d", prob->n_x,
                prob->n_u, n, m);
    int rc;
    if ((rc = MpcLoopCore::check_problem("srompc_loop_create", prob, m))) return rc;
    SRH_REQUIRE(n <= 128, "srompc_loop_create: n_x = %d exceeds the limit n_x <= 128 of the advance kernel", n);
    if (plant) {
        SRH_REQUIRE(plant->n == n && plant->m == m, "srompc_loop_create: the plant has n_x = %d, n_u = %d, the controller n_x = %d, n_u = %d", plant->n,
                    plant->m, n, m);
        SRH_REQUIRE(plant->has_discrete, "srompc_loop_create: the plant has not been pre-discretised at dt_sim");
    }
    if ((rc = loop_check_periods("srompc_loop_create", N, dt_mpc, dt_sim, n_replan, max_steps_per_run))) return rc;
    const size_t lds = rl_advance_lds_bytes(n, m, ny, plant != nullptr);
    SRH_REQUIRE(lds <= (size_t)160 * 1024, "srompc_loop_create: the advance kernel needs %zu bytes of LDS (160 KiB available)", lds);
    srompc_loop *h = new srompc_loop();
    auto fail = [&](int code) { delete h; return code; };
    h->ctrl = ctrl; h->plant = plant; h->ny = ny; h->nzc = ctrl->nz; h->lds = lds;
    const char *what = "set up the advance kernel / the stream";
    if (hipFuncSetAttribute((const void *)rompc_loop_advance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return fail(loop_setup_failed("srompc_loop_create", what));
    const size_t D = sizeof(double), Bz = (size_t)B;
    h->XHrec.shape(D * n, 1); h->Yrec.shape(D * ny, 0); h->Vd.shape(D * ny, 0);
    h->UBrec.shape(D * m, 0); h->XBrec.shape(D * n, 1); h->XPd.shape(D * n, 1);
    if ((rc = h->setup("srompc_loop_create", what, N, n, m, prob->n_z, B, dt_mpc, dt_sim, n_replan, max_steps_per_run, (size_t)ctrl->nz)) ||
        (rc = h->alloc_recs({&h->XHrec, &h->Yrec, &h->UBrec, &h->XBrec})) || (rc = h->cst.alloc(D * h->cst_doubles())) ||
        (rc = h->xreq.alloc(D * Bz * n)) || (rc = h->make_horizon("srompc_loop_create", prob, A_mpc, B_mpc, d_mpc)))
        return fail(rc);
    {
        // where the period ends in the plan: the schedule's rule for tau = n_replan dt_sim, every product and sum rounded on its own
#pragma clang fp contract(off)
        const double tau = (double)n_replan * dt_sim;
        const double q = tau / dt_mpc;
        h->j_end = std::min((int)q, N - 1);
        const double back = (double)h->j_end * dt_mpc;
        h->th_end = (tau - back) / dt_mpc;
    }
    h->Xrec.row0 = h->xcur.p; h->XHrec.row0 = ctrl->est();
    *out = h;
    return SRH_OK;
}

int srompc_loop_destroy(srompc_loop_t *h) {
    delete h;
    return SRH_OK;
}

int srompc_loop_set_target(srompc_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase) {
    return loop_set_target(h, "srompc_loop_set_target", T, t, z, u_des, phase);
}

int srompc_loop_reset(srompc_loop_t *h, const double *x0, const double *x_hat0, double t_start) {
    SRH_REQUIRE(h && x0, "srompc_loop_reset: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipStreamSynchronize(h->ctrl->stream));
    h->have_state = false;
    const size_t bytes = sizeof(double) * (size_t)h->B * h->n;
    const double *xh = x_hat0 ? x_hat0 : x0;
    SRH_CHECK_HIP(hipMemcpy(h->xcur.p, x0, bytes, hipMemcpyHostToDevice));
    SRH_CHECK_HIP(hipMemcpy(h->ctrl->est(), xh, bytes, hipMemcpyHostToDevice));
    SRH_CHECK_HIP(hipMemcpy(h->xreq.p, xh, bytes, hipMemcpyHostToDevice));          // the first request starts from the estimate
    int rc = h->upload_consts();
    if (rc) return rc;
    h->t_start = t_start; h->k = 0; h->have_state = true;
    return SRH_OK;
}

int srompc_loop_run(srompc_loop_t *h, int periods, const double *W, const double *V, const double *X_plant, double *X, double *XH, double *Y,
                    double *Z, double *U, double *Ubar, double *Xbar, double *J, int32_t *status, int32_t *iters) {
    SRH_REQUIRE(h, "srompc_loop_run: null handle");
    SRH_REQUIRE(periods >= 1, "srompc_loop_run: periods must be positive");
    SRH_REQUIRE(h->have_state, "srompc_loop_run: no plant state and estimate yet (call srompc_loop_reset first)");
    SRH_REQUIRE(h->plant || X_plant, "srompc_loop_run: the loop was created without a plant (replay only): X_plant is required");
    h->Wd.host = (void *)W; h->Vd.host = (void *)V; h->XPd.host = (void *)X_plant;
    h->Xrec.host = X; h->XHrec.host = XH; h->Yrec.host = Y; h->Zrec.host = Z; h->Urec.host = U; h->UBrec.host = Ubar; h->XBrec.host = Xbar;
    h->Jrec.host = J; h->Srec.host = status; h->Irec.host = iters;
    const bool replay = X_plant != nullptr;
    double *xcur = h->xcur.as<double>(), *est = h->ctrl->est();
    // the request starts from xreq (the estimate of the reset, then the plan's end); no output map for the prepare kernel: row 0 of X and
    // XH is where the loops stand (LoopRec::row0), row 0 of Z the advance kernel's
    const PrepUnit u{h->xreq.as<double>(), nullptr, nullptr, h->zf_dev(), false};
    return loop_run_periods(h, "srompc_loop_run", periods, u, [&](int p, const PrepArgs &a, const LoopRows &r) -> int {
        int rc;
        if ((rc = h->solve(p, a))) return rc;
        ShiftArgs c = h->shift_args();
        h->shift_in_place(c, p, a);
        c.x0_next = h->xreq.as<double>();
        if ((rc = h->launch_shift(c))) return rc;
        h->take_solution();
        RlAdvArgs v = h->adv_args();
        v.plant = replay ? 0 : 1; v.z0 = p == 0 ? 1 : 0;
        v.xopt = h->xopt.as<double>(); v.uopt = h->uopt.as<double>();
        v.W = (W && !replay) ? h->Wd.as<double>() : nullptr; v.Vn = V ? h->Vd.as<double>() : nullptr; v.w_step0 = r.w_step0;
        v.Xp = replay ? h->XPd.as<double>() : nullptr;
        v.x_in = xcur; v.xh_in = est; v.x_out = xcur; v.xh_out = est; v.x0_next = h->xreq.as<double>();
        v.X = X ? h->Xrec.as<double>() : nullptr; v.XH = XH ? h->XHrec.as<double>() : nullptr; v.Z = Z ? h->Zrec.as<double>() : nullptr;
        v.Xbar = Xbar ? h->XBrec.as<double>() : nullptr; v.Y = Y ? h->Yrec.as<double>() : nullptr; v.U = U ? h->Urec.as<double>() : nullptr;
        v.Ubar = Ubar ? h->UBrec.as<double>() : nullptr;
        v.rows_x = r.rows_x; v.row0_x = r.row0_x; v.rows_u = r.rows_u; v.row0_u = r.row0_u;
        return h->launch_advance(v);
    });
}

int srompc_loop_last_inputs(srompc_loop_t *h, double *x0, double *z, double *zf, double *u_des) {
    return mpc_last_inputs(h, "srompc_loop_last_inputs", x0, z, zf, u_des);
}

int srompc_loop_last_plan(srompc_loop_t *h, double *xopt, double *uopt) { return loop_last_plan(h, "srompc_loop_last_plan", xopt, uopt); }

int srompc_loop_stats(srompc_loop_t *h, int64_t *steps, int64_t *waits_last_run) { return loop_stats(h, "srompc_loop_stats", steps, waits_last_run); }

int srompc_loop_chain(srompc_loop_t *h, const double *xopt_prev, const double *uopt_prev, const double *xopt, const double *uopt, const double *x0,
                      const int32_t *status, int first, double *xopt_out, double *uopt_out, double *x0_next) {
    SRH_REQUIRE(h && xopt && uopt && x0 && status && xopt_out && uopt_out && x0_next, "srompc_loop_chain: null argument");
    SRH_REQUIRE(first || (xopt_prev && uopt_prev), "srompc_loop_chain: the previous plan is required behind the first period");
    return mpc_shift_alone(h, h->shift_args(), xopt_prev, uopt_prev, xopt, uopt, x0, status, first, xopt_out, uopt_out, x0_next);
}

int srompc_loop_advance(srompc_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *x_hat, const double *W,
                        const double *V, const double *X_plant, double *X, double *XH, double *Y, double *Z, double *U, double *Ubar, double *Xbar) {
    SRH_REQUIRE(h && xopt && uopt && x && x_hat && X && XH && Y && Z && U && Ubar && Xbar, "srompc_loop_advance: null argument");
    SRH_REQUIRE(h->plant || X_plant, "srompc_loop_advance: the loop was created without a plant (replay only): X_plant is required");
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m, nz = h->nzc, ny = h->ny, nk = h->n_keep;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc;
    if ((rc = h->upload_consts())) return rc;
    srh::DevBuf dxo, duo, dx, dxh, dW, dV, dXp, dX, dXH, dY, dZ, dU, dUb, dXb;
    // X, XH, Z and X_plant carry a row in front (row 0: where the launch starts), as the records of a run do; it is not copied back
    if ((rc = dxo.upload(xopt, D * B * (N + 1) * n)) || (rc = duo.upload(uopt, D * B * N * m)) || (rc = dx.upload(x, D * B * n)) ||
        (rc = dxh.upload(x_hat, D * B * n)) || (W && (rc = dW.upload(W, D * nk * B * n))) || (V && (rc = dV.upload(V, D * nk * B * ny))) ||
        (X_plant && (rc = dXp.upload(X_plant, D * B * (nk + 1) * n))) || (rc = dX.alloc(D * B * (nk + 1) * n)) ||
        (rc = dXH.alloc(D * B * (nk + 1) * n)) || (rc = dY.alloc(D * B * nk * ny)) || (rc = dZ.alloc(D * B * (nk + 1) * nz)) ||
        (rc = dU.alloc(D * B * nk * m)) || (rc = dUb.alloc(D * B * nk * m)) || (rc = dXb.alloc(D * B * (nk + 1) * n)))
        return rc;
    RlAdvArgs v = h->adv_args();
    v.plant = X_plant ? 0 : 1; v.z0 = 1;
    v.xopt = dxo.as<double>(); v.uopt = duo.as<double>();
    v.W = (W && !X_plant) ? dW.as<double>() : nullptr; v.Vn = V ? dV.as<double>() : nullptr; v.w_step0 = 0;
    v.Xp = X_plant ? dXp.as<double>() : nullptr;
    v.x_in = dx.as<double>(); v.xh_in = dxh.as<double>();
    v.X = dX.as<double>(); v.XH = dXH.as<double>(); v.Z = dZ.as<double>(); v.Xbar = dXb.as<double>();
    v.Y = dY.as<double>(); v.U = dU.as<double>(); v.Ubar = dUb.as<double>();
    v.rows_x = (int64_t)nk + 1; v.row0_x = 1; v.rows_u = (int64_t)nk; v.row0_u = 0;
    if ((rc = loop_wait(h->launch_advance(v), h->stream))) return rc;
    // rows 1 .. n_keep of the S + 1 row blocks (rows 0 .. n_keep - 1 of Xbar) -> the caller's (B x n_keep x .) arrays
    auto rows = [&](const srh::DevBuf &d, double *dst, size_t w, size_t skip) { return loop_rows_to_host(d, dst, B, nk, D * w, skip); };
    if ((rc = rows(dX, X, n, 1)) || (rc = rows(dXH, XH, n, 1)) || (rc = rows(dZ, Z, nz, 1)) || (rc = rows(dXb, Xbar, n, 0)) ||
        (rc = dY.download(Y, D * B * nk * ny)) || (rc = dU.download(U, D * B * nk * m)) || (rc = dUb.download(Ubar, D * B * nk * m)))
        return rc;
    return SRH_OK;
}

}  // extern "C"
