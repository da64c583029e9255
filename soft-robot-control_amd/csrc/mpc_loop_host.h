// What the two linear MPC loops (rompc_loop.hip, koopman_loop.hip) share beyond gusto_loop_host.h, stated once: the QP with a constant
// horizon (MpcLoopCore: the plan handle, the (A, B, d) tiled over B x N, the buffers the solve writes, the resident solve call and the
// swap behind it), THE PLAN SHIFT of a member whose solve failed (loop_plan_shift_kernel and the stand-alone entry around it), and the
// copy of a stand-alone advance's (n_keep + 1)-row blocks to the caller.  Included by those two units only.
#pragma once
#include "gusto_loop_host.h"

namespace {

// `count` copies of src (len) behind one another: the constant horizon of the QP
__global__ __launch_bounds__(256) void loop_tile_kernel(const double *src, int64_t len, int64_t count, double *dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + SRH_TID;
    if (e < len * count) dst[e] = src[e % len];
}

struct ShiftArgs {
    int N, n, m, first;
    int pin_row0;                       // 1: row 0 of the states is the request's x0 whatever the solve says
    int j_end;                          // interval and position in the plan of the next request's state (x0_next only)
    double th_end;
    const double *xprev, *uprev;        // the plan as the previous period left it (B x (N+1) x n), (B x N x m); not read when first
    const double *xsol, *usol;          // the QP's answer (may be xout / uout: every element is read by the thread that writes it)
    const double *x0;                   // (B x n) the request's state
    const double *u_idle, *uoff, *ufac; // (m) each or null: the idle input (null: 0.0) and the scaling it is taken through (null: as given)
    const int32_t *status;              // (B) the QP's status words
    double *xout, *uout;                // the plan of this period
    double *x0_next;                    // (B x n) the next request's state, or null: not formed
    double *xlift;                      // (B x n) the period's row of the request record, or null
};

// THE PLAN SHIFT (ros.py:223-227).  One workgroup of 256 per member.  Every element of the plan as it stands behind the kernel is a
// function of the inputs alone; with failed = status[b] != 0:
//   state_at(k, c) = not failed:           (pin_row0 && k == 0) ? x0[c] : xsol[k][c]
//                    failed, first period: x0[c]
//                    failed, later period: (pin_row0 && k == 0) ? x0[c] : xprev[min(k + 1, N)][c]      one row up, the last row held
//   input_at(k, c) = not failed:           usol[k][c]
//                    failed, first period: the idle input: 0.0 without u_idle, u_idle[c] without uoff, else (u_idle[c] - uoff[c]) / ufac[c]
//                                          (the two operations of scale_down, koopman_utils.py:98-101, each rounded on its own)
//                    failed, later period: uprev[min(k + 1, N - 1)][c]
//   x0_next[c] = lerp(state_at(j_end, c), state_at(j_end + 1, c), th_end)        the plan point of gusto_loop_prep.h
//   xlift[b][c] = x0[c]
// The copies and x0_next are formed from the same values and nothing is read back.  Every value of a pass is formed before the pass's
// first store: xsol may be xout (the loops run it in place), and then rows >= 1 are written with the value read.
__global__ __launch_bounds__(256) void loop_plan_shift_kernel(ShiftArgs a) {
    const size_t b = blockIdx.x;
    const int N = a.N, n = a.n, m = a.m, tid = SRH_TID;
    cgptr xs = (cgptr)a.xsol + b * (size_t)(N + 1) * n, us = (cgptr)a.usol + b * (size_t)N * m;
    cgptr xp = (cgptr)a.xprev + b * (size_t)(N + 1) * n, up = (cgptr)a.uprev + b * (size_t)N * m;
    cgptr x0 = (cgptr)a.x0 + b * n;
    cgptr ui = (cgptr)a.u_idle, uoff = (cgptr)a.uoff, ufac = (cgptr)a.ufac;
    const bool failed = ((cgiptr)a.status)[b] != 0, first = a.first != 0, pin = a.pin_row0 != 0;
    auto state_at = [&](int k, int c) -> double {
        if ((pin && k == 0) || (failed && first)) return x0[c];
        return failed ? xp[(size_t)min(k + 1, N) * n + c] : xs[(size_t)k * n + c];
    };
    auto input_at = [&](int k, int c) -> double {
        if (!failed) return us[(size_t)k * m + c];
        if (!first) return up[(size_t)min(k + 1, N - 1) * m + c];
        if (ui == nullptr) return 0.0;
        return uoff == nullptr ? ui[c] : (ui[c] - uoff[c]) / ufac[c];
    };
    gptr xo = (gptr)a.xout + b * (size_t)(N + 1) * n, uo = (gptr)a.uout + b * (size_t)N * m;
    for (int e0 = 0; e0 < (N + 1) * n; e0 += 256) {
        const int e = e0 + tid;
        double v = 0.0;
        if (e < (N + 1) * n) v = state_at(e / n, e % n);
        if (e < (N + 1) * n) xo[e] = v;
    }
    for (int e0 = 0; e0 < N * m; e0 += 256) {
        const int e = e0 + tid;
        double v = 0.0;
        if (e < N * m) v = input_at(e / m, e % m);
        if (e < N * m) uo[e] = v;
    }
    if (a.x0_next)
        for (int c = tid; c < n; c += 256) ((gptr)a.x0_next)[b * n + c] = lerp(state_at(a.j_end, c), state_at(a.j_end + 1, c), a.th_end);
    if (a.xlift)
        for (int c = tid; c < n; c += 256) ((gptr)a.xlift)[b * n + c] = x0[c];
}

struct MpcLoopCore : LoopCore {
    slocp_plan_t *qp = nullptr;
    bool has_Qzf = false, horizon_resident = false;
    // Ah, Bh, dh: the QP's constant horizon tiled over B x N; zero: B zeros (the QP's delta and omega); xalt, ualt: the plan the solve
    // writes (swapped with xopt, uopt behind the shift kernel); zf: the terminal target
    srh::DevBuf Ah, Bh, dh, zero, xalt, ualt, zf;
    ~MpcLoopCore() {
        drain();
        if (qp) slocp_plan_destroy(qp);
    }
    // what the resident loop refuses of a QP (m: the controller's inputs); the widths against the controller are the unit's own check
    static int check_problem(const char *who, const slocp_problem *prob, int m_) {
        SRH_REQUIRE(!prob->tr_active, "%s: the MPC QP has no trust region (is_tr_active=False, baselines/ros.py:161)", who);
        SRH_REQUIRE(prob->ndU == 0, "%s: input-rate rows (dU) are not offered by the resident loop", who);
        SRH_REQUIRE(m_ <= 16, "%s: n_u = %d exceeds the limit n_u <= 16 of the advance kernel", who, m_);
        return SRH_OK;
    }
    // Behind setup(): the QP plan, its buffers, and the constant (A, B, d) tiled over B x N once (d null: zeros); waits for the stream
    int make_horizon(const char *who, const slocp_problem *prob, const double *A, const double *Bm, const double *d) {
        const size_t D = sizeof(double), Bz = (size_t)B, Nz = (size_t)N;
        has_Qzf = prob->Qzf != nullptr;
        srh::DevBuf a1, b1, d1;
        int rc;
        if ((rc = slocp_plan_create(&qp, prob, B)) || (rc = Ah.alloc(D * Bz * Nz * n * n)) || (rc = Bh.alloc(D * Bz * Nz * n * m)) ||
            (rc = dh.alloc(D * Bz * Nz * n)) || (rc = zero.alloc(D * Bz)) || (rc = xalt.alloc(D * Bz * (Nz + 1) * n)) ||
            (rc = ualt.alloc(D * Bz * Nz * m)) || (rc = zf.alloc(D * Bz * prob->n_z)) || (rc = a1.upload(A, D * n * n)) ||
            (rc = b1.upload(Bm, D * n * m)) || (d && (rc = d1.upload(d, D * n))))
            return rc;
        const int64_t cnt = B * N;
        loop_tile_kernel<<<(unsigned)srh::cdiv(cnt * n * n, 256), 256, 0, stream>>>(a1.as<double>(), (int64_t)n * n, cnt, Ah.as<double>());
        loop_tile_kernel<<<(unsigned)srh::cdiv(cnt * n * m, 256), 256, 0, stream>>>(b1.as<double>(), (int64_t)n * m, cnt, Bh.as<double>());
        if (d) loop_tile_kernel<<<(unsigned)srh::cdiv(cnt * n, 256), 256, 0, stream>>>(d1.as<double>(), (int64_t)n, cnt, dh.as<double>());
        if (hipGetLastError() != hipSuccess || (!d && hipMemsetAsync(dh.p, 0, D * Bz * Nz * n, stream) != hipSuccess) ||
            hipMemsetAsync(zero.p, 0, D * Bz, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
            return loop_setup_failed(who, "tile the horizon");
        return SRH_OK;
    }
    // period p's solve from the prepare kernel's arguments, all members in one launch.  It writes (xalt, ualt): (xopt, uopt) still hold
    // the previous period's plan for the shift.
    int solve(int p, const PrepArgs &a) {
        const size_t o = (size_t)p * (size_t)B;
        int rc = slocp_plan_solve_dev_resident(qp, horizon_resident ? 0 : 1, Ah.as<double>(), Bh.as<double>(), dh.as<double>(), a.x0, nullptr,
                                               zero.as<double>(), zero.as<double>(), has_z ? a.z : nullptr, a.zf, has_ud ? a.ud : nullptr,
                                               xalt.as<double>(), ualt.as<double>(), nullptr, Jrec.as<double>() + o, Srec.as<int32_t>() + o,
                                               Irec.as<int32_t>() + o, (void *)stream);
        if (rc) return rc;
        horizon_resident = true;
        return SRH_OK;
    }
    // the arguments of the shift of period p inside a run: in place on what the solve wrote
    void shift_in_place(ShiftArgs &c, int p, const PrepArgs &a) const {
        c.first = a.first;
        c.xprev = xopt.as<double>(); c.uprev = uopt.as<double>();
        c.xsol = xalt.as<double>(); c.usol = ualt.as<double>();
        c.x0 = a.x0; c.status = Srec.as<int32_t>() + (size_t)p * (size_t)B;
        c.xout = xalt.as<double>(); c.uout = ualt.as<double>();
    }
    int launch_shift(const ShiftArgs &c) const {
        loop_plan_shift_kernel<<<(unsigned)B, 256, 0, stream>>>(c);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    // behind the shift: the plan of this period becomes (xopt, uopt) (same sizes; the launches hold the pointers they were given)
    void take_solution() {
        std::swap(xopt.p, xalt.p);
        std::swap(uopt.p, ualt.p);
    }
    double *zf_dev() const { return (has_z && has_Qzf) ? zf.as<double>() : nullptr; }          // the terminal target of a run, or none
};

// last_inputs of the last period's solve: the common blocks, then zf (B x nz) when the run formed one
int mpc_last_inputs(MpcLoopCore *h, const char *who, double *x0, double *z, double *zf, double *u_des) {
    int rc = loop_last_inputs(h, who, x0, nullptr, nullptr, z, u_des);
    if (rc) return rc;
    if (zf && h->zf_dev() && (rc = h->zf.download(zf, sizeof(double) * h->B * h->nz))) return rc;
    return SRH_OK;
}

// The shift kernel alone on host arrays (srompc_loop_chain, skoop_loop_fixup): c holds the unit's constants; x0_next may be null
int mpc_shift_alone(MpcLoopCore *h, ShiftArgs c, const double *xopt_prev, const double *uopt_prev, const double *xopt, const double *uopt,
                    const double *x0, const int32_t *status, int first, double *xopt_out, double *uopt_out, double *x0_next) {
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m;
    srh::DevBuf dxp, dup, dxs, dus, dx0, dst, dxo, duo, dxn;
    int rc;
    if ((xopt_prev && (rc = dxp.upload(xopt_prev, D * B * (N + 1) * n))) || (uopt_prev && (rc = dup.upload(uopt_prev, D * B * N * m))) ||
        (rc = dxs.upload(xopt, D * B * (N + 1) * n)) || (rc = dus.upload(uopt, D * B * N * m)) || (rc = dx0.upload(x0, D * B * n)) ||
        (rc = dst.upload(status, sizeof(int32_t) * B)) || (rc = dxo.alloc(D * B * (N + 1) * n)) || (rc = duo.alloc(D * B * N * m)) ||
        (x0_next && (rc = dxn.alloc(D * B * n))))
        return rc;
    c.first = first ? 1 : 0;
    // (a first period never reads the previous plan: the solve's arrays stand in for the missing pointers)
    c.xprev = xopt_prev ? dxp.as<double>() : dxs.as<double>(); c.uprev = uopt_prev ? dup.as<double>() : dus.as<double>();
    c.xsol = dxs.as<double>(); c.usol = dus.as<double>(); c.x0 = dx0.as<double>(); c.status = dst.as<int32_t>();
    c.xout = dxo.as<double>(); c.uout = duo.as<double>(); c.x0_next = x0_next ? dxn.as<double>() : nullptr; c.xlift = nullptr;
    if ((rc = loop_wait(h->launch_shift(c), h->stream))) return rc;
    if ((rc = dxo.download(xopt_out, D * B * (N + 1) * n)) || (rc = duo.download(uopt_out, D * B * N * m)) ||
        (x0_next && (rc = dxn.download(x0_next, D * B * n))))
        return rc;
    return SRH_OK;
}

// Rows skip .. skip + n_keep - 1 of a (B x (n_keep + 1) x w) device block -> the caller's (B x n_keep x w) array; w in bytes.  The
// records of a stand-alone advance carry a row in front (row 0: where the launch starts), as those of a run do; skip = 1 leaves it out.
int loop_rows_to_host(const srh::DevBuf &d, void *dst, size_t B, size_t n_keep, size_t w, size_t skip) {
    SRH_CHECK_HIP(hipMemcpy2D(dst, n_keep * w, (const char *)d.p + skip * w, (n_keep + 1) * w, n_keep * w, B, hipMemcpyDeviceToHost));
    return SRH_OK;
}

}  // namespace
