// What the SCP kernels (scp.hip, gusto.hip, lean.hip, gusto_ssm.hip) share: kernel argument blocks, the layouts of a rollout's work block and
// of a plan's pinned block, GuSTO's step rule -- the (J, delta, omega) state machine of every GuSTO kernel and of the host replay
// (sgusto_rule_replay), stated ONCE here; how a kernel walks its data to the numbers the rule judges is tuning and stays in the kernel --
// with the TPWL kernels' hand-over record, and the launch entry points of lean.hip (its own translation unit: the variants compile in parallel).
#pragma once
#include "scp_host.h"

struct GustoPar {
    double delta0, omega0, rho, beta_fail, gamma_fail, epsilon, omega_max, convg_thresh, dt;
    int max_iters, max_trace;
    int warm_across;                    // 1: the first QP of a solve starts from the minimiser / multipliers the rollout's PREVIOUS solve left
                                        // (the reference's `warm_start=True`: its cvxpy problem keeps the solver state between solves, locp.py:181)
    int poison_warm;                    // test knobs of the lean kernel, read when the plan is created.  bit 0 (SRH_LEAN_POISON_WARM=1): every warm-started
                                        // QP fails and is repeated cold; bits 4.. (SRH_LEAN_FORCE_HANDOVER=k): k + 1, SCP iteration k is handed to the fused kernel
                                        // bit 1 (SRH_GUSTO_TRACE_QIT=1): trace slot 3 = interior-point iterations; bit 2 (SRH_LEAN_SERIAL_WAVE=1): the half-size
                                        // lean workgroup picks its serial wave by its wave slot (ql::serial_wave_pick; measured: see DESIGN.md section 15)
    int warm_full;                      // fused kernel, OFF unless SRH_GUSTO_WARM_FULL=1 at plan creation: a full (trust-region-active) QP behind a rejected
                                        // step starts from the previous one's (u, s, lambda).  Built and measured in round 6: the
                                        // uncapped tail's full QPs keep their 18-40 interior-point iterations -- the active set of the slack rows moves with
                                        // every omega x 5 -- so the default stays the cold start
};

// GustoPar of a plan from the API's parameters, with the one debug knob both GuSTO plans read (SRH_GUSTO_TRACE_QIT); the TPWL
// plan ORs in its own test knobs
inline GustoPar gusto_par(const sgusto_params *p, double dt, int max_trace) {
    return GustoPar{p->delta0, p->omega0, p->rho, p->beta_fail, p->gamma_fail, p->epsilon, p->omega_max, p->convg_thresh, dt,
                    p->max_gusto_iters, max_trace, 0, getenv("SRH_GUSTO_TRACE_QIT") != nullptr ? 2 : 0, 0};
}

struct GustoBatch {
    const double *x0, *u_init, *x_init, *z, *zf, *ud;
    const double *fs;                   // 1/|f_char| (n)
    double *xopt, *uopt, *zopt;
    int32_t *iters, *status;
    double *trace;
    double *work;                       // per problem: [qp work | xk | uk | acc | ints | resume record | condensed block]
    size_t work_stride;
    const int32_t *order;               // workgroup -> rollout (longest expected solve first), or null
    int32_t *last_iters;                // SCP iterations of this solve per rollout: the next solve's dispatch key
    int mode;                           // fused kernel: 0 = solve every rollout, 2 = only those a lean launch handed over
    int32_t *handed_over;               // lean kernel: counts the rollouts it hands to the fused kernel (or null)
    double *Jopt;                       // per rollout: LOCP optimal value of the solution returned (the last accepted step), or null
    int host_args;                      // x0, z, zf, ud point into pinned host memory (zero-copy solve): the kernels keep copies in the work block
};

struct LocpBatch {
    const double *Ad, *AdT, *Bd, *BdT, *dd;     // (batch x N x ...)
    const double *x0, *xk, *delta, *omega, *z, *zf, *ud;
    double *x, *u, *s, *J;
    int32_t *status, *iters;
    double *work;
    size_t work_stride;
    double *dbg;
    int only_pending;                   // fused kernel: 1 = only the problems a lean launch left with status LEAN_PENDING
    int32_t *handed_over;               // lean kernel: counts the QPs it hands to the fused kernel (or null)
};

namespace {

constexpr int LEAN_PENDING = -77;       // status of a QP / rollout the lean kernel hands to the fused kernel
constexpr int SSM_NEEDS_HOST = -78;     // status of a rollout the SSM kernel returns unsolved: rate rows present and the trust region binding (gusto_ssm.hip)
constexpr int GUSTO_REC = 10;           // doubles of the TPWL kernels' resume record behind the SCP loop's index arrays; its slots:
enum GustoRecSlot {
    REC_PENDING = 0,                    // 1.0: the lean kernel handed this rollout over, the slots below hold its SCP state
    REC_DELTA, REC_OMEGA, REC_J_PREV, REC_D_PREV, REC_O_PREV, REC_ITR,
    REC_QP_STATUS,                      // status of the QP the lean kernel stopped at (100.0: relaxed minimiser outside the trust region)
    REC_WARM                            // 1.0: the work block holds a converged lean QP of the previous solve (GustoPar::warm_across)
};
constexpr int SSM_REC_WARM = 0;         // the SSM kernel's own record (gusto_ssm.hip: SsmGustoWork::rec) has this one slot, meaning as REC_WARM

// ---- GuSTO's step rule (sofacontrol/scp/gusto.py:371-428; reads like GuSTO._judge of sofacontrol_amd/scp/gusto.py).  Plain scalars, no
// LDS, no barriers of its own.  A kernel's loop: gusto_start; while (gusto_running) { QP; md = max_k |x_scale (x_k - xbar_k)|_inf;
// gusto_inside ? gusto_judge : gusto_outside; trace row; ++itr; move the linearisation point if accepted }; gusto_final_status.
#define SRH_RULE __host__ __device__ __forceinline__
// radius and penalty of the next QP; (J, delta, omega) of the last accepted step; QPs solved so far
struct GustoState { double delta, omega, J_prev, d_prev, o_prev; int itr; bool converged; };
SRH_RULE GustoState gusto_start(const GustoPar &par) { return GustoState{par.delta0, par.omega0, INFINITY, INFINITY, INFINITY, 0, false}; }
SRH_RULE bool gusto_running(const GustoPar &par, const GustoState &s) { return s.itr <= par.max_iters && !s.converged && s.omega <= par.omega_max; }
SRH_RULE bool gusto_inside(const GustoPar &par, const GustoState &s, double md) { return !(md - s.delta > par.epsilon); }      // gusto.py:174-183
// the minimiser used the whole trust region: if the step is rejected the next QP (same linearisation point) is certain to bind (tr_hot)
SRH_RULE bool gusto_on_boundary(const GustoState &s, double md) { return md >= s.delta * (1.0 - 1e-9); }
SRH_RULE void gusto_outside(const GustoPar &par, GustoState &s) { s.omega = par.gamma_fail * s.omega; }       // harder penalty, same QP data
// A step inside the trust region: accepted (true) or not.  viol() = the largest state-constraint violation (gusto.py:185-201), dsum() =
// sum_k |x_scale (x_k - xbar_k)|_2 (gusto.py:150-161): callables, evaluated on the accept path only and in this order -- the kernels'
// contain workgroup reductions, which every thread reaches because the rule is uniform over the workgroup.
template <class Viol, class Dsum>
SRH_RULE bool gusto_judge(const GustoPar &par, GustoState &s, double J, double rho_k, int N, int n, Viol &&viol, Dsum &&dsum) {
    bool new_solution = false;
    if (rho_k > par.rho && s.itr != 1) {
        s.delta = par.beta_fail * s.delta;               // model too inaccurate over this step: shrink, same QP data
    } else {
        if (s.d_prev == s.delta && s.o_prev == s.omega && s.J_prev <= J) s.delta = par.beta_fail * s.delta;
        s.d_prev = s.delta; s.J_prev = J; s.o_prev = s.omega;
        const bool X_ok = !(viol() > par.epsilon);
        if (!X_ok) s.omega = par.gamma_fail * s.omega;
        const double dsol = (1.0 / N) * ((1.0 / n) * dsum());
        s.converged = (dsol <= par.convg_thresh) && X_ok;
        new_solution = true;
    }
    return new_solution;
}
// status of a solve whose loop ended: a QP failure (1) stands, else 2 = omega > omega_max, 3 = max iterations
SRH_RULE int gusto_final_status(const GustoPar &par, const GustoState &s, int status) {
    if (status == 0) {
        if (s.omega > par.omega_max) status = 2;
        else if (s.itr - 1 > par.max_iters) status = 3;
    }
    return status;
}
// The lean kernel hands a rollout it cannot finish to the fused kernel (mode 2) through the resume record: the state in front of the QP it
// stopped at.  (The fused kernel carves the work block differently: nothing there to start the next solve from, REC_WARM = 0.)
__device__ __forceinline__ void gusto_rec_save(gptr rec, const GustoState &s, int qp_status) {
    rec[REC_PENDING] = 1.0; rec[REC_DELTA] = s.delta; rec[REC_OMEGA] = s.omega; rec[REC_J_PREV] = s.J_prev; rec[REC_D_PREV] = s.d_prev;
    rec[REC_O_PREV] = s.o_prev; rec[REC_ITR] = (double)s.itr; rec[REC_QP_STATUS] = (double)qp_status; rec[REC_WARM] = 0.0;
}
// false: nothing pending.  (The caller clears REC_PENDING once every thread has read the record.)
__device__ __forceinline__ bool gusto_rec_load(gptr rec, GustoState &s, int *qp_status) {
    if (rec[REC_PENDING] != 1.0) return false;
    s = GustoState{rec[REC_DELTA], rec[REC_OMEGA], rec[REC_J_PREV], rec[REC_D_PREV], rec[REC_O_PREV], (int)rec[REC_ITR], false}; *qp_status = (int)rec[REC_QP_STATUS];
    return true;
}
// The arguments of a zero-copy solve (GustoBatch::host_args) sit in pinned HOST memory, where every QP / interior-point iteration would read
// them: the kernel works on copies in the work block (x0, z, zf, ud -> x0c, zc, zfc, udc; a null argument stays null).  copy = false: an
// earlier launch made the copies.
__device__ __forceinline__ void gusto_stage_args(cgptr &x0, cgptr &zp, cgptr &zfp, cgptr &udp, gptr x0c, gptr zc, gptr zfc, gptr udc, int N, int n,
                                                 int m, int nz, bool copy, int tid, int nt) {
    if (copy) {
        for (int e = tid; e < n; e += nt) x0c[e] = x0[e];
        if (zp) for (int e = tid; e < (N + 1) * nz; e += nt) zc[e] = zp[e];
        if (zfp) for (int e = tid; e < nz; e += nt) zfc[e] = zfp[e];
        if (udp) for (int e = tid; e < N * m; e += nt) udc[e] = udp[e];
    }
    x0 = (cgptr)x0c;
    if (zp) zp = (cgptr)zc;
    if (zfp) zfp = (cgptr)zfc;
    if (udp) udp = (cgptr)udc;
}
// Row `itr` of rollout p's trace (J, delta and omega of the QP, rho_k) by thread 0; debug(row): a kernel's own debug overwrite
template <class Debug>
__device__ __forceinline__ void gusto_trace_row(const GustoPar &par, double *trace, size_t p, int itr, int tid, double J, double d_cur, double o_cur,
                                                double rho_k, Debug &&debug) {
    if (trace && itr < par.max_trace && tid == 0) {
        double *tr = trace + (p * par.max_trace + itr) * 4;
        tr[0] = J; tr[1] = d_cur; tr[2] = o_cur; tr[3] = rho_k;
        debug(tr);
    }
}
// xopt, uopt and zopt = H xopt (gusto.py:486) of rollout p from its accepted iterate; by all threads
template <class HPtr>
__device__ __forceinline__ void gusto_write_out(double *xopt, double *uopt, double *zopt, size_t p, int N, int n, int m, int nz, HPtr H, gptr xk, gptr uk, int tid, int nt) {
    __syncthreads();
    for (int e = tid; e < (N + 1) * n; e += nt) xopt[p * (size_t)(N + 1) * n + e] = xk[e];
    for (int e = tid; e < N * m; e += nt) uopt[p * (size_t)N * m + e] = uk[e];
    for (int e = tid; e < (N + 1) * nz; e += nt) {
        const int k = e / nz, a = e - k * nz;
        double v = 0.0;
        for (int j = 0; j < n; ++j) v = fma(H[a * n + j], xk[(size_t)k * n + j], v);
        zopt[p * (size_t)(N + 1) * nz + e] = v;
    }
}

// offsets (doubles) of the SCP loop's own arrays inside a rollout's work block
struct GustoWork { size_t xk, uk, acc, idx, rec, x0c, zc, zfc, udc, end; };
__host__ __device__ inline GustoWork gusto_work(const QPDims &d) {
    GustoWork g;
    const size_t N = d.N, n = d.n, m = d.m;
    g.xk = qp_work_doubles(d);
    g.uk = g.xk + (N + 1) * n;
    g.acc = g.uk + N * m;
    g.idx = g.acc + 2 * N;
    g.rec = g.idx + (2 * N + 1) / 2;
    g.x0c = g.rec + GUSTO_REC;                  // copies of x0, the targets and the desired inputs: the arguments of a zero-copy solve sit in
    g.zc = g.x0c + n;                           // pinned HOST memory (gusto.hip) and every QP / interior-point iteration reads them
    g.zfc = g.zc + (N + 1) * d.nz;              // (GustoBatch::host_args; the short-horizon lean kernels copy x0 and z always)
    g.udc = g.zfc + d.nz;
    g.end = g.udc + N * m;
    return g;
}

// The pinned, device-visible block of a GuSTO plan's zero-copy solves, [inputs | outputs]: byte offsets (64-byte aligned) and the
// extents they were made for.  has_zf = false (the SSM plan): no terminal target.
struct PinLayout {
    size_t x0, u_init, x_init, z, zf, ud, xopt, uopt, zopt, iters, status, trace, total;
    size_t N, n, m, nz, B;
    int max_trace;
};
inline PinLayout pin_layout(size_t N, size_t n, size_t m, size_t nz, size_t B, int max_trace, bool has_zf) {
    const size_t D = sizeof(double);
    PinLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 63) & ~(size_t)63; return at; };
    L.x0 = take(D * B * n); L.u_init = take(D * B * N * m); L.x_init = take(D * B * (N + 1) * n);
    L.z = take(D * B * (N + 1) * nz); L.zf = take(has_zf ? D * B * nz : 0); L.ud = take(D * B * N * m);
    L.xopt = take(D * B * (N + 1) * n); L.uopt = take(D * B * N * m); L.zopt = take(D * B * (N + 1) * nz);
    L.iters = take(sizeof(int32_t) * B); L.status = take(sizeof(int32_t) * B);
    L.trace = take(D * B * (size_t)std::max(1, max_trace) * 4);
    L.total = o;
    L.N = N; L.n = n; L.m = m; L.nz = nz; L.B = B; L.max_trace = max_trace;
    return L;
}

// device addresses of the staged arguments and of the results (null where the caller passed none)
struct PinArgs {
    const double *x0, *u_init, *x_init, *z, *zf, *ud;
    double *xopt, *uopt, *zopt, *trace;
    int32_t *iters, *status;
};
// the caller's arguments -> the pinned block `pin`, whose device address is dp
inline PinArgs pin_stage(const PinLayout &L, char *pin, char *dp, const double *x0, const double *u_init, const double *x_init,
                         const double *z, const double *zf, const double *ud, bool trace) {
    const size_t D = sizeof(double), N = L.N, n = L.n, m = L.m, nz = L.nz, B = L.B;
    memcpy(pin + L.x0, x0, D * B * n);
    memcpy(pin + L.u_init, u_init, D * B * N * m);
    memcpy(pin + L.x_init, x_init, D * B * (N + 1) * n);
    if (z) memcpy(pin + L.z, z, D * B * (N + 1) * nz);
    if (zf) memcpy(pin + L.zf, zf, D * B * nz);
    if (ud) memcpy(pin + L.ud, ud, D * B * N * m);
    auto dv = [&](size_t off) { return reinterpret_cast<double *>(dp + off); };
    return PinArgs{dv(L.x0), dv(L.u_init), dv(L.x_init), z ? dv(L.z) : nullptr, zf ? dv(L.zf) : nullptr, ud ? dv(L.ud) : nullptr,
                   dv(L.xopt), dv(L.uopt), dv(L.zopt), trace ? dv(L.trace) : nullptr,
                   reinterpret_cast<int32_t *>(dp + L.iters), reinterpret_cast<int32_t *>(dp + L.status)};
}
// the results out of the pinned block (iters, status, trace: null = not wanted)
inline void pin_copy_out(const PinLayout &L, const char *pin, double *xopt, double *uopt, double *zopt, int32_t *iters, int32_t *status,
                         double *trace) {
    const size_t D = sizeof(double), N = L.N, n = L.n, m = L.m, nz = L.nz, B = L.B;
    memcpy(xopt, pin + L.xopt, D * B * (N + 1) * n);
    memcpy(uopt, pin + L.uopt, D * B * N * m);
    memcpy(zopt, pin + L.zopt, D * B * (N + 1) * nz);
    if (iters) memcpy(iters, pin + L.iters, sizeof(int32_t) * B);
    if (status) memcpy(status, pin + L.status, sizeof(int32_t) * B);
    if (trace) memcpy(trace, pin + L.trace, D * B * (size_t)L.max_trace * 4);
}

}  // namespace

// lean.hip
int lean_select(const QPDims &d, int args[6]);          // index into the instantiation list (-1: none) + its template arguments
int lean_prepare(int variant, size_t lds);
int lean_launch_gusto(int variant, const QPDims &d, const QPConst &c, const TpwlDev &T, const GustoPar &par, const GustoBatch &b, unsigned grid,
                      size_t lds, hipStream_t stream);
int lean_launch_locp(int variant, const QPDims &d, const QPConst &c, const LocpBatch &b, unsigned grid, size_t lds, hipStream_t stream);
