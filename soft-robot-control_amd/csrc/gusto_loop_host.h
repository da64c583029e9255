// The host shell of the five closed-loop units (gusto_loop.hip: TPWL plans, gusto_ssm_loop.hip: SSM plans, rompc_loop.hip: the chained
// linear MPC of the ROMPC baseline, koopman_loop.hip: the Koopman baseline's MPC, ilqr_loop.hip: the tracked iLQR policy), stated once:
// what every run stages (LoopStage: stream, waits, the blocks of a run that cross PCIe as a table of LoopRec, and loop_run_staged: the
// copies up, row 0, the unit's launches, the copies back, ONE wait, the drain on an error), the common part of a handle with periods
// (LoopCore), the checks and set-up of a create, the bodies of set_target / last_inputs / last_plan / stats, and the periods of a run
// (loop_run_periods: capacity, per period the prepare kernel and the unit's own part).  What a unit keeps: its advance kernels, which
// rollout / solve it calls, and where row 0 of its records comes from.  The device side of what they share is gusto_loop_prep.h; the
// constant-horizon QP and the plan shift of the two linear MPC units are mpc_loop_host.h, the observed sub-step chain of the TPWL and
// iLQR units is loop_observed_host.h.
#pragma once
#include "gusto_loop_prep.h"

#include <initializer_list>

namespace {

struct PinBuf {
    char *p = nullptr;
    size_t cap = 0;
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    int need(size_t bytes) {
        if (bytes <= cap) return SRH_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
        SRH_CHECK_HIP(hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return SRH_OK;
    }
};

// One block of a run that crosses PCIe through pinned memory: a record (device -> host behind the periods) or a noise block (host ->
// device in front of them).  A run of S plant steps in P periods moves unit * B * (per_period ? P : S + extra) bytes of it.
struct LoopRec {
    srh::DevBuf d;
    PinBuf pin;
    size_t unit = 0;                    // bytes of one row of one member
    int extra = 0;                      // rows beyond S (1: row 0 is where the run starts)
    bool per_period = false;
    void *host = nullptr;               // the caller's array of this run; null: the block is not part of it
    const void *row0 = nullptr;         // device (B x unit) copied into row 0 in front of the periods; null: the unit's kernels write it
    void shape(size_t unit_, int extra_, bool per_period_ = false) { unit = unit_; extra = extra_; per_period = per_period_; }
    size_t bytes(size_t B, size_t S, size_t P) const { return unit * B * (per_period ? P : S + extra); }
    int alloc(size_t B, size_t S, size_t P) {
        int rc = pin.need(bytes(B, S, P));
        return rc ? rc : d.alloc(bytes(B, S, P));
    }
    template <typename T> T *as() const { return d.as<T>(); }
};

// what the unit supplies to the prepare kernel: the states the plans start from, the plant states for row 0 (null: xcur), the planner's
// output map and the terminal target (null: none), and whether the kernel writes row 0 of the X / Z records
struct PrepUnit {
    const double *xcur, *xplant, *H;
    double *zf;
    bool rec_row0;
};

// where period p of a run of S steps writes: record rows (X, Z: S + 1 per member; U: S) and the first step of its noise
struct LoopRows {
    int64_t rows_x, row0_x, rows_u, row0_u, w_step0;
};

// What a run needs whether or not it has periods: the members, the stream, and the blocks that cross PCIe in front of the launches
// (ins) and behind them (recs, in the order of their copies back)
struct LoopStage {
    int64_t B = 0;
    int64_t waits = 0;                  // blocking host waits of the last run
    bool have_state = false;
    hipStream_t stream = nullptr;
    std::vector<LoopRec *> recs, ins;
    void drain() { if (stream) (void)hipStreamSynchronize(stream); }
    ~LoopStage() {
        drain();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct LoopCore : LoopStage {
    int N = 0, n = 0, m = 0, nz = 0, n_keep = 0, T = 0;
    int64_t max_steps = 0;
    double dt = 0.0, dt_sim = 0.0, t_start = 0.0;
    bool has_z = false, has_ud = false, has_phase = false;
    int64_t k = 0;                      // periods since the last reset
    size_t lds = 0;
    srh::DevBuf x0, u_init, x_init, z, ud, xopt, uopt, zopt, xcur, tt, tz, tu, phase, js, theta;
    // records: states (B x (S + 1) x n, allocated by the first run that asks for it), outputs, inputs (B x S x m), iterations, status and
    // cost of every solve (P x B), estimates (B x (S + 1) x n), measurements; noise: W (steps x B x n), V.  A unit shapes Z, XH, Y and V
    // (their widths and rows are its own) and appends what only it records.
    LoopRec Xrec, Zrec, Urec, Irec, Srec, Jrec, XHrec, Yrec, Wd, Vd;
    // the records in the order of their copies back, largest first: the S + 1 row blocks, the inputs, then the per-period words; the
    // blocks of a run that go the other way, in front of the periods: the noise, and what a unit appends (a recorded plant)
    LoopCore() {
        recs = {&Xrec, &Zrec, &Yrec, &XHrec, &Urec, &Irec, &Srec, &Jrec};
        ins = {&Wd, &Vd};
    }
    int alloc_recs(std::initializer_list<LoopRec *> list) {
        int rc;
        for (LoopRec *r : list)
            if ((rc = r->alloc((size_t)B, (size_t)max_steps, (size_t)(max_steps / n_keep)))) return rc;
        return SRH_OK;
    }
    // Behind the checks of a create: the fields, the schedule of a period's sub-steps, the stream, the common blocks (zw: width of Z)
    int setup(const char *who, const char *what, int N_, int n_, int m_, int nz_, int64_t B_, double dt_, double dt_sim_, int n_keep_,
              int64_t max_steps_, size_t zw);
};

int loop_setup_failed(const char *who, const char *what) {
    srh::set_error("%s: could not %s: %s", who, what, hipGetErrorString(hipGetLastError()));
    return SRH_EHIP;
}

int loop_check_periods(const char *who, int N, double dt, double dt_sim, int n_keep, int64_t max_steps_per_run) {
    SRH_REQUIRE(dt_sim > 0.0 && n_keep >= 1, "%s: need dt_sim > 0 and n_keep >= 1", who);
    SRH_REQUIRE(!((double)n_keep * dt_sim > (double)N * dt),
                "%s: n_keep * dt_sim = %g exceeds the horizon N * dt = %g (the shift of the previous plan would find no row)", who,
                (double)n_keep * dt_sim, (double)N * dt);
    SRH_REQUIRE(max_steps_per_run >= n_keep, "%s: max_steps_per_run = %lld is below n_keep = %d", who, (long long)max_steps_per_run, n_keep);
    return SRH_OK;
}

int LoopCore::setup(const char *who, const char *what, int N_, int n_, int m_, int nz_, int64_t B_, double dt_, double dt_sim_, int n_keep_,
                    int64_t max_steps_, size_t zw) {
    N = N_; n = n_; m = m_; nz = nz_; n_keep = n_keep_; B = B_; max_steps = max_steps_; dt = dt_; dt_sim = dt_sim_;
    std::vector<int32_t> j(n_keep);
    std::vector<double> th(n_keep);
    (void)sgusto_loop_schedule(N, dt, dt_sim, n_keep, 0.0, 0, nullptr, nullptr, j.data(), th.data());
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return loop_setup_failed(who, what);
    const size_t D = sizeof(double), Bz = (size_t)B;
    Xrec.shape(D * n, 1); Zrec.shape(D * zw, 1); Urec.shape(D * m, 0); Wd.shape(D * n, 0);
    Irec.shape(sizeof(int32_t), 0, true); Srec.shape(sizeof(int32_t), 0, true); Jrec.shape(D, 0, true);
    int rc;
    if ((rc = x0.alloc(D * Bz * n)) || (rc = u_init.alloc(D * Bz * N * m)) || (rc = x_init.alloc(D * Bz * (N + 1) * n)) ||
        (rc = z.alloc(D * Bz * (N + 1) * nz)) || (rc = ud.alloc(D * Bz * N * m)) || (rc = xopt.alloc(D * Bz * (N + 1) * n)) ||
        (rc = uopt.alloc(D * Bz * N * m)) || (rc = zopt.alloc(D * Bz * (N + 1) * nz)) || (rc = xcur.alloc(D * Bz * n)) ||
        (rc = js.upload(j.data(), sizeof(int32_t) * n_keep)) || (rc = theta.upload(th.data(), D * n_keep)))
        return rc;
    return alloc_recs({&Zrec, &Urec, &Irec, &Srec, &Jrec});
}

int loop_set_target(LoopCore *h, const char *who, int T, const double *t, const double *z, const double *u_des, const double *phase) {
    SRH_REQUIRE(h && t && (z || u_des), "%s: null argument", who);
    SRH_REQUIRE(T >= 2, "%s: the table needs at least two rows", who);
    for (int i = 1; i < T; ++i) SRH_REQUIRE(t[i] > t[i - 1], "%s: t must increase (row %d)", who, i);
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc;
    if ((rc = h->tt.upload(t, sizeof(double) * T))) return rc;
    if (z && (rc = h->tz.upload(z, sizeof(double) * T * h->nz))) return rc;
    if (u_des && (rc = h->tu.upload(u_des, sizeof(double) * T * h->m))) return rc;
    if (phase && (rc = h->phase.upload(phase, sizeof(double) * h->B))) return rc;
    h->T = T; h->has_z = z != nullptr; h->has_ud = u_des != nullptr; h->has_phase = phase != nullptr;
    return SRH_OK;
}

int loop_last_inputs(LoopCore *h, const char *who, double *x0, double *u_init, double *x_init, double *z, double *u_des) {
    SRH_REQUIRE(h, "%s: null handle", who);
    SRH_REQUIRE(h->have_state && h->k > 0, "%s: no period has run since the last reset", who);
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m, nz = h->nz;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc;
    if (x0 && (rc = h->x0.download(x0, D * B * n))) return rc;
    if (u_init && (rc = h->u_init.download(u_init, D * B * N * m))) return rc;
    if (x_init && (rc = h->x_init.download(x_init, D * B * (N + 1) * n))) return rc;
    if (z && h->has_z && (rc = h->z.download(z, D * B * (N + 1) * nz))) return rc;
    if (u_des && h->has_ud && (rc = h->ud.download(u_des, D * B * N * m))) return rc;
    return SRH_OK;
}

int loop_last_plan(LoopCore *h, const char *who, double *xopt, double *uopt) {
    SRH_REQUIRE(h, "%s: null handle", who);
    SRH_REQUIRE(h->have_state && h->k > 0, "%s: no period has run since the last reset", who);
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc;
    if (xopt && (rc = h->xopt.download(xopt, D * B * (N + 1) * h->n))) return rc;
    if (uopt && (rc = h->uopt.download(uopt, D * B * N * h->m))) return rc;
    return SRH_OK;
}

int loop_stats(LoopCore *h, const char *who, int64_t *steps, int64_t *waits_last_run) {
    SRH_REQUIRE(h, "%s: null handle", who);
    if (steps) *steps = h->k;
    if (waits_last_run) *waits_last_run = h->waits;
    return SRH_OK;
}

// Behind launches whose buffers are temporaries (they go back to the allocation cache when the caller returns): wait for the kernels
// whatever the launch answered, then report the launch's error, or the wait's
int loop_wait(int rc, hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return rc;
    SRH_CHECK_HIP(e);
    return SRH_OK;
}

// The frame of a run of S steps in P periods: the `host` arrays of h->ins through pinned memory and up, row 0 of the records that name
// one (LoopRec::row0), enqueue() -- the unit's launches on h->stream --, the records of h->recs down, ONE wait, and the copy to the
// caller's arrays.  From the first copy on work is enqueued on the handle's stream: on any error it is drained before returning.
template <class Enqueue>
int loop_run_staged(LoopStage *h, size_t S, size_t P, Enqueue enqueue) {
    const size_t B = (size_t)h->B;
    h->waits = 0;
    hipStream_t st = h->stream;
    int rc;
    auto body = [&]() -> int {
        for (LoopRec *r : h->ins)
            if (r->host) {
                memcpy(r->pin.p, r->host, r->bytes(B, S, P));
                SRH_CHECK_HIP(hipMemcpyAsync(r->d.p, r->pin.p, r->bytes(B, S, P), hipMemcpyHostToDevice, st));
            }
        for (LoopRec *r : h->recs)
            if (r->host && r->row0)
                SRH_CHECK_HIP(hipMemcpy2DAsync(r->d.p, r->unit * (S + 1), r->row0, r->unit, r->unit, B, hipMemcpyDeviceToDevice, st));
        if ((rc = enqueue())) return rc;
        for (LoopRec *r : h->recs)
            if (r->host) SRH_CHECK_HIP(hipMemcpyAsync(r->pin.p, r->d.p, r->bytes(B, S, P), hipMemcpyDeviceToHost, st));
        h->waits += 1;
        SRH_CHECK_HIP(hipStreamSynchronize(st));
        return SRH_OK;
    };
    if ((rc = body())) {
        (void)hipStreamSynchronize(st);
        h->have_state = false;          // part of a run was enqueued: the state is not the one the caller knows
        return rc;
    }
    for (LoopRec *r : h->recs)
        if (r->host) memcpy(r->host, r->pin.p, r->bytes(B, S, P));
    return SRH_OK;
}

// `periods` periods from where the handle stands, the records into the `host` arrays of h->recs, noise from those of Wd / Vd.
// period(p, a, r): the unit's part of period p behind the prepare kernel -- first guess (a.first), solve, costs, advance -- enqueued on
// h->stream; a: the prepare kernel's arguments (the solve's inputs), r: the rows of the records the advance writes.
template <class Period>
int loop_run_periods(LoopCore *h, const char *who, int periods, const PrepUnit &u, Period period) {
    const int N = h->N, m = h->m, nk = h->n_keep;
    const size_t D = sizeof(double), B = (size_t)h->B, S = (size_t)periods * nk, P = (size_t)periods;
    SRH_REQUIRE((int64_t)S <= h->max_steps, "%s: periods * n_keep = %lld exceeds max_steps_per_run = %lld", who, (long long)S, (long long)h->max_steps);
    int rc;
    if (h->Xrec.host && !h->Xrec.d.p && (rc = h->alloc_recs({&h->Xrec}))) return rc;          // the blocks only some runs ask for
    for (LoopRec *r : h->ins)
        if (r->host && !r->d.p && (rc = h->alloc_recs({r}))) return rc;
    hipStream_t st = h->stream;
    rc = loop_run_staged(h, S, P, [&]() -> int {
        for (int p = 0; p < periods; ++p) {
            const int64_t k = h->k + p;
            PrepArgs a{};
            a.N = N; a.n = h->n; a.m = m; a.nz = h->nz; a.T = h->T;
            a.first = k == 0 ? 1 : 0;
            a.dt = h->dt;
            (void)sgusto_loop_schedule(N, h->dt, h->dt_sim, nk, h->t_start, k, &a.tk, &a.idx0, nullptr, nullptr);
            a.xcur = u.xcur; a.xplant = u.xplant; a.H = u.H; a.zf = u.zf;
            a.xopt = h->xopt.as<double>(); a.uopt = h->uopt.as<double>();
            a.tt = h->tt.as<double>();
            a.tz = h->has_z ? h->tz.as<double>() : nullptr;
            a.tu = h->has_ud ? h->tu.as<double>() : nullptr;
            a.phase = h->has_phase ? h->phase.as<double>() : nullptr;
            a.x0 = h->x0.as<double>(); a.x_init = h->x_init.as<double>(); a.u_init = h->u_init.as<double>();
            a.z = h->z.as<double>(); a.ud = h->ud.as<double>();
            a.Xrec = (p == 0 && u.rec_row0 && h->Xrec.host) ? h->Xrec.as<double>() : nullptr;
            a.Zrec = (p == 0 && u.rec_row0) ? h->Zrec.as<double>() : nullptr;
            a.rec_rows = (int64_t)S + 1;
            if (a.first) SRH_CHECK_HIP(hipMemsetAsync(h->u_init.p, 0, D * B * N * m, st));
            loop_prepare_kernel<<<(unsigned)B, 256, 0, st>>>(a);
            SRH_CHECK_HIP(hipGetLastError());
            const LoopRows r{(int64_t)S + 1, (int64_t)p * nk + 1, (int64_t)S, (int64_t)p * nk, (int64_t)p * nk};
            int e = period(p, a, r);
            if (e) return e;
        }
        return SRH_OK;
    });
    if (!rc) h->k += periods;
    return rc;
}

}  // namespace
