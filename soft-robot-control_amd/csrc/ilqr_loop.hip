// Batched closed loop of the iLQR controller: every member tracks a per-step policy (x_bar, u_bar, K) -- the one a resident iLQR plan has
// just solved, or an uploaded one (TrajTracking's TV-LQR gains) -- on a TPWL plant stepped at the simulation step, and a whole run of
// steps is one launch sequence on the handle's stream with one host wait.  Reference: sofacontrol/tpwl/controllers.py:199-215 (ilqr /
// TrajTracking compute_input), tpwl/tpwl.py:160-168, 336-339 (plant step), examples/diamond/diamond.py:318-389 (run_ilqr).
//
// THE POLICY.  B members, controller step dt, simulation step dt_sim, dt = r dt_sim, r an integer >= 1.  Controller step j fires at
// simulation step s = j r since the last reset and reads the policy row rows[j]: the table row_j = int(round(j dt, 4) / dt) of the
// reference's clock (which is not j: at dt = 0.05 steps 3, 6, 7 read rows 2, 5, 6) is computed on the host in float64 and uploaded
// (silqr_loop_set_rows); the kernel does no time arithmetic.  A step whose row is outside 0 .. N-1 -- the table says -1 (behind
// final_time), row_j >= N (where the reference raises IndexError), or j beyond the table -- gets the idle input u0.
// One simulation step s (il_advance_kernel):
//   1. if s % r == 0: u = u_bar[row] + K[row] (xl - x_bar[row]), xl the filter's estimate with an observer, else the plant state;
//      otherwise the held u
//   2. x <- d_d[i] + A_d[i] x + B_d[i] u (+ w_s), i the plant's nearest point to x (THE STEP RULE of tpwl_dev.h)
//   3. z = H x
//   4. with an observer: y = (C x + y_ref) + v_s (measure_row), then one step of every filter with (u, y)
// The held input and the step counter live in the handle: a run may stop and resume in the middle of a controller step.
// Not offered: SSM plants or plans, weighting-mode plants, input clipping, re-planning during a run, the start-up phase before t_delay.
// The staging of a run is LoopStage / loop_run_staged of gusto_loop_host.h (there are no periods here, so LoopCore, loop_run_periods and
// the prepare kernel are not used); the observed chain -- shared with gusto_loop.hip -- is loop_observed_host.h.
#include "ilqr_host.h"
#include "loop_observed_host.h"

#include <algorithm>

namespace {

struct IlAdvArgs {
    int N, n, m, nz, r;
    int64_t S, step0;                   // simulation steps of this launch; the step counter (since the reset) at its first
    const double *xbar, *ubar, *K;      // the policy: rows (N+1) x n, N x m, N x m x n of member b at b * sx, b * su, b * sK
    size_t sx, su, sK;                  // member strides in doubles (0: one policy shared by all members)
    const int32_t *rows;                // (n_rows) policy row of controller step j; outside 0 .. N-1: the idle input
    int64_t n_rows;
    const double *u0;                   // (m) idle input
    const double *H;                    // (nz x n)
    const double *W;                    // (steps x B x n) disturbances, or null; this launch reads steps w_step0 ..
    const double *x_in;                 // (B x n)
    double *x_out;                      // (B x n) or null (may be x_in)
    const double *u_in;                 // (B x m) the held inputs the launch starts with
    double *u_out;                      // (B x m) or null (may be u_in)
    double *X, *Z, *U;                  // records: row row0 + s of member b (X may be null)
    int32_t *ip;                        // (B x S) points picked, or null
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
    // with an observer (il_advance_kernel<true>): the law reads the estimate, and the step ends with a measurement
    const double *xhat;                 // (B x n) the filters' estimates
    const double *C, *y_ref, *Vn;       // (ny x n), (ny) or null, (steps x B x ny) or null (indexed as W)
    double *Y;                          // (B x rows_u x ny) record, rows as U: the batched filter reads its y from it
    int ny;
};

__host__ __device__ inline int il_even(int v) { return (v + 1) & ~1; }

// LDS in doubles: x | x_bar | x - x_bar (n each, padded to even) | u_bar (16) | u (16) | the staged step of tpwl_dev.h with the point
// word behind its partial sums | OBS: the estimate (n)
size_t il_advance_lds_bytes(int n, int m, bool observed) {
    return srh::lds_request(sizeof(double) * ((size_t)3 * il_even(n) + 16 + 16 + 2 + tpwl::step_doubles(n, m, 256) + (observed ? il_even(n) : 0)));
}

// the policy row of controller step j, or -1: the idle input
__device__ __forceinline__ int il_row_of(const IlAdvArgs &a, int64_t j) {
    if (j >= a.n_rows) return -1;
    const int row = ((cgiptr)a.rows)[j];
    return (unsigned)row < (unsigned)a.N ? row : -1;
}

// One policy row in registers, laid out as the gain product reads it: wave w holds the gain rows w, w + 4, w + 8, w + 12 (n_u <= 16),
// lane l their columns l and l + 64 (n_x <= 128): every load of a wave is one contiguous run of a K row.  Threads 0 .. n-1 hold
// x_bar, threads 128 .. 128 + m - 1 u_bar.
struct IlRow {
    double k[4][2];
    double xb, ub;
    int row;                            // -1: idle, nothing loaded
};

__device__ __forceinline__ void il_row_load(IlRow &R, const IlAdvArgs &a, size_t b, int row, int tid, int wave, int lane) {
    const int n = a.n, m = a.m;
    R.row = row;
    if (row < 0) return;
    cgptr Kg = (cgptr)a.K + b * a.sK + (size_t)row * m * n;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = wave + 4 * q, c = lane + 64 * h;
            R.k[q][h] = (e < m && c < n) ? Kg[e * n + c] : 0.0;
        }
    R.xb = tid < n ? ((cgptr)a.xbar)[b * a.sx + (size_t)row * n + tid] : 0.0;
    R.ub = (tid >= 128 && tid < 128 + m) ? ((cgptr)a.ubar)[b * a.su + (size_t)row * m + (tid - 128)] : 0.0;
}

// One workgroup of 256 threads per member, S simulation steps.  The plant's region panel [A_d^T | B_d^T | d_d] sits in LDS and is
// reloaded only when the plant's nearest point changes; the state, x_bar and x - x_bar stay in LDS for the whole launch.  The policy row
// of the NEXT controller step does not depend on the state: its loads (x_bar, u_bar, at most 8 doubles of K per thread) are issued in
// front of the point search of the step before it fires, and are consumed -- from registers -- a step later.  Fixed summation orders:
//   (K dx)_e = wave sum over the lanes of fma(K[e][l + 64], dx[l + 64], fma(K[e][l], dx[l], 0)); u_e = u_bar[e] + (K dx)_e
//   x' = THE STEP RULE of tpwl_dev.h (+ w); z_e = out_row; y_e = measure_row (gusto_loop_prep.h)
// OBS: one step per launch (the filter is another kernel); the law reads the estimate x_hat.
template <bool OBS>
__global__ __launch_bounds__(256) void il_advance_kernel(TpwlDev TL, IlAdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = a.n, m = a.m, nz = a.nz, ne = il_even(n);
    lptr xc = (lptr)smem;                                // n      plant state
    lptr xb = xc + ne;                                   // n      x_bar
    lptr dx = xb + ne;                                   // n      xl - x_bar
    lptr ub = dx + ne;                                   // 16     u_bar
    lptr uc = ub + 16;                                   // 16     u, held between controller steps
    tpwl::StepLds L;                                     //        partial sums, (two doubles) the plant point, the panel of region `cur`
    lptr xh = tpwl::step_carve(L, uc + 16, n, m, 256, 2);        // n      OBS: the estimate
    liptr ip = (liptr)(L.pb + 256);
    clptr xl = OBS ? xh : xc;                            //        what the law reads
    const size_t b = blockIdx.x;
    const int tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int S = max(1, 256 / n), j = tid % n, sl = tid / n;
    cgptr H = (cgptr)a.H, Wd = (cgptr)a.W, u0 = (cgptr)a.u0;
    for (int e = tid; e < n; e += 256) xc[e] = ((cgptr)a.x_in)[b * n + e];
    if (OBS)
        for (int e = tid; e < n; e += 256) xh[e] = ((cgptr)a.xhat)[b * n + e];
    if (tid < m) uc[tid] = ((cgptr)a.u_in)[b * m + tid];
    IlRow R;
    R.row = -1;
    if (a.step0 % a.r == 0) il_row_load(R, a, b, il_row_of(a, a.step0 / a.r), tid, wave, lane);       // the launch's first step fires
    __syncthreads();
    int cur = -1;
    for (int64_t s = 0; s < a.S; ++s) {
        const int64_t step = a.step0 + s;
        const bool fire = step % a.r == 0;
        if (fire) {                                      // 1. the law at the row the registers hold
            const bool live = R.row >= 0;
            if (live) {
                if (tid < n) {                           // (n <= 128: waves 0 and 1)
                    xb[tid] = R.xb;
                    dx[tid] = xl[tid] - R.xb;
                } else if (tid >= 128 && tid < 128 + m) {
                    ub[tid - 128] = R.ub;
                }
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = wave + 4 * q;
                    if (e < m) {
                        double acc = 0.0;
                        if (lane < n) acc = fma(R.k[q][0], dx[lane], acc);
                        if (lane + 64 < n) acc = fma(R.k[q][1], dx[lane + 64], acc);
                        acc = wg::wave_sum(acc);
                        if (lane == 0) uc[e] = ub[e] + acc;
                    }
                }
            } else if (tid < m) {
                uc[tid] = u0[tid];
            }
        }
        // the next controller step's row, requested in front of this step's point search
        if ((step + 1) % a.r == 0 && s + 1 < a.S) il_row_load(R, a, b, il_row_of(a, (step + 1) / a.r), tid, wave, lane);
        if (wave == 0) {                                 // 2. the plant's point
            const int i = tpwl::nearest_wave(TL, xc);
            if (lane == 0) ip[0] = (unsigned)i < (unsigned)TL.P ? i : 0;           // (a state that is not a number: no minimum)
        }
        __syncthreads();
        const int p = ip[0];
        tpwl::panel_load(L, TL, p, cur, n, m, tid, 256);            // (the same for every thread; the barrier below covers the copies)
        __syncthreads();
        tpwl::step_slices(L, xc, uc, n, m, S, j, sl);
        __syncthreads();
        const size_t rx = b * (size_t)a.rows_x + a.row0_x + s, ru = b * (size_t)a.rows_u + a.row0_u + s;
        if (tid < n) {
            double v = tpwl::step_sum(L, n, S, tid);
            if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * n + tid];
            xc[tid] = v;
            if (a.X) ((gptr)a.X)[rx * n + tid] = v;
        } else if (tid >= 128 && tid < 128 + m) {
            ((gptr)a.U)[ru * m + (tid - 128)] = uc[tid - 128];
        } else if (tid == 255) {
            if (a.ip) ((giptr)a.ip)[b * (size_t)a.S + s] = p;
        }
        __syncthreads();
        // 3. z = H x.  xc is next written behind three barriers of the next step.
        for (int e = tid; e < nz; e += 256) ((gptr)a.Z)[rx * nz + e] = out_row(H, e, n, xc);
        if (OBS) {                                       // 4. the measurement of the new plant state
            cgptr Cg = (cgptr)a.C, yr = (cgptr)a.y_ref, Vn = (cgptr)a.Vn;
            for (int e = tid; e < a.ny; e += 256)
                ((gptr)a.Y)[ru * a.ny + e] = measure_row(Cg, e, n, xc, yr, Vn, ((size_t)(a.w_step0 + s) * a.B + b) * a.ny + e);
        }
    }
    if (a.x_out)
        for (int e = tid; e < n; e += 256) ((gptr)a.x_out)[b * n + e] = xc[e];
    if (a.u_out && tid < m) ((gptr)a.u_out)[b * m + tid] = uc[tid];
}

// Row 0 of the X and Z records of a run: the plant states it starts from and their outputs
__global__ __launch_bounds__(64) void il_row0_kernel(const double *x, const double *H, double *X, double *Z, int n, int nz, int64_t rows) {
    const size_t b = blockIdx.x;
    cgptr xc = (cgptr)x + b * n;
    if (X)
        for (int e = SRH_TID; e < n; e += 64) ((gptr)X)[b * (size_t)rows * n + e] = xc[e];
    for (int e = SRH_TID; e < nz; e += 64) ((gptr)Z)[b * (size_t)rows * nz + e] = out_row((cgptr)H, e, n, xc);
}

}  // namespace

struct silqr_loop : LoopStage {
    silqr_plan *plan = nullptr;
    stpwl *plant = nullptr;
    sekf_batch *obs = nullptr;
    int N = 0, n = 0, m = 0, nz = 0, r = 1, ny = 0;
    int64_t max_steps = 0;
    int64_t step = 0;                   // simulation steps since the last reset
    bool have_policy = false, policy_is_plan = false, policy_shared = false;
    size_t lds = 0, lds_obs = 0;
    // xcur, uheld: where the plants stand and the inputs they hold; u0: the idle input; rows: the row table; pxb, pub, pK: an uploaded policy
    srh::DevBuf xcur, uheld, u0, rows, pxb, pub, pK;
    int64_t n_rows = 0;
    std::vector<double> u0h;            // host copy of the idle input (a reset installs it as every member's held input)
    std::vector<double> idle_inputs() const {
        std::vector<double> u((size_t)B * m);
        for (size_t e = 0; e < u.size(); ++e) u[e] = u0h[e % m];
        return u;
    }
    // records: states, outputs, estimates (B x (S + 1) x .), inputs, measurements (B x S x .), the filters' status (B); noise W, V (S x B x .)
    LoopRec Xrec, Zrec, XHrec, Urec, Yrec, Erec, Wd, Vd;
    silqr_loop() {
        recs = {&Xrec, &Zrec, &XHrec, &Yrec, &Urec, &Erec};
        ins = {&Wd, &Vd};
    }
    ~silqr_loop() { drain(); }
    IlAdvArgs adv_args() const {
        IlAdvArgs a{};
        a.N = N; a.n = n; a.m = m; a.nz = nz; a.r = r;
        const size_t Nz = (size_t)N;
        if (policy_is_plan) {
            a.xbar = plan->x_dev(); a.ubar = plan->u_dev(); a.K = plan->K_dev();
            a.sx = (Nz + 1) * n; a.su = Nz * m; a.sK = Nz * m * n;
        } else {
            a.xbar = pxb.as<double>(); a.ubar = pub.as<double>(); a.K = pK.as<double>();
            a.sx = policy_shared ? 0 : (Nz + 1) * n; a.su = policy_shared ? 0 : Nz * m; a.sK = policy_shared ? 0 : Nz * m * n;
        }
        a.rows = rows.as<int32_t>(); a.n_rows = n_rows;
        a.u0 = u0.as<double>();
        a.H = plant->H.as<double>();
        a.B = B;
        return a;
    }
    int launch_advance(const IlAdvArgs &a) const {
        il_advance_kernel<false><<<(unsigned)B, 256, lds, stream>>>(plant->view(), a);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    // The observed chain (loop_observed_host.h): a launch covers one step.  v: the arguments of the whole run; XH: the estimate record
    // (rows as X); E: the status record (B).
    int launch_observed_chain(IlAdvArgs v, double *XH, int32_t *E) const {
        v.xhat = obs->x_dev(); v.C = obs->C.as<double>(); v.y_ref = obs->yref_dev(); v.ny = ny;
        const int64_t S = v.S, step0 = v.step0, row0_x = v.row0_x, row0_u = v.row0_u, w0 = v.w_step0;
        return loop_observed_chain(this, obs, S, ObsRecs{v.U, v.Y, v.rows_u, row0_u, XH, v.rows_x, row0_x, E, nullptr, 0}, [&](int64_t s) -> int {
            v.S = 1; v.step0 = step0 + s; v.row0_x = row0_x + s; v.row0_u = row0_u + s; v.w_step0 = w0 + s;
            il_advance_kernel<true><<<(unsigned)B, 256, lds_obs, stream>>>(plant->view(), v);
            SRH_CHECK_HIP(hipGetLastError());
            return SRH_OK;
        });
    }
};

extern "C" {

int silqr_loop_create(silqr_loop_t **out, silqr_plan_t *plan, stpwl_t *plant, int N, int r, int64_t batch, int64_t max_steps_per_run) {
    SRH_REQUIRE(out && plant, "silqr_loop_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(N >= 1 && r >= 1 && batch >= 1 && max_steps_per_run >= 1,
                "silqr_loop_create: need N >= 1, r >= 1 (dt = r dt_sim), batch >= 1 and max_steps_per_run >= 1");
    const int n = plant->n, m = plant->m, nz = plant->nz;
    SRH_REQUIRE(m <= 16, "silqr_loop_create: n_u = %d exceeds the limit n_u <= 16 of the advance kernel", m);
    SRH_REQUIRE(n <= 128, "silqr_loop_create: the plant's n_x = %d exceeds the limit n_x <= 128 of the advance kernel", n);
    SRH_REQUIRE(plant->has_discrete, "silqr_loop_create: the plant has not been pre-discretised at dt_sim");
    SRH_REQUIRE(nz > 0 && plant->H.p, "silqr_loop_create: the plant has no output map (z = H x)");
    if (plan) {
        SRH_REQUIRE(plan->n == n && plan->m == m, "silqr_loop_create: the plant has n_x = %d, n_u = %d, the policy n_x = %d, n_u = %d", n, m, plan->n,
                    plan->m);
        SRH_REQUIRE(plan->N == N && plan->batch == batch, "silqr_loop_create: the plan has N = %d, batch = %lld, the loop N = %d, batch = %lld",
                    plan->N, (long long)plan->batch, N, (long long)batch);
    }
    const size_t lds = il_advance_lds_bytes(n, m, false);
    SRH_REQUIRE(lds <= (size_t)160 * 1024, "silqr_loop_create: the advance kernel needs %zu bytes of LDS (160 KiB available)", lds);
    silqr_loop *h = new silqr_loop();
    auto fail = [&](int code) { delete h; return code; };
    h->plan = plan; h->plant = plant; h->N = N; h->n = n; h->m = m; h->nz = nz; h->r = r; h->B = batch; h->max_steps = max_steps_per_run;
    h->lds = lds;
    const char *what = "set up the advance kernel / the stream";
    if (hipFuncSetAttribute((const void *)il_advance_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(loop_setup_failed("silqr_loop_create", what));
    const size_t D = sizeof(double), Bz = (size_t)batch, S = (size_t)max_steps_per_run;
    h->Xrec.shape(D * n, 1); h->Zrec.shape(D * nz, 1); h->Urec.shape(D * m, 0); h->Wd.shape(D * n, 0);
    // the identity row table until silqr_loop_set_rows installs the clock's; the idle input zero
    std::vector<int32_t> rows((size_t)N);
    for (int j = 0; j < N; ++j) rows[j] = j;
    const std::vector<double> zeros((size_t)m, 0.0);
    int rc;
    if ((rc = h->xcur.alloc(D * Bz * n)) || (rc = h->uheld.alloc(D * Bz * m)) || (rc = h->u0.upload(zeros.data(), D * m)) ||
        (rc = h->rows.upload(rows.data(), sizeof(int32_t) * N)) || (rc = h->Zrec.alloc(Bz, S, 1)) || (rc = h->Urec.alloc(Bz, S, 1)))
        return fail(rc);
    h->n_rows = N; h->u0h = zeros;
    *out = h;
    return SRH_OK;
}

int silqr_loop_destroy(silqr_loop_t *h) {
    SRH_REQUIRE(h, "silqr_loop_destroy: null handle");
    delete h;
    return SRH_OK;
}

int silqr_loop_set_policy(silqr_loop_t *h, const double *x_bar, const double *u_bar, const double *K, int shared) {
    SRH_REQUIRE(h, "silqr_loop_set_policy: null handle");
    SRH_REQUIRE(x_bar && u_bar && K, "silqr_loop_set_policy: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    const size_t D = sizeof(double), c = shared ? 1 : (size_t)h->B, N = h->N, n = h->n, m = h->m;
    h->have_policy = false;
    int rc;
    if ((rc = h->pxb.upload(x_bar, D * c * (N + 1) * n)) || (rc = h->pub.upload(u_bar, D * c * N * m)) || (rc = h->pK.upload(K, D * c * N * m * n)))
        return rc;
    h->have_policy = true; h->policy_is_plan = false; h->policy_shared = shared != 0;
    return SRH_OK;
}

int silqr_loop_set_rows(silqr_loop_t *h, const int32_t *rows, int64_t count) {
    SRH_REQUIRE(h, "silqr_loop_set_rows: null handle");
    SRH_REQUIRE(rows && count >= 1, "silqr_loop_set_rows: need a table of at least one row");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc = h->rows.upload(rows, sizeof(int32_t) * (size_t)count);
    if (rc) { h->n_rows = 0; return rc; }
    h->n_rows = count;
    return SRH_OK;
}

int silqr_loop_set_idle_input(silqr_loop_t *h, const double *u0) {
    SRH_REQUIRE(h, "silqr_loop_set_idle_input: null handle");
    SRH_REQUIRE(u0, "silqr_loop_set_idle_input: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipMemcpy(h->u0.p, u0, sizeof(double) * h->m, hipMemcpyHostToDevice));
    h->u0h.assign(u0, u0 + h->m);
    return SRH_OK;
}

int silqr_loop_set_observer(silqr_loop_t *h, sekf_batch_t *observer) {
    SRH_REQUIRE(h, "silqr_loop_set_observer: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->obs = nullptr; h->have_state = false;
    if (!observer) return SRH_OK;
    int rc;
    if ((rc = loop_check_observer("silqr_loop_set_observer", observer, h->B, h->n, h->m))) return rc;
    h->lds_obs = il_advance_lds_bytes(h->n, h->m, true);
    SRH_REQUIRE(h->lds_obs <= (size_t)160 * 1024, "silqr_loop_set_observer: the observed advance kernel needs %zu bytes of LDS (160 KiB available)",
                h->lds_obs);
    SRH_CHECK_HIP(hipFuncSetAttribute((const void *)il_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_obs));
    const size_t B = (size_t)h->B, S = (size_t)h->max_steps;
    loop_shape_observed(h->XHrec, h->Yrec, h->Erec, h->Vd, h->n, observer->ny);
    if ((rc = h->XHrec.alloc(B, S, 1)) || (rc = h->Yrec.alloc(B, S, 1)) || (rc = h->Erec.alloc(B, S, 1))) return rc;
    h->obs = observer; h->ny = observer->ny;
    return SRH_OK;
}

int silqr_loop_reset(silqr_loop_t *h, const double *x0, const double *x_hat0) {
    SRH_REQUIRE(h, "silqr_loop_reset: null handle");
    SRH_REQUIRE(x0, "silqr_loop_reset: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->have_state = false;
    const size_t D = sizeof(double), B = (size_t)h->B;
    SRH_CHECK_HIP(hipMemcpy(h->xcur.p, x0, D * B * h->n, hipMemcpyHostToDevice));
    // every member holds the idle input until its first controller step fires (step 0)
    SRH_CHECK_HIP(hipMemcpy(h->uheld.p, h->idle_inputs().data(), D * B * h->m, hipMemcpyHostToDevice));
    if (h->obs) {
        SRH_CHECK_HIP(hipMemcpy(h->obs->x_dev(), x_hat0 ? x_hat0 : x0, D * B * h->n, hipMemcpyHostToDevice));
        int rc = sekf_batch_install_sigma0(h->obs);
        if (rc) return rc;
    }
    h->step = 0; h->have_state = true;
    return SRH_OK;
}

int silqr_loop_plan(silqr_loop_t *h, const double *u_warm) {
    SRH_REQUIRE(h, "silqr_loop_plan: null handle");
    SRH_REQUIRE(h->plan, "silqr_loop_plan: the loop was created without a plan (install a policy with silqr_loop_set_policy)");
    SRH_REQUIRE(h->have_state, "silqr_loop_plan: no belief yet (call silqr_loop_reset first)");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    silqr_plan *p = h->plan;
    if (u_warm) SRH_CHECK_HIP(hipMemcpy(p->uw.p, u_warm, sizeof(double) * h->B * h->N * h->m, hipMemcpyHostToDevice));
    // from the belief where it stands on the device: the estimates with an observer, else the plant states
    const double *belief = h->obs ? h->obs->x_dev() : h->xcur.as<double>();
    int rc = silqr_plan_solve_dev(p, belief, u_warm ? p->uw.as<double>() : nullptr, h->stream);
    if (rc) return rc;
    h->have_policy = true; h->policy_is_plan = true; h->policy_shared = false;
    return SRH_OK;
}

int silqr_loop_run(silqr_loop_t *h, int64_t steps, const double *W, const double *V, double *X, double *Z, double *U, double *Xhat, double *Y,
                   int32_t *ekf_status) {
    SRH_REQUIRE(h, "silqr_loop_run: null handle");
    SRH_REQUIRE(Z && U, "silqr_loop_run: null argument");
    SRH_REQUIRE(steps >= 1, "silqr_loop_run: steps must be positive");
    SRH_REQUIRE(steps <= h->max_steps, "silqr_loop_run: steps = %lld exceeds max_steps_per_run = %lld", (long long)steps, (long long)h->max_steps);
    SRH_REQUIRE(h->have_state, "silqr_loop_run: no plant state yet (call silqr_loop_reset first)");
    SRH_REQUIRE(h->have_policy, "silqr_loop_run: no policy yet (call silqr_loop_plan or silqr_loop_set_policy first)");
    const bool observed = h->obs != nullptr;
    SRH_REQUIRE(!observed || (Xhat && Y && ekf_status), "silqr_loop_run: a loop with an observer records Xhat, Y and ekf_status");
    const size_t B = (size_t)h->B, S = (size_t)steps, Sm = (size_t)h->max_steps;
    h->Wd.host = (void *)W; h->Vd.host = (void *)(observed ? V : nullptr);
    h->Xrec.host = X; h->Zrec.host = Z; h->Urec.host = U;
    h->XHrec.host = observed ? Xhat : nullptr; h->Yrec.host = observed ? Y : nullptr; h->Erec.host = observed ? ekf_status : nullptr;
    int rc;
    if (X && !h->Xrec.d.p && (rc = h->Xrec.alloc(B, Sm, 1))) return rc;              // the blocks only some runs ask for
    for (LoopRec *r : h->ins)
        if (r->host && !r->d.p && (rc = r->alloc(B, Sm, 1))) return rc;
    h->XHrec.row0 = observed ? h->obs->x_dev() : nullptr;             // row 0 of the estimate record: the estimates the run starts from
    rc = loop_run_staged(h, S, 1, [&]() -> int {
        il_row0_kernel<<<(unsigned)B, 64, 0, h->stream>>>(h->xcur.as<double>(), h->plant->H.as<double>(), X ? h->Xrec.as<double>() : nullptr,
                                                           h->Zrec.as<double>(), h->n, h->nz, (int64_t)S + 1);
        SRH_CHECK_HIP(hipGetLastError());
        IlAdvArgs v = h->adv_args();
        v.S = (int64_t)S; v.step0 = h->step;
        v.W = W ? h->Wd.as<double>() : nullptr; v.w_step0 = 0;
        v.x_in = h->xcur.as<double>(); v.x_out = h->xcur.as<double>();
        v.u_in = h->uheld.as<double>(); v.u_out = h->uheld.as<double>();
        v.X = X ? h->Xrec.as<double>() : nullptr; v.Z = h->Zrec.as<double>(); v.U = h->Urec.as<double>();
        v.rows_x = (int64_t)S + 1; v.row0_x = 1; v.rows_u = (int64_t)S; v.row0_u = 0;
        if (!observed) return h->launch_advance(v);
        v.Vn = V ? h->Vd.as<double>() : nullptr; v.Y = h->Yrec.as<double>();
        return h->launch_observed_chain(v, h->XHrec.as<double>(), h->Erec.as<int32_t>());
    });
    if (!rc) h->step += steps;
    return rc;
}

int silqr_loop_last_policy(silqr_loop_t *h, double *x_bar, double *u_bar, double *K, int *shared) {
    SRH_REQUIRE(h, "silqr_loop_last_policy: null handle");
    SRH_REQUIRE(h->have_policy, "silqr_loop_last_policy: no policy yet (call silqr_loop_plan or silqr_loop_set_policy first)");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    if (shared) *shared = h->policy_shared ? 1 : 0;
    if (h->policy_is_plan) return silqr_plan_policy(h->plan, x_bar, u_bar, K, nullptr, nullptr);
    const size_t D = sizeof(double), c = h->policy_shared ? 1 : (size_t)h->B, N = h->N, n = h->n, m = h->m;
    int rc;
    if ((x_bar && (rc = h->pxb.download(x_bar, D * c * (N + 1) * n))) || (u_bar && (rc = h->pub.download(u_bar, D * c * N * m))) ||
        (K && (rc = h->pK.download(K, D * c * N * m * n))))
        return rc;
    return SRH_OK;
}

int silqr_loop_plan_info(silqr_loop_t *h, double *cost, int32_t *iters) {
    SRH_REQUIRE(h, "silqr_loop_plan_info: null handle");
    SRH_REQUIRE(h->plan && h->policy_is_plan && h->have_policy, "silqr_loop_plan_info: the loop's policy is not a plan's (call silqr_loop_plan first)");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    return silqr_plan_policy(h->plan, nullptr, nullptr, nullptr, cost, iters);
}

int silqr_loop_stats(silqr_loop_t *h, int64_t *steps, int64_t *waits_last_run) {
    SRH_REQUIRE(h, "silqr_loop_stats: null handle");
    if (steps) *steps = h->step;
    if (waits_last_run) *waits_last_run = h->waits;
    return SRH_OK;
}

int silqr_loop_advance(silqr_loop_t *h, const double *x, const double *u_held, int64_t steps, int64_t step0, const double *W, double *X, double *Z,
                       double *U, int32_t *idx) {
    SRH_REQUIRE(h, "silqr_loop_advance: null handle");
    SRH_REQUIRE(x && X && Z && U, "silqr_loop_advance: null argument");
    SRH_REQUIRE(steps >= 1 && step0 >= 0, "silqr_loop_advance: need steps >= 1 and step0 >= 0");
    SRH_REQUIRE(h->have_policy, "silqr_loop_advance: no policy yet (call silqr_loop_plan or silqr_loop_set_policy first)");
    const size_t D = sizeof(double), B = (size_t)h->B, n = h->n, m = h->m, nz = h->nz, S = (size_t)steps;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    srh::DevBuf dx, du, dW, dX, dZ, dU, dp;
    int rc;
    if ((rc = dx.upload(x, D * B * n)) || (u_held ? (rc = du.upload(u_held, D * B * m)) : (rc = du.alloc(D * B * m))) ||
        (W && (rc = dW.upload(W, D * S * B * n))) || (rc = dX.alloc(D * B * S * n)) || (rc = dZ.alloc(D * B * S * nz)) ||
        (rc = dU.alloc(D * B * S * m)) || (rc = dp.alloc(sizeof(int32_t) * B * S)))
        return rc;
    if (!u_held) SRH_CHECK_HIP(hipMemcpy(du.p, h->idle_inputs().data(), D * B * m, hipMemcpyHostToDevice));
    IlAdvArgs v = h->adv_args();
    v.S = steps; v.step0 = step0;
    v.W = W ? dW.as<double>() : nullptr; v.w_step0 = 0;
    v.x_in = dx.as<double>(); v.x_out = nullptr; v.u_in = du.as<double>(); v.u_out = nullptr;
    v.X = dX.as<double>(); v.Z = dZ.as<double>(); v.U = dU.as<double>(); v.ip = dp.as<int32_t>();
    v.rows_x = steps; v.row0_x = 0; v.rows_u = steps; v.row0_u = 0;
    if ((rc = loop_wait(h->launch_advance(v), h->stream))) return rc;
    if ((rc = dX.download(X, D * B * S * n)) || (rc = dZ.download(Z, D * B * S * nz)) || (rc = dU.download(U, D * B * S * m))) return rc;
    if (idx && (rc = dp.download(idx, sizeof(int32_t) * B * S))) return rc;
    return SRH_OK;
}

}  // extern "C"
