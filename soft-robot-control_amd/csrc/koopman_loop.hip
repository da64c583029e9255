// Batched closed loop of the Koopman baseline: every problem of an skoop_t handle's batch is its own loop of the reference's controller --
// lift the delay-embedded measurements of the ring into the QP's state, solve the linear MPC on the lifted model, apply the plan's rows
// to the plant at the simulation step and push every new measurement into the ring -- and a whole run of periods is one launch sequence
// on the handle's stream with one host wait.  Reference: sofacontrol/baselines/koopman/koopman.py:75-170 (compute_policy, evaluate),
// koopman/koopman_utils.py:16-47 (add_measurement, get_zeta), baselines/ros.py:202-235 (the MPC node and its failure shift),
// baselines/mpc.py (get_target).
//
// THE POLICY.  B members, controller step Ts (the model's), simulation step dt_sim with Ts = r dt_sim, r an integer >= 1 (other ratios are
// refused: |Ts / dt_sim - round(Ts / dt_sim)| > 1e-9).  rollout_horizon = rh controller steps per period, n_keep = rh r sub-steps, rh <= N.
// Period p starts at t_p = t_start + p n_keep dt_sim (sgusto_loop_schedule, for t_k only).
//   reset     the ring of every member <- the `delays` older raw samples (y_hist, u_hist), oldest first, then the sample at the first
//             solve: y_0 = (C x0 + y_ref) + v0, or y_0 given when there is no plant, pushed with u_prev0 (the reference's
//             add_measurement(y, u_prev) in front of its first compute_policy).  Row 0 of the y record is y_0.
//   request   x0_p = W psi(zeta) of the ring as it stands (the KP_RING lift of koopman.hip, written into the QP's x0 behind the shared
//             prepare kernel).  Targets: the window at (t_p + phase_b) + Ts k; zf its last row when the cost has Qf; u_des N rows
//             (loop_prepare_kernel).
//   solve     the trust-region-free QP on the constant (A_d, B_d), d = 0, all members in one launch (slocp_plan_solve_dev_resident).
//   fix-up    a member whose QP reports a non-zero status goes on with the previous plan moved up ONE row, its last row held (ros.py:
//             223-227, whatever rh is); in period 0 such a member gets x0 in every state row and the scaled-down u0 in every input row;
//             the status is recorded either way (THE PLAN SHIFT of mpc_loop_host.h with row 0 as solved, the idle input u0 through the
//             input scaling, and the request copied into its record).
//   sub-steps s = 0..n_keep-1, all of them in ONE launch, one workgroup per member (koop_loop_advance_kernel):
//               1. u_s = uopt[s / r] * u_factor + u_offset          scale_up of the plan row of the controller step that has fired:
//                                                                    integer row arithmetic, no interpolation, no gain
//               2. x_{s+1} = A_p[i] x_s + B_p[i] u_s + d_p[i] (+ w_s), i the plant's nearest point to x_s (THE STEP RULE of tpwl_dev.h)
//               3. y_{s+1} = (C x_{s+1} + y_ref) + v_s  (measure_row), or y_{s+1} read from the given record Y_plant
//               3b. with a Y (skoop_loop_set_reproject): a sample outside Y = {y : A y <= b} is replaced by its Euclidean projection
//                  (koopman.py:150-151; the device function of spoly_project, poly_dev.h), with a plant and in replay alike -- the
//                  reference's evaluate projects whatever it is handed.  The status word of every sample is recorded (0 inside, 1
//                  projected, -1 no certified projection, -2 not finite); with -1 and -2 the raw sample is used.  The reset passes y_0
//                  through the stand-alone entry, the same function; the y_hist rows are taken as given.
//               4. push (y_{s+1}, u_s) -- with a recorded input: (y_{s+1}, U_applied_s) -- scaled down by the two operations of
//                  koop_push_kernel into the member's ring (the sample as used, behind 3b); the head advances inside the kernel, the
//                  host advances head / count of the skoop handle behind the enqueue.
// The reference reads its input tape at its own knots, so input_hold changes nothing and is not a parameter.
// Not offered: the start-up phase before t_delay, projecting the y_hist rows, input clipping, dU, input_nullspace,
// nonlinear_observer, weighting-mode plants, the lifted model as its own plant.  The host shell of a handle and of a run is
// gusto_loop_host.h, the constant-horizon QP and the plan shift mpc_loop_host.h, the target window gusto_loop_prep.h.
#include "koopman_host.h"
#include "tpwl_host.h"
#include "mpc_loop_host.h"

#include <algorithm>
#include <cmath>

namespace {

// scale_down / scale_up of KoopmanScaling (koopman_utils.py:98-107): two operations each, rounded on their own
__device__ __forceinline__ double koop_scale_down(double v, double off, double fac) { return (v - off) / fac; }
__device__ __forceinline__ double koop_scale_up(double v, double off, double fac) {
#pragma clang fp contract(off)
    const double p = v * fac;
    return p + off;
}

struct KlAdvArgs {
    int N, n_keep, r, np, m, ny;
    int plant;                          // 1: the TPWL plant is stepped and measured; 0: y_{s+1} is read from Yp
    int slots, head;                    // the ring: slots per member, the newest slot as the launch finds it (-1: none yet)
    const double *uopt;                 // the plans' inputs (B x N x m), scaled down as the QP holds them
    const double *C, *yref;             // (ny x np), (ny): the plant's measurement (plant only)
    const double *scale;                // [y_offset (ny) | y_factor (ny) | u_offset (m) | u_factor (m)] of the lift handle
    const double *W, *Vn;               // (steps x B x np), (steps x B x ny) or null; this launch reads steps w_step0 ..
    const double *Yp;                   // (B x rows_x x ny) the recorded measurements (rows as Y), or null
    const double *Ua;                   // (B x rows_u x m) the recorded applied inputs (rows as U), or null
    const double *x_in;                 // (B x np) plant states
    double *x_out, *y_out;              // (B x np) (may be x_in), (B x ny) the last measurement; or null
    double *ring;                       // (B x slots x (ny + m)) scaled samples
    double *X, *Y;                      // records (B x rows_x x .): row row0_x + s holds what sub-step s ends with
    double *U;                          // record (B x rows_u x m): row row0_u + s
    int32_t *idx;                       // (B x n_keep) the plant's point of every sub-step, or null
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
    ReprojArgs Yp_;                     // the admissible set Y and the two records of the re-projection (<true> instantiation only)
    double *yu_out;                     // (B x ny) the last used sample, or null
    int32_t *pj_out;                    // (B) its status word, or null
};

// LDS of the launch in doubles: x (np) | u (16) | y (ny) | y_ref (ny) | y_offset, y_factor (ny each) | u_offset, u_factor (16 each) |
// C (ny x np) | the staged step of tpwl_dev.h: partial sums of A x, B u (256 each), the point (2), the plant's panel A^T, B^T, d.
// np, ny and ny np are padded to even so that the panel is 16-byte aligned.  Without a plant only u and the scaling vectors are used.
__host__ __device__ inline int kl_even(int v) { return (v + 1) & ~1; }
// With Y (the <true> instantiation) the launch's LDS starts with wave 0's projection area, reproject_doubles(ny) doubles.
size_t kl_advance_lds_bytes(int np, int m, int ny, bool plant, bool proj = false) {
    const size_t d = (size_t)kl_even(np) + 16 + 4 * (size_t)kl_even(ny) + 2 * 16 + (size_t)kl_even(ny * np) + (proj ? reproject_doubles(ny) : 0);
    return srh::lds_request(sizeof(double) * (d + (plant ? tpwl::step_doubles(np, m, 256) + 2 : 0)));
}

// One workgroup of 256 threads per member, all n_keep sub-steps of a period.  The plant's region panel [A_d^T | B_d^T | d_d] sits in LDS
// and is reloaded only when the plant's nearest point changes (as rompc_loop_advance_kernel); C, y_ref and the scaling vectors are
// staged in LDS once per launch.  Fixed summation orders:
//   u_e   = uopt[s / r][e] * u_factor[e], then + u_offset[e]                      (two roundings: scale_up)
//   x'    = THE STEP RULE of tpwl_dev.h (+ w)
//   y_e   = measure_row (gusto_loop_prep.h): (C x')_e + y_ref[e], then + v_e
//   ring  = (y_e - y_offset[e]) / y_factor[e], (u_e - u_offset[e]) / u_factor[e]    (the two operations of koop_push_kernel)
// PROJ (the loop has a Y): behind step 3 and one barrier, wave 0 projects the sample onto Y (reproject_sample of gusto_loop_prep.h: the
// device function of spoly_project, its row of A and b in registers for the whole launch); behind a second barrier step 4 pushes the
// USED sample.  The raw sample keeps its record, the used one and its status word get theirs; the plant state is never touched.
// <false> is the kernel as it was: every PROJ part is compiled out.
template <bool PROJ>
__global__ __launch_bounds__(256) void koop_loop_advance_kernel(TpwlDev TL, KlAdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int np = a.np, m = a.m, ny = a.ny, N = a.N, w = ny + m;
    lptr xc = (lptr)smem + (PROJ ? reproject_doubles(ny) : 0);     // np     plant state
    lptr uc = xc + kl_even(np);                          // 16     raw input of the sub-step
    lptr yc = uc + 16;                                   // ny     raw measurement
    lptr yr = yc + kl_even(ny);                          // ny     y_ref
    lptr yoff = yr + kl_even(ny);                        // ny
    lptr yfac = yoff + kl_even(ny);                      // ny
    lptr uoff = yfac + kl_even(ny);                      // 16
    lptr ufac = uoff + 16;                               // 16
    lptr Cl = ufac + 16;                                 // ny x np
    tpwl::StepLds L;                                     //        partial sums of A x, B u | ip | the panel of region `cur`
    tpwl::step_carve(L, Cl + kl_even(ny * np), np, m, 256, 2);
    liptr ip = (liptr)(L.pb + 256);                      // (two doubles) plant point
    const size_t b = blockIdx.x;
    const int tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int npd = max(np, 1), S = max(1, 256 / npd), j = tid % npd, sl = tid / npd;
    cgptr uo = (cgptr)a.uopt + b * (size_t)N * m;
    cgptr sc = (cgptr)a.scale, Wd = (cgptr)a.W, Vd = (cgptr)a.Vn, Yp = (cgptr)a.Yp, Ua = (cgptr)a.Ua;
    gptr ring = (gptr)a.ring + b * (size_t)a.slots * w;
    for (int e = tid; e < ny; e += 256) {
        yoff[e] = sc[e];
        yfac[e] = sc[ny + e];
    }
    if (tid < m) {
        uoff[tid] = sc[2 * ny + tid];
        ufac[tid] = sc[2 * ny + m + tid];
    }
    if (a.plant) {
        for (int e = tid; e < np; e += 256) xc[e] = ((cgptr)a.x_in)[b * np + e];
        for (int e = tid; e < ny; e += 256) yr[e] = ((cgptr)a.yref)[e];
        for (int e = tid; e < ny * np; e += 256) Cl[e] = ((cgptr)a.C)[e];
    }
    [[maybe_unused]] ReprojWave yw;
    [[maybe_unused]] lptr yu = nullptr;
    [[maybe_unused]] int pj = 0;
    if constexpr (PROJ) {
        yu = reproject_used((lptr)smem);
        if (wave == 0) reproject_load(a.Yp_, ny, lane, yw);
    }
    __syncthreads();
    int cur = -1, head = a.head;
    for (int s = 0; s < a.n_keep; ++s) {
        const size_t rx = b * (size_t)a.rows_x + a.row0_x + s, ru = b * (size_t)a.rows_u + a.row0_u + s;
        head = head + 1 == a.slots ? 0 : head + 1;       // the slot of the sample (y_{s+1}, u_s)
        if (tid < m) {                                   // 1. the plan row of the controller step that has fired, scaled up
            const double u = koop_scale_up(uo[(size_t)(s / a.r) * m + tid], uoff[tid], ufac[tid]);
            uc[tid] = u;
            if (a.U) ((gptr)a.U)[ru * m + tid] = u;
            const double up = Ua != nullptr ? Ua[ru * m + tid] : u;
            ring[(size_t)head * w + ny + tid] = koop_scale_down(up, uoff[tid], ufac[tid]);
        }
        if (a.plant) {
            if (wave == 3) {                             // (the wave without input rows)
                const int i = tpwl::nearest_wave(TL, xc);
                if (lane == 0) {
                    const int p = (unsigned)i < (unsigned)TL.P ? i : 0;           // (a state that is not a number: no minimum)
                    ip[0] = p;
                    if (a.idx) ((giptr)a.idx)[b * (size_t)a.n_keep + s] = p;
                }
            }
            __syncthreads();
            tpwl::panel_load(L, TL, ip[0], cur, np, m, SRH_TID, 256);            // (the same for every thread; the barrier below covers the copies)
            __syncthreads();
            tpwl::step_slices(L, xc, uc, np, m, S, j, sl);                        // 2. the slices of both products
            __syncthreads();
            if (tid < np) {
                double v = tpwl::step_sum(L, np, S, tid);
                if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * np + tid];
                xc[tid] = v;
                if (a.X) ((gptr)a.X)[rx * np + tid] = v;
            }
            __syncthreads();
        }
        for (int e = tid; e < ny; e += 256) {            // 3. the measurement of the new plant state, 4. into the ring
            const double v = a.plant ? measure_row(Cl, e, np, xc, yr, Vd, ((size_t)(a.w_step0 + s) * a.B + b) * ny + e) : Yp[rx * ny + e];
            yc[e] = v;
            if (a.Y) ((gptr)a.Y)[rx * ny + e] = v;
            if constexpr (!PROJ) ring[(size_t)head * w + e] = koop_scale_down(v, yoff[e], yfac[e]);
        }
        if constexpr (PROJ) {
            __syncthreads();                             // the sample is complete
            if (wave == 0) {
                pj = reproject_sample(yw, a.Yp_.rows, ny, (clptr)yc, yu, (lptr)smem, lane);
                if (lane == 0 && a.Yp_.proj) ((giptr)a.Yp_.proj)[rx] = pj;
            }
            __syncthreads();
            for (int e = tid; e < ny; e += 256) {        // 4. the used sample into the ring
                const double v = yu[e];
                if (a.Yp_.Yu) ((gptr)a.Yp_.Yu)[rx * ny + e] = v;
                ring[(size_t)head * w + e] = koop_scale_down(v, yoff[e], yfac[e]);
            }
        }
    }
    __syncthreads();
    if constexpr (PROJ) {
        if (a.yu_out)
            for (int e = tid; e < ny; e += 256) ((gptr)a.yu_out)[b * ny + e] = yu[e];
        if (a.pj_out && tid == 0) ((giptr)a.pj_out)[b] = pj;
    }
    if (a.plant && a.x_out)
        for (int e = tid; e < np; e += 256) ((gptr)a.x_out)[b * np + e] = xc[e];
    if (a.y_out)
        for (int e = tid; e < ny; e += 256) ((gptr)a.y_out)[b * ny + e] = yc[e];
}

}  // namespace

struct skoop_loop : MpcLoopCore {
    skoop *koop = nullptr;
    stpwl *plant = nullptr;
    int np = 0, ny = 0, r = 1;          // plant states, measurements, simulation steps per controller step
    std::vector<double> Ch, yrh, u0h;   // host copies of C, y_ref and u0 (the reset forms y_0 from them)
    // cst: C | y_ref | u0; xp, ycur: where the plants and their measurements stand (the QP's horizon has d = 0)
    srh::DevBuf cst, xp, ycur;
    LoopRec XLrec, YPd, UAd;            // record: the requests (P x B x n); inputs: recorded measurements (B x (S + 1) x ny), inputs (B x S x m)
    // the re-projection onto Y (skoop_loop_set_reproject): Y on the host and on the device (A | b), where the used sample and its status
    // word stand (row 0 of the next run's records), the two records
    int yrows = 0;
    size_t lds_proj = 0;
    std::vector<double> YAh, Ybh;
    srh::DevBuf Yd, yucur, pjcur;
    LoopRec YUrec, PJrec;
    __attribute__((always_inline)) skoop_loop() {              // (inlined: no constructor among the library's dynamic symbols)
        recs.push_back(&XLrec); recs.push_back(&YUrec); recs.push_back(&PJrec);
        ins.push_back(&YPd); ins.push_back(&UAd);
    }
    ~skoop_loop() { drain(); }
    const double *scale() const { return koop->scale.as<double>(); }
    KlAdvArgs adv_args() const {
        KlAdvArgs a{};
        a.N = N; a.n_keep = n_keep; a.r = r; a.np = np; a.m = m; a.ny = ny;
        a.slots = koop->slots; a.head = koop->head;
        a.C = cst.as<double>(); a.yref = a.C + (size_t)ny * np;
        a.scale = scale();
        a.ring = koop->ring.as<double>();
        a.B = B;
        if (yrows) {
            a.Yp_.A = Yd.as<double>(); a.Yp_.b = a.Yp_.A + (size_t)yrows * ny; a.Yp_.rows = yrows;
        }
        return a;
    }
    // the fix-up: row 0 as solved, the scaled-down idle input behind a failed first solve
    ShiftArgs shift_args() const {
        ShiftArgs c{};
        c.N = N; c.n = n; c.m = m;
        c.u_idle = cst.as<double>() + (size_t)ny * np + ny;
        c.uoff = scale() + 2 * ny; c.ufac = c.uoff + m;
        return c;
    }
    // the launch, and behind it the ring's head and count as the n_keep pushes leave them
    int launch_advance(const KlAdvArgs &a) {
        if (a.Yp_.rows) koop_loop_advance_kernel<true><<<(unsigned)B, 256, lds_proj, stream>>>(a.plant ? plant->view() : TpwlDev{}, a);
        else koop_loop_advance_kernel<false><<<(unsigned)B, 256, lds, stream>>>(a.plant ? plant->view() : TpwlDev{}, a);
        SRH_CHECK_HIP(hipGetLastError());
        koop->head = (int)(((int64_t)koop->head + n_keep) % koop->slots);
        koop->count += n_keep;
        return SRH_OK;
    }
};

extern "C" {

int skoop_loop_create(skoop_loop_t **out, skoop_t *koop, const slocp_problem *prob, const double *A, const double *Bm, double Ts, stpwl_t *plant,
                      const double *C, const double *y_ref, const double *u0, double dt_sim, int rollout_horizon, int64_t max_steps_per_run) {
    SRH_REQUIRE(out && koop && prob && A && Bm, "skoop_loop_create: null argument");
    *out = nullptr;
    const int N = prob->N, n = koop->Nw, m = koop->m, ny = koop->ny;
    const int64_t B = koop->batch;
    SRH_REQUIRE(N >= 1 && Ts > 0.0 && dt_sim > 0.0, "skoop_loop_create: need a horizon N >= 1, Ts > 0 and dt_sim > 0");
    SRH_REQUIRE(prob->n_x == n && prob->n_u == m, "skoop_loop_create: the QP has n_x = %d, n_u = %d, the lift writes %d states and the model has n_u = %d",
                prob->n_x, prob->n_u, n, m);
    int rc;
    if ((rc = MpcLoopCore::check_problem("skoop_loop_create", prob, m))) return rc;
    SRH_REQUIRE(n <= 96, "skoop_loop_create: n_lift = %d exceeds the limit n_lift <= 96 of the QP", n);
    const double ratio = Ts / dt_sim, rr = std::round(ratio);
    SRH_REQUIRE(!(std::fabs(ratio - rr) > 1e-9) && rr >= 1.0 && rr <= 1e6,
                "skoop_loop_create: Ts / dt_sim = %.12g is not an integer >= 1 (the controller step must be a whole number of simulation steps)", ratio);
    SRH_REQUIRE(rollout_horizon >= 1 && rollout_horizon <= N, "skoop_loop_create: rollout_horizon = %d is outside 1 .. N = %d", rollout_horizon, N);
    const int r = (int)rr, n_keep = rollout_horizon * r;
    SRH_REQUIRE(max_steps_per_run >= n_keep, "skoop_loop_create: max_steps_per_run = %lld is below n_keep = %d", (long long)max_steps_per_run, n_keep);
    int np = 0;
    if (plant) {
        np = plant->n;
        SRH_REQUIRE(np <= 128, "skoop_loop_create: the plant's n_x = %d exceeds the limit n_x <= 128 of the advance kernel", np);
        SRH_REQUIRE(plant->m == m, "skoop_loop_create: the plant has n_u = %d, the model n_u = %d", plant->m, m);
        SRH_REQUIRE(plant->has_discrete, "skoop_loop_create: the plant has not been pre-discretised at dt_sim");
        SRH_REQUIRE(C && y_ref, "skoop_loop_create: a plant needs its measurement C (n_y x n_plant) and y_ref (n_y)");
    }
    const size_t lds = kl_advance_lds_bytes(np, m, ny, plant != nullptr);
    SRH_REQUIRE(lds <= (size_t)160 * 1024, "skoop_loop_create: the advance kernel needs %zu bytes of LDS (160 KiB available)", lds);
    skoop_loop *h = new skoop_loop();
    auto fail = [&](int code) { delete h; return code; };
    h->koop = koop; h->plant = plant; h->np = np; h->ny = ny; h->r = r; h->lds = lds;
    const char *what = "set up the advance kernel / the stream";
    if (hipFuncSetAttribute((const void *)koop_loop_advance_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return fail(loop_setup_failed("skoop_loop_create", what));
    const size_t D = sizeof(double), Bz = (size_t)B;
    if ((rc = h->setup("skoop_loop_create", what, N, n, m, prob->n_z, B, Ts, dt_sim, n_keep, max_steps_per_run, (size_t)prob->n_z))) return fail(rc);
    // the plant's records and noise have the plant's width, not the QP's
    h->Xrec.shape(D * std::max(np, 1), 1); h->Wd.shape(D * std::max(np, 1), 0);
    h->Yrec.shape(D * ny, 1); h->Vd.shape(D * ny, 0); h->XLrec.shape(D * n, 0, true);
    h->YPd.shape(D * ny, 1); h->UAd.shape(D * m, 0);
    h->YUrec.shape(D * ny, 1); h->PJrec.shape(sizeof(int32_t), 1);
    h->yrh.assign((size_t)ny, 0.0);
    h->u0h.assign((size_t)m, 0.0);
    if (plant) {
        h->Ch.assign(C, C + (size_t)ny * np);
        std::copy(y_ref, y_ref + ny, h->yrh.begin());
    }
    if (u0) std::copy(u0, u0 + m, h->u0h.begin());
    std::vector<double> c(h->Ch);                        // C (none without a plant) | y_ref | u0
    c.insert(c.end(), h->yrh.begin(), h->yrh.end());
    c.insert(c.end(), h->u0h.begin(), h->u0h.end());
    if ((rc = h->alloc_recs({&h->Yrec, &h->XLrec})) || (rc = h->cst.upload(c.data(), D * c.size())) ||
        (rc = h->xp.alloc(D * Bz * std::max(np, 1))) || (rc = h->ycur.alloc(D * Bz * ny)))
        return fail(rc);
    // the prepare kernel's state source (xcur) is zeros: the lift overwrites x0 behind it; the QP's horizon is (A, B), d = 0
    if (hipMemsetAsync(h->xcur.p, 0, D * Bz * n, h->stream) != hipSuccess) return fail(loop_setup_failed("skoop_loop_create", "tile the horizon"));
    if ((rc = h->make_horizon("skoop_loop_create", prob, A, Bm, nullptr))) return fail(rc);
    h->Xrec.row0 = h->xp.p; h->Yrec.row0 = h->ycur.p;
    *out = h;
    return SRH_OK;
}

int skoop_loop_destroy(skoop_loop_t *h) {
    SRH_REQUIRE(h, "skoop_loop_destroy: null handle");
    delete h;
    return SRH_OK;
}

int skoop_loop_set_target(skoop_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase) {
    return loop_set_target(h, "skoop_loop_set_target", T, t, z, u_des, phase);
}

int skoop_loop_reset(skoop_loop_t *h, const double *x0, const double *y0, const double *y_hist, const double *u_hist, const double *u_prev0,
                     const double *v0, double t_start) {
    SRH_REQUIRE(h, "skoop_loop_reset: null handle");
    SRH_REQUIRE(!h->plant || x0, "skoop_loop_reset: x0 is required");
    SRH_REQUIRE(h->plant || y0, "skoop_loop_reset: the loop was created without a plant (replay only): y0 is required");
    skoop *k = h->koop;
    SRH_REQUIRE(k->delay == 0 || (y_hist && u_hist), "skoop_loop_reset: the model has %d delays: y_hist and u_hist are required", k->delay);
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->have_state = false;
    const size_t B = (size_t)h->B, ny = h->ny, m = h->m, np = h->np, D = sizeof(double);
    // y_0 = (C x0 + y_ref) + v0 in the order of measure_row
    std::vector<double> y(B * ny), u(B * m);
    for (size_t b = 0; b < B; ++b)
        for (size_t e = 0; e < ny; ++e) {
            double v;
            if (h->plant) {
                v = 0.0;
                for (size_t c = 0; c < np; ++c) v = std::fma(h->Ch[e * np + c], x0[b * np + c], v);
                v += h->yrh[e];
                if (v0) v += v0[b * ny + e];
            } else {
                v = y0[b * ny + e];
            }
            y[b * ny + e] = v;
        }
    int rc;
    // with a Y the sample y_0 passes through it like every later one: the stand-alone entry runs the advance kernel's device function
    std::vector<double> yu(y);
    std::vector<int32_t> pj(B, 0);
    if (h->yrows && (rc = spoly_project_status(h->YAh.data(), h->Ybh.data(), h->yrows, (int)ny, y.data(), (int64_t)B, yu.data(), pj.data())))
        return rc;
    if ((rc = skoop_reset(k))) return rc;
    // the older samples, oldest first (taken as given: Y is not applied to them), then (y_0 as used, u_prev0): skoop_push scales them down
    std::vector<double> yj(B * ny), uj(B * m);
    for (int j = 0; j < k->delay; ++j) {
        for (size_t b = 0; b < B; ++b) {
            std::copy(y_hist + (b * k->delay + j) * ny, y_hist + (b * k->delay + j + 1) * ny, yj.begin() + b * ny);
            std::copy(u_hist + (b * k->delay + j) * m, u_hist + (b * k->delay + j + 1) * m, uj.begin() + b * m);
        }
        if ((rc = skoop_push(k, yj.data(), uj.data()))) return rc;
    }
    for (size_t b = 0; b < B; ++b)
        for (size_t e = 0; e < m; ++e) u[b * m + e] = u_prev0 ? u_prev0[b * m + e] : h->u0h[e];
    if ((rc = skoop_push(k, yu.data(), u.data()))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(k->stream));
    k->push_pending = false;
    if (h->plant) SRH_CHECK_HIP(hipMemcpy(h->xp.p, x0, D * B * np, hipMemcpyHostToDevice));
    SRH_CHECK_HIP(hipMemcpy(h->ycur.p, y.data(), D * B * ny, hipMemcpyHostToDevice));
    if (h->yrows) {
        SRH_CHECK_HIP(hipMemcpy(h->yucur.p, yu.data(), D * B * ny, hipMemcpyHostToDevice));
        SRH_CHECK_HIP(hipMemcpy(h->pjcur.p, pj.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice));
    }
    h->t_start = t_start; h->k = 0; h->have_state = true;
    return SRH_OK;
}

}  // extern "C"

namespace {

// a run, with the two records of the re-projection when the loop has a Y (Y_used, proj: null without one)
int koop_loop_run(skoop_loop *h, const char *who, int periods, const double *W, const double *V, const double *Y_plant, const double *U_applied,
                  double *X, double *Y, double *U, double *Xlift, double *J, int32_t *status, int32_t *iters, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(periods >= 1, "%s: periods must be positive", who);
    SRH_REQUIRE(h->have_state, "%s: no measurement history yet (call skoop_loop_reset first)", who);
    SRH_REQUIRE(h->plant || Y_plant, "%s: the loop was created without a plant (replay only): Y_plant is required", who);
    h->YUrec.host = Y_used; h->PJrec.host = proj;
    const bool replay = Y_plant != nullptr;
    h->Wd.host = (void *)((W && !replay) ? W : nullptr); h->Vd.host = (void *)((V && !replay) ? V : nullptr);
    h->YPd.host = (void *)Y_plant; h->UAd.host = (void *)U_applied;
    h->Xrec.host = (h->plant && !replay) ? X : nullptr; h->Yrec.host = Y; h->Urec.host = U; h->XLrec.host = Xlift;
    h->Jrec.host = J; h->Srec.host = status; h->Irec.host = iters;
    // the prepare kernel copies zeros into x0 and forms the target window; the ring lift overwrites x0 behind it
    const PrepUnit u{h->xcur.as<double>(), nullptr, nullptr, h->zf_dev(), false};
    return loop_run_periods(h, "skoop_loop_run", periods, u, [&](int p, const PrepArgs &a, const LoopRows &r) -> int {
        int rc;
        KoopLiftArgs la{};
        la.rows = h->B; la.ring = h->koop->ring.as<double>(); la.head = h->koop->head; la.out = a.x0;
        if ((rc = koop_launch_lift(h->koop, KP_RING, la, h->stream))) return rc;
        if ((rc = h->solve(p, a))) return rc;
        ShiftArgs c = h->shift_args();
        h->shift_in_place(c, p, a);
        c.xlift = h->XLrec.as<double>() + (size_t)p * (size_t)h->B * h->n;
        if ((rc = h->launch_shift(c))) return rc;
        h->take_solution();
        KlAdvArgs v = h->adv_args();
        v.plant = replay ? 0 : 1;
        v.uopt = h->uopt.as<double>();
        v.W = h->Wd.host ? h->Wd.as<double>() : nullptr; v.Vn = h->Vd.host ? h->Vd.as<double>() : nullptr; v.w_step0 = r.w_step0;
        v.Yp = replay ? h->YPd.as<double>() : nullptr; v.Ua = U_applied ? h->UAd.as<double>() : nullptr;
        v.x_in = h->xp.as<double>(); v.x_out = h->xp.as<double>(); v.y_out = h->ycur.as<double>();
        v.X = h->Xrec.host ? h->Xrec.as<double>() : nullptr; v.Y = Y ? h->Yrec.as<double>() : nullptr; v.U = U ? h->Urec.as<double>() : nullptr;
        v.rows_x = r.rows_x; v.row0_x = r.row0_x; v.rows_u = r.rows_u; v.row0_u = r.row0_u;
        v.Yp_.Yu = Y_used ? h->YUrec.as<double>() : nullptr; v.Yp_.proj = proj ? h->PJrec.as<int32_t>() : nullptr;
        v.yu_out = h->yucur.as<double>(); v.pj_out = h->pjcur.as<int32_t>();
        return h->launch_advance(v);
    });
}

}  // namespace

extern "C" {

int skoop_loop_run(skoop_loop_t *h, int periods, const double *W, const double *V, const double *Y_plant, const double *U_applied, double *X,
                   double *Y, double *U, double *Xlift, double *J, int32_t *status, int32_t *iters) {
    SRH_REQUIRE(h, "skoop_loop_run: null handle");
    return koop_loop_run(h, "skoop_loop_run", periods, W, V, Y_plant, U_applied, X, Y, U, Xlift, J, status, iters, nullptr, nullptr);
}

int skoop_loop_run_reprojected(skoop_loop_t *h, int periods, const double *W, const double *V, const double *Y_plant, const double *U_applied,
                               double *X, double *Y, double *U, double *Xlift, double *J, int32_t *status, int32_t *iters, double *Y_used,
                               int32_t *proj) {
    SRH_REQUIRE(h, "skoop_loop_run_reprojected: null handle");
    SRH_REQUIRE(h->yrows, "skoop_loop_run_reprojected: the loop has no Y (skoop_loop_set_reproject)");
    return koop_loop_run(h, "skoop_loop_run_reprojected", periods, W, V, Y_plant, U_applied, X, Y, U, Xlift, J, status, iters, Y_used, proj);
}

int skoop_loop_set_reproject(skoop_loop_t *h, const double *A, const double *b, int rows) {
    SRH_REQUIRE(h, "skoop_loop_set_reproject: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->have_state = false;               // the first sample of the ring was pushed under the previous rule: a reset states it anew
    if (!A || !b) {
        h->yrows = 0;
        return SRH_OK;
    }
    const int ny = h->ny;
    SRH_REQUIRE(ny <= poly::PN && rows > 0 && rows <= poly::PM,
                "skoop_loop_set_reproject: Y needs n_y <= 16 and 0 < rows <= 64 (got n_y = %d, rows = %d)", ny, rows);
    for (int i = 0; i < rows * ny; ++i) SRH_REQUIRE(std::isfinite(A[i]), "skoop_loop_set_reproject: Y is not finite (A, row %d)", i / ny);
    for (int i = 0; i < rows; ++i) SRH_REQUIRE(std::isfinite(b[i]), "skoop_loop_set_reproject: Y is not finite (b, row %d)", i);
    const size_t lds = kl_advance_lds_bytes(h->np, h->m, ny, h->plant != nullptr, true);
    SRH_REQUIRE(lds <= (size_t)160 * 1024, "skoop_loop_set_reproject: the advance kernel needs %zu bytes of LDS (160 KiB available)", lds);
    if (hipFuncSetAttribute((const void *)koop_loop_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return loop_setup_failed("skoop_loop_set_reproject", "set up the advance kernel");
    std::vector<double> c(A, A + (size_t)rows * ny);
    c.insert(c.end(), b, b + rows);
    const size_t D = sizeof(double), B = (size_t)h->B;
    int rc;
    if ((rc = h->Yd.upload(c.data(), D * c.size())) || (rc = h->yucur.alloc(D * B * ny)) || (rc = h->pjcur.alloc(sizeof(int32_t) * B)) ||
        (!h->YUrec.d.p && (rc = h->alloc_recs({&h->YUrec, &h->PJrec}))))
        return rc;
    h->YAh.assign(A, A + (size_t)rows * ny); h->Ybh.assign(b, b + rows);
    h->YUrec.row0 = h->yucur.p; h->PJrec.row0 = h->pjcur.p;
    h->lds_proj = lds; h->yrows = rows;
    return SRH_OK;
}

int skoop_loop_last_inputs(skoop_loop_t *h, double *x0, double *z, double *zf, double *u_des) {
    return mpc_last_inputs(h, "skoop_loop_last_inputs", x0, z, zf, u_des);
}

int skoop_loop_last_plan(skoop_loop_t *h, double *xopt, double *uopt) { return loop_last_plan(h, "skoop_loop_last_plan", xopt, uopt); }

int skoop_loop_stats(skoop_loop_t *h, int64_t *steps, int64_t *waits_last_run) { return loop_stats(h, "skoop_loop_stats", steps, waits_last_run); }

int skoop_loop_fixup(skoop_loop_t *h, const double *xopt_prev, const double *uopt_prev, const double *xopt, const double *uopt, const double *x0,
                     const int32_t *status, int first, double *xopt_out, double *uopt_out) {
    SRH_REQUIRE(h && xopt && uopt && x0 && status && xopt_out && uopt_out, "skoop_loop_fixup: null argument");
    SRH_REQUIRE(first || (xopt_prev && uopt_prev), "skoop_loop_fixup: the previous plan is required behind the first period");
    return mpc_shift_alone(h, h->shift_args(), xopt_prev, uopt_prev, xopt, uopt, x0, status, first, xopt_out, uopt_out, nullptr);
}

}  // extern "C"

namespace {

int koop_loop_advance(skoop_loop *h, const char *who, const double *uopt, const double *x, const double *W, const double *V, const double *Y_plant,
                      const double *U_applied, double *X, double *Y, double *U, int32_t *idx, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(h->plant || Y_plant, "%s: the loop was created without a plant (replay only): Y_plant is required", who);
    SRH_REQUIRE(Y_plant || (x && X), "%s: a stepped plant needs its states x and the record X", who);
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, m = h->m, ny = h->ny, np = h->np, nk = h->n_keep;
    const bool replay = Y_plant != nullptr;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipStreamSynchronize(h->koop->stream));
    h->have_state = false;               // the ring moves on, the loop's plant state and measurement do not
    int rc;
    srh::DevBuf duo, dx, dW, dV, dYp, dUa, dX, dY, dU, di, dYu, dPj;
    if ((Y_used && (rc = dYu.alloc(D * B * (nk + 1) * ny))) || (proj && (rc = dPj.alloc(sizeof(int32_t) * B * (nk + 1))))) return rc;
    // X, Y and Y_plant carry a row in front (row 0: where the launch starts), as the records of a run do; it is not copied back
    if ((rc = duo.upload(uopt, D * B * N * m)) || (!replay && (rc = dx.upload(x, D * B * np))) ||
        (W && !replay && (rc = dW.upload(W, D * nk * B * np))) || (V && !replay && (rc = dV.upload(V, D * nk * B * ny))) ||
        (replay && (rc = dYp.upload(Y_plant, D * B * (nk + 1) * ny))) || (U_applied && (rc = dUa.upload(U_applied, D * B * nk * m))) ||
        (!replay && (rc = dX.alloc(D * B * (nk + 1) * np))) || (rc = dY.alloc(D * B * (nk + 1) * ny)) || (rc = dU.alloc(D * B * nk * m)) ||
        (rc = di.alloc(sizeof(int32_t) * B * nk)))
        return rc;
    SRH_CHECK_HIP(hipMemsetAsync(di.p, 0xff, sizeof(int32_t) * B * nk, h->stream));                 // (-1 where no plant is stepped)
    KlAdvArgs v = h->adv_args();
    v.plant = replay ? 0 : 1;
    v.uopt = duo.as<double>();
    v.W = (W && !replay) ? dW.as<double>() : nullptr; v.Vn = (V && !replay) ? dV.as<double>() : nullptr; v.w_step0 = 0;
    v.Yp = replay ? dYp.as<double>() : nullptr; v.Ua = U_applied ? dUa.as<double>() : nullptr;
    v.x_in = dx.as<double>();
    v.X = replay ? nullptr : dX.as<double>(); v.Y = dY.as<double>(); v.U = dU.as<double>(); v.idx = di.as<int32_t>();
    v.rows_x = (int64_t)nk + 1; v.row0_x = 1; v.rows_u = (int64_t)nk; v.row0_u = 0;
    v.Yp_.Yu = Y_used ? dYu.as<double>() : nullptr; v.Yp_.proj = proj ? dPj.as<int32_t>() : nullptr;
    if ((rc = loop_wait(h->launch_advance(v), h->stream))) return rc;
    // rows 1 .. n_keep of the n_keep + 1 row blocks -> the caller's (B x n_keep x .) arrays
    auto rows = [&](const srh::DevBuf &d, void *dst, size_t w) { return loop_rows_to_host(d, dst, B, nk, w, 1); };
    if ((!replay && (rc = rows(dX, X, D * np))) || (rc = rows(dY, Y, D * ny)) || (rc = dU.download(U, D * B * nk * m)) ||
        (rc = di.download(idx, sizeof(int32_t) * B * nk)) || (Y_used && (rc = rows(dYu, Y_used, D * ny))) ||
        (proj && (rc = rows(dPj, proj, sizeof(int32_t)))))
        return rc;
    return SRH_OK;
}

}  // namespace

extern "C" {

int skoop_loop_advance(skoop_loop_t *h, const double *uopt, const double *x, const double *W, const double *V, const double *Y_plant,
                       const double *U_applied, double *X, double *Y, double *U, int32_t *idx) {
    SRH_REQUIRE(h && uopt && Y && U && idx, "skoop_loop_advance: null argument");
    return koop_loop_advance(h, "skoop_loop_advance", uopt, x, W, V, Y_plant, U_applied, X, Y, U, idx, nullptr, nullptr);
}

int skoop_loop_advance_reprojected(skoop_loop_t *h, const double *uopt, const double *x, const double *W, const double *V, const double *Y_plant,
                                   const double *U_applied, double *X, double *Y, double *U, int32_t *idx, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(h && uopt && Y && U && idx && Y_used && proj, "skoop_loop_advance_reprojected: null argument");
    SRH_REQUIRE(h->yrows, "skoop_loop_advance_reprojected: the loop has no Y (skoop_loop_set_reproject)");
    return koop_loop_advance(h, "skoop_loop_advance_reprojected", uopt, x, W, V, Y_plant, U_applied, X, Y, U, idx, Y_used, proj);
}

}  // extern "C"
