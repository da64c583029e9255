// Batched closed loop on a resident TPWL GuSTO plan: every rollout of the plan's batch is its own receding-horizon loop -- plan, apply
// n_keep inputs to a TPWL plant, shift, re-plan from the plant state -- and a whole run of periods is one launch sequence on the handle's
// stream with one host wait.  Reference: sofacontrol/scp/standalone.py:29-33 (targets, first guess), scp/ros.py:109-114 (shift),
// tpwl/controllers.py:298-333 (the scp controller's interpolated plan and feedback law), tpwl/tpwl.py:160-168, 336-339 (plant step).
// The solve itself is sgusto_plan_solve_dev (gusto.hip); this unit is the glue around it: loop_prepare_kernel (gusto_loop_prep.h) turns
// the previous period's output into the next solve's input, loop_advance_kernel runs the plant under the feedback law for the n_keep
// sub-steps.  The host shell of a handle and of a run -- shared with the four other loop units -- is gusto_loop_host.h, the observed
// sub-step chain -- shared with ilqr_loop.hip -- loop_observed_host.h.
#include "loop_observed_host.h"

namespace {

struct AdvArgs {
    int N, n_keep, nz;
    const double *xopt, *uopt;          // the plans (B x (N+1) x n), (B x N x m)
    const double *K;                    // (P x m x n) gains at the planner's points, or null
    const double *H;                    // (nz x n)
    const double *W;                    // (steps x B x n) disturbances, or null; this launch reads steps w_step0 ..
    const int32_t *js;                  // (n_keep) plan interval of every sub-step
    const double *theta;                // (n_keep) position inside it
    const double *x_in;                 // (B x n)
    double *x_out;                      // (B x n) or null (may be x_in)
    double *X, *Z, *U;                  // records: row row0 + s of rollout b (X may be null)
    int32_t *ip, *ig;                   // (B x n_keep) points picked, or null
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
    int s0, s1;                         // the sub-steps of this launch: s0 <= s < s1 (the whole period without an observer)
    // with an observer (loop_advance_kernel<true>): the law reads the estimate, and every sub-step ends with a measurement
    const double *xhat;                 // (B x n) the filters' estimates
    const double *C, *y_ref, *Vn;       // (ny x n), (ny) or null, (steps x B x ny) measurement noise or null (indexed as W)
    double *Y;                          // (B x rows_u x ny) record, rows as U: the batched filter reads its y from it
    int ny;
};

// One workgroup per rollout, all n_keep sub-steps.  The plant's region panel [A_d^T | B_d^T | d_d] sits in LDS and is reloaded only when
// the plant's nearest point changes (as rollout_staged_kernel, tpwl.hip); the state, the plan point x_bar and x - x_bar stay in LDS
// for the whole launch.  Per sub-step: waves 0-2 interpolate the plan; wave 0 searches the plant's table at x while wave 1 searches the
// planner's at x_bar (tpwl::nearest_wave both: one tie rule); the four waves form K (x - x_bar) a row each; the plant step is THE STEP
// RULE of tpwl_dev.h, plan points, z and y the rules of gusto_loop_prep.h.
// OBS: the observed loop's sub-step.  The law reads the filter's estimate x_hat in place of x, and the sub-step ends with the measurement
// y = C x' + y_ref (+ v).  The filter itself is another kernel (512 threads, up to 160 KB of LDS), so a launch then covers one sub-step
// and the region panel is loaded per launch.
template <bool OBS>
__global__ __launch_bounds__(256) void loop_advance_kernel(TpwlDev TP, TpwlDev TL, AdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = TL.n, m = TL.m, N = a.N, nz = a.nz;
    lptr xc = (lptr)smem;                                // n      plant state
    lptr xb = xc + n;                                    // n      x_bar
    lptr dx = xb + n;                                    // n      x - x_bar
    lptr ub = dx + n;                                    // 16     u_bar
    lptr uc = ub + 16;                                   // 16     u
    tpwl::StepLds L;                                     //        partial sums, (two doubles) plant point and gain point, the panel of region `cur`
    lptr xh = tpwl::step_carve(L, uc + 16, n, m, 256, 2);        // n      OBS: the estimate
    liptr ip = (liptr)(L.pb + 256);
    clptr xl = OBS ? xh : xc;                            //        what the law reads
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int S = max(1, 256 / n), j = tid % n, sl = tid / n;
    cgptr xo = (cgptr)a.xopt + b * (size_t)(N + 1) * n, uo = (cgptr)a.uopt + b * (size_t)N * m;
    cgptr Kt = (cgptr)a.K, H = (cgptr)a.H, Wd = (cgptr)a.W, thg = (cgptr)a.theta, xin = (cgptr)a.x_in;
    cgiptr jsg = (cgiptr)a.js;
    for (int e = tid; e < n; e += 256) xc[e] = xin[b * n + e];
    if (OBS)
        for (int e = tid; e < n; e += 256) xh[e] = ((cgptr)a.xhat)[b * n + e];
    __syncthreads();
    int cur = -1;
    for (int s = a.s0; s < a.s1; ++s) {
        const int js = jsg[s];
        const double th = thg[s];
        if (tid < n) {                                   // (n <= 128: waves 0 and 1)
            const double v = plan_at(xo, n, js, js + 1, th, tid);
            xb[tid] = v;
            dx[tid] = xl[tid] - v;
        } else if (tid >= 128 && tid < 128 + m) {        // the input is held over the last interval (controllers.py:299)
            ub[tid - 128] = plan_at(uo, m, js, min(js + 1, N - 1), th, tid - 128);
        }
        __syncthreads();
        if (wave == 0) {
            const int i = tpwl::nearest_wave(TL, xc);
            if (lane == 0) ip[0] = (unsigned)i < (unsigned)TL.P ? i : 0;           // (a state that is not a number: no minimum)
        } else if (wave == 1 && Kt != nullptr) {
            const int i = tpwl::nearest_wave(TP, xb);
            if (lane == 0) ip[1] = (unsigned)i < (unsigned)TP.P ? i : 0;
        }
        __syncthreads();
        const int p = ip[0];
        tpwl::panel_load(L, TL, p, cur, n, m, tid, blockDim.x);            // (the same for every thread; the barrier below covers the copies)
        if (Kt != nullptr) {
            cgptr Kg = Kt + (size_t)ip[1] * m * n;
            for (int e = wave; e < m; e += 4) {
                double acc = 0.0;
                for (int c = lane; c < n; c += 64) acc = fma(Kg[e * n + c], dx[c], acc);
                acc = wg::wave_sum(acc);
                if (lane == 0) uc[e] = ub[e] + acc;
            }
        } else if (tid < m) {
            uc[tid] = ub[tid];
        }
        __syncthreads();
        tpwl::step_slices(L, xc, uc, n, m, S, j, sl);
        __syncthreads();
        if (tid < n) {
            double v = tpwl::step_sum(L, n, S, tid);
            if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * n + tid];
            xc[tid] = v;
            if (a.X) ((gptr)a.X)[(b * (size_t)a.rows_x + a.row0_x + s) * n + tid] = v;
        } else if (tid >= 128 && tid < 128 + m) {
            ((gptr)a.U)[(b * (size_t)a.rows_u + a.row0_u + s) * m + (tid - 128)] = uc[tid - 128];
        } else if (tid == 255) {
            if (a.ip) a.ip[b * a.n_keep + s] = p;
            if (a.ig) a.ig[b * a.n_keep + s] = Kt != nullptr ? ip[1] : -1;
        }
        __syncthreads();
        // z = H x.  xc is next written behind two barriers of the next sub-step.
        for (int e = tid; e < nz; e += 256) ((gptr)a.Z)[(b * (size_t)a.rows_x + a.row0_x + s) * nz + e] = out_row(H, e, n, xc);
        if (OBS) {
            cgptr Cg = (cgptr)a.C, yr = (cgptr)a.y_ref, Vn = (cgptr)a.Vn;
            for (int e = tid; e < a.ny; e += 256)
                ((gptr)a.Y)[(b * (size_t)a.rows_u + a.row0_u + s) * a.ny + e] =
                    measure_row(Cg, e, n, xc, yr, Vn, ((size_t)(a.w_step0 + s) * a.B + b) * a.ny + e);
        }
    }
    if (a.x_out)
        for (int e = tid; e < n; e += 256) ((gptr)a.x_out)[b * n + e] = xc[e];
}

size_t advance_lds_bytes(int n, int m, bool observed) {
    return srh::lds_request(sizeof(double) * ((size_t)3 * n + 16 + 16 + 2 + tpwl::step_doubles(n, m, 256) + (observed ? n : 0)));
}

// THE CHAINED POLICY (the reference's default, mpc=False: tpwl/controllers.py:269-274, 298-315).  Plan k + 1 starts from the END of the
// part of plan k that the robot follows -- the plan point at tau_end = n_keep dt_sim, (j_end, theta_end) of sgusto_loop_end_row --
// not from the plant: the plans no longer depend on the plant, only the law and the filter close the loop.  loop_chain_kernel, behind
// the solve of a chained period, forms that point for every member (x_next) and the period's rows of the nominal tape the reference
// stitches (x_opt / u_opt of save_controller_info): row s = 0..n_keep of a period is the plan point at tau = s dt_sim, s = n_keep the
// end point.  All of it by plan_at, with the (j, theta) the advance kernel reads: a tape row has the bits of that kernel's x_bar / u_bar.
struct ChainArgs {
    int N, n, m, n_keep;
    int j_end;                          // the plan interval and the position inside it of tau_end
    double theta_end;
    const double *xopt, *uopt;          // the plans (B x (N+1) x n), (B x N x m)
    const int32_t *js;                  // (n_keep) the schedule of the sub-steps, as AdvArgs
    const double *theta;
    double *x_next;                     // (B x n) the next period's start state, or null
    double *Xbar, *Ubar;                // tape records: row row0 + s of member b, or null
    int64_t rows, row0, B;              // rows per member of both records
    int x_row0;                         // whether row s = 0 of Xbar is written (period 0 after a reset: later it is the old plan's end, which
                                        // the reference keeps -- x_opt_new[1:] is appended --, while u_opt[:-1] gives way to the new plan's row)
};

// One thread per lerp: element e = (s, c) of member b, s = 0..n_keep, c < n a state, otherwise input c - n; consecutive threads write
// consecutive addresses of a record row.  No LDS, no cross-lane traffic: any n <= 128, m <= 16, B.
__global__ __launch_bounds__(256) void loop_chain_kernel(ChainArgs a) {
    const int n = a.n, m = a.m, N = a.N, w = n + m;
    const size_t per = (size_t)(a.n_keep + 1) * w;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)a.B * per) return;
    const size_t b = g / per;
    const int e = (int)(g - b * per), s = e / w, c = e - s * w;
    const bool end = s == a.n_keep;
    const int j = end ? a.j_end : ((cgiptr)a.js)[s];
    const double th = end ? a.theta_end : ((cgptr)a.theta)[s];
    const size_t row = b * (size_t)a.rows + a.row0 + s;
    if (c < n) {
        const double v = plan_at((cgptr)a.xopt + b * (size_t)(N + 1) * n, n, j, j + 1, th, c);
        if (end && a.x_next) ((gptr)a.x_next)[b * n + c] = v;
        if (a.Xbar && (s > 0 || a.x_row0)) ((gptr)a.Xbar)[row * n + c] = v;
    } else if (a.Ubar) {
        ((gptr)a.Ubar)[row * m + (c - n)] = plan_at((cgptr)a.uopt + b * (size_t)N * m, m, j, min(j + 1, N - 1), th, c - n);
    }
}

}  // namespace

struct sgusto_loop : LoopCore {
    sgusto_plan_t *plan = nullptr;
    stpwl *planner = nullptr, *plant = nullptr;
    bool has_Qzf = false, has_K = false;
    // the observed loop: the attached filters (sgusto_loop_set_observer) and whether the state is an observed one (plant states and
    // estimates installed together by sgusto_loop_reset_observed)
    sekf_batch *obs = nullptr;
    int ny = 0;
    bool observed_state = false;
    size_t lds_obs = 0;
    srh::DevBuf K, zf;
    LoopRec Erec;                       // observed loop: the filters' status (P x B); Y is (B x S x ny) here
    // the chained policy (sgusto_loop_set_chained): the next period's start state (B x n; it holds one whenever k > 0), the end row of
    // the schedule, and the tape records (B x (S + 1) x n), (B x (S + 1) x m), allocated by the first run that asks for them
    bool chained = false;
    int j_end = 0;
    double theta_end = 0.0;
    srh::DevBuf xchain;
    LoopRec XBrec, UBrec;
    __attribute__((always_inline)) sgusto_loop() { recs.insert(recs.end(), {&Erec, &XBrec, &UBrec}); }       // (inlined: no constructor among the library's dynamic symbols)
    ~sgusto_loop() { drain(); }
    AdvArgs adv_args() const {
        AdvArgs a{};
        a.N = N; a.n_keep = n_keep; a.nz = nz;
        a.K = has_K ? K.as<double>() : nullptr;
        a.H = planner->H.as<double>();
        a.js = js.as<int32_t>(); a.theta = theta.as<double>();
        a.B = B;
        a.s0 = 0; a.s1 = n_keep;
        return a;
    }
    ChainArgs chain_args() const {
        ChainArgs c{};
        c.N = N; c.n = n; c.m = m; c.n_keep = n_keep; c.j_end = j_end; c.theta_end = theta_end;
        c.js = js.as<int32_t>(); c.theta = theta.as<double>();
        c.B = B;
        return c;
    }
    int launch_chain(const ChainArgs &c) const {
        const size_t blocks = ((size_t)B * (n_keep + 1) * (n + m) + 255) / 256;
        SRH_REQUIRE(blocks <= (size_t)0x7fffffff, "sgusto_loop: the chain kernel's grid of %zu workgroups exceeds 2^31 - 1", blocks);
        loop_chain_kernel<<<(unsigned)blocks, 256, 0, stream>>>(c);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    int launch_advance(const AdvArgs &a) const {
        loop_advance_kernel<false><<<(unsigned)B, 256, lds, stream>>>(planner->view(), plant->view(), a);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    // The observed sub-step chain of one period (loop_observed_host.h): a launch covers one sub-step.  v: the arguments of the whole
    // period (records, plan, W / Vn, x_in / x_out); XH / xh_rows / xh_row0: the estimate record and the row of sub-step 0's estimate;
    // E: the period's status entry (B); pick: (B x n_keep) filter regions or null.
    int launch_observed_chain(AdvArgs v, double *XH, int64_t xh_rows, int64_t xh_row0, int32_t *E, int32_t *pick) const {
        v.xhat = obs->x_dev(); v.C = obs->C.as<double>(); v.y_ref = obs->yref_dev(); v.ny = ny;
        return loop_observed_chain(this, obs, n_keep, ObsRecs{v.U, v.Y, v.rows_u, v.row0_u, XH, xh_rows, xh_row0, E, pick, n_keep}, [&](int64_t s) -> int {
            v.s0 = (int)s; v.s1 = (int)s + 1;
            loop_advance_kernel<true><<<(unsigned)B, 256, lds_obs, stream>>>(planner->view(), plant->view(), v);
            SRH_CHECK_HIP(hipGetLastError());
            return SRH_OK;
        });
    }
};

extern "C" {

int sgusto_loop_schedule(int N, double dt, double dt_sim, int n_keep, double t_start, int64_t k, double *t_k, int *idx0, int32_t *j,
                         double *theta) {
#pragma clang fp contract(off)          // every product and sum rounded on its own, as the numpy statement of the schedule
    SRH_REQUIRE(N >= 1 && dt > 0.0 && dt_sim > 0.0 && n_keep >= 1 && k >= 0, "sgusto_loop_schedule: bad argument");
    const double step = (double)n_keep * dt_sim;
    const double tk = t_start + (double)k * step;
    if (t_k) *t_k = tk;
    if (idx0) {
        *idx0 = 0;
        if (k > 0) {
            // (at n_keep dt_sim == N dt the two sums may round an ulp apart and no row reaches t_k: the last row is held throughout)
            const double tp = t_start + (double)(k - 1) * step;
            int i0 = N;
            for (int i = 0; i <= N; ++i) {
                const double ti = tp + dt * (double)i;
                if (ti >= tk) { i0 = i; break; }
            }
            *idx0 = i0;
        }
    }
    for (int s = 0; s < n_keep; ++s) {
        const double tau = (double)s * dt_sim;
        const double q = tau / dt;
        const int js = std::min((int)q, N - 1);
        if (j) j[s] = js;
        if (theta) {
            const double back = (double)js * dt;
            theta[s] = (tau - back) / dt;
        }
    }
    return SRH_OK;
}

int sgusto_loop_end_row(int N, double dt, double dt_sim, int n_keep, int32_t *j_end, double *theta_end) {
#pragma clang fp contract(off)          // as sgusto_loop_schedule: the rule of a sub-step at tau = n_keep dt_sim
    SRH_REQUIRE(N >= 1 && dt > 0.0 && dt_sim > 0.0 && n_keep >= 1, "sgusto_loop_end_row: bad argument");
    const double tau = (double)n_keep * dt_sim;
    const double q = tau / dt;
    const int je = std::min((int)q, N - 1);
    if (j_end) *j_end = je;
    if (theta_end) {
        const double back = (double)je * dt;
        *theta_end = (tau - back) / dt;
    }
    return SRH_OK;
}

int sgusto_loop_create(sgusto_loop_t **out, sgusto_plan_t *plan, stpwl_t *planner_model, stpwl_t *plant, double dt_sim, int n_keep,
                       int64_t max_steps_per_run) {
    SRH_REQUIRE(out && plan && planner_model && plant, "sgusto_loop_create: null argument");
    int N, n, m, nz, has_Qzf;
    int64_t B;
    double dt;
    int rc = sgusto_plan_dims(plan, &N, &n, &m, &nz, &B, &dt, &has_Qzf);
    if (rc) return rc;
    SRH_REQUIRE(n <= 128 && m <= 16, "sgusto_loop_create: n_x = %d, n_u = %d exceed the limits n_x <= 128, n_u <= 16", n, m);
    SRH_REQUIRE(planner_model->n == n && planner_model->m == m && planner_model->has_discrete,
                "sgusto_loop_create: the planner's model (n_x = %d, n_u = %d) is not the pre-discretised model of the plan (n_x = %d, n_u = %d)",
                planner_model->n, planner_model->m, n, m);
    SRH_REQUIRE(planner_model->nz == nz && planner_model->H.p, "sgusto_loop_create: the planner's model has no output map of the plan's n_z = %d", nz);
    SRH_REQUIRE(plant->n == n && plant->m == m, "sgusto_loop_create: the plant has n_x = %d, n_u = %d, the plan n_x = %d, n_u = %d",
                plant->n, plant->m, n, m);
    SRH_REQUIRE(plant->has_discrete, "sgusto_loop_create: the plant has not been pre-discretised at dt_sim");
    if ((rc = loop_check_periods("sgusto_loop_create", N, dt, dt_sim, n_keep, max_steps_per_run))) return rc;
    sgusto_loop *h = new sgusto_loop();
    h->plan = plan; h->planner = planner_model; h->plant = plant;
    h->has_Qzf = has_Qzf != 0;
    h->lds = advance_lds_bytes(n, m, false);
    const char *what = "set up the advance kernel / the stream";
    auto fail = [&](int code) { delete h; return code; };
    if (h->lds > (size_t)160 * 1024) {
        srh::set_error("sgusto_loop_create: the advance kernel needs %zu bytes of LDS (160 KiB available)", h->lds);
        return fail(SRH_EINVAL);
    }
    if (hipFuncSetAttribute((const void *)loop_advance_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess)
        return fail(loop_setup_failed("sgusto_loop_create", what));
    if ((rc = h->setup("sgusto_loop_create", what, N, n, m, nz, B, dt, dt_sim, n_keep, max_steps_per_run, nz)) ||
        (rc = h->zf.alloc(sizeof(double) * B * nz)))
        return fail(rc);
    (void)sgusto_loop_end_row(N, dt, dt_sim, n_keep, &h->j_end, &h->theta_end);
    h->XBrec.shape(sizeof(double) * n, 1); h->UBrec.shape(sizeof(double) * m, 1);
    *out = h;
    return SRH_OK;
}

int sgusto_loop_destroy(sgusto_loop_t *h) {
    delete h;
    return SRH_OK;
}

int sgusto_loop_set_target(sgusto_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase) {
    return loop_set_target(h, "sgusto_loop_set_target", T, t, z, u_des, phase);
}

int sgusto_loop_set_feedback(sgusto_loop_t *h, const double *K) {
    SRH_REQUIRE(h, "sgusto_loop_set_feedback: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->has_K = false;
    if (!K) return SRH_OK;
    int rc = h->K.upload(K, sizeof(double) * h->planner->P * h->m * h->n);
    if (rc) return rc;
    h->has_K = true;
    return SRH_OK;
}

int sgusto_loop_set_chained(sgusto_loop_t *h, int on) {
    SRH_REQUIRE(h, "sgusto_loop_set_chained: null handle");
    SRH_REQUIRE(h->k == 0, "sgusto_loop_set_chained: %lld period(s) have run since the last reset: the policy of a loop changes only in front "
                "of its first period (call sgusto_loop_reset first)", (long long)h->k);
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    int rc;
    if (on && !h->xchain.p && (rc = h->xchain.alloc(sizeof(double) * h->B * h->n))) return rc;
    h->chained = on != 0;
    return SRH_OK;
}

int sgusto_loop_reset(sgusto_loop_t *h, const double *x0, double t_start) {
    SRH_REQUIRE(h && x0, "sgusto_loop_reset: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipMemcpy(h->xcur.p, x0, sizeof(double) * h->B * h->n, hipMemcpyHostToDevice));
    h->t_start = t_start; h->k = 0; h->have_state = true; h->observed_state = false;
    return SRH_OK;
}

// sgusto_loop_run and sgusto_loop_run_observed: Xhat != null is the observed loop (Vn, Y_cl, ekf_status belong to it)
// Xbar / Ubar: the tape of the chained policy (sgusto_loop_run_tape), or null
static int loop_run(sgusto_loop_t *h, int periods, const double *W, const double *Vn, double *X_cl, double *Z_cl, double *U_cl, int32_t *iters,
                    int32_t *status, double *J, double *Xhat, double *Y_cl, int32_t *ekf_status, double *Xbar = nullptr, double *Ubar = nullptr) {
    const bool observed = Xhat != nullptr;
    const size_t B = (size_t)h->B;
    double *xhat = observed ? h->obs->x_dev() : nullptr, *xcur = h->xcur.as<double>(), *xchain = h->xchain.as<double>();
    int rc0;
    if (Xbar && !h->XBrec.d.p && (rc0 = h->alloc_recs({&h->XBrec}))) return rc0;
    if (Ubar && !h->UBrec.d.p && (rc0 = h->alloc_recs({&h->UBrec}))) return rc0;
    h->XBrec.host = Xbar; h->UBrec.host = Ubar;
    h->XBrec.row0 = h->k > 0 ? xchain : nullptr;          // row 0 of a later run: the old plan's end, where the run's first plan starts
    h->Wd.host = (void *)W; h->Vd.host = (void *)Vn; h->Xrec.host = X_cl; h->Zrec.host = Z_cl; h->Urec.host = U_cl; h->Irec.host = iters;
    h->Srec.host = status; h->Jrec.host = J; h->XHrec.host = Xhat; h->Yrec.host = Y_cl; h->Erec.host = ekf_status;
    h->XHrec.row0 = xhat;               // row 0 of the estimate record: the estimates the run starts from
    // with an observer the plan starts from the estimate; row 0 of the records (the prepare kernel's) is the plant's state all the same
    PrepUnit u{observed ? xhat : xcur, observed ? xcur : nullptr, h->planner->H.as<double>(),
               (h->has_z && h->has_Qzf) ? h->zf.as<double>() : nullptr, true};
    // a chained period k >= 1 starts from the chain state; row 0 of the records stays the plant's state
    auto chain_on = [&]() { u.xcur = xchain; u.xplant = xcur; };
    if (h->chained && h->k > 0) chain_on();
    return loop_run_periods(h, "sgusto_loop_run", periods, u, [&](int p, const PrepArgs &a, const LoopRows &r) -> int {
        int rc;
        // scp/standalone.py:32-33: the first guess is the planner's own zero-input rollout from x0
        if (a.first && (rc = stpwl_rollout_dev(h->planner, a.x0, a.u_init, h->N, h->B, a.x_init, nullptr, (void *)h->stream))) return rc;
        if ((rc = sgusto_plan_solve_dev(h->plan, a.x0, a.u_init, a.x_init, h->has_z ? a.z : nullptr, a.zf, h->has_ud ? a.ud : nullptr,
                                        h->xopt.as<double>(), h->uopt.as<double>(), h->zopt.as<double>(), h->Irec.as<int32_t>() + p * B,
                                        h->Srec.as<int32_t>() + p * B, nullptr, (void *)h->stream)) ||
            (rc = sgusto_plan_costs_dev(h->plan, h->Jrec.as<double>() + p * B, (void *)h->stream)))
            return rc;
        if (h->chained) {
            ChainArgs c = h->chain_args();
            c.xopt = a.xopt; c.uopt = a.uopt;
            c.x_next = xchain;
            c.Xbar = Xbar ? h->XBrec.as<double>() : nullptr; c.Ubar = Ubar ? h->UBrec.as<double>() : nullptr;
            c.rows = r.rows_x; c.row0 = r.row0_u; c.x_row0 = a.first;
            if ((rc = h->launch_chain(c))) return rc;
            chain_on();                 // (read by the next period's prepare launch)
        }
        AdvArgs v = h->adv_args();
        v.xopt = a.xopt; v.uopt = a.uopt;
        v.W = W ? h->Wd.as<double>() : nullptr; v.w_step0 = r.w_step0;
        v.x_in = xcur; v.x_out = xcur;
        v.X = X_cl ? h->Xrec.as<double>() : nullptr; v.Z = h->Zrec.as<double>(); v.U = h->Urec.as<double>();
        v.rows_x = r.rows_x; v.row0_x = r.row0_x; v.rows_u = r.rows_u; v.row0_u = r.row0_u;
        if (!observed) return h->launch_advance(v);
        v.Vn = Vn ? h->Vd.as<double>() : nullptr; v.Y = h->Yrec.as<double>();
        return h->launch_observed_chain(v, h->XHrec.as<double>(), r.rows_x, r.row0_x, h->Erec.as<int32_t>() + p * B, nullptr);
    });
}

int sgusto_loop_run(sgusto_loop_t *h, int periods, const double *W, double *X_cl, double *Z_cl, double *U_cl, int32_t *iters,
                    int32_t *status, double *J) {
    SRH_REQUIRE(h && Z_cl && U_cl && iters && status && J, "sgusto_loop_run: null argument");
    SRH_REQUIRE(periods >= 1, "sgusto_loop_run: periods must be positive");
    SRH_REQUIRE(h->have_state, "sgusto_loop_run: no plant state yet (call sgusto_loop_reset first)");
    SRH_REQUIRE(!h->observed_state, "sgusto_loop_run: the loop was reset with estimates (sgusto_loop_reset_observed): continue it with "
                "sgusto_loop_run_observed, or call sgusto_loop_reset");
    return loop_run(h, periods, W, nullptr, X_cl, Z_cl, U_cl, iters, status, J, nullptr, nullptr, nullptr);
}

int sgusto_loop_set_observer(sgusto_loop_t *h, sekf_batch_t *observer) {
    SRH_REQUIRE(h, "sgusto_loop_set_observer: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->obs = nullptr; h->observed_state = false;
    if (!observer) return SRH_OK;
    int rc;
    if ((rc = loop_check_observer("sgusto_loop_set_observer", observer, h->B, h->n, h->m))) return rc;
    h->lds_obs = advance_lds_bytes(h->n, h->m, true);
    SRH_REQUIRE(h->lds_obs <= (size_t)160 * 1024, "sgusto_loop_set_observer: the observed advance kernel needs %zu bytes of LDS (160 KiB available)",
                h->lds_obs);
    SRH_CHECK_HIP(hipFuncSetAttribute((const void *)loop_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_obs));
    loop_shape_observed(h->XHrec, h->Yrec, h->Erec, h->Vd, h->n, observer->ny);
    if ((rc = h->alloc_recs({&h->XHrec, &h->Yrec, &h->Erec}))) return rc;
    h->obs = observer; h->ny = observer->ny;
    return SRH_OK;
}

int sgusto_loop_reset_observed(sgusto_loop_t *h, const double *x0, const double *x_hat0, double t_start) {
    SRH_REQUIRE(h && x0, "sgusto_loop_reset_observed: null argument");
    SRH_REQUIRE(h->obs, "sgusto_loop_reset_observed: no observer attached (sgusto_loop_set_observer)");
    int rc = sgusto_loop_reset(h, x0, t_start);
    if (rc) return rc;
    h->have_state = false;
    SRH_CHECK_HIP(hipMemcpy(h->obs->x_dev(), x_hat0 ? x_hat0 : x0, sizeof(double) * h->B * h->n, hipMemcpyHostToDevice));
    if ((rc = sekf_batch_install_sigma0(h->obs))) return rc;
    h->have_state = true; h->observed_state = true;
    return SRH_OK;
}

int sgusto_loop_run_observed(sgusto_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                             int32_t *iters, int32_t *status, double *J, double *Xhat, double *Y_cl, int32_t *ekf_status) {
    SRH_REQUIRE(h && Z_cl && U_cl && iters && status && J && Xhat && Y_cl && ekf_status, "sgusto_loop_run_observed: null argument");
    SRH_REQUIRE(periods >= 1, "sgusto_loop_run_observed: periods must be positive");
    SRH_REQUIRE(h->obs, "sgusto_loop_run_observed: no observer attached (sgusto_loop_set_observer)");
    SRH_REQUIRE(h->have_state && h->observed_state, "sgusto_loop_run_observed: no plant state and estimate yet (call sgusto_loop_reset_observed first)");
    return loop_run(h, periods, W, V, X_cl, Z_cl, U_cl, iters, status, J, Xhat, Y_cl, ekf_status);
}

int sgusto_loop_run_tape(sgusto_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                         int32_t *iters, int32_t *status, double *J, double *Xhat, double *Y_cl, int32_t *ekf_status, double *Xbar, double *Ubar) {
    SRH_REQUIRE(h && Z_cl && U_cl && iters && status && J, "sgusto_loop_run_tape: null argument");
    SRH_REQUIRE(h->chained || (!Xbar && !Ubar), "sgusto_loop_run_tape: the loop re-plans from the plant (mpc=True): it follows no nominal tape "
                "(sgusto_loop_set_chained)");
    const bool observed = Xhat != nullptr;
    SRH_REQUIRE(observed ? (Y_cl && ekf_status) : (!V && !Y_cl && !ekf_status), "sgusto_loop_run_tape: Xhat, Y_cl and ekf_status come together "
                "(the observed loop), V with them");
    SRH_REQUIRE(periods >= 1, "sgusto_loop_run_tape: periods must be positive");
    if (!observed) {
        SRH_REQUIRE(h->have_state, "sgusto_loop_run_tape: no plant state yet (call sgusto_loop_reset first)");
        SRH_REQUIRE(!h->observed_state, "sgusto_loop_run_tape: the loop was reset with estimates (sgusto_loop_reset_observed): pass Xhat, Y_cl and "
                    "ekf_status, or call sgusto_loop_reset");
    } else {
        SRH_REQUIRE(h->obs, "sgusto_loop_run_tape: no observer attached (sgusto_loop_set_observer)");
        SRH_REQUIRE(h->have_state && h->observed_state, "sgusto_loop_run_tape: no plant state and estimate yet (call sgusto_loop_reset_observed first)");
    }
    return loop_run(h, periods, W, V, X_cl, Z_cl, U_cl, iters, status, J, Xhat, Y_cl, ekf_status, Xbar, Ubar);
}

int sgusto_loop_chain(sgusto_loop_t *h, const double *xopt, const double *uopt, double *x_next, double *Xbar_rows, double *Ubar_rows) {
    SRH_REQUIRE(h && xopt && uopt, "sgusto_loop_chain: null argument");
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m, nk = h->n_keep;
    srh::DevBuf dxo, duo, dx, dX, dU;
    int rc;
    if ((rc = dxo.upload(xopt, D * B * (N + 1) * n)) || (rc = duo.upload(uopt, D * B * N * m)) || (x_next && (rc = dx.alloc(D * B * n))) ||
        (Xbar_rows && (rc = dX.alloc(D * B * (nk + 1) * n))) || (Ubar_rows && (rc = dU.alloc(D * B * (nk + 1) * m))))
        return rc;
    ChainArgs c = h->chain_args();
    c.xopt = dxo.as<double>(); c.uopt = duo.as<double>();
    c.x_next = x_next ? dx.as<double>() : nullptr;
    c.Xbar = Xbar_rows ? dX.as<double>() : nullptr; c.Ubar = Ubar_rows ? dU.as<double>() : nullptr;
    c.rows = (int64_t)nk + 1; c.row0 = 0; c.x_row0 = 1;
    if ((rc = loop_wait(h->launch_chain(c), h->stream))) return rc;
    if (x_next && (rc = dx.download(x_next, D * B * n))) return rc;
    if (Xbar_rows && (rc = dX.download(Xbar_rows, D * B * (nk + 1) * n))) return rc;
    if (Ubar_rows && (rc = dU.download(Ubar_rows, D * B * (nk + 1) * m))) return rc;
    return SRH_OK;
}

int sgusto_loop_last_inputs(sgusto_loop_t *h, double *x0, double *u_init, double *x_init, double *z, double *zf, double *u_des) {
    int rc = loop_last_inputs(h, "sgusto_loop_last_inputs", x0, u_init, x_init, z, u_des);
    if (rc) return rc;
    if (zf && h->has_z && h->has_Qzf && (rc = h->zf.download(zf, sizeof(double) * h->B * h->nz))) return rc;
    return SRH_OK;
}

int sgusto_loop_last_plan(sgusto_loop_t *h, double *xopt, double *uopt) { return loop_last_plan(h, "sgusto_loop_last_plan", xopt, uopt); }

int sgusto_loop_advance(sgusto_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *W, double *X,
                        double *Z, double *U, int32_t *idx_plant, int32_t *idx_gain) {
    SRH_REQUIRE(h && xopt && uopt && x && X && Z && U, "sgusto_loop_advance: null argument");
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m, nz = h->nz, nk = h->n_keep;
    srh::DevBuf dxo, duo, dx, dW, dX, dZ, dU, dp, dg;
    int rc;
    if ((rc = dxo.upload(xopt, D * B * (N + 1) * n)) || (rc = duo.upload(uopt, D * B * N * m)) || (rc = dx.upload(x, D * B * n)) ||
        (W && (rc = dW.upload(W, D * nk * B * n))) || (rc = dX.alloc(D * B * nk * n)) || (rc = dZ.alloc(D * B * nk * nz)) ||
        (rc = dU.alloc(D * B * nk * m)) || (rc = dp.alloc(sizeof(int32_t) * B * nk)) || (rc = dg.alloc(sizeof(int32_t) * B * nk)))
        return rc;
    AdvArgs v = h->adv_args();
    v.xopt = dxo.as<double>(); v.uopt = duo.as<double>();
    v.W = W ? dW.as<double>() : nullptr; v.w_step0 = 0;
    v.x_in = dx.as<double>(); v.x_out = nullptr;
    v.X = dX.as<double>(); v.Z = dZ.as<double>(); v.U = dU.as<double>();
    v.ip = dp.as<int32_t>(); v.ig = dg.as<int32_t>();
    v.rows_x = (int64_t)nk; v.row0_x = 0; v.rows_u = (int64_t)nk; v.row0_u = 0;
    if ((rc = loop_wait(h->launch_advance(v), h->stream))) return rc;
    if ((rc = dX.download(X, D * B * nk * n)) || (rc = dZ.download(Z, D * B * nk * nz)) || (rc = dU.download(U, D * B * nk * m))) return rc;
    if (idx_plant && (rc = dp.download(idx_plant, sizeof(int32_t) * B * nk))) return rc;
    if (idx_gain && (rc = dg.download(idx_gain, sizeof(int32_t) * B * nk))) return rc;
    return SRH_OK;
}

int sgusto_loop_advance_observed(sgusto_loop_t *h, const double *xopt, const double *uopt, const double *x, const double *x_hat, const double *W,
                                 const double *V, double *X, double *Z, double *U, double *Xhat, double *Y, int32_t *idx_plant,
                                 int32_t *idx_gain, int32_t *idx_filter, int32_t *ekf_status) {
    SRH_REQUIRE(h && xopt && uopt && x && x_hat && X && Z && U && Xhat && Y, "sgusto_loop_advance_observed: null argument");
    SRH_REQUIRE(h->obs, "sgusto_loop_advance_observed: no observer attached (sgusto_loop_set_observer)");
    const size_t D = sizeof(double), B = (size_t)h->B, N = h->N, n = h->n, m = h->m, nz = h->nz, nk = h->n_keep, ny = h->ny;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    // the attached filters start from x_hat and Sigma0; the loop's own state is no longer the one the caller knows
    h->have_state = false;
    SRH_CHECK_HIP(hipMemcpy(h->obs->x_dev(), x_hat, D * B * n, hipMemcpyHostToDevice));
    srh::DevBuf dxo, duo, dx, dW, dV, dX, dZ, dU, dXH, dY, dp, dg, df, dE;
    int rc;
    if ((rc = sekf_batch_install_sigma0(h->obs)) || (rc = dxo.upload(xopt, D * B * (N + 1) * n)) || (rc = duo.upload(uopt, D * B * N * m)) ||
        (rc = dx.upload(x, D * B * n)) || (W && (rc = dW.upload(W, D * nk * B * n))) || (V && (rc = dV.upload(V, D * nk * B * ny))) ||
        (rc = dX.alloc(D * B * nk * n)) || (rc = dZ.alloc(D * B * nk * nz)) || (rc = dU.alloc(D * B * nk * m)) || (rc = dXH.alloc(D * B * nk * n)) ||
        (rc = dY.alloc(D * B * nk * ny)) || (rc = dp.alloc(sizeof(int32_t) * B * nk)) || (rc = dg.alloc(sizeof(int32_t) * B * nk)) ||
        (rc = df.alloc(sizeof(int32_t) * B * nk)) || (rc = dE.alloc(sizeof(int32_t) * B)))
        return rc;
    AdvArgs v = h->adv_args();
    v.xopt = dxo.as<double>(); v.uopt = duo.as<double>();
    v.W = W ? dW.as<double>() : nullptr; v.Vn = V ? dV.as<double>() : nullptr; v.w_step0 = 0;
    v.x_in = dx.as<double>(); v.x_out = dx.as<double>();          // the plant state travels from launch to launch
    v.X = dX.as<double>(); v.Z = dZ.as<double>(); v.U = dU.as<double>(); v.Y = dY.as<double>();
    v.ip = dp.as<int32_t>(); v.ig = dg.as<int32_t>();
    v.rows_x = (int64_t)nk; v.row0_x = 0; v.rows_u = (int64_t)nk; v.row0_u = 0;
    if ((rc = loop_wait(h->launch_observed_chain(v, dXH.as<double>(), (int64_t)nk, 0, dE.as<int32_t>(), df.as<int32_t>()), h->stream))) return rc;
    if ((rc = dX.download(X, D * B * nk * n)) || (rc = dZ.download(Z, D * B * nk * nz)) || (rc = dU.download(U, D * B * nk * m)) ||
        (rc = dXH.download(Xhat, D * B * nk * n)) || (rc = dY.download(Y, D * B * nk * ny)))
        return rc;
    if (idx_plant && (rc = dp.download(idx_plant, sizeof(int32_t) * B * nk))) return rc;
    if (idx_gain && (rc = dg.download(idx_gain, sizeof(int32_t) * B * nk))) return rc;
    if (idx_filter && (rc = df.download(idx_filter, sizeof(int32_t) * B * nk))) return rc;
    if (ekf_status && (rc = dE.download(ekf_status, sizeof(int32_t) * B))) return rc;
    return SRH_OK;
}

int sgusto_loop_stats(sgusto_loop_t *h, int64_t *steps, int64_t *waits_last_run) { return loop_stats(h, "sgusto_loop_stats", steps, waits_last_run); }

}  // extern "C"
