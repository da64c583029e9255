// Batched closed loop on a resident SSM GuSTO plan: every rollout of the plan's batch is its own receding-horizon loop of the reference's
// hardware driver -- plan, apply n_keep interpolated inputs to an SSM plant, measure, estimate, shift, re-plan from the estimate -- and a
// whole run of periods is one launch sequence on the handle's stream with one host wait.  Reference: examples/hardware/diamond_SSM.py:
// 353-361 (the loop), scp/ros.py:78-79, 109-114 (first guess, shift), SSM/controllers.py:204, 237 (u = u_bar(t), no gain) and its
// SSMObserver (x_hat = W_map(y - z_ref)), SSM/ssm.py:198-218, 279-301 (plant step).
// The solve is sgusto_ssm_plan_solve_dev (gusto_ssm.hip), the first guess sssm_rollout_dev (ssm.hip), shift and target window the
// prepare kernel shared with gusto_loop.hip (gusto_loop_prep.h), the host shell of a handle and of a run the one shared with it too
// (gusto_loop_host.h).  New here: ssm_loop_advance_kernel.  Because the observer is a map and not a filter, the whole sub-step -- input
// from the plan, plant step, measurement, estimate -- is one kernel for all n_keep sub-steps.
// The plant may also be a nearest-point TPWL model of more states than the planner's, measured by y = C x + y_ref (the reference's
// drivers: the controller sees only the measured tip): ssm_loop_advance_tpwl_kernel puts the point search and the step rule of
// tpwl_dev.h, measure_row and plan_at of gusto_loop_prep.h and the estimate (ssm_loop_estimate, stated once for both kernels) together;
// the handle is the same sgusto_ssm_loop with a plant kind (sgusto_ssm_loop_create_tpwl).
#include "ssm_host.h"
#include "ssm_step_dev.h"
#include "tpwl_host.h"
#include "gusto_loop_host.h"

#include <algorithm>

namespace {

constexpr int SL_NT = 256;

struct SsmAdvArgs {
    int N, n_keep, mode;                // horizon of the plan, sub-steps of this launch (0: none), the plant's discretisation
    int init;                           // 1: measure and estimate at x_in before the sub-steps (reset: row 0 of the records)
    int same;                           // the observer's model is the plant: its ssm basis is staged once
    double dt_sim;
    const double *uopt;                 // the plans' inputs (B x N x m)
    const int32_t *js;                  // (n_keep) plan interval of every sub-step
    const double *theta;                // (n_keep) position inside it
    const double *W, *Vn;               // (steps x B x n), (steps x B x no) or null; this launch reads steps w_step0 ..
    const double *v0;                   // init: (B x no) noise of the first measurement, or null
    const double *x_in;                 // (B x n)
    double *x_out, *z_out, *y_out, *xh_out;     // where the launch ends (B x .), any may be null (x_out may be x_in)
    double *X, *Z, *U, *Y, *Xhat;       // records: row row0 + s of rollout b (any may be null)
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
    ReprojArgs Yp_;                     // the admissible set Y of the measurements and the two records (<true> instantiation only)
    double *yu_out;                     // (B x no) the last used measurement, or null
    int32_t *pj_out;                    // (B) its status word, or null
};

// What the kernel reads of the observer's model (the planner's): the observed -> reduced map and the ssm basis it is written in
struct SsmObsDev {
    int ns, order_s;
    const int *ps, *vs, *lvs;           // parent / variable of every monomial, first index of every degree (ssm::basis)
    cgptr Vc, z_ref;                    // v_coeff (n x ns), z_ref (no)
};

SsmObsDev obs_view(const sssm *h) {
    const SsmDev S = h->view();
    return SsmObsDev{S.ns, S.order_s, S.ps, S.vs, S.lvs, S.Vc, S.z_ref};
}

// LDS of the launch in doubles: [work area | x, x', x_hat, u, zeta, y, y - z_ref, the two z_ref | A, B, d | V of the observer's model |
// the plant's tables (ssm::stage) | the observer's ssm basis when it is another model]
size_t ssm_loop_front_doubles(int n, int m, int no, int nr, int ns_max) {
    return ssm::work_doubles(n, m, no, nr, ns_max) + 3 * (size_t)n + 16 + 5 * (size_t)no + (size_t)n * n + (size_t)n * m + n;
}

// With a Y (the <true> instantiations) the launch's LDS starts with wave 0's projection area, reproject_doubles(no) doubles.
size_t ssm_loop_lds_bytes(const sssm *plant, const sssm *obs, bool proj = false) {
    const int ns_max = std::max(plant->ns, obs->ns);
    size_t d = ssm_loop_front_doubles(plant->n, plant->m, plant->no, plant->nr, ns_max) + (size_t)plant->n * obs->ns +
               ssm::lds_tab_doubles(plant->n, plant->no, plant->nr, plant->ns, 0) + (proj ? reproject_doubles(plant->no) : 0);
    if (obs != plant) d += (size_t)obs->ns + 1;
    return srh::lds_request(sizeof(double) * (d + 2));
}

// THE ESTIMATE, stated once for both advance kernels: x_hat = V phi_s(yd), yd = y - z_ref of the observer's model (no entries, LDS).
// ps / vs: parent and variable of every monomial of its ssm basis, lv: first index of every degree, Vl: its v_coeff (n x ns) in LDS,
// phi: ns doubles of work.  The monomials degree by degree (ssm::basis_l without a derivative table: only parent / variable are read),
// then row o by eight lanes, lane g summing the columns g, g + 8, ... by fma from 0.0, and wg::group_sum<8> -- as ssm::observe_l.
// Writes xh (LDS) and, unless null, the record row XHr.  All nt threads; ends with a sync.
__device__ __forceinline__ void ssm_loop_estimate(liptr ps, liptr vs, const int *lv, int order_s, int ns, int no, int n, clptr yd, lptr phi,
                                                  clptr Vl, lptr xh, gptr XHr, int tid, int nt) {
    ssm::basis_l(ps, ps, vs, ps, lv, order_s, ns, no, yd, phi, (lptr) nullptr);
    const int g8 = tid & 7;
    for (int o0 = 0; o0 < n; o0 += nt / 8) {
        const int o = o0 + (tid >> 3);
        double acc = 0.0;
        if (o < n) for (int k = g8; k < ns; k += 8) acc = fma(Vl[(size_t)o * ns + k], phi[k], acc);
        acc = wg::group_sum<8>(acc);
        if (g8 == 0 && o < n) {
            xh[o] = acc;
            if (XHr != nullptr) XHr[o] = acc;
        }
    }
    __syncthreads();
}

// One workgroup per loop, all n_keep sub-steps of a period.  S: the plant, P: the model of the observer (the planner's).  The plant's
// coefficient rows and the evaluation tables of both its bases are staged once per launch (ssm::stage), V and z_ref of the observer's
// model behind them; x, u, y and x_hat stay in LDS between sub-steps and only the records go to HBM.  Per sub-step: the input from the
// plan; the plant's continuous Jacobians at (x, u) from the staged tables (ssm::jacobians_l) discretised at dt_sim on the elimination
// paths of ssm::discretize; x' = A_d x + B_d u + d_d (+ w) in the sums of ssm_rollout_kernel; then `measure`: zeta = C_plant(x')
// (ssm::observe_l), y = (zeta + z_ref_plant) + v, x_hat = V phi_s(y - z_ref_observer).  With init = 1 `measure` runs once at x_in first:
// a launch of zero sub-steps is the reset's first observer update, so the maps are stated once.
// PROJ (the loop has a Y): between the barrier behind y and the estimate, wave 0 projects y onto Y and the estimate reads y_used - z_ref
// (reproject_measurement of gusto_loop_prep.h, SSM/controllers.py:96-97); the init measurement of a reset passes through it too.  <false>
// (the default) is the kernel as it was: every PROJ part is compiled out.
template <bool PROJ = false>
__global__ __launch_bounds__(SL_NT) void ssm_loop_advance_kernel(SsmDev S, SsmObsDev P, SsmAdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = S.n, m = S.m, no = S.no, N = a.N, tid = threadIdx.x, nt = SL_NT;
    const size_t b = blockIdx.x;
    const bool dm = a.mode == SSM_DISCRETE_MAP;
    SsmDev Sc = S;
    Sc.ns = max(S.ns, P.ns);                               // the work area's monomial vector serves both ssm bases
    lptr base = (lptr)smem + (PROJ ? reproject_doubles(no) : 0);
    ssm::Work w;
    ssm::carve(w, base, Sc);
    lptr xs = base + ssm::work_doubles(n, m, no, S.nr, Sc.ns);
    lptr xn = xs + n, xh = xn + n, us = xh + n;            // n each, u: 16
    lptr zs = us + 16, ys = zs + no, yd = ys + no, zrl = yd + no, zrp = zrl + no;       // no each
    lptr Al = zrp + no, Bl = Al + (size_t)n * n, dl = Bl + (size_t)n * m;
    lptr Vl = dl + n;                                      // n x P.ns
    lptr tab = Vl + (size_t)n * P.ns;
    SsmLds T;
    ssm::stage(T, tab, S, dm, 0);
    liptr pps = T.ps, pvs = T.vs;                          // parent / variable tables of the observer's ssm basis
    int plv[SSM_MAX_ORDER + 1];
    for (int q = 0; q <= SSM_MAX_ORDER; ++q) plv[q] = a.same ? T.lvs[q] : (q <= P.order_s ? P.lvs[q] : 0);
    if (!a.same) {
        pps = (liptr)(tab + ssm::lds_tab_doubles(n, no, S.nr, S.ns, 0));
        pvs = pps + P.ns;
        for (int e = tid; e < P.ns; e += nt) { pps[e] = P.ps[e]; pvs[e] = P.vs[e]; }
    }
    for (int e = tid; e < n * P.ns; e += nt) Vl[e] = P.Vc[e];
    for (int e = tid; e < no; e += nt) { zrl[e] = S.z_ref[e]; zrp[e] = P.z_ref[e]; }
    for (int e = tid; e < n; e += nt) xs[e] = ((cgptr)a.x_in)[b * n + e];
    [[maybe_unused]] ReprojWave yw;
    [[maybe_unused]] lptr yu = nullptr;
    [[maybe_unused]] int pj = 0;
    if constexpr (PROJ) {
        yu = reproject_used((lptr)smem);
        if (tid < 64) reproject_load(a.Yp_, no, tid, yw);
    }
    __syncthreads();

    // zeta, y and x_hat of the state in xs; v (no) or null; rows of the records or null (row: of the two records of Y, < 0: none).
    // Ends with a sync.
    auto measure = [&](cgptr v, gptr Zr, gptr Yr, gptr XHr, [[maybe_unused]] int64_t row) {
        ssm::observe_l(S, T, xs, w, zs);
        for (int e = tid; e < no; e += nt) {
            double y = zs[e] + zrl[e];
            if (v != nullptr) y += v[e];
            ys[e] = y;
            if constexpr (!PROJ) yd[e] = y - zrp[e];
            if (Zr != nullptr) Zr[e] = zs[e];
            if (Yr != nullptr) Yr[e] = y;
        }
        __syncthreads();
        if constexpr (PROJ)
            pj = reproject_measurement(yw, a.Yp_.rows, no, ys, yu, (lptr)smem, zrp, yd, (row >= 0 && a.Yp_.Yu) ? (gptr)a.Yp_.Yu + row * no : (gptr) nullptr,
                                       (row >= 0 && a.Yp_.proj) ? (giptr)a.Yp_.proj + row : (giptr) nullptr, tid, nt);
        ssm_loop_estimate(pps, pvs, plv, P.order_s, P.ns, no, n, yd, w.phi, Vl, xh, XHr, tid, nt);
    };

    if (a.init) measure(a.v0 ? (cgptr)a.v0 + b * no : (cgptr) nullptr, (gptr) nullptr, (gptr) nullptr, (gptr) nullptr, -1);
    cgptr uo = (cgptr)a.uopt + b * (size_t)N * m, Wd = (cgptr)a.W, Vd = (cgptr)a.Vn, thg = (cgptr)a.theta;
    cgiptr jsg = (cgiptr)a.js;
    for (int s = 0; s < a.n_keep; ++s) {
        const int js = jsg[s];
        const double th = thg[s];
        if (tid < m) {                                     // the input is held over the last interval (SSM/controllers.py:204)
            const double v = plan_at(uo, m, js, min(js + 1, N - 1), th, tid);
            us[tid] = v;
            if (a.U) ((gptr)a.U)[(b * (size_t)a.rows_u + a.row0_u + s) * m + tid] = v;
        }
        __syncthreads();
        ssm::jacobians_l(S, T, dm, xs, us, w, Al, n, Bl, dl);
        ssm::discretize(S, a.mode, a.dt_sim, w, Al, n, Bl, dl);
        for (int i = tid; i < n; i += nt) {
            double v = ssm_step_affine_row(Al, Bl, dl, xs, us, n, m, i);               // (ssm_step_dev.h: the SSM horizon error calls it too)
            if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * n + i];
            xn[i] = v;
        }
        __syncthreads();
        const size_t row = b * (size_t)a.rows_x + a.row0_x + s;
        for (int e = tid; e < n; e += nt) {
            xs[e] = xn[e];
            if (a.X) ((gptr)a.X)[row * n + e] = xn[e];
        }
        __syncthreads();
        measure(Vd != nullptr ? Vd + ((size_t)(a.w_step0 + s) * a.B + b) * no : (cgptr) nullptr, a.Z ? (gptr)a.Z + row * no : (gptr) nullptr,
                a.Y ? (gptr)a.Y + row * no : (gptr) nullptr, a.Xhat ? (gptr)a.Xhat + row * n : (gptr) nullptr, (int64_t)row);
    }
    for (int e = tid; e < n; e += nt) {
        if (a.x_out) ((gptr)a.x_out)[b * n + e] = xs[e];
        if (a.xh_out) ((gptr)a.xh_out)[b * n + e] = xh[e];
    }
    for (int e = tid; e < no; e += nt) {
        if (a.z_out) ((gptr)a.z_out)[b * no + e] = zs[e];
        if (a.y_out) ((gptr)a.y_out)[b * no + e] = ys[e];
    }
    if constexpr (PROJ) {
        if (a.yu_out)
            for (int e = tid; e < no; e += nt) ((gptr)a.yu_out)[b * no + e] = yu[e];
        if (a.pj_out && tid == 0) ((giptr)a.pj_out)[b] = pj;
    }
}

// what both the loop and the stand-alone entry ask of the two models; `who` names the caller in the message
int ssm_loop_check_models(const char *who, const sssm *plant, int plant_mode, const sssm *obs, size_t *lds) {
    SRH_REQUIRE(plant_mode >= SSM_FE && plant_mode <= SSM_DISCRETE_MAP, "%s: plant_mode %d is not one of fe (1), be (2), bil (3), discrete map (4)", who,
                plant_mode);
    SRH_REQUIRE(plant_mode != SSM_DISCRETE_MAP || plant->has_discrete, "%s: the plant has no discrete map (rd_coeff, Bd) for plant_mode = 4", who);
    SRH_REQUIRE(plant->n == obs->n && plant->m == obs->m && plant->no == obs->no,
                "%s: the plant has n_x = %d, n_u = %d, n_o = %d, the planner's model n_x = %d, n_u = %d, n_o = %d", who, plant->n, plant->m, plant->no,
                obs->n, obs->m, obs->no);
    SRH_REQUIRE(plant->n == plant->no, "%s: the reduced -> observed map needs n_x == n_o (n_x = %d, n_o = %d)", who, plant->n, plant->no);
    SRH_REQUIRE(plant->m <= 16, "%s: n_u = %d exceeds the limit n_u <= 16 of the staged input matrix", who, plant->m);
    *lds = ssm_loop_lds_bytes(plant, obs);
    SRH_REQUIRE(*lds <= (size_t)160 * 1024, "%s: the advance kernel needs %zu bytes of LDS for the plant's tables, the observer's V and the work area "
                "(160 KiB = 163840 available)", who, *lds);
    return SRH_OK;
}

// (lds: of the instantiation the arguments choose -- with a Y, ssm_loop_lds_bytes(.., true))
int ssm_loop_launch(const sssm *plant, const sssm *obs, size_t lds, const SsmAdvArgs &a, hipStream_t st) {
    if (a.Yp_.rows) {
        SRH_CHECK_HIP(hipFuncSetAttribute((const void *)ssm_loop_advance_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ssm_loop_advance_kernel<true><<<(unsigned)a.B, SL_NT, lds, st>>>(plant->view(), obs_view(obs), a);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    SRH_CHECK_HIP(hipFuncSetAttribute((const void *)ssm_loop_advance_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ssm_loop_advance_kernel<<<(unsigned)a.B, SL_NT, lds, st>>>(plant->view(), obs_view(obs), a);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

// ---- the same loop on a nearest-point TPWL plant of np states, measured by y = C x + y_ref (the reference's drivers: the controller
// sees only the measured tip) ----
struct SsmTpwlAdvArgs {
    int N, n_keep, np, m, n, no;        // horizon of the plan, sub-steps of this launch (0: none), plant states, inputs, the observer model's n_x, n_o
    int init;                           // 1: measure and estimate at x_in before the sub-steps (reset: row 0 of the records)
    const double *uopt;                 // the plans' inputs (B x N x m)
    const int32_t *js;                  // (n_keep) plan interval of every sub-step
    const double *theta;                // (n_keep) position inside it
    const double *C, *yref;             // (no x np), (no): the plant's measurement
    const double *W, *Vn;               // (steps x B x np), (steps x B x no) or null; this launch reads steps w_step0 ..
    const double *v0;                   // init: (B x no) noise of the first measurement, or null
    const double *x_in;                 // (B x np)
    double *x_out, *z_out, *y_out, *xh_out;     // where the launch ends (B x .), any may be null (x_out may be x_in)
    double *X, *Z, *U, *Y, *Xhat;       // records: row row0 + s of rollout b (any may be null)
    int32_t *idx;                       // (B x n_keep) the plant's point of every sub-step, or null
    int64_t rows_x, row0_x, rows_u, row0_u, B, w_step0;
    ReprojArgs Yp_;                     // the admissible set Y of the measurements and the two records (<true> instantiation only)
    double *yu_out;                     // (B x no) the last used measurement, or null
    int32_t *pj_out;                    // (B) its status word, or null
};

// LDS of the launch in doubles, every block padded to even so that the panel is 16-byte aligned: x (np) | u (16) | zeta, y, y - z_ref,
// y_ref, the observer's z_ref (no each) | x_hat (n) | phi (ns) | C (no x np) | V of the observer's model (n x ns) | parent and variable
// tables of its ssm basis (2 ns ints) | the staged step of tpwl_dev.h: partial sums of A x, B u (256 each), the point (2), the plant's
// panel A^T, B^T, d (np is even: x = [v; q]).
__host__ __device__ inline int sl_even(int v) { return (v + 1) & ~1; }
size_t ssm_loop_tpwl_lds_bytes(int np, int m, int n, int no, int ns, bool proj = false) {
    const size_t d = (size_t)sl_even(np) + 16 + 5 * (size_t)sl_even(no) + (size_t)sl_even(n) + 2 * (size_t)sl_even(ns) + (size_t)sl_even(no * np) +
                     (size_t)sl_even(n * ns) + tpwl::step_doubles(np, m, SL_NT) + 2 + (proj ? reproject_doubles(no) : 0);
    return srh::lds_request(sizeof(double) * d);
}

// One workgroup of 256 threads per loop, all n_keep sub-steps of a period.  TL: the plant, P: the model of the observer (the planner's).
// C, y_ref, the observer's z_ref, V and basis tables are staged once per launch; the plant's region panel [A_d^T | B_d^T | d_d] sits in
// LDS and is reloaded only when the plant's nearest point changes (as koop_loop_advance_kernel); x, u, y and x_hat stay in LDS between
// sub-steps and only the records go to HBM.  Fixed summation orders per sub-step:
//   u_e    = plan_at(uopt, m, j, min(j + 1, N - 1), theta, e)                        no gain (SSM/controllers.py:204, 237)
//   i      = THE POINT-SEARCH RULE of tpwl_dev.h at x (tpwl::nearest_wave on the wave without input rows; not a number: point 0)
//   x'     = THE STEP RULE of tpwl_dev.h (+ w)
//   zeta_e = out_row(C, e, np, x'), y_e = measure_row: (zeta_e + y_ref[e]) + v_e     (gusto_loop_prep.h); the record Z is zeta
//   x_hat  = THE ESTIMATE (ssm_loop_estimate) of y - z_ref_observer
// With init = 1 the measurement and the estimate run once at x_in first: a launch of zero sub-steps is the reset's first observer update.
// PROJ: as ssm_loop_advance_kernel -- y is projected onto Y between its barrier and the estimate, which then reads y_used - z_ref.
template <bool PROJ = false>
__global__ __launch_bounds__(SL_NT) void ssm_loop_advance_tpwl_kernel(TpwlDev TL, SsmObsDev P, SsmTpwlAdvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int np = a.np, m = a.m, n = a.n, no = a.no, ns = P.ns, N = a.N, nt = SL_NT;
    lptr xc = (lptr)smem + (PROJ ? reproject_doubles(no) : 0);      // np     plant state
    lptr uc = xc + sl_even(np);                          // 16     input of the sub-step
    lptr zs = uc + 16;                                   // no     zeta = C x
    lptr ys = zs + sl_even(no);                          // no     measurement
    lptr yd = ys + sl_even(no);                          // no     y - z_ref of the observer's model
    lptr yr = yd + sl_even(no);                          // no     y_ref
    lptr zrp = yr + sl_even(no);                         // no     z_ref of the observer's model
    lptr xh = zrp + sl_even(no);                         // n      estimate
    lptr phi = xh + sl_even(n);                          // ns     monomials of the observer's ssm basis
    lptr Cl = phi + sl_even(ns);                         // no x np
    lptr Vl = Cl + sl_even(no * np);                     // n x ns
    liptr pps = (liptr)(Vl + sl_even(n * ns)), pvs = pps + ns;            // ns ints each (sl_even(ns) doubles)
    tpwl::StepLds L;                                     //        partial sums of A x, B u | ip | the panel of region `cur`
    tpwl::step_carve(L, Vl + sl_even(n * ns) + sl_even(ns), np, m, SL_NT, 2);
    liptr ip = (liptr)(L.pb + SL_NT);                    // (two doubles) plant point
    const size_t b = blockIdx.x;
    const int tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int npd = max(np, 1), S = max(1, SL_NT / npd), jc = tid % npd, sl = tid / npd;
    int plv[SSM_MAX_ORDER + 1];
    for (int q = 0; q <= SSM_MAX_ORDER; ++q) plv[q] = q <= P.order_s ? P.lvs[q] : 0;
    for (int e = tid; e < ns; e += nt) { pps[e] = P.ps[e]; pvs[e] = P.vs[e]; }
    for (int e = tid; e < n * ns; e += nt) Vl[e] = P.Vc[e];
    for (int e = tid; e < no * np; e += nt) Cl[e] = ((cgptr)a.C)[e];
    for (int e = tid; e < no; e += nt) { yr[e] = ((cgptr)a.yref)[e]; zrp[e] = P.z_ref[e]; }
    for (int e = tid; e < np; e += nt) xc[e] = ((cgptr)a.x_in)[b * np + e];
    [[maybe_unused]] ReprojWave yw;
    [[maybe_unused]] lptr yu = nullptr;
    [[maybe_unused]] int pj = 0;
    if constexpr (PROJ) {
        yu = reproject_used((lptr)smem);
        if (wave == 0) reproject_load(a.Yp_, no, lane, yw);
    }
    __syncthreads();

    // zeta, y and x_hat of the state in xc; noise: the block the row iv0 .. iv0 + no - 1 is read from, or null; rows of the records or
    // null (row: of the two records of Y, < 0: none).  Ends with a sync.
    auto measure = [&](cgptr noise, size_t iv0, gptr Zr, gptr Yr, gptr XHr, [[maybe_unused]] int64_t row) {
        for (int e = tid; e < no; e += nt) {
            const double zeta = out_row(Cl, e, np, xc);
            const double y = measure_row(Cl, e, np, xc, yr, noise, iv0 + e);
            zs[e] = zeta;
            ys[e] = y;
            if constexpr (!PROJ) yd[e] = y - zrp[e];
            if (Zr != nullptr) Zr[e] = zeta;
            if (Yr != nullptr) Yr[e] = y;
        }
        __syncthreads();
        if constexpr (PROJ)
            pj = reproject_measurement(yw, a.Yp_.rows, no, ys, yu, (lptr)smem, zrp, yd, (row >= 0 && a.Yp_.Yu) ? (gptr)a.Yp_.Yu + row * no : (gptr) nullptr,
                                       (row >= 0 && a.Yp_.proj) ? (giptr)a.Yp_.proj + row : (giptr) nullptr, tid, nt);
        ssm_loop_estimate(pps, pvs, plv, P.order_s, ns, no, n, yd, phi, Vl, xh, XHr, tid, nt);
    };

    if (a.init) measure((cgptr)a.v0, b * no, (gptr) nullptr, (gptr) nullptr, (gptr) nullptr, -1);
    cgptr uo = (cgptr)a.uopt + b * (size_t)N * m, Wd = (cgptr)a.W, Vd = (cgptr)a.Vn, thg = (cgptr)a.theta;
    cgiptr jsg = (cgiptr)a.js;
    int cur = -1;
    for (int s = 0; s < a.n_keep; ++s) {
        const int js = jsg[s];
        const double th = thg[s];
        if (tid < m) {                                   // 1. the input is held over the last interval (SSM/controllers.py:204)
            const double v = plan_at(uo, m, js, min(js + 1, N - 1), th, tid);
            uc[tid] = v;
            if (a.U) ((gptr)a.U)[(b * (size_t)a.rows_u + a.row0_u + s) * m + tid] = v;
        }
        if (wave == 3) {                                 // 2. (the wave without input rows)
            const int i = tpwl::nearest_wave(TL, xc);
            if (lane == 0) {
                const int p = (unsigned)i < (unsigned)TL.P ? i : 0;               // (a state that is not a number: no minimum)
                ip[0] = p;
                if (a.idx) ((giptr)a.idx)[b * (size_t)a.n_keep + s] = p;
            }
        }
        __syncthreads();
        tpwl::panel_load(L, TL, ip[0], cur, np, m, tid, SL_NT);                   // (the same for every thread; the barrier below covers the copies)
        __syncthreads();
        tpwl::step_slices(L, xc, uc, np, m, S, jc, sl);                           // 3. the slices of both products
        __syncthreads();
        const size_t row = b * (size_t)a.rows_x + a.row0_x + s;
        if (tid < np) {
            double v = tpwl::step_sum(L, np, S, tid);
            if (Wd != nullptr) v += Wd[((size_t)(a.w_step0 + s) * a.B + b) * np + tid];
            xc[tid] = v;
            if (a.X) ((gptr)a.X)[row * np + tid] = v;
        }
        __syncthreads();
        measure(Vd, ((size_t)(a.w_step0 + s) * a.B + b) * no, a.Z ? (gptr)a.Z + row * no : (gptr) nullptr,       // 4., 5.
                a.Y ? (gptr)a.Y + row * no : (gptr) nullptr, a.Xhat ? (gptr)a.Xhat + row * n : (gptr) nullptr, (int64_t)row);
    }
    for (int e = tid; e < np; e += nt)
        if (a.x_out) ((gptr)a.x_out)[b * np + e] = xc[e];
    for (int e = tid; e < n; e += nt)
        if (a.xh_out) ((gptr)a.xh_out)[b * n + e] = xh[e];
    for (int e = tid; e < no; e += nt) {
        if (a.z_out) ((gptr)a.z_out)[b * no + e] = zs[e];
        if (a.y_out) ((gptr)a.y_out)[b * no + e] = ys[e];
    }
    if constexpr (PROJ) {
        if (a.yu_out)
            for (int e = tid; e < no; e += nt) ((gptr)a.yu_out)[b * no + e] = yu[e];
        if (a.pj_out && tid == 0) ((giptr)a.pj_out)[b] = pj;
    }
}

// what the loop on a TPWL plant and the stand-alone entry ask of the plant, its measurement and the observer's model; `who` names the caller
int ssm_loop_check_tpwl(const char *who, const stpwl *plant, int n_o, const sssm *obs, size_t *lds) {
    SRH_REQUIRE(plant->n <= 128, "%s: the plant's n_x = %d exceeds the limit n_x <= 128 of the advance kernel", who, plant->n);
    SRH_REQUIRE(obs->m <= 16, "%s: n_u = %d exceeds the limit n_u <= 16 of the advance kernel", who, obs->m);
    SRH_REQUIRE(plant->m == obs->m, "%s: the plant has n_u = %d, the planner's model n_u = %d", who, plant->m, obs->m);
    SRH_REQUIRE(n_o == obs->no, "%s: C has n_o = %d rows, the planner's model measures n_o = %d outputs", who, n_o, obs->no);
    SRH_REQUIRE(plant->has_discrete, "%s: the plant has not been pre-discretised at dt_sim", who);
    *lds = ssm_loop_tpwl_lds_bytes(plant->n, plant->m, obs->n, obs->no, obs->ns);
    SRH_REQUIRE(*lds <= (size_t)160 * 1024, "%s: the advance kernel needs %zu bytes of LDS for the plant's panel (n_x = %d), C and the observer's V "
                "(%d x %d) (160 KiB = 163840 available)", who, *lds, plant->n, obs->n, obs->ns);
    return SRH_OK;
}

int ssm_loop_launch_tpwl(const stpwl *plant, const sssm *obs, size_t lds, const SsmTpwlAdvArgs &a, hipStream_t st) {
    if (a.Yp_.rows) {
        SRH_CHECK_HIP(hipFuncSetAttribute((const void *)ssm_loop_advance_tpwl_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ssm_loop_advance_tpwl_kernel<true><<<(unsigned)a.B, SL_NT, lds, st>>>(plant->view(), obs_view(obs), a);
        SRH_CHECK_HIP(hipGetLastError());
        return SRH_OK;
    }
    SRH_CHECK_HIP(hipFuncSetAttribute((const void *)ssm_loop_advance_tpwl_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ssm_loop_advance_tpwl_kernel<<<(unsigned)a.B, SL_NT, lds, st>>>(plant->view(), obs_view(obs), a);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

}  // namespace

struct sgusto_ssm_loop : LoopCore {
    sgusto_ssm_plan_t *plan = nullptr;
    sssm *planner = nullptr, *plant = nullptr;
    stpwl *tplant = nullptr;            // the plant kind: a nearest-point TPWL model (then plant is null), measured by cst = C | y_ref
    int no = 0, np = 0, plan_mode = 0, plant_mode = 0;
    bool observe = true;
    srh::DevBuf zcur, ycur, xhcur, v0;  // where the loops stand beside the plant state xcur: its output, the last measurement, the estimate
    srh::DevBuf cst, xp;                // TPWL plant: C (no x np) | y_ref (no); the plant states (B x np) -- xcur has the planner's width
    // the re-projection onto Y (sgusto_ssm_loop_set_reproject): Y on the device (A | b), the LDS of the <true> instantiation, where the
    // used measurement and its status word stand (row 0 of the next run's records), the two records
    int yrows = 0;
    size_t lds_proj = 0;
    srh::DevBuf Yd, yucur, pjcur;
    LoopRec YUrec, PJrec;
    __attribute__((always_inline)) sgusto_ssm_loop() {         // (inlined: no constructor among the library's dynamic symbols)
        recs.push_back(&YUrec); recs.push_back(&PJrec);
    }
    size_t lds_now() const { return yrows ? lds_proj : lds; }
    template <class Args> void reproject_args(Args &a) const {
        if (!yrows) return;
        a.Yp_.A = Yd.as<double>(); a.Yp_.b = a.Yp_.A + (size_t)yrows * no; a.Yp_.rows = yrows;
        a.yu_out = yucur.as<double>(); a.pj_out = pjcur.as<int32_t>();
    }
    ~sgusto_ssm_loop() { drain(); }
    SsmTpwlAdvArgs adv_args_tpwl() const {
        SsmTpwlAdvArgs a{};
        a.N = N; a.n_keep = n_keep; a.np = np; a.m = m; a.n = n; a.no = no;
        a.js = js.as<int32_t>(); a.theta = theta.as<double>();
        a.C = cst.as<double>(); a.yref = a.C + (size_t)no * np;
        a.B = B;
        reproject_args(a);
        return a;
    }
    SsmAdvArgs adv_args() const {
        SsmAdvArgs a{};
        a.N = N; a.n_keep = n_keep; a.mode = plant_mode; a.same = planner == plant ? 1 : 0;
        a.dt_sim = dt_sim;
        a.js = js.as<int32_t>(); a.theta = theta.as<double>();
        a.B = B;
        reproject_args(a);
        return a;
    }
};

extern "C" {

int sgusto_ssm_loop_create(sgusto_ssm_loop_t **out, sgusto_ssm_plan_t *plan, sssm_t *planner_model, sssm_t *plant, int plant_mode, double dt_sim,
                           int n_keep, int observe, int64_t max_steps_per_run) {
    SRH_REQUIRE(out && plan && planner_model && plant, "sgusto_ssm_loop_create: null argument");
    int N, n, m, nz, mode, ndU;
    int64_t B;
    double dt;
    int rc = sgusto_ssm_plan_dims(plan, &N, &n, &m, &nz, &B, &dt, &mode, &ndU);
    if (rc) return rc;
    SRH_REQUIRE(ndU == 0, "sgusto_ssm_loop_create: the plan has %d input-rate rows (dU): a rollout whose trust region binds under them returns status -78 "
                "for the host loop, which a loop resident on the device cannot serve", ndU);
    SRH_REQUIRE(planner_model->n == n && planner_model->m == m, "sgusto_ssm_loop_create: the planner's model (n_x = %d, n_u = %d) is not the model of the "
                "plan (n_x = %d, n_u = %d)", planner_model->n, planner_model->m, n, m);
    size_t lds = 0;
    if ((rc = ssm_loop_check_models("sgusto_ssm_loop_create", plant, plant_mode, planner_model, &lds)) ||
        (rc = loop_check_periods("sgusto_ssm_loop_create", N, dt, dt_sim, n_keep, max_steps_per_run)))
        return rc;
    sgusto_ssm_loop *h = new sgusto_ssm_loop();
    h->plan = plan; h->planner = planner_model; h->plant = plant;
    h->no = plant->no; h->plan_mode = mode; h->plant_mode = plant_mode; h->observe = observe != 0; h->lds = lds;
    const size_t D = sizeof(double), Bz = (size_t)B, no = (size_t)plant->no;
    // the output, the measurement and the estimate are recorded in every run, row 0 included: S + 1 rows, row 0 where the loops stand
    h->XHrec.shape(D * n, 1); h->Yrec.shape(D * no, 1); h->Vd.shape(D * no, 0);
    if ((rc = h->setup("sgusto_ssm_loop_create", "create the stream", N, n, m, nz, B, dt, dt_sim, n_keep, max_steps_per_run, no)) ||
        (rc = h->alloc_recs({&h->Yrec, &h->XHrec})) || (rc = h->zcur.alloc(D * Bz * no)) || (rc = h->ycur.alloc(D * Bz * no)) ||
        (rc = h->xhcur.alloc(D * Bz * n)) || (rc = h->v0.alloc(D * Bz * no))) {
        delete h;
        return rc;
    }
    h->Xrec.row0 = h->xcur.p; h->Zrec.row0 = h->zcur.p; h->Yrec.row0 = h->ycur.p; h->XHrec.row0 = h->xhcur.p;
    *out = h;
    return SRH_OK;
}

int sgusto_ssm_loop_create_tpwl(sgusto_ssm_loop_t **out, sgusto_ssm_plan_t *plan, sssm_t *planner_model, stpwl_t *plant, const double *Cm,
                                const double *y_ref, int n_o, double dt_sim, int n_keep, int64_t max_steps_per_run) {
    SRH_REQUIRE(out && plan && planner_model && plant && Cm && y_ref, "sgusto_ssm_loop_create_tpwl: null argument");
    *out = nullptr;
    int N, n, m, nz, mode, ndU;
    int64_t B;
    double dt;
    int rc = sgusto_ssm_plan_dims(plan, &N, &n, &m, &nz, &B, &dt, &mode, &ndU);
    if (rc) return rc;
    SRH_REQUIRE(ndU == 0, "sgusto_ssm_loop_create_tpwl: the plan has %d input-rate rows (dU): a rollout whose trust region binds under them returns "
                "status -78 for the host loop, which a loop resident on the device cannot serve", ndU);
    SRH_REQUIRE(planner_model->n == n && planner_model->m == m, "sgusto_ssm_loop_create_tpwl: the planner's model (n_x = %d, n_u = %d) is not the model "
                "of the plan (n_x = %d, n_u = %d)", planner_model->n, planner_model->m, n, m);
    size_t lds = 0;
    if ((rc = ssm_loop_check_tpwl("sgusto_ssm_loop_create_tpwl", plant, n_o, planner_model, &lds)) ||
        (rc = loop_check_periods("sgusto_ssm_loop_create_tpwl", N, dt, dt_sim, n_keep, max_steps_per_run)))
        return rc;
    sgusto_ssm_loop *h = new sgusto_ssm_loop();
    h->plan = plan; h->planner = planner_model; h->tplant = plant;
    h->no = n_o; h->np = plant->n; h->plan_mode = mode; h->observe = true; h->lds = lds;
    const size_t D = sizeof(double), Bz = (size_t)B, no = (size_t)n_o, np = (size_t)plant->n;
    std::vector<double> c(Cm, Cm + no * np);             // C | y_ref
    c.insert(c.end(), y_ref, y_ref + no);
    h->XHrec.shape(D * n, 1); h->Yrec.shape(D * no, 1); h->Vd.shape(D * no, 0);
    if ((rc = h->setup("sgusto_ssm_loop_create_tpwl", "create the stream", N, n, m, nz, B, dt, dt_sim, n_keep, max_steps_per_run, no))) {
        delete h;
        return rc;
    }
    // the plant's records and disturbances have the plant's width, not the plan's (both blocks are allocated by the first run that asks)
    h->Xrec.shape(D * np, 1); h->Wd.shape(D * np, 0);
    if ((rc = h->alloc_recs({&h->Yrec, &h->XHrec})) || (rc = h->zcur.alloc(D * Bz * no)) || (rc = h->ycur.alloc(D * Bz * no)) ||
        (rc = h->xhcur.alloc(D * Bz * n)) || (rc = h->v0.alloc(D * Bz * no)) || (rc = h->xp.alloc(D * Bz * np)) ||
        (rc = h->cst.upload(c.data(), D * c.size()))) {
        delete h;
        return rc;
    }
    h->Xrec.row0 = h->xp.p; h->Zrec.row0 = h->zcur.p; h->Yrec.row0 = h->ycur.p; h->XHrec.row0 = h->xhcur.p;
    *out = h;
    return SRH_OK;
}

int sgusto_ssm_loop_destroy(sgusto_ssm_loop_t *h) {
    delete h;
    return SRH_OK;
}

int sgusto_ssm_loop_set_target(sgusto_ssm_loop_t *h, int T, const double *t, const double *z, const double *u_des, const double *phase) {
    return loop_set_target(h, "sgusto_ssm_loop_set_target", T, t, z, u_des, phase);
}

int sgusto_ssm_loop_reset(sgusto_ssm_loop_t *h, const double *x0, const double *v0, double t_start) {
    SRH_REQUIRE(h && x0, "sgusto_ssm_loop_reset: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->have_state = false;
    const size_t D = sizeof(double), B = (size_t)h->B;
    if (v0) SRH_CHECK_HIP(hipMemcpy(h->v0.p, v0, D * B * h->no, hipMemcpyHostToDevice));
    // the first observer update: the advance kernel with zero sub-steps
    if (h->tplant) {
        SRH_CHECK_HIP(hipMemcpy(h->xp.p, x0, D * B * h->np, hipMemcpyHostToDevice));
        SsmTpwlAdvArgs a = h->adv_args_tpwl();
        a.n_keep = 0; a.init = 1;
        a.v0 = v0 ? h->v0.as<double>() : nullptr;
        a.x_in = h->xp.as<double>();
        a.z_out = h->zcur.as<double>(); a.y_out = h->ycur.as<double>(); a.xh_out = h->xhcur.as<double>();
        const int rc = loop_wait(ssm_loop_launch_tpwl(h->tplant, h->planner, h->lds_now(), a, h->stream), h->stream);
        if (rc) return rc;
        h->t_start = t_start; h->k = 0; h->have_state = true;
        return SRH_OK;
    }
    SRH_CHECK_HIP(hipMemcpy(h->xcur.p, x0, D * B * h->n, hipMemcpyHostToDevice));
    SsmAdvArgs a = h->adv_args();
    a.n_keep = 0; a.init = 1;
    a.v0 = v0 ? h->v0.as<double>() : nullptr;
    a.x_in = h->xcur.as<double>();
    a.z_out = h->zcur.as<double>(); a.y_out = h->ycur.as<double>(); a.xh_out = h->xhcur.as<double>();
    const int rc = loop_wait(ssm_loop_launch(h->plant, h->planner, h->lds_now(), a, h->stream), h->stream);
    if (rc) return rc;
    h->t_start = t_start; h->k = 0; h->have_state = true;
    return SRH_OK;
}

}  // extern "C"

namespace {

// a run, with the two records of the re-projection when the loop has a Y (Y_used, proj: null without one)
int ssm_loop_run(sgusto_ssm_loop *h, const char *who, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                 double *Y_cl, double *Xhat, int32_t *iters, int32_t *status, double *J, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(h && Z_cl && U_cl && Y_cl && Xhat && iters && status && J, "%s: null argument", who);
    SRH_REQUIRE(periods >= 1, "%s: periods must be positive", who);
    SRH_REQUIRE(h->have_state, "%s: no plant state yet (call sgusto_ssm_loop_reset first)", who);
    const size_t B = (size_t)h->B;
    h->YUrec.host = Y_used; h->PJrec.host = proj;
    h->Wd.host = (void *)W; h->Vd.host = (void *)V; h->Xrec.host = X_cl; h->Zrec.host = Z_cl; h->Urec.host = U_cl; h->Yrec.host = Y_cl;
    h->XHrec.host = Xhat; h->Irec.host = iters; h->Srec.host = status; h->Jrec.host = J;
    // the plan starts from the estimate (the reference's loop) or from the plant state (perfect state feedback); no H, no zf, and row 0 of
    // the records is where the loops stand (LoopRec::row0, set at create): the advance kernel writes the records
    // (a TPWL plant's state is not the planner's: its plans always start from the estimate)
    const PrepUnit u{(h->observe || h->tplant) ? h->xhcur.as<double>() : h->xcur.as<double>(), nullptr, nullptr, nullptr, false};
    return loop_run_periods(h, who, periods, u, [&](int p, const PrepArgs &a, const LoopRows &r) -> int {
        int rc;
        // scp/ros.py:78-79: the first guess is the planner's own zero-input rollout from x0
        if (a.first && (rc = sssm_rollout_dev(h->planner, a.x0, a.u_init, h->N, h->B, h->plan_mode, h->dt, a.x_init, nullptr, (void *)h->stream)))
            return rc;
        if ((rc = sgusto_ssm_plan_solve_dev(h->plan, a.x0, a.u_init, a.x_init, h->has_z ? a.z : nullptr, h->has_ud ? a.ud : nullptr,
                                            h->xopt.as<double>(), h->uopt.as<double>(), h->zopt.as<double>(), h->Irec.as<int32_t>() + p * B,
                                            h->Srec.as<int32_t>() + p * B, nullptr, (void *)h->stream)) ||
            (rc = sgusto_ssm_plan_costs_dev(h->plan, h->Jrec.as<double>() + p * B, (void *)h->stream)))
            return rc;
        if (h->tplant) {
            SsmTpwlAdvArgs v = h->adv_args_tpwl();
            v.uopt = a.uopt;
            v.W = W ? h->Wd.as<double>() : nullptr; v.Vn = V ? h->Vd.as<double>() : nullptr; v.w_step0 = r.w_step0;
            v.x_in = h->xp.as<double>();
            v.x_out = h->xp.as<double>(); v.z_out = h->zcur.as<double>(); v.y_out = h->ycur.as<double>(); v.xh_out = h->xhcur.as<double>();
            v.X = X_cl ? h->Xrec.as<double>() : nullptr; v.Z = h->Zrec.as<double>(); v.U = h->Urec.as<double>();
            v.Y = h->Yrec.as<double>(); v.Xhat = h->XHrec.as<double>();
            v.rows_x = r.rows_x; v.row0_x = r.row0_x; v.rows_u = r.rows_u; v.row0_u = r.row0_u;
            v.Yp_.Yu = Y_used ? h->YUrec.as<double>() : nullptr; v.Yp_.proj = proj ? h->PJrec.as<int32_t>() : nullptr;
            return ssm_loop_launch_tpwl(h->tplant, h->planner, h->lds_now(), v, h->stream);
        }
        SsmAdvArgs v = h->adv_args();
        v.uopt = a.uopt;
        v.W = W ? h->Wd.as<double>() : nullptr; v.Vn = V ? h->Vd.as<double>() : nullptr; v.w_step0 = r.w_step0;
        v.x_in = h->xcur.as<double>();
        v.x_out = h->xcur.as<double>(); v.z_out = h->zcur.as<double>(); v.y_out = h->ycur.as<double>(); v.xh_out = h->xhcur.as<double>();
        v.X = X_cl ? h->Xrec.as<double>() : nullptr; v.Z = h->Zrec.as<double>(); v.U = h->Urec.as<double>();
        v.Y = h->Yrec.as<double>(); v.Xhat = h->XHrec.as<double>();
        v.rows_x = r.rows_x; v.row0_x = r.row0_x; v.rows_u = r.rows_u; v.row0_u = r.row0_u;
        v.Yp_.Yu = Y_used ? h->YUrec.as<double>() : nullptr; v.Yp_.proj = proj ? h->PJrec.as<int32_t>() : nullptr;
        return ssm_loop_launch(h->plant, h->planner, h->lds_now(), v, h->stream);
    });
}

// Y of a stand-alone advance entry on the device (A | b), checked as set_reproject checks it
int ssm_loop_stage_Y(const char *who, const double *A, const double *b, int rows, int no, srh::DevBuf &d, ReprojArgs &r) {
    SRH_REQUIRE(A && b, "%s: null argument", who);
    SRH_REQUIRE(no <= poly::PN && rows > 0 && rows <= poly::PM, "%s: Y needs n_o <= 16 and 0 < rows <= 64 (got n_o = %d, rows = %d)", who, no, rows);
    for (int i = 0; i < rows * no; ++i) SRH_REQUIRE(std::isfinite(A[i]), "%s: Y is not finite (A, row %d)", who, i / no);
    for (int i = 0; i < rows; ++i) SRH_REQUIRE(std::isfinite(b[i]), "%s: Y is not finite (b, row %d)", who, i);
    std::vector<double> c(A, A + (size_t)rows * no);
    c.insert(c.end(), b, b + rows);
    const int rc = d.upload(c.data(), sizeof(double) * c.size());
    if (rc) return rc;
    r.A = d.as<double>(); r.b = r.A + (size_t)rows * no; r.rows = rows;
    return SRH_OK;
}

}  // namespace

extern "C" {

int sgusto_ssm_loop_run(sgusto_ssm_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl, double *Y_cl,
                        double *Xhat, int32_t *iters, int32_t *status, double *J) {
    return ssm_loop_run(h, "sgusto_ssm_loop_run", periods, W, V, X_cl, Z_cl, U_cl, Y_cl, Xhat, iters, status, J, nullptr, nullptr);
}

int sgusto_ssm_loop_run_reprojected(sgusto_ssm_loop_t *h, int periods, const double *W, const double *V, double *X_cl, double *Z_cl, double *U_cl,
                                    double *Y_cl, double *Xhat, int32_t *iters, int32_t *status, double *J, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(h, "sgusto_ssm_loop_run_reprojected: null argument");
    SRH_REQUIRE(h->yrows, "sgusto_ssm_loop_run_reprojected: the loop has no Y (sgusto_ssm_loop_set_reproject)");
    return ssm_loop_run(h, "sgusto_ssm_loop_run_reprojected", periods, W, V, X_cl, Z_cl, U_cl, Y_cl, Xhat, iters, status, J, Y_used, proj);
}

int sgusto_ssm_loop_set_reproject(sgusto_ssm_loop_t *h, const double *A, const double *b, int rows) {
    SRH_REQUIRE(h, "sgusto_ssm_loop_set_reproject: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->have_state = false;               // the estimate the loops stand at was formed under the previous rule: a reset forms it anew
    if (!A || !b) {
        h->yrows = 0;
        return SRH_OK;
    }
    SRH_REQUIRE(h->observe, "sgusto_ssm_loop_set_reproject: the loop was created with observe = 0 (plans start from the plant state): no "
                "measurement is read, a Y would change nothing");
    const int no = h->no;
    SRH_REQUIRE(no <= poly::PN && rows > 0 && rows <= poly::PM,
                "sgusto_ssm_loop_set_reproject: Y needs n_o <= 16 and 0 < rows <= 64 (got n_o = %d, rows = %d)", no, rows);
    const size_t lds = h->tplant ? ssm_loop_tpwl_lds_bytes(h->np, h->m, h->n, no, h->planner->ns, true) : ssm_loop_lds_bytes(h->plant, h->planner, true);
    SRH_REQUIRE(lds <= (size_t)160 * 1024, "sgusto_ssm_loop_set_reproject: the advance kernel needs %zu bytes of LDS (160 KiB available)", lds);
    ReprojArgs r{};
    int rc;
    const size_t D = sizeof(double), B = (size_t)h->B;
    if ((rc = ssm_loop_stage_Y("sgusto_ssm_loop_set_reproject", A, b, rows, no, h->Yd, r)) || (rc = h->yucur.alloc(D * B * no)) ||
        (rc = h->pjcur.alloc(sizeof(int32_t) * B)))
        return rc;
    if (!h->YUrec.d.p) {
        h->YUrec.shape(D * no, 1); h->PJrec.shape(sizeof(int32_t), 1);
        if ((rc = h->alloc_recs({&h->YUrec, &h->PJrec}))) return rc;
    }
    h->YUrec.row0 = h->yucur.p; h->PJrec.row0 = h->pjcur.p;
    h->lds_proj = lds; h->yrows = rows;
    return SRH_OK;
}

int sgusto_ssm_loop_last_inputs(sgusto_ssm_loop_t *h, double *x0, double *u_init, double *x_init, double *z, double *u_des) {
    return loop_last_inputs(h, "sgusto_ssm_loop_last_inputs", x0, u_init, x_init, z, u_des);
}

int sgusto_ssm_loop_last_plan(sgusto_ssm_loop_t *h, double *xopt, double *uopt) { return loop_last_plan(h, "sgusto_ssm_loop_last_plan", xopt, uopt); }

int sgusto_ssm_loop_stats(sgusto_ssm_loop_t *h, int64_t *steps, int64_t *waits_last_run) {
    return loop_stats(h, "sgusto_ssm_loop_stats", steps, waits_last_run);
}

}  // extern "C"

namespace {

// YA (rows x n_o), Yb: the admissible set of the measurements, or null (then Y_used and proj are not written)
int ssm_loop_advance(const char *who, sssm_t *plant, int plant_mode, sssm_t *observer_model, double dt_sim, int N, int n_keep, int64_t batch,
                     const int32_t *j, const double *theta, const double *uopt, const double *x, const double *W, const double *V, double *X, double *Z,
                     double *U, double *Y, double *Xhat, const double *YA, const double *Yb, int yrows, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(plant && observer_model && j && theta && uopt && x && X && Z && U && Y && Xhat, "%s: null argument", who);
    SRH_REQUIRE(N >= 1 && n_keep >= 1 && batch >= 1 && dt_sim > 0.0, "%s: need N, n_keep, batch >= 1 and dt_sim > 0", who);
    for (int s = 0; s < n_keep; ++s)
        SRH_REQUIRE(j[s] >= 0 && j[s] <= N - 1, "%s: j[%d] = %d is not an interval 0..N-1 of the plan (N = %d)", who, s, j[s], N);
    size_t lds = 0;
    int rc;
    if ((rc = ssm_loop_check_models(who, plant, plant_mode, observer_model, &lds))) return rc;
    const size_t D = sizeof(double), B = (size_t)batch, n = plant->n, m = plant->m, no = plant->no, nk = n_keep;
    srh::DevBuf dj, dth, duo, dx, dW, dV, dX, dZ, dU, dY, dXH, dYs, dYu, dPj;
    ReprojArgs yp{};
    if (YA) {
        if ((rc = ssm_loop_stage_Y(who, YA, Yb, yrows, (int)no, dYs, yp)) || (rc = dYu.alloc(D * B * nk * no)) || (rc = dPj.alloc(sizeof(int32_t) * B * nk)))
            return rc;
        yp.Yu = dYu.as<double>(); yp.proj = dPj.as<int32_t>();
        lds = ssm_loop_lds_bytes(plant, observer_model, true);
        SRH_REQUIRE(lds <= (size_t)160 * 1024, "%s: the advance kernel needs %zu bytes of LDS (160 KiB available)", who, lds);
    }
    if ((rc = dj.upload(j, sizeof(int32_t) * nk)) || (rc = dth.upload(theta, D * nk)) || (rc = duo.upload(uopt, D * B * N * m)) ||
        (rc = dx.upload(x, D * B * n)) || (W && (rc = dW.upload(W, D * nk * B * n))) || (V && (rc = dV.upload(V, D * nk * B * no))) ||
        (rc = dX.alloc(D * B * nk * n)) || (rc = dZ.alloc(D * B * nk * no)) || (rc = dU.alloc(D * B * nk * m)) || (rc = dY.alloc(D * B * nk * no)) ||
        (rc = dXH.alloc(D * B * nk * n)))
        return rc;
    SsmAdvArgs a{};
    a.N = N; a.n_keep = n_keep; a.mode = plant_mode; a.same = observer_model == plant ? 1 : 0;
    a.dt_sim = dt_sim;
    a.js = dj.as<int32_t>(); a.theta = dth.as<double>();
    a.uopt = duo.as<double>();
    a.W = W ? dW.as<double>() : nullptr; a.Vn = V ? dV.as<double>() : nullptr;
    a.x_in = dx.as<double>();
    a.X = dX.as<double>(); a.Z = dZ.as<double>(); a.U = dU.as<double>(); a.Y = dY.as<double>(); a.Xhat = dXH.as<double>();
    a.rows_x = (int64_t)nk; a.rows_u = (int64_t)nk; a.B = batch;
    a.Yp_ = yp;
    if ((rc = loop_wait(ssm_loop_launch(plant, observer_model, lds, a, nullptr), nullptr))) return rc;
    if ((rc = dX.download(X, D * B * nk * n)) || (rc = dZ.download(Z, D * B * nk * no)) || (rc = dU.download(U, D * B * nk * m)) ||
        (rc = dY.download(Y, D * B * nk * no)) || (rc = dXH.download(Xhat, D * B * nk * n)) ||
        (YA && ((rc = dYu.download(Y_used, D * B * nk * no)) || (rc = dPj.download(proj, sizeof(int32_t) * B * nk)))))
        return rc;
    return SRH_OK;
}

int ssm_loop_advance_tpwl(const char *who, stpwl_t *plant, const double *Cm, const double *y_ref, int n_o, sssm_t *observer_model, double dt_sim, int N,
                          int n_keep, int64_t batch, const int32_t *j, const double *theta, const double *uopt, const double *x, const double *W,
                          const double *V, double *X, double *Z, double *U, double *Y, double *Xhat, int32_t *idx, const double *YA, const double *Yb,
                          int yrows, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(plant && Cm && y_ref && observer_model && j && theta && uopt && x && X && Z && U && Y && Xhat && idx, "%s: null argument", who);
    SRH_REQUIRE(N >= 1 && n_keep >= 1 && batch >= 1 && dt_sim > 0.0, "%s: need N, n_keep, batch >= 1 and dt_sim > 0", who);
    for (int s = 0; s < n_keep; ++s)
        SRH_REQUIRE(j[s] >= 0 && j[s] <= N - 1, "%s: j[%d] = %d is not an interval 0..N-1 of the plan (N = %d)", who, s, j[s], N);
    size_t lds = 0;
    int rc;
    if ((rc = ssm_loop_check_tpwl(who, plant, n_o, observer_model, &lds))) return rc;
    const size_t D = sizeof(double), B = (size_t)batch, np = plant->n, n = observer_model->n, m = plant->m, no = (size_t)n_o, nk = n_keep;
    std::vector<double> c(Cm, Cm + no * np);             // C | y_ref
    c.insert(c.end(), y_ref, y_ref + no);
    srh::DevBuf dc, dj, dth, duo, dx, dW, dV, dX, dZ, dU, dY, dXH, di, dYs, dYu, dPj;
    ReprojArgs yp{};
    if (YA) {
        if ((rc = ssm_loop_stage_Y(who, YA, Yb, yrows, n_o, dYs, yp)) || (rc = dYu.alloc(D * B * nk * no)) || (rc = dPj.alloc(sizeof(int32_t) * B * nk)))
            return rc;
        yp.Yu = dYu.as<double>(); yp.proj = dPj.as<int32_t>();
        lds = ssm_loop_tpwl_lds_bytes(plant->n, plant->m, observer_model->n, n_o, observer_model->ns, true);
        SRH_REQUIRE(lds <= (size_t)160 * 1024, "%s: the advance kernel needs %zu bytes of LDS (160 KiB available)", who, lds);
    }
    if ((rc = dc.upload(c.data(), D * c.size())) || (rc = dj.upload(j, sizeof(int32_t) * nk)) || (rc = dth.upload(theta, D * nk)) ||
        (rc = duo.upload(uopt, D * B * N * m)) || (rc = dx.upload(x, D * B * np)) || (W && (rc = dW.upload(W, D * nk * B * np))) ||
        (V && (rc = dV.upload(V, D * nk * B * no))) || (rc = dX.alloc(D * B * nk * np)) || (rc = dZ.alloc(D * B * nk * no)) ||
        (rc = dU.alloc(D * B * nk * m)) || (rc = dY.alloc(D * B * nk * no)) || (rc = dXH.alloc(D * B * nk * n)) ||
        (rc = di.alloc(sizeof(int32_t) * B * nk)))
        return rc;
    SsmTpwlAdvArgs a{};
    a.N = N; a.n_keep = n_keep; a.np = (int)np; a.m = (int)m; a.n = (int)n; a.no = n_o;
    a.js = dj.as<int32_t>(); a.theta = dth.as<double>();
    a.C = dc.as<double>(); a.yref = a.C + no * np;
    a.uopt = duo.as<double>();
    a.W = W ? dW.as<double>() : nullptr; a.Vn = V ? dV.as<double>() : nullptr;
    a.x_in = dx.as<double>();
    a.X = dX.as<double>(); a.Z = dZ.as<double>(); a.U = dU.as<double>(); a.Y = dY.as<double>(); a.Xhat = dXH.as<double>(); a.idx = di.as<int32_t>();
    a.rows_x = (int64_t)nk; a.rows_u = (int64_t)nk; a.B = batch;
    a.Yp_ = yp;
    if ((rc = loop_wait(ssm_loop_launch_tpwl(plant, observer_model, lds, a, nullptr), nullptr))) return rc;
    if ((rc = dX.download(X, D * B * nk * np)) || (rc = dZ.download(Z, D * B * nk * no)) || (rc = dU.download(U, D * B * nk * m)) ||
        (rc = dY.download(Y, D * B * nk * no)) || (rc = dXH.download(Xhat, D * B * nk * n)) || (rc = di.download(idx, sizeof(int32_t) * B * nk)) ||
        (YA && ((rc = dYu.download(Y_used, D * B * nk * no)) || (rc = dPj.download(proj, sizeof(int32_t) * B * nk)))))
        return rc;
    return SRH_OK;
}

}  // namespace

extern "C" {

int sgusto_ssm_loop_advance(sssm_t *plant, int plant_mode, sssm_t *observer_model, double dt_sim, int N, int n_keep, int64_t batch, const int32_t *j,
                            const double *theta, const double *xopt, const double *uopt, const double *x, const double *W, const double *V, double *X,
                            double *Z, double *U, double *Y, double *Xhat) {
    (void)xopt;                         // (the law u = u_bar(t) has no gain: the plan's states are not read)
    return ssm_loop_advance("sgusto_ssm_loop_advance", plant, plant_mode, observer_model, dt_sim, N, n_keep, batch, j, theta, uopt, x, W, V, X, Z, U,
                            Y, Xhat, nullptr, nullptr, 0, nullptr, nullptr);
}

int sgusto_ssm_loop_advance_reprojected(sssm_t *plant, int plant_mode, sssm_t *observer_model, double dt_sim, int N, int n_keep, int64_t batch,
                                        const int32_t *j, const double *theta, const double *uopt, const double *x, const double *W, const double *V,
                                        const double *YA, const double *Yb, int y_rows, double *X, double *Z, double *U, double *Y, double *Xhat,
                                        double *Y_used, int32_t *proj) {
    SRH_REQUIRE(YA && Yb && Y_used && proj, "sgusto_ssm_loop_advance_reprojected: null argument");
    return ssm_loop_advance("sgusto_ssm_loop_advance_reprojected", plant, plant_mode, observer_model, dt_sim, N, n_keep, batch, j, theta, uopt, x, W, V,
                            X, Z, U, Y, Xhat, YA, Yb, y_rows, Y_used, proj);
}

int sgusto_ssm_loop_advance_tpwl(stpwl_t *plant, const double *Cm, const double *y_ref, int n_o, sssm_t *observer_model, double dt_sim, int N,
                                 int n_keep, int64_t batch, const int32_t *j, const double *theta, const double *uopt, const double *x,
                                 const double *W, const double *V, double *X, double *Z, double *U, double *Y, double *Xhat, int32_t *idx) {
    return ssm_loop_advance_tpwl("sgusto_ssm_loop_advance_tpwl", plant, Cm, y_ref, n_o, observer_model, dt_sim, N, n_keep, batch, j, theta, uopt, x, W,
                                 V, X, Z, U, Y, Xhat, idx, nullptr, nullptr, 0, nullptr, nullptr);
}

int sgusto_ssm_loop_advance_tpwl_reprojected(stpwl_t *plant, const double *Cm, const double *y_ref, int n_o, sssm_t *observer_model, double dt_sim,
                                             int N, int n_keep, int64_t batch, const int32_t *j, const double *theta, const double *uopt,
                                             const double *x, const double *W, const double *V, const double *YA, const double *Yb, int y_rows,
                                             double *X, double *Z, double *U, double *Y, double *Xhat, int32_t *idx, double *Y_used, int32_t *proj) {
    SRH_REQUIRE(YA && Yb && Y_used && proj, "sgusto_ssm_loop_advance_tpwl_reprojected: null argument");
    return ssm_loop_advance_tpwl("sgusto_ssm_loop_advance_tpwl_reprojected", plant, Cm, y_ref, n_o, observer_model, dt_sim, N, n_keep, batch, j, theta,
                                 uopt, x, W, V, X, Z, U, Y, Xhat, idx, YA, Yb, y_rows, Y_used, proj);
}

}  // extern "C"
