// The interior point's rule on ONE inequality row  a . v <= h  (slack t, multiplier lambda), stated ONCE for the seven QP kernels --
// the fused Riccati solve (locp_dev.h), the condensed solve (locp_cond.h), the four lean forms (locp_lean.h) and the dense-in-u form
// (locp_dense_u.h) -- and for the host replay (sqp_ipm_rule_replay).  Mehrotra predictor-corrector with a dual regularisation dreg,
// as oracle/condensed_ipm.py / oracle/riccati_ipm.py state it.  Plain doubles in, plain doubles out: no LDS, no thread indices, no
// reductions.  How a kernel finds a row's value g = a . v - h and its direction a . d, where its rows live, how it reduces over them, its
// phase order, barriers, profiling laps and debug trace are tuning and stay in the kernel.  A kernel's iteration:
//   cold:  init_row -> Newton step -> start_shift(min g, max g), start_cold          warm:  start_warm (no starting system)
//   scales (once per QP), then per iteration
//   PRED:  pred_row -> Newton system -> direction(pred), step_bound -> verdict -> step_affine, affine_term -> centring
//          The lean forms (locp_lean.h) test convergence BEFORE the system, as the oracle does (condensed_ipm.py:286-292): behind
//          pred_row, where may_converge holds, they take the dual residual from the product G^T g_yd alone and stop with status 0 if
//          converged holds -- no Newton system is built for an iterate that needs no step (QPDims::ipm_late_stop = 1 keeps the test
//          inside verdict only).  The fused, condensed and dense-in-u kernels test in verdict, behind the system.
//   CORR:  corr_row -> Newton system -> direction(!pred), step_bound -> step_length, advance
// The operation order and grouping of every expression is what the kernels' results depend on bit for bit: keep it.
#pragma once
#include <cmath>

#define SRH_IPM __host__ __device__ __forceinline__

namespace ipm {

constexpr double WARM_FLOOR = 1e-2;     // warm start: slacks and multipliers at least this far from zero (oracle/condensed_ipm.py: WARM_FLOOR)
constexpr int GO_ON = -1;               // verdict(): no reason to stop

// ---- starting point, cold: the unit-weight Newton system (unit = 0 where the QP has no rows at all), gradient shift = row value
SRH_IPM void init_row(double g, double unit, double &D, double &rho, double &lam) { D = unit; rho = g; lam = 0.0; }
// Mehrotra's shifts from the smallest and the largest row value at the Newton point: every slack and multiplier >= 1
struct Shift { double t, l; };
SRH_IPM Shift start_shift(double zmin, double zmax) {
    const double sh_t = zmax >= 0.0 ? 1.0 + zmax : 0.0, sh_l = zmin <= 0.0 ? 1.0 - zmin : 0.0;
    return Shift{sh_t, sh_l};
}
SRH_IPM void start_cold(double g, const Shift &sh, double &t, double &lam) { t = -g + sh.t; lam = g + sh.l; }
// ---- starting point, warm: the slack from THIS QP's row value, the previous QP's multiplier (poison: +inf, the test knob that makes
// the warm attempt fail).  lam_prev(): a callable, the kernel's load of that multiplier -- not made for a poisoned start
template <class LamPrev>
SRH_IPM void start_warm(double g, LamPrev &&lam_prev, bool poison, double &t, double &lam) {
    t = fmax(-g, WARM_FLOOR);
    lam = poison ? INFINITY : fmax(lam_prev(), WARM_FLOOR);
}
// ---- residual scales of the stopping test from the two maxima a kernel reduced, and the regularisation relative to the dual scale
SRH_IPM void scales(double omega, double delta, double reg, double &sd, double &sp, double &dreg) {
    sd = fmax(sd, omega);
    sp = fmax(sp, fabs(delta));
    dreg = reg / sd;
}
// ---- predictor row: residual rg, regularised weight D = lambda / (t + dreg lambda), gradient shift rho; the row's terms of
// sum lambda t (musum) and max |rg| (rpm) are accumulated
SRH_IPM void pred_row(double g, double t, double lam, double dreg, double &rg_out, double &D_out, double &rho, double &musum, double &rpm) {
    const double rg = g + t;
    rg_out = rg;
    const double D = lam / (t + dreg * lam);
    D_out = D;
    rho = D * (rg + dreg * lam);
    musum += lam * t;
    rpm = fmax(rpm, fabs(rg));
}
// ---- corrector row: centring residual rc and its gradient shift
SRH_IPM void corr_row(double t, double lam, double rg, double dt, double dl, double sig, double mu, double dreg, double &rc_out, double &rho) {
    const double rc = lam * t + dt * dl - sig * mu;
    rc_out = rc;
    rho = lam + (lam * rg - rc) / (t + dreg * lam);
}
// ---- row direction from ad = a . d (pred: the affine direction, else the centred one), and the largest step that keeps t, lambda > 0
SRH_IPM void direction(bool pred, double t, double lam, double rg, double rc, double ad, double dreg, double &dl_out, double &dt_out) {
    const double rga = rg + ad;
    const double dl = ((pred ? -lam * t : -rc) + lam * rga) / (t + dreg * lam);
    const double dtv = -rga + dreg * dl;
    dl_out = dl; dt_out = dtv;
}
SRH_IPM void step_bound(double t, double lam, double dt, double dl, double &amax) {
    if (dt < 0.0) amax = fmin(amax, -t / dt);
    if (dl < 0.0) amax = fmin(amax, -lam / dl);
}
// ---- step lengths from the bound: the affine step may reach the boundary, the step taken stays strictly interior
SRH_IPM double step_affine(double amax) { return fmin(1.0, amax); }
SRH_IPM double step_length(double amax) { return fmin(1.0, 0.99 * amax); }
// the row's term of the affine complementarity sum, and the centring parameter from its mean
SRH_IPM double affine_term(double t, double lam, double dt, double dl, double a_aff) { return (lam + a_aff * dl) * (t + a_aff * dt); }
SRH_IPM double centring(double mu_aff, double mu) { return mu > 0.0 ? (mu_aff / mu) * (mu_aff / mu) * (mu_aff / mu) : 0.0; }
SRH_IPM void advance(double a, double dt, double dl, double &t, double &lam) { t += a * dt; lam += a * dl; }
// ---- the stopping ladder of the predictor phase: a status to stop with, or GO_ON.  A factorisation that breaks down (or a NaN) in the
// last digits of an already converged iterate -- weights D = lambda / t up to 1e13 -- is accepted at the looser 1e-8 certificate the
// iteration before left in near_opt; the linear residuals have a round-off floor of 1e-9 relative.
SRH_IPM int verdict_failed(bool ok, double mu, double rd, bool near_opt) {
    if (!ok) return near_opt ? 0 : 2;
    if (!(mu == mu)) return near_opt ? 0 : 5;
    if (!(rd == rd)) return near_opt ? 0 : 6;
    return GO_ON;
}
// the stopping test itself (NaN in any argument: not converged), and the part of it that needs no product with G: the gate of the
// lean forms' early test
SRH_IPM bool converged(double mu, double rd, double rp, double sd, double sp, double tol) {
    const double ltol = fmax(tol, 1e-9);
    return rd <= ltol * sd && rp <= ltol * sp && mu <= tol;
}
SRH_IPM bool may_converge(double mu, double rp, double sp, double tol) {
    const double ltol = fmax(tol, 1e-9);
    return rp <= ltol * sp && mu <= tol;
}
SRH_IPM int verdict_converged(double mu, double rd, double rp, double sd, double sp, double tol, int it, int max_iter, bool &near_opt) {
    if (converged(mu, rd, rp, sd, sp, tol)) return 0;
    near_opt = (rd <= 1e-8 * sd && rp <= 1e-8 * sp && mu <= 1e-8);
    if (it >= max_iter) return 1;
    return GO_ON;
}
// the ladder in one piece; a kernel that writes its debug trace between the two halves, as it always has, calls them one by one
SRH_IPM int verdict(bool ok, double mu, double rd, double rp, double sd, double sp, double tol, int it, int max_iter, bool &near_opt) {
    const int v = verdict_failed(ok, mu, rd, near_opt);
    return v != GO_ON ? v : verdict_converged(mu, rd, rp, sd, sp, tol, it, max_iter, near_opt);
}
// the starting system and the corrector system have no certificate to fall back on; a QP without rows is solved by its starting system
SRH_IPM int verdict_system(bool ok) { return ok ? GO_ON : 2; }
SRH_IPM int verdict_no_rows(int ng) { return ng == 0 ? 0 : GO_ON; }
// `if (ipm::stops(ipm::verdict...(..), status)) break;`
SRH_IPM bool stops(int v, int &status) {
    if (v == GO_ON) return false;
    status = v;
    return true;
}

}  // namespace ipm

#undef SRH_IPM
