// The Euclidean projection onto a polyhedron {p : A p <= b} as a device unit of ONE wave (the method is described in poly.hip, which
// states the stand-alone kernel and the host entries; the closed-loop advance kernels of koopman_loop.hip call the same function on the
// measurement of every sub-step, so that a sample projected inside a loop has the bits of the stand-alone call).
//
// The calling wave may sit in a larger workgroup: the unit calls no workgroup barrier.  Lane i owns row i (its row of A and b_i are
// handed in in registers, so that a loop loads them once per launch), the n-vectors are uniform in every lane, and what one lane
// writes to LDS for the others to read -- the normal matrix and its factor, the closing step's q, R and multipliers -- lives in a work
// area of the wave's own (poly::Work, poly::LDS_BYTES) and is ordered with __builtin_amdgcn_wave_barrier(): the LDS operations of one
// wave are carried out in the order they are issued, the barrier only keeps the compiler from moving them.
//
// project_wave never ends a launch.  It answers
//    0   already inside (max(A x - b) > 0 is false): out = x bit for bit
//    1   projected, with the certificate of poly.hip (max(A p - b) <= 1e-12 scale, multipliers >= -1e-12 scale)
//   -1   no certified projection in max_iter iterations (an empty polyhedron, for instance); NOT_PD where the normal matrix lost its
//        definiteness on the way (status_word folds it into -1; spoly_project words its message by it)
//   -2   the point is not finite (the wave reductions drop NaNs: without this test a NaN point would count as inside)
// and for -1 and -2 out = x.
#pragma once
#include "common.h"
#include "dev_la.h"

namespace poly {

constexpr int PN = 16;      // max dimension
constexpr int PM = 64;      // max rows

constexpr int INSIDE = 0, PROJECTED = 1, NO_CERTIFICATE = -1, NOT_FINITE = -2, NOT_PD = -3;
__host__ __device__ inline int status_word(int code) { return code == NOT_PD ? NO_CERTIFICATE : code; }

constexpr double IDENT_MU = 1e-9;      // the closing step is tried once mu <= IDENT_MU scale and both residuals <= IDENT_RES scale
constexpr double IDENT_RES = 1e-6;
constexpr double CERT_TOL = 1e-12;     // feasibility and sign of the multipliers of a returned point, relative to scale
constexpr double DEPENDENT = 1e-18;    // |z|^2 / |a|^2 below this: the row depends on the rows already taken (an angle of 1e-9)
constexpr int CLOSING_ROUNDS = 16;
constexpr int MAX_ITER = 60;

// the work area of one calling wave, in doubles: M, Lc, Rm (PN x PN each) | rhs, sol, qs, cs, ls (PN each) | lmin | then the words
// sel (PN), jmin, flag
constexpr int WORK_DOUBLES = 3 * PN * PN + 5 * PN + 1;
constexpr int WORK_INTS = PN + 2;
constexpr int LDS_BYTES = (WORK_DOUBLES * 8 + WORK_INTS * 4 + 15) & ~15;          // 6864: about 6.9 KB

struct Work {
    lptr M, Lc, rhs, sol;
    lptr Rm, qs, cs, ls, lmin;          // closing step: R of A_S^T = Q R, the current q, Q^T (x - p), lam
    liptr sel, jmin, flag;
};

__device__ __forceinline__ Work carve(lptr base) {
    Work w;
    w.M = base; w.Lc = w.M + PN * PN; w.Rm = w.Lc + PN * PN;
    w.rhs = w.Rm + PN * PN; w.sol = w.rhs + PN; w.qs = w.sol + PN; w.cs = w.qs + PN; w.ls = w.cs + PN; w.lmin = w.ls + PN;
    w.sel = (liptr)(w.lmin + 1); w.jmin = w.sel + PN; w.flag = w.jmin + 1;
    return w;
}

// wg::chol_factor for one wave: the same arithmetic on lane 0, the verdict through `flag`, no workgroup barrier
__device__ __forceinline__ bool chol_factor_wave(clptr Q, lptr Lbuf, int m, liptr flag, int lane, bool allow_shift) {
    if (lane == 0) {
        bool ok = false;
        double dmax = 0.0;
        for (int i = 0; i < m; ++i) dmax = fmax(dmax, fabs(Q[i * m + i]));
        double shift = 0.0;
        for (int attempt = 0; attempt < (allow_shift ? 8 : 1) && !ok; ++attempt) {
            ok = true;
            for (int i = 0; i < m && ok; ++i) {
                for (int j = 0; j <= i; ++j) {
                    double sum = Q[i * m + j] + (i == j ? shift : 0.0);
                    for (int k = 0; k < j; ++k) sum -= Lbuf[i * m + k] * Lbuf[j * m + k];
                    if (i == j) {
                        if (!(sum > 0.0)) { ok = false; break; }
                        Lbuf[i * m + i] = sqrt(sum);
                    } else {
                        Lbuf[i * m + j] = sum / Lbuf[j * m + j];
                    }
                }
            }
            shift = (shift == 0.0) ? 1e-14 * dmax : shift * 100.0;
        }
        *flag = ok ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
    return *flag != 0;
}

// One wave, all 64 lanes.  ar, bi: row `lane` of A (zeros beyond n and beyond mc) and its bound (1 beyond mc); x: the point (n, any
// address space; read more than once, never written); out (n): the answer, may not overlap x; w: the wave's work area.
template <typename XP, typename OP>
__device__ __forceinline__ int project_wave(const double (&ar)[PN], const double bi, const int mc, const int n, XP x, OP out, const Work &w,
                                            const int lane, const int max_iter) {
    const bool act = lane < mc;
    lptr M = w.M, Lc = w.Lc, rhs = w.rhs, sol = w.sol, Rm = w.Rm, qs = w.qs, cs = w.cs, ls = w.ls;
    liptr sel = w.sel;
    double p[PN];
    bool fin = true;
#pragma unroll
    for (int k = 0; k < PN; ++k) {
        p[k] = k < n ? x[k] : 0.0;
        fin = fin && fabs(p[k]) <= 1.79769313486231570815e308;         // (false for a NaN and for an Inf)
    }
    if (!fin) {
        if (lane < n) out[lane] = x[lane];
        return NOT_FINITE;
    }
    auto adot = [&](const double (&v)[PN]) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < PN; ++k) s = fma(ar[k], v[k], s);
        return s;
    };
    // scale of the data for the stopping rule
    double xs = 0.0;
#pragma unroll
    for (int k = 0; k < PN; ++k) xs = fmax(xs, fabs(p[k]));
    const double scale = fmax(1.0, fmax(xs, wg::wave_max(act ? fabs(bi) : 0.0)));
    double viol = act ? adot(p) - bi : -1.0;
    int st = 0, it = 0;
    if (!(wg::wave_max(viol) > 0.0)) {          // already inside: the projection is x itself
        if (lane < n) out[lane] = x[lane];
        return INSIDE;
    }
    double s = act ? fmax(-viol, 1e-2 * scale) : 1.0, lam = act ? fmax(viol, 1e-2 * scale) : 0.0;
    // one Newton solve: (I + A^T D A) dp = -r_d - A^T (D r_p - r_c / s), then d lam, d s; r_c passed in
    double rd[PN];
    auto newton = [&](double rp, double rc, double &dlam, double &ds, double (&dp)[PN]) -> bool {
        const double d = act ? lam / s : 0.0;
        const double wv = act ? d * rp - rc / s : 0.0;
        for (int r = 0; r < n; ++r) {
            for (int c = r; c < n; ++c) {
                const double v = wg::wave_sum(d * ar[r] * ar[c]);
                if (lane == 0) { M[r * n + c] = v + (r == c ? 1.0 : 0.0); M[c * n + r] = M[r * n + c]; }
            }
            const double g = wg::wave_sum(ar[r] * wv);
            if (lane == 0) rhs[r] = rd[r] + g;          // solve gives -(M^-1) rhs
        }
        __builtin_amdgcn_wave_barrier();
        if (!chol_factor_wave((clptr)M, Lc, n, w.flag, lane, true)) return false;
        if (lane == 0) wg::chol_solve_neg((clptr)Lc, n, (clptr)rhs, 1, sol, 1);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < PN; ++k) dp[k] = k < n ? sol[k] : 0.0;
        __builtin_amdgcn_wave_barrier();
        dlam = act ? d * (adot(dp) + rp) - rc / s : 0.0;
        ds = act ? -(rc + s * dlam) / lam : 0.0;
        return true;
    };
    auto max_step = [&](double v, double dv) { return (act && dv < 0.0) ? -v / dv : INFINITY; };
    // the closing step (stage 2 of poly.hip) from the current lam, s; true with the certified point in pw
    double pw[PN];
    auto closing = [&]() -> bool {
        bool inW = act && lam >= s;
        double na2 = 0.0;
#pragma unroll
        for (int k = 0; k < PN; ++k) na2 = fma(ar[k], ar[k], na2);
        const double tolc = CERT_TOL * scale;
        for (int round = 0; round < CLOSING_ROUNDS; ++round) {
            double z[PN], h[PN];
#pragma unroll
            for (int k = 0; k < PN; ++k) { z[k] = ar[k]; h[k] = 0.0; pw[k] = k < n ? x[k] : 0.0; }
            bool taken = false;
            int nsel = 0;
#pragma unroll
            for (int k = 0; k < PN; ++k) {
                if (k >= n) break;
                double zz = 0.0;
#pragma unroll
                for (int m = 0; m < PN; ++m) zz = fma(z[m], z[m], zz);
                const double cand = (inW && !taken && na2 > 0.0) ? zz / na2 : -1.0;
                const double best = wg::wave_max(cand);
                if (!(best > DEPENDENT)) break;
                const int j = __ffsll((long long)__ballot(cand == best)) - 1;         // the first lane that holds the maximum
                if (lane == j) {
                    const double nz = sqrt(zz);
#pragma unroll
                    for (int m = 0; m < PN; ++m) qs[m] = z[m] / nz;
#pragma unroll
                    for (int m = 0; m < PN; ++m)
                        if (m < k) Rm[m * PN + k] = h[m];
                    Rm[k * PN + k] = nz;
                    cs[k] = (adot(pw) - bi) / nz;           // the step along q that puts row j on its bound; earlier rows stay
                    sel[k] = j;
                    taken = true;
                }
                __builtin_amdgcn_wave_barrier();
                double q[PN];
#pragma unroll
                for (int m = 0; m < PN; ++m) q[m] = qs[m];
                const double ck = cs[k];
#pragma unroll
                for (int m = 0; m < PN; ++m) pw[m] = fma(-ck, q[m], pw[m]);
                for (int pass = 0; pass < 2; ++pass) {              // orthogonalised twice
                    double g = 0.0;
#pragma unroll
                    for (int m = 0; m < PN; ++m) g = fma(z[m], q[m], g);
#pragma unroll
                    for (int m = 0; m < PN; ++m) z[m] = fma(-g, q[m], z[m]);
                    h[k] += g;
                }
                nsel = k + 1;
                __builtin_amdgcn_wave_barrier();
            }
            // x - p = Q c = A_S^T lam:  R lam = c
            if (lane == 0) {
                double lm = INFINITY;
                int jm = -1;
                for (int i = nsel - 1; i >= 0; --i) {
                    double sum = cs[i];
                    for (int m = i + 1; m < nsel; ++m) sum -= Rm[i * PN + m] * ls[m];
                    ls[i] = sum / Rm[i * PN + i];
                }
                for (int i = 0; i < nsel; ++i)
                    if (ls[i] < lm) { lm = ls[i]; jm = sel[i]; }
                *w.lmin = lm;
                *w.jmin = jm;
            }
            __builtin_amdgcn_wave_barrier();
            const double lm = *w.lmin;
            const int jm = *w.jmin;
            __builtin_amdgcn_wave_barrier();
            if (nsel > 0 && !(lm >= -tolc)) {               // the most negative multiplier leaves (a NaN ends the step below)
                if (!(lm < 0.0)) return false;
                if (lane == jm) inW = false;
                continue;
            }
            const double v = act ? adot(pw) - bi : -INFINITY;
            const double vmax = wg::wave_max(v);
            bool finite = vmax > -1e300;
#pragma unroll
            for (int k = 0; k < PN; ++k) finite = finite && fabs(pw[k]) < 1e300;
            if (!finite) return false;
            if (!(vmax > tolc)) return true;
            const int j = __ffsll((long long)__ballot(v == vmax)) - 1;              // the most violated row joins
            if ((__ballot(inW) >> j) & 1) return false;    // it is in the set already and depends on the rows taken
            if (lane == j) inW = true;
        }
        return false;
    };
    bool certified = false;
    for (;; ++it) {
        // residuals
        double rdn = 0.0;
#pragma unroll
        for (int k = 0; k < PN; ++k) {
            rd[k] = k < n ? p[k] - x[k] + wg::wave_sum(ar[k] * lam) : 0.0;
            rdn = fmax(rdn, fabs(rd[k]));
        }
        const double rp = act ? adot(p) + s - bi : 0.0;
        const double rpn = wg::wave_max(fabs(rp));
        const double mu = wg::wave_sum(act ? s * lam : 0.0) / mc;
        if (mu <= IDENT_MU * scale && rpn <= IDENT_RES * scale && rdn <= IDENT_RES * scale && closing()) { certified = true; break; }
        if (it >= max_iter) { st = 1; break; }
        double dla, dsa, dpa[PN], dl, dsv, dp[PN];
        if (!newton(rp, act ? s * lam : 0.0, dla, dsa, dpa)) { st = 2; break; }
        double aa = fmin(1.0, wg::wave_min(fmin(max_step(s, dsa), max_step(lam, dla))));
        const double mua = wg::wave_sum(act ? (s + aa * dsa) * (lam + aa * dla) : 0.0) / mc;
        const double sig = (mua / mu) * (mua / mu) * (mua / mu);
        if (!newton(rp, act ? s * lam + dsa * dla - sig * mu : 0.0, dl, dsv, dp)) { st = 2; break; }
        const double al = fmin(1.0, 0.99 * wg::wave_min(fmin(max_step(s, dsv), max_step(lam, dl))));
#pragma unroll
        for (int k = 0; k < PN; ++k) p[k] += al * dp[k];
        if (act) { s += al * dsv; lam += al * dl; }
    }
    if (lane < n) out[lane] = certified ? pw[lane < PN ? lane : 0] : x[lane];
    return certified ? PROJECTED : (st == 2 ? NOT_PD : NO_CERTIFICATE);
}

// row `lane` of A (rows x n, row-major) and b into the registers project_wave takes
template <typename AP>
__device__ __forceinline__ void load_row(AP A, AP b, const int mc, const int n, const int lane, double (&ar)[PN], double &bi) {
    const bool act = lane < mc;
#pragma unroll
    for (int k = 0; k < PN; ++k) ar[k] = (act && k < n) ? A[lane * n + k] : 0.0;
    bi = act ? b[lane] : 1.0;
}

}  // namespace poly
