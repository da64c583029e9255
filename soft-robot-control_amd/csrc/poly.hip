// Euclidean projection onto a polyhedron {p : A p <= b}: min 1/2 |p - x|^2 s.t. A p <= b.
// Reference: sofacontrol/utils.py:364-407 (Polyhedron(with_reproject=True).project_to_polyhedron: the same QP handed to
// OSQP with P = I, q = -x); used on measurements that left the admissible set, SSM/controllers.py:96-97.
// One wave per point, lane i owns constraint i (slack, multiplier, row of A in registers), the n-vectors are kept uniform in
// every lane (n <= 16, rows <= 64: these are output-space boxes and a few facets).  Two stages:
//   1. a Mehrotra predictor-corrector interior point finds the active set: the n x n normal matrix I + A^T D A is summed with
//      wave reductions and factored in LDS.  In float64 its iterate is no better than sqrt(rows mu) at a weakly active row, and its
//      multipliers lose eps |dp| lam / s on the strongly active ones, so it is never the result.
//   2. a closing step on the rows it points to (lam_i >= s_i): the projection of x onto the affine hull of an independent part of
//      them (pivoted modified Gram-Schmidt, each lane orthogonalising its own row), the multipliers from the triangular factor,
//      then the two checks of an active-set method -- a negative multiplier leaves the set, the most violated row joins it --
//      and again.  It returns only a point with max(A p - b) <= 1e-12 scale and multipliers >= -1e-12 scale that is stationary
//      and complementary by construction: the KKT certificate of the unique projection.  scale = max(1, |x|_inf, |b|_inf).
// Success means that certificate; a point the interior point reaches without one (60 iterations) is reported, never returned.
#include "common.h"
#include "dev_la.h"

namespace {

constexpr int PN = 16;      // max dimension
constexpr int PM = 64;      // max rows

struct PolyArgs {
    const double *A, *b, *X;
    double *out;
    int *status;
    int mc, n;
    int max_iter;
};

constexpr double IDENT_MU = 1e-9;      // the closing step is tried once mu <= IDENT_MU scale and both residuals <= IDENT_RES scale
constexpr double IDENT_RES = 1e-6;
constexpr double CERT_TOL = 1e-12;     // feasibility and sign of the multipliers of a returned point, relative to scale
constexpr double DEPENDENT = 1e-18;    // |z|^2 / |a|^2 below this: the row depends on the rows already taken (an angle of 1e-9)
constexpr int CLOSING_ROUNDS = 16;

__global__ __launch_bounds__(64) void poly_project_kernel(PolyArgs a) {
    __shared__ double M[PN * PN], Lc[PN * PN], rhs[PN], sol[PN];
    __shared__ double Rm[PN * PN], qs[PN], cs[PN], ls[PN], lmin_s;     // closing step: R of A_S^T = Q R, the current q, Q^T (x - p), lam
    __shared__ int sel[PN], jmin_s;
    __shared__ int flag;
    const int lane = threadIdx.x, n = a.n, mc = a.mc;
    const bool act = lane < mc;
    const double *x = a.X + (size_t)blockIdx.x * n;
    double ar[PN], p[PN];
#pragma unroll
    for (int k = 0; k < PN; ++k) {
        ar[k] = (act && k < n) ? a.A[lane * n + k] : 0.0;
        p[k] = k < n ? x[k] : 0.0;
    }
    const double bi = act ? a.b[lane] : 1.0;
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
        if (lane < n) a.out[(size_t)blockIdx.x * n + lane] = x[lane];
        if (lane == 0) a.status[blockIdx.x] = 0;
        return;
    }
    double s = act ? fmax(-viol, 1e-2 * scale) : 1.0, lam = act ? fmax(viol, 1e-2 * scale) : 0.0;
    // one Newton solve: (I + A^T D A) dp = -r_d - A^T (D r_p - r_c / s), then d lam, d s; r_c passed in
    double rd[PN];
    auto newton = [&](double rp, double rc, double &dlam, double &ds, double (&dp)[PN]) -> bool {
        const double d = act ? lam / s : 0.0;
        const double w = act ? d * rp - rc / s : 0.0;
        for (int r = 0; r < n; ++r) {
            for (int c = r; c < n; ++c) {
                const double v = wg::wave_sum(d * ar[r] * ar[c]);
                if (lane == 0) { M[r * n + c] = v + (r == c ? 1.0 : 0.0); M[c * n + r] = M[r * n + c]; }
            }
            const double g = wg::wave_sum(ar[r] * w);
            if (lane == 0) rhs[r] = rd[r] + g;          // solve gives -(M^-1) rhs
        }
        __syncthreads();
        if (!wg::chol_factor((clptr)M, (lptr)Lc, n, (liptr)&flag, true)) return false;
        if (lane == 0) wg::chol_solve_neg((clptr)Lc, n, (clptr)rhs, 1, (lptr)sol, 1);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PN; ++k) dp[k] = k < n ? sol[k] : 0.0;
        __syncthreads();
        dlam = act ? d * (adot(dp) + rp) - rc / s : 0.0;
        ds = act ? -(rc + s * dlam) / lam : 0.0;
        return true;
    };
    auto max_step = [&](double v, double dv) { return (act && dv < 0.0) ? -v / dv : INFINITY; };
    // the closing step (stage 2 above) from the current lam, s; true with the certified point in pw
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
                __syncthreads();
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
                __syncthreads();
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
                lmin_s = lm;
                jmin_s = jm;
            }
            __syncthreads();
            const double lm = lmin_s;
            const int jm = jmin_s;
            __syncthreads();
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
        if (it >= a.max_iter) { st = 1; break; }
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
    if (lane < n) a.out[(size_t)blockIdx.x * n + lane] = certified ? pw[lane < PN ? lane : 0] : p[lane < PN ? lane : 0];
    if (lane == 0) a.status[blockIdx.x] = st;
}

}  // namespace

extern "C" {

int spoly_project(const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out) {
    SRH_REQUIRE(A && b && X && out, "spoly_project: null argument");
    SRH_REQUIRE(n > 0 && n <= PN && n_rows > 0 && n_rows <= PM, "spoly_project: need 0 < n <= 16 and 0 < rows <= 64 (got %d, %d)",
                n, n_rows);
    // fmax / fmin drop NaNs: a non-finite number would pass the kernel's first test as "already inside"
    for (int i = 0; i < n_rows * n; ++i) SRH_REQUIRE(std::isfinite(A[i]), "spoly_project: the polyhedron is not finite (A, row %d)", i / n);
    for (int i = 0; i < n_rows; ++i) SRH_REQUIRE(std::isfinite(b[i]), "spoly_project: the polyhedron is not finite (b, row %d)", i);
    for (int64_t i = 0; i < batch * n; ++i)
        if (!std::isfinite(X[i])) {
            srh::set_error("spoly_project: point %lld is not finite (coordinate %d is NaN or Inf)", (long long)(i / n), (int)(i % n));
            return SRH_ENUMERIC;
        }
    if (batch == 0) return SRH_OK;
    srh::DevBuf dA, db, dX, dO, dS;
    int rc;
    if ((rc = dA.upload(A, sizeof(double) * n_rows * n)) || (rc = db.upload(b, sizeof(double) * n_rows)) ||
        (rc = dX.upload(X, sizeof(double) * batch * n)) || (rc = dO.alloc(sizeof(double) * batch * n)) ||
        (rc = dS.alloc(sizeof(int) * batch)))
        return rc;
    PolyArgs a{dA.as<double>(), db.as<double>(), dX.as<double>(), dO.as<double>(), dS.as<int>(), n_rows, n, 60};
    poly_project_kernel<<<(unsigned)batch, 64>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    std::vector<int> st((size_t)batch);
    if ((rc = dS.download(st.data(), sizeof(int) * batch))) return rc;
    for (int64_t i = 0; i < batch; ++i)
        if (st[i] != 0) {
            srh::set_error("spoly_project: point %lld: %s", (long long)i,
                           st[i] == 1 ? "no certified projection in 60 iterations (empty polyhedron?)"
                                      : "normal matrix not positive definite: the iteration diverged (empty polyhedron?)");
            return SRH_ENUMERIC;
        }
    return dO.download(out, sizeof(double) * batch * n);
}

}  // extern "C"
