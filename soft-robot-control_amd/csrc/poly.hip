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
// The method itself is poly_dev.h (poly::project_wave, one wave, no workgroup barrier: the closed-loop advance kernels call it too);
// this unit is its stand-alone kernel and the two host entries: spoly_project fails the call at the first point without a projection,
// spoly_project_status hands back the status word of every point.
#include "poly_dev.h"

namespace {

using poly::PN;
using poly::PM;

struct PolyArgs {
    const double *A, *b, *X;
    double *out;
    int *status;                        // the words of poly_dev.h (0, 1, -1, -2), or null
    int *detail;                        // the same with NOT_PD kept apart, or null
    int mc, n;
    int max_iter;
};

// One workgroup of one wave per point: the thin caller of poly::project_wave
__global__ __launch_bounds__(64) void poly_project_kernel(PolyArgs a) {
    __shared__ __attribute__((aligned(16))) char work[poly::LDS_BYTES];
    const int lane = threadIdx.x, n = a.n;
    double ar[PN], bi;
    poly::load_row(a.A, a.b, a.mc, n, lane, ar, bi);
    const int code = poly::project_wave(ar, bi, a.mc, n, a.X + (size_t)blockIdx.x * n, a.out + (size_t)blockIdx.x * n,
                                        poly::carve((lptr)work), lane, a.max_iter);
    if (lane == 0) {
        if (a.status) a.status[blockIdx.x] = poly::status_word(code);
        if (a.detail) a.detail[blockIdx.x] = code;
    }
}

// the checks both entries share, then the launch.  strict (spoly_project): a point that is not finite, or that gets no certificate,
// fails the call and `out` is not written; otherwise words (batch) receives the status words of poly_dev.h.
int poly_run(const char *who, const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out,
             int32_t *words, bool strict) {
    SRH_REQUIRE(n > 0 && n <= PN && n_rows > 0 && n_rows <= PM, "%s: need 0 < n <= 16 and 0 < rows <= 64 (got %d, %d)", who, n, n_rows);
    // fmax / fmin drop NaNs: a non-finite number would pass the kernel's first test as "already inside"
    for (int i = 0; i < n_rows * n; ++i) SRH_REQUIRE(std::isfinite(A[i]), "%s: the polyhedron is not finite (A, row %d)", who, i / n);
    for (int i = 0; i < n_rows; ++i) SRH_REQUIRE(std::isfinite(b[i]), "%s: the polyhedron is not finite (b, row %d)", who, i);
    for (int64_t i = 0; strict && i < batch * n; ++i)
        if (!std::isfinite(X[i])) {
            srh::set_error("%s: point %lld is not finite (coordinate %d is NaN or Inf)", who, (long long)(i / n), (int)(i % n));
            return SRH_ENUMERIC;
        }
    if (batch == 0) return SRH_OK;
    srh::DevBuf dA, db, dX, dO, dS;
    int rc;
    if ((rc = dA.upload(A, sizeof(double) * n_rows * n)) || (rc = db.upload(b, sizeof(double) * n_rows)) ||
        (rc = dX.upload(X, sizeof(double) * batch * n)) || (rc = dO.alloc(sizeof(double) * batch * n)) ||
        (rc = dS.alloc(sizeof(int) * batch)))
        return rc;
    PolyArgs a{dA.as<double>(), db.as<double>(), dX.as<double>(), dO.as<double>(), strict ? nullptr : dS.as<int>(),
               strict ? dS.as<int>() : nullptr, n_rows, n, poly::MAX_ITER};
    poly_project_kernel<<<(unsigned)batch, 64>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    std::vector<int> st((size_t)batch);
    if ((rc = dS.download(st.data(), sizeof(int) * batch))) return rc;
    for (int64_t i = 0; i < batch; ++i) {
        if (strict && st[i] < 0) {
            srh::set_error("%s: point %lld: %s", who, (long long)i,
                           st[i] == poly::NO_CERTIFICATE ? "no certified projection in 60 iterations (empty polyhedron?)"
                                                         : "normal matrix not positive definite: the iteration diverged (empty polyhedron?)");
            return SRH_ENUMERIC;
        }
        if (words) words[i] = st[i];
    }
    return dO.download(out, sizeof(double) * batch * n);
}

}  // namespace

extern "C" {

int spoly_project(const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out) {
    SRH_REQUIRE(A && b && X && out, "spoly_project: null argument");
    return poly_run("spoly_project", A, b, n_rows, n, X, batch, out, nullptr, true);
}

int spoly_project_status(const double *A, const double *b, int n_rows, int n, const double *X, int64_t batch, double *out, int32_t *status) {
    SRH_REQUIRE(A && b && X && out && status, "spoly_project_status: null argument");
    return poly_run("spoly_project_status", A, b, n_rows, n, X, batch, out, status, false);
}

}  // extern "C"
