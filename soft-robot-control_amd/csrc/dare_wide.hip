// DARE by structure-preserving doubling for a wide input block: 1 <= n_u <= 64 (sric_dare stops at 16).
// reference: sofacontrol/baselines/rompc/observer.py:27 -- the Luenberger gain is dare(A_d^T, C^T, Q, R), whose "input"
// dimension is the measurement dimension (30 with the Diamond drivers' MeasurementModel of five nodes).
// The doubling loop only sees n x n matrices and is dare_sda_kernel's (lqr.hip), stated once in dare_sda.h.
// This kernel's own is everything that is m wide: R and R + B^T P B (up to 64 x 64) are factored by the whole workgroup in LDS
// (right-looking Cholesky, one column per trip), the m x n solves run in place on an LDS block, one column per thread, and the
// final gain keeps only m x m + 2 m n doubles in LDS (P and P A sit in the n x n slots, wherever those are).
#include "dare_sda.h"

namespace {

constexpr int DW_NT = 512;
constexpr int DW_MAX_M = 64;

// In-place lower Cholesky factor of S (m x m, LDS, row-major; the strict upper triangle is left as it was) by the whole
// workgroup.  false (to every thread) when a pivot is not positive.  Ends synchronised.
__device__ inline bool dw_chol(lptr S, int m, liptr flag) {
    const int tid = SRH_TID, nt = blockDim.x;
    if (tid == 0) *flag = 1;
    __syncthreads();
    for (int j = 0; j < m; ++j) {
        const double piv = S[j * m + j];
        if (!(piv > 0.0) || !(piv < 1e300)) {      // uniform: every thread reads the same LDS word
            if (tid == 0) *flag = 0;
            break;
        }
        const double rd = 1.0 / sqrt(piv);
        __syncthreads();
        for (int i = j + tid; i < m; i += nt) S[i * m + j] = (i == j) ? sqrt(piv) : S[i * m + j] * rd;
        __syncthreads();
        const int w = m - j - 1;
        for (int e = tid; e < w * w; e += nt) {
            const int i = j + 1 + e / w, k = j + 1 + e % w;
            if (k <= i) S[i * m + k] = fma(-S[i * m + j], S[k * m + j], S[i * m + k]);
        }
        __syncthreads();
    }
    __syncthreads();
    return *flag != 0;
}

// X <- -(L L^T)^-1 X in place for the n columns of X (m x n, LDS), one column per thread.  Ends synchronised.
__device__ inline void dw_solve_neg(clptr L, int m, lptr X, int n) {
    for (int j = SRH_TID; j < n; j += blockDim.x) {
        for (int i = 0; i < m; ++i) {
            double s = X[i * n + j];
            for (int k = 0; k < i; ++k) s = fma(-L[i * m + k], X[k * n + j], s);
            X[i * n + j] = s / L[i * m + i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double s = X[i * n + j];
            for (int k = i + 1; k < m; ++k) s = fma(-L[k * m + i], X[k * n + j], s);
            X[i * n + j] = s / L[i * m + i];
        }
        for (int i = 0; i < m; ++i) X[i * n + j] = -X[i * n + j];
    }
    __syncthreads();
}

// LDS tail behind the slots: S (m x m) and two m x n blocks, then the rows of sda::Rows
__host__ __device__ inline size_t dw_tail_doubles(int n, int m) { return (size_t)m * m + 2 * (size_t)m * n + sda::rows_doubles(n); }

__global__ __launch_bounds__(DW_NT) void dare_wide_kernel(const double *A, const double *B, int n, int m, const double *Q,
                                                           const double *R, double tol, int max_iter, double *work, int lds_slots,
                                                           double *Lout, double *Pout, int *iters, int *status) {
    extern __shared__ __attribute__((aligned(16))) char dw_smem[];
    const size_t p = blockIdx.x;
    const int tid = SRH_TID, nt = blockDim.x;
    sda::Slots S;
    sda::Rows T;
    const lptr Sm = sda::carve_slots(S, dw_smem, work, p, n, lds_slots), Bt = Sm + (size_t)m * m, Yn = Bt + (size_t)m * n;
    sda::carve_rows(T, Yn + (size_t)m * n, n);
    double *const S1 = S.S1, *const S4 = S.S4;
    const int ld = S.ld;
    const liptr flag = T.flag;
    const double *Ag = A + p * n * n, *Bg = B + p * n * m;
    int st = 0;

    // ---- G0 = B R^-1 B^T, H0 = Q, A0 = A
    for (int e = tid; e < m * m; e += nt) Sm[e] = R[e];
    for (int e = tid; e < m * n; e += nt) {
        const double b = Bg[(e % n) * m + e / n];
        Bt[e] = b; Yn[e] = b;
    }
    __syncthreads();
    if (!dw_chol(Sm, m, flag)) st = 2;
    if (st == 0) {
        dw_solve_neg(Sm, m, Yn, n);                       // Yn = -R^-1 B^T
        sda::start(S, (cgptr)Ag, (cgptr)Q, Bt, Yn, n, m);
    }
    const sda::Result res = sda::iterate(S, T, n, tol, max_iter, st, Pout + p * n * n);
    st = res.st;
    const int it = res.it;
    // ---- gain K = -(R + B^T P B)^-1 B^T P A from the converged P (S4): P A -> S1, P B -> Bt's block (as n x m),
    // R + B^T P B -> Sm, B^T P A -> Yn, solved in place
    if (st != 2) {
        lptr PB = Bt;
        sda::mm<false, false>(S1, ld, S4, ld, Ag, n, n, n, n);
        for (int e = tid; e < n * m; e += nt) {
            const int r = e / m, a = e - r * m;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = fma(S4[r * ld + k], Bg[k * m + a], acc);
            PB[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < m * m; e += nt) {
            const int a = e / m, b = e - a * m;
            double acc = R[e];
            for (int k = 0; k < n; ++k) acc = fma(Bg[k * m + a], PB[k * m + b], acc);
            Sm[e] = acc;
        }
        for (int e = tid; e < m * n; e += nt) {
            const int a = e / n, c = e - a * n;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = fma(Bg[k * m + a], S1[k * ld + c], acc);
            Yn[e] = acc;
        }
        __syncthreads();
        if (!dw_chol(Sm, m, flag)) { if (st == 0) st = 2; }
        else {
            dw_solve_neg(Sm, m, Yn, n);
            for (int e = tid; e < m * n; e += nt) Lout[p * m * n + e] = Yn[e];
        }
    }
    if (tid == 0) { if (iters) iters[p] = it; status[p] = st; }
}

}  // namespace

extern "C" {

int sric_dare_wide(const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R,
                   double tol, int max_iter, double *L, double *P, int32_t *iters) {
    SRH_REQUIRE(A && B && Q && R && L && P, "sric_dare_wide: null argument");
    SRH_REQUIRE(batch > 0 && n_x > 0 && n_u > 0 && n_u <= DW_MAX_M, "sric_dare_wide: bad dimensions (need 1 <= n_u <= %d)", DW_MAX_M);
    const size_t tail = dw_tail_doubles(n_x, n_u) * sizeof(double);
    SRH_REQUIRE(tail <= 160 * 1024, "sric_dare_wide: state dimension too large for LDS");
    return sda::run(sda::Launch("sric_dare_wide", dare_wide_kernel, DW_NT, tail, 0), A, B, batch, n_x, n_u, Q, R, tol, max_iter, L, P, iters);
}

}  // extern "C"
