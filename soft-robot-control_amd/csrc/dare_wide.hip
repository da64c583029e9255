// DARE by structure-preserving doubling for a wide input block: 1 <= n_u <= 64 (sric_dare stops at 16).
// reference: sofacontrol/baselines/rompc/observer.py:27 -- the Luenberger gain is dare(A_d^T, C^T, Q, R), whose "input"
// dimension is the measurement dimension (30 with the Diamond drivers' MeasurementModel of five nodes).
// The doubling loop is the arithmetic of dare_sda_kernel (lqr.hip; it only sees n x n matrices):
//   G = B R^-1 B^T, H = Q;   W = I + G H,  [V1 V2] = W^-1 [A G];   A <- A V1,  G <- G + A V2 A^T,  H <- H + A^T (H V1)
// What differs is everything that is m wide: R and R + B^T P B (up to 64 x 64) are factored by the whole workgroup in LDS
// (right-looking Cholesky, one column per trip), the m x n solves run in place on an LDS block, one column per thread, and the
// final gain keeps only m x m + 2 m n doubles in LDS (P and P A sit in the n x n slots, wherever those are).
#include "common.h"
#include "dev_la.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr int DW_NT = 512;
constexpr int DW_MAX_M = 64;

// C (M x N) = op(A) op(B), row-major, generic pointers (the n x n slots are LDS or HBM).  Ends with __syncthreads().
template <bool TA, bool TB>
__device__ inline void dw_mm(double *C, int ldc, const double *A, int lda, const double *B, int ldb, int M, int N, int K) {
    for (int e = SRH_TID; e < M * N; e += blockDim.x) {
        const int i = e / N, j = e - i * N;
        double acc = 0.0;
        int k = 0;
        for (; k + 8 <= K; k += 8) {
            double av[8], bv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                av[q] = TA ? A[(k + q) * lda + i] : A[i * lda + k + q];
                bv[q] = TB ? B[j * ldb + k + q] : B[(k + q) * ldb + j];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = fma(av[q], bv[q], acc);
        }
        for (; k < K; ++k) acc = fma(TA ? A[k * lda + i] : A[i * lda + k], TB ? B[j * ldb + k] : B[k * ldb + j], acc);
        C[i * ldc + j] = acc;
    }
    __syncthreads();
}

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

// LDS tail behind the slots: S (m x m), two m x n blocks, the Gauss-Jordan rows, reduction scratch, flags
__host__ __device__ inline size_t dw_tail_doubles(int n, int m) { return (size_t)m * m + 2 * (size_t)m * n + 7 * (size_t)n + 16 + 8; }

__global__ __launch_bounds__(DW_NT) void dare_wide_kernel(const double *A, const double *B, int n, int m, const double *Q,
                                                           const double *R, double tol, int max_iter, double *work, int lds_slots,
                                                           double *Lout, double *Pout, int *iters, int *status) {
    extern __shared__ __attribute__((aligned(16))) char dw_smem[];
    const size_t p = blockIdx.x;
    const int ld = n | 1, tid = SRH_TID, nt = blockDim.x;
    const size_t nn = (size_t)n * ld;
    double *wk = work + p * (7 * nn);
    double *gA = wk, *gG = wk + nn;
    double *sm = (double *)dw_smem;
    double *S1, *S2, *S3, *S4, *S5;
    lptr tail;
    if (lds_slots) {
        S1 = sm; S2 = sm + nn; S3 = sm + 2 * nn; S4 = sm + 3 * nn; S5 = sm + 4 * nn;
        tail = (lptr)dw_smem + 5 * nn;
    } else {
        S1 = wk + 2 * nn; S2 = wk + 3 * nn; S3 = wk + 4 * nn; S4 = wk + 5 * nn; S5 = wk + 6 * nn;
        tail = (lptr)dw_smem;
    }
    lptr Sm, Bt, Yn, fcol, prow, jrow, red;
    liptr flag, ipiv;
    {
        lptr q = tail;
        auto take = [&](size_t c) { lptr r0 = q; q += c; return r0; };
        Sm = take((size_t)m * m); Bt = take((size_t)m * n); Yn = take((size_t)m * n);
        fcol = take(n); prow = take(3 * (size_t)n); jrow = take(3 * (size_t)n); red = take(16);
        flag = (liptr)take(4); ipiv = (liptr)take(4);
    }
    const double *Ag = A + p * n * n, *Bg = B + p * n * m;
    int st = 0, it = 0;

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
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            double g = 0.0;
            for (int a = 0; a < m; ++a) g = fma(-Bt[a * n + r], Yn[a * n + c], g);
            S3[r * ld + c] = g; gG[r * ld + c] = g;
            const double av = Ag[e];
            S2[r * ld + c] = av; gA[r * ld + c] = av;
            S4[r * ld + c] = Q[e];
        }
        __syncthreads();
    }
    while (st == 0 && it < max_iter) {
        // W = I + G H
        dw_mm<false, false>(S1, ld, S3, ld, S4, ld, n, n, n);
        for (int e = tid; e < n; e += nt) S1[e * ld + e] += 1.0;
        __syncthreads();
        // [V1 V2] = W^-1 [A G]: Gauss-Jordan with partial pivoting (physical row swaps) on [S1 | S2 | S3]
        for (int j = 0; j < n && st == 0; ++j) {
            if (tid < 64) {
                double best = -1.0;
                int bi = j;
                for (int i = j + tid; i < n; i += 64) {
                    const double v = fabs(S1[i * ld + j]);
                    if (v > best) { best = v; bi = i; }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                if (tid == 0) { ipiv[0] = bi; ipiv[1] = (best > 1e-300 && best < 1e300) ? 1 : 0; }
            }
            __syncthreads();
            const int pv = ipiv[0];
            if (ipiv[1] == 0) { st = 3; break; }
            for (int c = tid; c < 3 * n; c += nt) {
                double *blk = c < n ? S1 : (c < 2 * n ? S2 : S3);
                const int cc = c < n ? c : (c < 2 * n ? c - n : c - 2 * n);
                prow[c] = blk[pv * ld + cc];
                jrow[c] = blk[j * ld + cc];
            }
            for (int i = tid; i < n; i += nt) fcol[i] = S1[(i == pv ? j : i) * ld + j];
            __syncthreads();
            const double rp = 1.0 / prow[j];
            for (int e = tid; e < 3 * n * n; e += nt) {
                const int i = e / (3 * n), c = e - i * 3 * n;
                double *blk = c < n ? S1 : (c < 2 * n ? S2 : S3);
                const int cc = c < n ? c : (c < 2 * n ? c - n : c - 2 * n);
                const double pr = prow[c] * rp;
                double v;
                if (i == j) v = pr;
                else {
                    const double src = (i == pv) ? jrow[c] : blk[i * ld + cc];
                    v = fma(-fcol[i], pr, src);
                }
                blk[i * ld + cc] = v;
            }
            __syncthreads();
        }
        if (st != 0) break;
        dw_mm<false, false>(S5, ld, gA, ld, S2, ld, n, n, n);            // A_next = A V1
        dw_mm<false, false>(S1, ld, gA, ld, S3, ld, n, n, n);            // T2 = A V2
        dw_mm<false, true>(S3, ld, S1, ld, gA, ld, n, n, n);             // T2 A^T  (V2 is dead)
        for (int e = tid; e < n * n; e += nt) { const int r = e / n, c = e - r * n; S3[r * ld + c] += gG[r * ld + c]; }
        dw_mm<false, false>(S1, ld, S4, ld, S2, ld, n, n, n);            // T3 = H V1
        dw_mm<true, false>(S2, ld, gA, ld, S1, ld, n, n, n);             // A^T T3  (V1 is dead)
        double dmax = 0.0, hmax = 0.0;
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            const double d = S2[r * ld + c], h = S4[r * ld + c] + d;
            S4[r * ld + c] = h;
            dmax = fmax(dmax, fabs(d)); hmax = fmax(hmax, fabs(h));
            const double an = S5[r * ld + c];
            S2[r * ld + c] = an; gA[r * ld + c] = an;
            gG[r * ld + c] = S3[r * ld + c];
        }
        dmax = wg::reduce(dmax, 1, red);
        hmax = wg::reduce(hmax, 1, red);
        __syncthreads();
        ++it;
        if (!(dmax == dmax) || !(hmax < 1e300)) { st = 3; break; }
        if (dmax <= tol * hmax) break;
    }
    if (st == 0 && it >= max_iter) st = 1;
    for (int e = tid; e < n * n; e += nt) { const int r = e / n, c = e - r * n; Pout[p * n * n + e] = S4[r * ld + c]; }
    __syncthreads();
    // ---- gain K = -(R + B^T P B)^-1 B^T P A from the converged P (S4): P A -> S1, P B -> Bt's block (as n x m),
    // R + B^T P B -> Sm, B^T P A -> Yn, solved in place
    if (st != 2) {
        lptr PB = Bt;
        dw_mm<false, false>(S1, ld, S4, ld, Ag, n, n, n, n);
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
    const int ld = n_x | 1;
    const size_t nn = (size_t)n_x * ld;
    const size_t tail = dw_tail_doubles(n_x, n_u) * sizeof(double);
    SRH_REQUIRE(tail <= 160 * 1024, "sric_dare_wide: state dimension too large for LDS");
    srh::DevBuf dA, dB, dQ, dR, dL, dP, dI, dS, dW;
    int rc;
    if ((rc = dA.upload(A, sizeof(double) * batch * n_x * n_x)) || (rc = dB.upload(B, sizeof(double) * batch * n_x * n_u)) ||
        (rc = dQ.upload(Q, sizeof(double) * n_x * n_x)) || (rc = dR.upload(R, sizeof(double) * n_u * n_u)) ||
        (rc = dL.alloc(sizeof(double) * batch * n_u * n_x)) || (rc = dP.alloc(sizeof(double) * batch * n_x * n_x)) ||
        (rc = dI.alloc(sizeof(int32_t) * batch)) || (rc = dS.alloc(sizeof(int32_t) * batch)) ||
        (rc = dW.alloc(sizeof(double) * batch * 7 * nn)))
        return rc;
    const int lds_slots = (5 * nn * sizeof(double) + tail <= 160 * 1024 && !getenv("SRH_DARE_HBM_SLOTS")) ? 1 : 0;
    const size_t lds = srh::lds_request((lds_slots ? 5 * nn * sizeof(double) : 0) + tail);
    SRH_CHECK_HIP(hipFuncSetAttribute((const void *)dare_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dare_wide_kernel<<<(unsigned)batch, DW_NT, lds>>>(dA.as<double>(), dB.as<double>(), n_x, n_u, dQ.as<double>(), dR.as<double>(),
                                                      tol, max_iter, dW.as<double>(), lds_slots, dL.as<double>(), dP.as<double>(),
                                                      dI.as<int>(), dS.as<int>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    std::vector<int32_t> st((size_t)batch);
    if ((rc = dS.download(st.data(), sizeof(int32_t) * batch))) return rc;
    for (int64_t i = 0; i < batch; ++i)
        if (st[i] != 0) {
            srh::set_error("sric_dare_wide: problem %lld: %s", (long long)i,
                           st[i] == 1 ? "no convergence within max_iter doubling steps"
                                      : (st[i] == 2 ? "R or R + B^T P B is not positive definite" : "singular I + G H (not stabilisable / detectable?)"));
            return SRH_ENUMERIC;
        }
    if ((rc = dL.download(L, sizeof(double) * batch * n_u * n_x)) || (rc = dP.download(P, sizeof(double) * batch * n_x * n_x))) return rc;
    if (iters) return dI.download(iters, sizeof(int32_t) * batch);
    return SRH_OK;
}

}  // extern "C"
