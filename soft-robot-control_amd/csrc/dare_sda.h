// DARE by structure-preserving doubling, the part dare_sda_kernel (lqr.hip, n_u <= 16) and dare_wide_kernel (dare_wide.hip,
// n_u <= 64) share, stated ONCE: the doubling loop only sees n x n matrices, so nothing in it depends on how wide the input block is.
//   G = B R^-1 B^T, H = Q;   W = I + G H,  [V1 V2] = W^-1 [A G]
//   A <- A V1,   G <- G + A V2 A^T,   H <- H + A^T (H V1)            ->   H converges quadratically to P
// Here: the product routine `mm`, the carve of the five n x n slots and of the Gauss-Jordan rows behind each kernel's own m-wide
// head, the G0 / A0 / H0 fill, the pivoted elimination on a three-block tableau, the iteration from its `while` to the write-out of
// P, and the host launcher of the three DARE entry points (sric_dare, sric_dare_wide, sric_dare_fixed_point).  What is m wide stays
// in the kernels: the factor of R, the m x n solve and the gain phase with its status handling.
// care_sda_kernel (care.hip, sric_care) brings the continuous equation to the same loop by a Cayley transform: its start phase runs
// `eliminate` twice and then calls `iterate` and `run` as the DARE kernels do.
// The operation order and grouping of every expression is what the kernels' results depend on bit for bit: keep it.
#pragma once
#include "common.h"
#include "dev_la.h"

#include <algorithm>
#include <cstdlib>

namespace sda {

// ---- tiny dense helpers (row-major, any address space, runtime sizes; one output per thread-iteration)
// C (M x N) = op(A) * op(B) ; op = transpose flag.  Ends with __syncthreads().
template <bool TA, bool TB, typename CP, typename AP, typename BP>
__device__ inline void mm(CP C, int ldc, AP A, int lda, BP B, int ldb, int M, int N, int K) {
    for (int e = SRH_TID; e < M * N; e += blockDim.x) {
        const int i = e / N, j = e - i * N;
        double acc = 0.0;
        int k = 0;
        // 8 independent operand pairs in flight per trip: with one or two waves per SIMD the dependent
        // load -> fma chain of a rolled loop is bound by the LDS / L2 latency of every single k
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
        for (; k < K; ++k) {
            const double a = TA ? A[k * lda + i] : A[i * lda + k];
            const double b = TB ? B[j * ldb + k] : B[k * ldb + j];
            acc = fma(a, b, acc);
        }
        C[i * ldc + j] = acc;
    }
    __syncthreads();
}

// Five n x n slots (row stride ld = n | 1) in LDS when they fit (lds_slots), else in the per-problem HBM workspace, next to the
// copies of A_k, G_k that the products read through L2.  The workspace is 7 nn doubles per problem either way.
struct Slots {
    double *S1, *S2, *S3, *S4, *S5;     // W / scratch, A -> V1, G -> V2, H, A_next
    double *gA, *gG;                    // A_k, G_k
    int ld;
    size_t nn;
};

// Returns where the LDS tail behind the slots begins.
__device__ __forceinline__ lptr carve_slots(Slots &s, char *smem, double *work, size_t p, int n, int lds_slots) {
    s.ld = n | 1;
    s.nn = (size_t)n * s.ld;
    const size_t nn = s.nn;
    double *wk = work + p * (7 * nn);
    s.gA = wk; s.gG = wk + nn;
    double *sm = (double *)smem;
    if (lds_slots) {
        s.S1 = sm; s.S2 = sm + nn; s.S3 = sm + 2 * nn; s.S4 = sm + 3 * nn; s.S5 = sm + 4 * nn;
        return (lptr)smem + 5 * nn;
    }
    s.S1 = wk + 2 * nn; s.S2 = wk + 3 * nn; s.S3 = wk + 4 * nn; s.S4 = wk + 5 * nn; s.S5 = wk + 6 * nn;
    return (lptr)smem;
}

// The part of the tail both kernels lay out alike, behind each kernel's own m-wide head
struct Rows {
    lptr fcol, prow, jrow;   // Gauss-Jordan: multipliers (n), pivot row (3n), old row j (3n)
    lptr red;
    liptr flag, ipiv;
};

__host__ __device__ inline size_t rows_doubles(int n) { return 7 * (size_t)n + 16 + 8; }

__device__ __forceinline__ void carve_rows(Rows &T, lptr q, int n) {
    auto take = [&](size_t c) { lptr r0 = q; q += c; return r0; };
    T.fcol = take(n); T.prow = take(3 * (size_t)n); T.jrow = take(3 * (size_t)n); T.red = take(16);
    T.flag = (liptr)take(4); T.ipiv = (liptr)take(4);
}

// G0 = B R^-1 B^T from Bt = B^T and Yn = -R^-1 B^T (both m x n), A0 = A, H0 = Q.  Ends synchronised.
__device__ __forceinline__ void start(const Slots &s, cgptr Ag, cgptr Qg, clptr Bt, clptr Yn, int n, int m) {
    const int ld = s.ld, tid = SRH_TID, nt = blockDim.x;
    for (int e = tid; e < n * n; e += nt) {
        const int r = e / n, c = e - r * n;
        double g = 0.0;
        for (int a = 0; a < m; ++a) g = fma(-Bt[a * n + r], Yn[a * n + c], g);
        s.S3[r * ld + c] = g; s.gG[r * ld + c] = g;
        const double av = Ag[e];
        s.S2[r * ld + c] = av; s.gA[r * ld + c] = av;
        s.S4[r * ld + c] = Qg[e];
    }
    __syncthreads();
}

// [S2 S3] <- S1^-1 [S2 S3] (and S1 <- I): Gauss-Jordan elimination with partial pivoting (physical row swaps) on the tableau
// [S1 | S2 | S3] of three n x n blocks -- [W | A | G] in `iterate`, the two tableaus of the Cayley start in care.hip.  false (to every
// thread) at a pivot that is zero or not finite.  The blocks must be visible to the workgroup; ends synchronised.
__device__ __forceinline__ bool eliminate(double *S1, double *S2, double *S3, const Rows &T, int n, int ld) {
    const int tid = SRH_TID, nt = blockDim.x;
    for (int j = 0; j < n; ++j) {
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
            if (tid == 0) { T.ipiv[0] = bi; T.ipiv[1] = (best > 1e-300 && best < 1e300) ? 1 : 0; }
        }
        __syncthreads();
        const int pv = T.ipiv[0];
        if (T.ipiv[1] == 0) return false;
        // snapshot: pivot row (old row pv), old row j, multipliers of every row as they will sit after the swap
        for (int c = tid; c < 3 * n; c += nt) {
            double *blk = c < n ? S1 : (c < 2 * n ? S2 : S3);
            const int cc = c < n ? c : (c < 2 * n ? c - n : c - 2 * n);
            T.prow[c] = blk[pv * ld + cc];
            T.jrow[c] = blk[j * ld + cc];
        }
        for (int i = tid; i < n; i += nt) T.fcol[i] = S1[(i == pv ? j : i) * ld + j];
        __syncthreads();
        const double rp = 1.0 / T.prow[j];
        for (int e = tid; e < 3 * n * n; e += nt) {
            const int i = e / (3 * n), c = e - i * 3 * n;
            double *blk = c < n ? S1 : (c < 2 * n ? S2 : S3);
            const int cc = c < n ? c : (c < 2 * n ? c - n : c - 2 * n);
            const double pr = T.prow[c] * rp;
            double v;
            if (i == j) v = pr;
            else {
                const double src = (i == pv) ? T.jrow[c] : blk[i * ld + cc];
                v = fma(-T.fcol[i], pr, src);
            }
            blk[i * ld + cc] = v;
        }
        __syncthreads();
    }
    return true;
}

// status of a problem: 0 converged, 1 max_iter doubling steps without convergence (care.hip: or a converged fixed point that is not
// stabilising), 2 R or R + B^T P B not positive definite, 3 singular I + G H (care.hip: or A - gamma I, W of the Cayley start), or
// a value that is not finite
struct Result { int st, it; };

// The doubling steps (none if the caller's factorisation of R already failed: st != 0) and the write-out of H = P (n x n, dense)
// to Pout.  Ends synchronised.
__device__ __forceinline__ Result iterate(const Slots &s, const Rows &T, int n, double tol, int max_iter, int st, double *Pout) {
    double *const S1 = s.S1, *const S2 = s.S2, *const S3 = s.S3, *const S4 = s.S4, *const S5 = s.S5, *const gA = s.gA, *const gG = s.gG;
    const int ld = s.ld, tid = SRH_TID, nt = blockDim.x;
    int it = 0;
    while (st == 0 && it < max_iter) {
        // W = I + G H
        mm<false, false>(S1, ld, S3, ld, S4, ld, n, n, n);
        for (int e = tid; e < n; e += nt) S1[e * ld + e] += 1.0;
        __syncthreads();
        // [V1 V2] = W^-1 [A G]
        if (!eliminate(S1, S2, S3, T, n, ld)) { st = 3; break; }
        mm<false, false>(S5, ld, gA, ld, S2, ld, n, n, n);            // A_next = A V1
        mm<false, false>(S1, ld, gA, ld, S3, ld, n, n, n);            // T2 = A V2
        mm<false, true>(S3, ld, S1, ld, gA, ld, n, n, n);             // T2 A^T  (V2 is dead)
        for (int e = tid; e < n * n; e += nt) { const int r = e / n, c = e - r * n; S3[r * ld + c] += gG[r * ld + c]; }
        mm<false, false>(S1, ld, S4, ld, S2, ld, n, n, n);            // T3 = H V1
        mm<true, false>(S2, ld, gA, ld, S1, ld, n, n, n);             // A^T T3  (V1 is dead)
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
        dmax = wg::reduce(dmax, 1, T.red);
        hmax = wg::reduce(hmax, 1, T.red);
        __syncthreads();
        ++it;
        if (!(dmax == dmax) || !(hmax < 1e300)) { st = 3; break; }
        if (dmax <= tol * hmax) break;
    }
    if (st == 0 && it >= max_iter) st = 1;
    for (int e = tid; e < n * n; e += nt) { const int r = e / n, c = e - r * n; Pout[e] = S4[r * ld + c]; }
    __syncthreads();
    return Result{st, it};
}

// ---- host: what the three DARE entry points do around their kernel
// the two kernel signatures `run` can launch (its argument array is untyped: the constructors below are the type check)
using DoublingKernel = void (*)(const double *A, const double *B, int n, int m, const double *Q, const double *R, double tol, int max_iter,
                                double *work, int lds_slots, double *L, double *P, int *iters, int *status);
using FixedPointKernel = void (*)(const double *A, const double *B, int n, int m, const double *Q, const double *R, double tol,
                                  int max_iter, double *L, double *P, int *iters, int *status);

struct Launch {
    const char *name;       // the entry point, for messages
    const void *kernel;     // one workgroup per problem
    int threads;
    size_t tail_lds;        // bytes of LDS behind the five slots
    size_t min_lds;         // bytes of LDS the kernel carves whatever the slots (the gain phase's LqrLds)
    bool doubling;          // a DoublingKernel: takes the workspace and reports the doubling's statuses
    // the texts of statuses 1, 2 and 3 (sric_care sets its own after construction)
    const char *stalled = "no convergence within max_iter doubling steps";
    const char *not_pd = "R or R + B^T P B is not positive definite";
    const char *singular = "singular I + G H (not stabilisable / detectable?)";
    Launch(const char *name_, DoublingKernel k, int threads_, size_t tail_lds_, size_t min_lds_)
        : name(name_), kernel((const void *)k), threads(threads_), tail_lds(tail_lds_), min_lds(min_lds_), doubling(true) {}
    Launch(const char *name_, FixedPointKernel k, int threads_, size_t lds_)
        : name(name_), kernel((const void *)k), threads(threads_), tail_lds(0), min_lds(lds_), doubling(false),
          not_pd("R + B^T P B is not positive definite") {}
};

inline int run(const Launch &k, const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R,
               double tol, int max_iter, double *L, double *P, int32_t *iters) {
    const size_t nn = (size_t)n_x * (n_x | 1);
    srh::DevBuf dA, dB, dQ, dR, dL, dP, dI, dS, dW;
    int rc;
    if ((rc = dA.upload(A, sizeof(double) * batch * n_x * n_x)) || (rc = dB.upload(B, sizeof(double) * batch * n_x * n_u)) ||
        (rc = dQ.upload(Q, sizeof(double) * n_x * n_x)) || (rc = dR.upload(R, sizeof(double) * n_u * n_u)) ||
        (rc = dL.alloc(sizeof(double) * batch * n_u * n_x)) || (rc = dP.alloc(sizeof(double) * batch * n_x * n_x)) ||
        (rc = dI.alloc(sizeof(int32_t) * batch)) || (rc = dS.alloc(sizeof(int32_t) * batch)) ||
        (k.doubling && (rc = dW.alloc(sizeof(double) * batch * 7 * nn))))
        return rc;
    int lds_slots = (k.doubling && 5 * nn * sizeof(double) + k.tail_lds <= 160 * 1024 && !getenv("SRH_DARE_HBM_SLOTS")) ? 1 : 0;
    const size_t lds = srh::lds_request(std::max(k.min_lds, (lds_slots ? 5 * nn * sizeof(double) : 0) + k.tail_lds));
    const double *pA = dA.as<double>(), *pB = dB.as<double>(), *pQ = dQ.as<double>(), *pR = dR.as<double>();
    double *pW = dW.as<double>(), *pL = dL.as<double>(), *pP = dP.as<double>();
    int *pI = dI.as<int>(), *pS = dS.as<int>();
    void *args[] = {&pA, &pB, &n_x, &n_u, &pQ, &pR, &tol, &max_iter, &pW, &lds_slots, &pL, &pP, &pI, &pS};
    if (!k.doubling) std::copy(args + 10, args + 14, args + 8);          // the fixed point's kernel has no (work, lds_slots)
    SRH_CHECK_HIP(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SRH_CHECK_HIP(hipLaunchKernel(k.kernel, dim3((unsigned)batch), dim3(k.threads), args, lds, nullptr));
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    // a failed factorisation leaves no gain to return (fixed point: max_iter reached is not an error: the reference has none)
    std::vector<int32_t> st((size_t)batch);
    if ((rc = dS.download(st.data(), sizeof(int32_t) * batch))) return rc;
    for (int64_t i = 0; i < batch; ++i)
        if (st[i] != 0) {
            srh::set_error("%s: problem %lld: %s", k.name, (long long)i,
                           st[i] == 1 ? k.stalled
                                      : (st[i] == 2 ? k.not_pd : k.singular));
            return SRH_ENUMERIC;
        }
    if ((rc = dL.download(L, sizeof(double) * batch * n_u * n_x)) || (rc = dP.download(P, sizeof(double) * batch * n_x * n_x))) return rc;
    if (iters) return dI.download(iters, sizeof(int32_t) * batch);
    return SRH_OK;
}

}  // namespace sda
