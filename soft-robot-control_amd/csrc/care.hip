// Continuous-time algebraic Riccati equation on the device: A^T X + X A - X G X + H = 0, G = B R^-1 B^T, H = Q; K = -R^-1 B^T X.
// reference: sofacontrol/lqr/lqr.py:57-64 (CLQR: control.lqr, i.e. slycot's continuous Riccati solver), tpwl/controllers.py:440-444.
// A Cayley transform of the Hamiltonian with a shift gamma > 0 (Chu, Fan, Lin 2005) turns the equation into the fixed point of the
// structure-preserving doubling loop of the DARE kernels (dare_sda.h), which is called unchanged:
//   A_g = A - gamma I,   [T1 | Ainv] = A_g^-1 [G | I],   W = A_g^T + H T1,   [Hs | Winv] = W^-1 [H Ainv | I]
//   E0 = I + 2 gamma Winv^T,   G0 = 2 gamma T1 Winv,   H0 = 2 gamma Hs           (W^T = A_g + G A_g^-T H)
// Both tableaus are three n x n blocks wide and go through sda::eliminate, the elimination of the loop's own [W | A | G].
// gamma = 1.5 max(||A||_inf, 1e-3): any gamma > ||A||_inf >= rho(A) makes A_g non-singular (a factor of exactly 1 does not: n = 1,
// A > 0 gives A_g = 0); the floor serves A = 0.  E_k = E0^(2^k) tends to zero exactly when the closed loop is stable, and
// ||E_k||_inf >= rho(E_k): a converged problem with ||E_k||_inf >= 1 is reported as not converged, so no fixed point that is not
// stabilising is ever returned as a result.  That guard cannot see a closed-loop mode ON the imaginary axis (A = 0, B = [0; 1]): its
// eigenvalue of E0 is -1 in exact arithmetic and 2 gamma fl(-1 / gamma) + 1 = -1 + O(2^-53) here, so E_k stays at modulus 1 for some
// fifty steps and then decays (or grows) after all, and the loop converges to the huge solution of a problem perturbed by rounding.
// Convergence at step k means rho(E0) ~ 1 - 16 / 2^k; past CARE_STEP_CAP = 48 steps that distance (a stability margin below
// gamma 2^-45) is within a few hundred roundings of E0 and says nothing: the loop is given min(max_iter, 48) steps, and a legitimate
// problem needs 6 to 18.
// One workgroup per (A, B) pair, Q and R shared; thread count, slot carve and LDS tail as dare_sda_kernel (lqr.hip).
#include "dare_sda.h"

namespace {

constexpr int CARE_NT = 512;
constexpr int CARE_STEP_CAP = 48;

// m-wide head of the LDS tail behind the slots: R (m x m, m <= 16) and its Cholesky factor in 256 doubles each, B^T and -R^-1 B^T
// (m x n); then the rows of sda::Rows
__host__ __device__ inline size_t care_tail_doubles(int n, int m) { return 512 + 2 * (size_t)m * n + sda::rows_doubles(n); }

// max over the rows of sum_c |M[r][c]| (n x n, row stride ld), to every thread; +inf if a row sum is not finite
template <typename MP>
__device__ __forceinline__ double norm_inf(MP M, int ld, int n, lptr red) {
    double rs = 0.0;
    for (int r = SRH_TID; r < n; r += blockDim.x) {
        double s = 0.0;
        for (int c = 0; c < n; ++c) s += fabs(M[r * ld + c]);
        rs = s < 1e300 ? fmax(rs, s) : __builtin_inf();
    }
    return wg::reduce(rs, 1, red);
}

__global__ __launch_bounds__(CARE_NT) void care_sda_kernel(const double *A, const double *B, int n, int m, const double *Q,
                                                           const double *R, double tol, int max_iter, double *work,
                                                           int lds_slots, double *Kout, double *Pout, int *iters,
                                                           int *status) {
    extern __shared__ __attribute__((aligned(16))) char care_smem[];
    const size_t p = blockIdx.x;
    const int tid = SRH_TID, nt = blockDim.x;
    sda::Slots S;
    sda::Rows T;
    const lptr Rq = sda::carve_slots(S, care_smem, work, p, n, lds_slots), Lc = Rq + 256, Bt = Lc + 256, Yn = Bt + (size_t)m * n;
    sda::carve_rows(T, Yn + (size_t)m * n, n);
    double *const S1 = S.S1, *const S2 = S.S2, *const S3 = S.S3, *const S4 = S.S4, *const S5 = S.S5;
    const int ld = S.ld;
    cgptr Ag = (cgptr)A + p * n * n, Bg = (cgptr)B + p * n * m, Qg = (cgptr)Q, Rg = (cgptr)R;
    int st = 0;

    // ---- Yn = -R^-1 B^T
    for (int e = tid; e < m * m; e += nt) Rq[e] = Rg[e];
    for (int e = tid; e < m * n; e += nt) Bt[e] = Bg[(e % n) * m + e / n];
    __syncthreads();
    if (!wg::chol_factor(Rq, Lc, m, T.flag, false)) st = 2;
    double gam = 0.0;
    if (st == 0) {
        for (int j = tid; j < n; j += nt) wg::chol_solve_neg(Lc, m, Bt + j, n, Yn + j, n);
        gam = 1.5 * fmax(norm_inf(Ag, n, n, T.red), 1e-3);
        if (!(gam < 1e300)) st = 3;
    }
    // ---- Cayley start: [T1 | Ainv] = A_g^-1 [G | I] on [S1 | S2 | S3]
    if (st == 0) {
        __syncthreads();
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            double g = 0.0;
            for (int a = 0; a < m; ++a) g = fma(-Bt[a * n + r], Yn[a * n + c], g);
            S2[r * ld + c] = g;
            S1[r * ld + c] = Ag[e] - (r == c ? gam : 0.0);
            S3[r * ld + c] = r == c ? 1.0 : 0.0;
        }
        __syncthreads();
        if (!sda::eliminate(S1, S2, S3, T, n, ld)) st = 3;
    }
    // W = A_g^T + H T1 -> S1, H Ainv -> S4;  [Hs | Winv] = W^-1 [H Ainv | I] on [S1 | S4 | S3]  (T1 stays in S2)
    if (st == 0) {
        sda::mm<false, false>(S4, ld, Qg, n, S3, ld, n, n, n);
        sda::mm<false, false>(S1, ld, Qg, n, S2, ld, n, n, n);
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            S1[r * ld + c] += Ag[c * n + r] - (r == c ? gam : 0.0);
            S3[r * ld + c] = r == c ? 1.0 : 0.0;
        }
        __syncthreads();
        if (!sda::eliminate(S1, S4, S3, T, n, ld)) st = 3;
    }
    // E0 = I + 2 gamma Winv^T -> S2 / gA,  G0 = 2 gamma T1 Winv -> S3 / gG,  H0 = 2 gamma Hs -> S4: where sda::iterate expects them
    if (st == 0) {
        const double g2 = 2.0 * gam;
        sda::mm<false, false>(S5, ld, S2, ld, S3, ld, n, n, n);
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            const double e0 = fma(g2, S3[c * ld + r], r == c ? 1.0 : 0.0);
            S2[r * ld + c] = e0; S.gA[r * ld + c] = e0;
            S4[r * ld + c] *= g2;
        }
        __syncthreads();                                  // every read of Winv^T is done before G0 takes its slot
        for (int e = tid; e < n * n; e += nt) {
            const int r = e / n, c = e - r * n;
            const double g0 = g2 * S5[r * ld + c];
            S3[r * ld + c] = g0; S.gG[r * ld + c] = g0;
        }
        __syncthreads();
    }
    const sda::Result res = sda::iterate(S, T, n, tol, max_iter < CARE_STEP_CAP ? max_iter : CARE_STEP_CAP, st, Pout + p * n * n);
    st = res.st;
    // ---- converged: the fixed point is the stabilising one only if E_k (S2) has gone to zero
    if (st == 0) {
        if (!(norm_inf(S2, ld, n, T.red) < 1.0)) st = 1;
    }
    // ---- gain K = -R^-1 B^T P = Yn P (m x n), P in S4
    if (st == 0) {
        for (int e = tid; e < m * n; e += nt) {
            const int a = e / n, c = e - a * n;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = fma(Yn[a * n + k], S4[k * ld + c], acc);
            Kout[p * m * n + e] = acc;
        }
    }
    if (tid == 0) { if (iters) iters[p] = res.it; status[p] = st; }
}

}  // namespace

extern "C" {

int sric_care(const double *A, const double *B, int64_t batch, int n_x, int n_u, const double *Q, const double *R, double tol,
              int max_iter, double *K, double *P, int32_t *iters) {
    SRH_REQUIRE(A && B && Q && R && K && P, "sric_care: null argument");
    SRH_REQUIRE(batch > 0 && n_x > 0 && n_u > 0 && n_u <= 16, "sric_care: bad dimensions");
    const size_t tail = care_tail_doubles(n_x, n_u) * sizeof(double);
    SRH_REQUIRE(tail <= 160 * 1024, "sric_care: state dimension too large for LDS");
    sda::Launch k("sric_care", care_sda_kernel, CARE_NT, tail, 0);
    k.stalled = "no convergence to a stabilising solution within min(max_iter, 48) doubling steps (not stabilisable / detectable?)";
    k.not_pd = "R is not positive definite";
    k.singular = "singular A - gamma I, A_gamma^T + Q A_gamma^-1 G or I + G H, or a value that is not finite (not stabilisable / detectable?)";
    return sda::run(k, A, B, batch, n_x, n_u, Q, R, tol, max_iter, K, P, iters);
}

}  // extern "C"
