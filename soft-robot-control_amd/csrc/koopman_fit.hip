// Koopman model identification (EDMD) on the device: records (y, u) -> the sums of the normal equations -> [A B].
//
// THE FIT (this text defines it; the reference's model was trained by an external MATLAB package that is not part of it).
//   Records: E episodes, each y (T x n_y), u (T x m), raw.  `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode (a record at
//   dt_sim read at Ts = s dt_sim; the input is held over a controller step, so row i s carries it); T' = the rows kept.
//   zeta_i = [y_i, y_{i-1} .. y_{i-d}, u_{i-1} .. u_{i-d}] of scaled samples for kept row i >= d (d = delays): what skoop_embed_lift
//   builds, a scaled sample (v - offset) / factor being rounded once here (kf_scale_down; within one ulp of the lift's).
//   psi_i = psi(zeta_i): the lift handle's observable table, the constant last unless dmd.
//   v_i = scale_down(u[i + u_lag]), u_lag in {0, 1}: 0 when row i holds the input applied AFTER y_i (the loops' res.y / res.u), 1 when
//   it holds the input applied BEFORE y_i (the rows KoopmanData.add_measurement and the device ring keep).
//   Pairs (i, i + 1) for d <= i <= T' - 2, never across an episode; an episode with T' <= d + 1 contributes nothing.
//   With Phi_i = [psi_i; v_i] (n = P + m):  G = sum Phi_i Phi_i^T (n x n),  R = sum psi_{i+1} Phi_i^T (P x n),  Q = sum |psi_{i+1}|^2,
//   S = the number of pairs.  [A B] = R (G + ridge I)^-1, ridge >= 0: the minimiser of
//   sum |psi_{i+1} - A psi_i - B v_i|^2 + ridge |[A B]|_F^2.
//   Scaling: given (the lift handle's), or from the records over the kept rows: offset = (max + min) / 2, factor = (max - min) / 2.
//   A pivot of G + ridge I that is not positive, not finite, or not above n eps of its diagonal entry: SRH_ENUMERIC, the pivot is
//   named ("increase ridge").
//   Not offered: an L1 (lasso) constraint, sample weights, non-polynomial observables, truncation (a lift handle with W is refused).
//   Limits: n = P + m <= 128 and the lift's own (nzeta <= 64, degree <= 4).
//
// Kernels.  kf_accum_kernel: a workgroup owns a run of consecutive chunks; a chunk is KF_TR consecutive pairs of one episode, i.e.
// KF_TR kept rows and a one-row halo.  The chunk's rows are scaled, embedded and lifted once into an LDS panel (row-major, Phi);
// G accumulates rows 0 .. TR-1 against themselves and R rows 1 .. TR against rows 0 .. TR-1 on v_mfma_f64_16x16x4_f64, the k index
// of the product being the panel row.  Only the tiles of G on or above the diagonal are computed.  The 16 x 16 tiles (G's, then R's)
// are dealt to the four waves and stay in registers over all the chunks of the workgroup; each workgroup then writes its partial
// sums to scratch, and kf_reduce_kernel adds the partials to the handle's running sums in block order.  The chunk map and the grid
// are functions of (E, T, stride, delays) and the model's shape alone and nothing is accumulated with atomics: the same records give
// the same bits on every run.  kf_solve_kernel: one workgroup, Cholesky of G + ridge I as a packed lower triangle in LDS, the rows
// of R solved by the waves (a row's right-hand side lives in the lanes of a wave, two entries each).
#include "koopman_host.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "dev_la.h"

namespace {

constexpr int KF_TR = 64;                 // pairs of a chunk (a multiple of 4: the k step of the MFMA)
constexpr int KF_NT = 256;                // threads of every kernel here (4 waves)
constexpr int KF_MAX_N = 128;             // n = P + m
constexpr int KF_MAX_NZ = 64, KF_MAX_DEG = 4;   // the lift's limits (koopman.hip), restated for the host-side plan
constexpr int KF_MAX_BLOCKS = 768;        // workgroups of an accumulate launch (three per CU where registers and LDS admit them)
constexpr size_t KF_SCRATCH_BYTES = (size_t)64 << 20;   // bound of the partial-sum scratch
typedef double kf_d4 __attribute__((ext_vector_type(4)));

// Shape of a fit: tiles and strides, stated once for the plan, the handle and the kernels.
struct KfShape {
    int P, m, n, nz;
    int T16;        // 16-column tiles across Phi
    int PT;         // 16-row tiles down R
    int NG;         // tiles of G on or above the diagonal; R's tiles follow them
    int ntile;
    int ld;         // row stride of the LDS panel: = 16 (mod 32) doubles, so the two rows a half-wave reads fall on different banks
    int ntw;        // tiles per wave of the kernel instance used
    int64_t len;    // doubles of one set of sums: (ntile + 1) x 256, the last block = the 256 per-thread parts of Q
    size_t lds;     // dynamic LDS of the accumulate kernel
};

KfShape kf_shape(int P, int m, int nz) {
    KfShape s{};
    s.P = P; s.m = m; s.n = P + m; s.nz = nz;
    s.T16 = (s.n + 15) / 16;
    s.PT = (P + 15) / 16;
    s.NG = s.T16 * (s.T16 + 1) / 2;
    s.ntile = s.NG + s.PT * s.T16;
    s.ld = 16 * s.T16;
    if (s.ld % 32 != 16) s.ld += 16;
    const int need = (s.ntile + 3) / 4;
    s.ntw = need <= 4 ? 4 : (need <= 10 ? 10 : (need <= 16 ? 16 : 25));
    s.len = (int64_t)(s.ntile + 1) * 256;
    // zeta tile and panel of KF_TR + 1 rows; behind them the scale vectors (ny + m <= nz + m offsets and factors) and the table (2 P ints)
    s.lds = srh::lds_request(sizeof(double) * ((size_t)(KF_TR + 1) * (size_t)(nz + s.ld) + 2 * (size_t)(nz + m) + (size_t)P));
    return s;
}

// scale_down rounded once: (v - offset) / factor with the subtraction's error (TwoSum) and the division's remainder (one fma) folded
// back, so the result is within one rounding of the exact quotient and at most one ulp from the lift's two-operation value.  A sum's
// term is a product of up to 2 degree scaled samples, and its error is led by theirs: a sample that occurs g times in a term counts g
// times.  With (0 - 0) / 1 and with offset 0, factor 1 the result is the input, as before
__device__ __forceinline__ double kf_scale_down(double v, double off, double fac) {
    const double d = v - off;
    const double t = d - v;
    const double e = (v - (d - t)) - (off + t);      // v - off = d + e exactly
    const double q = d / fac;
    return q + (fma(-q, fac, d) + e) / fac;
}

__host__ __device__ inline int kf_gtile(int ti, int tj, int T16) { return ti * T16 - ti * (ti - 1) / 2 + (tj - ti); }

struct KfAccArgs {
    const double *y, *u;          // (E x T x ny), (E x T x m), raw
    int64_t T;                    // samples of an episode
    int64_t ppe, cpe, nchunk;     // pairs and chunks of an episode, chunks of the launch
    int nblk, stride, ulag;
    int ny, m, delay, nz, P, n, ld, nlev, has_const, ntile;
    const double *yoff, *yfac, *uoff, *ufac;
    const int32_t *par, *var, *lev;
    const int32_t *tiles;         // (ntile): next-row flag << 16 | tile row << 8 | tile column
    double *part;                 // (nblk x (ntile + 1) x 256)
};

template <int NTW>
__global__ void __launch_bounds__(KF_NT) kf_accum_kernel(KfAccArgs a) {
    extern __shared__ double kf_smem[];
    const int ld = a.ld, nz = a.nz, P = a.P, n = a.n, ny = a.ny, m = a.m, delay = a.delay;
    constexpr int ROWS = KF_TR + 1;
    double *zt = kf_smem;                        // ROWS x nz
    double *ps = kf_smem + (size_t)ROWS * nz;    // ROWS x ld: [psi | v | zeros]
    // the handle's tables, staged once: a level of the recurrence then waits for LDS, not for L2, at every step
    double *soff = ps + (size_t)ROWS * ld;       // ny + m offsets [y | u]
    double *sfac = soff + ny + m;                // ny + m factors
    int *spar = reinterpret_cast<int *>(sfac + ny + m), *svar = spar + P;   // P parents, P variables
    const int tid = threadIdx.x;
    for (int e = tid; e < ny + m; e += KF_NT) {
        soff[e] = e < ny ? a.yoff[e] : a.uoff[e - ny];
        sfac[e] = e < ny ? a.yfac[e] : a.ufac[e - ny];
    }
    const int nmono = P - a.has_const;
    for (int e = tid; e < nmono; e += KF_NT) { spar[e] = a.par[e]; svar[e] = a.var[e]; }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l16 = lane & 15, kk = lane >> 4;
    // the tiles of this wave: A operand Phi[k + next][16 ti + l16], B operand Phi[k][16 tj + l16], D row kk + 4 q, column l16
    int offA[NTW], offB[NTW];
    kf_d4 acc[NTW];
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
        const int t = wave + 4 * q;
        const int code = t < a.ntile ? a.tiles[t] : 0;
        offA[q] = (code >> 16) * ld + 16 * ((code >> 8) & 255);
        offB[q] = 16 * (code & 255);
        acc[q] = kf_d4{0.0, 0.0, 0.0, 0.0};
    }
    // columns n .. ld - 1 are read by the last tile: zeros, written once (the lift writes columns < n only)
    const int padc = ld - n;
    for (int e = tid; e < ROWS * padc; e += KF_NT) {
        const int r = e / padc;
        ps[r * ld + n + (e - r * padc)] = 0.0;
    }
    double qloc = 0.0;
    const int64_t c0 = a.nchunk * blockIdx.x / a.nblk, c1 = a.nchunk * (blockIdx.x + 1) / a.nblk;
    const int yb = ny * (delay + 1);
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t ep = c / a.cpe, ci = c - ep * a.cpe;
        const int64_t i0 = delay + ci * KF_TR;                                  // kept row of panel row 0
        const int np = (int)min((int64_t)KF_TR, a.ppe - ci * KF_TR);            // pairs of this chunk: panel rows 0 .. np hold data
        const int64_t s0 = ep * a.T;
        __syncthreads();                                                        // the previous chunk's products have read the panel
        // zeta of the panel rows 0 .. np (zeros behind them), four elements per thread and pass: the loads of a pass are issued
        // together.  scale_down: (v - offset) / factor rounded once (kf_scale_down); an unused element is (0 - 0) / 1
        for (int e0 = tid; e0 < ROWS * nz; e0 += 4 * KF_NT) {
            double raw[4], of[4], fa[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * KF_NT;
                const int r = e / nz, cz = e - r * nz;
                raw[q] = 0.0; of[q] = 0.0; fa[q] = 1.0;
                if (e < ROWS * nz && r <= np) {
                    const bool isy = cz < yb;
                    const int cc = isy ? cz : cz - yb;
                    const int w = isy ? ny : m;
                    const int j = cc / w + (isy ? 0 : 1), el = cc - (cc / w) * w;
                    const int64_t s = s0 + (i0 + r - j) * a.stride;
                    raw[q] = isy ? a.y[s * ny + el] : a.u[s * m + el];
                    of[q] = soff[isy ? el : ny + el];
                    fa[q] = sfac[isy ? el : ny + el];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * KF_NT;
                if (e < ROWS * nz) zt[e] = kf_scale_down(raw[q], of[q], fa[q]);
            }
        }
        // v_i = scale_down(u[i + u_lag]) of the pair's first row; the halo row and the rows behind it carry none
        for (int e0 = tid; e0 < ROWS * m; e0 += 4 * KF_NT) {
            double raw[4], of[4], fa[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * KF_NT;
                const int r = e / m, el = e - r * m;
                raw[q] = 0.0; of[q] = 0.0; fa[q] = 1.0;
                if (e < ROWS * m && r < np) {
                    raw[q] = a.u[(s0 + (i0 + r + a.ulag) * a.stride) * m + el];
                    of[q] = soff[ny + el];
                    fa[q] = sfac[ny + el];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * KF_NT;
                if (e < ROWS * m) ps[(e / m) * ld + P + (e - (e / m) * m)] = kf_scale_down(raw[q], of[q], fa[q]);
            }
        }
        __syncthreads();
        for (int L = 0; L < a.nlev; ++L) {
            const int k0 = a.lev[L], nk = a.lev[L + 1] - k0;
            for (int e = tid; e < ROWS * nk; e += KF_NT) {
                const int r = e / nk, k = k0 + (e - r * nk);
                const int p = spar[k];
                ps[r * ld + k] = (p < 0 ? 1.0 : ps[r * ld + p]) * zt[r * nz + svar[k]];
            }
            __syncthreads();
        }
        if (a.has_const) {
            for (int r = tid; r < ROWS; r += KF_NT) ps[r * ld + P - 1] = 1.0;
            __syncthreads();
        }
        // Q: |psi|^2 of panel rows 1 .. np, a fixed share per thread
        for (int e = tid; e < np * P; e += KF_NT) {
            const int r = e / P;
            const double v = ps[(r + 1) * ld + (e - r * P)];
            qloc = fma(v, v, qloc);
        }
        const int ksteps = (np + 3) >> 2;
        for (int s = 0; s < ksteps; ++s) {
            const int r = 4 * s + kk;
            const bool live = r < np;                    // rows np .. are no pair's first row: their B operand is zero
            const double *row = ps + r * ld + l16;
#pragma unroll
            for (int q = 0; q < NTW; ++q) {
                if (wave + 4 * q < a.ntile) {
                    const double av = row[offA[q]];
                    const double bv = live ? row[offB[q]] : 0.0;
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
                }
            }
        }
    }
    double *dst = a.part + (size_t)blockIdx.x * (size_t)(a.ntile + 1) * 256;
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
        const int t = wave + 4 * q;
        if (t < a.ntile) {
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[(size_t)t * 256 + (kk + 4 * g) * 16 + l16] = acc[q][g];
        }
    }
    dst[(size_t)a.ntile * 256 + tid] = qloc;
}

// sums += the partials of the workgroups, in workgroup order
__global__ void __launch_bounds__(KF_NT) kf_reduce_kernel(const double *__restrict__ part, int nblk, int64_t len, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * KF_NT + threadIdx.x;
    if (i >= len) return;
    double v = sums[i];
    for (int b = 0; b < nblk; ++b) v += part[(int64_t)b * len + i];
    sums[i] = v;
}

// min and max of every channel of v (E x T x w) over the kept rows: one (min, max) pair per channel and workgroup
__global__ void __launch_bounds__(KF_NT) kf_minmax_kernel(const double *__restrict__ v, int64_t T, int64_t Tk, int64_t rows, int stride, int w,
                                                          int64_t rpb, double *__restrict__ part) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    for (int c = 0; c < w; ++c) {
        double lo = INFINITY, hi = -INFINITY;
        for (int64_t r = r0 + tid; r < r1; r += KF_NT) {
            const int64_t ep = r / Tk, i = r - ep * Tk;
            const double x = v[(ep * T + i * stride) * w + c];
            lo = fmin(lo, x); hi = fmax(hi, x);
        }
        lo = wg::reduce(lo, 2, (lptr)red);
        hi = wg::reduce(hi, 1, (lptr)red);
        if (tid == 0) {
            part[((size_t)blockIdx.x * 2) * w + c] = lo;
            part[((size_t)blockIdx.x * 2 + 1) * w + c] = hi;
        }
    }
}

// out (2 x w) = min / max over the workgroups' pairs, in workgroup order
__global__ void kf_minmax_final_kernel(const double *__restrict__ part, int nblk, int w, double *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * w) return;
    const bool ismax = e >= w;
    double v = ismax ? -INFINITY : INFINITY;
    for (int b = 0; b < nblk; ++b) {
        const double x = part[(size_t)b * 2 * w + e];
        v = ismax ? fmax(v, x) : fmin(v, x);
    }
    out[e] = v;
}

struct KfSolveArgs {
    const double *sums;
    int P, m, n, T16, NG;
    double ridge;
    double *A, *B;        // (P x P), (P x m)
    int32_t *info;        // -1, the failing pivot, or n (a non-finite entry in the solution that no pivot caught)
};

__device__ __forceinline__ double kf_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(KF_NT) kf_solve_kernel(KfSolveArgs a) {
    extern __shared__ double kf_L[];             // packed lower triangle: (i, j), j <= i, at i (i + 1) / 2 + j
    __shared__ int bad, nonfinite;
    __shared__ double kf_d0[KF_MAX_N];           // the diagonal of G + ridge I as given
    const int n = a.n, P = a.P, T16 = a.T16, tid = threadIdx.x;
    if (tid == 0) { bad = -1; nonfinite = 0; }
    for (int e = tid; e < n * n; e += KF_NT) {
        const int i = e / n, j = e - i * n;
        if (j > i) continue;
        // G[i][j] = G[j][i], held in the tile on or above the diagonal
        const double g = a.sums[(size_t)kf_gtile(j >> 4, i >> 4, T16) * 256 + (j & 15) * 16 + (i & 15)];
        kf_L[i * (i + 1) / 2 + j] = i == j ? g + a.ridge : g;
        if (i == j) kf_d0[i] = g + a.ridge;
    }
    __syncthreads();
    const double rel = n * 2.220446049250313e-16;
    for (int j = 0; j < n; ++j) {
        const double d = kf_L[j * (j + 1) / 2 + j];
        // a pivot that the elimination has brought down to the rounding level of its diagonal entry (n eps of it) is not positive:
        // its sign is noise (a rank-deficient G would otherwise pass or fail by chance).  The same value in every thread
        if (!(d > rel * kf_d0[j]) || !(d > 0.0) || !(d < INFINITY)) {
            if (tid == 0) bad = j;
            break;
        }
        const double ljj = sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < n; i += KF_NT) {
            const int at = i * (i + 1) / 2 + j;
            kf_L[at] = i == j ? ljj : kf_L[at] / ljj;
        }
        __syncthreads();
        const int w = n - j - 1;
        for (int e = tid; e < w * w; e += KF_NT) {
            const int i = j + 1 + e / w, k = j + 1 + (e - (e / w) * w);
            if (k > i) continue;
            const int at = i * (i + 1) / 2 + k;
            kf_L[at] = fma(-kf_L[i * (i + 1) / 2 + j], kf_L[k * (k + 1) / 2 + j], kf_L[at]);
        }
        __syncthreads();
    }
    __syncthreads();
    if (bad >= 0) {
        if (tid == 0) *a.info = bad;
        return;
    }
    // row r of X: (L L^T) x = R[r][:]^T; the lanes of a wave hold x[lane] and x[lane + 64]
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i0 = lane, i1 = lane + 64;
    for (int r = wave; r < P; r += KF_NT / 64) {
        const size_t rb = (size_t)(a.NG + (r >> 4) * T16) * 256 + (r & 15) * 16;
        double x0 = i0 < n ? a.sums[rb + (size_t)(i0 >> 4) * 256 + (i0 & 15)] : 0.0;
        double x1 = i1 < n ? a.sums[rb + (size_t)(i1 >> 4) * 256 + (i1 & 15)] : 0.0;
        for (int j = 0; j < n; ++j) {
            const double zj = kf_lane(j < 64 ? x0 : x1, j & 63) / kf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = zj;
            if (i1 == j) x1 = zj;
            if (i0 > j && i0 < n) x0 = fma(-kf_L[i0 * (i0 + 1) / 2 + j], zj, x0);
            if (i1 > j && i1 < n) x1 = fma(-kf_L[i1 * (i1 + 1) / 2 + j], zj, x1);
        }
        for (int j = n - 1; j >= 0; --j) {
            const double xj = kf_lane(j < 64 ? x0 : x1, j & 63) / kf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = xj;
            if (i1 == j) x1 = xj;
            if (i0 < j) x0 = fma(-kf_L[j * (j + 1) / 2 + i0], xj, x0);
            if (i1 < j) x1 = fma(-kf_L[j * (j + 1) / 2 + i1], xj, x1);
        }
        if (i0 < n) {
            if (i0 < P) a.A[(size_t)r * P + i0] = x0; else a.B[(size_t)r * a.m + (i0 - P)] = x0;
            if (!(fabs(x0) < INFINITY)) atomicOr(&nonfinite, 1);
        }
        if (i1 < n) {
            if (i1 < P) a.A[(size_t)r * P + i1] = x1; else a.B[(size_t)r * a.m + (i1 - P)] = x1;
            if (!(fabs(x1) < INFINITY)) atomicOr(&nonfinite, 1);
        }
    }
    __syncthreads();
    if (tid == 0) *a.info = nonfinite ? n : -1;
}

const void *kf_accum_fn(int ntw) {
    switch (ntw) {
        case 4: return (const void *)kf_accum_kernel<4>;
        case 10: return (const void *)kf_accum_kernel<10>;
        case 16: return (const void *)kf_accum_kernel<16>;
        default: return (const void *)kf_accum_kernel<25>;
    }
}

// the dynamic-LDS limit of a kernel, raised once to the largest request seen (as koop_prepare_launch does for the lift)
int kf_grant_lds(const void *fn, int slot, size_t bytes) {
    static std::mutex mu;
    static size_t granted[5] = {0, 0, 0, 0, 0};
    std::lock_guard<std::mutex> lock(mu);
    if (granted[slot] >= bytes) return SRH_OK;
    SRH_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted[slot] = bytes;
    return SRH_OK;
}

int kf_slot(int ntw) { return ntw == 4 ? 0 : (ntw == 10 ? 1 : (ntw == 16 ? 2 : 3)); }

int64_t kf_kept_rows(int64_t T, int stride) { return (T - 1) / stride + 1; }

}  // namespace

struct skoop_fit {
    skoop *lift = nullptr;
    KfShape s{};
    int64_t pairs = 0;
    size_t solve_lds = 0;
    srh::DevBuf sums, part, tiles, A, B, info;
};

// min / max of the channels of a device record (E x T x w) over the kept rows -> lo, hi (w) on the host
static int kf_minmax_dev(const double *v_dev, int64_t E, int64_t T, int w, int stride, hipStream_t st, double *lo, double *hi) {
    const int64_t Tk = kf_kept_rows(T, stride), rows = E * Tk;
    const int nblk = (int)std::min<int64_t>(256, srh::cdiv(rows, KF_NT));
    const int64_t rpb = srh::cdiv(rows, nblk);
    srh::DevBuf part, out;
    int rc;
    if ((rc = part.alloc(sizeof(double) * (size_t)nblk * 2 * w)) || (rc = out.alloc(sizeof(double) * 2 * w))) return rc;
    kf_minmax_kernel<<<(unsigned)nblk, KF_NT, 0, st>>>(v_dev, T, Tk, rows, stride, w, rpb, part.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    kf_minmax_final_kernel<<<(unsigned)srh::cdiv(2 * w, 64), 64, 0, st>>>(part.as<double>(), nblk, w, out.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    std::vector<double> h(2 * (size_t)w);
    SRH_CHECK_HIP(hipMemcpyAsync(h.data(), out.p, sizeof(double) * 2 * w, hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    std::copy(h.begin(), h.begin() + w, lo);
    std::copy(h.begin() + w, h.end(), hi);
    return SRH_OK;
}

static int kf_scale_of(const char *name, int w, const double *lo, const double *hi, double *offset, double *factor) {
    for (int c = 0; c < w; ++c) {
        SRH_REQUIRE(lo[c] <= hi[c] && std::isfinite(lo[c]) && std::isfinite(hi[c]), "skoop_fit_minmax: channel %s[%d] has no finite range", name, c);
        SRH_REQUIRE(lo[c] < hi[c], "skoop_fit_minmax: channel %s[%d] is constant (max == min = %g): it cannot be scaled", name, c, lo[c]);
        offset[c] = (hi[c] + lo[c]) / 2;
        factor[c] = (hi[c] - lo[c]) / 2;
    }
    return SRH_OK;
}

extern "C" {

int skoop_fit_plan(int nzeta, int degree, int dmd, int m, int *n_psi, int *n, int *rows_per_chunk, int64_t *lds_bytes) {
    if (n_psi) *n_psi = 0;
    if (n) *n = 0;
    if (rows_per_chunk) *rows_per_chunk = 0;
    if (lds_bytes) *lds_bytes = 0;
    SRH_REQUIRE(nzeta > 0 && degree > 0 && m > 0, "skoop_fit_plan: need nzeta, degree, m > 0");
    SRH_REQUIRE(nzeta <= KF_MAX_NZ && degree <= KF_MAX_DEG, "skoop_fit_plan: need nzeta <= %d and degree <= %d (the lift's limits)", KF_MAX_NZ,
                KF_MAX_DEG);
    const int P = skoop_num_observables(nzeta, degree, dmd);
    SRH_REQUIRE(P + m <= KF_MAX_N, "skoop_fit_plan: n = n_psi + m = %d + %d = %d exceeds the limit n <= %d", P, m, P + m, KF_MAX_N);
    const KfShape s = kf_shape(P, m, nzeta);
    if (n_psi) *n_psi = P;
    if (n) *n = s.n;
    if (rows_per_chunk) *rows_per_chunk = KF_TR;
    if (lds_bytes) *lds_bytes = (int64_t)s.lds;
    return SRH_OK;
}

int skoop_fit_create(skoop_fit_t **out, skoop_t *lift) {
    SRH_REQUIRE(out && lift, "skoop_fit_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(!lift->has_w, "skoop_fit_create: the lift handle projects with W; truncated models are not fitted (create it without W)");
    int rc;
    if ((rc = skoop_fit_plan(lift->nz, lift->degree, lift->dmd, lift->m, nullptr, nullptr, nullptr, nullptr))) return rc;
    auto *f = new skoop_fit();
    auto fail = [&](int code) { delete f; return code; };
    f->lift = lift;
    f->s = kf_shape(lift->P, lift->m, lift->nz);
    const KfShape &s = f->s;
    std::vector<int32_t> tiles;
    for (int ti = 0; ti < s.T16; ++ti)
        for (int tj = ti; tj < s.T16; ++tj) tiles.push_back((ti << 8) | tj);
    for (int ti = 0; ti < s.PT; ++ti)
        for (int tj = 0; tj < s.T16; ++tj) tiles.push_back((1 << 16) | (ti << 8) | tj);
    f->solve_lds = srh::lds_request(sizeof(double) * (size_t)s.n * (s.n + 1) / 2);
    if ((rc = f->tiles.upload(tiles.data(), sizeof(int32_t) * tiles.size())) || (rc = f->sums.alloc(sizeof(double) * (size_t)s.len)) ||
        (rc = f->A.alloc(sizeof(double) * (size_t)s.P * s.P)) || (rc = f->B.alloc(sizeof(double) * (size_t)s.P * s.m)) ||
        (rc = f->info.alloc(sizeof(int32_t))) || (rc = kf_grant_lds(kf_accum_fn(s.ntw), kf_slot(s.ntw), s.lds)) ||
        (rc = kf_grant_lds((const void *)kf_solve_kernel, 4, f->solve_lds)))
        return fail(rc);
    if (hipMemset(f->sums.p, 0, f->sums.bytes) != hipSuccess) { srh::set_error("skoop_fit_create: hipMemset failed"); return fail(SRH_EHIP); }
    *out = f;
    return SRH_OK;
}

int skoop_fit_destroy(skoop_fit_t *f) {
    SRH_REQUIRE(f, "skoop_fit_destroy: null handle");
    (void)hipDeviceSynchronize();
    delete f;
    return SRH_OK;
}

int skoop_fit_reset(skoop_fit_t *f) {
    SRH_REQUIRE(f, "skoop_fit_reset: null handle");
    SRH_CHECK_HIP(hipDeviceSynchronize());
    SRH_CHECK_HIP(hipMemset(f->sums.p, 0, f->sums.bytes));
    f->pairs = 0;
    return SRH_OK;
}

int skoop_fit_minmax_dev(const double *y_dev, const double *u_dev, int64_t E, int64_t T, int n_y, int m, int stride, double *y_offset,
                         double *y_factor, double *u_offset, double *u_factor, void *stream) {
    SRH_REQUIRE(y_dev && u_dev && y_offset && y_factor && u_offset && u_factor, "skoop_fit_minmax_dev: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1 && n_y >= 1 && m >= 1, "skoop_fit_minmax_dev: need E, T, n_y, m >= 1");
    SRH_REQUIRE(stride >= 1, "skoop_fit_minmax_dev: stride = %d, need stride >= 1", stride);
    std::vector<double> lo(std::max(n_y, m)), hi(std::max(n_y, m));
    int rc;
    if ((rc = kf_minmax_dev(y_dev, E, T, n_y, stride, (hipStream_t)stream, lo.data(), hi.data()))) return rc;
    if ((rc = kf_scale_of("y", n_y, lo.data(), hi.data(), y_offset, y_factor))) return rc;
    if ((rc = kf_minmax_dev(u_dev, E, T, m, stride, (hipStream_t)stream, lo.data(), hi.data()))) return rc;
    return kf_scale_of("u", m, lo.data(), hi.data(), u_offset, u_factor);
}

int skoop_fit_minmax(const double *y, const double *u, int64_t E, int64_t T, int n_y, int m, int stride, double *y_offset, double *y_factor,
                     double *u_offset, double *u_factor) {
    SRH_REQUIRE(y && u && y_offset && y_factor && u_offset && u_factor, "skoop_fit_minmax: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1 && n_y >= 1 && m >= 1, "skoop_fit_minmax: need E, T, n_y, m >= 1");
    SRH_REQUIRE(stride >= 1, "skoop_fit_minmax: stride = %d, need stride >= 1", stride);
    srh::DevBuf dy, du;
    int rc;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)E * T * n_y)) || (rc = du.upload(u, sizeof(double) * (size_t)E * T * m))) return rc;
    return skoop_fit_minmax_dev(dy.as<double>(), du.as<double>(), E, T, n_y, m, stride, y_offset, y_factor, u_offset, u_factor, nullptr);
}

int skoop_fit_add_dev(skoop_fit_t *f, const double *y_dev, const double *u_dev, int64_t E, int64_t T, int stride, int u_lag, void *stream) {
    SRH_REQUIRE(f, "skoop_fit_add_dev: null handle");
    SRH_REQUIRE(y_dev && u_dev, "skoop_fit_add_dev: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "skoop_fit_add_dev: need E >= 1 episodes of T >= 1 samples");
    SRH_REQUIRE(stride >= 1, "skoop_fit_add_dev: stride = %d, need stride >= 1", stride);
    SRH_REQUIRE(u_lag == 0 || u_lag == 1, "skoop_fit_add_dev: u_lag = %d, need 0 (row i holds the input after y_i) or 1 (before y_i)", u_lag);
    const skoop *h = f->lift;
    const KfShape &s = f->s;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t Tk = kf_kept_rows(T, stride);
    const int64_t ppe = Tk - 1 - h->delay;
    if (ppe <= 0) return SRH_OK;                  // T' <= d + 1: no pair
    KfAccArgs a{};
    a.y = y_dev; a.u = u_dev; a.T = T; a.ppe = ppe; a.cpe = srh::cdiv(ppe, KF_TR); a.nchunk = E * a.cpe;
    // workgroups: as many as there are chunks, up to what the scratch bound and the launch bound admit (whole rounds of 256 above 256)
    int64_t cap = std::min<int64_t>(KF_MAX_BLOCKS, (int64_t)(KF_SCRATCH_BYTES / (sizeof(double) * (size_t)s.len)));
    if (cap > 256) cap = cap / 256 * 256;
    a.nblk = (int)std::max<int64_t>(1, std::min(a.nchunk, cap));
    a.stride = stride; a.ulag = u_lag;
    a.ny = h->ny; a.m = h->m; a.delay = h->delay; a.nz = h->nz; a.P = s.P; a.n = s.n; a.ld = s.ld; a.nlev = h->nlev;
    a.has_const = h->dmd ? 0 : 1; a.ntile = s.ntile;
    const double *sc = h->scale.as<double>();
    a.yoff = sc; a.yfac = sc + h->ny; a.uoff = sc + 2 * h->ny; a.ufac = sc + 2 * h->ny + h->m;
    a.par = h->par.as<int32_t>(); a.var = h->var.as<int32_t>(); a.lev = h->lev.as<int32_t>();
    a.tiles = f->tiles.as<int32_t>();
    const size_t need = sizeof(double) * (size_t)a.nblk * (size_t)s.len;
    if (need > f->part.bytes) {
        SRH_CHECK_HIP(hipStreamSynchronize(st));   // an earlier launch may still read the block that is replaced
        int rc = f->part.alloc(need);
        if (rc) return rc;
    }
    a.part = f->part.as<double>();
    void *args[] = {&a};
    SRH_CHECK_HIP(hipLaunchKernel(kf_accum_fn(s.ntw), dim3((unsigned)a.nblk), dim3(KF_NT), args, s.lds, st));
    kf_reduce_kernel<<<(unsigned)srh::cdiv(s.len, KF_NT), KF_NT, 0, st>>>(a.part, a.nblk, s.len, f->sums.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    f->pairs += E * ppe;
    return SRH_OK;
}

int skoop_fit_add(skoop_fit_t *f, const double *y, const double *u, int64_t E, int64_t T, int stride, int u_lag) {
    SRH_REQUIRE(f, "skoop_fit_add: null handle");
    SRH_REQUIRE(y && u, "skoop_fit_add: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "skoop_fit_add: need E >= 1 episodes of T >= 1 samples");
    SRH_REQUIRE(stride >= 1, "skoop_fit_add: stride = %d, need stride >= 1", stride);
    SRH_REQUIRE(u_lag == 0 || u_lag == 1, "skoop_fit_add: u_lag = %d, need 0 (row i holds the input after y_i) or 1 (before y_i)", u_lag);
    srh::DevBuf dy, du;
    int rc;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)E * T * f->lift->ny)) || (rc = du.upload(u, sizeof(double) * (size_t)E * T * f->lift->m)))
        return rc;
    if ((rc = skoop_fit_add_dev(f, dy.as<double>(), du.as<double>(), E, T, stride, u_lag, nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return SRH_OK;
}

int skoop_fit_sums(skoop_fit_t *f, double *G, double *R, double *Q, int64_t *pairs) {
    SRH_REQUIRE(f, "skoop_fit_sums: null handle");
    const KfShape &s = f->s;
    if (pairs) *pairs = f->pairs;
    if (!G && !R && !Q) return SRH_OK;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> h((size_t)s.len);
    int rc = f->sums.download(h.data(), sizeof(double) * h.size());
    if (rc) return rc;
    const int n = s.n, P = s.P;
    if (G)
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) {
                const double v = h[(size_t)kf_gtile(i >> 4, j >> 4, s.T16) * 256 + (i & 15) * 16 + (j & 15)];
                G[(size_t)i * n + j] = v;
                G[(size_t)j * n + i] = v;
            }
    if (R)
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < n; ++j) R[(size_t)i * n + j] = h[(size_t)(s.NG + (i >> 4) * s.T16 + (j >> 4)) * 256 + (i & 15) * 16 + (j & 15)];
    if (Q) {
        double q = 0.0;
        for (int t = 0; t < 256; ++t) q += h[(size_t)s.ntile * 256 + t];
        *Q = q;
    }
    return SRH_OK;
}

int skoop_fit_solve(skoop_fit_t *f, double ridge, double *A, double *B, int32_t *info) {
    SRH_REQUIRE(f, "skoop_fit_solve: null handle");
    if (info) *info = -1;
    SRH_REQUIRE(A && B, "skoop_fit_solve: null argument");
    SRH_REQUIRE(ridge >= 0.0 && std::isfinite(ridge), "skoop_fit_solve: need a finite ridge >= 0");
    SRH_REQUIRE(f->pairs > 0, "skoop_fit_solve: no pairs have been added (S = 0)");
    const KfShape &s = f->s;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    KfSolveArgs a{f->sums.as<double>(), s.P, s.m, s.n, s.T16, s.NG, ridge, f->A.as<double>(), f->B.as<double>(), f->info.as<int32_t>()};
    kf_solve_kernel<<<1, KF_NT, f->solve_lds, nullptr>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    int32_t bad = -1;
    int rc = f->info.download(&bad, sizeof(int32_t));
    if (rc) return rc;
    if (info) *info = bad;
    if (bad >= 0 && bad < s.n) {
        srh::set_error("skoop_fit_solve: pivot %d of G + ridge I (n = %d, ridge = %g) is not positive (above n eps of its diagonal entry) or not "
                       "finite: increase ridge", bad, s.n, ridge);
        return SRH_ENUMERIC;
    }
    if (bad >= s.n) {
        srh::set_error("skoop_fit_solve: the solution holds a non-finite entry (a non-finite value of the sums that no pivot caught)");
        return SRH_ENUMERIC;
    }
    if ((rc = f->A.download(A, sizeof(double) * (size_t)s.P * s.P)) || (rc = f->B.download(B, sizeof(double) * (size_t)s.P * s.m))) return rc;
    return SRH_OK;
}

}  // extern "C"
