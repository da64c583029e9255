// TPWL model identification on the device: records (x, u) of a reduced state and P linearisation points -> per-point sums of one affine
// least-squares fit -> the tables A_c, B_c, d_c, u of a TPWL model (stpwl_create).
//
// THE FIT ("TPWL model identification", defines it; the reference builds its tables from the simulator's Jacobians and
// ships no fit).
//   Records: E episodes, each x (T x n_x), x = [v; q], n_x = 2 r, and u (T x m).  Row i holds the input applied after x_i.  `stride`
//   s >= 1 keeps rows 0, s, 2s, .. of every episode; T' = the rows kept.  Samples: the kept rows i <= T' - 2 (those with a kept successor
//   in their episode); T' < 2 contributes nothing; no sample pairs across episodes.
//   Points: (q_p, v_p), p < P, and the weights (w_q, w_v); x_p = [v_p; q_p].  p(i) = the nearest point to x_i by THE POINT-SEARCH RULE of
//   tpwl_dev.h (tpwl::nearest_wave is called, not restated).
//   Regressor phi_i = [x_i - x_p; u_i; 1], n = n_x + m + 1.  Target g_i = (x_{i+1} - x_i) / Ts over kept rows.
//   Sums per point over its samples: G_p = sum phi phi^T, R_p = sum g phi^T, Q_p = sum |g|^2, S_p = the samples.
//   Solve per point: with D = diag(G_p), (D^-1/2 G_p D^-1/2 + ridge I) z = D^-1/2 r for every row r of R_p, [A_c | B_c | c] = the rows
//   D^-1/2 z; d_c = c - A_c x_p; u = the mean input of the point's samples (G_p[input][constant] / S_p).
//
// Kernels.  tf_assign_kernel: the region of every sample through tpwl::nearest_wave, the first kept row that is not finite (an integer
// atomicMin on the row number) and one integer histogram of the regions per workgroup.  tf_scan_kernel / tf_scatter_kernel: a stable
// counting sort of the row numbers by region -- an exclusive scan of the (region, workgroup) counts, then every row goes to its
// workgroup's offset plus its rank among the workgroup's earlier rows of the same region (wave ballots; integer LDS counters).
// tf_accum_kernel has the plan of sf_accum_kernel (ssm_fit.hip): a workgroup owns a granule, up to TF_GRAN chunks of TF_TR consecutive
// entries of ONE region's ordered list; per chunk it gathers x_i, x_{i+1}, u_i by row number into the panel
// [x_i - x_p | u | 1 | zeros | g | zeros]; G's upper tiles are phi-block x phi-block, R's tiles g-block x phi-block, on
// v_mfma_f64_16x16x4_f64 with the panel row as the k index.  Tiles stay in registers over the granule; tf_reduce_kernel adds the
// granules' partials to the running sums of their region in granule order.  tf_solve_kernel: one workgroup per point.
// No floating-point atomics: every chain of additions is fixed by the records and the sequence of add calls (the ordered lists, the
// granule map and the MFMA's k order), so the same calls give the same bits and device records give the bits of host arrays.  Two add
// calls do NOT give the bits of one: their ordered lists, hence their granules, differ.
//
// The tile map, the reduce and the packed Cholesky have the plan of ssm_fit.hip's and koopman_fit.hip's and are restated here, not
// shared: the gather by row number, the per-point sums and the per-point status differ, and those units stay what their tests pinned.
#include "tpwl_host.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr int TF_TR = 64;                 // list entries of a chunk (a multiple of 4: the k step of the MFMA)
constexpr int TF_NT = 256;                // threads of the scan, accumulate, reduce and solve kernels (4 waves)
constexpr int TF_AB = 1024;               // kept rows of an assign / scatter workgroup
constexpr int TF_ANT = 1024;              // threads of the assign kernel: 16 waves, 64 searches each (a search is a chain of L2 round trips)
constexpr int TF_MAX_N = 128;             // n = n_x + m + 1: the packed Cholesky's LDS, and 36 + 64 tiles = 25 per wave
constexpr int TF_MAX_M = 16;              // stpwl_create's limit
constexpr int TF_MAX_P = 1024;            // the LDS histogram of the assign kernel and the footprint of P sets of sums
constexpr int TF_MAX_BLOCKS = 768;        // workgroups of an accumulate launch
constexpr int TF_GRAN = 8;                // chunks of a granule
constexpr size_t TF_SCRATCH_BYTES = (size_t)64 << 20;
constexpr size_t TF_LDS_MAX = (size_t)160 * 1024;
constexpr int TF_MAX_DEV = 16;
typedef double tf_d4 __attribute__((ext_vector_type(4)));

struct TfShape {
    int nx, m, n;
    int T16;        // 16-column tiles across phi
    int TT;         // 16-row tiles down R
    int NG;         // tiles of G on or above the diagonal; R's tiles follow them
    int ntile;
    int ld;         // row stride of the panel: = 16 (mod 32) doubles
    int tg;         // first column of g in a panel row (16 T16)
    int ntw;        // tiles per wave of the kernel instance used
    int64_t len;    // doubles of one point's sums: (ntile + 1) x 256, the last block = the per-thread parts of Q
    size_t lds;     // dynamic LDS of the accumulate kernel
};

TfShape tf_shape(int nx, int m) {
    TfShape s{};
    s.nx = nx; s.m = m; s.n = nx + m + 1;
    s.T16 = (s.n + 15) / 16;
    s.TT = (nx + 15) / 16;
    s.NG = s.T16 * (s.T16 + 1) / 2;
    s.ntile = s.NG + s.TT * s.T16;
    s.tg = 16 * s.T16;
    s.ld = 16 * (s.T16 + s.TT);
    if (s.ld % 32 != 16) s.ld += 16;
    const int need = (s.ntile + 3) / 4;
    s.ntw = need <= 4 ? 4 : (need <= 10 ? 10 : (need <= 16 ? 16 : 25));
    s.len = (int64_t)(s.ntile + 1) * 256;
    // the panel; behind it x_p (nx) and the first source row of every panel row (TF_TR 64-bit integers)
    s.lds = srh::lds_request(sizeof(double) * ((size_t)TF_TR * (size_t)s.ld + (size_t)nx + (size_t)TF_TR));
    return s;
}

__host__ __device__ inline int tf_gtile(int ti, int tj, int T16) { return ti * T16 - ti * (ti - 1) / 2 + (tj - ti); }

// kept row k of the call -> its row in the records: episode k / Tk, kept row k % Tk of it
__device__ __forceinline__ int64_t tf_src_row(int64_t k, int64_t T, int64_t Tk, int stride) {
    const int64_t ep = k / Tk;
    return ep * T + (k - ep * Tk) * stride;
}

// region[k] of the samples (-1 of the kept rows that are none), the first kept row that is not finite, the workgroup's histogram
__global__ void __launch_bounds__(TF_ANT) tf_assign_kernel(TpwlDev Tb, const double *__restrict__ X, const double *__restrict__ U, int64_t T,
                                                          int64_t Tk, int stride, int64_t nrows, int32_t *__restrict__ region,
                                                          int32_t *__restrict__ hist, unsigned long long *__restrict__ bad) {
    extern __shared__ int tf_hist[];
    const int tid = threadIdx.x, P = Tb.P, n = Tb.n, m = Tb.m;
    for (int e = tid; e < P; e += TF_ANT) tf_hist[e] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int64_t k0 = (int64_t)blockIdx.x * TF_AB, k1 = min(nrows, k0 + TF_AB);
    for (int64_t k = k0 + wave; k < k1; k += TF_ANT / 64) {
        const int64_t ep = k / Tk, i = k - ep * Tk, row = ep * T + i * stride;
        const double *x = X + row * n, *u = U + row * m;
        bool ok = true;
        for (int j = lane; j < n; j += 64) ok = ok && (fabs(x[j]) < INFINITY);
        for (int j = lane; j < m; j += 64) ok = ok && (fabs(u[j]) < INFINITY);
        if (__builtin_amdgcn_ballot_w64(!ok) != 0 && lane == 0) atomicMin(bad, (unsigned long long)k);
        int p = -1;
        if (i < Tk - 1) p = tpwl::nearest_wave(Tb, x);          // the same for every lane of the wave
        if (lane == 0) {
            region[k] = p;
            if (p >= 0) atomicAdd(&tf_hist[p], 1);
        }
    }
    __syncthreads();
    for (int e = tid; e < P; e += TF_ANT) hist[(size_t)blockIdx.x * P + e] = tf_hist[e];
}

// offs[p * nblk + b] = the position in the ordered list of the first row of region p that workgroup b holds: the exclusive scan of the
// counts in (region, workgroup) order.  start[p] = offs[p * nblk], start[P] = the samples.  One workgroup.
__global__ void __launch_bounds__(TF_NT) tf_scan_kernel(const int32_t *__restrict__ hist, int nblk, int P, int32_t *__restrict__ offs,
                                                        int32_t *__restrict__ start) {
    __shared__ int tot[TF_NT];
    const int tid = threadIdx.x;
    const int64_t M = (int64_t)P * nblk, seg = (M + TF_NT - 1) / TF_NT, e0 = min(M, tid * seg), e1 = min(M, e0 + seg);
    int s = 0;
    for (int64_t e = e0; e < e1; ++e) s += hist[(e % nblk) * P + e / nblk];
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < TF_NT; ++t) { const int v = tot[t]; tot[t] = run; run += v; }
        start[P] = run;
    }
    __syncthreads();
    int run = tot[tid];
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t p = e / nblk, b = e - p * nblk;
        offs[e] = run;
        if (b == 0) start[p] = run;
        run += hist[b * P + p];
    }
}

// list[offs[region][workgroup] + rank] = k, rank = the workgroup's earlier rows of the same region.  One wave per workgroup: it walks
// its rows 64 at a time in order, and in a group of 64 the rank is the count of the lower lanes that hold the same region
__global__ void __launch_bounds__(64) tf_scatter_kernel(const int32_t *__restrict__ region, const int32_t *__restrict__ offs, int nblk, int P,
                                                        int64_t nrows, int32_t *__restrict__ list) {
    extern __shared__ int tf_cnt[];
    const int lane = threadIdx.x;
    for (int e = lane; e < P; e += 64) tf_cnt[e] = offs[(size_t)e * nblk + blockIdx.x];
    __syncthreads();
    const int64_t k0 = (int64_t)blockIdx.x * TF_AB, k1 = min(nrows, k0 + TF_AB);
    for (int64_t kb = k0; kb < k1; kb += 64) {
        const int64_t k = kb + lane;
        const int rg = k < k1 ? region[k] : -1;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(rg >= 0);
        while (todo) {
            const int leader = __builtin_ctzll(todo);
            const int lr = __shfl(rg, leader, 64);
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(rg == lr);
            if (rg == lr) list[tf_cnt[lr] + __builtin_popcountll(mask & ((1ull << lane) - 1ull))] = (int32_t)k;
            __syncthreads();
            if (lane == leader) tf_cnt[lr] += __builtin_popcountll(mask);
            __syncthreads();
            todo &= ~mask;
        }
    }
}

struct TfAccArgs {
    const double *X, *U;          // (E x T x nx), (E x T x m)
    int64_t T, Tk;
    int stride;
    int nx, m, n, ld, tg, ntile;
    double Ts;
    const double *xp;             // (P x nx)
    const int32_t *list;          // the kept rows ordered by region
    const int32_t *gran;          // (ngran x 3): region, first entry in list, entries
    int64_t g0;                   // granule of workgroup 0 of this launch
    const int32_t *tiles;         // (ntile): column block of the A operand << 8 | column block of the B operand
    double *part;                 // (nblk x (ntile + 1) x 256)
};

template <int NTW>
__global__ void __launch_bounds__(TF_NT) tf_accum_kernel(TfAccArgs a) {
    extern __shared__ double tf_smem[];
    const int ld = a.ld, nx = a.nx, m = a.m, n = a.n, tg = a.tg;
    double *ps = tf_smem;                           // TF_TR x ld: [x - x_p | u | 1 | zeros | g | zeros]
    double *sxp = ps + (size_t)TF_TR * ld;          // nx
    long long *srow = reinterpret_cast<long long *>(sxp + nx);   // TF_TR: the row of x_i in the records
    const int tid = threadIdx.x;
    const int64_t gr = a.g0 + blockIdx.x;
    const int p = a.gran[3 * gr], first = a.gran[3 * gr + 1], len = a.gran[3 * gr + 2];
    for (int e = tid; e < nx; e += TF_NT) sxp[e] = a.xp[(size_t)p * nx + e];
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l16 = lane & 15, kk = lane >> 4;
    // the tiles of this wave: A operand row[16 ca + l16], B operand row[16 cb + l16] of panel row k; D row kk + 4 g, column l16
    int offA[NTW], offB[NTW];
    tf_d4 acc[NTW];
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
        const int t = wave + 4 * q;
        const int code = t < a.ntile ? a.tiles[t] : 0;
        offA[q] = 16 * ((code >> 8) & 255);
        offB[q] = 16 * (code & 255);
        acc[q] = tf_d4{0.0, 0.0, 0.0, 0.0};
    }
    // the columns no step below writes (n .. tg - 1 and tg + nx .. ld - 1) are read by the last tiles: zeros, written once
    for (int e = tid; e < TF_TR * ld; e += TF_NT) {
        const int c = e % ld;
        if ((c >= n && c < tg) || c >= tg + nx) ps[e] = 0.0;
    }
    double qg = 0.0;
    const int nchunk = (len + TF_TR - 1) / TF_TR;
    for (int ci = 0; ci < nchunk; ++ci) {
        const int np = min(TF_TR, len - ci * TF_TR);                 // entries of this chunk: panel rows 0 .. np - 1 hold data
        __syncthreads();                                             // the previous chunk's products have read the panel
        if (tid < TF_TR) srow[tid] = tid < np ? tf_src_row(a.list[first + ci * TF_TR + tid], a.T, a.Tk, a.stride) : 0;
        __syncthreads();
        // x_i - x_p (one rounding) and g = (x_{i+1} - x_i) / Ts (two); the rows behind the entries are zeros in every column
        for (int e = tid; e < TF_TR * nx; e += TF_NT) {
            const int r = e / nx, j = e - r * nx;
            double d = 0.0, g = 0.0;
            if (r < np) {
                const double xi = a.X[srow[r] * nx + j], xn = a.X[(srow[r] + a.stride) * nx + j];
                d = xi - sxp[j];
                g = (xn - xi) / a.Ts;
            }
            ps[r * ld + j] = d;
            ps[r * ld + tg + j] = g;
        }
        for (int e = tid; e < TF_TR * (m + 1); e += TF_NT) {
            const int r = e / (m + 1), el = e - r * (m + 1);
            ps[r * ld + nx + el] = r < np ? (el < m ? a.U[srow[r] * m + el] : 1.0) : 0.0;
        }
        __syncthreads();
        // |g|^2 over the chunk, a fixed share per thread
        for (int e = tid; e < np * nx; e += TF_NT) {
            const int r = e / nx, cc = e - r * nx;
            const double v = ps[r * ld + tg + cc];
            qg = fma(v, v, qg);
        }
        const int ksteps = (np + 3) >> 2;
        for (int s = 0; s < ksteps; ++s) {
            const double *row = ps + (4 * s + kk) * ld + l16;        // 4 s + kk <= 63
#pragma unroll
            for (int q = 0; q < NTW; ++q) {
                if (wave + 4 * q < a.ntile) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[offA[q]], row[offB[q]], acc[q], 0, 0, 0);
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
    dst[(size_t)a.ntile * 256 + tid] = qg;
}

// sums of point blockIdx.y += the partials of its granules among the launch's g0 .. g0 + nblk - 1, in granule order
__global__ void __launch_bounds__(TF_NT) tf_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ gfirst, int64_t g0, int nblk,
                                                          int64_t len, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * TF_NT + threadIdx.x;
    if (i >= len) return;
    const int p = blockIdx.y;
    const int64_t lo = max((int64_t)gfirst[p], g0), hi = min((int64_t)gfirst[p + 1], g0 + nblk);
    if (lo >= hi) return;
    double v = sums[(int64_t)p * len + i];
    for (int64_t b = lo; b < hi; ++b) v += part[(b - g0) * len + i];
    sums[(int64_t)p * len + i] = v;
}

struct TfSolveArgs {
    const double *sums;
    int64_t len;
    const int64_t *counts;   // (P)
    int64_t min_samples;
    int n, nx, m, T16, NG;
    double ridge;
    double *X;               // (P x nx x n): the rows [A_c | B_c | c]
    double *umean;           // (P x m)
    int32_t *info;           // (P x 2): status; the failing column, n for a non-finite solution that no pivot caught, or -1
};

__device__ __forceinline__ double tf_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// one workgroup per point (sf_solve_kernel's plan on the full column set)
__global__ void __launch_bounds__(TF_NT) tf_solve_kernel(TfSolveArgs a) {
    extern __shared__ double tf_L[];             // packed lower triangle: (i, j), j <= i, at i (i + 1) / 2 + j
    __shared__ int bad, nonfinite;
    __shared__ double tf_dinv[TF_MAX_N];         // D^-1/2
    const int n = a.n, nx = a.nx, T16 = a.T16, tid = threadIdx.x, p = blockIdx.x;
    const double *sums = a.sums + (size_t)p * a.len;
    double *X = a.X + (size_t)p * nx * n;
    int32_t *info = a.info + 2 * p;
    const int64_t S = a.counts[p];
    for (int e = tid; e < nx * n; e += TF_NT) X[e] = 0.0;
    // the mean input: G[input k][constant] / S (0 of a point without samples)
    for (int k = tid; k < a.m; k += TF_NT) {
        const int i = nx + k, j = n - 1;
        a.umean[(size_t)p * a.m + k] = S > 0 ? sums[(size_t)tf_gtile(i >> 4, j >> 4, T16) * 256 + (i & 15) * 16 + (j & 15)] / (double)S : 0.0;
    }
    if (S < a.min_samples) {
        if (tid == 0) { info[0] = 1; info[1] = -1; }
        return;
    }
    if (tid == 0) { bad = n; nonfinite = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += TF_NT) {
        const double g = sums[(size_t)tf_gtile(i >> 4, i >> 4, T16) * 256 + (i & 15) * 17];
        // a diagonal entry that is negative or not finite cannot be scaled: the first one is reported as the pivot.  A zero one is a
        // column of zeros (an input held at 0 over the point's samples): it keeps the scale 1 and the diagonal 0 + ridge, so its pivot
        // fails at ridge = 0 and its coefficient is 0 at ridge > 0
        if (!(g >= 0.0) || !(g < INFINITY)) atomicMin(&bad, i);
        tf_dinv[i] = g > 0.0 ? 1.0 / sqrt(g) : 1.0;
    }
    __syncthreads();
    if (bad < n) {
        if (tid == 0) { info[0] = 2; info[1] = bad; }
        return;
    }
    for (int e = tid; e < n * n; e += TF_NT) {
        const int i = e / n, j = e - i * n;
        if (j > i) continue;
        // G[i][j] = G[j][i], j <= i, held in the tile on or above the diagonal; the scaled block has the diagonal 1 + ridge exactly
        const double g = sums[(size_t)tf_gtile(j >> 4, i >> 4, T16) * 256 + (j & 15) * 16 + (i & 15)];
        tf_L[i * (i + 1) / 2 + j] = i == j ? (g > 0.0 ? 1.0 + a.ridge : a.ridge) : g * tf_dinv[i] * tf_dinv[j];
    }
    __syncthreads();
    const double floor_ = n * 2.220446049250313e-16 * (1.0 + a.ridge);
    int fail = -1;
    for (int j = 0; j < n; ++j) {
        const double d = tf_L[j * (j + 1) / 2 + j];
        // a pivot that the elimination has brought down to the rounding level of its diagonal entry (n eps of it) is not positive:
        // its sign is noise.  The same value in every thread
        if (!(d > floor_) || !(d < INFINITY)) { fail = j; break; }
        const double ljj = sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < n; i += TF_NT) {
            const int at = i * (i + 1) / 2 + j;
            tf_L[at] = i == j ? ljj : tf_L[at] / ljj;
        }
        __syncthreads();
        const int w = n - j - 1;
        for (int e = tid; e < w * w; e += TF_NT) {
            const int i = j + 1 + e / w, k = j + 1 + (e - (e / w) * w);
            if (k > i) continue;
            const int at = i * (i + 1) / 2 + k;
            tf_L[at] = fma(-tf_L[i * (i + 1) / 2 + j], tf_L[k * (k + 1) / 2 + j], tf_L[at]);
        }
        __syncthreads();
    }
    if (fail >= 0) {
        if (tid == 0) { info[0] = 2; info[1] = fail; }
        return;
    }
    // row r of X: (L L^T) z = D^-1/2 R[r]^T, x = D^-1/2 z; the lanes of a wave hold entries lane and lane + 64
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i0 = lane, i1 = lane + 64;
    for (int r = wave; r < nx; r += TF_NT / 64) {
        const size_t rb = (size_t)(a.NG + (r >> 4) * T16) * 256 + (r & 15) * 16;
        double x0 = i0 < n ? sums[rb + (size_t)(i0 >> 4) * 256 + (i0 & 15)] * tf_dinv[i0] : 0.0;
        double x1 = i1 < n ? sums[rb + (size_t)(i1 >> 4) * 256 + (i1 & 15)] * tf_dinv[i1] : 0.0;
        for (int j = 0; j < n; ++j) {
            const double zj = tf_lane(j < 64 ? x0 : x1, j & 63) / tf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = zj;
            if (i1 == j) x1 = zj;
            if (i0 > j && i0 < n) x0 = fma(-tf_L[i0 * (i0 + 1) / 2 + j], zj, x0);
            if (i1 > j && i1 < n) x1 = fma(-tf_L[i1 * (i1 + 1) / 2 + j], zj, x1);
        }
        for (int j = n - 1; j >= 0; --j) {
            const double xj = tf_lane(j < 64 ? x0 : x1, j & 63) / tf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = xj;
            if (i1 == j) x1 = xj;
            if (i0 < j) x0 = fma(-tf_L[j * (j + 1) / 2 + i0], xj, x0);
            if (i1 < j) x1 = fma(-tf_L[j * (j + 1) / 2 + i1], xj, x1);
        }
        if (i0 < n) {
            x0 *= tf_dinv[i0];
            X[(size_t)r * n + i0] = x0;
            if (!(fabs(x0) < INFINITY)) atomicOr(&nonfinite, 1);
        }
        if (i1 < n) {
            x1 *= tf_dinv[i1];
            X[(size_t)r * n + i1] = x1;
            if (!(fabs(x1) < INFINITY)) atomicOr(&nonfinite, 1);
        }
    }
    __syncthreads();
    if (tid == 0) { info[0] = nonfinite ? 2 : 0; info[1] = nonfinite ? n : -1; }
}

const void *tf_accum_fn(int ntw) {
    switch (ntw) {
        case 4: return (const void *)tf_accum_kernel<4>;
        case 10: return (const void *)tf_accum_kernel<10>;
        case 16: return (const void *)tf_accum_kernel<16>;
        default: return (const void *)tf_accum_kernel<25>;
    }
}

// the dynamic-LDS limit of a kernel on the current device, raised once per device to the largest request seen
int tf_grant_lds(const void *fn, int slot, size_t bytes) {
    static std::mutex mu;
    static size_t granted[TF_MAX_DEV][5] = {};
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    SRH_CHECK_HIP(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < TF_MAX_DEV;
    if (known && granted[dev][slot] >= bytes) return SRH_OK;
    SRH_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) granted[dev][slot] = bytes;
    return SRH_OK;
}

int tf_slot(int ntw) { return ntw == 4 ? 0 : (ntw == 10 ? 1 : (ntw == 16 ? 2 : 3)); }

int64_t tf_kept_rows(int64_t T, int stride) { return (T - 1) / stride + 1; }

int tf_check_shape(const char *who, int P, int r, int m) {
    SRH_REQUIRE(P > 0 && r > 0 && m > 0, "%s: need P, r, m > 0", who);
    SRH_REQUIRE(m <= TF_MAX_M, "%s: m = %d exceeds the limit m <= %d (stpwl_create's)", who, m, TF_MAX_M);
    SRH_REQUIRE((int64_t)2 * r + m + 1 <= TF_MAX_N, "%s: n = n_x + m + 1 = %lld + %d + 1 = %lld exceeds the limit n <= %d", who,
                (long long)2 * r, m, (long long)2 * r + m + 1, TF_MAX_N);
    SRH_REQUIRE(P <= TF_MAX_P, "%s: P = %d exceeds the limit P <= %d", who, P, TF_MAX_P);
    return SRH_OK;
}

}  // namespace

struct stpwl_fit {
    TfShape s{};
    int P = 0, r = 0;
    double w_q = 1.0, w_v = 0.0, Ts = 0.0;
    std::vector<int64_t> counts;           // (P) samples per point
    std::vector<double> xp;                // (P x nx) host copy of [v_p; q_p]
    srh::DevBuf qT, vT, xp_dev, sums, tiles, part;
    srh::DevBuf region, hist, offs, start, list, bad, gran, gfirst;          // the work arrays of an add call (kept between calls)
    TpwlDev view() const {
        TpwlDev T{};
        T.P = P; T.r = r; T.n = 2 * r; T.m = s.m; T.nz = 0;
        T.w_q = w_q; T.w_v = w_v;
        T.qT = (cgptr)qT.as<double>(); T.vT = (cgptr)vT.as<double>();
        return T;
    }
};

// a work array of at least `bytes` (the handle is idle: every add call ends synchronised)
static int tf_room(srh::DevBuf &b, size_t bytes) { return b.bytes >= bytes ? SRH_OK : b.alloc(bytes); }

extern "C" {

int stpwl_fit_plan(int P, int r, int m, int *n, int *rows_per_chunk, int *tiles_per_wave, int64_t *lds_bytes) {
    if (n) *n = 0;
    if (rows_per_chunk) *rows_per_chunk = 0;
    if (tiles_per_wave) *tiles_per_wave = 0;
    if (lds_bytes) *lds_bytes = 0;
    int rc;
    if ((rc = tf_check_shape("stpwl_fit_plan", P, r, m))) return rc;
    const TfShape s = tf_shape(2 * r, m);
    SRH_REQUIRE(s.lds <= TF_LDS_MAX, "stpwl_fit_plan: the panel of n = %d regressors and n_x = %d targets needs %zu bytes of LDS, above %zu", s.n,
                s.nx, s.lds, TF_LDS_MAX);
    if (n) *n = s.n;
    if (rows_per_chunk) *rows_per_chunk = TF_TR;
    if (tiles_per_wave) *tiles_per_wave = s.ntw;
    if (lds_bytes) *lds_bytes = (int64_t)s.lds;
    return SRH_OK;
}

int stpwl_fit_create(stpwl_fit_t **out, int P, int r, int m, const double *q, const double *v, double w_q, double w_v, double Ts) {
    SRH_REQUIRE(out && q && v, "stpwl_fit_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(Ts > 0.0 && std::isfinite(Ts), "stpwl_fit_create: need a finite Ts > 0");
    SRH_REQUIRE(std::isfinite(w_q) && std::isfinite(w_v), "stpwl_fit_create: the distance weights must be finite");
    int rc;
    if ((rc = stpwl_fit_plan(P, r, m, nullptr, nullptr, nullptr, nullptr))) return rc;
    for (int64_t e = 0; e < (int64_t)P * r; ++e)
        SRH_REQUIRE(std::isfinite(q[e]) && std::isfinite(v[e]), "stpwl_fit_create: point %lld holds a non-finite entry", (long long)(e / r));
    auto *f = new stpwl_fit();
    auto fail = [&](int code) { delete f; return code; };
    f->s = tf_shape(2 * r, m);
    f->P = P; f->r = r; f->w_q = w_q; f->w_v = w_v; f->Ts = Ts;
    f->counts.assign(P, 0);
    const TfShape &s = f->s;
    std::vector<double> qT((size_t)P * r), vT((size_t)P * r);
    f->xp.resize((size_t)P * s.nx);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < r; ++j) {
            qT[(size_t)j * P + p] = q[(size_t)p * r + j];
            vT[(size_t)j * P + p] = v[(size_t)p * r + j];
            f->xp[(size_t)p * s.nx + j] = v[(size_t)p * r + j];
            f->xp[(size_t)p * s.nx + r + j] = q[(size_t)p * r + j];
        }
    std::vector<int32_t> tiles;
    for (int ti = 0; ti < s.T16; ++ti)
        for (int tj = ti; tj < s.T16; ++tj) tiles.push_back((ti << 8) | tj);
    for (int ti = 0; ti < s.TT; ++ti)
        for (int tj = 0; tj < s.T16; ++tj) tiles.push_back(((s.T16 + ti) << 8) | tj);
    const size_t solve_lds = srh::lds_request(sizeof(double) * (size_t)s.n * (s.n + 1) / 2);
    if ((rc = f->qT.upload(qT.data(), sizeof(double) * qT.size())) || (rc = f->vT.upload(vT.data(), sizeof(double) * vT.size())) ||
        (rc = f->xp_dev.upload(f->xp.data(), sizeof(double) * f->xp.size())) ||
        (rc = f->tiles.upload(tiles.data(), sizeof(int32_t) * tiles.size())) || (rc = f->sums.alloc(sizeof(double) * (size_t)P * s.len)) ||
        (rc = f->bad.alloc(sizeof(unsigned long long))) || (rc = tf_grant_lds(tf_accum_fn(s.ntw), tf_slot(s.ntw), s.lds)) ||
        (rc = tf_grant_lds((const void *)tf_solve_kernel, 4, solve_lds)))
        return fail(rc);
    if (hipMemset(f->sums.p, 0, f->sums.bytes) != hipSuccess) { srh::set_error("stpwl_fit_create: hipMemset failed"); return fail(SRH_EHIP); }
    *out = f;
    return SRH_OK;
}

int stpwl_fit_destroy(stpwl_fit_t *f) {
    SRH_REQUIRE(f, "stpwl_fit_destroy: null handle");
    (void)hipDeviceSynchronize();
    delete f;
    return SRH_OK;
}

int stpwl_fit_reset(stpwl_fit_t *f) {
    SRH_REQUIRE(f, "stpwl_fit_reset: null handle");
    SRH_CHECK_HIP(hipDeviceSynchronize());
    SRH_CHECK_HIP(hipMemset(f->sums.p, 0, f->sums.bytes));
    std::fill(f->counts.begin(), f->counts.end(), 0);
    return SRH_OK;
}

int stpwl_fit_add_dev(stpwl_fit_t *f, const double *x_dev, const double *u_dev, int64_t E, int64_t T, int stride, void *stream) {
    SRH_REQUIRE(f, "stpwl_fit_add_dev: null handle");
    SRH_REQUIRE(x_dev && u_dev, "stpwl_fit_add_dev: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "stpwl_fit_add_dev: need E >= 1 episodes of T >= 1 rows");
    SRH_REQUIRE(stride >= 1, "stpwl_fit_add_dev: stride = %d, need stride >= 1", stride);
    const TfShape &s = f->s;
    const hipStream_t st = (hipStream_t)stream;
    const int P = f->P;
    const int64_t Tk = tf_kept_rows(T, stride), nrows = E * Tk;
    SRH_REQUIRE(nrows < ((int64_t)1 << 31), "stpwl_fit_add_dev: %lld kept rows in one call, need fewer than 2^31 (split the records)", (long long)nrows);
    const int nblk = (int)srh::cdiv(nrows, TF_AB);
    int rc;
    if ((rc = tf_room(f->region, sizeof(int32_t) * (size_t)nrows)) || (rc = tf_room(f->list, sizeof(int32_t) * (size_t)nrows)) ||
        (rc = tf_room(f->hist, sizeof(int32_t) * (size_t)nblk * P)) || (rc = tf_room(f->offs, sizeof(int32_t) * (size_t)nblk * P)) ||
        (rc = tf_room(f->start, sizeof(int32_t) * (size_t)(P + 1))))
        return rc;
    // assign -> scan -> scatter; the first non-finite kept row and the regions' first entries come back before anything touches the sums
    SRH_CHECK_HIP(hipMemsetAsync(f->bad.p, 0xff, sizeof(unsigned long long), st));
    tf_assign_kernel<<<(unsigned)nblk, TF_ANT, sizeof(int) * (size_t)P, st>>>(f->view(), x_dev, u_dev, T, Tk, stride, nrows, f->region.as<int32_t>(),
                                                                             f->hist.as<int32_t>(), f->bad.as<unsigned long long>());
    SRH_CHECK_HIP(hipGetLastError());
    tf_scan_kernel<<<1, TF_NT, 0, st>>>(f->hist.as<int32_t>(), nblk, P, f->offs.as<int32_t>(), f->start.as<int32_t>());
    SRH_CHECK_HIP(hipGetLastError());
    tf_scatter_kernel<<<(unsigned)nblk, 64, sizeof(int) * (size_t)P, st>>>(f->region.as<int32_t>(), f->offs.as<int32_t>(), nblk, P, nrows,
                                                                           f->list.as<int32_t>());
    SRH_CHECK_HIP(hipGetLastError());
    unsigned long long bad = 0;
    std::vector<int32_t> start((size_t)P + 1);
    SRH_CHECK_HIP(hipMemcpyAsync(&bad, f->bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipMemcpyAsync(start.data(), f->start.p, sizeof(int32_t) * start.size(), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    if (bad != ~0ull) {
        srh::set_error("stpwl_fit_add: episode %lld, row %lld of the records is not finite (x or u); nothing was added", (long long)(bad / Tk),
                       (long long)((bad % Tk) * stride));
        return SRH_EINVAL;
    }
    if (start[P] == 0) return SRH_OK;              // T' < 2: no sample
    // the granules: region by region, TF_GRAN chunks of the region's ordered list each
    std::vector<int32_t> gran, gfirst((size_t)P + 1);
    for (int p = 0; p < P; ++p) {
        gfirst[p] = (int32_t)(gran.size() / 3);
        const int cnt = start[p + 1] - start[p];
        for (int at = 0; at < cnt; at += TF_GRAN * TF_TR) {
            gran.push_back(p);
            gran.push_back(start[p] + at);
            gran.push_back(std::min(TF_GRAN * TF_TR, cnt - at));
        }
    }
    const int64_t ngran = (int64_t)(gran.size() / 3);
    gfirst[P] = (int32_t)ngran;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(TF_MAX_BLOCKS, (int64_t)(TF_SCRATCH_BYTES / (sizeof(double) * (size_t)s.len))));
    if ((rc = f->gran.upload(gran.data(), sizeof(int32_t) * gran.size())) || (rc = f->gfirst.upload(gfirst.data(), sizeof(int32_t) * gfirst.size())) ||
        (rc = tf_room(f->part, sizeof(double) * (size_t)std::min(ngran, cap) * (size_t)s.len)))
        return rc;
    TfAccArgs a{};
    a.X = x_dev; a.U = u_dev; a.T = T; a.Tk = Tk; a.stride = stride;
    a.nx = s.nx; a.m = s.m; a.n = s.n; a.ld = s.ld; a.tg = s.tg; a.ntile = s.ntile;
    a.Ts = f->Ts;
    a.xp = f->xp_dev.as<double>(); a.list = f->list.as<int32_t>(); a.gran = f->gran.as<int32_t>(); a.tiles = f->tiles.as<int32_t>();
    a.part = f->part.as<double>();
    // One workgroup per granule, in rounds; after every round the partials join the running sums of their points in granule order
    for (int64_t g0 = 0; g0 < ngran; g0 += cap) {
        const int nb = (int)std::min(cap, ngran - g0);
        a.g0 = g0;
        void *args[] = {&a};
        SRH_CHECK_HIP(hipLaunchKernel(tf_accum_fn(s.ntw), dim3((unsigned)nb), dim3(TF_NT), args, s.lds, st));
        tf_reduce_kernel<<<dim3((unsigned)srh::cdiv(s.len, TF_NT), (unsigned)P), TF_NT, 0, st>>>(a.part, f->gfirst.as<int32_t>(), g0, nb, s.len,
                                                                                                 f->sums.as<double>());
        SRH_CHECK_HIP(hipGetLastError());
    }
    SRH_CHECK_HIP(hipStreamSynchronize(st));      // the work arrays are the handle's: the next call may replace them
    for (int p = 0; p < P; ++p) f->counts[p] += start[p + 1] - start[p];
    return SRH_OK;
}

int stpwl_fit_add(stpwl_fit_t *f, const double *x, const double *u, int64_t E, int64_t T, int stride) {
    SRH_REQUIRE(f, "stpwl_fit_add: null handle");
    SRH_REQUIRE(x && u, "stpwl_fit_add: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "stpwl_fit_add: need E >= 1 episodes of T >= 1 rows");
    SRH_REQUIRE(stride >= 1, "stpwl_fit_add: stride = %d, need stride >= 1", stride);
    srh::DevBuf dx, du;
    int rc;
    if ((rc = dx.upload(x, sizeof(double) * (size_t)E * T * f->s.nx)) || (rc = du.upload(u, sizeof(double) * (size_t)E * T * f->s.m))) return rc;
    return stpwl_fit_add_dev(f, dx.as<double>(), du.as<double>(), E, T, stride, nullptr);
}

int stpwl_fit_counts(stpwl_fit_t *f, int64_t *counts) {
    SRH_REQUIRE(f && counts, "stpwl_fit_counts: null argument");
    std::copy(f->counts.begin(), f->counts.end(), counts);
    return SRH_OK;
}

int stpwl_fit_sums(stpwl_fit_t *f, int p, double *G, double *R, double *Q, int64_t *samples) {
    SRH_REQUIRE(f, "stpwl_fit_sums: null handle");
    SRH_REQUIRE(p >= 0 && p < f->P, "stpwl_fit_sums: point %d is outside 0 .. %d", p, f->P - 1);
    const TfShape &s = f->s;
    if (samples) *samples = f->counts[p];
    if (!G && !R && !Q) return SRH_OK;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> h((size_t)s.len);
    SRH_CHECK_HIP(hipMemcpy(h.data(), f->sums.as<double>() + (size_t)p * s.len, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    const int n = s.n;
    if (G)
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) {
                const double v = h[(size_t)tf_gtile(i >> 4, j >> 4, s.T16) * 256 + (i & 15) * 16 + (j & 15)];
                G[(size_t)i * n + j] = v;
                G[(size_t)j * n + i] = v;
            }
    if (R)
        for (int i = 0; i < s.nx; ++i)
            for (int j = 0; j < n; ++j) R[(size_t)i * n + j] = h[(size_t)(s.NG + (i >> 4) * s.T16 + (j >> 4)) * 256 + (i & 15) * 16 + (j & 15)];
    if (Q) {
        double q = 0.0;
        for (int t = 0; t < 256; ++t) q += h[(size_t)s.ntile * 256 + t];
        *Q = q;
    }
    return SRH_OK;
}

int stpwl_fit_solve(stpwl_fit_t *f, double ridge, int64_t min_samples, double *A_c, double *B_c, double *d_c, double *u, int32_t *status,
                    int32_t *column) {
    SRH_REQUIRE(f, "stpwl_fit_solve: null handle");
    SRH_REQUIRE(A_c && B_c && d_c && u && status && column, "stpwl_fit_solve: null argument");
    SRH_REQUIRE(ridge >= 0.0 && std::isfinite(ridge), "stpwl_fit_solve: need a finite ridge >= 0");
    const TfShape &s = f->s;
    const int P = f->P, n = s.n, nx = s.nx, m = s.m;
    int64_t total = 0;
    for (int p = 0; p < P; ++p) total += f->counts[p];
    SRH_REQUIRE(total > 0, "stpwl_fit_solve: no samples have been added (S = 0)");
    if (min_samples < 0) min_samples = n + 1;
    if (min_samples < 1) min_samples = 1;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    srh::DevBuf cnt, X, um, info;
    int rc;
    if ((rc = cnt.upload(f->counts.data(), sizeof(int64_t) * P)) || (rc = X.alloc(sizeof(double) * (size_t)P * nx * n)) ||
        (rc = um.alloc(sizeof(double) * (size_t)P * m)) || (rc = info.alloc(sizeof(int32_t) * 2 * (size_t)P)))
        return rc;
    TfSolveArgs a{f->sums.as<double>(), s.len, cnt.as<int64_t>(), min_samples, n, nx, m, s.T16, s.NG, ridge, X.as<double>(), um.as<double>(),
                  info.as<int32_t>()};
    tf_solve_kernel<<<(unsigned)P, TF_NT, srh::lds_request(sizeof(double) * (size_t)n * (n + 1) / 2), nullptr>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    std::vector<double> hX((size_t)P * nx * n);
    std::vector<int32_t> hi((size_t)2 * P);
    if ((rc = X.download(hX.data(), sizeof(double) * hX.size())) || (rc = um.download(u, sizeof(double) * (size_t)P * m)) ||
        (rc = info.download(hi.data(), sizeof(int32_t) * hi.size())))
        return rc;
    for (int p = 0; p < P; ++p) {
        status[p] = hi[2 * p];
        column[p] = hi[2 * p + 1];
        const double *xp = f->xp.data() + (size_t)p * nx;
        for (int i = 0; i < nx; ++i) {
            const double *row = hX.data() + ((size_t)p * nx + i) * n;
            std::copy(row, row + nx, A_c + ((size_t)p * nx + i) * nx);
            std::copy(row + nx, row + nx + m, B_c + ((size_t)p * nx + i) * m);
            // d_c = c - A_c x_p, the products by fma in the order j = 0, 1, ..
            double acc = 0.0;
            for (int j = 0; j < nx; ++j) acc = std::fma(row[j], xp[j], acc);
            d_c[(size_t)p * nx + i] = row[n - 1] - acc;
        }
    }
    return SRH_OK;
}

}  // extern "C"
