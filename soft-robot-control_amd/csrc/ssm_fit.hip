// SSM model identification on the device: records (y, u) -> the sums of three polynomial least-squares fits over one regressor ->
// rd_coeff / Bd, r_coeff / B, w_coeff.
//
// THE FIT ("SSM model identification", defines it; the reference ships one trained model and no trainer).
//   Records: E episodes, each y (T x n_y), u (T x m), raw.  `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode; T' = the rows kept.
//   Chart: x_i = V^T (y_i - y_ref), V (n_y x n_x) given (sssm_fit_cov gives the covariance a PCA chart is read from).
//   Samples: the interior rows 1 <= i <= T' - 2 of every episode, never across an episode; T' < 3 contributes nothing.
//   Regressor: Phi_i = [phi(x_i); u_i], phi the monomials of sssm_exponents(n_x, P), P = max(rom_order, ssm_order), no constant;
//   n = nmon(n_x, P) + m.  Row i holds the input applied after y_i.
//   Sums: G = sum Phi_i Phi_i^T, R_d = sum x_{i+1} Phi_i^T, R_c = sum ((x_{i+1} - x_{i-1}) / (2 Ts)) Phi_i^T,
//   R_w = sum (y_i - y_ref) phi(x_i)^T, S = the samples, Q_d, Q_c, Q_w = the squared norms of the three targets.
//   Solves: [rd_coeff Bd] and [r_coeff B] on the columns {monomials up to rom_order} + {inputs}, w_coeff on the monomials up to
//   ssm_order, each block equilibrated by its own diagonal: with D = diag(G_S), (D^-1/2 G_S D^-1/2 + ridge I) z = D^-1/2 r, coeff = D^-1/2 z.
//
// Kernels.  sf_accum_kernel follows kf_accum_kernel (koopman_fit.hip): a workgroup owns a granule, SF_GRAN consecutive chunks of one
// episode; a chunk is SF_TR consecutive samples of one episode and a halo row on each side.  A panel row holds
// [Phi | zeros | targets | zeros] of its kept row: y - y_ref, then x as a compensated dot product (rounded once), the monomials by the parent / variable recurrence, and the targets
// [x_{i+1} | (x_{i+1} - x_{i-1}) / (2 Ts) | y_i - y_ref] read from the neighbouring rows' x.  Both operands of every 16 x 16 tile then
// come from the same panel row: G's upper tiles are Phi-block x Phi-block, the stacked R's tiles target-block x Phi-block, on
// v_mfma_f64_16x16x4_f64 with the panel row as the k index.  The tiles are dealt to the four waves and stay in registers over all the
// chunks of the granule; the granules' partials join the running sums in granule order (sf_reduce_kernel), in rounds of at most
// SF_MAX_BLOCKS.  No floating-point atomics, and a granule map that depends on (T, stride) alone: the same records give the same bits,
// and records split over several add calls at episode boundaries give the bits of one call.  sf_cov_kernel accumulates
// sum (y - y_ref)(y - y_ref)^T the same way on plain FMAs (the pass is n_y^2 per row).  sf_solve_kernel: one workgroup, an index set,
// the equilibration, a packed Cholesky in LDS, the right-hand sides in the lanes of the waves.
//
// The tile map, the reduce and the packed Cholesky have the plan of koopman_fit.hip's and are restated here, not shared: the operand
// addressing (one row, two column blocks), the sums' tail (three squared norms) and the solve (index set, equilibration) differ, and
// the Koopman unit stays byte for byte what its tests pinned.
#include "ssm_host.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dev_la.h"

namespace {

constexpr int SF_TR = 64;                 // samples of a chunk (a multiple of 4: the k step of the MFMA)
constexpr int SF_ROWS = SF_TR + 2;        // panel rows: the samples and a halo row on each side
constexpr int SF_NT = 256;                // threads of every kernel here (4 waves)
constexpr int SF_MAX_N = 128;             // n = nmon + m
constexpr int SF_MAX_NX = 32;             // sssm_create's limit
constexpr int SF_MAX_NY = 64;             // the covariance kernel keeps n_y (n_y + 1) / 2 <= 9 x 256 entries in registers
constexpr int SF_COV_PQ = 9;
constexpr int SF_MAX_BLOCKS = 768;        // workgroups of an accumulate launch
constexpr int SF_GRAN = 8;                // chunks of a granule: the run of one workgroup, and the unit of the reduce
constexpr size_t SF_SCRATCH_BYTES = (size_t)64 << 20;   // bound of the partial-sum scratch
constexpr size_t SF_LDS_MAX = (size_t)160 * 1024;
constexpr int SF_MAX_DEV = 16;
typedef double sf_d4 __attribute__((ext_vector_type(4)));

// Shape of a fit: tiles and strides, stated once for the plan, the handle and the kernels.
struct SfShape {
    int nx, ny, m, P, nmon, nrom, nssm, n, nt;   // nt = 2 nx + ny: rows of the stacked R = [R_d; R_c; R_w]
    int T16;        // 16-column tiles across Phi
    int TT;         // 16-row tiles down the stacked R
    int NG;         // tiles of G on or above the diagonal; R's tiles follow them
    int ntile;
    int ld;         // row stride of the panel: = 16 (mod 32) doubles, so the two rows a half-wave reads fall on different banks
    int tg;         // first column of the targets in a panel row (16 T16)
    int ntw;        // tiles per wave of the kernel instance used
    int64_t len;    // doubles of one set of sums: (ntile + 3) x 256, the last three blocks = the per-thread parts of Q_d, Q_c, Q_w
    size_t lds;     // dynamic LDS of the accumulate kernel
};

int sf_nmon(int dim, int order) { return (int)(ssm_exponents(dim, order).size() / dim); }

SfShape sf_shape(int nx, int ny, int m, int rom_order, int ssm_order) {
    SfShape s{};
    s.nx = nx; s.ny = ny; s.m = m; s.P = std::max(rom_order, ssm_order);
    s.nmon = sf_nmon(nx, s.P); s.nrom = sf_nmon(nx, rom_order); s.nssm = sf_nmon(nx, ssm_order);
    s.n = s.nmon + m; s.nt = 2 * nx + ny;
    s.T16 = (s.n + 15) / 16;
    s.TT = (s.nt + 15) / 16;
    s.NG = s.T16 * (s.T16 + 1) / 2;
    s.ntile = s.NG + s.TT * s.T16;
    s.tg = 16 * s.T16;
    s.ld = 16 * (s.T16 + s.TT);
    if (s.ld % 32 != 16) s.ld += 16;
    const int need = (s.ntile + 3) / 4;
    s.ntw = need <= 4 ? 4 : (need <= 10 ? 10 : (need <= 16 ? 16 : 25));
    s.len = (int64_t)(s.ntile + 3) * 256;
    // the panel; behind it the low parts of y - y_ref (SF_ROWS x ny), V (ny x nx), y_ref (ny) and the table (2 nmon ints)
    s.lds = srh::lds_request(sizeof(double) * ((size_t)SF_ROWS * (size_t)(s.ld + ny) + (size_t)ny * nx + (size_t)ny + (size_t)s.nmon));
    return s;
}

__host__ __device__ inline int sf_gtile(int ti, int tj, int T16) { return ti * T16 - ti * (ti - 1) / 2 + (tj - ti); }

struct SfAccArgs {
    const double *y, *u;          // (E x T x ny), (E x T x m), raw
    int64_t T;                    // samples of an episode
    int64_t spe, cpe, gpe;        // samples, chunks and granules of an episode
    int64_t g0;                   // granule of workgroup 0 of this launch (granules are numbered episode by episode over the add call)
    int stride;
    int nx, ny, m, nmon, n, nt, ld, tg, nlev, ntile;
    double two_ts;
    const double *V, *yref;       // (ny x nx), (ny)
    const int32_t *par, *var, *lev;
    const int32_t *tiles;         // (ntile): column block of the A operand << 8 | column block of the B operand
    double *part;                 // (nblk x (ntile + 3) x 256)
};

// x_j = sum_c V[c][j] (dh[c] + dl[c]) with the products and the running sum kept as unevaluated pairs: the result is the exact sum
// rounded once, up to n_y eps^2 sum |V| |y - y_ref|.  No contraction: an fma formed across the TwoSum would break it
__device__ __forceinline__ double sf_chart_dot(const double *__restrict__ V, int nx, int j, const double *__restrict__ dh,
                                               const double *__restrict__ dl, int ny) {
#pragma clang fp contract(off)
    double sh = 0.0, sl = 0.0;
    for (int c = 0; c < ny; ++c) {
        const double a = V[c * nx + j], h = dh[c];
        const double p = a * h;
        const double pe = __builtin_fma(a, dl[c], __builtin_fma(a, h, -p));   // a (h + l) = p + pe
        const double t = sh + p;
        const double bb = t - sh;
        const double er = (sh - (t - bb)) + (p - bb);                          // sh + p = t + er exactly
        sh = t;
        sl = sl + (er + pe);
    }
    return sh + sl;
}

template <int NTW>
__global__ void __launch_bounds__(SF_NT) sf_accum_kernel(SfAccArgs a) {
    extern __shared__ double sf_smem[];
    const int ld = a.ld, nx = a.nx, ny = a.ny, m = a.m, nmon = a.nmon, n = a.n, nt = a.nt, tg = a.tg;
    double *ps = sf_smem;                           // SF_ROWS x ld: [phi | u | zeros | x+ | xdot | y - y_ref | zeros]
    double *dlo = ps + (size_t)SF_ROWS * ld;        // SF_ROWS x ny: the low parts of y - y_ref
    double *sV = dlo + (size_t)SF_ROWS * ny;        // ny x nx
    double *sref = sV + (size_t)ny * nx;            // ny
    int *spar = reinterpret_cast<int *>(sref + ny), *svar = spar + nmon;
    const int tid = threadIdx.x;
    for (int e = tid; e < ny * nx; e += SF_NT) sV[e] = a.V[e];
    for (int e = tid; e < ny; e += SF_NT) sref[e] = a.yref[e];
    for (int e = tid; e < nmon; e += SF_NT) { spar[e] = a.par[e]; svar[e] = a.var[e]; }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l16 = lane & 15, kk = lane >> 4;
    // the tiles of this wave: A operand row[16 ca + l16], B operand row[16 cb + l16] of panel row k; D row kk + 4 g, column l16
    int offA[NTW], offB[NTW];
    sf_d4 acc[NTW];
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
        const int t = wave + 4 * q;
        const int code = t < a.ntile ? a.tiles[t] : 0;
        offA[q] = 16 * ((code >> 8) & 255);
        offB[q] = 16 * (code & 255);
        acc[q] = sf_d4{0.0, 0.0, 0.0, 0.0};
    }
    // the columns no step below writes (n .. tg - 1 and tg + nt .. ld - 1) are read by the last tiles: zeros, written once
    for (int e = tid; e < SF_ROWS * ld; e += SF_NT) {
        const int c = e % ld;
        if ((c >= n && c < tg) || c >= tg + nt) ps[e] = 0.0;
    }
    double qd = 0.0, qc = 0.0, qw = 0.0;
    // this workgroup's granule: SF_GRAN consecutive chunks of one episode (fewer at the episode's end), whatever the launch holds
    const int64_t gr = a.g0 + blockIdx.x, ep = gr / a.gpe, c0 = (gr - ep * a.gpe) * SF_GRAN, c1 = min(a.cpe, c0 + SF_GRAN);
    for (int64_t ci = c0; ci < c1; ++ci) {
        const int64_t i0 = ci * SF_TR;                                          // kept row of panel row 0 (the first sample is row 1)
        const int np = (int)min((int64_t)SF_TR, a.spe - ci * SF_TR);            // samples of this chunk: panel rows 0 .. np + 1 hold data
        const int64_t s0 = ep * a.T;
        __syncthreads();                                                        // the previous chunk's products have read the panel
        // y - y_ref of the panel rows 0 .. np + 1 as a pair (TwoSum), zeros behind them; four elements per thread and pass
        for (int e0 = tid; e0 < SF_ROWS * ny; e0 += 4 * SF_NT) {
            double raw[4], rf[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * SF_NT;
                const int r = e / ny, el = e - r * ny;
                raw[q] = 0.0; rf[q] = 0.0;
                if (e < SF_ROWS * ny && r <= np + 1) {
                    raw[q] = a.y[(s0 + (i0 + r) * a.stride) * ny + el];
                    rf[q] = sref[el];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = e0 + q * SF_NT;
                if (e < SF_ROWS * ny) {
                    const int r = e / ny, el = e - r * ny;
                    const double d = raw[q] - rf[q];
                    const double t = d - raw[q];
                    ps[r * ld + tg + 2 * nx + el] = d;
                    dlo[e] = (raw[q] - (d - t)) - (rf[q] + t);                  // y - y_ref = d + this, exactly
                }
            }
        }
        // u_i of the samples; the halo rows and the rows behind them carry none
        for (int e = tid; e < SF_ROWS * m; e += SF_NT) {
            const int r = e / m, el = e - r * m;
            ps[r * ld + nmon + el] = (r >= 1 && r <= np) ? a.u[(s0 + (i0 + r) * a.stride) * m + el] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < SF_ROWS * nx; e += SF_NT) {
            const int r = e / nx, j = e - r * nx;
            ps[r * ld + j] = sf_chart_dot(sV, nx, j, ps + r * ld + tg + 2 * nx, dlo + r * ny, ny);
        }
        __syncthreads();
        // the targets of the samples from the neighbouring rows' x; zeros on the other rows
        for (int e = tid; e < SF_ROWS * 2 * nx; e += SF_NT) {
            const int r = e / (2 * nx), cc = e - r * 2 * nx;
            double v = 0.0;
            if (r >= 1 && r <= np) {
                const int j = cc < nx ? cc : cc - nx;
                const double xp = ps[(r + 1) * ld + j];
                v = cc < nx ? xp : (xp - ps[(r - 1) * ld + j]) / a.two_ts;
            }
            ps[r * ld + tg + cc] = v;
        }
        // the monomials above degree 1: phi_k = phi_parent x_var (the degree-1 monomials are x itself, in order)
        for (int L = 1; L < a.nlev; ++L) {
            const int k0 = a.lev[L], nk = a.lev[L + 1] - k0;
            for (int e = tid; e < SF_ROWS * nk; e += SF_NT) {
                const int r = e / nk, k = k0 + (e - r * nk);
                ps[r * ld + k] = ps[r * ld + spar[k]] * ps[r * ld + svar[k]];
            }
            __syncthreads();
        }
        __syncthreads();
        // the targets' squared norms over panel rows 1 .. np, a fixed share per thread
        for (int e = tid; e < np * nt; e += SF_NT) {
            const int r = e / nt, cc = e - r * nt;
            const double v = ps[(r + 1) * ld + tg + cc];
            if (cc < nx) qd = fma(v, v, qd);
            else if (cc < 2 * nx) qc = fma(v, v, qc);
            else qw = fma(v, v, qw);
        }
        const int ksteps = (np + 3) >> 2;
        for (int s = 0; s < ksteps; ++s) {
            const int r = 1 + 4 * s + kk;                // <= 64 < SF_ROWS
            const bool live = r <= np;                   // the rows behind the samples are no sample: their B operand is zero
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
    double *dst = a.part + (size_t)blockIdx.x * (size_t)(a.ntile + 3) * 256;
#pragma unroll
    for (int q = 0; q < NTW; ++q) {
        const int t = wave + 4 * q;
        if (t < a.ntile) {
#pragma unroll
            for (int g = 0; g < 4; ++g) dst[(size_t)t * 256 + (kk + 4 * g) * 16 + l16] = acc[q][g];
        }
    }
    dst[(size_t)a.ntile * 256 + tid] = qd;
    dst[(size_t)(a.ntile + 1) * 256 + tid] = qc;
    dst[(size_t)(a.ntile + 2) * 256 + tid] = qw;
}

// sums += the partials of the workgroups, in workgroup order
__global__ void __launch_bounds__(SF_NT) sf_reduce_kernel(const double *__restrict__ part, int nblk, int64_t len, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * SF_NT + threadIdx.x;
    if (i >= len) return;
    double v = sums[i];
    for (int b = 0; b < nblk; ++b) v += part[(int64_t)b * len + i];
    sums[i] = v;
}

// part[block][p] = sum over the block's kept rows of d_i d_j, d = y - y_ref, p the packed upper pair (i <= j) of thread and slot
__global__ void __launch_bounds__(SF_NT) sf_cov_kernel(const double *__restrict__ y, int64_t T, int64_t Tk, int64_t rows, int stride, int ny,
                                                       const double *__restrict__ yref, int64_t rpb, int64_t len, double *__restrict__ part) {
    __shared__ double d[SF_TR * SF_MAX_NY];
    const int tid = threadIdx.x, npair = ny * (ny + 1) / 2;
    int pi[SF_COV_PQ], pj[SF_COV_PQ];
    double acc[SF_COV_PQ];
#pragma unroll
    for (int q = 0; q < SF_COV_PQ; ++q) {
        int p = tid + SF_NT * q, i = 0;
        const bool in = p < npair;
        if (in) while (p >= ny - i) { p -= ny - i; ++i; }
        pi[q] = in ? i : 0; pj[q] = in ? i + p : 0;
        acc[q] = 0.0;
    }
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(rows, r0 + rpb);
    for (int64_t rb = r0; rb < r1; rb += SF_TR) {
        const int nr = (int)min((int64_t)SF_TR, r1 - rb);
        __syncthreads();
        for (int e = tid; e < nr * ny; e += SF_NT) {
            const int r = e / ny, el = e - r * ny;
            const int64_t g = rb + r, ep = g / Tk, i = g - ep * Tk;
            d[e] = y[(ep * T + i * stride) * ny + el] - yref[el];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SF_COV_PQ; ++q) {
            if (tid + SF_NT * q < npair) {
                double s = acc[q];
                for (int r = 0; r < nr; ++r) s = fma(d[r * ny + pi[q]], d[r * ny + pj[q]], s);
                acc[q] = s;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SF_COV_PQ; ++q)
        if (tid + SF_NT * q < npair) part[(int64_t)blockIdx.x * len + tid + SF_NT * q] = acc[q];
}

struct SfSolveArgs {
    const double *sums;
    const int32_t *idx;   // (ns) ascending columns of Phi: the block G_S
    int ns, T16, NG;
    int row0, nrows;      // rows row0 .. row0 + nrows - 1 of the stacked R
    double ridge;
    double *X;            // (nrows x ns)
    int32_t *info;        // -1, the failing position in idx, or ns (a non-finite entry in the solution that no pivot caught)
};

__device__ __forceinline__ double sf_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(SF_NT) sf_solve_kernel(SfSolveArgs a) {
    extern __shared__ double sf_L[];             // packed lower triangle: (i, j), j <= i, at i (i + 1) / 2 + j
    __shared__ int bad, nonfinite;
    __shared__ double sf_dinv[SF_MAX_N];         // D^-1/2
    __shared__ int sf_idx[SF_MAX_N];
    const int ns = a.ns, T16 = a.T16, tid = threadIdx.x;
    if (tid == 0) { bad = ns; nonfinite = 0; }
    __syncthreads();
    for (int i = tid; i < ns; i += SF_NT) {
        const int c = a.idx[i];
        sf_idx[i] = c;
        const double g = a.sums[(size_t)sf_gtile(c >> 4, c >> 4, T16) * 256 + (c & 15) * 17];
        // a diagonal entry that is not positive and finite cannot be scaled: the first one is reported as the pivot
        if (!(g > 0.0) || !(g < INFINITY)) atomicMin(&bad, i);
        sf_dinv[i] = 1.0 / sqrt(g);
    }
    __syncthreads();
    if (bad < ns) {
        if (tid == 0) *a.info = bad;
        return;
    }
    for (int e = tid; e < ns * ns; e += SF_NT) {
        const int i = e / ns, j = e - i * ns;
        if (j > i) continue;
        // G[ci][cj] = G[cj][ci], cj <= ci, held in the tile on or above the diagonal; the scaled block has a unit diagonal exactly
        const int ci = sf_idx[i], cj = sf_idx[j];
        const double g = a.sums[(size_t)sf_gtile(cj >> 4, ci >> 4, T16) * 256 + (cj & 15) * 16 + (ci & 15)];
        sf_L[i * (i + 1) / 2 + j] = i == j ? 1.0 + a.ridge : g * sf_dinv[i] * sf_dinv[j];
    }
    __syncthreads();
    const double floor_ = ns * 2.220446049250313e-16 * (1.0 + a.ridge);
    int fail = -1;
    for (int j = 0; j < ns; ++j) {
        const double d = sf_L[j * (j + 1) / 2 + j];
        // a pivot that the elimination has brought down to the rounding level of its diagonal entry (ns eps of it) is not positive:
        // its sign is noise.  The same value in every thread
        if (!(d > floor_) || !(d < INFINITY)) { fail = j; break; }
        const double ljj = sqrt(d);
        __syncthreads();
        for (int i = j + tid; i < ns; i += SF_NT) {
            const int at = i * (i + 1) / 2 + j;
            sf_L[at] = i == j ? ljj : sf_L[at] / ljj;
        }
        __syncthreads();
        const int w = ns - j - 1;
        for (int e = tid; e < w * w; e += SF_NT) {
            const int i = j + 1 + e / w, k = j + 1 + (e - (e / w) * w);
            if (k > i) continue;
            const int at = i * (i + 1) / 2 + k;
            sf_L[at] = fma(-sf_L[i * (i + 1) / 2 + j], sf_L[k * (k + 1) / 2 + j], sf_L[at]);
        }
        __syncthreads();
    }
    if (fail >= 0) {
        if (tid == 0) *a.info = fail;
        return;
    }
    // row r of X: (L L^T) z = D^-1/2 R[row0 + r][idx]^T, x = D^-1/2 z; the lanes of a wave hold entries lane and lane + 64
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i0 = lane, i1 = lane + 64;
    for (int r = wave; r < a.nrows; r += SF_NT / 64) {
        const int rr = a.row0 + r;
        const size_t rb = (size_t)(a.NG + (rr >> 4) * T16) * 256 + (rr & 15) * 16;
        const int g0 = i0 < ns ? sf_idx[i0] : 0, g1 = i1 < ns ? sf_idx[i1] : 0;
        double x0 = i0 < ns ? a.sums[rb + (size_t)(g0 >> 4) * 256 + (g0 & 15)] * sf_dinv[i0] : 0.0;
        double x1 = i1 < ns ? a.sums[rb + (size_t)(g1 >> 4) * 256 + (g1 & 15)] * sf_dinv[i1] : 0.0;
        for (int j = 0; j < ns; ++j) {
            const double zj = sf_lane(j < 64 ? x0 : x1, j & 63) / sf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = zj;
            if (i1 == j) x1 = zj;
            if (i0 > j && i0 < ns) x0 = fma(-sf_L[i0 * (i0 + 1) / 2 + j], zj, x0);
            if (i1 > j && i1 < ns) x1 = fma(-sf_L[i1 * (i1 + 1) / 2 + j], zj, x1);
        }
        for (int j = ns - 1; j >= 0; --j) {
            const double xj = sf_lane(j < 64 ? x0 : x1, j & 63) / sf_L[j * (j + 1) / 2 + j];
            if (i0 == j) x0 = xj;
            if (i1 == j) x1 = xj;
            if (i0 < j) x0 = fma(-sf_L[j * (j + 1) / 2 + i0], xj, x0);
            if (i1 < j) x1 = fma(-sf_L[j * (j + 1) / 2 + i1], xj, x1);
        }
        if (i0 < ns) {
            x0 *= sf_dinv[i0];
            a.X[(size_t)r * ns + i0] = x0;
            if (!(fabs(x0) < INFINITY)) atomicOr(&nonfinite, 1);
        }
        if (i1 < ns) {
            x1 *= sf_dinv[i1];
            a.X[(size_t)r * ns + i1] = x1;
            if (!(fabs(x1) < INFINITY)) atomicOr(&nonfinite, 1);
        }
    }
    __syncthreads();
    if (tid == 0) *a.info = nonfinite ? ns : -1;
}

const void *sf_accum_fn(int ntw) {
    switch (ntw) {
        case 4: return (const void *)sf_accum_kernel<4>;
        case 10: return (const void *)sf_accum_kernel<10>;
        case 16: return (const void *)sf_accum_kernel<16>;
        default: return (const void *)sf_accum_kernel<25>;
    }
}

// the dynamic-LDS limit of a kernel on the current device, raised once per device to the largest request seen
int sf_grant_lds(const void *fn, int slot, size_t bytes) {
    static std::mutex mu;
    static size_t granted[SF_MAX_DEV][5] = {};
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    SRH_CHECK_HIP(hipGetDevice(&dev));
    const bool known = dev >= 0 && dev < SF_MAX_DEV;       // the attribute is the device's: a device beyond the table is set every time
    if (known && granted[dev][slot] >= bytes) return SRH_OK;
    SRH_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known) granted[dev][slot] = bytes;
    return SRH_OK;
}

int sf_slot(int ntw) { return ntw == 4 ? 0 : (ntw == 10 ? 1 : (ntw == 16 ? 2 : 3)); }

int64_t sf_kept_rows(int64_t T, int stride) { return (T - 1) / stride + 1; }

// "x1^2 x3" or "u2": the name of column c of Phi
std::string sf_column_name(const std::vector<int> &exps, int nx, int nmon, int c) {
    if (c >= nmon) return "input u" + std::to_string(c - nmon + 1);
    std::string s = "monomial";
    for (int i = 0; i < nx; ++i) {
        const int e = exps[(size_t)c * nx + i];
        if (e == 0) continue;
        s += " x" + std::to_string(i + 1);
        if (e > 1) s += "^" + std::to_string(e);
    }
    return s;
}

}  // namespace

struct sssm_fit {
    SfShape s{};
    int rom_order = 0, ssm_order = 0, nlev = 0;
    double Ts = 0.0;
    int64_t samples = 0;
    std::vector<int> exps;         // (nmon x nx)
    std::vector<int32_t> idx_dyn, idx_w;
    srh::DevBuf sums, part, tiles, V, yref, par, var, lev, idx, X, info;
};

static int sf_check_shape(const char *who, int n_x, int n_y, int m, int rom_order, int ssm_order) {
    SRH_REQUIRE(n_x > 0 && n_y > 0 && m > 0 && rom_order > 0 && ssm_order > 0, "%s: need n_x, n_y, m, rom_order, ssm_order > 0", who);
    SRH_REQUIRE(n_x <= SF_MAX_NX && rom_order <= SSM_MAX_ORDER && ssm_order <= SSM_MAX_ORDER,
                "%s: need n_x <= %d and orders <= %d (sssm_create's limits), got n_x = %d, orders %d and %d", who, SF_MAX_NX, SSM_MAX_ORDER, n_x,
                rom_order, ssm_order);
    SRH_REQUIRE(n_x <= n_y, "%s: the chart V (n_y x n_x) needs n_x <= n_y, got n_x = %d, n_y = %d", who, n_x, n_y);
    SRH_REQUIRE(n_y <= SF_MAX_NY, "%s: n_y = %d exceeds the limit n_y <= %d", who, n_y, SF_MAX_NY);
    // the monomial count without building the table: C(n_x + P, P) - 1 (at most C(39, 7) under the limits above)
    const int P = std::max(rom_order, ssm_order);
    int64_t cnt = 1;
    for (int k = 1; k <= P; ++k) cnt = cnt * (n_x + k) / k;
    SRH_REQUIRE(cnt - 1 + m <= SF_MAX_N, "%s: n = nmon + m = %lld + %d = %lld exceeds the limit n <= %d (n_x = %d, order %d)", who,
                (long long)(cnt - 1), m, (long long)(cnt - 1 + m), SF_MAX_N, n_x, P);
    return SRH_OK;
}

// C (ny x ny) += sum over the kept rows of (y - y_ref)(y - y_ref)^T of device records; synchronises `st`
static int sf_cov_dev(const double *y_dev, int64_t E, int64_t T, int ny, int stride, const double *yref_host, hipStream_t st, double *C,
                      int64_t *count) {
    const int64_t Tk = sf_kept_rows(T, stride), rows = E * Tk;
    const int nblk = (int)std::min<int64_t>(SF_MAX_BLOCKS, srh::cdiv(rows, SF_TR));
    const int64_t rpb = srh::cdiv(srh::cdiv(rows, nblk), SF_TR) * SF_TR;
    const int64_t len = (int64_t)ny * (ny + 1) / 2;
    srh::DevBuf part, out, ref;
    int rc;
    if ((rc = part.alloc(sizeof(double) * (size_t)nblk * len)) || (rc = out.alloc(sizeof(double) * (size_t)len)) ||
        (rc = ref.upload(yref_host, sizeof(double) * ny)))
        return rc;
    SRH_CHECK_HIP(hipMemsetAsync(out.p, 0, out.bytes, st));       // every workgroup writes its part, one that owns no row zeros
    sf_cov_kernel<<<(unsigned)nblk, SF_NT, 0, st>>>(y_dev, T, Tk, rows, stride, ny, ref.as<double>(), rpb, len, part.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    sf_reduce_kernel<<<(unsigned)srh::cdiv(len, SF_NT), SF_NT, 0, st>>>(part.as<double>(), nblk, len, out.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    std::vector<double> h((size_t)len);
    SRH_CHECK_HIP(hipMemcpyAsync(h.data(), out.p, sizeof(double) * len, hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    size_t p = 0;
    for (int i = 0; i < ny; ++i)
        for (int j = i; j < ny; ++j, ++p) {
            C[(size_t)i * ny + j] = h[p];
            C[(size_t)j * ny + i] = h[p];
        }
    if (count) *count = rows;
    return SRH_OK;
}

extern "C" {

int sssm_fit_plan(int n_x, int n_y, int m, int rom_order, int ssm_order, int *n_mon, int *n, int *rows_per_chunk, int64_t *lds_bytes) {
    if (n_mon) *n_mon = 0;
    if (n) *n = 0;
    if (rows_per_chunk) *rows_per_chunk = 0;
    if (lds_bytes) *lds_bytes = 0;
    int rc;
    if ((rc = sf_check_shape("sssm_fit_plan", n_x, n_y, m, rom_order, ssm_order))) return rc;
    const SfShape s = sf_shape(n_x, n_y, m, rom_order, ssm_order);
    SRH_REQUIRE(s.lds <= SF_LDS_MAX, "sssm_fit_plan: the panel of n = %d regressors and 2 n_x + n_y = %d targets needs %zu bytes of LDS, above %zu",
                s.n, s.nt, s.lds, SF_LDS_MAX);
    if (n_mon) *n_mon = s.nmon;
    if (n) *n = s.n;
    if (rows_per_chunk) *rows_per_chunk = SF_TR;
    if (lds_bytes) *lds_bytes = (int64_t)s.lds;
    return SRH_OK;
}

int sssm_fit_create(sssm_fit_t **out, int n_x, int n_y, int m, int rom_order, int ssm_order, double Ts, const double *V, const double *y_ref) {
    SRH_REQUIRE(out && V, "sssm_fit_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(Ts > 0.0 && std::isfinite(Ts), "sssm_fit_create: need a finite Ts > 0");
    int rc;
    if ((rc = sssm_fit_plan(n_x, n_y, m, rom_order, ssm_order, nullptr, nullptr, nullptr, nullptr))) return rc;
    for (int e = 0; e < n_y * n_x; ++e) SRH_REQUIRE(std::isfinite(V[e]), "sssm_fit_create: V holds a non-finite entry");
    for (int e = 0; y_ref && e < n_y; ++e) SRH_REQUIRE(std::isfinite(y_ref[e]), "sssm_fit_create: y_ref holds a non-finite entry");
    auto *f = new sssm_fit();
    auto fail = [&](int code) { delete f; return code; };
    f->s = sf_shape(n_x, n_y, m, rom_order, ssm_order);
    f->rom_order = rom_order; f->ssm_order = ssm_order; f->Ts = Ts;
    const SfShape &s = f->s;
    f->exps = ssm_exponents(n_x, s.P);
    // parent / variable of every monomial and the first index of every degree (as ssm.hip's evaluation tables)
    std::map<std::vector<int>, int> index;
    for (int j = 0; j < s.nmon; ++j) index[std::vector<int>(f->exps.begin() + (size_t)j * n_x, f->exps.begin() + (size_t)(j + 1) * n_x)] = j;
    std::vector<int32_t> par(s.nmon), var(s.nmon), lev;
    int prev = 0;
    for (int j = 0; j < s.nmon; ++j) {
        std::vector<int> e(f->exps.begin() + (size_t)j * n_x, f->exps.begin() + (size_t)(j + 1) * n_x);
        int deg = 0, last = 0;
        for (int i = 0; i < n_x; ++i) { deg += e[i]; if (e[i] > 0) last = i; }
        if (deg != prev) { lev.push_back(j); prev = deg; }
        var[j] = last;
        if (deg == 1) { par[j] = -1; continue; }
        e[last] -= 1;
        par[j] = index.at(e);
    }
    lev.push_back(s.nmon);
    f->nlev = (int)lev.size() - 1;
    std::vector<int32_t> tiles;
    for (int ti = 0; ti < s.T16; ++ti)
        for (int tj = ti; tj < s.T16; ++tj) tiles.push_back((ti << 8) | tj);
    for (int ti = 0; ti < s.TT; ++ti)
        for (int tj = 0; tj < s.T16; ++tj) tiles.push_back(((s.T16 + ti) << 8) | tj);
    for (int k = 0; k < s.nrom; ++k) f->idx_dyn.push_back(k);
    for (int k = 0; k < m; ++k) f->idx_dyn.push_back(s.nmon + k);
    for (int k = 0; k < s.nssm; ++k) f->idx_w.push_back(k);
    std::vector<double> zero(n_y, 0.0);
    const size_t solve_lds = srh::lds_request(sizeof(double) * (size_t)s.n * (s.n + 1) / 2);
    if ((rc = f->tiles.upload(tiles.data(), sizeof(int32_t) * tiles.size())) || (rc = f->sums.alloc(sizeof(double) * (size_t)s.len)) ||
        (rc = f->V.upload(V, sizeof(double) * (size_t)n_y * n_x)) || (rc = f->yref.upload(y_ref ? y_ref : zero.data(), sizeof(double) * n_y)) ||
        (rc = f->par.upload(par.data(), sizeof(int32_t) * par.size())) || (rc = f->var.upload(var.data(), sizeof(int32_t) * var.size())) ||
        (rc = f->lev.upload(lev.data(), sizeof(int32_t) * lev.size())) || (rc = f->idx.alloc(sizeof(int32_t) * SF_MAX_N)) ||
        (rc = f->X.alloc(sizeof(double) * (size_t)SF_MAX_N * SF_MAX_N)) || (rc = f->info.alloc(sizeof(int32_t))) ||
        (rc = sf_grant_lds(sf_accum_fn(s.ntw), sf_slot(s.ntw), s.lds)) || (rc = sf_grant_lds((const void *)sf_solve_kernel, 4, solve_lds)))
        return fail(rc);
    if (hipMemset(f->sums.p, 0, f->sums.bytes) != hipSuccess) { srh::set_error("sssm_fit_create: hipMemset failed"); return fail(SRH_EHIP); }
    *out = f;
    return SRH_OK;
}

int sssm_fit_destroy(sssm_fit_t *f) {
    SRH_REQUIRE(f, "sssm_fit_destroy: null handle");
    (void)hipDeviceSynchronize();
    delete f;
    return SRH_OK;
}

int sssm_fit_reset(sssm_fit_t *f) {
    SRH_REQUIRE(f, "sssm_fit_reset: null handle");
    SRH_CHECK_HIP(hipDeviceSynchronize());
    SRH_CHECK_HIP(hipMemset(f->sums.p, 0, f->sums.bytes));
    f->samples = 0;
    return SRH_OK;
}

int sssm_fit_cov_dev(const double *y_dev, int64_t E, int64_t T, int n_y, int stride, const double *y_ref, double *C, int64_t *count,
                     void *stream) {
    SRH_REQUIRE(y_dev && C, "sssm_fit_cov_dev: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1 && n_y >= 1, "sssm_fit_cov_dev: need E, T, n_y >= 1");
    SRH_REQUIRE(n_y <= SF_MAX_NY, "sssm_fit_cov_dev: n_y = %d exceeds the limit n_y <= %d", n_y, SF_MAX_NY);
    SRH_REQUIRE(stride >= 1, "sssm_fit_cov_dev: stride = %d, need stride >= 1", stride);
    std::vector<double> zero(n_y, 0.0);
    return sf_cov_dev(y_dev, E, T, n_y, stride, y_ref ? y_ref : zero.data(), (hipStream_t)stream, C, count);
}

int sssm_fit_cov(const double *y, int64_t E, int64_t T, int n_y, int stride, const double *y_ref, double *C, int64_t *count) {
    SRH_REQUIRE(y && C, "sssm_fit_cov: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1 && n_y >= 1, "sssm_fit_cov: need E, T, n_y >= 1");
    SRH_REQUIRE(n_y <= SF_MAX_NY, "sssm_fit_cov: n_y = %d exceeds the limit n_y <= %d", n_y, SF_MAX_NY);
    SRH_REQUIRE(stride >= 1, "sssm_fit_cov: stride = %d, need stride >= 1", stride);
    srh::DevBuf dy;
    int rc;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)E * T * n_y))) return rc;
    return sssm_fit_cov_dev(dy.as<double>(), E, T, n_y, stride, y_ref, C, count, nullptr);
}

int sssm_fit_add_dev(sssm_fit_t *f, const double *y_dev, const double *u_dev, int64_t E, int64_t T, int stride, void *stream) {
    SRH_REQUIRE(f, "sssm_fit_add_dev: null handle");
    SRH_REQUIRE(y_dev && u_dev, "sssm_fit_add_dev: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "sssm_fit_add_dev: need E >= 1 episodes of T >= 1 samples");
    SRH_REQUIRE(stride >= 1, "sssm_fit_add_dev: stride = %d, need stride >= 1", stride);
    const SfShape &s = f->s;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t Tk = sf_kept_rows(T, stride);
    const int64_t spe = Tk - 2;
    if (spe <= 0) return SRH_OK;                  // T' < 3: no interior row
    SfAccArgs a{};
    a.y = y_dev; a.u = u_dev; a.T = T; a.spe = spe; a.cpe = srh::cdiv(spe, SF_TR); a.gpe = srh::cdiv(a.cpe, SF_GRAN);
    a.stride = stride;
    a.nx = s.nx; a.ny = s.ny; a.m = s.m; a.nmon = s.nmon; a.n = s.n; a.nt = s.nt; a.ld = s.ld; a.tg = s.tg; a.nlev = f->nlev; a.ntile = s.ntile;
    a.two_ts = 2.0 * f->Ts;
    a.V = f->V.as<double>(); a.yref = f->yref.as<double>();
    a.par = f->par.as<int32_t>(); a.var = f->var.as<int32_t>(); a.lev = f->lev.as<int32_t>();
    a.tiles = f->tiles.as<int32_t>();
    // One workgroup per granule, in rounds of as many as the scratch bound and the launch bound admit; after every round the partials
    // join the running sums in granule order.  A granule's partial depends on its own episode alone and the chain of additions runs
    // over the granules in order whatever the rounds are: records split over several calls at episode boundaries give the bits of one
    const int64_t ngran = E * a.gpe;
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(SF_MAX_BLOCKS, (int64_t)(SF_SCRATCH_BYTES / (sizeof(double) * (size_t)s.len))));
    const size_t need = sizeof(double) * (size_t)std::min(ngran, cap) * (size_t)s.len;
    if (need > f->part.bytes) {
        SRH_CHECK_HIP(hipStreamSynchronize(st));   // an earlier launch may still read the block that is replaced
        int rc = f->part.alloc(need);
        if (rc) return rc;
    }
    a.part = f->part.as<double>();
    for (int64_t g0 = 0; g0 < ngran; g0 += cap) {
        const int nblk = (int)std::min(cap, ngran - g0);
        a.g0 = g0;
        void *args[] = {&a};
        SRH_CHECK_HIP(hipLaunchKernel(sf_accum_fn(s.ntw), dim3((unsigned)nblk), dim3(SF_NT), args, s.lds, st));
        sf_reduce_kernel<<<(unsigned)srh::cdiv(s.len, SF_NT), SF_NT, 0, st>>>(a.part, nblk, s.len, f->sums.as<double>());
        SRH_CHECK_HIP(hipGetLastError());
    }
    f->samples += E * spe;
    return SRH_OK;
}

int sssm_fit_add(sssm_fit_t *f, const double *y, const double *u, int64_t E, int64_t T, int stride) {
    SRH_REQUIRE(f, "sssm_fit_add: null handle");
    SRH_REQUIRE(y && u, "sssm_fit_add: null argument");
    SRH_REQUIRE(E >= 1 && T >= 1, "sssm_fit_add: need E >= 1 episodes of T >= 1 samples");
    SRH_REQUIRE(stride >= 1, "sssm_fit_add: stride = %d, need stride >= 1", stride);
    srh::DevBuf dy, du;
    int rc;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)E * T * f->s.ny)) || (rc = du.upload(u, sizeof(double) * (size_t)E * T * f->s.m))) return rc;
    if ((rc = sssm_fit_add_dev(f, dy.as<double>(), du.as<double>(), E, T, stride, nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return SRH_OK;
}

int sssm_fit_sums(sssm_fit_t *f, double *G, double *Rd, double *Rc, double *Rw, double *Q, int64_t *samples) {
    SRH_REQUIRE(f, "sssm_fit_sums: null handle");
    const SfShape &s = f->s;
    if (samples) *samples = f->samples;
    if (!G && !Rd && !Rc && !Rw && !Q) return SRH_OK;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    std::vector<double> h((size_t)s.len);
    int rc = f->sums.download(h.data(), sizeof(double) * h.size());
    if (rc) return rc;
    const int n = s.n;
    if (G)
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) {
                const double v = h[(size_t)sf_gtile(i >> 4, j >> 4, s.T16) * 256 + (i & 15) * 16 + (j & 15)];
                G[(size_t)i * n + j] = v;
                G[(size_t)j * n + i] = v;
            }
    auto rows = [&](double *dst, int row0, int nrows, int ncols) {
        for (int i = 0; i < nrows; ++i)
            for (int j = 0; j < ncols; ++j) {
                const int r = row0 + i;
                dst[(size_t)i * ncols + j] = h[(size_t)(s.NG + (r >> 4) * s.T16 + (j >> 4)) * 256 + (r & 15) * 16 + (j & 15)];
            }
    };
    if (Rd) rows(Rd, 0, s.nx, n);
    if (Rc) rows(Rc, s.nx, s.nx, n);
    if (Rw) rows(Rw, 2 * s.nx, s.ny, s.nmon);
    if (Q)
        for (int k = 0; k < 3; ++k) {
            double q = 0.0;
            for (int t = 0; t < 256; ++t) q += h[(size_t)(s.ntile + k) * 256 + t];
            Q[k] = q;
        }
    return SRH_OK;
}

// one block: X (nrows x ns) of the rows row0 .. of the stacked R on the index set idx
static int sf_solve_block(sssm_fit_t *f, const char *what, const std::vector<int32_t> &idx, int row0, int nrows, double ridge, double *X,
                          int32_t *info) {
    const SfShape &s = f->s;
    const int ns = (int)idx.size();
    SRH_CHECK_HIP(hipMemcpy(f->idx.p, idx.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice));
    SfSolveArgs a{f->sums.as<double>(), f->idx.as<int32_t>(), ns, s.T16, s.NG, row0, nrows, ridge, f->X.as<double>(), f->info.as<int32_t>()};
    sf_solve_kernel<<<1, SF_NT, srh::lds_request(sizeof(double) * (size_t)ns * (ns + 1) / 2), nullptr>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    int32_t bad = -1;
    int rc = f->info.download(&bad, sizeof(int32_t));
    if (rc) return rc;
    if (bad >= 0 && bad < ns) {
        if (info) { info[0] = bad; info[1] = idx[bad]; }
        srh::set_error("sssm_fit_solve: pivot %d of the equilibrated %s block (%d columns, ridge = %g) is not positive (above n eps of its "
                       "diagonal entry) or not finite: column %d of Phi, %s: increase ridge", bad, what, ns, ridge, idx[bad],
                       sf_column_name(f->exps, s.nx, s.nmon, idx[bad]).c_str());
        return SRH_ENUMERIC;
    }
    if (bad >= ns) {
        if (info) { info[0] = ns; info[1] = -1; }
        srh::set_error("sssm_fit_solve: the %s solution holds a non-finite entry (a non-finite value of the sums that no pivot caught)", what);
        return SRH_ENUMERIC;
    }
    return f->X.download(X, sizeof(double) * (size_t)nrows * ns);
}

int sssm_fit_solve(sssm_fit_t *f, double ridge, double *rd_coeff, double *Bd, double *r_coeff, double *B, double *w_coeff, int32_t *info) {
    SRH_REQUIRE(f, "sssm_fit_solve: null handle");
    if (info) { info[0] = -1; info[1] = -1; }
    SRH_REQUIRE(rd_coeff && Bd && r_coeff && B && w_coeff, "sssm_fit_solve: null argument");
    SRH_REQUIRE(ridge >= 0.0 && std::isfinite(ridge), "sssm_fit_solve: need a finite ridge >= 0");
    SRH_REQUIRE(f->samples > 0, "sssm_fit_solve: no samples have been added (S = 0)");
    const SfShape &s = f->s;
    SRH_CHECK_HIP(hipDeviceSynchronize());
    const int nd = s.nrom + s.m;
    std::vector<double> X((size_t)2 * s.nx * nd);
    int rc;
    // [rd_coeff Bd] and [r_coeff B] share the block: one factorisation, 2 n_x right-hand sides
    if ((rc = sf_solve_block(f, "dynamics", f->idx_dyn, 0, 2 * s.nx, ridge, X.data(), info))) return rc;
    for (int i = 0; i < s.nx; ++i) {
        const double *xd = X.data() + (size_t)i * nd, *xc = X.data() + (size_t)(s.nx + i) * nd;
        std::copy(xd, xd + s.nrom, rd_coeff + (size_t)i * s.nrom);
        std::copy(xd + s.nrom, xd + nd, Bd + (size_t)i * s.m);
        std::copy(xc, xc + s.nrom, r_coeff + (size_t)i * s.nrom);
        std::copy(xc + s.nrom, xc + nd, B + (size_t)i * s.m);
    }
    return sf_solve_block(f, "observation", f->idx_w, 2 * s.nx, s.ny, ridge, w_coeff, info);
}

}  // extern "C"
