// TPWL models: the k-step prediction error over records on the device (the open-loop model check of the reference,
// examples/hardware/diamond.py:20-73 TPWL_rollout, as a unit that reads the records in place).
//
// THE HORIZON ERROR ("TPWL horizon error", defines it).
//   Records: E episodes X (E x T x n_x), U (E x T x m) as the fit defines them (row i holds the input applied after x_i); `stride`
//   s >= 1 keeps rows 0, s, 2s, .. (T' kept rows).
//   Windows: starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, numbered episode by
//   episode in row order; an episode with T' <= H has none.
//   Prediction of a window: xh_0 = x_{j0}; xh_{k+1} = THE STEP RULE of tpwl_dev.h applied to (xh_k, u_{j0+k}) with THE POINT-SEARCH RULE
//   of the same file, k = 0 .. H - 1: what stpwl_rollout computes from (x_{j0}, U[j0 : j0 + H]), bit for bit.
//   Errors: e_k = xh_k - x_{j0+k}; with an output model ez_k = H e_k (z_ref cancels).
//   Window status: 0 ok; 1 some xh_k is not finite; 2 some record row the window reads (the states j0 .. j0 + H, the inputs
//   j0 .. j0 + H - 1) is not finite; 2 wins over 1.  Only status-0 windows enter the sums and the maxima.
//   Results for k = 0 .. H: sse_x[k] = sum_w |e_k|^2, sse_z[k]; worst_x[k] = max_w |e_k|_2 with the window that attains it (ties: the
//   lowest window number); the counts of status-1 and status-2 windows.  Row 0 is exactly 0.
//
// Arithmetic of the norms (one wave, fixed): lane l sums e_j^2 over j = l, l + 64, .. by fma from 0.0, the 64 lane sums join in
// wg::wave_sum's fixed tree; ez_a is the same sum of H[a][j] e_j, and |ez|^2 = fma(ez_a, ez_a, .) over a = 0, 1, ..  A norm is the
// correctly rounded sqrt of its square.
//
// Kernels.  th_window_kernel: a workgroup of 256 threads takes one block of consecutive windows of one episode (`block` windows, the
// plan's).  Per step it runs the sequence of rollout_staged_kernel (tpwl.hip) at the same 256 threads, so the slice layout and with it
// every bit of xh is the rollout kernel's: the search on wave 0 (tpwl::nearest_wave, or the HELD register table under
// tpwl::nearest_many's limits), tpwl::panel_load only when the point changes -- consecutive windows mostly keep their panel --
// tpwl::step_slices, the barrier, tpwl::step_sum.  The input row (wave 1) and the record row to compare with (threads t < n) are
// requested before the products.  Threads t < n form e = v - x_rec[t]; wave 3 turns the e of the previous step into the two squared
// norms while wave 0 searches, into a per-window row of LDS (2 (H + 1) doubles) that is added to the block's accumulators (LDS too;
// entry k always by the same thread) only when the window ends with status 0.  A window leaves its step loop at the first state or
// record row that is not finite.  Where the staged layout plus the accumulators exceed the 160 KB of a CU the L2-fed step
// (tpwl::step_l2) is used: the same bits by the rule.
// th_join_kernel joins the blocks' partial sums in block order and takes the maxima with their window numbers (strictly greater only:
// the lowest window number keeps a tie).  No floating-point atomics; the blocks are a function of the shapes alone, so the result does
// not depend on the CU count.  One stream, one host wait.
#include "tpwl_host.h"

#include <cmath>
#include <vector>

namespace {

constexpr int TH_NT = 256;                          // threads of th_window_kernel: the rollout kernels'
constexpr int TH_BLOCK = 16;                        // windows of a block ..
constexpr int64_t TH_BLOCKS = 2048;                 // .. doubled while the call would have more blocks than this (and an episode has more windows)
constexpr int TH_MAX_NX = 128, TH_MAX_M = 16;       // the plant limits of the closed loops
constexpr int TH_MAX_H = 1024;
constexpr int64_t TH_PRED_CAP = (int64_t)256 << 20; // bytes of x_pred a call may ask for
constexpr size_t TH_LDS_MAX = (size_t)160 * 1024;   // LDS of a CU (gfx950); a single workgroup may hold all of it
constexpr size_t TH_LDS_PLAIN = (size_t)64 * 1024;  // what a launch may ask for without the attribute

typedef __attribute__((address_space(3))) long long *llptr;

struct ThArgs {
    const double *X, *U;                            // records (E x T x n), (E x T x m)
    int64_t T, We, bpe, W;                          // rows of an episode, windows and blocks of an episode, windows of the call
    int H, stride, every, block;
    double *part;                                   // (blocks x 4 x (H + 1)): sse_x, sse_z, worst_x, worst_z of every block
    long long *arg;                                 // (blocks x 2 x (H + 1)): the windows of worst_x, worst_z (-1: none)
    int *cnt;                                       // (blocks x 2): status-1 and status-2 windows
    double *fin;                                    // (2 x W) final_x, final_z, or null
    int *status;                                    // (W) or null
    double *pred;                                   // (W x (H + 1) x n) or null
};

struct ThPlan { int64_t Tk, We, W, bpe, blocks; int block, mode; size_t lds; };

__host__ __device__ inline size_t th_common_doubles(int n, int m, int H1) {
    return 2 * (size_t)n + (size_t)((m + 3) & ~3) + 8 * (size_t)H1 + 2;        // state, e, input, window row (2), accumulators (4 + 2), the flags
}

__device__ __forceinline__ bool th_finite(double x) { return fabs(x) < INFINITY; }

// squared norms of e (n doubles of LDS) by ONE wave: |e|^2 and |H e|^2 (0 without an output model)
__device__ __forceinline__ void th_norms(const TpwlDev &T, clptr el, int n, int nz, int lane, lptr sx_out, lptr sz_out) {
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s = fma(el[j], el[j], s);
    const double sx = wg::wave_sum(s);
    double sz = 0.0;
    for (int a = 0; a < nz; ++a) {
        double d = 0.0;
        for (int j = lane; j < n; j += 64) d = fma(T.H[a * n + j], el[j], d);
        const double ez = wg::wave_sum(d);
        sz = fma(ez, ez, sz);
    }
    if (lane == 0) { *sx_out = sx; *sz_out = sz; }
}

// MODE 0: the L2-fed step; 1: the staged step, general search; 2: the staged step, HELD search (w_v = 0, P <= 64, r <= 32)
template <int MODE>
__global__ __launch_bounds__(TH_NT) void th_window_kernel(TpwlDev T, ThArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = T.n, m = T.m, r = T.r, nz = T.H != nullptr ? T.nz : 0, H = a.H, H1 = a.H + 1;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    lptr xc = (lptr)smem;                                // n        the state xh_k
    lptr el = xc + n;                                    // n        e_k
    lptr uc = el + n;                                    // m        u_{j0+k}
    lptr row = uc + ((m + 3) & ~3);                      // 2 H1     the window's |e_k|^2, |ez_k|^2
    lptr acc = row + 2 * H1;                             // 4 H1     the block's sse_x, sse_z, worst_x, worst_z
    llptr arg = (llptr)(acc + 4 * H1);                   // 2 H1     the windows of the two maxima
    liptr ip = (liptr)(acc + 6 * H1);                    // the point; two flag words (windows alternate); every offset so far is even
    liptr flag = ip + 1;
    lptr step = acc + 6 * H1 + 2;
    tpwl::StepLds L;
    lptr xn = step, part = step + n;                     // MODE 0: the next state and wg::matTvec's partial sums
    if constexpr (MODE != 0) tpwl::step_carve(L, step, n, m, TH_NT, 0);
    const int S = max(1, TH_NT / n), j = tid % n, s = tid / n;                              // wg::matTvec's slices
    const int64_t b = blockIdx.x, ep = b / a.bpe, wl0 = (b - ep * a.bpe) * a.block;
    const int nwin = (int)min((int64_t)a.block, a.We - wl0);
    const double *Xe = a.X + ep * a.T * n, *Ue = a.U + ep * a.T * m;
    const int64_t xs = (int64_t)a.stride * n, us = (int64_t)a.stride * m;                    // doubles between kept rows

    for (int k = tid; k < H1; k += TH_NT) {
        acc[k] = 0.0; acc[H1 + k] = 0.0; acc[2 * H1 + k] = -1.0; acc[3 * H1 + k] = -1.0;
        arg[k] = -1; arg[H1 + k] = -1;
    }
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    // HELD, as in rollout_staged_kernel: lane i of wave 0 keeps ITS table point in registers for the whole block (tq[c] = 0.0 for c >= r),
    // lane c < r the coordinate x[r + c] of the state (xq, 0.0 for c >= r): a term c >= r of the search is fma(0.0, 0.0, sq) = sq exactly.
    double tq[32], xq = 0.0;
    if constexpr (MODE == 2) {
        if (wave == 0) {
            const int pl = lane < T.P ? lane : T.P - 1;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const double t = T.qT[(c < r ? c : r - 1) * T.P + pl];
                tq[c] = c < r ? t : 0.0;
            }
        }
    }
    int cur = -1, ndiv = 0, nbad = 0;
    __syncthreads();

    for (int wi = 0; wi < nwin; ++wi) {
        const int64_t wl = wl0 + wi, win = ep * a.We + wl;
        const double *xr0 = Xe + wl * a.every * xs, *ur0 = Ue + wl * a.every * us;
        double *pw = a.pred ? a.pred + win * (int64_t)H1 * n : nullptr;
        liptr fl = flag + (wi & 1);
        if (tid < n) {
            const double x = xr0[tid];
            xc[tid] = x;
            if (!th_finite(x)) atomicOr((int *)fl, 2);
            if (pw) pw[tid] = x;
        }
        if (tid == 0) { row[0] = 0.0; row[H1] = 0.0; }             // e_0 = 0 exactly
        if constexpr (MODE == 2) {
            if (wave == 0) xq = lane < r ? xr0[r + lane] : 0.0;
        }
        __syncthreads();
        int k = 0;
        for (; k < H; ++k) {
            if (*fl) break;                              // (written in front of the last barrier only: the same for every thread)
            double xr = 0.0, uv = 0.0;
            if (tid < n) xr = xr0[(int64_t)(k + 1) * xs + tid];                             // the row to compare with: requested before the products
            if (wave == 0) {
                int i;
                if constexpr (MODE == 2) {
                    double sq = 0.0;
#pragma unroll
                    for (int c0 = 0; c0 < 32; c0 += 8) {
                        if (c0 < r) {
#pragma unroll
                            for (int c = c0; c < c0 + 8; ++c) {
                                const int lo = __builtin_amdgcn_readlane(__double2loint(xq), c), hi = __builtin_amdgcn_readlane(__double2hiint(xq), c);
                                const double e = tq[c] - __hiloint2double(hi, lo);
                                sq = fma(e, e, sq);
                            }
                        }
                    }
                    const double dist = lane < T.P ? T.w_q * sqrt(sq) : INFINITY;
                    i = tpwl::wave_first_min(dist, lane, T.P);
                } else {
                    i = tpwl::nearest_wave(T, xc);
                }
                if (lane == 0) *ip = i;
            } else if (wave == 1) {
                if (lane < m) { uv = ur0[(int64_t)k * us + lane]; uc[lane] = uv; }          // (m <= 16)
            } else if (wave == 3) {
                if (k > 0) th_norms(T, el, n, nz, lane, row + k, row + H1 + k);             // e_k of the step before, while wave 0 searches
            }
            __syncthreads();
            const int i = *ip;
            double v = 0.0;
            if constexpr (MODE == 0) {
                tpwl::step_l2(xn, T, (size_t)i, n, m, xc, uc, part);
                if (tid < n) v = xn[tid];
            } else {
                if (i != cur) {                          // (the same for every thread)
                    tpwl::panel_load(L, T, i, cur, n, m, tid, TH_NT);
                    __syncthreads();
                }
                tpwl::step_slices(L, xc, uc, n, m, S, j, s);
                __syncthreads();
                if (tid < n) v = tpwl::step_sum(L, n, S, tid);
            }
            if (tid < n) {
                xc[tid] = v;
                el[tid] = v - xr;
                if (pw) pw[(int64_t)(k + 1) * n + tid] = v;
                const int f = (th_finite(v) ? 0 : 1) | (th_finite(xr) ? 0 : 2);
                if (f) atomicOr((int *)fl, f);
            }
            if (wave == 1 && lane < m && !th_finite(uv)) atomicOr((int *)fl, 2);
            if constexpr (MODE == 2) {
                if (wave == 0) xq = lane < r ? xc[r + lane] : 0.0;                          // (written just above by this wave: LDS keeps a wave's order)
            }
            __syncthreads();
        }
        // states 0 .. k are formed, the record's states 0 .. k and inputs 0 .. k - 1 are examined
        const int f0 = *fl;
        if (f0 == 0) {
            if (wave == 3 && H > 0) th_norms(T, el, n, nz, lane, row + H, row + H1 + H);
        } else if (!(f0 & 2)) {                          // left early, diverged: status 2 wins, so the rows it did not reach are examined too
            __syncthreads();                             // (every thread has read f0)
            const int rest = H - k;
            bool bad = false;
            for (int e = tid; e < rest * n; e += TH_NT) bad |= !th_finite(xr0[(int64_t)(k + 1 + e / n) * xs + e % n]);
            for (int e = tid; e < rest * m; e += TH_NT) bad |= !th_finite(ur0[(int64_t)(k + e / m) * us + e % m]);
            if (bad) atomicOr((int *)fl, 2);
        }
        if (tid == 0) flag[(wi + 1) & 1] = 0;            // the next window's word: last read in front of the previous window's last barrier
        __syncthreads();
        const int f1 = *fl, st = (f1 & 2) ? 2 : ((f1 & 1) ? 1 : 0);
        if (st == 0) {
            for (int q = tid; q < H1; q += TH_NT) {      // entry q always by this thread
                const double sx = row[q], sz = row[H1 + q];
                acc[q] += sx;
                acc[H1 + q] += sz;
                const double nx = sqrt(sx), nzv = sqrt(sz);
                if (nx > acc[2 * H1 + q]) { acc[2 * H1 + q] = nx; arg[q] = win; }           // strictly greater: the first window keeps a tie
                if (nzv > acc[3 * H1 + q]) { acc[3 * H1 + q] = nzv; arg[H1 + q] = win; }
            }
        } else if (pw) {                                 // the rows that were not formed
            for (int e = tid; e < (H - k) * n; e += TH_NT) pw[(int64_t)(k + 1) * n + e] = NAN;
        }
        if (tid == 0) {
            ndiv += st == 1;
            nbad += st == 2;
            if (a.fin) {
                a.fin[win] = st == 0 ? sqrt(row[H]) : NAN;
                a.fin[a.W + win] = st == 0 ? sqrt(row[H1 + H]) : NAN;
            }
            if (a.status) a.status[win] = st;
        }
        __syncthreads();                                 // the row and the flag are read; the next window may write them
    }
    double *po = a.part + b * 4 * (int64_t)H1;
    long long *ao = a.arg + b * 2 * (int64_t)H1;
    for (int q = tid; q < 4 * H1; q += TH_NT) po[q] = acc[q];
    for (int q = tid; q < 2 * H1; q += TH_NT) ao[q] = arg[q];
    if (tid == 0) { a.cnt[2 * b] = ndiv; a.cnt[2 * b + 1] = nbad; }
}

// entry (q, k) of the result: q = 0, 1 the sums in block order; q = 2, 3 the maxima with their windows; the counts by the first thread
__global__ __launch_bounds__(256) void th_join_kernel(const double *__restrict__ part, const long long *__restrict__ arg, const int *__restrict__ cnt,
                                                      int64_t blocks, int H1, double *__restrict__ out, long long *__restrict__ oarg,
                                                      long long *__restrict__ ocnt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        long long d = 0, bd = 0;
        for (int64_t b = 0; b < blocks; ++b) { d += cnt[2 * b]; bd += cnt[2 * b + 1]; }
        ocnt[0] = d; ocnt[1] = bd;
    }
    if (e >= 4 * H1) return;
    const int q = e / H1, k = e - q * H1;
    const double *p = part + (int64_t)q * H1 + k;
    const int64_t ld = 4 * (int64_t)H1;
    if (q < 2) {
        double sum = 0.0;
#pragma unroll 8
        for (int64_t b = 0; b < blocks; ++b) sum += p[b * ld];
        out[e] = sum;
    } else {
        double best = -1.0;
        int64_t bb = -1;
#pragma unroll 8
        for (int64_t b = 0; b < blocks; ++b) {
            const double v = p[b * ld];
            if (v > best) { best = v; bb = b; }          // strictly greater: the first block keeps a tie
        }
        out[e] = best;
        oarg[e - 2 * H1] = bb < 0 ? -1 : arg[bb * 2 * (int64_t)H1 + (int64_t)(q - 2) * H1 + k];
    }
}

// everything that is decided without a value of the records or the tables
int th_plan(const char *who, int r, int m, int P, int nz, double w_v, int64_t E, int64_t T, int H, int stride, int every, ThPlan *p) {
    SRH_REQUIRE(r >= 1, "%s: r = %d, need r >= 1 (n_x = 2 r)", who, r);
    SRH_REQUIRE(2 * (int64_t)r <= TH_MAX_NX, "%s: n_x = %lld exceeds the limit n_x <= %d", who, 2 * (long long)r, TH_MAX_NX);
    SRH_REQUIRE(m >= 1 && m <= TH_MAX_M, "%s: m = %d, need 1 <= m <= %d", who, m, TH_MAX_M);
    SRH_REQUIRE(P >= 1, "%s: P = %d, need P >= 1", who, P);
    SRH_REQUIRE(nz >= 0, "%s: n_z = %d, need n_z >= 0", who, nz);
    SRH_REQUIRE(H >= 1 && H <= TH_MAX_H, "%s: H = %d, need 1 <= H <= %d", who, H, TH_MAX_H);
    SRH_REQUIRE(E >= 1 && T >= 1, "%s: need E >= 1 episodes of T >= 1 rows, got E = %lld, T = %lld", who, (long long)E, (long long)T);
    SRH_REQUIRE(stride >= 1, "%s: stride = %d, need stride >= 1", who, stride);
    SRH_REQUIRE(every >= 1, "%s: every = %d, need every >= 1", who, every);
    const int n = 2 * r, H1 = H + 1;
    p->Tk = (T - 1) / stride + 1;
    p->We = p->Tk > H ? (p->Tk - 1 - H) / every + 1 : 0;
    p->W = E * p->We;
    SRH_REQUIRE(p->W >= 1, "%s: W = 0 windows: T' = %lld kept rows per episode, H = %d needs T' >= %d", who, (long long)p->Tk, H, H + 1);
    int block = TH_BLOCK;
    while (E * srh::cdiv(p->We, block) > TH_BLOCKS && block < p->We) block *= 2;
    p->block = block;
    p->bpe = srh::cdiv(p->We, block);
    p->blocks = E * p->bpe;
    SRH_REQUIRE(p->blocks < ((int64_t)1 << 31), "%s: %lld blocks of windows exceed the limit of 2^31 - 1 of a launch", who, (long long)p->blocks);
    const size_t common = th_common_doubles(n, m, H1);
    const size_t staged = srh::lds_request(sizeof(double) * (common + tpwl::step_doubles(n, m, TH_NT)));
    const size_t fed = srh::lds_request(sizeof(double) * (common + (size_t)n + TH_NT));
    const bool st = staged <= TH_LDS_MAX;
    p->mode = !st ? 0 : ((w_v == 0.0 && P <= 64 && r <= 32) ? 2 : 1);
    p->lds = st ? staged : fed;
    return SRH_OK;
}

template <int MODE>
int th_launch(const TpwlDev &T, const ThArgs &a, const ThPlan &p, hipStream_t st) {
    if (p.lds > TH_LDS_PLAIN)
        SRH_CHECK_HIP(hipFuncSetAttribute((const void *)th_window_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    th_window_kernel<MODE><<<(unsigned)p.blocks, TH_NT, p.lds, st>>>(T, a);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

int th_run(const char *who, const stpwl *h, const double *x_dev, const double *u_dev, int64_t E, int64_t T, int H, int stride, int every,
           double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms, int32_t *status, double *x_pred,
           hipStream_t st) {
    ThPlan p;
    int rc;
    if ((rc = th_plan(who, h->r, h->m, h->P, h->nz, h->w_v, E, T, H, stride, every, &p))) return rc;
    const int n = h->n, H1 = H + 1;
    const size_t pred_bytes = sizeof(double) * (size_t)p.W * H1 * n;
    SRH_REQUIRE(!x_pred || pred_bytes <= (size_t)TH_PRED_CAP, "%s: predictions of %lld windows x %d rows x %d need %zu bytes, above the cap of %lld bytes",
                who, (long long)p.W, H1, n, pred_bytes, (long long)TH_PRED_CAP);
    srh::DevBuf part, arg, cnt, out, oarg, ocnt, fin, stat, pred;
    if ((rc = part.alloc(sizeof(double) * (size_t)p.blocks * 4 * H1)) || (rc = arg.alloc(sizeof(long long) * (size_t)p.blocks * 2 * H1)) ||
        (rc = cnt.alloc(sizeof(int) * (size_t)p.blocks * 2)) || (rc = out.alloc(sizeof(double) * 4 * H1)) ||
        (rc = oarg.alloc(sizeof(long long) * 2 * H1)) || (rc = ocnt.alloc(sizeof(long long) * 2)))
        return rc;
    if (final_norms && (rc = fin.alloc(sizeof(double) * 2 * (size_t)p.W))) return rc;
    if (status && (rc = stat.alloc(sizeof(int) * (size_t)p.W))) return rc;
    if (x_pred && (rc = pred.alloc(pred_bytes))) return rc;
    ThArgs a{};
    a.X = x_dev; a.U = u_dev; a.T = T; a.We = p.We; a.bpe = p.bpe; a.W = p.W;
    a.H = H; a.stride = stride; a.every = every; a.block = p.block;
    a.part = part.as<double>(); a.arg = arg.as<long long>(); a.cnt = cnt.as<int>();
    a.fin = final_norms ? fin.as<double>() : nullptr;
    a.status = status ? stat.as<int>() : nullptr;
    a.pred = x_pred ? pred.as<double>() : nullptr;
    const TpwlDev Tv = h->view();
    if ((rc = p.mode == 0 ? th_launch<0>(Tv, a, p, st) : (p.mode == 1 ? th_launch<1>(Tv, a, p, st) : th_launch<2>(Tv, a, p, st)))) return rc;
    th_join_kernel<<<(unsigned)srh::cdiv(4 * H1, 256), 256, 0, st>>>(a.part, a.arg, a.cnt, p.blocks, H1, out.as<double>(), oarg.as<long long>(),
                                                                     ocnt.as<long long>());
    SRH_CHECK_HIP(hipGetLastError());
    // everything comes back behind one wait
    std::vector<double> ho(4 * (size_t)H1);
    std::vector<long long> ha(2 * (size_t)H1);
    long long hc[2] = {0, 0};
    SRH_CHECK_HIP(hipMemcpyAsync(ho.data(), out.p, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipMemcpyAsync(ha.data(), oarg.p, sizeof(long long) * ha.size(), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipMemcpyAsync(hc, ocnt.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    if (final_norms) SRH_CHECK_HIP(hipMemcpyAsync(final_norms, fin.p, sizeof(double) * 2 * (size_t)p.W, hipMemcpyDeviceToHost, st));
    if (status) SRH_CHECK_HIP(hipMemcpyAsync(status, stat.p, sizeof(int) * (size_t)p.W, hipMemcpyDeviceToHost, st));
    if (x_pred) SRH_CHECK_HIP(hipMemcpyAsync(x_pred, pred.p, pred_bytes, hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    for (int e = 0; e < 2 * H1; ++e) {
        if (sse) sse[e] = ho[e];
        if (worst) worst[e] = ho[2 * H1 + e];
        if (worst_at) {
            const long long w = ha[e];
            worst_at[2 * e] = w < 0 ? -1 : w / p.We;
            worst_at[2 * e + 1] = w < 0 ? -1 : (w % p.We) * every * stride;
        }
    }
    counts[0] = p.W; counts[1] = hc[0]; counts[2] = hc[1];
    return SRH_OK;
}

int th_check(const char *who, const stpwl *h, const void *x, const void *u, const int64_t *counts) {
    SRH_REQUIRE(h, "%s: null handle", who);
    SRH_REQUIRE(x && u, "%s: null argument (the records)", who);
    SRH_REQUIRE(counts, "%s: null argument (counts)", who);
    SRH_REQUIRE(h->has_discrete, "%s: the handle has no discrete tables (model has not been pre-discretised)", who);
    return SRH_OK;
}

}  // namespace

extern "C" {

int stpwl_horizon_plan(int r, int n_u, int P, int n_z, double w_v, int64_t E, int64_t T, int horizon, int stride, int every, int64_t *windows,
                       int *block, int64_t *blocks, int *mode, int64_t *lds_bytes, int64_t *launches, int64_t *pred_cap_bytes) {
    if (windows) *windows = 0;
    if (block) *block = 0;
    if (blocks) *blocks = 0;
    if (mode) *mode = 0;
    if (lds_bytes) *lds_bytes = 0;
    if (launches) *launches = 0;
    if (pred_cap_bytes) *pred_cap_bytes = TH_PRED_CAP;
    ThPlan p;
    int rc;
    if ((rc = th_plan("stpwl_horizon_plan", r, n_u, P, n_z, w_v, E, T, horizon, stride, every, &p))) return rc;
    if (windows) *windows = p.W;
    if (block) *block = p.block;
    if (blocks) *blocks = p.blocks;
    if (mode) *mode = p.mode;
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    if (launches) *launches = 2;
    return SRH_OK;
}

int stpwl_horizon_error_dev(stpwl_t *h, const double *x_dev, const double *u_dev, int64_t E, int64_t T, int horizon, int stride, int every,
                            double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms, int32_t *status,
                            double *x_pred, void *stream) {
    static const char *who = "stpwl_horizon_error_dev";
    int rc;
    if ((rc = th_check(who, h, x_dev, u_dev, counts))) return rc;
    return th_run(who, h, x_dev, u_dev, E, T, horizon, stride, every, sse, worst, worst_at, counts, final_norms, status, x_pred, (hipStream_t)stream);
}

int stpwl_horizon_error(stpwl_t *h, const double *x, const double *u, int64_t E, int64_t T, int horizon, int stride, int every, double *sse,
                        double *worst, int64_t *worst_at, int64_t *counts, double *final_norms, int32_t *status, double *x_pred) {
    static const char *who = "stpwl_horizon_error";
    int rc;
    if ((rc = th_check(who, h, x, u, counts))) return rc;
    ThPlan p;
    if ((rc = th_plan(who, h->r, h->m, h->P, h->nz, h->w_v, E, T, horizon, stride, every, &p))) return rc;        // (refusals before the upload)
    srh::DevBuf dx, du;
    if ((rc = dx.upload(x, sizeof(double) * (size_t)E * (size_t)T * h->n)) || (rc = du.upload(u, sizeof(double) * (size_t)E * (size_t)T * h->m)))
        return rc;
    return th_run(who, h, dx.as<double>(), du.as<double>(), E, T, horizon, stride, every, sse, worst, worst_at, counts, final_norms, status, x_pred,
                  nullptr);
}

}  // extern "C"
