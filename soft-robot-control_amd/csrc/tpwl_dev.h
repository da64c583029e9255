// Device view of a TPWL model (tables resident in HBM/L2) and workgroup-cooperative helpers.
// Reference: sofacontrol/tpwl/tpwl.py (nearest-neighbour TPWL), sofacontrol/scp/models/tpwl.py.
#pragma once
#include "dev_la.h"

struct TpwlDev {
    int P, r, n, m, nz;
    double w_q, w_v;
    cgptr qT, vT;            // (r x P) transposed point tables (coalesced over points)
    cgptr u;                          // (P x m)
    cgptr Ac, Bc, dc;       // continuous tables (P x n x n), (P x n x m), (P x n)
    cgptr AcT;                // (P x n x n) transposed
    cgptr Ad, Bd, dd;       // discrete tables or null
    cgptr AdT;                // transposed discrete A
    cgptr BdT;                // (P x m x n) transposed discrete B
    cgptr BcT;                // (P x m x n)
    cgptr H, z_ref;          // (nz x n), (nz) or null
};

namespace tpwl {

// THE POINT-SEARCH RULE, stated once for the four places that search the table (nearest_wave; the register-table branch of nearest_many;
// the HELD search of rollout_staged_kernel and weights_kernel in tpwl.hip):
//   d_i = w_q ||q_i - q|| + w_v ||v_i - v||, each squared norm summed by fma in the order j = 0, 1, ... from 0.0; with w_v == 0 the
//   velocity part of the state is not read;
//   the nearest point is the FIRST minimum of d (np.argmin: the smallest index among the minima), and 0 when there is none -- every
//   d_i +inf or not a number (a diverged state, a NaN of a failed solve upstream): np.argmin gives 0 there too, and the index is always
//   one of the table's.
// A search keeps "no candidate yet" as (+inf, index 0): only a d < +inf takes its place, so a search that ends without a candidate ends
// with 0, and in a comparison of two of them 0 stays.  (wave_first_min below has no such pair to start from and maps its own marker.)

// candidate (da, ia) goes before (db, ib): nearer, or as near with the smaller index
__device__ __forceinline__ bool goes_before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }
// first minimum over the lanes of ONE wave, lane i holding d_i (+inf in the lanes past the table); every lane returns the index
__device__ __forceinline__ int wave_first_min(double dist, int lane, int P) {
    const double dmin = wg::wave_min(dist);
    const int imin = (int)wg::wave_min(dist == dmin ? (double)lane : 1e9);        // (1e9: no lane holds the minimum -- it is not a number)
    return imin < P ? imin : 0;
}

// The rule for the state x (LDS or global, x = [v; q]).  Executed by ONE wave (64 lanes); every lane returns the index.
template <typename XP>
__device__ inline int nearest_wave(const TpwlDev &T, XP x) {
    const int lane = SRH_TID & 63;
    double best = INFINITY;                              // no candidate yet
    int besti = 0;
    // sum_j (tab[j][i] - x[xoff + j])^2 in the order j = 0, 1, ...: sixteen table / state loads are requested before the
    // first FMA (a rolled load -> FMA loop pays the L2 latency r times per point; same sums, same order)
    auto sqdist = [&](cgptr tab, int xoff, int i) {
        double sq = 0.0;
        for (int j0 = 0; j0 < T.r; j0 += 16) {
            double tv[16], xv[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = j0 + q < T.r ? j0 + q : T.r - 1;
                tv[q] = tab[j * T.P + i];
                xv[q] = x[xoff + j];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (j0 + q < T.r) { const double e = tv[q] - xv[q]; sq = fma(e, e, sq); }
            }
        }
        return sq;
    };
    for (int i0 = 0; i0 < T.P; i0 += 64) {
        const int i = i0 + lane;
        double d = INFINITY;
        if (i < T.P) {
            d = T.w_q * sqrt(sqdist(T.qT, T.r, i));
            if (T.w_v != 0.0) d += T.w_v * sqrt(sqdist(T.vT, 0, i));
        }
        if (d < best) { best = d; besti = i; }
    }
    // wave argmin with smallest-index tie break
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(besti, o, 64);
        if (goes_before(ob, oi, best, besti)) { best = ob; besti = oi; }
    }
    return besti;
}

// nearest point for `count` states X (count x n, LDS or global) -> idx (LDS/global int array).
// All waves of the workgroup participate; ends with __syncthreads().
// Position-weighted tables of at most 64 points and 32 coordinates (every shipped model: w_v = 0, P = 64, r = 30 / 36 is the general
// path): lane i keeps ITS point in registers for all the states of the call, the coordinates of a state arrive with one coalesced load
// (requested one state ahead) and are broadcast lane by lane -- nearest_wave pays four L2 round trips, a library sqrt and eighteen
// ds_bpermute per state (6-8 k clocks; 60 k per SCP iteration at C2).  Same sums in the same order, same first minimum.
template <typename XP, typename IP>
__device__ inline void nearest_many(const TpwlDev &T, XP X, int ldx, int count, IP idx) {
    const int wave = __builtin_amdgcn_readfirstlane(SRH_TID >> 6), nw = blockDim.x >> 6, lane = SRH_TID & 63;
    if (T.w_v == 0.0 && T.P <= 64 && T.r <= 32 && count >= 2 * nw) {            // (fewer states than two rounds: the table load does not pay)
        const int r = T.r;
        const bool live = lane < T.P;
        const int pl = live ? lane : T.P - 1, xl = lane < r ? lane : r - 1;
        double tq[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) tq[j] = T.qT[(j < r ? j : r - 1) * T.P + pl];     // unconditional (clamped) loads: all in flight at once
        int k = wave;
        double xv = (double)X[(size_t)(k < count ? k : count - 1) * ldx + r + xl];
        while (k < count) {
            const int kn = k + nw;
            const double xn = (double)X[(size_t)(kn < count ? kn : count - 1) * ldx + r + xl];             // the next state, while this one is worked on
            double sq = 0.0;
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                if (j < r) {
                    const int lo = __builtin_amdgcn_readlane(__double2loint(xv), j), hi = __builtin_amdgcn_readlane(__double2hiint(xv), j);
                    const double e = tq[j] - __hiloint2double(hi, lo);
                    sq = fma(e, e, sq);
                }
            }
            const double dist = live ? T.w_q * sqrt(sq) : INFINITY;
            const int imin = wave_first_min(dist, lane, T.P);
            if (lane == 0) idx[k] = imin;
            k = kn;
            xv = xn;
        }
    } else {
        for (int k = wave; k < count; k += nw) {
            const int i = nearest_wave(T, X + (size_t)k * ldx);
            if (lane == 0) idx[k] = i;
        }
    }
    __syncthreads();
}

// THE STEP RULE, stated once for the kernels that step a TPWL plant (rollout_kernel and rollout_staged_kernel in tpwl.hip,
// loop_advance_kernel in gusto_loop.hip, rompc_loop_advance_kernel in rompc_loop.hip, the TPWL forward pass of ilqr_kernel in lqr.hip):
//   x' = d_d[i] + A_d[i] x + B_d[i] u, i the nearest point to x, read from the transposed tables (coalesced along the columns);
//   with len = n columns and S = max(1, threads / n) slices, slice s sums the rows s, s + S, ... of a product by fma from 0.0
//   (wg::matTvec's slices; for n > threads one slice, and thread t takes the columns t, t + threads, ...);
//   x'[t] = d[t] + p_A[0][t] + ... + p_A[S-1][t], then + p_B[0][t] + ... + p_B[S-1][t]: first the partials of A x, then those of B u, each
//   in slice order.  A disturbance w is added behind that by the caller.
// The L2-fed step (step_l2) is two wg::matTvec calls, the second adding onto the first.  The staged step keeps the region's panel
// [A_d^T | B_d^T | d_d] in LDS (StepLds), reloads it only when the point changes (panel_load) and forms both products under one barrier
// (step_slices, the caller's barrier, step_sum).  The staged helpers read no thread index and hold no barrier: thread index, slice, column
// and thread count are the caller's, so each kernel keeps its own reads and its own barriers (wg::matTvec has its own of both).
typedef double d2 __attribute__((ext_vector_type(2)));

// 16-byte copy of `count` doubles from global memory into LDS (count even, both 16-byte aligned)
__device__ __forceinline__ void copy16(lptr dst, cgptr src, int count, int tid, int nt) {
    auto d = (__attribute__((address_space(3))) d2 *)dst;
    auto s = (const __attribute__((address_space(1))) d2 *)src;
    for (int e = tid; e < (count >> 1); e += nt) d[e] = s[e];
}

// LDS of the staged step: two partial buffers of nt doubles, the panel.  A kernel may keep `gap` doubles of its own between pb and At
// (the point words; every panel offset stays even).
struct StepLds { lptr pa, pb, At, Bt, dl; };
__host__ __device__ inline size_t step_doubles(int n, int m, int nt) { return 2 * (size_t)nt + (size_t)n * n + (size_t)m * n + n; }
// returns the first double behind the panel
__device__ __forceinline__ lptr step_carve(StepLds &L, lptr base, int n, int m, int nt, int gap) {
    L.pa = base;                                         // nt     partial sums of A x
    L.pb = L.pa + nt;                                    // nt     partial sums of B u
    L.At = L.pb + nt + gap;                              // n x n  the panel of the region
    L.Bt = L.At + n * n;                                 // m x n
    L.dl = L.Bt + m * n;                                 // n
    return L.dl + n;
}

// the panel of point p unless it is the one loaded (cur); true when it loaded.  The same for every thread; no barrier.
__device__ __forceinline__ bool panel_load(const StepLds &L, const TpwlDev &T, int p, int &cur, int n, int m, int tid, int nt) {
    if (p == cur) return false;
    copy16(L.At, T.AdT + (size_t)p * n * n, n * n, tid, nt);
    copy16(L.Bt, T.BdT + (size_t)p * m * n, m * n, tid, nt);
    copy16(L.dl, T.dd + (size_t)p * n, n, tid, nt);
    cur = p;
    return true;
}

// slice sl of both products for column j
__device__ __forceinline__ void step_slices(const StepLds &L, clptr xc, clptr uc, int n, int m, int S, int j, int sl) {
    if (sl < S) {
        double a = 0.0, c = 0.0;
#pragma unroll 4
        for (int q = sl; q < n; q += S) a = fma(L.At[q * n + j], xc[q], a);
        for (int q = sl; q < m; q += S) c = fma(L.Bt[q * n + j], uc[q], c);
        L.pa[sl * n + j] = a;
        L.pb[sl * n + j] = c;
    }
}

// x'[t], behind the barrier that follows step_slices
__device__ __forceinline__ double step_sum(const StepLds &L, int n, int S, int t) {
    double v = L.dl[t];
    for (int q = 0; q < S; ++q) v += L.pa[q * n + t];
    for (int q = 0; q < S; ++q) v += L.pb[q * n + t];
    return v;
}

// xn = d_d[i] + A_d[i] xc + B_d[i] uc from the tables in L2, n <= threads (wg::matTvec: ends with __syncthreads())
__device__ __forceinline__ void step_l2(lptr xn, const TpwlDev &T, size_t i, int n, int m, clptr xc, clptr uc, lptr part) {
    wg::matTvec(xn, T.AdT + i * n * n, n, n, n, xc, T.dd + i * n, part);
    wg::matTvec(xn, T.BdT + i * m * n, n, m, n, uc, (clptr)xn, part);
}

// wg::matTvec for len > nt threads, where its (slice, j) layout has one slice and no thread for the columns j >= nt: thread t takes the
// columns t, t + nt, ...  The sums are those of the rule with one slice: rows 0, 1, ... by fma from 0.0, then add[j] + sum.
// add may be y (each column is read and written by its own thread).  Ends with __syncthreads().
template <typename MP, typename AP, typename NT>
__device__ inline void matTvec_strided(lptr y, MP M, int ldm, int rows, int len, clptr v, AP add, int tid, NT nt) {
    for (int j = tid; j < len; j += nt) {
        double acc = 0.0;
#pragma unroll 4
        for (int i = 0; i < rows; ++i) acc = fma(M[i * ldm + j], v[i], acc);
        double r = add ? add[j] : 0.0;
        r += acc;
        y[j] = r;
    }
    __syncthreads();
}
// step_l2 for n > nt threads (nt of the caller's type: blockDim.x is unsigned)
template <typename NT>
__device__ __forceinline__ void step_l2_strided(lptr xn, const TpwlDev &T, size_t i, int n, int m, clptr xc, clptr uc, int tid, NT nt) {
    matTvec_strided(xn, T.AdT + i * n * n, n, n, n, xc, T.dd + i * n, tid, nt);
    matTvec_strided(xn, T.BdT + i * m * n, n, m, n, uc, (clptr)xn, tid, nt);
}

}  // namespace tpwl
