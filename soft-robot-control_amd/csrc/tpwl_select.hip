// TPWL point selection from records on the device: the reference's distance rule (sofacontrol/tpwl/tpwl_utils.py:156-196,
// TPWLSnapshotData.evaluate_point / evaluate_point_dist) as a greedy scan over recorded reduced states.
//
// THE SELECTION RULE ("TPWL model identification", defines it).
//   Records: E episodes, each x (T x n_x), x = [v; q], n_x = 2 r; `stride` s >= 1 keeps rows 0, s, 2s, .. of every episode.  The candidates
//   are ALL kept rows (the last kept row of an episode too), scanned episode by episode and inside an episode in row order.
//   Points: the table starts as the seed (q0, v0), P0 >= 0 rows; with an empty table the first candidate is taken unconditionally.
//   Distances of a candidate c to a point p: dq = w_q ||q_p - q_c||, dv = w_v ||v_p - v_c|| in the arithmetic of THE POINT-SEARCH RULE
//   of tpwl_dev.h (each squared norm summed by fma in the order j = 0, 1, ... from 0.0, a correctly rounded sqrt); with w_v == 0 the
//   velocity part is not read and dv = 0.
//   Decision: separate == 0: c is taken iff dq + dv >= threshold for EVERY point of the table; separate != 0: iff dq >= threshold for
//   every point, or dv >= threshold for every point.  A taken candidate joins the table before the next candidate is examined.
//   Cap: when a candidate would become point max_points + 1 the scan stops there (status 1, stopped_at = that candidate).
//
// Kernels.  The decisions are sequential, the distances are not: min is exact, so "d >= threshold for every point" is
// "min over the points >= threshold" however the (candidate, point) pairs are split.  The candidates are processed in chunks of C in scan
// order, two launches per chunk on one stream:
//   ts_dmin_kernel (all CUs; one lane per candidate): the chunk's minima against the WHOLE table as it stands (its count is read from
//   device memory); the points pass through LDS in tiles of TS_TP, a lane keeps TS_TP running sums per norm and reads each of its own
//   coordinates once per tile.
//   ts_scan_kernel (one workgroup): the greedy scan through the chunk.  The first candidate whose minima pass is taken: its row joins the
//   table, its index and minima are written; every later candidate of the chunk that still passes is measured against the new point
//   (the point sits in LDS), and the first that still passes is next (an integer atomicMin in LDS).  A candidate that fails once is
//   never looked at again: the minima only fall.  On the cap the stop record is set and every later launch returns at once.
// ts_finite_kernel names the first kept row that is not finite (an integer atomicMin); the scan kernels return at once behind it.
// No floating-point atomics; count, flags and tables stay on the device between the launches, and the host waits once, at the end.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int TS_TP = 16;                 // points of an LDS tile of ts_dmin_kernel (TS_TP running sums per norm and lane)
constexpr int TS_NT1 = 256;               // threads of ts_dmin_kernel and ts_finite_kernel
constexpr int TS_NT2 = 1024;              // threads of ts_scan_kernel
constexpr int TS_CHUNK_SMALL = 2048;      // candidates of a chunk for calls of at most TS_SMALL_CALL candidates
constexpr int TS_CHUNK_LARGE = 16384;     // .. and of larger calls (64 workgroups per ts_dmin launch; 16 candidates per scan thread)
constexpr int64_t TS_SMALL_CALL = 65536;
constexpr int TS_MAX_R = 128;             // the tile of 2 x TS_TP x r doubles stays at 32 KB
constexpr int TS_MAX_P = 1024;            // the fit's limit on P (tpwl_fit.hip)
constexpr int TS_NONE = 0x7fffffff;

struct TsCtl {
    unsigned long long bad;               // the first kept row that is not finite (~0: none)
    long long stopped;                    // the candidate that met the cap
    int count;                            // points of the table
    int stop;                             // 1: the cap was met
};

struct TsArgs {
    const double *X;                      // (E x T x nx) records
    int64_t T, Tk, ncand;
    int stride, r, separate, P0, max_points, chunk;
    double w_q, w_v, thr;
    TsCtl *ctl;
    double *tq, *tv;                      // (max_points x r) the table, point-major
    double *mq, *mv;                      // (chunk) the minima of the chunk's candidates: dq + dv in mq, or dq and dv when separate
    long long *index;                     // (max_points) the candidate number of every taken point
    double *dmin;                         // (max_points x 2) the minima of every taken point at the moment it was taken
};

// candidate k of the call -> its row in the records: episode k / Tk, kept row k % Tk of it
__device__ __forceinline__ int64_t ts_src_row(int64_t k, int64_t T, int64_t Tk, int stride) {
    const int64_t ep = k / Tk;
    return ep * T + (k - ep * Tk) * stride;
}

// min that keeps a NaN (np.min): the minima of a table start at +inf
__device__ __forceinline__ double ts_min(double m, double d) { return (d < m || d != d) ? d : m; }

__device__ __forceinline__ bool ts_pass(const TsArgs &a, double mq, double mv) {
    return a.separate ? (mq >= a.thr || mv >= a.thr) : (mq >= a.thr);
}

__global__ void __launch_bounds__(TS_NT1) ts_finite_kernel(const double *__restrict__ X, int64_t T, int64_t Tk, int stride, int nx, int64_t ncand,
                                                          TsCtl *__restrict__ ctl) {
    const int64_t e = (int64_t)blockIdx.x * TS_NT1 + threadIdx.x;
    if (e >= ncand * nx) return;
    const int64_t k = e / nx;
    const double x = X[ts_src_row(k, T, Tk, stride) * nx + (e - k * nx)];
    if (!(fabs(x) < INFINITY)) atomicMin(&ctl->bad, (unsigned long long)k);
}

// the minima of the candidates k0 .. k0 + chunk - 1 against the table as it stands
__global__ void __launch_bounds__(TS_NT1) ts_dmin_kernel(TsArgs a, int64_t k0) {
    extern __shared__ double ts_tile[];              // [TS_TP x r] of q, then of v
    const TsCtl ctl = *a.ctl;
    if (ctl.stop || ctl.bad != ~0ull) return;
    const int tid = threadIdx.x, r = a.r, nx = 2 * r, P = ctl.count;
    const int c = blockIdx.x * TS_NT1 + tid;
    const int64_t k = k0 + c;
    const bool live = c < a.chunk && k < a.ncand;
    const bool vel = a.w_v != 0.0;
    const double *x = a.X + ts_src_row(live ? k : k0, a.T, a.Tk, a.stride) * nx;
    double *tq = ts_tile, *tv = ts_tile + TS_TP * r;
    double mq = INFINITY, mv = INFINITY;
    for (int p0 = 0; p0 < P; p0 += TS_TP) {
        const int np = min(TS_TP, P - p0);
        __syncthreads();
        for (int e = tid; e < TS_TP * r; e += TS_NT1) {
            const bool in = e < np * r;
            tq[e] = in ? a.tq[(size_t)p0 * r + e] : 0.0;
            tv[e] = in && vel ? a.tv[(size_t)p0 * r + e] : 0.0;
        }
        __syncthreads();
        double sq[TS_TP], sv[TS_TP];
#pragma unroll
        for (int p = 0; p < TS_TP; ++p) { sq[p] = 0.0; sv[p] = 0.0; }
        for (int j = 0; j < r; ++j) {
            const double xq = x[r + j];
#pragma unroll
            for (int p = 0; p < TS_TP; ++p) { const double e = tq[p * r + j] - xq; sq[p] = fma(e, e, sq[p]); }
            if (vel) {
                const double xv = x[j];
#pragma unroll
                for (int p = 0; p < TS_TP; ++p) { const double e = tv[p * r + j] - xv; sv[p] = fma(e, e, sv[p]); }
            }
        }
#pragma unroll
        for (int p = 0; p < TS_TP; ++p) {
            if (p < np) {
                const double dq = a.w_q * sqrt(sq[p]);
                if (a.separate) {
                    mq = ts_min(mq, dq);
                    mv = ts_min(mv, vel ? a.w_v * sqrt(sv[p]) : 0.0);
                } else {
                    double d = dq;
                    if (vel) d += a.w_v * sqrt(sv[p]);
                    mq = ts_min(mq, d);
                }
            }
        }
    }
    if (live) {
        a.mq[c] = mq;
        if (a.separate) a.mv[c] = mv;
    }
}

// the greedy scan through the candidates k0 .. k0 + chunk - 1; one workgroup
__global__ void __launch_bounds__(TS_NT2) ts_scan_kernel(TsArgs a, int64_t k0) {
    extern __shared__ double ts_pt[];                // [v; q] of the point taken last
    __shared__ int first[2];
    const TsCtl ctl = *a.ctl;
    if (ctl.stop || ctl.bad != ~0ull) return;
    const int tid = threadIdx.x, r = a.r, nx = 2 * r;
    const int nc = (int)min((int64_t)a.chunk, a.ncand - k0);
    const bool vel = a.w_v != 0.0;
    int cnt = ctl.count, slot = 0;
    if (tid == 0) { first[0] = TS_NONE; first[1] = TS_NONE; }
    __syncthreads();
    {
        int best = TS_NONE;
        for (int j = tid; j < nc; j += TS_NT2)
            if (ts_pass(a, a.mq[j], a.separate ? a.mv[j] : 0.0)) { best = j; break; }
        if (best != TS_NONE) atomicMin(&first[0], best);
    }
    __syncthreads();
    int i = first[0];
    while (i != TS_NONE) {
        const int64_t k = k0 + i;
        if (cnt >= a.max_points) {                   // candidate k would be point max_points + 1
            if (tid == 0) { a.ctl->stopped = k; a.ctl->stop = 1; }
            break;
        }
        const double *xi = a.X + ts_src_row(k, a.T, a.Tk, a.stride) * nx;
        for (int j = tid; j < nx; j += TS_NT2) {
            const double val = xi[j];
            ts_pt[j] = val;
            if (j < r) a.tv[(size_t)cnt * r + j] = val; else a.tq[(size_t)cnt * r + (j - r)] = val;
        }
        if (tid == 0) {
            a.index[cnt] = k;
            a.dmin[2 * (size_t)cnt] = a.mq[i];
            a.dmin[2 * (size_t)cnt + 1] = a.separate ? a.mv[i] : 0.0;
            first[slot ^ 1] = TS_NONE;               // last read in front of the previous barrier; written again behind the next one
        }
        ++cnt;
        __syncthreads();
        int best = TS_NONE;
        for (int j = i + 1 + tid; j < nc; j += TS_NT2) {
            double mq = a.mq[j], mv = a.separate ? a.mv[j] : 0.0;
            if (!ts_pass(a, mq, mv)) continue;       // failed once: the minima only fall
            const double *x = a.X + ts_src_row(k0 + j, a.T, a.Tk, a.stride) * nx;
            double sq = 0.0, sv = 0.0;
            for (int q = 0; q < r; ++q) { const double e = ts_pt[r + q] - x[r + q]; sq = fma(e, e, sq); }
            if (vel)
                for (int q = 0; q < r; ++q) { const double e = ts_pt[q] - x[q]; sv = fma(e, e, sv); }
            const double dq = a.w_q * sqrt(sq);
            if (a.separate) {
                mq = ts_min(mq, dq);
                mv = ts_min(mv, vel ? a.w_v * sqrt(sv) : 0.0);
                a.mv[j] = mv;
            } else {
                double d = dq;
                if (vel) d += a.w_v * sqrt(sv);
                mq = ts_min(mq, d);
            }
            a.mq[j] = mq;
            if (best == TS_NONE && ts_pass(a, mq, mv)) best = j;
        }
        slot ^= 1;
        if (best != TS_NONE) atomicMin(&first[slot], best);
        __syncthreads();
        i = first[slot];
    }
    if (tid == 0) a.ctl->count = cnt;
}

int64_t ts_kept_rows(int64_t T, int stride) { return (T - 1) / stride + 1; }
int ts_chunk(int64_t candidates) { return candidates <= TS_SMALL_CALL ? TS_CHUNK_SMALL : TS_CHUNK_LARGE; }
size_t ts_lds(int r) { return sizeof(double) * 2 * (size_t)TS_TP * (size_t)r; }

// everything that is decided without the records' values
int ts_check(const char *who, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold, int P0, const double *q0,
             const double *v0, int max_points, const int *count) {
    SRH_REQUIRE(count, "%s: null argument (count)", who);
    SRH_REQUIRE(r >= 1, "%s: r = %d, need r >= 1 (n_x = 2 r)", who, r);
    SRH_REQUIRE(r <= TS_MAX_R, "%s: r = %d exceeds the limit r <= %d", who, r, TS_MAX_R);
    SRH_REQUIRE(E >= 1 && T >= 1, "%s: need E >= 1 episodes of T >= 1 rows", who);
    SRH_REQUIRE(stride >= 1, "%s: stride = %d, need stride >= 1", who, stride);
    SRH_REQUIRE(std::isfinite(threshold) && threshold > 0.0, "%s: threshold = %g, need a finite threshold > 0", who, threshold);
    SRH_REQUIRE(std::isfinite(w_q) && w_q >= 0.0, "%s: the weight w_q = %g is negative or not finite", who, w_q);
    SRH_REQUIRE(std::isfinite(w_v) && w_v >= 0.0, "%s: the weight w_v = %g is negative or not finite", who, w_v);
    SRH_REQUIRE(w_q != 0.0 || w_v != 0.0, "%s: both weights are zero", who);
    SRH_REQUIRE(P0 >= 0, "%s: P0 = %d, need P0 >= 0", who, P0);
    SRH_REQUIRE(max_points >= (P0 > 1 ? P0 : 1) && max_points <= TS_MAX_P, "%s: max_points = %d, need max(P0, 1) = %d <= max_points <= %d", who,
                max_points, P0 > 1 ? P0 : 1, TS_MAX_P);
    SRH_REQUIRE(P0 == 0 || (q0 && v0), "%s: null argument (a seed of P0 = %d points needs q0 and v0)", who, P0);
    for (int64_t e = 0; e < (int64_t)P0 * r; ++e)
        SRH_REQUIRE(std::isfinite(q0[e]) && std::isfinite(v0[e]), "%s: seed point %lld holds a non-finite entry", who, (long long)(e / r));
    return SRH_OK;
}

int ts_run(const char *who, const double *x_dev, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold, int separate,
           int P0, const double *q0, const double *v0, int max_points, int *count, int64_t *index, double *q, double *v, double *dmin, int *status,
           int64_t *stopped_at, hipStream_t st) {
    const int nx = 2 * r;
    const int64_t Tk = ts_kept_rows(T, stride), ncand = E * Tk;
    const int chunk = ts_chunk(ncand);
    const size_t tab = sizeof(double) * (size_t)max_points * r;
    srh::DevBuf ctl, tq, tv, mq, mv, idx, dm;
    int rc;
    if ((rc = ctl.alloc(sizeof(TsCtl))) || (rc = tq.alloc(tab)) || (rc = tv.alloc(tab)) || (rc = mq.alloc(sizeof(double) * (size_t)chunk)) ||
        (rc = mv.alloc(sizeof(double) * (size_t)chunk)) || (rc = idx.alloc(sizeof(long long) * (size_t)max_points)) ||
        (rc = dm.alloc(sizeof(double) * 2 * (size_t)max_points)))
        return rc;
    TsCtl h{};
    h.bad = ~0ull; h.stopped = -1; h.count = P0; h.stop = 0;
    SRH_CHECK_HIP(hipMemcpyAsync(ctl.p, &h, sizeof(h), hipMemcpyHostToDevice, st));
    if (P0 > 0) {
        SRH_CHECK_HIP(hipMemcpyAsync(tq.p, q0, sizeof(double) * (size_t)P0 * r, hipMemcpyHostToDevice, st));
        SRH_CHECK_HIP(hipMemcpyAsync(tv.p, v0, sizeof(double) * (size_t)P0 * r, hipMemcpyHostToDevice, st));
    }
    TsArgs a{};
    a.X = x_dev; a.T = T; a.Tk = Tk; a.ncand = ncand;
    a.stride = stride; a.r = r; a.separate = separate ? 1 : 0; a.P0 = P0; a.max_points = max_points; a.chunk = chunk;
    a.w_q = w_q; a.w_v = w_v; a.thr = threshold;
    a.ctl = ctl.as<TsCtl>(); a.tq = tq.as<double>(); a.tv = tv.as<double>(); a.mq = mq.as<double>(); a.mv = mv.as<double>();
    a.index = idx.as<long long>(); a.dmin = dm.as<double>();
    ts_finite_kernel<<<(unsigned)srh::cdiv(ncand * nx, TS_NT1), TS_NT1, 0, st>>>(x_dev, T, Tk, stride, nx, ncand, a.ctl);
    SRH_CHECK_HIP(hipGetLastError());
    const unsigned nb1 = (unsigned)srh::cdiv(chunk, TS_NT1);
    for (int64_t k0 = 0; k0 < ncand; k0 += chunk) {
        ts_dmin_kernel<<<nb1, TS_NT1, ts_lds(r), st>>>(a, k0);
        ts_scan_kernel<<<1, TS_NT2, sizeof(double) * (size_t)nx, st>>>(a, k0);
    }
    SRH_CHECK_HIP(hipGetLastError());
    // everything comes back behind one wait: the control words and the whole (small) tables
    const int ntake = max_points - P0;
    std::vector<long long> hidx((size_t)max_points);
    std::vector<double> hq((size_t)max_points * r), hv((size_t)max_points * r), hd(2 * (size_t)max_points);
    SRH_CHECK_HIP(hipMemcpyAsync(&h, ctl.p, sizeof(h), hipMemcpyDeviceToHost, st));
    if (ntake > 0) {
        SRH_CHECK_HIP(hipMemcpyAsync(hidx.data(), idx.p, sizeof(long long) * hidx.size(), hipMemcpyDeviceToHost, st));
        SRH_CHECK_HIP(hipMemcpyAsync(hq.data(), tq.p, tab, hipMemcpyDeviceToHost, st));
        SRH_CHECK_HIP(hipMemcpyAsync(hv.data(), tv.p, tab, hipMemcpyDeviceToHost, st));
        SRH_CHECK_HIP(hipMemcpyAsync(hd.data(), dm.p, sizeof(double) * hd.size(), hipMemcpyDeviceToHost, st));
    }
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    if (h.bad != ~0ull) {
        srh::set_error("%s: episode %lld, row %lld of the records is not finite; nothing was selected", who, (long long)(h.bad / (unsigned long long)Tk),
                       (long long)((h.bad % (unsigned long long)Tk) * stride));
        return SRH_EINVAL;
    }
    SRH_REQUIRE(h.count >= P0 && h.count <= max_points, "%s: the device reports %d points, outside %d .. %d", who, h.count, P0, max_points);
    *count = h.count;
    if (status) *status = h.stop ? 1 : 0;
    if (stopped_at) {
        stopped_at[0] = h.stop ? h.stopped / Tk : -1;
        stopped_at[1] = h.stop ? (h.stopped % Tk) * stride : -1;
    }
    const int nsep = separate ? 2 : 1;
    for (int p = P0; p < h.count; ++p) {
        const size_t o = (size_t)(p - P0);
        if (index) { index[2 * o] = hidx[p] / Tk; index[2 * o + 1] = (hidx[p] % Tk) * stride; }
        if (q) std::copy(hq.begin() + (size_t)p * r, hq.begin() + (size_t)(p + 1) * r, q + o * r);
        if (v) std::copy(hv.begin() + (size_t)p * r, hv.begin() + (size_t)(p + 1) * r, v + o * r);
        if (dmin)
            for (int s = 0; s < nsep; ++s) dmin[o * nsep + s] = hd[2 * (size_t)p + s];
    }
    return SRH_OK;
}

}  // namespace

extern "C" {

int stpwl_select_plan(int r, int64_t candidates, int *chunk, int64_t *lds_bytes, int64_t *launches) {
    if (chunk) *chunk = 0;
    if (lds_bytes) *lds_bytes = 0;
    if (launches) *launches = 0;
    SRH_REQUIRE(r >= 1, "stpwl_select_plan: r = %d, need r >= 1", r);
    SRH_REQUIRE(r <= TS_MAX_R, "stpwl_select_plan: r = %d exceeds the limit r <= %d", r, TS_MAX_R);
    SRH_REQUIRE(candidates >= 1, "stpwl_select_plan: need candidates >= 1");
    const int c = ts_chunk(candidates);
    if (chunk) *chunk = c;
    if (lds_bytes) *lds_bytes = (int64_t)ts_lds(r);
    if (launches) *launches = 1 + 2 * srh::cdiv(candidates, c);
    return SRH_OK;
}

int stpwl_select_points_dev(const double *x_dev, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold, int separate,
                            int P0, const double *q0, const double *v0, int max_points, int *count, int64_t *index, double *q, double *v,
                            double *dmin, int *status, int64_t *stopped_at, void *stream) {
    static const char *who = "stpwl_select_points_dev";
    SRH_REQUIRE(x_dev, "%s: null argument (x_dev)", who);
    int rc;
    if ((rc = ts_check(who, E, T, r, stride, w_q, w_v, threshold, P0, q0, v0, max_points, count))) return rc;
    return ts_run(who, x_dev, E, T, r, stride, w_q, w_v, threshold, separate, P0, q0, v0, max_points, count, index, q, v, dmin, status, stopped_at,
                  (hipStream_t)stream);
}

int stpwl_select_points(const double *x, int64_t E, int64_t T, int r, int stride, double w_q, double w_v, double threshold, int separate, int P0,
                        const double *q0, const double *v0, int max_points, int *count, int64_t *index, double *q, double *v, double *dmin,
                        int *status, int64_t *stopped_at) {
    static const char *who = "stpwl_select_points";
    SRH_REQUIRE(x, "%s: null argument (x)", who);
    int rc;
    if ((rc = ts_check(who, E, T, r, stride, w_q, w_v, threshold, P0, q0, v0, max_points, count))) return rc;
    const int nx = 2 * r;
    const int64_t Tk = ts_kept_rows(T, stride);
    for (int64_t ep = 0; ep < E; ++ep)                         // host records: the first kept row that is not finite, before any device call
        for (int64_t i = 0; i < Tk; ++i) {
            const double *row = x + (ep * T + i * stride) * nx;
            for (int j = 0; j < nx; ++j)
                SRH_REQUIRE(std::isfinite(row[j]), "%s: episode %lld, row %lld of the records is not finite; nothing was selected", who,
                            (long long)ep, (long long)(i * stride));
        }
    srh::DevBuf dx;
    if ((rc = dx.upload(x, sizeof(double) * (size_t)E * (size_t)T * nx))) return rc;
    return ts_run(who, dx.as<double>(), E, T, r, stride, w_q, w_v, threshold, separate, P0, q0, v0, max_points, count, index, q, v, dmin, status,
                  stopped_at, nullptr);
}

}  // extern "C"
