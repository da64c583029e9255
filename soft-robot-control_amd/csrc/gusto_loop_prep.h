// The device side of what the five closed-loop units (gusto_loop.hip: TPWL plans, gusto_ssm_loop.hip: SSM plans, rompc_loop.hip: the
// ROMPC baseline, koopman_loop.hip: the Koopman baseline, ilqr_loop.hip: the iLQR policy) share, stated once: the plan point of a
// sub-step, the output and measurement rows, the target table's interpolation, the query times, the measurement's re-projection, and
// loop_prepare_kernel -- the kernel that turns the previous period's output into the next solve's input (x0, the shifted guess, the
// target window).  Its one launch, and the host shell around it, is gusto_loop_host.h.  Each unit gets its own instance of the kernel
// (anonymous namespace; the iLQR loop, which has no periods, never launches its own); an SSM loop passes no H (it has no linear output
// map) and no zf (no terminal cost).
#pragma once
#include "common.h"
#include "dev_la.h"
#include "poly_dev.h"

namespace {

// THE PLAN POINT of a sub-step: lo + theta (hi - lo), in this association, of the plan's rows j_lo and j_hi (rows x ld) at column c.
// States pass j_hi = j + 1; inputs pass j_hi = min(j + 1, N - 1): the input is held over the last interval (controllers.py:299).
__device__ __forceinline__ double lerp(double lo, double hi, double th) { return lo + th * (hi - lo); }
__device__ __forceinline__ double plan_at(cgptr rows, int ld, int j_lo, int j_hi, double th, int c) {
    return lerp(rows[(size_t)j_lo * ld + c], rows[(size_t)j_hi * ld + c], th);
}

// THE OUTPUT ROW e of M x (z = H x, y = C x; M (rows x n) row-major, x in LDS or global): by fma from 0.0 in the order c = 0, 1, ... --
// the sum of gusto_write_out (zopt = H xopt).
template <typename MP, typename XP>
__device__ __forceinline__ double out_row(MP M, int e, int n, XP x) {
    double v = 0.0;
    for (int c = 0; c < n; ++c) v = fma(M[e * n + c], x[c], v);
    return v;
}

// The measurement ((C x)_e + y_ref[e]) + noise[iv], in this order; y_ref and noise may each be null (that addend is then left out).
// C and y_ref are in global memory or in LDS.
template <typename MP, typename XP, typename RP>
__device__ __forceinline__ double measure_row(MP Cm, int e, int n, XP x, RP y_ref, cgptr noise, size_t iv) {
    double v = out_row(Cm, e, n, x);
    if (y_ref != nullptr) v += y_ref[e];
    if (noise != nullptr) v += noise[iv];
    return v;
}

// Row `a` of the table (tt (T), ty (T x ld)) at tq: scipy's interp1d(kind='linear', bounds_error=False, fill_value=(y[0], y[-1])) --
// i = searchsorted(tt, tq) (first tt[i] >= tq) clipped to 1..T-1, slope (y[i] - y[i-1]) / (tt[i] - tt[i-1]), slope (tq - tt[i-1]) + y[i-1];
// the first / last row outside the table.  A tq that is not a number picks i = 1 and gives not-a-number: no index leaves the table.
__device__ __forceinline__ double table_at(cgptr tt, cgptr ty, int T, int ld, int a, double tq) {
    if (tq < tt[0]) return ty[a];
    if (tq > tt[T - 1]) return ty[(size_t)(T - 1) * ld + a];
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tt[mid] < tq) lo = mid + 1; else hi = mid;
    }
    const int i = min(max(lo, 1), T - 1);
    const double t0 = tt[i - 1], y0 = ty[(size_t)(i - 1) * ld + a];
    const double slope = (ty[(size_t)i * ld + a] - y0) / (tt[i] - t0);
    return slope * (tq - t0) + y0;
}

// t0 + dt k with the product and the sum rounded on their own (no fused multiply-add): numpy's statement of the query times
__device__ __forceinline__ double query_time(double t0, double dt, int k) {
#pragma clang fp contract(off)
    const double s = dt * (double)k;
    return t0 + s;
}

// THE RE-PROJECTION OF A MEASUREMENT onto the admissible set Y = {y : A y <= b} inside an advance kernel (koopman.py:150-151,
// SSM/controllers.py:96-97: `if not Y.contains(y): y = Y.project_to_polyhedron(y)`), stated once for the advance kernels that offer
// it.  Wave 0 of the workgroup does it between two workgroup barriers: the sample is complete in LDS in front of the first, the used
// sample is complete in LDS behind the second.  The arithmetic is poly::project_wave, the device function of spoly_project: a sample
// projected here has the bits of the stand-alone call.  A sample without a projection (status -1, -2) is used as it is.
struct ReprojArgs {
    const double *A, *b;                // (rows x ny), (rows): Y, on the device
    int rows;
    double *Yu;                         // record (B x rows_x x ny) of the used samples (rows as the Y record), or null
    int32_t *proj;                      // record (B x rows_x) of the status words, or null
};
struct ReprojWave {                     // what a lane of wave 0 holds for the whole launch: its row of A, its b
    double ar[poly::PN], bi;
};
// the LDS of the re-projection in doubles, at the start of the launch's LDS: the wave's work area | the used sample (ny, padded to even)
__host__ __device__ inline int reproject_doubles(int ny) { return poly::LDS_BYTES / 8 + ((ny + 1) & ~1); }
__device__ __forceinline__ lptr reproject_used(lptr area) { return area + poly::LDS_BYTES / 8; }
__device__ __forceinline__ void reproject_load(const ReprojArgs &r, int ny, int lane, ReprojWave &yw) {
    poly::load_row((cgptr)r.A, (cgptr)r.b, r.rows, ny, lane, yw.ar, yw.bi);
}
// all 64 lanes of one wave: yu (ny) <- the sample the controller uses in place of y (ny); the status word of poly_dev.h
__device__ __forceinline__ int reproject_sample(const ReprojWave &yw, int rows, int ny, clptr y, lptr yu, lptr area, int lane) {
    return poly::status_word(poly::project_wave(yw.ar, yw.bi, rows, ny, y, yu, poly::carve(area), lane, poly::MAX_ITER));
}

// The same for an observer map that reads y - z_ref (the two advance kernels of gusto_ssm_loop.hip), between the barrier behind the sample
// y (no, LDS) and the estimate: yu <- the used sample, yd <- yu - zref, the record rows Yur (no) / pjr (one word) unless null.  All nt
// threads of the workgroup; ends with a sync.  Returns the status word (valid in wave 0).
__device__ __forceinline__ int reproject_measurement(const ReprojWave &yw, int rows, int no, clptr y, lptr yu, lptr area, clptr zref, lptr yd,
                                                     gptr Yur, giptr pjr, int tid, int nt) {
    int pj = 0;
    if (__builtin_amdgcn_readfirstlane(tid >> 6) == 0) {
        pj = reproject_sample(yw, rows, no, y, yu, area, tid & 63);
        if ((tid & 63) == 0 && pjr != nullptr) *pjr = pj;
    }
    __syncthreads();
    for (int e = tid; e < no; e += nt) {
        const double v = yu[e];
        yd[e] = v - zref[e];
        if (Yur != nullptr) Yur[e] = v;
    }
    __syncthreads();
    return pj;
}

struct PrepArgs {
    int N, n, m, nz, T;
    int first, idx0;                    // first period after a reset: no shift (the guess is the planner's zero-input rollout)
    double tk, dt;
    const double *xcur, *xopt, *uopt;   // the states the plans start from (B x n: the plant's, or the filters' estimates), previous plan
    const double *xplant;               // observed loop: the plant states, for row 0 of the records (null: xcur)
    const double *tt, *tz, *tu, *phase; // target table (tz / tu / phase may be null)
    const double *H;                    // (nz x n) of the planner's model
    double *x0, *x_init, *u_init, *z, *zf, *ud;
    double *Xrec, *Zrec;                // row 0 of the run's records (null: not this period / not wanted)
    int64_t rec_rows;                   // rows per rollout of Xrec / Zrec
};

// one workgroup per rollout: x0 <- plant state, the shifted guess, the target window
__global__ __launch_bounds__(256) void loop_prepare_kernel(PrepArgs a) {
    const size_t b = blockIdx.x;
    const int N = a.N, n = a.n, m = a.m, nz = a.nz, tid = threadIdx.x;
    cgptr xc = (cgptr)a.xcur + b * n;
    cgptr xr = a.xplant ? (cgptr)a.xplant + b * n : xc;
    gptr x0 = (gptr)a.x0 + b * n;
    for (int e = tid; e < n; e += 256) {
        x0[e] = xc[e];
        if (a.Xrec) ((gptr)a.Xrec)[b * (size_t)a.rec_rows * n + e] = xr[e];
    }
    if (a.Zrec) {
        cgptr H = (cgptr)a.H;
        for (int e = tid; e < nz; e += 256) ((gptr)a.Zrec)[b * (size_t)a.rec_rows * nz + e] = out_row(H, e, n, xr);
    }
    if (!a.first) {
        // rows idx0.. of the previous plan move to the front, its last row is held over the rest (ros.py:110-114)
        cgptr xo = (cgptr)a.xopt + b * (size_t)(N + 1) * n, uo = (cgptr)a.uopt + b * (size_t)N * m;
        gptr xi = (gptr)a.x_init + b * (size_t)(N + 1) * n, ui = (gptr)a.u_init + b * (size_t)N * m;
        for (int e = tid; e < (N + 1) * n; e += 256) {
            const int k = e / n, c = e - k * n;
            xi[e] = xo[(size_t)min(k + a.idx0, N) * n + c];
        }
        for (int e = tid; e < N * m; e += 256) {
            const int k = e / m, c = e - k * m;
            ui[e] = uo[(size_t)min(k + a.idx0, N - 1) * m + c];
        }
    }
    if (a.tz || a.tu) {
        const double t0 = a.tk + (a.phase ? ((cgptr)a.phase)[b] : 0.0);
        cgptr tt = (cgptr)a.tt;
        if (a.tz) {
            gptr z = (gptr)a.z + b * (size_t)(N + 1) * nz;
            for (int e = tid; e < (N + 1) * nz; e += 256) {
                const int k = e / nz, c = e - k * nz;
                const double v = table_at(tt, (cgptr)a.tz, a.T, nz, c, query_time(t0, a.dt, k));
                z[e] = v;
                if (a.zf && k == N) ((gptr)a.zf)[b * nz + c] = v;
            }
        }
        if (a.tu) {
            gptr ud = (gptr)a.ud + b * (size_t)N * m;
            for (int e = tid; e < N * m; e += 256) {
                const int k = e / m, c = e - k * m;
                ud[e] = table_at(tt, (cgptr)a.tu, a.T, m, c, query_time(t0, a.dt, k));
            }
        }
    }
}

}  // namespace
