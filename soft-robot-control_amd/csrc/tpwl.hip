// TPWL model on the device: nearest-point linearisation, table gather, batched rollout.
// Reference: sofacontrol/tpwl/tpwl.py:160-168 (calc_nearest_point), 236-270 (get_jacobians, nn),
// 193-216 (rollout), 336-339 (update_dynamics); sofacontrol/scp/models/tpwl.py:66-84.
#include "tpwl_host.h"

namespace {

__global__ void nearest_kernel(TpwlDev T, const double *__restrict__ X, int64_t B, int32_t *__restrict__ idx) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * nw + wave;
    if (k >= B) return;
    const int i = tpwl::nearest_wave(T, X + k * T.n);
    if ((threadIdx.x & 63) == 0) idx[k] = i;
}

// tpwl::nearest_many as the GuSTO kernels call it (one workgroup, the states in a row-major block), for stpwl_nearest_many
__global__ __launch_bounds__(512) void nearest_many_kernel(TpwlDev T, const double *__restrict__ X, int count, int32_t *__restrict__ idx) {
    tpwl::nearest_many(T, (cgptr)X, T.n, count, (giptr)idx);
}

__global__ void gather_kernel(TpwlDev T, const int32_t *__restrict__ idx, int64_t B, int discrete,
                              double *__restrict__ A, double *__restrict__ Bm, double *__restrict__ d) {
    const int64_t b = blockIdx.x;
    const int i = idx[b];
    cgptr As = (discrete ? T.Ad : T.Ac) + (size_t)i * T.n * T.n;
    cgptr Bs = (discrete ? T.Bd : T.Bc) + (size_t)i * T.n * T.m;
    cgptr ds = (discrete ? T.dd : T.dc) + (size_t)i * T.n;
    for (int e = threadIdx.x; e < T.n * T.n; e += blockDim.x) A[b * T.n * T.n + e] = As[e];
    for (int e = threadIdx.x; e < T.n * T.m; e += blockDim.x) Bm[b * T.n * T.m + e] = Bs[e];
    for (int e = threadIdx.x; e < T.n; e += blockDim.x) d[b * T.n + e] = ds[e];
}


// softmin weights over the stored points (tpwl.py:170-191): w_i = exp(-beta d_i / d_min) / sum_j(...),
// one-hot at the first minimum (the rule of tpwl_dev.h) when d_min == 0.  One workgroup per query state; W (B x P).
// A state that is not a number gives a row that is not a number (d_i / d_min is not one).
__global__ __launch_bounds__(256) void weights_kernel(TpwlDev T, const double *__restrict__ X, int64_t B,
                                                      double beta, double *__restrict__ W) {
    __shared__ double rv[256];
    __shared__ int ri[256];
    const int64_t b = blockIdx.x;
    const double *x = X + b * T.n;
    double *w = W + b * T.P;
    double best = INFINITY;                              // no candidate yet (the rule of tpwl_dev.h)
    int besti = 0;
    for (int i = threadIdx.x; i < T.P; i += blockDim.x) {
        double sq = 0.0, sv = 0.0;
        for (int j = 0; j < T.r; ++j) {
            const double e = T.qT[j * T.P + i] - x[T.r + j];
            sq = fma(e, e, sq);
        }
        if (T.w_v != 0.0) {                              // (the rule of tpwl_dev.h: w_v == 0 does not read the velocity)
            for (int j = 0; j < T.r; ++j) {
                const double f = T.vT[j * T.P + i] - x[j];
                sv = fma(f, f, sv);
            }
        }
        const double d = T.w_v != 0.0 ? T.w_q * sqrt(sq) + T.w_v * sqrt(sv) : T.w_q * sqrt(sq);     // (one expression, as ever: the same fma contraction)
        w[i] = d;
        if (d < best) { best = d; besti = i; }
    }
    rv[threadIdx.x] = best; ri[threadIdx.x] = besti;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double ob = rv[threadIdx.x + o];
            const int oi = ri[threadIdx.x + o];
            if (tpwl::goes_before(ob, oi, rv[threadIdx.x], ri[threadIdx.x])) {
                rv[threadIdx.x] = ob; ri[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const double dmin = rv[0];
    const int imin = ri[0];
    __syncthreads();
    if (dmin == 0.0) {
        for (int i = threadIdx.x; i < T.P; i += blockDim.x) w[i] = (i == imin) ? 1.0 : 0.0;
        return;
    }
    double part = 0.0;
    for (int i = threadIdx.x; i < T.P; i += blockDim.x) {
        const double e = exp(-beta * w[i] / dmin);
        w[i] = e;
        part += e;
    }
    rv[threadIdx.x] = part;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) rv[threadIdx.x] += rv[threadIdx.x + o];
        __syncthreads();
    }
    const double tot = rv[0];
    for (int i = threadIdx.x; i < T.P; i += blockDim.x) w[i] = w[i] / tot;
}

// weighted tables (tpwl.py:244-248): A = sum_i w_i A_c[i], B = sum_i w_i B_c[i], d = sum_i w_i d_c[i]
__global__ __launch_bounds__(256) void blend_kernel(TpwlDev T, const double *__restrict__ W, int64_t B,
                                                    double *__restrict__ A, double *__restrict__ Bm,
                                                    double *__restrict__ d) {
    const int64_t b = blockIdx.x;
    const double *w = W + b * T.P;
    const int nn = T.n * T.n, nm = T.n * T.m, tot = nn + nm + T.n;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < tot; e += gridDim.y * blockDim.x) {
        double s = 0.0;
        if (e < nn) {
            for (int i = 0; i < T.P; ++i) s = fma(w[i], T.Ac[(size_t)i * nn + e], s);
            A[b * nn + e] = s;
        } else if (e < nn + nm) {
            const int f = e - nn;
            for (int i = 0; i < T.P; ++i) s = fma(w[i], T.Bc[(size_t)i * nm + f], s);
            Bm[b * nm + f] = s;
        } else {
            const int f = e - nn - nm;
            for (int i = 0; i < T.P; ++i) s = fma(w[i], T.dc[(size_t)i * T.n + f], s);
            d[b * T.n + f] = s;
        }
    }
}

// one workgroup per rollout: x_{k+1} = A_d[i_k] x_k + B_d[i_k] u_k + d_d[i_k], i_k = nearest(x_k)
__global__ __launch_bounds__(256) void rollout_kernel(TpwlDev T, const double *__restrict__ x0,
                                                      const double *__restrict__ U, int N,
                                                      double *__restrict__ X, double *__restrict__ Z) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lptr xc = (lptr)smem;                                // n
    lptr xn = xc + T.n;                                  // n
    lptr uc = xn + T.n;                                  // m
    lptr part = uc + ((T.m + 3) & ~3);                   // blockDim
    liptr ip = (liptr)(part + blockDim.x);
    const int64_t b = blockIdx.x;
    const int n = T.n, m = T.m;
    double *Xb = X + b * (size_t)(N + 1) * n;
    for (int e = threadIdx.x; e < n; e += blockDim.x) { xc[e] = x0[b * n + e]; Xb[e] = xc[e]; }
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        if (threadIdx.x < 64) {
            const int i = tpwl::nearest_wave(T, xc);
            if (threadIdx.x == 0) *ip = i;
        }
        for (int e = threadIdx.x; e < m; e += blockDim.x) uc[e] = U[(b * N + k) * m + e];
        __syncthreads();
        const int i = *ip;
        // xn = A x + d  (via the transposed table: coalesced), then += B u: the L2-fed step of tpwl_dev.h
        if (n <= (int)blockDim.x) tpwl::step_l2(xn, T, i, n, m, xc, uc, part);
        else tpwl::step_l2_strided(xn, T, i, n, m, xc, uc, threadIdx.x, blockDim.x);      // (n_x > 256: wg::matTvec has no thread for the columns past blockDim.x)
        for (int e = threadIdx.x; e < n; e += blockDim.x) { xc[e] = xn[e]; Xb[(size_t)(k + 1) * n + e] = xn[e]; }
        __syncthreads();
    }
    if (Z != nullptr && T.H != nullptr) {
        double *Zb = Z + b * (size_t)(N + 1) * T.nz;
        for (int e = threadIdx.x; e < (N + 1) * T.nz; e += blockDim.x) {
            const int k = e / T.nz, a = e % T.nz;
            double s = 0.0;
            for (int j = 0; j < n; ++j) s = fma(T.H[a * n + j], Xb[(size_t)k * n + j], s);
            Zb[e] = s + T.z_ref[a];
        }
    }
}

// The same rollout with the region's panel [A_d^T | B_d^T | d_d] in LDS, reloaded (coalesced 16-byte loads) only when the nearest point
// changes, and both products of a stage under one barrier.  rollout_kernel reads the panel (31 KB at n_x = 60) from L2 at every stage
// and runs wg::matTvec twice: four barriers and two L2-fed products per stage.  Both are THE STEP RULE of tpwl_dev.h: X and Z are
// bit-identical to rollout_kernel's.
// HELD (w_v = 0, P <= 64, r <= 32, hence n <= 64: wave 0 owns the whole state): lane i of wave 0 keeps ITS table point in registers for
// the rollout and lane c < r the coordinate x[r + c] of the state the wave has just summed; the coordinates are broadcast with v_readlane as in
// tpwl::nearest_many -- same sums in the order j = 0, 1, ..., same sqrt, first minimum, index 0 for a state that is not a number --
// and the barrier between a stage's sums and the next search is not needed.  Otherwise wave 0 calls tpwl::nearest_wave on the LDS state.
template <bool HELD>
__global__ __launch_bounds__(256) void rollout_staged_kernel(TpwlDev T, const double *__restrict__ x0,
                                                             const double *__restrict__ U, int N,
                                                             double *__restrict__ X, double *__restrict__ Z) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = T.n, m = T.m, r = T.r;
    lptr xc = (lptr)smem;                                // n
    lptr uc = xc + n;                                    // m
    tpwl::StepLds L;                                     // partial sums, (two doubles) the point, the panel of region `cur`: every offset is even (n = 2 r)
    tpwl::step_carve(L, uc + ((m + 3) & ~3), n, m, blockDim.x, 2);
    liptr ip = (liptr)(L.pb + blockDim.x);
    const int64_t b = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int S = max(1, (int)blockDim.x / n), j = threadIdx.x % n, s = threadIdx.x / n;          // wg::matTvec's slices
    double *Xb = X + b * (size_t)(N + 1) * n;
    for (int e = threadIdx.x; e < n; e += blockDim.x) { xc[e] = x0[b * n + e]; Xb[e] = xc[e]; }
    // tq[c]: coordinate c of the lane's point, 0.0 for c >= r; xq: coordinate r + lane of the state (its position part), 0.0 for lane >= r.
    // A term c >= r of the search is then fma(0.0, 0.0, sq) = sq exactly, so the sums run in blocks of eight without a test per term.
    double tq[32], xq = 0.0;
    if constexpr (HELD) {
        if (wave == 0) {
            const int pl = lane < T.P ? lane : T.P - 1;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const double t = T.qT[(c < r ? c : r - 1) * T.P + pl];                     // unconditional (clamped) loads: all in flight at once
                tq[c] = c < r ? t : 0.0;
            }
            if (lane < r) xq = x0[b * n + r + lane];
        }
    }
    __syncthreads();
    int cur = -1;
    for (int k = 0; k < N; ++k) {
        if (wave == 0) {
            int i;
            if constexpr (HELD) {
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
            if (lane < m) uc[lane] = U[(b * N + k) * m + lane];                               // (m <= 16)
        }
        __syncthreads();
        const int i = *ip;
        if (i != cur) {                                  // (the same for every thread; the test is stated here too: the barrier is this kernel's)
            tpwl::panel_load(L, T, i, cur, n, m, threadIdx.x, blockDim.x);
            __syncthreads();
        }
        tpwl::step_slices(L, xc, uc, n, m, S, j, s);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const double v = tpwl::step_sum(L, n, S, threadIdx.x);
            xc[threadIdx.x] = v;
            Xb[(size_t)(k + 1) * n + threadIdx.x] = v;
        }
        if constexpr (HELD) {
            if (wave == 0) xq = lane < r ? xc[r + lane] : 0.0;                                // (written just above by this wave: LDS keeps a wave's order)
        }
        if constexpr (!HELD) __syncthreads();            // (HELD: only wave 0 touches the state before the next barrier)
    }
    if constexpr (HELD) __syncthreads();
    if (Z != nullptr && T.H != nullptr) {
        double *Zb = Z + b * (size_t)(N + 1) * T.nz;
        for (int e = threadIdx.x; e < (N + 1) * T.nz; e += blockDim.x) {
            const int k = e / T.nz, a = e % T.nz;
            double sum = 0.0;
            for (int c = 0; c < n; ++c) sum = fma(T.H[a * n + c], Xb[(size_t)k * n + c], sum);
            Zb[e] = sum + T.z_ref[a];
        }
    }
}

// f_i = A_c[j] x_i + B_c[j] u_i + d_c[j] at the stored points, j = nearest(x_i)  (models/tpwl.py:77-82)
__global__ __launch_bounds__(64) void char_kernel(TpwlDev T, double *__restrict__ xabs, double *__restrict__ fabs_) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lptr x = (lptr)smem;
    const int i = blockIdx.x, n = T.n, r = T.r;
    for (int e = threadIdx.x; e < n; e += 64) x[e] = e < r ? T.vT[e * T.P + i] : T.qT[(e - r) * T.P + i];
    __syncthreads();
    const int j = tpwl::nearest_wave(T, x);
    for (int e = threadIdx.x; e < n; e += 64) {
        double s = T.dc[(size_t)j * n + e];
        for (int c = 0; c < n; ++c) s = fma(T.Ac[((size_t)j * n + e) * n + c], x[c], s);
        for (int c = 0; c < T.m; ++c) s = fma(T.Bc[((size_t)j * n + e) * T.m + c], T.u[i * T.m + c], s);
        xabs[(size_t)i * n + e] = fabs(x[e]);
        fabs_[(size_t)i * n + e] = fabs(s);
    }
}

__global__ void colmax_kernel(const double *__restrict__ M, int rows, int cols, double *__restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    double v = 0.0;
    for (int i = 0; i < rows; ++i) v = fmax(v, M[(size_t)i * cols + c]);
    out[c] = v;
}

std::vector<double> transpose_batch(const double *src, int P, int rows, int cols) {
    std::vector<double> out((size_t)P * rows * cols);
    for (int p = 0; p < P; ++p)
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                out[((size_t)p * cols + j) * rows + i] = src[((size_t)p * rows + i) * cols + j];
    return out;
}

// Which kernel a rollout of the handle launches, and its dynamic LDS.  staged: the region panel in LDS (rollout_staged_kernel) when the
// layout fits the 64 KB a launch may ask for without an attribute (n_x <= 82 at n_u = 4) and the handle was not created under
// SRH_TPWL_ROLLOUT_PLAIN=1; held: the point table in registers (the limits of tpwl::nearest_many).
struct RolloutPlan { bool staged, held; size_t lds; };

RolloutPlan rollout_plan(const stpwl *h) {
    const size_t n = h->n, m = h->m, um = (m + 3) & ~(size_t)3;
    const size_t plain = sizeof(double) * (2 * n + um + 256) + 16;                              // two states, input, one partial buffer, index
    const size_t staged = srh::lds_request(sizeof(double) * (n + um + 2 + tpwl::step_doubles(h->n, h->m, 256)));      // state, input, index, the step's
    RolloutPlan p;
    p.staged = !h->rollout_plain && staged <= (size_t)64 * 1024;
    p.held = p.staged && h->w_v == 0.0 && h->P <= 64 && h->r <= 32;
    p.lds = p.staged ? staged : plain;
    return p;
}

int rollout_launch(const stpwl *h, const double *x0, const double *U, int N, int64_t batch, double *X, double *Z, hipStream_t stream) {
    const RolloutPlan p = rollout_plan(h);
    if (!p.staged) rollout_kernel<<<(unsigned)batch, 256, p.lds, stream>>>(h->view(), x0, U, N, X, Z);
    else if (p.held) rollout_staged_kernel<true><<<(unsigned)batch, 256, p.lds, stream>>>(h->view(), x0, U, N, X, Z);
    else rollout_staged_kernel<false><<<(unsigned)batch, 256, p.lds, stream>>>(h->view(), x0, U, N, X, Z);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

}  // namespace

TpwlDev stpwl::view() const {
    TpwlDev T{};
    T.P = P; T.r = r; T.n = n; T.m = m; T.nz = nz;
    T.w_q = w_q; T.w_v = w_v;
    auto g = [](const srh::DevBuf &b) { return (cgptr)b.as<double>(); };
    T.qT = g(qT); T.vT = g(vT); T.u = g(u);
    T.Ac = g(Ac); T.Bc = g(Bc); T.dc = g(dc);
    T.AcT = g(AcT); T.BcT = g(BcT);
    T.Ad = g(Ad); T.Bd = g(Bd); T.dd = g(dd);
    T.AdT = g(AdT); T.BdT = g(BdT);
    T.H = g(H); T.z_ref = g(z_ref);
    return T;
}

extern "C" {

int stpwl_set_discrete(stpwl_t *h, const double *A_d, const double *B_d, const double *d_d) {
    SRH_REQUIRE(h && A_d && B_d && d_d, "stpwl_set_discrete: null argument");
    int rc;
    const size_t nn = (size_t)h->P * h->n * h->n, nm = (size_t)h->P * h->n * h->m;
    auto AT = transpose_batch(A_d, h->P, h->n, h->n);
    auto BT = transpose_batch(B_d, h->P, h->n, h->m);
    // ekf_wide_kernel (observer.hip) reads A^T of a point as an MFMA operand in k-steps of 4: for n_x % 4 != 0 its last step reads up to
    // three rows past the point's n x n block (against zero rows of the other operand).  For every point but the last that is the next
    // point's table; behind the last one it was the end of the allocation.  Three rows of zeros make it the table's own.
    AT.resize(nn + 3 * (size_t)h->n, 0.0);
    if ((rc = h->Ad.upload(A_d, sizeof(double) * nn)) || (rc = h->Bd.upload(B_d, sizeof(double) * nm)) ||
        (rc = h->dd.upload(d_d, sizeof(double) * h->P * h->n)) ||
        (rc = h->AdT.upload(AT.data(), sizeof(double) * AT.size())) || (rc = h->BdT.upload(BT.data(), sizeof(double) * nm)))
        return rc;
    h->has_discrete = true;
    return SRH_OK;
}

int stpwl_create(stpwl_t **out, int P, int r, int n_u, const double *q, const double *v, const double *u,
                 const double *A_c, const double *B_c, const double *d_c, const double *A_d,
                 const double *B_d, const double *d_d, double w_q, double w_v) {
    SRH_REQUIRE(out && q && v && u && A_c && B_c && d_c, "stpwl_create: null argument");
    SRH_REQUIRE(P > 0 && r > 0 && n_u > 0 && n_u <= 16, "stpwl_create: need P, r > 0 and 0 < n_u <= 16");
    stpwl *h = new stpwl();
    h->P = P; h->r = r; h->n = 2 * r; h->m = n_u; h->nz = 0;
    h->w_q = w_q; h->w_v = w_v;
    if (const char *e = getenv("SRH_TPWL_ROLLOUT_PLAIN")) h->rollout_plain = atoi(e) != 0;        // (once per handle: nothing is read per launch)
    const int n = h->n, m = h->m;
    auto qT = transpose_batch(q, 1, P, r);
    auto vT = transpose_batch(v, 1, P, r);
    auto AT = transpose_batch(A_c, P, n, n);
    auto BT = transpose_batch(B_c, P, n, m);
    int rc;
    if ((rc = h->qT.upload(qT.data(), sizeof(double) * P * r)) || (rc = h->vT.upload(vT.data(), sizeof(double) * P * r)) ||
        (rc = h->u.upload(u, sizeof(double) * P * m)) ||
        (rc = h->Ac.upload(A_c, sizeof(double) * P * n * n)) || (rc = h->Bc.upload(B_c, sizeof(double) * P * n * m)) ||
        (rc = h->dc.upload(d_c, sizeof(double) * P * n)) ||
        (rc = h->AcT.upload(AT.data(), sizeof(double) * P * n * n)) || (rc = h->BcT.upload(BT.data(), sizeof(double) * P * n * m))) {
        delete h;
        return rc;
    }
    if (A_d && B_d && d_d) {
        if ((rc = stpwl_set_discrete(h, A_d, B_d, d_d))) { delete h; return rc; }
    }
    *out = h;
    return SRH_OK;
}

int stpwl_destroy(stpwl_t *h) {
    delete h;
    return SRH_OK;
}

int stpwl_set_output(stpwl_t *h, const double *H, const double *z_ref, int n_z) {
    SRH_REQUIRE(h && H && n_z > 0, "stpwl_set_output: null argument");
    std::vector<double> zr(n_z, 0.0);
    if (z_ref) zr.assign(z_ref, z_ref + n_z);
    int rc;
    if ((rc = h->H.upload(H, sizeof(double) * n_z * h->n)) || (rc = h->z_ref.upload(zr.data(), sizeof(double) * n_z)))
        return rc;
    h->nz = n_z;
    h->H_host.assign(H, H + (size_t)n_z * h->n);
    h->zref_host = zr;
    return SRH_OK;
}

int stpwl_nearest_dev(stpwl_t *h, const double *X_dev, int64_t B, int32_t *idx_dev, void *stream) {
    SRH_REQUIRE(h && X_dev && idx_dev, "stpwl_nearest_dev: null argument");
    if (B == 0) return SRH_OK;
    nearest_kernel<<<(unsigned)srh::cdiv(B, 4), 256, 0, (hipStream_t)stream>>>(h->view(), X_dev, B, idx_dev);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

int stpwl_nearest(stpwl_t *h, const double *X, int64_t B, int32_t *idx) {
    SRH_REQUIRE(h && X && idx, "stpwl_nearest: null argument");
    if (B == 0) return SRH_OK;
    srh::DevBuf dX, dI;
    int rc;
    if ((rc = dX.upload(X, sizeof(double) * B * h->n)) || (rc = dI.alloc(sizeof(int32_t) * B))) return rc;
    if ((rc = stpwl_nearest_dev(h, dX.as<double>(), B, dI.as<int32_t>(), nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return dI.download(idx, sizeof(int32_t) * B);
}

int stpwl_nearest_many(stpwl_t *h, const double *X, int count, int threads, int32_t *idx) {
    SRH_REQUIRE(h && X && idx, "stpwl_nearest_many: null argument");
    SRH_REQUIRE(count >= 1, "stpwl_nearest_many: need count >= 1");
    SRH_REQUIRE(threads == 256 || threads == 512, "stpwl_nearest_many: threads must be 256 or 512");
    srh::DevBuf dX, dI;
    int rc;
    if ((rc = dX.upload(X, sizeof(double) * count * h->n)) || (rc = dI.alloc(sizeof(int32_t) * count))) return rc;
    nearest_many_kernel<<<1, threads>>>(h->view(), dX.as<double>(), count, dI.as<int32_t>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return dI.download(idx, sizeof(int32_t) * count);
}

int stpwl_linearize(stpwl_t *h, const double *X, int64_t B, int discrete, double *A, double *Bm, double *d,
                    int32_t *idx) {
    SRH_REQUIRE(h && X && A && Bm && d, "stpwl_linearize: null argument");
    SRH_REQUIRE(!discrete || h->has_discrete, "stpwl_linearize: model has not been pre-discretised");
    if (B == 0) return SRH_OK;
    const int n = h->n, m = h->m;
    srh::DevBuf dX, dI, dA, dB, dd;
    int rc;
    if ((rc = dX.upload(X, sizeof(double) * B * n)) || (rc = dI.alloc(sizeof(int32_t) * B)) ||
        (rc = dA.alloc(sizeof(double) * B * n * n)) || (rc = dB.alloc(sizeof(double) * B * n * m)) ||
        (rc = dd.alloc(sizeof(double) * B * n)))
        return rc;
    if ((rc = stpwl_nearest_dev(h, dX.as<double>(), B, dI.as<int32_t>(), nullptr))) return rc;
    gather_kernel<<<(unsigned)B, 256>>>(h->view(), dI.as<int32_t>(), B, discrete, dA.as<double>(), dB.as<double>(), dd.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    if ((rc = dA.download(A, sizeof(double) * B * n * n)) || (rc = dB.download(Bm, sizeof(double) * B * n * m)) ||
        (rc = dd.download(d, sizeof(double) * B * n)))
        return rc;
    if (idx) return dI.download(idx, sizeof(int32_t) * B);
    return SRH_OK;
}

int stpwl_weights(stpwl_t *h, const double *X, int64_t B, double beta, double *W) {
    SRH_REQUIRE(h && X && W, "stpwl_weights: null argument");
    if (B == 0) return SRH_OK;
    srh::DevBuf dX, dW;
    int rc;
    if ((rc = dX.upload(X, sizeof(double) * B * h->n)) || (rc = dW.alloc(sizeof(double) * B * h->P))) return rc;
    weights_kernel<<<(unsigned)B, 256>>>(h->view(), dX.as<double>(), B, beta, dW.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return dW.download(W, sizeof(double) * B * h->P);
}

int stpwl_linearize_weighted(stpwl_t *h, const double *X, int64_t B, double beta, double *A, double *Bm, double *d,
                             double *W) {
    SRH_REQUIRE(h && X && A && Bm && d, "stpwl_linearize_weighted: null argument");
    if (B == 0) return SRH_OK;
    const int n = h->n, m = h->m;
    srh::DevBuf dX, dW, dA, dB, dd;
    int rc;
    if ((rc = dX.upload(X, sizeof(double) * B * n)) || (rc = dW.alloc(sizeof(double) * B * h->P)) ||
        (rc = dA.alloc(sizeof(double) * B * n * n)) || (rc = dB.alloc(sizeof(double) * B * n * m)) ||
        (rc = dd.alloc(sizeof(double) * B * n)))
        return rc;
    weights_kernel<<<(unsigned)B, 256>>>(h->view(), dX.as<double>(), B, beta, dW.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    const int tot = n * n + n * m + n;
    blend_kernel<<<dim3((unsigned)B, (unsigned)srh::cdiv(tot, 256)), 256>>>(h->view(), dW.as<double>(), B,
                                                                            dA.as<double>(), dB.as<double>(),
                                                                            dd.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    if ((rc = dA.download(A, sizeof(double) * B * n * n)) || (rc = dB.download(Bm, sizeof(double) * B * n * m)) ||
        (rc = dd.download(d, sizeof(double) * B * n)))
        return rc;
    if (W) return dW.download(W, sizeof(double) * B * h->P);
    return SRH_OK;
}

int stpwl_rollout(stpwl_t *h, const double *x0, const double *U, int N, int64_t batch, double *X, double *Z) {
    SRH_REQUIRE(h && x0 && U && X, "stpwl_rollout: null argument");
    SRH_REQUIRE(h->has_discrete, "stpwl_rollout: model has not been pre-discretised");
    SRH_REQUIRE(N >= 0 && batch >= 0, "stpwl_rollout: negative size");
    SRH_REQUIRE(Z == nullptr || h->nz > 0, "stpwl_rollout: Need to set output or meas. model");
    if (batch == 0) return SRH_OK;
    const int n = h->n, m = h->m;
    srh::DevBuf d0, dU, dX, dZ;
    int rc;
    if ((rc = d0.upload(x0, sizeof(double) * batch * n)) || (rc = dU.upload(U, sizeof(double) * batch * N * m)) ||
        (rc = dX.alloc(sizeof(double) * batch * (N + 1) * n)))
        return rc;
    if (Z && (rc = dZ.alloc(sizeof(double) * batch * (N + 1) * h->nz))) return rc;
    if ((rc = rollout_launch(h, d0.as<double>(), dU.as<double>(), N, batch, dX.as<double>(), Z ? dZ.as<double>() : nullptr, nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    if ((rc = dX.download(X, sizeof(double) * batch * (N + 1) * n))) return rc;
    if (Z) return dZ.download(Z, sizeof(double) * batch * (N + 1) * h->nz);
    return SRH_OK;
}

int stpwl_rollout_dev(stpwl_t *h, const double *x0_dev, const double *U_dev, int N, int64_t batch, double *X_dev, double *Z_dev,
                      void *stream) {
    SRH_REQUIRE(h && x0_dev && U_dev && X_dev, "stpwl_rollout_dev: null argument");
    SRH_REQUIRE(h->has_discrete, "stpwl_rollout_dev: model has not been pre-discretised");
    SRH_REQUIRE(N >= 0 && batch >= 0, "stpwl_rollout_dev: negative size");
    SRH_REQUIRE(Z_dev == nullptr || h->nz > 0, "stpwl_rollout_dev: Need to set output or meas. model");
    if (batch == 0) return SRH_OK;
    return rollout_launch(h, x0_dev, U_dev, N, batch, X_dev, Z_dev, (hipStream_t)stream);
}

int stpwl_rollout_plan(stpwl_t *h, int N, int64_t batch, int *staged, int *held, size_t *lds_bytes) {
    SRH_REQUIRE(h, "stpwl_rollout_plan: null handle");
    SRH_REQUIRE(N >= 0 && batch >= 0, "stpwl_rollout_plan: negative size");
    const RolloutPlan p = rollout_plan(h);           // (the same for every horizon and batch: one workgroup per rollout)
    if (staged) *staged = p.staged ? 1 : 0;
    if (held) *held = p.held ? 1 : 0;
    if (lds_bytes) *lds_bytes = p.lds;
    return SRH_OK;
}

int stpwl_characteristic(stpwl_t *h, double *x_char, double *f_char) {
    SRH_REQUIRE(h && x_char && f_char, "stpwl_characteristic: null argument");
    const int n = h->n;
    srh::DevBuf xa, fa, xo, fo;
    int rc;
    if ((rc = xa.alloc(sizeof(double) * h->P * n)) || (rc = fa.alloc(sizeof(double) * h->P * n)) ||
        (rc = xo.alloc(sizeof(double) * n)) || (rc = fo.alloc(sizeof(double) * n)))
        return rc;
    char_kernel<<<h->P, 64, sizeof(double) * n>>>(h->view(), xa.as<double>(), fa.as<double>());
    colmax_kernel<<<(unsigned)srh::cdiv(n, 64), 64>>>(xa.as<double>(), h->P, n, xo.as<double>());
    colmax_kernel<<<(unsigned)srh::cdiv(n, 64), 64>>>(fa.as<double>(), h->P, n, fo.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    if ((rc = xo.download(x_char, sizeof(double) * n))) return rc;
    return fo.download(f_char, sizeof(double) * n);
}

}  // extern "C"
