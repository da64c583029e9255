// ROMPC baseline: resident control step of the linear reduced-order MPC with a Luenberger observer.
// reference: sofacontrol/baselines/rompc/rompc.py:57-89 (ROMPC.evaluate: u = ubar + K (x_hat - xbar), line 79, then
// observer.update), rompc/observer.py:30-46 (initialize: x_hat = V^T (x_f - x_ref); update: x_hat <- A x_hat + B u + d +
// L ((y - y_ref) - C x_hat); update_z: z = H x_hat + z_ref, or C x_hat + y_ref without an output model),
// rompc/rompc_utils.py:52-53 (update_state).
//
// FOLDED FORM: the kernels never see A and C apart.  F = A - L C is formed once on the host whenever the gains change
// (srompc_create / srompc_set_gains), so the update is x_hat <- [F | B | L] [x_hat ; u ; y - y_ref] + d: one product of
// inner dimension n_x + n_u + n_y, and C only stays in LDS when it doubles as the output map (H == NULL).
//
// One workgroup owns a tile of 16 problems.  It copies the packed constants ([F B L], K, H, d, y_ref, z_ref) to LDS once,
// keeps the tile [x_hat | u | y - y_ref] (16 rows) in LDS across all T steps of a launch, and forms the three products
// (K (x_hat - xbar), the update, the output) on v_mfma_f64_16x16x4_f64: problems are the 16 rows of the A operand, one
// 16-column block of the result per wave.  A problem's row of an MFMA result depends on that row of the operand alone, so a
// problem computes the same bits alone, inside any batch, by T steps or by one replay.  Rows of a ragged last tile are never
// read from or written to global memory (their LDS rows stay zero).
#include "rompc_host.h"
#include "dev_la.h"

#include <algorithm>
#include <mutex>
#include <vector>

namespace {

constexpr int RP_NT = 512;               // 8 waves: at most 8 column blocks of 16 per product
constexpr int RP_TILE = 16;              // problems per workgroup
constexpr int RP_MAX_DIM = 16 * (RP_NT / 64);
constexpr size_t RP_LDS_MAX = 160 * 1024;
typedef double rp_d4 __attribute__((ext_vector_type(4)));

struct RompcArgs {
    int64_t batch;
    int n, m, ny, nz, T;          // T == 0: outputs of the current estimate only
    int n4, m4, ny4, ld1, ldk;    // blocks rounded up to 4 (zero padded), row strides of [F B L] and of K / H
    int nconst;                   // doubles of the packed constants
    const double *consts;         // [F B L] (n x ld1) | K (m x ldk) | Hz (nz x ldk) | d (n) | y_ref (ny) | z_ref (nz)
    double *x;                    // (batch x n) estimate, read at the start and written at the end
    const double *Y;              // (T x batch x ny)
    const double *Ugiven;         // (T x batch x m) or NULL: feedback
    const double *Ubar, *Xbar;    // (T x batch x m), (T x batch x n) when Ugiven is NULL
    double *Uout, *Xout, *Zout;   // (max(T, 1) x batch x m | n | nz)
};

// acc (problem kk + 4 q, column `col`) = sum_k V[problem][k] M[col][k], k < 4 K4; V, M zero padded up to 4 K4
__device__ __forceinline__ rp_d4 rp_gemm(clptr V, int ldv, clptr M, int ldm, int K4, int col, bool colok, int l16, int kk) {
    rp_d4 acc = {0.0, 0.0, 0.0, 0.0};
    clptr vr = V + l16 * ldv + kk, mr = M + col * ldm + kk;
    int s = 0;
    for (; s + 4 <= K4; s += 4) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a[q] = vr[4 * (s + q)]; b[q] = colok ? mr[4 * (s + q)] : 0.0; }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q], acc, 0, 0, 0);
    }
    for (; s < K4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vr[4 * s], colok ? mr[4 * s] : 0.0, acc, 0, 0, 0);
    return acc;
}

__global__ void __launch_bounds__(RP_NT) rompc_kernel(RompcArgs a) {
    extern __shared__ __attribute__((aligned(16))) char rp_smem[];
    const int tid = SRH_TID;
    const int n = a.n, m = a.m, ny = a.ny, nz = a.nz, ld1 = a.ld1, ldk = a.ldk;
    lptr cs = (lptr)rp_smem;
    lptr M1 = cs, Kp = M1 + n * ld1, Hz = Kp + m * ldk, dv = Hz + nz * ldk, yref = dv + n, zref = yref + ny;
    lptr V = cs + a.nconst;                  // RP_TILE x ld1: [x_hat (n4) | u (m4) | y - y_ref (ny4)]
    lptr W = V + RP_TILE * ld1;              // RP_TILE x ldk: x_hat - xbar
    const int64_t p0 = (int64_t)blockIdx.x * RP_TILE;
    const int np = (int)min((int64_t)RP_TILE, a.batch - p0);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l16 = lane & 15, kk = lane >> 4;
    const int col = 16 * wave + l16;
    const int uoff = a.n4, yoff = a.n4 + a.m4;

    for (int e = tid; e < a.nconst; e += RP_NT) cs[e] = a.consts[e];
    for (int e = tid; e < RP_TILE * (ld1 + ldk); e += RP_NT) V[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < np * n; e += RP_NT) {
        const int p = e / n, i = e - p * n;
        V[p * ld1 + i] = a.x[(p0 + p) * n + i];
    }
    __syncthreads();

    // z = Hz x_hat + z_ref of the tile's current estimate into slot t of Zout
    auto outputs = [&](int t) {
        if (16 * wave < nz) {
            const bool ok = col < nz;
            const int c = ok ? col : nz - 1;
            const rp_d4 acc = rp_gemm(V, ld1, Hz, ldk, a.n4 >> 2, c, ok, l16, kk);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = kk + 4 * q;
                if (ok && p < np) a.Zout[((int64_t)t * a.batch + p0 + p) * nz + c] = acc[q] + zref[c];
            }
        }
    };
    if (a.T == 0) { outputs(0); return; }

    const bool feedback = a.Ugiven == nullptr;
    for (int t = 0; t < a.T; ++t) {
        const int64_t r0 = (int64_t)t * a.batch + p0;
        for (int e = tid; e < np * ny; e += RP_NT) {
            const int p = e / ny, j = e - p * ny;
            V[p * ld1 + yoff + j] = a.Y[(r0 + p) * ny + j] - yref[j];
        }
        if (feedback) {
            for (int e = tid; e < np * n; e += RP_NT) {
                const int p = e / n, i = e - p * n;
                W[p * ldk + i] = V[p * ld1 + i] - a.Xbar[(r0 + p) * n + i];
            }
        } else {
            for (int e = tid; e < np * m; e += RP_NT) {
                const int p = e / m, j = e - p * m;
                const double u = a.Ugiven[(r0 + p) * m + j];
                V[p * ld1 + uoff + j] = u;
                a.Uout[(r0 + p) * m + j] = u;
            }
        }
        __syncthreads();
        if (feedback) {
            // u = ubar + K (x_hat - xbar)                                              (rompc.py:79)
            if (16 * wave < m) {
                const bool ok = col < m;
                const int c = ok ? col : m - 1;
                const rp_d4 acc = rp_gemm(W, ldk, Kp, ldk, a.n4 >> 2, c, ok, l16, kk);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int p = kk + 4 * q;
                    if (ok && p < np) {
                        const double u = acc[q] + a.Ubar[(r0 + p) * m + c];
                        V[p * ld1 + uoff + c] = u;
                        a.Uout[(r0 + p) * m + c] = u;
                    }
                }
            }
            __syncthreads();
        }
        // x_hat <- [F B L] [x_hat ; u ; y - y_ref] + d                                 (observer.py:39, folded)
        rp_d4 acc = {0.0, 0.0, 0.0, 0.0};
        const bool xok = col < n;
        const int xc = xok ? col : n - 1;
        if (16 * wave < n) acc = rp_gemm(V, ld1, M1, ld1, (a.n4 + a.m4 + a.ny4) >> 2, xc, xok, l16, kk);
        __syncthreads();                       // every wave has read the old estimate
        if (16 * wave < n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = kk + 4 * q;
                if (xok && p < np) {
                    const double v = acc[q] + dv[xc];
                    V[p * ld1 + xc] = v;
                    a.Xout[(r0 + p) * n + xc] = v;
                }
            }
        }
        __syncthreads();
        outputs(t);                            // reads the x columns only; the next trip writes u / y columns and W
    }
    for (int e = tid; e < np * n; e += RP_NT) {
        const int p = e / n, i = e - p * n;
        a.x[(p0 + p) * n + i] = V[p * ld1 + i];
    }
}

inline int up4(int v) { return (v + 3) / 4 * 4; }

}  // namespace

// pack [F B L], K, Hz, d, y_ref, z_ref and send them to the device (blocking: set-up path)
static int rompc_upload_consts(srompc *h) {
    const int n = h->n, m = h->m, ny = h->ny, nz = h->nz, ld1 = h->ld1, ldk = h->ldk;
    std::vector<double> c((size_t)h->nconst, 0.0);
    double *M1 = c.data(), *Kp = M1 + (size_t)n * ld1, *Hz = Kp + (size_t)m * ldk, *dv = Hz + (size_t)nz * ldk, *yr = dv + n, *zr = yr + ny;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            M1[(size_t)i * ld1 + j] = h->fold(i, j);
        }
        for (int j = 0; j < m; ++j) M1[(size_t)i * ld1 + h->n4 + j] = h->B[(size_t)i * m + j];
        for (int j = 0; j < ny; ++j) M1[(size_t)i * ld1 + h->n4 + h->m4 + j] = h->L[(size_t)i * ny + j];
    }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < n; ++j) Kp[(size_t)i * ldk + j] = h->K[(size_t)i * n + j];
    const std::vector<double> &Ho = h->has_H ? h->H : h->C;
    for (int i = 0; i < nz; ++i)
        for (int j = 0; j < n; ++j) Hz[(size_t)i * ldk + j] = Ho[(size_t)i * n + j];
    std::copy(h->d.begin(), h->d.end(), dv);
    std::copy(h->yref.begin(), h->yref.end(), yr);
    std::copy(h->zref.begin(), h->zref.end(), zr);
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipMemcpy(h->consts.p, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice));
    return SRH_OK;
}

static int rompc_launch(srompc *h, int T, const double *Y, const double *Ug, const double *Ub, const double *Xb, double *Uo,
                        double *Xo, double *Zo) {
    RompcArgs a{};
    a.batch = h->batch; a.n = h->n; a.m = h->m; a.ny = h->ny; a.nz = h->nz; a.T = T;
    a.n4 = h->n4; a.m4 = h->m4; a.ny4 = h->ny4; a.ld1 = h->ld1; a.ldk = h->ldk; a.nconst = h->nconst;
    a.consts = h->consts.as<double>(); a.x = h->est();
    a.Y = Y; a.Ugiven = Ug; a.Ubar = Ub; a.Xbar = Xb; a.Uout = Uo; a.Xout = Xo; a.Zout = Zo;
    rompc_kernel<<<(unsigned)srh::cdiv(h->batch, RP_TILE), RP_NT, h->lds, h->stream>>>(a);
    SRH_CHECK_HIP(hipGetLastError());
    return SRH_OK;
}

// full-order states (batch x 2 n_f) through the handle's pinned block, projected straight into the estimate
static int rompc_enqueue_project(srompc *h, srom_t *rom, const double *x_full, const char *who) {
    int64_t n_f = 0;
    int r = 0;
    int rc = srom_dims(rom, &n_f, &r);
    if (rc) return rc;
    SRH_REQUIRE(2 * r == h->n, "%s: the POD basis gives %d reduced states, the model has %d", who, 2 * r, h->n);
    const size_t cnt = (size_t)h->batch * 2 * (size_t)n_f;
    if (h->xfull_doubles != cnt) {           // first use with this basis: the only allocation a step can make
        SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
        if (h->pin_xf) { (void)hipHostFree(h->pin_xf); h->pin_xf = nullptr; }
        h->xfull_doubles = 0;
        if ((rc = h->xfull.alloc(sizeof(double) * cnt))) return rc;
        SRH_CHECK_HIP(hipHostMalloc((void **)&h->pin_xf, sizeof(double) * cnt, hipHostMallocDefault));
        h->xfull_doubles = cnt;
    }
    std::memcpy(h->pin_xf, x_full, sizeof(double) * cnt);
    SRH_CHECK_HIP(hipMemcpyAsync(h->xfull.p, h->pin_xf, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream));
    return srom_project_dev(rom, SROM_X, h->xfull.as<double>(), h->batch, 2 * n_f, h->est(), h->n, (void *)h->stream);
}

static int rompc_mark(srompc *h, int which) {
    if (h->timing) SRH_CHECK_HIP(hipEventRecord(h->ev[which], h->stream));
    return SRH_OK;
}

// after the stream has drained: the device-side duration of the call
static int rompc_elapsed(srompc *h) {
    if (!h->timing) return SRH_OK;
    float ms = 0.f;
    SRH_CHECK_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->last_ms = ms;
    return SRH_OK;
}

// the result block [u | x_hat | z] back through the pinned mirror: the one blocking wait of a call
static int rompc_collect(srompc *h, bool with_u, double *u_out, double *x_out, double *z_out) {
    const size_t Bt = (size_t)h->batch, off = with_u ? 0 : Bt * h->m;
    SRH_CHECK_HIP(hipMemcpyAsync(h->pin_out + off, h->res.as<double>() + off, sizeof(double) * (h->res_doubles - off),
                                 hipMemcpyDeviceToHost, h->stream));
    int rc = rompc_mark(h, 1);
    if (rc) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->step_waits += 1;
    if ((rc = rompc_elapsed(h))) return rc;
    if (with_u && u_out) std::memcpy(u_out, h->pin_out, sizeof(double) * Bt * h->m);
    if (x_out) std::memcpy(x_out, h->pin_out + Bt * h->m, sizeof(double) * Bt * h->n);
    if (z_out) std::memcpy(z_out, h->pin_out + Bt * (h->m + h->n), sizeof(double) * Bt * h->nz);
    return SRH_OK;
}

extern "C" {

int srompc_create(srompc_t **out, int64_t batch, int n_x, int n_u, int n_y, int n_z, const double *A_d, const double *B_d,
                  const double *d_d, const double *C, const double *y_ref, const double *H, const double *z_ref, const double *K,
                  const double *L) {
    SRH_REQUIRE(out, "srompc_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(A_d && B_d && d_d && C && y_ref && L, "srompc_create: A_d, B_d, d_d, C, y_ref and L are required");
    SRH_REQUIRE(batch > 0 && n_x > 0 && n_u > 0 && n_y > 0 && n_z > 0, "srompc_create: need batch, n_x, n_u, n_y, n_z > 0");
    SRH_REQUIRE(H || n_z == n_y, "srompc_create: without an output model z = C x + y_ref, so n_z must equal n_y = %d (got %d)", n_y, n_z);
    SRH_REQUIRE(!H || z_ref, "srompc_create: H given without z_ref");
    SRH_REQUIRE(n_x <= RP_MAX_DIM && n_u <= RP_MAX_DIM && n_y <= RP_MAX_DIM && n_z <= RP_MAX_DIM,
                "srompc_create: n_x = %d, n_u = %d, n_y = %d, n_z = %d: each is limited to %d", n_x, n_u, n_y, n_z, RP_MAX_DIM);
    const int n4 = up4(n_x), m4 = up4(n_u), ny4 = up4(n_y), ld1 = (n4 + m4 + ny4) | 1, ldk = n4 | 1;
    const size_t nconst = (size_t)n_x * ld1 + (size_t)(n_u + n_z) * ldk + n_x + n_y + n_z;
    const size_t lds_bytes = sizeof(double) * (nconst + (size_t)RP_TILE * (ld1 + ldk));
    SRH_REQUIRE(lds_bytes <= RP_LDS_MAX,
                "srompc_create: n_x = %d, n_u = %d, n_y = %d, n_z = %d need %zu bytes of LDS for [A - L C | B | L], K and the output map "
                "(limit %zu)%s", n_x, n_u, n_y, n_z, lds_bytes, RP_LDS_MAX, H ? "" : "; an output model H with fewer rows than C would fit");
    auto *h = new srompc();
    auto fail = [&](int code) { srompc_destroy(h); return code; };
    h->batch = batch; h->n = n_x; h->m = n_u; h->ny = n_y; h->nz = n_z; h->has_H = H != nullptr;
    h->n4 = n4; h->m4 = m4; h->ny4 = ny4; h->ld1 = ld1; h->ldk = ldk; h->nconst = (int)nconst;
    const size_t n = n_x, m = n_u, ny = n_y, nz = n_z, Bt = (size_t)batch;
    h->A.assign(A_d, A_d + n * n); h->B.assign(B_d, B_d + n * m); h->d.assign(d_d, d_d + n);
    h->C.assign(C, C + ny * n); h->yref.assign(y_ref, y_ref + ny);
    if (H) { h->H.assign(H, H + nz * n); h->zref.assign(z_ref, z_ref + nz); }
    else h->zref = h->yref;
    if (K) h->K.assign(K, K + m * n); else h->K.assign(m * n, 0.0);
    h->L.assign(L, L + n * ny);
    h->lds = srh::lds_request(lds_bytes);
    {
        static std::mutex mu;
        static size_t granted = 0;
        std::lock_guard<std::mutex> lock(mu);
        if (granted < h->lds) {
            if (hipFuncSetAttribute((const void *)rompc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) {
                srh::set_error("srompc_create: the dynamic LDS limit could not be raised to %zu bytes", h->lds);
                return fail(SRH_EHIP);
            }
            granted = h->lds;
        }
    }
    h->in_doubles = Bt * (ny + m + n);
    h->res_doubles = Bt * (m + n + nz);
    int rc;
    if ((rc = h->consts.alloc(sizeof(double) * nconst)) || (rc = h->in.alloc(sizeof(double) * h->in_doubles)) ||
        (rc = h->res.alloc(sizeof(double) * h->res_doubles)))
        return fail(rc);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&h->pin_in, sizeof(double) * h->in_doubles, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void **)&h->pin_out, sizeof(double) * h->res_doubles, hipHostMallocDefault) != hipSuccess ||
        hipMemset(h->res.p, 0, sizeof(double) * h->res_doubles) != hipSuccess) {
        srh::set_error("srompc_create: stream / pinned blocks failed");
        return fail(SRH_EHIP);
    }
    if ((rc = rompc_upload_consts(h))) return fail(rc);
    *out = h;
    return SRH_OK;
}

int srompc_destroy(srompc_t *h) {
    if (!h) return SRH_OK;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    if (h->pin_xf) (void)hipHostFree(h->pin_xf);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SRH_OK;
}

int srompc_set_gains(srompc_t *h, const double *K, const double *L) {
    SRH_REQUIRE(h && (K || L), "srompc_set_gains: null argument");
    if (K) h->K.assign(K, K + (size_t)h->m * h->n);
    if (L) h->L.assign(L, L + (size_t)h->n * h->ny);
    return rompc_upload_consts(h);
}

int srompc_set_state(srompc_t *h, const double *x) {
    SRH_REQUIRE(h && x, "srompc_set_state: null argument");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    SRH_CHECK_HIP(hipMemcpy(h->est(), x, sizeof(double) * (size_t)h->batch * h->n, hipMemcpyHostToDevice));
    return SRH_OK;
}

int srompc_get_state(srompc_t *h, double *x, double *z) {
    SRH_REQUIRE(h && (x || z), "srompc_get_state: null argument");
    int rc;
    if ((rc = rompc_mark(h, 0))) return rc;
    if (z && (rc = rompc_launch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h->zres()))) return rc;
    return rompc_collect(h, false, nullptr, x, z);
}

int srompc_initialize(srompc_t *h, srom_t *rom, const double *x_full, double *x_out, double *z_out) {
    SRH_REQUIRE(h && rom && x_full, "srompc_initialize: null argument");
    int rc;
    h->step_waits = 0;
    if ((rc = rompc_mark(h, 0))) return rc;
    if ((rc = rompc_enqueue_project(h, rom, x_full, "srompc_initialize"))) return rc;
    if ((rc = rompc_launch(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h->zres()))) return rc;
    return rompc_collect(h, false, nullptr, x_out, z_out);
}

int srompc_step(srompc_t *h, srom_t *rom, const double *x_full, const double *u_given, const double *ubar, const double *xbar,
                const double *y, double *u_out, double *x_out, double *z_out) {
    SRH_REQUIRE(h && y, "srompc_step: null argument (y is required)");
    SRH_REQUIRE(u_given || (ubar && xbar), "srompc_step: need u_given, or ubar and xbar for the feedback u = ubar + K (x - xbar)");
    SRH_REQUIRE(!x_full || rom, "srompc_step: x_full given without the POD handle");
    const size_t Bt = (size_t)h->batch, n = h->n, m = h->m, ny = h->ny, D = sizeof(double);
    int rc;
    h->step_waits = 0;
    if ((rc = rompc_mark(h, 0))) return rc;
    // the pinned blocks are free: every call of the handle ends with the stream drained
    if (x_full && (rc = rompc_enqueue_project(h, rom, x_full, "srompc_step"))) return rc;
    std::memcpy(h->pin_in, y, D * Bt * ny);
    size_t cnt = Bt * (ny + m);
    if (u_given) std::memcpy(h->pin_in + Bt * ny, u_given, D * Bt * m);
    else {
        std::memcpy(h->pin_in + Bt * ny, ubar, D * Bt * m);
        std::memcpy(h->pin_in + Bt * (ny + m), xbar, D * Bt * n);
        cnt = h->in_doubles;
    }
    double *in = h->in.as<double>(), *r = h->res.as<double>();
    SRH_CHECK_HIP(hipMemcpyAsync(in, h->pin_in, D * cnt, hipMemcpyHostToDevice, h->stream));
    const double *uin = in + Bt * ny;
    if ((rc = rompc_launch(h, 1, in, u_given ? uin : nullptr, u_given ? nullptr : uin, u_given ? nullptr : in + Bt * (ny + m), r,
                           h->est(), h->zres())))
        return rc;
    if ((rc = rompc_collect(h, true, u_out, x_out, z_out))) return rc;
    h->steps += 1;
    return SRH_OK;
}

int srompc_replay(srompc_t *h, int T, const double *Y, const double *U_given, const double *Ubar, const double *Xbar,
                  double *U_out, double *X_out, double *Z_out) {
    SRH_REQUIRE(h && Y && T > 0, "srompc_replay: null argument, or T <= 0");
    SRH_REQUIRE(U_given || (Ubar && Xbar), "srompc_replay: need U_given, or Ubar and Xbar");
    const size_t Bt = (size_t)h->batch, n = h->n, m = h->m, ny = h->ny, nz = h->nz, D = sizeof(double), Tt = (size_t)T;
    srh::DevBuf dY, dU, dX, oU, oX, oZ;
    int rc;
    if ((rc = dY.upload(Y, D * Tt * Bt * ny)) || (rc = dU.upload(U_given ? U_given : Ubar, D * Tt * Bt * m)) ||
        (!U_given && (rc = dX.upload(Xbar, D * Tt * Bt * n))) || (rc = oU.alloc(D * Tt * Bt * m)) || (rc = oX.alloc(D * Tt * Bt * n)) ||
        (rc = oZ.alloc(D * Tt * Bt * nz)))
        return rc;
    h->step_waits = 0;
    if ((rc = rompc_mark(h, 0))) return rc;
    if ((rc = rompc_launch(h, T, dY.as<double>(), U_given ? dU.as<double>() : nullptr, U_given ? nullptr : dU.as<double>(),
                           U_given ? nullptr : dX.as<double>(), oU.as<double>(), oX.as<double>(), oZ.as<double>())))
        return rc;
    if ((rc = rompc_mark(h, 1))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->step_waits += 1;
    if ((rc = rompc_elapsed(h))) return rc;
    h->steps += T;
    if (U_out && (rc = oU.download(U_out, D * Tt * Bt * m))) return rc;
    if (X_out && (rc = oX.download(X_out, D * Tt * Bt * n))) return rc;
    if (Z_out && (rc = oZ.download(Z_out, D * Tt * Bt * nz))) return rc;
    return SRH_OK;
}

int srompc_stats(srompc_t *h, int64_t *steps, int64_t *waits_last_step) {
    SRH_REQUIRE(h, "srompc_stats: null handle");
    if (steps) *steps = h->steps;
    if (waits_last_step) *waits_last_step = h->step_waits;
    return SRH_OK;
}

int srompc_set_timing(srompc_t *h, int on) {
    SRH_REQUIRE(h, "srompc_set_timing: null handle");
    if (on && !h->ev[0])
        for (hipEvent_t &e : h->ev) SRH_CHECK_HIP(hipEventCreate(&e));
    h->timing = on != 0;
    h->last_ms = -1.0;
    return SRH_OK;
}

int srompc_last_device_ms(srompc_t *h, double *ms) {
    SRH_REQUIRE(h && ms, "srompc_last_device_ms: null argument");
    *ms = h->last_ms;
    return SRH_OK;
}

}  // extern "C"
