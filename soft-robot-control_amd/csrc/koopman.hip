// Koopman baseline: delay embedding, scaling and polynomial lift of the measurements, and a resident constant-(A, B)
// MPC step on top of the LOCP plan.
// reference: sofacontrol/baselines/koopman/koopman_utils.py (KoopmanData.get_zeta 30-47, add_zeta_offline 75-83,
// KoopmanScaling 86-107, KoopmanModel.get_lifting_function 156-175), koopman/koopman.py:75-125 (compute_policy: W lift(zeta)
// -> MPC request), baselines/ros.py:139-235 (MPCSolverNode: LOCP with is_tr_active=False and A_d, B_d constant over N).
#include "koopman_host.h"

#include <algorithm>
#include <functional>
#include <mutex>
#include <vector>

namespace {

constexpr int KP_MAX_NZ = 64;            // zeta dimension
constexpr int KP_MAX_DEG = 4;            // observable degree
constexpr int KP_MAX_PSI = 1024;         // observables (the largest tile: nz 43, degree 2 -- 16 rows x (992 + 43) doubles, 133 120 B of LDS)
constexpr size_t KP_LDS_TARGET = 64 * 1024;
typedef double kp_d4 __attribute__((ext_vector_type(4)));

// zeta element c of output row r: [y_t, y_{t-1} .. y_{t-delay}, u_{t-1} .. u_{t-delay}] (get_zeta, koopman_utils.py:30-47)
template <int MODE>
__device__ __forceinline__ double kp_zeta(const KoopLiftArgs &a, int64_t r, int c) {
    if (MODE == KP_ZETA) return a.zeta[r * a.nz + c];
    const int yb = a.ny * (a.delay + 1);
    const bool isy = c < yb;
    const int cc = isy ? c : c - yb;
    const int w = isy ? a.ny : a.m;
    const int j = cc / w + (isy ? 0 : 1), e = cc - (cc / w) * w;
    if (MODE == KP_RECORD) {
        const int64_t t = r + a.delay - j;
        // scale_down (koopman_utils.py:104-107): (v - offset) / factor, the same two operations
        return isy ? (a.y[t * a.ny + e] - a.yoff[e]) / a.yfac[e] : (a.u[t * a.m + e] - a.uoff[e]) / a.ufac[e];
    }
    int s = a.head - j;
    s += s < 0 ? a.slots : 0;
    return a.ring[(r * a.slots + s) * (a.ny + a.m) + (isy ? 0 : a.ny) + e];
}

// One block = TR rows: zeta tile -> psi tile in LDS (level by level, the recurrence of the observable table) -> either the
// psi tile straight out (coalesced: the tile's rows are contiguous in the output) or W psi on f64 MFMA from the LDS tile, so
// psi never goes through HBM.
template <int MODE, bool HAS_W>
__global__ void __launch_bounds__(KP_NT) koop_lift_kernel(KoopLiftArgs a) {
    extern __shared__ double kp_smem[];
    const int TR = a.TR, ld = a.ld, nz = a.nz, P = a.P;
    double *zt = kp_smem;                       // TR x nz
    double *ps = kp_smem + (size_t)TR * nz;     // TR x ld
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int rows = (int)min((int64_t)TR, a.rows - row0);
    for (int e = tid; e < TR * nz; e += KP_NT) {
        const int r = e / nz, c = e - r * nz;
        zt[e] = r < rows ? kp_zeta<MODE>(a, row0 + r, c) : 0.0;
    }
    // the padding columns P .. ld - 1 are read by the MFMA k loop: zeros
    const int padc = ld - P;
    for (int e = tid; e < TR * padc; e += KP_NT) {
        const int r = e / padc;
        ps[r * ld + P + (e - r * padc)] = 0.0;
    }
    __syncthreads();
    for (int L = 0; L < a.nlev; ++L) {
        const int k0 = a.lev[L], nk = a.lev[L + 1] - k0;
        for (int e = tid; e < TR * nk; e += KP_NT) {
            const int r = e / nk, k = k0 + (e - r * nk);
            const int p = a.par[k];
            ps[r * ld + k] = (p < 0 ? 1.0 : ps[r * ld + p]) * zt[r * nz + a.var[k]];
        }
        __syncthreads();
    }
    if (a.has_const) {
        for (int r = tid; r < TR; r += KP_NT) ps[r * ld + P - 1] = 1.0;
        __syncthreads();
    }
    if (!HAS_W) {
        double *o = a.out + row0 * P;
        for (int e = tid; e < rows * P; e += KP_NT) {
            const int r = e / P;
            o[e] = ps[r * ld + (e - r * P)];
        }
        return;
    }
    // out (rows x Nw) = psi (rows x P) W^T: 16 x 16 output tiles dealt to the waves; A operand psi[16 ti + l16][4 s + kk] from
    // LDS, B operand W[16 tj + l16][4 s + kk] from global (L2 resident: one W for every block), D row kk + 4 q, column l16
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l16 = lane & 15, kk = lane >> 4;
    const int TI = TR >> 4, TJ = (a.Nw + 15) >> 4, K4 = ld >> 2, Nw = a.Nw;
    for (int t = wave; t < TI * TJ; t += KP_NT / 64) {
        const int ti = t / TJ, tj = t - ti * TJ;
        const int col = 16 * tj + l16;
        const double *wr = a.W + (size_t)min(col, Nw - 1) * P;
        const bool colok = col < Nw;
        kp_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < K4; ++s) {
            const int k = 4 * s + kk;
            const double bv = (colok && k < P) ? wr[k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ps[(16 * ti + l16) * ld + k], bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * ti + kk + 4 * q;
            if (r < rows && colok) a.out[(row0 + r) * Nw + col] = acc[q];
        }
    }
}

// one scaled sample per problem into slot `head` of its ring: raw (batch x (ny + m)) = [y | u]
__global__ void koop_push_kernel(const double *__restrict__ raw, int64_t batch, int ny, int m, int slots, int head,
                                 const double *__restrict__ yoff, const double *__restrict__ yfac, const double *__restrict__ uoff,
                                 const double *__restrict__ ufac, double *__restrict__ ring) {
    const int w = ny + m;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * w) return;
    const int64_t b = i / w;
    const int e = (int)(i - b * w);
    const double v = raw[i];
    ring[(b * slots + head) * w + e] = e < ny ? (v - yoff[e]) / yfac[e] : (v - uoff[e - ny]) / ufac[e - ny];
}

// dst (count x len) = count copies of src (len)
__global__ void koop_tile_kernel(const double *__restrict__ src, int64_t len, int64_t count, double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len * count) dst[i] = src[i % len];
}

}  // namespace

// Observable order of get_lifting_function (koopman_utils.py:156-175): sorted(itermonomials(zeta, d), key=monomial_key('grlex',
// reversed(zeta))) -- graded, and within a degree ascending in the exponent tuple read from the LAST variable to the first
// (3 variables, degree 2: z1^2, z1 z2, z2^2, z1 z3, z2 z3, z3^2); the constant then moves to the end (DMD: dropped).
// Returned without the constant: (n x dim) exponents of degrees 1 .. degree.
static std::vector<int> koop_exponents(int dim, int degree) {
    std::vector<int> out;
    std::vector<std::vector<int>> lvl;
    for (int deg = 1; deg <= degree; ++deg) {
        lvl.clear();
        // every exponent vector of total degree `deg`
        std::vector<int> e(dim, 0);
        std::function<void(int, int)> rec = [&](int pos, int left) {
            if (pos == dim - 1) { e[pos] = left; lvl.push_back(e); return; }
            for (int v = 0; v <= left; ++v) { e[pos] = v; rec(pos + 1, left - v); }
        };
        rec(0, deg);
        std::sort(lvl.begin(), lvl.end(), [dim](const std::vector<int> &x, const std::vector<int> &y) {
            for (int i = dim - 1; i >= 0; --i)
                if (x[i] != y[i]) return x[i] < y[i];
            return false;
        });
        for (auto &v : lvl) out.insert(out.end(), v.begin(), v.end());
    }
    return out;
}

static int64_t koop_count(int dim, int degree) {
    // C(dim + degree, degree) - 1 without overflow for the sizes that are checked against the limits
    double c = 1.0;
    for (int i = 1; i <= degree; ++i) c = c * (dim + i) / i;
    return (int64_t)(c + 0.5) - 1;
}

struct skoop_mpc {
    skoop *h = nullptr;
    slocp_plan_t *qp = nullptr;
    int N = 0, n = 0, m = 0, nzo = 0;
    int64_t batch = 0;
    srh::DevBuf Ad, Bd, dd, del, om, tgt, res;
    size_t zoff = 0, zfoff = 0, udoff = 0, tgt_doubles = 0;
    bool have_z = false, have_zf = false, have_ud = false;
    size_t res_doubles = 0;
    double *pin = nullptr;        // targets in, results out
    bool horizon_resident = false;  // the tiled A / B went through the QP plan's transpose once (slocp_plan_solve_dev_resident)
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // step start, QP start, QP end, results copied
    int64_t steps = 0, step_waits = 0;
    double last_ms[4] = {-1.0, -1.0, -1.0, -1.0};
};

const void *koop_lift_fn(int mode, bool has_w) {
    const void *fn = nullptr;
#define KP_PICK(M, HW) if (mode == M && has_w == HW) fn = (const void *)koop_lift_kernel<M, HW>;
    KP_PICK(KP_ZETA, false) KP_PICK(KP_ZETA, true) KP_PICK(KP_RECORD, false) KP_PICK(KP_RECORD, true)
    KP_PICK(KP_RING, false) KP_PICK(KP_RING, true)
#undef KP_PICK
    return fn;
}

// Tile shape of a handle, and the dynamic-LDS limit of its three lift kernels raised to what it needs -- once, when the handle is
// created (a limit is only ever raised: another handle's larger tile keeps working), so a launch makes no attribute call.
static int koop_prepare_launch(skoop *h) {
    static std::mutex mu;
    static size_t granted[6] = {0, 0, 0, 0, 0, 0};
    h->ld = (h->P + 3) / 4 * 4;
    if (h->ld == h->P) h->ld += 4;   // some padding breaks the power-of-two LDS strides of the MFMA operand reads
    const size_t row_bytes = sizeof(double) * (size_t)(h->ld + h->nz);
    int TR = 64;
    while (TR > 16 && (size_t)TR * row_bytes > KP_LDS_TARGET) TR >>= 1;
    h->TR = TR;
    h->lds = srh::lds_request((size_t)TR * row_bytes);
    std::lock_guard<std::mutex> lock(mu);
    for (int mode = 0; mode < 3; ++mode) {
        const int slot = 2 * mode + (h->has_w ? 1 : 0);
        if (granted[slot] >= h->lds) continue;
        SRH_CHECK_HIP(hipFuncSetAttribute(koop_lift_fn(mode, h->has_w), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds));
        granted[slot] = h->lds;
    }
    return SRH_OK;
}

extern "C" {

int skoop_num_observables(int nzeta, int degree, int dmd) {
    if (nzeta <= 0 || degree <= 0) return 0;
    return (int)koop_count(nzeta, degree) + (dmd ? 0 : 1);
}

int skoop_exponents(int nzeta, int degree, int dmd, int32_t *exps) {
    SRH_REQUIRE(nzeta > 0 && degree > 0 && exps, "skoop_exponents: bad argument");
    SRH_REQUIRE(nzeta <= KP_MAX_NZ && degree <= KP_MAX_DEG && koop_count(nzeta, degree) + 1 <= KP_MAX_PSI,
                "skoop_exponents: need nzeta <= %d, degree <= %d and at most %d observables", KP_MAX_NZ, KP_MAX_DEG, KP_MAX_PSI);
    auto e = koop_exponents(nzeta, degree);
    std::copy(e.begin(), e.end(), exps);
    if (!dmd) std::fill(exps + e.size(), exps + e.size() + nzeta, 0);
    return SRH_OK;
}

int skoop_create(skoop_t **out, int n_y, int m, int delays, int degree, int dmd, const double *y_offset, const double *y_factor,
                 const double *u_offset, const double *u_factor, const double *W, int n_w, int64_t batch) {
    SRH_REQUIRE(out, "skoop_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(n_y > 0 && m > 0 && delays >= 0 && degree > 0 && batch > 0, "skoop_create: need n_y, m, degree, batch > 0 and delays >= 0");
    SRH_REQUIRE(y_offset && y_factor && u_offset && u_factor, "skoop_create: the four scale vectors are required");
    const int64_t nz = (int64_t)n_y * (delays + 1) + (int64_t)m * delays;
    SRH_REQUIRE(nz <= KP_MAX_NZ, "skoop_create: zeta dimension %lld exceeds %d", (long long)nz, KP_MAX_NZ);
    SRH_REQUIRE(degree <= KP_MAX_DEG, "skoop_create: observable degree %d exceeds %d", degree, KP_MAX_DEG);
    const int64_t P = koop_count((int)nz, degree) + (dmd ? 0 : 1);
    SRH_REQUIRE(P <= KP_MAX_PSI, "skoop_create: %lld observables exceed %d", (long long)P, KP_MAX_PSI);
    SRH_REQUIRE(!W || (n_w > 0 && n_w <= P), "skoop_create: W needs 0 < rows <= %lld observables", (long long)P);
    auto *h = new skoop();
    h->ny = n_y; h->m = m; h->delay = delays; h->degree = degree; h->dmd = dmd ? 1 : 0; h->nz = (int)nz; h->P = (int)P;
    h->Nw = W ? n_w : (int)P; h->batch = batch; h->slots = delays + 1;
    int rc = SRH_OK;
    auto fail = [&](int code) { skoop_destroy(h); return code; };
    // the recurrence table in the reference's order (constant, when kept, is handled by the kernel as the last column)
    const auto E = koop_exponents((int)nz, degree);
    const int nm = (int)(E.size() / nz);
    std::vector<int32_t> par(nm), var(nm), lev;
    {
        std::vector<std::vector<int>> rows(nm);
        for (int j = 0; j < nm; ++j) rows[j].assign(E.begin() + (size_t)j * nz, E.begin() + (size_t)(j + 1) * nz);
        int prev = 0;
        for (int j = 0; j < nm; ++j) {
            int deg = 0, last = 0;
            for (int i = 0; i < nz; ++i) { deg += rows[j][i]; if (rows[j][i]) last = i; }
            if (deg != prev) { lev.push_back(j); prev = deg; }
            var[j] = last;
            if (deg == 1) { par[j] = -1; continue; }
            std::vector<int> p = rows[j];
            p[last] -= 1;
            // the parent has degree deg - 1: search that level (graded order: it sits before j)
            int found = -1;
            for (int q = lev[lev.size() - 2]; q < lev.back(); ++q)
                if (rows[q] == p) { found = q; break; }
            par[j] = found;
            if (found < 0) { srh::set_error("skoop_create: internal error in the observable table"); return fail(SRH_EINVAL); }
        }
        lev.push_back(nm);
    }
    h->nlev = (int)lev.size() - 1;
    if ((rc = h->par.upload(par.data(), sizeof(int32_t) * nm)) || (rc = h->var.upload(var.data(), sizeof(int32_t) * nm)) ||
        (rc = h->lev.upload(lev.data(), sizeof(int32_t) * lev.size())))
        return fail(rc);
    std::vector<double> sc;
    sc.insert(sc.end(), y_offset, y_offset + n_y); sc.insert(sc.end(), y_factor, y_factor + n_y);
    sc.insert(sc.end(), u_offset, u_offset + m); sc.insert(sc.end(), u_factor, u_factor + m);
    if ((rc = h->scale.upload(sc.data(), sizeof(double) * sc.size()))) return fail(rc);
    if (W) {
        // the identity (the reference's default when the model has no W, koopman_utils.py:127-130) is not multiplied
        bool ident = n_w == P;
        for (int64_t i = 0; ident && i < (int64_t)n_w * P; ++i) ident = W[i] == ((i / P == i % P) ? 1.0 : 0.0);
        if (!ident) {
            h->has_w = true;
            if ((rc = h->W.upload(W, sizeof(double) * (size_t)n_w * P))) return fail(rc);
        } else {
            h->Nw = (int)P;
        }
    }
    if ((rc = koop_prepare_launch(h))) return fail(rc);
    const size_t w = (size_t)(n_y + m);
    if ((rc = h->ring.alloc(sizeof(double) * (size_t)batch * h->slots * w)) || (rc = h->stage.alloc(sizeof(double) * (size_t)batch * w)))
        return fail(rc);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **)&h->pin, sizeof(double) * (size_t)batch * w, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&h->pushed, hipEventDisableTiming) != hipSuccess) {
        srh::set_error("skoop_create: stream / pinned block / event creation failed");
        return fail(SRH_EHIP);
    }
    if (hipMemset(h->ring.p, 0, h->ring.bytes) != hipSuccess) { srh::set_error("skoop_create: hipMemset failed"); return fail(SRH_EHIP); }
    *out = h;
    return SRH_OK;
}

int skoop_destroy(skoop_t *h) {
    if (!h) return SRH_OK;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->pushed) (void)hipEventDestroy(h->pushed);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SRH_OK;
}

int skoop_info(skoop_t *h, int *nzeta, int *n_psi, int *n_out, int *has_w) {
    SRH_REQUIRE(h, "skoop_info: null handle");
    if (nzeta) *nzeta = h->nz;
    if (n_psi) *n_psi = h->P;
    if (n_out) *n_out = h->Nw;
    if (has_w) *has_w = h->has_w ? 1 : 0;
    return SRH_OK;
}

int skoop_lift_dev(skoop_t *h, const double *zeta_dev, int64_t rows, double *out_dev, void *stream) {
    SRH_REQUIRE(h && rows >= 0, "skoop_lift_dev: bad argument");
    if (rows == 0) return SRH_OK;
    SRH_REQUIRE(zeta_dev && out_dev, "skoop_lift_dev: null argument");
    KoopLiftArgs a{};
    a.rows = rows; a.zeta = zeta_dev; a.out = out_dev;
    return koop_launch_lift(h, KP_ZETA, a, (hipStream_t)stream);
}

int skoop_embed_lift_dev(skoop_t *h, const double *y_dev, const double *u_dev, int64_t T, double *out_dev, void *stream) {
    SRH_REQUIRE(h && T >= 0, "skoop_embed_lift_dev: bad argument");
    const int64_t rows = T - h->delay;
    if (rows <= 0) return SRH_OK;        // fewer than delay + 1 samples: no zeta (get_zeta returns None)
    SRH_REQUIRE(y_dev && u_dev && out_dev, "skoop_embed_lift_dev: null argument");
    KoopLiftArgs a{};
    a.rows = rows; a.y = y_dev; a.u = u_dev; a.out = out_dev;
    const double *s = h->scale.as<double>();
    a.yoff = s; a.yfac = s + h->ny; a.uoff = s + 2 * h->ny; a.ufac = s + 2 * h->ny + h->m;
    return koop_launch_lift(h, KP_RECORD, a, (hipStream_t)stream);
}

int skoop_lift(skoop_t *h, const double *zeta, int64_t rows, double *out) {
    SRH_REQUIRE(h && rows >= 0, "skoop_lift: bad argument");
    if (rows == 0) return SRH_OK;
    SRH_REQUIRE(zeta && out, "skoop_lift: null argument");
    srh::DevBuf z, o;
    int rc;
    if ((rc = z.upload(zeta, sizeof(double) * (size_t)rows * h->nz)) || (rc = o.alloc(sizeof(double) * (size_t)rows * h->Nw))) return rc;
    if ((rc = skoop_lift_dev(h, z.as<double>(), rows, o.as<double>(), nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return o.download(out, sizeof(double) * (size_t)rows * h->Nw);
}

int skoop_embed_lift(skoop_t *h, const double *y, const double *u, int64_t T, double *out) {
    SRH_REQUIRE(h && T >= 0, "skoop_embed_lift: bad argument");
    const int64_t rows = T - h->delay;
    if (rows <= 0) return SRH_OK;
    SRH_REQUIRE(y && u && out, "skoop_embed_lift: null argument");
    srh::DevBuf dy, du, o;
    int rc;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)T * h->ny)) || (rc = du.upload(u, sizeof(double) * (size_t)T * h->m)) ||
        (rc = o.alloc(sizeof(double) * (size_t)rows * h->Nw)))
        return rc;
    if ((rc = skoop_embed_lift_dev(h, dy.as<double>(), du.as<double>(), T, o.as<double>(), nullptr))) return rc;
    SRH_CHECK_HIP(hipStreamSynchronize(nullptr));
    return o.download(out, sizeof(double) * (size_t)rows * h->Nw);
}

int skoop_push(skoop_t *h, const double *y, const double *u) {
    SRH_REQUIRE(h && y && u, "skoop_push: null argument");
    const int w = h->ny + h->m;
    // the previous push's copy must have left the pinned block before it is rewritten; nothing to wait for when the stream has
    // been synchronised since (every MPC step ends with that)
    if (h->push_pending) {
        SRH_CHECK_HIP(hipEventSynchronize(h->pushed));
        h->host_waits += 1;
    }
    for (int64_t b = 0; b < h->batch; ++b) {
        std::memcpy(h->pin + b * w, y + b * h->ny, sizeof(double) * h->ny);
        std::memcpy(h->pin + b * w + h->ny, u + b * h->m, sizeof(double) * h->m);
    }
    SRH_CHECK_HIP(hipMemcpyAsync(h->stage.p, h->pin, sizeof(double) * (size_t)h->batch * w, hipMemcpyHostToDevice, h->stream));
    SRH_CHECK_HIP(hipEventRecord(h->pushed, h->stream));
    h->push_pending = true;
    const int head = (h->head + 1) % h->slots;
    const double *s = h->scale.as<double>();
    const int64_t tot = h->batch * w;
    koop_push_kernel<<<(unsigned)srh::cdiv(tot, 256), 256, 0, h->stream>>>(h->stage.as<double>(), h->batch, h->ny, h->m, h->slots, head,
                                                                           s, s + h->ny, s + 2 * h->ny, s + 2 * h->ny + h->m,
                                                                           h->ring.as<double>());
    SRH_CHECK_HIP(hipGetLastError());
    h->head = head;
    h->count += 1;
    return SRH_OK;
}

int skoop_reset(skoop_t *h) {
    SRH_REQUIRE(h, "skoop_reset: null handle");
    SRH_CHECK_HIP(hipStreamSynchronize(h->stream));
    h->push_pending = false;
    h->head = -1;
    h->count = 0;
    return SRH_OK;
}

int skoop_state_dev(skoop_t *h, const double **ring_dev, int *slots, int *head, int64_t *count, void **stream) {
    SRH_REQUIRE(h, "skoop_state_dev: null handle");
    if (ring_dev) *ring_dev = h->ring.as<double>();
    if (slots) *slots = h->slots;
    if (head) *head = h->head;
    if (count) *count = h->count;
    if (stream) *stream = (void *)h->stream;
    return SRH_OK;
}

int skoop_ring_lift_dev(skoop_t *h, double *out_dev) {
    SRH_REQUIRE(h && out_dev, "skoop_ring_lift_dev: null argument");
    SRH_REQUIRE(h->count >= h->delay + 1, "skoop_ring_lift_dev: %lld samples pushed, zeta needs delays + 1 = %d",
                (long long)h->count, h->delay + 1);
    KoopLiftArgs a{};
    a.rows = h->batch; a.ring = h->ring.as<double>(); a.head = h->head; a.out = out_dev;
    return koop_launch_lift(h, KP_RING, a, h->stream);
}

int skoop_mpc_create(skoop_mpc_t **out, skoop_t *h, const slocp_problem *prob, const double *A, const double *B) {
    SRH_REQUIRE(out && h && prob && A && B, "skoop_mpc_create: null argument");
    *out = nullptr;
    SRH_REQUIRE(!prob->tr_active, "skoop_mpc_create: the MPC QP has no trust region (is_tr_active=False, baselines/ros.py:161)");
    SRH_REQUIRE(prob->n_x == h->Nw, "skoop_mpc_create: n_x = %d but the lift writes %d states", prob->n_x, h->Nw);
    SRH_REQUIRE(prob->ndU == 0, "skoop_mpc_create: input-rate constraints are not supported here");
    auto *pl = new skoop_mpc();
    auto fail = [&](int code) { skoop_mpc_destroy(pl); return code; };
    pl->h = h; pl->N = prob->N; pl->n = prob->n_x; pl->m = prob->n_u; pl->nzo = prob->n_z; pl->batch = h->batch;
    int rc;
    if ((rc = slocp_plan_create(&pl->qp, prob, h->batch))) return fail(rc);
    const size_t N = pl->N, n = pl->n, m = pl->m, nz = pl->nzo, Bt = (size_t)pl->batch, D = sizeof(double);
    // constant A_d, B_d (d_d = 0) tiled over batch x N once (baselines/ros.py:163-169)
    srh::DevBuf a1, b1;
    if ((rc = a1.upload(A, D * n * n)) || (rc = b1.upload(B, D * n * m)) || (rc = pl->Ad.alloc(D * Bt * N * n * n)) ||
        (rc = pl->Bd.alloc(D * Bt * N * n * m)) || (rc = pl->dd.alloc(D * Bt * N * n)) || (rc = pl->del.alloc(D * Bt)) ||
        (rc = pl->om.alloc(D * Bt)))
        return fail(rc);
    const int64_t ca = (int64_t)(Bt * N);
    koop_tile_kernel<<<(unsigned)srh::cdiv(ca * (int64_t)(n * n), 256), 256, 0, h->stream>>>(a1.as<double>(), (int64_t)(n * n), ca, pl->Ad.as<double>());
    koop_tile_kernel<<<(unsigned)srh::cdiv(ca * (int64_t)(n * m), 256), 256, 0, h->stream>>>(b1.as<double>(), (int64_t)(n * m), ca, pl->Bd.as<double>());
    if (hipGetLastError() != hipSuccess || hipMemsetAsync(pl->dd.p, 0, pl->dd.bytes, h->stream) != hipSuccess ||
        hipMemsetAsync(pl->del.p, 0, pl->del.bytes, h->stream) != hipSuccess ||
        hipMemsetAsync(pl->om.p, 0, pl->om.bytes, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
        srh::set_error("skoop_mpc_create: tiling the horizon failed");
        return fail(SRH_EHIP);
    }
    // targets (z, zf, u_des) one device block, so a step sends them in one copy; results (x0, x, u, J, status) likewise
    pl->zoff = 0; pl->zfoff = Bt * (N + 1) * nz; pl->udoff = pl->zfoff + Bt * nz; pl->tgt_doubles = pl->udoff + Bt * N * m;
    pl->res_doubles = Bt * n + Bt * (N + 1) * n + Bt * N * m + Bt + Bt;
    if ((rc = pl->tgt.alloc(D * pl->tgt_doubles)) || (rc = pl->res.alloc(D * pl->res_doubles))) return fail(rc);
    if (hipHostMalloc((void **)&pl->pin, D * std::max(pl->tgt_doubles, pl->res_doubles), hipHostMallocDefault) != hipSuccess) {
        srh::set_error("skoop_mpc_create: pinned block");
        return fail(SRH_EHIP);
    }
    *out = pl;
    return SRH_OK;
}

int skoop_mpc_set_timing(skoop_mpc_t *pl, int on) {
    SRH_REQUIRE(pl, "skoop_mpc_set_timing: null plan");
    if (on && !pl->ev[0])
        for (hipEvent_t &e : pl->ev) SRH_CHECK_HIP(hipEventCreate(&e));
    pl->timing = on != 0;
    for (double &v : pl->last_ms) v = -1.0;
    return SRH_OK;
}

int skoop_mpc_stats(skoop_mpc_t *pl, int64_t *steps, int64_t *waits_last_step, double *ms) {
    SRH_REQUIRE(pl, "skoop_mpc_stats: null plan");
    if (steps) *steps = pl->steps;
    if (waits_last_step) *waits_last_step = pl->step_waits;
    if (ms) std::copy(pl->last_ms, pl->last_ms + 4, ms);
    return SRH_OK;
}

int skoop_mpc_destroy(skoop_mpc_t *pl) {
    if (!pl) return SRH_OK;
    if (pl->h && pl->h->stream) (void)hipStreamSynchronize(pl->h->stream);
    if (pl->qp) slocp_plan_destroy(pl->qp);
    for (hipEvent_t e : pl->ev)
        if (e) (void)hipEventDestroy(e);
    if (pl->pin) (void)hipHostFree(pl->pin);
    delete pl;
    return SRH_OK;
}

int skoop_mpc_step(skoop_mpc_t *pl, const double *y, const double *u_prev, const double *z, const double *zf, const double *u_des,
                   double *x0, double *x, double *u, double *J, int32_t *status) {
    SRH_REQUIRE(pl && x && u && J && status, "skoop_mpc_step: null argument");
    SRH_REQUIRE((y == nullptr) == (u_prev == nullptr), "skoop_mpc_step: y and u_prev come together (both NULL: no push)");
    skoop *h = pl->h;
    const hipStream_t st = h->stream;
    const int64_t waits0 = h->host_waits;
    int rc;
    if (pl->timing) SRH_CHECK_HIP(hipEventRecord(pl->ev[0], st));
    if (y && (rc = skoop_push(h, y, u_prev))) return rc;
    SRH_REQUIRE(h->count >= h->delay + 1, "skoop_mpc_step: %lld samples pushed, zeta needs delays + 1 = %d", (long long)h->count, h->delay + 1);
    const size_t N = pl->N, n = pl->n, m = pl->m, nz = pl->nzo, Bt = (size_t)pl->batch, D = sizeof(double);
    double *tg = pl->tgt.as<double>();
    // targets given this step go up (async, behind the lift's inputs); the others stay resident.  The pinned block is free: the
    // previous step synchronised before reading its results out of it
    auto up = [&](const double *src, size_t off, size_t cnt) -> int {
        std::memcpy(pl->pin + off, src, D * cnt);
        SRH_CHECK_HIP(hipMemcpyAsync(tg + off, pl->pin + off, D * cnt, hipMemcpyHostToDevice, st));
        return SRH_OK;
    };
    if (z && (rc = up(z, pl->zoff, Bt * (N + 1) * nz))) return rc;
    if (zf && (rc = up(zf, pl->zfoff, Bt * nz))) return rc;
    if (u_des && (rc = up(u_des, pl->udoff, Bt * N * m))) return rc;
    pl->have_z |= z != nullptr; pl->have_zf |= zf != nullptr; pl->have_ud |= u_des != nullptr;
    double *r = pl->res.as<double>();
    double *rx0 = r, *rx = rx0 + Bt * n, *ru = rx + Bt * (N + 1) * n, *rJ = ru + Bt * N * m;
    int32_t *rst = reinterpret_cast<int32_t *>(rJ + Bt);
    if ((rc = skoop_ring_lift_dev(h, rx0))) return rc;
    if (pl->timing) SRH_CHECK_HIP(hipEventRecord(pl->ev[1], st));
    // the tiled horizon is constant: its transpose is made by the first step only
    if ((rc = slocp_plan_solve_dev_resident(pl->qp, pl->horizon_resident ? 0 : 1, pl->Ad.as<double>(), pl->Bd.as<double>(), pl->dd.as<double>(),
                                            rx0, nullptr, pl->del.as<double>(), pl->om.as<double>(), pl->have_z ? tg + pl->zoff : nullptr,
                                            pl->have_zf ? tg + pl->zfoff : nullptr, pl->have_ud ? tg + pl->udoff : nullptr, rx, ru, nullptr,
                                            rJ, rst, nullptr, (void *)st)))
        return rc;
    pl->horizon_resident = true;
    if (pl->timing) SRH_CHECK_HIP(hipEventRecord(pl->ev[2], st));
    SRH_CHECK_HIP(hipMemcpyAsync(pl->pin, r, D * pl->res_doubles, hipMemcpyDeviceToHost, st));
    if (pl->timing) SRH_CHECK_HIP(hipEventRecord(pl->ev[3], st));
    SRH_CHECK_HIP(hipStreamSynchronize(st));
    h->host_waits += 1;
    h->push_pending = false;
    pl->steps += 1;
    pl->step_waits = h->host_waits - waits0;
    if (pl->timing) {
        float ms = 0.f;
        const int from[4] = {0, 1, 2, 0}, to[4] = {1, 2, 3, 3};
        for (int i = 0; i < 4; ++i) {
            SRH_CHECK_HIP(hipEventElapsedTime(&ms, pl->ev[from[i]], pl->ev[to[i]]));
            pl->last_ms[i] = ms;
        }
    }
    const double *p = pl->pin;
    if (x0) std::memcpy(x0, p, D * Bt * n);
    std::memcpy(x, p + Bt * n, D * Bt * (N + 1) * n);
    std::memcpy(u, p + Bt * n + Bt * (N + 1) * n, D * Bt * N * m);
    std::memcpy(J, p + Bt * n + Bt * (N + 1) * n + Bt * N * m, D * Bt);
    std::memcpy(status, p + Bt * n + Bt * (N + 1) * n + Bt * N * m + Bt, sizeof(int32_t) * Bt);
    return SRH_OK;
}

}  // extern "C"
