// SSM models: the k-step prediction error over records on the device (the open-loop model check of the reference,
// examples/hardware/diamond_SSM.py:83-140 module_test, as a unit that reads the records in place and starts every window from the
// observer map exactly as the planners start).
//
// THE SSM HORIZON ERROR ("SSM horizon error", defines it).
//   Records: y (E x T x n_y) raw measurements as SSMSysID.add takes them, u (E x T x m), row i holds the input applied after y_i; `stride`
//   s >= 1 keeps rows 0, s, 2s, .. (T' kept rows).
//   Model: an sssm handle with n_x == n_o == n_y, a mode (discrete map, fe, be, bil), dt and the handle's z_ref.
//   Observed states: xo_j = W_map(y_j - z_ref) = V phi_s(y_j - z_ref) for every kept row (SSM/controllers.py:302-310).
//   Windows: starts at the kept rows j0 = 0, w, 2w, .. (`every` = w >= 1) of every episode while j0 + H <= T' - 1, numbered episode by
//   episode in row order; an episode with T' <= H has none; W = 0 is refused.  The window rule of stpwl_horizon_plan.
//   Prediction: xh_0 = xo_{j0} (or x_start for every window); xh_{k+1} = A_d xh_k + B_d u_{j0+k} + d_d with (A_d, B_d, d_d) linearised at
//   (xh_k, u_{j0+k}) and discretised by the mode at dt; zh_k = C_map(xh_k) + z_ref.
//   Errors: ez_k = zh_k - y_{j0+k} (NOT zero at k = 0), ex_k = xh_k - xo_{j0+k} (exactly 0 at k = 0 without x_start).
//   Window status: 0 ok; 1 some xh_k or zh_k is not finite; 2 some record row the window reads (y at j0 .. j0 + H, u at j0 .. j0 + H - 1)
//   is not finite; 2 wins over 1 (a status-2 window is not rolled out).  Only status-0 windows enter the sums and the maxima.
//   Results for k = 0 .. H: sse (2 x (H + 1)) = sums of |ex_k|^2, |ez_k|^2; worst = the largest norm with the window that attains it (ties:
//   the lowest window number); counts.
//
// The arithmetic of a step is the SSM closed loop's plant step, called and not copied: ssm::stage once per workgroup, then per step
// ssm::jacobians_l, ssm::discretize, ssm_step_affine_row (ssm_step_dev.h), ssm::observe_l and (zeta + z_ref) in the order of
// ssm_loop_advance_kernel (gusto_ssm_loop.hip) at its 256 threads, and xo by THE ESTIMATE (ssm_step_estimate of ssm_step_dev.h: the loop
// unit keeps its own statement of it, ssm_loop_estimate, and tests hold the two equal in text and in bits): x_pred and z_pred are the
// X and Z + z_ref records of sgusto_ssm_loop_advance bit for bit.  (Not the bits of sssm_rollout: the staged evaluator sums in another
// order than ssm_rollout_kernel.)
// Arithmetic of the norms (one wave, fixed): lane l sums e_j^2 over j = l, l + 64, .. by fma from 0.0 (n_x, n_o <= 32: one term), the 64
// lane sums join in wg::wave_sum's fixed tree.  A norm is the correctly rounded sqrt of its square.
//
// Kernels.  sh_observe_kernel: a workgroup stages V and the ssm basis tables once and takes SH_OBS_ROWS consecutive kept rows in turn:
// y - z_ref into LDS, THE ESTIMATE into xo (E x T' x n_x, HBM), and the row's flags (bit 0: y not finite, bit 1: u not finite).
// Windows overlap whenever every < H: the map is evaluated once per row, not once per window that reads it.
// sh_window_kernel: a workgroup of 256 threads takes one block of consecutive windows of one episode (`block` windows, the plan's).  The
// model's tables are staged once per workgroup; xh, u, the linearisation and the work area stay in LDS across steps.  A window's status
// 2 is decided from the row flags before its first step.  Per step k: zeta = C_map(xh_k) (all threads); ex, ez by threads < n_x and
// 64 .. 64 + n_o, the input row by 128 .. 128 + m; wave 3 turns ex, ez into the two squared norms (a per-window row of LDS) while the
// other waves enter the linearisation of step k + 1; a window leaves its loop at the first xh_k or zh_k that is not finite.  The row is
// added to the block's accumulators (LDS; entry k always by the same thread) only when the window ends with status 0.
// sh_join_kernel joins the blocks' partial sums in block order and takes the maxima with their window numbers (strictly greater only:
// the lowest window number keeps a tie).  No floating-point atomics; blocks and rows are a function of the shapes alone, so the result
// does not depend on the CU count.  One stream, one host wait.
#include "ssm_host.h"
#include "ssm_step_dev.h"

#include <cmath>
#include <vector>

namespace {

constexpr int SH_NT = 256;                          // threads of both kernels: the loop kernel's
constexpr int SH_BLOCK = 16;                        // windows of a block ..
constexpr int64_t SH_BLOCKS = 2048;                 // .. doubled while the call would have more blocks than this (and an episode has more windows)
constexpr int SH_OBS_ROWS = 32;                     // kept rows of a workgroup of the observe pass
constexpr int SH_MAX_NX = 32, SH_MAX_M = 16;        // the handle's limit; the staged input matrix of ssm::stage
constexpr int SH_MAX_H = 1024;
constexpr int64_t SH_PRED_CAP = (int64_t)256 << 20; // bytes of x_pred + z_pred + x_obs a call may ask for
constexpr size_t SH_LDS_MAX = (size_t)160 * 1024;   // LDS of a CU (gfx950); a single workgroup may hold all of it
constexpr size_t SH_LDS_PLAIN = (size_t)64 * 1024;  // what a launch may ask for without the attribute

typedef __attribute__((address_space(3))) long long *llptr;

struct ShArgs {
    const double *Y, *U;                            // records (E x T x n_o), (E x T x m)
    const double *xo;                               // (E x T' x n) the observed states
    const int *bad;                                 // (E x T') flags of the kept rows
    const double *x_start;                          // (n) or null
    int64_t T, Tk, We, bpe, W;                      // rows and kept rows of an episode, its windows and blocks, windows of the call
    int H, stride, every, block, mode;
    double dt;
    double *part;                                   // (blocks x 4 x (H + 1)): sse_x, sse_z, worst_x, worst_z of every block
    long long *arg;                                 // (blocks x 2 x (H + 1)): the windows of worst_x, worst_z (-1: none)
    int *cnt;                                       // (blocks x 2): status-1 and status-2 windows
    double *fin;                                    // (2 x W) final_x, final_z, or null
    int *status;                                    // (W) or null
    double *xpred, *zpred;                          // (W x (H + 1) x n), (W x (H + 1) x n_o) or null
};

struct ShPlan { int64_t Tk, We, W, bpe, blocks; int block; size_t lds, lds_obs; };

// LDS of sh_window_kernel in doubles: [work area | xh, x', u (16), zeta, z_ref, ex, ez | A, B, d | the window's row (2 H1), the block's
// accumulators (4 H1), the windows of the maxima (2 H1), the flag (2) | the model's tables (ssm::stage)]
size_t sh_window_doubles(int n, int m, int no, int nr, int ns, int H1) {
    return ssm::work_doubles(n, m, no, nr, ns) + 3 * (size_t)n + 16 + 3 * (size_t)no + (size_t)n * n + (size_t)n * m + n + 8 * (size_t)H1 + 2 +
           ssm::lds_tab_doubles(n, no, nr, ns, 0);
}
// LDS of sh_observe_kernel in doubles: [V (n x ns) | phi (ns) | y - z_ref, z_ref (no each) | x_hat (n) | parent, variable (2 ns ints)]
size_t sh_observe_doubles(int n, int no, int ns) { return (size_t)n * ns + 2 * (size_t)ns + 2 * (size_t)no + n + 2; }

__device__ __forceinline__ bool sh_finite(double x) { return fabs(x) < INFINITY; }

// squared norms of ex (n doubles of LDS) and ez (no) by ONE wave
__device__ __forceinline__ void sh_norms(clptr ex, clptr ez, int n, int no, int lane, lptr sx_out, lptr sz_out) {
    double s = 0.0, t = 0.0;
    for (int j = lane; j < n; j += 64) s = fma(ex[j], ex[j], s);
    for (int j = lane; j < no; j += 64) t = fma(ez[j], ez[j], t);
    const double sx = wg::wave_sum(s), sz = wg::wave_sum(t);
    if (lane == 0) { *sx_out = sx; *sz_out = sz; }
}

// xo and the flags of SH_OBS_ROWS consecutive kept rows (numbered over all episodes); bad is zeroed in front of the launch
__global__ __launch_bounds__(SH_NT) void sh_observe_kernel(SsmDev S, const double *__restrict__ Y, const double *__restrict__ U, int64_t T, int64_t Tk,
                                                           int stride, int64_t rows, double *__restrict__ xo, int *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = S.n, m = S.m, no = S.no, ns = S.ns, tid = threadIdx.x, nt = SH_NT;
    lptr Vl = (lptr)smem;                                // n x ns
    lptr phi = Vl + (size_t)n * ns;                      // ns
    lptr yd = phi + ns, zr = yd + no, xh = zr + no;      // no, no, n
    liptr ps = (liptr)(xh + n), vs = ps + ns;            // ns ints each
    int lv[SSM_MAX_ORDER + 1];
    for (int q = 0; q <= SSM_MAX_ORDER; ++q) lv[q] = q <= S.order_s ? S.lvs[q] : 0;
    for (int e = tid; e < ns; e += nt) { ps[e] = S.ps[e]; vs[e] = S.vs[e]; }
    for (int e = tid; e < n * ns; e += nt) Vl[e] = S.Vc[e];
    for (int e = tid; e < no; e += nt) zr[e] = S.z_ref[e];
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * SH_OBS_ROWS, r1 = min(r0 + SH_OBS_ROWS, rows);
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t ep = r / Tk, j = r - ep * Tk, src = ep * T + j * stride;
        if (tid < no) {
            const double y = Y[src * no + tid];
            yd[tid] = y - zr[tid];
            if (!sh_finite(y)) atomicOr(bad + r, 1);
        } else if (tid >= 64 && tid < 64 + m) {
            if (!sh_finite(U[src * m + tid - 64])) atomicOr(bad + r, 2);
        }
        __syncthreads();
        ssm_step_estimate(ps, vs, lv, S.order_s, ns, no, n, yd, phi, Vl, xh, (gptr)(xo + r * n), tid, nt);
    }
}

__global__ __launch_bounds__(SH_NT) void sh_window_kernel(SsmDev S, ShArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = S.n, m = S.m, no = S.no, H = a.H, H1 = a.H + 1, tid = threadIdx.x, nt = SH_NT;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const bool dm = a.mode == SSM_DISCRETE_MAP;
    lptr base = (lptr)smem;
    ssm::Work w;
    ssm::carve(w, base, S);
    lptr xs = base + ssm::work_doubles(n, m, no, S.nr, S.ns);
    lptr xn = xs + n, us = xn + n;                       // n each, u: 16
    lptr zs = us + 16, zrl = zs + no;                    // zeta, z_ref
    lptr ex = zrl + no, ez = ex + n;                     // the two errors of the step
    lptr Al = ez + no, Bl = Al + (size_t)n * n, dl = Bl + (size_t)n * m;
    lptr row = dl + n;                                   // 2 H1     the window's |ex_k|^2, |ez_k|^2
    lptr acc = row + 2 * H1;                             // 4 H1     the block's sse_x, sse_z, worst_x, worst_z
    llptr arg = (llptr)(acc + 4 * H1);                   // 2 H1     the windows of the two maxima
    liptr flag = (liptr)(acc + 6 * H1);                  // the window's status bits
    lptr tab = acc + 6 * H1 + 2;
    SsmLds T;
    ssm::stage(T, tab, S, dm, 0);
    for (int k = tid; k < H1; k += nt) {
        acc[k] = 0.0; acc[H1 + k] = 0.0; acc[2 * H1 + k] = -1.0; acc[3 * H1 + k] = -1.0;
        arg[k] = -1; arg[H1 + k] = -1;
    }
    for (int e = tid; e < no; e += nt) zrl[e] = S.z_ref[e];
    if (tid == 0) *flag = 0;
    const int64_t b = blockIdx.x, ep = b / a.bpe, wl0 = (b - ep * a.bpe) * a.block;
    const int nwin = (int)min((int64_t)a.block, a.We - wl0);
    const double *Ye = a.Y + ep * a.T * no, *Ue = a.U + ep * a.T * m, *xoe = a.xo + ep * a.Tk * n;
    const int *bade = a.bad + ep * a.Tk;
    const int64_t ys = (int64_t)a.stride * no, ust = (int64_t)a.stride * m;                 // doubles between kept rows
    int ndiv = 0, nbad = 0;
    __syncthreads();

    for (int wi = 0; wi < nwin; ++wi) {
        const int64_t wl = wl0 + wi, win = ep * a.We + wl, j0 = wl * a.every;
        double *xp = a.xpred ? a.xpred + win * (int64_t)H1 * n : nullptr, *zp = a.zpred ? a.zpred + win * (int64_t)H1 * no : nullptr;
        {   // status 2: the flags of the rows the window reads (y at j0 .. j0 + H, u at j0 .. j0 + H - 1)
            int f = 0;
            for (int k = tid; k < H1; k += nt) {
                const int v = bade[j0 + k];
                f |= (v & 1) | (k < H ? (v & 2) : 0);
            }
            if (f) atomicOr((int *)flag, 2);
        }
        __syncthreads();
        int st = *flag ? 2 : 0, k = 0;                   // (the same for every thread)
        if (st == 0) {
            if (tid < n) xs[tid] = a.x_start ? a.x_start[tid] : xoe[j0 * n + tid];
            __syncthreads();
            for (;; ++k) {
                ssm::observe_l(S, T, xs, w, zs);         // zeta_k = C_map(xh_k)
                const int64_t jr = j0 + k;
                if (tid < n) {
                    const double x = xs[tid];
                    ex[tid] = x - xoe[jr * n + tid];
                    if (xp) xp[(int64_t)k * n + tid] = x;
                    if (!sh_finite(x)) atomicOr((int *)flag, 1);
                } else if (tid >= 64 && tid < 64 + no) {
                    const int o = tid - 64;
                    const double z = zs[o] + zrl[o];
                    ez[o] = z - Ye[jr * ys + o];
                    if (zp) zp[(int64_t)k * no + o] = z;
                    if (!sh_finite(z)) atomicOr((int *)flag, 1);
                } else if (tid >= 128 && tid < 128 + m) {
                    if (k < H) us[tid - 128] = Ue[jr * ust + tid - 128];
                }
                __syncthreads();
                if (*flag) break;                        // (written in front of the barrier only: the same for every thread)
                if (wave == 3) sh_norms(ex, ez, n, no, lane, row + k, row + H1 + k);        // while the other waves enter the linearisation
                if (k == H) break;
                ssm::jacobians_l(S, T, dm, xs, us, w, Al, n, Bl, dl);
                ssm::discretize(S, a.mode, a.dt, w, Al, n, Bl, dl);
                for (int i = tid; i < n; i += nt) xn[i] = ssm_step_affine_row(Al, Bl, dl, xs, us, n, m, i);
                __syncthreads();
                for (int e = tid; e < n; e += nt) xs[e] = xn[e];
                __syncthreads();
            }
            if (*flag) st = 1;
        }
        __syncthreads();                                 // the last row of norms is written; every thread has read the flag
        if (st == 0) {
            for (int q = tid; q < H1; q += nt) {         // entry q always by this thread
                const double sx = row[q], sz = row[H1 + q];
                acc[q] += sx;
                acc[H1 + q] += sz;
                const double nx = sqrt(sx), nzv = sqrt(sz);
                if (nx > acc[2 * H1 + q]) { acc[2 * H1 + q] = nx; arg[q] = win; }           // strictly greater: the first window keeps a tie
                if (nzv > acc[3 * H1 + q]) { acc[3 * H1 + q] = nzv; arg[H1 + q] = win; }
            }
        } else {                                         // the rows that were not formed (status 2: none was)
            const int first = st == 2 ? 0 : k + 1;
            if (xp) for (int e = first * n + tid; e < H1 * n; e += nt) xp[e] = NAN;
            if (zp) for (int e = first * no + tid; e < H1 * no; e += nt) zp[e] = NAN;
        }
        if (tid == 0) {
            ndiv += st == 1;
            nbad += st == 2;
            if (a.fin) {
                a.fin[win] = st == 0 ? sqrt(row[H]) : NAN;
                a.fin[a.W + win] = st == 0 ? sqrt(row[H1 + H]) : NAN;
            }
            if (a.status) a.status[win] = st;
            *flag = 0;
        }
        __syncthreads();                                 // the row and the flag are read; the next window may write them
    }
    double *po = a.part + b * 4 * (int64_t)H1;
    long long *ao = a.arg + b * 2 * (int64_t)H1;
    for (int q = tid; q < 4 * H1; q += nt) po[q] = acc[q];
    for (int q = tid; q < 2 * H1; q += nt) ao[q] = arg[q];
    if (tid == 0) { a.cnt[2 * b] = ndiv; a.cnt[2 * b + 1] = nbad; }
}

// entry (q, k) of the result: q = 0, 1 the sums in block order; q = 2, 3 the maxima with their windows; the counts by the first thread
__global__ __launch_bounds__(256) void sh_join_kernel(const double *__restrict__ part, const long long *__restrict__ arg, const int *__restrict__ cnt,
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
int sh_plan(const char *who, int n, int m, int no, int ny, int rom_order, int ssm_order, int mode, bool has_discrete, int64_t E, int64_t T, int H,
            int stride, int every, ShPlan *p) {
    SRH_REQUIRE(n >= 1 && n <= SH_MAX_NX, "%s: n_x = %d, need 1 <= n_x <= %d (the limit of an SSM handle)", who, n, SH_MAX_NX);
    SRH_REQUIRE(m >= 1 && m <= SH_MAX_M, "%s: m = %d, need 1 <= m <= %d", who, m, SH_MAX_M);
    SRH_REQUIRE(n == no, "%s: n_x = %d != n_o = %d: the reduced -> observed map needs n_x == n_o", who, n, no);
    SRH_REQUIRE(ny == no, "%s: n_y = %d != n_o = %d: the records' rows are the model's outputs", who, ny, no);
    SRH_REQUIRE(rom_order >= 1 && rom_order <= SSM_MAX_ORDER && ssm_order >= 1 && ssm_order <= SSM_MAX_ORDER,
                "%s: ROM_order = %d, SSM_order = %d, need 1 <= order <= %d", who, rom_order, ssm_order, SSM_MAX_ORDER);
    SRH_REQUIRE(mode != SSM_CONT, "%s: mode %d (continuous) has no step: give fe (1), be (2), bil (3) or the discrete map (4)", who, mode);
    SRH_REQUIRE(mode >= SSM_FE && mode <= SSM_DISCRETE_MAP, "%s: mode %d is not one of fe (1), be (2), bil (3), discrete map (4)", who, mode);
    SRH_REQUIRE(mode != SSM_DISCRETE_MAP || has_discrete, "%s: mode %d (discrete map) on a model without rd_coeff, Bd", who, mode);
    // (ssm::discretize forms sep B_c in an n x (n | 1) scratch panel)
    SRH_REQUIRE((mode != SSM_BE && mode != SSM_BIL) || m <= (n | 1), "%s: m = %d exceeds n_x | 1 = %d, the width of the B_d scratch panel of the be / bil "
                "discretisation", who, m, n | 1);
    SRH_REQUIRE(H >= 1 && H <= SH_MAX_H, "%s: H = %d, need 1 <= H <= %d", who, H, SH_MAX_H);
    SRH_REQUIRE(E >= 1 && T >= 1, "%s: need E >= 1 episodes of T >= 1 rows, got E = %lld, T = %lld", who, (long long)E, (long long)T);
    SRH_REQUIRE(stride >= 1, "%s: stride = %d, need stride >= 1", who, stride);
    SRH_REQUIRE(every >= 1, "%s: every = %d, need every >= 1", who, every);
    const int H1 = H + 1;
    p->Tk = (T - 1) / stride + 1;
    p->We = p->Tk > H ? (p->Tk - 1 - H) / every + 1 : 0;
    p->W = E * p->We;
    SRH_REQUIRE(p->W >= 1, "%s: W = 0 windows: T' = %lld kept rows per episode, H = %d needs T' >= %d", who, (long long)p->Tk, H, H + 1);
    int block = SH_BLOCK;
    while (E * srh::cdiv(p->We, block) > SH_BLOCKS && block < p->We) block *= 2;
    p->block = block;
    p->bpe = srh::cdiv(p->We, block);
    p->blocks = E * p->bpe;
    SRH_REQUIRE(p->blocks < ((int64_t)1 << 31) && srh::cdiv(E * p->Tk, SH_OBS_ROWS) < ((int64_t)1 << 31),
                "%s: %lld blocks of windows, %lld kept rows exceed the limit of 2^31 - 1 workgroups of a launch", who, (long long)p->blocks,
                (long long)(E * p->Tk));
    // (orders <= 7 in <= 32 variables: the counts fit 64 bits, not always an int)
    auto nmon = [](int dim, int order) { double c = 1.0; for (int i = 1; i <= order; ++i) c = c * (dim + i) / i; return c - 1.0; };
    const double nr_d = nmon(n, rom_order), ns_d = nmon(no, ssm_order);
    const double est = 8.0 * (nr_d * n + ns_d * no) ;
    SRH_REQUIRE(est <= (double)SH_LDS_MAX, "%s: the model's coefficient rows alone need %.0f bytes of LDS, above the 163840 bytes of a launch", who, est);
    const int nr = (int)nr_d, ns = (int)ns_d;
    p->lds = srh::lds_request(sizeof(double) * sh_window_doubles(n, m, no, nr, ns, H1));
    p->lds_obs = srh::lds_request(sizeof(double) * sh_observe_doubles(n, no, ns));
    SRH_REQUIRE(p->lds <= SH_LDS_MAX && p->lds_obs <= SH_LDS_MAX, "%s: the window kernel needs %zu bytes of LDS for the model's tables, the work area "
                "and 8 (H + 1) accumulators, above the 163840 bytes of a launch", who, p->lds > p->lds_obs ? p->lds : p->lds_obs);
    return SRH_OK;
}

int sh_check(const char *who, const sssm *h, const void *y, const void *u, const int64_t *counts, int mode, double dt) {
    SRH_REQUIRE(h, "%s: null handle", who);
    SRH_REQUIRE(y && u, "%s: null argument (the records)", who);
    SRH_REQUIRE(counts, "%s: null argument (counts)", who);
    SRH_REQUIRE(mode == SSM_DISCRETE_MAP || (dt > 0.0 && std::isfinite(dt)), "%s: dt = %g, need a finite dt > 0", who, dt);
    return SRH_OK;
}

int sh_plan_of(const char *who, const sssm *h, int mode, int ny, int64_t E, int64_t T, int H, int stride, int every, ShPlan *p) {
    return sh_plan(who, h->n, h->m, h->no, ny, h->order_r, h->order_s, mode, h->has_discrete, E, T, H, stride, every, p);
}

int sh_run(const char *who, const sssm *h, int mode, double dt, const double *y_dev, const double *u_dev, int ny, int64_t E, int64_t T, int H,
           int stride, int every, const double *x_start, double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms,
           int32_t *status, double *x_pred, double *z_pred, double *x_obs, hipStream_t st) {
    ShPlan p;
    int rc;
    if ((rc = sh_plan_of(who, h, mode, ny, E, T, H, stride, every, &p))) return rc;
    const int n = h->n, no = h->no, H1 = H + 1;
    const size_t D = sizeof(double), xp_bytes = D * (size_t)p.W * H1 * n, zp_bytes = D * (size_t)p.W * H1 * no, xo_bytes = D * (size_t)E * p.Tk * n;
    const size_t asked = (x_pred ? xp_bytes : 0) + (z_pred ? zp_bytes : 0) + (x_obs ? xo_bytes : 0);
    SRH_REQUIRE(asked <= (size_t)SH_PRED_CAP, "%s: x_pred, z_pred and x_obs of %lld windows x %d rows and %lld kept rows need %zu bytes, above the "
                "cap of %lld bytes", who, (long long)p.W, H1, (long long)(E * p.Tk), asked, (long long)SH_PRED_CAP);
    srh::DevBuf xo, bad, xs0, part, arg, cnt, out, oarg, ocnt, fin, stat, xpd, zpd;
    const int64_t rows = E * p.Tk;
    if ((rc = xo.alloc(xo_bytes)) || (rc = bad.alloc(sizeof(int) * (size_t)rows)) || (rc = part.alloc(D * (size_t)p.blocks * 4 * H1)) ||
        (rc = arg.alloc(sizeof(long long) * (size_t)p.blocks * 2 * H1)) || (rc = cnt.alloc(sizeof(int) * (size_t)p.blocks * 2)) ||
        (rc = out.alloc(D * 4 * H1)) || (rc = oarg.alloc(sizeof(long long) * 2 * H1)) || (rc = ocnt.alloc(sizeof(long long) * 2)))
        return rc;
    if (x_start && (rc = xs0.upload(x_start, D * n))) return rc;
    if (final_norms && (rc = fin.alloc(D * 2 * (size_t)p.W))) return rc;
    if (status && (rc = stat.alloc(sizeof(int) * (size_t)p.W))) return rc;
    if (x_pred && (rc = xpd.alloc(xp_bytes))) return rc;
    if (z_pred && (rc = zpd.alloc(zp_bytes))) return rc;
    const SsmDev S = h->view();
    SRH_CHECK_HIP(hipMemsetAsync(bad.p, 0, sizeof(int) * (size_t)rows, st));
    if (p.lds_obs > SH_LDS_PLAIN)
        SRH_CHECK_HIP(hipFuncSetAttribute((const void *)sh_observe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_obs));
    sh_observe_kernel<<<(unsigned)srh::cdiv(rows, SH_OBS_ROWS), SH_NT, p.lds_obs, st>>>(S, y_dev, u_dev, T, p.Tk, stride, rows, xo.as<double>(),
                                                                                        bad.as<int>());
    SRH_CHECK_HIP(hipGetLastError());
    ShArgs a{};
    a.Y = y_dev; a.U = u_dev; a.xo = xo.as<double>(); a.bad = bad.as<int>(); a.x_start = x_start ? xs0.as<double>() : nullptr;
    a.T = T; a.Tk = p.Tk; a.We = p.We; a.bpe = p.bpe; a.W = p.W;
    a.H = H; a.stride = stride; a.every = every; a.block = p.block; a.mode = mode; a.dt = dt;
    a.part = part.as<double>(); a.arg = arg.as<long long>(); a.cnt = cnt.as<int>();
    a.fin = final_norms ? fin.as<double>() : nullptr;
    a.status = status ? stat.as<int>() : nullptr;
    a.xpred = x_pred ? xpd.as<double>() : nullptr;
    a.zpred = z_pred ? zpd.as<double>() : nullptr;
    if (p.lds > SH_LDS_PLAIN)
        SRH_CHECK_HIP(hipFuncSetAttribute((const void *)sh_window_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    sh_window_kernel<<<(unsigned)p.blocks, SH_NT, p.lds, st>>>(S, a);
    SRH_CHECK_HIP(hipGetLastError());
    sh_join_kernel<<<(unsigned)srh::cdiv(4 * H1, 256), 256, 0, st>>>(a.part, a.arg, a.cnt, p.blocks, H1, out.as<double>(), oarg.as<long long>(),
                                                                     ocnt.as<long long>());
    SRH_CHECK_HIP(hipGetLastError());
    // everything comes back behind one wait
    std::vector<double> ho(4 * (size_t)H1);
    std::vector<long long> ha(2 * (size_t)H1);
    long long hc[2] = {0, 0};
    SRH_CHECK_HIP(hipMemcpyAsync(ho.data(), out.p, D * ho.size(), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipMemcpyAsync(ha.data(), oarg.p, sizeof(long long) * ha.size(), hipMemcpyDeviceToHost, st));
    SRH_CHECK_HIP(hipMemcpyAsync(hc, ocnt.p, sizeof(hc), hipMemcpyDeviceToHost, st));
    if (final_norms) SRH_CHECK_HIP(hipMemcpyAsync(final_norms, fin.p, D * 2 * (size_t)p.W, hipMemcpyDeviceToHost, st));
    if (status) SRH_CHECK_HIP(hipMemcpyAsync(status, stat.p, sizeof(int) * (size_t)p.W, hipMemcpyDeviceToHost, st));
    if (x_pred) SRH_CHECK_HIP(hipMemcpyAsync(x_pred, xpd.p, xp_bytes, hipMemcpyDeviceToHost, st));
    if (z_pred) SRH_CHECK_HIP(hipMemcpyAsync(z_pred, zpd.p, zp_bytes, hipMemcpyDeviceToHost, st));
    if (x_obs) SRH_CHECK_HIP(hipMemcpyAsync(x_obs, xo.p, xo_bytes, hipMemcpyDeviceToHost, st));
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

}  // namespace

extern "C" {

int sssm_horizon_plan(int n_x, int n_u, int n_o, int n_y, int rom_order, int ssm_order, int mode, int has_discrete, int64_t E, int64_t T,
                      int horizon, int stride, int every, int64_t *windows, int *block, int64_t *blocks, int64_t *lds_bytes, int64_t *launches,
                      int64_t *pred_cap_bytes) {
    if (windows) *windows = 0;
    if (block) *block = 0;
    if (blocks) *blocks = 0;
    if (lds_bytes) *lds_bytes = 0;
    if (launches) *launches = 0;
    if (pred_cap_bytes) *pred_cap_bytes = SH_PRED_CAP;
    ShPlan p;
    int rc;
    if ((rc = sh_plan("sssm_horizon_plan", n_x, n_u, n_o, n_y, rom_order, ssm_order, mode, has_discrete != 0, E, T, horizon, stride, every, &p)))
        return rc;
    if (windows) *windows = p.W;
    if (block) *block = p.block;
    if (blocks) *blocks = p.blocks;
    if (lds_bytes) *lds_bytes = (int64_t)p.lds;
    if (launches) *launches = 3;
    return SRH_OK;
}

int sssm_horizon_error_dev(sssm_t *h, int mode, double dt, const double *y_dev, const double *u_dev, int n_y, int64_t E, int64_t T, int horizon,
                           int stride, int every, const double *x_start, double *sse, double *worst, int64_t *worst_at, int64_t *counts,
                           double *final_norms, int32_t *status, double *x_pred, double *z_pred, double *x_obs, void *stream) {
    static const char *who = "sssm_horizon_error_dev";
    int rc;
    if ((rc = sh_check(who, h, y_dev, u_dev, counts, mode, dt))) return rc;
    return sh_run(who, h, mode, dt, y_dev, u_dev, n_y, E, T, horizon, stride, every, x_start, sse, worst, worst_at, counts, final_norms, status,
                  x_pred, z_pred, x_obs, (hipStream_t)stream);
}

int sssm_horizon_error(sssm_t *h, int mode, double dt, const double *y, const double *u, int n_y, int64_t E, int64_t T, int horizon, int stride,
                       int every, const double *x_start, double *sse, double *worst, int64_t *worst_at, int64_t *counts, double *final_norms,
                       int32_t *status, double *x_pred, double *z_pred, double *x_obs) {
    static const char *who = "sssm_horizon_error";
    int rc;
    if ((rc = sh_check(who, h, y, u, counts, mode, dt))) return rc;
    ShPlan p;
    if ((rc = sh_plan_of(who, h, mode, n_y, E, T, horizon, stride, every, &p))) return rc;                      // (refusals before the upload)
    srh::DevBuf dy, du;
    if ((rc = dy.upload(y, sizeof(double) * (size_t)E * (size_t)T * h->no)) || (rc = du.upload(u, sizeof(double) * (size_t)E * (size_t)T * h->m)))
        return rc;
    return sh_run(who, h, mode, dt, dy.as<double>(), du.as<double>(), n_y, E, T, horizon, stride, every, x_start, sse, worst, worst_at, counts,
                  final_norms, status, x_pred, z_pred, x_obs, nullptr);
}

}  // extern "C"
