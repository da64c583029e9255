// Lean condensed interior point for the LOCP QP (sofacontrol/scp/locp.py:218-342) -- the kernel the SCP loop spends its
// time in, as its own code path: no stage-wise Riccati solver inlined next to it (the fused kernel of locp_dev.h +
// locp_cond.h sits at 256 VGPRs with ~1.5 KB of scratch per lane for that reason), and the block lower-triangular
//     G[k][j] = C_o Phi(k, j+1) B_j          (N p_o x N m; locp_cond.h has the mathematics)
// RESIDENT IN LDS in packed form instead of streaming from L2 four to six times per Newton system.
//
// Packed G^T: row (j, b) (input b of stage j) holds only its structurally non-zero columns i = p_o j .. N p_o - 1, rows in
// the order (j, b); p_o = 2:  off(j) = m (j NP - j (j - 1)) doubles, element (j, b, i) at off(j) + b (NP - 2 j) + i - 2 j.
// The rows of the stages j >= j0 live in LDS (`Gt`), the first j0 stages -- the longest rows -- in the problem's L2 block
// (`gh`); j0 is the smallest value for which the carve fits into the 160 KB of a CU (7 at the Diamond shape: 61 of 82 KB
// in LDS; the Trunk's eight inputs leave room for the last 27 of 50 stages).
//
// What changes against locp_cond.h, phase by phase (same iteration, same iterates up to rounding):
//   condensation   writes G packed (LDS / L2 head) -- no zero fill of the structurally empty part
//   Gram matrix    K = I + Ls^T (G D^-1 G^T) Ls: MFMA operands straight from the packed rows (weights applied to the B
//                  operand in registers), causal k-ranges (a tile row stops at the last stage that reaches it), tiles
//                  distributed by a host-built schedule; Ls and the Jacobi scaling applied to the accumulators
//   G / G^T        products from LDS (+ the L2 head)
// Requirements (checked on the host: QPDims::lean): the condensed path applies, p_o = 2, diagonal input Hessians
// (diagD), n_u a multiple of 4.  Everything else stays on the fused kernel.
#pragma once
#include "locp_dev.h"

// compile-time loop: f(integral_constant<int, I>) for I = B .. E - 1
template <int B, int E, class F>
__device__ __forceinline__ void srh_static_for(F &&f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); srh_static_for<B + 1, E>(f); }
}

namespace ql {

using qpc::TS;
using qpc::TSZ;
using qpc::QR;
using qpc::Prof;

struct Lds : qpc::Lds {
    lptr Gt;           // packed G^T rows of the stages j >= j0
    lptr panel;        // [A | B] panel while condensing (aliases Rinv / the u-space temporaries)
    // half-size layout (QPDims::lean_half): the free response yf and the region sequence of the condensation live in the problem's L2
    // block behind the packed G (read once per QP), Rinv == B marks "inverse of a diagonal tile in the tile's own place" (rinv_tile)
    gptr yfg;
    giptr goffg;
    gptr gtoep;        // half-size layout: the Toeplitz generators g_b[0 .. NP) (b < m) of a single-region condensation, behind goffg in the L2 block
    int ypad;          // zeros behind ya / yd / yg (gT_times): 48, or 24 when a pass has 32 rows (256 threads)
    int ldTc;          // row pitch of Theta^T while condensing: 16 KT + 1, or the widest column pass + 1
};
// inverse of the J-th diagonal tile of the factor
__device__ __forceinline__ lptr rinv_tile(const Lds &L, int J, int KT) {
    return L.Rinv == L.B ? L.B + (size_t)qpc::tile_index(J, J, KT) * TSZ : L.Rinv + (size_t)J * TSZ;
}

__host__ __device__ inline int goff(int j, int m, int NP) { return m * (j * NP - j * (j - 1)); }     // p_o = 2
constexpr int YPAD = 48;               // zeros behind the y-space vectors that feed gT_times (see there)
// condense(): item slots per wave.  A stage has at most KT * (NPa / 16) MFMA items spread over the 8 waves; the host only
// enables the lean path when they fit (scp_host.h:build_consts) -- an item past the last slot would silently never be written.
constexpr int CONDENSE_SLOTS = 5;
constexpr int GRAM_TASKS = 32;         // entries of QPConst::gram_sched ({I, J0, nJ, 0}, longest first, nJ = 0 behind the last one)
__host__ __device__ inline bool condense_fits(const QPDims &d, int nwaves) { return d.KT * (d.NPa / 16) <= nwaves * CONDENSE_SLOTS; }

struct Sizes { size_t regX, thetaT, tiles, rinv, nm4, gt, ldi, ls, ldG, ua, tx, ld, idx, ypad, ldTc, nyv, nvv, nidx; };
// first column tile of the second condensation pass of the half-size layout (pass A: tiles [T, KT), pass B: [0, T))
__host__ __device__ inline int half_split_tile(int KT) { return KT / 2; }
__host__ __device__ inline Sizes sizes(const QPDims &d, int nthreads, int j0) {
    Sizes s;
    const bool half = d.lean_half != 0;
    const size_t nk = (size_t)d.NK, nm = (size_t)d.N * d.m;
    s.ldG = 16 * (size_t)d.KT;
    s.nm4 = (nm + 3) & ~(size_t)3;
    s.ldTc = half ? 16 * (size_t)(d.KT - half_split_tile(d.KT)) + 1 : s.ldG + 1;
    s.thetaT = nk * s.ldTc;
    s.tiles = (size_t)d.KT * (d.KT + 1) / 2 * TSZ;
    s.rinv = half ? 0 : (size_t)d.KT * TSZ;
    const size_t a = s.thetaT + nk * d.ld, b = s.tiles + s.rinv + 3 * s.nm4 + (size_t)nthreads;
    s.regX = ((a > b ? a : b) + 3) & ~(size_t)3;
    const int NP = d.N * d.po;
    s.gt = ((size_t)(goff(d.N, d.m, NP) - goff(j0, d.m, NP)) + 3) & ~(size_t)3;
    s.ldi = s.nm4;
    s.ls = (size_t)d.N * d.po * d.po;
    s.ua = half ? 0 : ((size_t)d.nU * d.m + 3) & ~(size_t)3;             // (ipm_box reads its row coefficients from global memory)
    s.tx = half ? 0 : ((size_t)(d.nX + d.nXf) * d.po + 3) & ~(size_t)3;
    s.ld = ((size_t)d.ld + 3) & ~(size_t)3;
    s.idx = ((size_t)(d.N / 2 + 2) + 3) & ~(size_t)3;
    s.ypad = half ? 24 : 48;
    s.nyv = half ? 7 : 9;                   // y-space vectors of their own (half: yf in L2, yb shares yd's place)
    s.nvv = half ? 0 : 2;                   // rollout vectors of their own (half: in du's place, dead while a rollout runs)
    s.nidx = half ? 1 : 2;                  // int arrays of their own (half: goff in L2)
    return s;
}
__host__ __device__ inline size_t lds_doubles(const QPDims &d, int nthreads, int j0) {
    const Sizes s = sizes(d, nthreads, j0);
    return s.regX + s.gt + s.ldi + s.ls + 2 * s.nm4 + s.nyv * s.ldG + 3 * s.ypad + s.ua + s.tx + s.nvv * s.ld + 16 + 16 + 4 + s.nidx * s.idx;
}
// doubles of the half-size layout's homes in the L2 block behind the packed G: [pad (YPAD) | yf (16 KT) | goff (N ints) | g (m NP)]
__host__ __device__ inline size_t half_l2_off(const QPDims &d) { return (size_t)goff(d.N, d.m, d.N * d.po) + 48; }
__host__ __device__ inline size_t half_l2_doubles(const QPDims &d) {
    return half_l2_off(d) + 16 * (size_t)d.KT + (((size_t)(d.N / 2 + 2) + 3) & ~(size_t)3) + (size_t)d.m * d.N * d.po;
}
// first stage whose packed rows, with those of every later stage, fit the K-tile area (what a staged Gram fill reads from LDS)
__host__ __device__ inline int gram_stage_j0(const QPDims &d) {
    const int NP = d.N * d.po, cap = d.KT * (d.KT + 1) / 2 * TSZ;
    int j = 0;
    while (goff(d.N, d.m, NP) - goff(j, d.m, NP) > cap) ++j;
    return j;
}
// ------------------------------------------------------------------ the row roster of tile_cholesky_set
// Who works in tile row J < KT - 1 of the set factorisation, and every counter target that follows from it, stated once for the device code
// and for the host replay (slean_roster_replay, tests/test_lean_roster_cpu.py).  Wave 0 of the protocol is the chain (the one-wave
// factorisations and the tile (J, J + 1)), wave w >= 1 is worker w - 1.  A roster is a code and the uniform worker count nwk0 behind code 0:
//    0: nwk0 workers in every row (the full-size workgroup: 3; the half-size one: wave 1 alone)
//   +k: wave 1 alone in the rows < k, waves 1, 2, 3 in the rows k .. KT - 2   (half-size: waves 2, 3 come from the Newton front)
//   -k: waves 1, 2, 3 in the rows < k, wave 1 alone from row k on              (half-size: waves 2, 3 leave for the Newton front)
// with 1 <= k <= KT - 2.  The workers of a row are always the waves 1 .. nwk(J): a wave skips a row it does not work in without
// touching a counter, and enters a row behind the CUMULATIVE arrivals of the rows before (whose acquire makes their tiles visible to it).
constexpr int LEAN_ROSTER_DEFAULT = -1;      // the half-size kernel's code unless SRH_LEAN_ROSTER says otherwise (chosen by measurement: DESIGN.md sections 39 and 49)
__host__ __device__ inline bool roster_legal(int KT, int code) { const int k = code < 0 ? -code : code; return code == 0 || (k >= 1 && k <= KT - 2); }
__host__ __device__ inline int roster_nwk(int code, int nwk0, int J) {
    if (code == 0) return nwk0;
    return (code > 0 ? J >= code : J < -code) ? 3 : 1;
}
__host__ __device__ inline bool roster_works(int code, int nwk0, int worker, int J) { return worker < roster_nwk(code, nwk0, J); }
// Ftrail in front of row J: one arrival per worker and row before (code 0: nwk0 J)
__host__ __device__ inline int roster_trail_target(int code, int nwk0, int J) {
    if (code == 0) return nwk0 * J;
    const int wide = code > 0 ? (J > code ? J - code : 0) : (J < -code ? J : -code);      // rows before J with three workers
    return J + 2 * wide;
}
// Fpanel when the whole panel of row J is written: the chain and every worker, rows 0 .. J (code 0: (nwk0 + 1) (J + 1))
__host__ __device__ inline int roster_panel_target(int code, int nwk0, int J) { return roster_trail_target(code, nwk0, J + 1) + J + 1; }
// Fnext in front of the chain's row J: two arrivals per row before, from the row's workers 0 and 1 (worker 0 alone where it is the only one)
__host__ __device__ inline int roster_next_target(int J) { return 2 * J; }
// a worker's panel tiles of row J: (J, Jp), Jp = first, first + nwk, .. < KT   ((J, J + 1) is the chain's)
__host__ __device__ inline int roster_panel_first(int worker, int J) { return J + 2 + worker; }
// Trailing tile t of row J, 1 <= t < ntr = rem (rem + 1) / 2 with rem = KT - J - 1 (tile 0 = (J + 1, J + 1) is the chain's); worker w takes
// t = w + 1, w + 1 + nwk, ..  The two tiles the chain needs for the NEXT row -- t = 1: (J + 1, J + 2), and (J + 2, J + 2), which changes
// places with t = 2 -- are the first tiles of workers 0 and 1, each announced on Fnext on its own (*first).  Tile (I, Kc) -= (J, I)^T (J, Kc).
__host__ __device__ inline int roster_ntr(int KT, int J) { const int rem = KT - J - 1; return rem * (rem + 1) / 2; }
__host__ __device__ inline void roster_trailing_tile(int KT, int J, int t, int &I, int &Kc, bool &first) {
    const int rem = KT - J - 1;
    int tt = (t == 2 && rem > 2) ? rem : ((t == rem && rem > 2) ? 2 : t), Ir = 0;
    first = (rem >= 2) && (t == 1 || tt == rem);
    while (tt >= rem - Ir) { tt -= rem - Ir; ++Ir; }
    I = J + 1 + Ir; Kc = I + tt;
}

// ------------------------------------------------------------------ the (column, chain) schedule of y = G u, half-size layout
// g_times_fixed sums column i of the packed G^T in four chains, chain c over the stages j = c, c + 4, .. <= i / 2 of every input in turn,
// and the chains meet only in (a0 + a1) + (a2 + a3).  The half-size kernel deals the triangle by TASK = (column, chain): the four tasks of
// a column sit in one quad of lanes, a wave-ROUND is 16 adjacent columns x 4 chains, and step s of a round is stage c + 4 s in every lane.
// The rounds, who runs them and what a lane reads are stated here once, for the device code (g_times_tasks) and for the host listing
// (slean_gu_schedule, tests/test_lean_gu_schedule_cpu.py).  NP = 2 NF columns; the two waves of an input class (GU_WAVES) share the rounds.
//   Round 0 has the columns [0, lead), round r >= 1 the columns [lead + 16 (r - 1), lead + 16 r) below NP.  lead is 8 when that saves a
//   step per round without adding a round (NP mod 16 in 1 .. 8), else 16: a round's length follows its LAST column, and with the columns a
//   multiple of 8 only its last two steps meet the triangle's edge.  NP = 100: 8 + 5 x 16 + 12 columns in 1, 3, .. 13 steps = 49 per
//   input (lead 16: 2, 4, .. 12, 13 = 55, the last round with four columns).
//   The rounds go to the waves longest first, each to the wave with the fewer steps so far (ties: the lower wave): NP = 100, wave 0 the
//   rounds 6, 3, 2 (25 steps), wave 1 the rounds 5, 4, 1, 0 (24).
constexpr int GU_WAVES = 2;                  // waves of one input class: CW = 128 threads
__host__ __device__ constexpr int gu_lead(int NP) { return (NP % 16 >= 1 && NP % 16 <= 8) ? 8 : 16; }
__host__ __device__ constexpr int gu_rounds(int NP) { return NP <= gu_lead(NP) ? 1 : 1 + (NP - gu_lead(NP) + 15) / 16; }
__host__ __device__ constexpr int gu_round_col0(int NP, int r) { return r == 0 ? 0 : gu_lead(NP) + 16 * (r - 1); }
__host__ __device__ constexpr int gu_round_ncols(int NP, int r) {
    const int end = gu_lead(NP) + 16 * r;
    return (end < NP ? end : NP) - gu_round_col0(NP, r);
}
// steps of round r: its last column i reaches the stages 0 .. i / 2
__host__ __device__ constexpr int gu_round_steps(int NP, int r) { return ((gu_round_col0(NP, r) + gu_round_ncols(NP, r) - 1) / 2) / 4 + 1; }
__host__ __device__ constexpr int gu_round_wave(int NP, int r) {
    int load[GU_WAVES] = {};
    for (int q = gu_rounds(NP) - 1; q >= 0; --q) {           // (the rounds' lengths ascend with r)
        int w = 0;
        for (int v = 1; v < GU_WAVES; ++v) if (load[v] < load[w]) w = v;
        if (q == r) return w;
        load[w] += gu_round_steps(NP, q);
    }
    return -1;
}
// steps s >= gu_first_edge_step have lanes outside the triangle (stage c + 4 s > i / 2 for some live (i, c)): the last two
__host__ __device__ constexpr int gu_first_edge_step(int NP, int r) { const int s = gu_round_steps(NP, r) - 2; return s < 0 ? 0 : s; }
// lane -> task: chain = lane & 3; the column of quad lane >> 2, a quad past the round's last column repeats that column (never stored)
__host__ __device__ constexpr int gu_lane_col(int NP, int r, int lane) {
    const int q = lane >> 2, nc = gu_round_ncols(NP, r);
    return gu_round_col0(NP, r) + (q < nc ? q : nc - 1);
}
__host__ __device__ constexpr bool gu_lane_stores(int NP, int r, int lane) { return (lane & 3) == 0 && (lane >> 2) < gu_round_ncols(NP, r); }
// Element (j, b, i) of the packed rows by the walk the device code takes: from the task's first stage c in steps of four stages,
//     R(c + 4 s, b) + i = R(c, b) + i + E(s) - s (8 M c + 8 b),   E(s) = s (4 M NP - 12 M - 8) - 16 M s (s - 1)
// (four times the recurrence of R in the products' header below); a lane outside the triangle reads element (0, b, i) instead -- inside
// the packed block and inside the generators, whatever the stage would have been.
__host__ __device__ constexpr int gu_walk_e(int M, int NP, int s) { return s * (4 * M * NP - 12 * M - 8) - 16 * M * s * (s - 1); }
__host__ __device__ constexpr int gu_index_packed(int M, int NP, int c, int s, int b, int i) {
    return M * (c * NP - c * (c - 1)) + b * (NP - 2 * c) - 2 * c + i + gu_walk_e(M, NP, s) - s * (8 * M * c + 8 * b);
}
__host__ __device__ constexpr int gu_index_toeplitz(int NP, int c, int s, int b, int i) { return b * NP + i - 2 * c - 8 * s; }
__host__ __device__ constexpr int gu_index_outside(int NP, int b, int i) { return b * NP + i; }

__device__ inline void lds_carve(Lds &L, lptr base, const QPDims &d, int nthreads, gptr work_base = nullptr) {
    const Sizes s = sizes(d, nthreads, d.lean_j0);
    const bool half = d.lean_half != 0;
    lptr p = base;
    auto take = [&](size_t c) { lptr q = p; p += c; return q; };
    lptr X = take(s.regX);
    // interior-point view: K tiles | inverses of the diagonal tiles | u-space temporaries | reduction scratch
    L.B = X; L.Rinv = half ? X : X + s.tiles;
    L.ta = X + s.tiles + s.rinv; L.tb = L.ta + s.nm4; L.tc = L.tb + s.nm4; L.part = L.tc + s.nm4;
    // condensation view: Theta^T (in L.B) | [A | B] panel
    L.panel = X + s.thetaT;
    L.A = L.panel;
    L.Gt = take(s.gt);
    L.Ldi = take(s.ldi); L.Ls = take(s.ls);
    L.u = take(s.nm4); L.du = take(s.nm4);
    L.y = take(s.ldG); L.dy = take(s.ldG);
    L.yf = half ? (lptr) nullptr : take(s.ldG);
    // ya, yd, yg feed gT_times: `ypad` zeros behind each (written once by ipm, never touched again)
    L.ya = take(s.ldG + s.ypad); L.yd = take(s.ldG + s.ypad); L.yg = take(s.ldG + s.ypad);
    L.yb = half ? L.yd : take(s.ldG);          // (yb = G t is dead once yc = ks Ls^T yb is formed; yd is written behind the K solve)
    L.yc = take(s.ldG); L.ks = take(s.ldG);
    L.UA = take(s.ua); L.Tx = take(s.tx);
    if (half) { L.v1 = L.du; L.v2 = L.du + s.ld; } else { L.v1 = take(s.ld); L.v2 = take(s.ld); }
    L.Qu = take(16); L.red = take(16);
    L.flag = (liptr)take(4);
    L.idxl = (liptr)take(s.idx);
    L.goff = half ? (liptr) nullptr : (liptr)take(s.idx);
    L.ypad = (int)s.ypad;
    L.ldTc = (int)s.ldTc;
    L.yfg = nullptr; L.goffg = nullptr; L.gtoep = nullptr;
    if (half && work_base != nullptr) {
        gptr hb = work_base + d.qc_off + half_l2_off(d);
        L.yfg = hb;
        L.goffg = (giptr)(hb + s.ldG);
        L.gtoep = hb + s.ldG + s.idx;
    }
}

// packed G^T: head rows in the problem's L2 block, the rest in LDS
// NF_ > 0: the horizon and the first LDS-resident stage are compile-time constants of the kernel instantiation (the fixed
// layouts of lean.hip) -- the products can then address every stage with immediate offsets (g_times_fixed)
template <int NF_ = 0, int J0F_ = 0>
struct GPackT {
    cgptr gh;          // rows of the stages j < j0
    clptr gt;          // rows of the stages j >= j0, offset so that gt[goff(j) + ...] addresses stage j
    int j0, m, NP;
    cgptr gto;         // the Toeplitz generators g_b[0 .. NP) when the L2-resident rows are their expansion (row (j, b) = g_b[0 .. NP - 2 j)), else null
    static constexpr int NF = NF_, J0F = J0F_;
};
using GPack = GPackT<0, 0>;

// ------------------------------------------------------------------ wave sets
// The factorisation of K is a chain of seven one-wave 16 x 16 factorisations with short all-wave phases in between (35 k of
// its 52 k clocks at C2 belong to wave 0 alone), and the first half of the Newton solve that follows -- G^T g_y, the dual
// residual, D^-1, G t, Ls^T -- does not depend on the factor.  ipm_box() therefore splits the workgroup for that stretch:
// one half of the waves factors, the other runs the products, and they meet again at an s_barrier.  The halves are taken BY
// SIMD (a workgroup's waves w and w + 4 share one: set 0 = waves 0, 1, 4, 5, set 1 = waves 2, 3, 6, 7), so that the wave
// with the one-wave factorisations shares its SIMD with a wave of its own set, which waits most of the time, and not with
// a wave that streams the products.  Inside the stretch a set cannot use
// s_barrier (it counts every wave of the workgroup): a set synchronises on its own monotone arrival counter in LDS -- each
// wave adds one and waits for the next multiple of the set size (the LDS pipe is in order per wave, so a wave's earlier
// LDS writes have landed when its arrival is seen; the workgroup-scope fences keep the compiler from moving accesses
// across and drain the global-memory counters).  HALF = false: the whole workgroup, plain s_barrier.
template <bool HALF>
struct Waves {
    int tid, nt, wave, nw;             // thread / wave index inside the set, set sizes
    liptr ctr;                         // HALF: arrival counter of this set (zeroed by the caller before the split)
    int target;
    bool sleepy;                       // HALF: s_sleep between polls (the set whose waits are long; the other polls back to back)
    __device__ __forceinline__ void sync() {
        if constexpr (!HALF) {
            __syncthreads();
        } else {
            target += nw;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if ((SRH_TID & 63) == 0) {
                __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target) { if (sleepy) __builtin_amdgcn_s_sleep(1); }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
};
__device__ __forceinline__ Waves<false> all_waves() {
    return Waves<false>{(int)SRH_TID, (int)blockDim.x, __builtin_amdgcn_readfirstlane((int)SRH_TID >> 6), (int)blockDim.x >> 6, (liptr) nullptr, 0, false};
}
// the two halves of an 8-wave workgroup by SIMD: set (w >> 1) & 1, wave (w & 1) + 2 (w >> 2) inside it; ctr0: the arrival counter
// of set 1 (set 0 synchronises through the counters of tile_cholesky_set)
// (a 4-wave workgroup -- the half-size layout, one wave per SIMD -- splits 2 + 2: waves 0, 1 and waves 2, 3)
// The one-wave phases of a 4-wave workgroup (tile factorisations, block substitutions) run on its SERIAL WAVE: wave 0, or wave 2 when the
// workgroup finds its wave 0 in the second wave slot of its SIMD -- i.e. when another workgroup got to this CU first (two half-size
// workgroups share a CU, one wave of each per SIMD: with both serial chains on wave 0 they would share ONE SIMD's issue slots while three
// SIMDs idle).  serial_wave_pick() is called once per kernel by every wave; the choice is kept in L.Qu[15].
__device__ __forceinline__ void serial_wave_pick(Lds &L, bool enable = true) {
    if (SRH_TID == 0) {
        const unsigned slot = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 4);      // HW_REG_HW_ID [3:0]: wave slot inside the SIMD
        L.Qu[15] = (enable && blockDim.x == 256 && (slot & 1u)) ? 2.0 : 0.0;
    }
}
__device__ __forceinline__ int serial_wave(const Lds &L) {
    return blockDim.x == 256 ? __builtin_amdgcn_readfirstlane((int)L.Qu[15]) : 0;
}
__device__ __forceinline__ int half_of_wave(int w) { return (w >> 1) & 1; }
__device__ __forceinline__ Waves<true> half_waves(liptr ctr0, int sw = 0) {
    const int w = __builtin_amdgcn_readfirstlane((int)SRH_TID >> 6) ^ sw, which = half_of_wave(w);
    const bool four = blockDim.x == 256;
    const int lw = four ? (w & 1) : (w & 1) + 2 * (w >> 2), sz = four ? 2 : 4;
    return Waves<true>{lw * 64 + ((int)SRH_TID & 63), sz * 64, lw, sz, ctr0, 0, which == 1};      // (only set 1 calls sync(): one counter)
}

// ------------------------------------------------------------------ rollout x_{k+1} = A_k x_k + B_k u_k + d_k  (u null: zero inputs)
// One dot product of length n + m per state row through the [A | B] panel in LDS (reloaded only when the TPWL region
// changes: ~12 % of the stages), ONE barrier per stage: 8 lanes per row, lane (il, s) of a 16-lane DPP row takes the columns
// 2 s + h + 16 q of row 2 r + il (bank = (row + column) mod 16: conflict free), three DPP additions finish the row.
// The stage vector [x_k ; u_k ; 0] is double buffered in v1 / v2.  (qp::rollout: two L2-fed products and four barriers
// per stage, 7.6 k clocks per stage against ~0.8 k.)
// XS: the trajectory is ALSO written to xs (LDS: the start of the Theta^T area, free during a rollout) for the tests that follow it --
// objective, trust region, and the SCP loop's tests in the GuSTO kernel.  (A flag, not a null test: the area starts at LDS offset 0,
// which is what a null pointer of address space 3 compares equal to.)
template <int MSEL, int NSEL, bool XS = false, int WG = 8>
__device__ __forceinline__ void rollout(const QPDims &d, const QPDyn &dyn, cgptr x0, cgptr u, gptr x, Lds &L, lptr xs = nullptr) {
    const int N = d.N, n = d.n, m = d.m, ld = d.ld, NPa = d.NPa, nk = d.NK;
    const int tid = SRH_TID, nt = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l = lane & 15, il = l >> 3, sl = l & 7;
    const int i_lo = 8 * wave + 2 * (lane >> 4) + il;                 // + 8 rows per wave per row block (n_x > 64, or a 4-wave workgroup: more passes)
    constexpr int rows_pass = 8 * WG;
    constexpr bool ONE_BLOCK = NSEL > 0 && NSEL <= rows_pass;
    const int vlen = (int)(((size_t)ld + 3) & ~(size_t)3);
    lptr va = L.v1, vb = L.v2;
    for (int e = tid; e < nk * ld; e += nt) L.panel[e] = 0.0;
    for (int e = tid; e < vlen; e += nt) {
        const double v = e < n ? x0[e] : (e < n + m && u ? u[e - n] : 0.0);
        va[e] = v; vb[e] = 0.0;
        if (e < n) { x[e] = v; if constexpr (XS) xs[e] = v; }
    }
    __syncthreads();
    QPLds P{};
    P.AB = L.panel; P.idxl = L.idxl; P.psel = -1;
    if (qp::panel_load(d, dyn, P, 0)) __syncthreads();
    const int nq = NPa >> 4;
    for (int k = 0; k < N; ++k) {
        const int sel = __builtin_amdgcn_readfirstlane(L.idxl[k]);
        const double un = (tid < m && u && k + 1 < N) ? u[(size_t)(k + 1) * m + tid] : 0.0;
        for (int ib = 0; ib < (ONE_BLOCK ? 1 : n); ib += rows_pass) {
            const int i = i_lo + ib, ic = i < n ? i : n - 1;
            const double dk = dyn.d[(size_t)sel * n + ic];
            clptr row = L.panel + ic * ld + 2 * sl;
            double acc = 0.0;
            for (int q = 0; q < nq; ++q) {
                acc = fma(row[16 * q], va[2 * sl + 16 * q], acc);
                acc = fma(row[16 * q + 1], va[2 * sl + 16 * q + 1], acc);
            }
            acc = wg::group_sum<8>(acc) + dk;
            if (sl == 0 && i < n) { vb[i] = acc; x[(size_t)(k + 1) * n + i] = acc; if constexpr (XS) xs[(size_t)(k + 1) * n + i] = acc; }
        }
        if (tid < m) vb[n + tid] = un;
        __syncthreads();
        if (k + 1 < N) {
            const int nsel = __builtin_amdgcn_readfirstlane(L.idxl[k + 1]);
            if (dyn.idx == nullptr || nsel != sel) { if (qp::panel_load(d, dyn, P, k + 1)) __syncthreads(); }
        }
        lptr t = va; va = vb; vb = t;
    }
}

// ------------------------------------------------------------------ condensation (once per QP)
// As qpc::condense (adjoint recursion Theta_{j-1} = [C_o ; Theta_j A_j], G[:, j] = Theta_j B_j, one MFMA product per
// stage with the [A_j | B_j] panel in LDS); G goes to the packed store.
template <int MSEL, int NSEL>
__device__ __forceinline__ void condense(const QPDims &d, const QPConst &c, const QPDyn &dyn, cgptr x, gptr gh, Lds &L) {
    const int N = d.N, n = d.n, m = d.m, po = d.po, ld = d.ld, KT = d.KT, ldG = 16 * d.KT, ldT = ldG + 1;
    const int nk = d.NK, NPa = d.NPa, NP = N * po, j0 = d.lean_j0;
    const int tid = SRH_TID, nt = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nt >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    for (int e = tid; e < ldG; e += nt) {
        double v = 0.0;
        if (e < NP) {
            const int k = e / po + 1, a = e - (k - 1) * po;
            for (int j = 0; j < n; ++j) v = fma(c.Co[(size_t)a * n + j], x[(size_t)k * n + j], v);
        }
        L.yf[e] = v;
    }
    for (int e = tid; e < nk * ldT; e += nt) L.B[e] = 0.0;
    for (int e = tid; e < nk * ld; e += nt) L.panel[e] = 0.0;
    // gT_times runs its lanes past the end of a row (times zeros of y): finite values behind the last L2-resident row
    for (int e = tid; e < YPAD; e += nt) gh[goff(j0, m, NP) + e] = 0.0;
    __syncthreads();
    QPLds P{};
    P.AB = L.panel; P.idxl = L.idxl; P.psel = -1;
    const int MT = NPa >> 4;
    const int KS = (n + 3) >> 2;
    const int goff0 = goff(j0, m, NP);
    // Work items of a stage = (column tile ti of Theta^T that already has columns, row tile ci of [A | B]^T): spread over
    // ALL waves (a wave per column tile left most SIMDs idle late in the recursion, when few output stages are "born").
    // Phase A: every wave multiplies its items (operands from LDS, results in registers); barrier; phase B: results into
    // Theta^T / the packed G, the C_o columns of the next output stage, the panel of the next stage if its region differs.
    (void)qp::panel_load(d, dyn, P, N - 1);
    for (int e = tid; e < po * n; e += nt) { const int a = e / n, r = e - a * n; L.B[r * ldT + (N - 1) * po + a] = c.Co[(size_t)a * n + r]; }
    __syncthreads();
    constexpr int KSMAX = NSEL > 0 ? (NSEL + 3) / 4 : 32;
    for (int j = N - 1; j >= 0; --j) {
        const int t_first = (j * po) >> 4;
        const int count = (KT - t_first) * MT;
        const int len = NP - po * j, gj = goff(j, m, NP);
        constexpr int RMAX = CONDENSE_SLOTS;             // item slots per wave: KT * MT <= 8 * 5 items over 8 waves (condense_fits)
        wg::qp_d4 acc[RMAX];
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            acc[r] = {0.0, 0.0, 0.0, 0.0};
            const int it = wave + nw * r;
            if (it < count) {
                const int ti = t_first + it / MT, ci = it - (it / MT) * MT;
                double aop[KSMAX], bop[KSMAX];
#pragma unroll
                for (int s = 0; s < KSMAX; ++s) {
                    aop[s] = s < KS ? L.panel[(4 * s + kk) * ld + 16 * ci + l16] : 0.0;
                    bop[s] = s < KS ? L.B[(4 * s + kk) * ldT + 16 * ti + l16] : 0.0;
                }
#pragma unroll
                for (int s = 0; s < KSMAX; ++s)
                    if (s < KS) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[s], bop[s], acc[r], 0, 0, 0);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const int it = wave + nw * r;
            if (it < count) {
                const int ti = t_first + it / MT, ci = it - (it / MT) * MT;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = 16 * ci + kk + 4 * q, i = 16 * ti + l16;
                    if (i >= po * j && i < NP) {                 // columns of the output stages k > j ("born")
                        if (row < n) {
                            L.B[row * ldT + i] = acc[r][q];
                        } else if (row < n + m) {
                            const int at = gj + (row - n) * len + (i - po * j);
                            if (j < j0) gh[at] = acc[r][q]; else L.Gt[at - goff0] = acc[r][q];
                        }
                    }
                }
            }
        }
        if (j > 0) {
            for (int e = tid; e < po * n; e += nt) { const int a = e / n, r = e - a * n; L.B[r * ldT + (j - 1) * po + a] = c.Co[(size_t)a * n + r]; }
            (void)qp::panel_load(d, dyn, P, j - 1);
        }
        __syncthreads();
    }
}

// The condensation for the half-size layout (QPDims::lean_half): Theta^T has room for about half of its N p_o columns (Lds::ldTc), so the
// adjoint recursion runs twice -- pass A over the column tiles [T, KT) from stage N - 1 down, pass B over the tiles [0, T) from the last stage
// that still reaches them (columns < 16 T are "born" at the stages j <= (16 T - 1) / p_o) -- each with the products of condense() restricted
// to its tiles.  1.5 x the MFMA work of the one-pass form; G goes to the L2 block whole (lean_j0 = N), yf and the pad behind G as well.
template <int MSEL, int NSEL>
__device__ __forceinline__ void condense_half(const QPDims &d, const QPConst &c, const QPDyn &dyn, cgptr x, gptr gh, Lds &L) {
    const int N = d.N, n = d.n, m = d.m, po = d.po, ld = d.ld, KT = d.KT, ldG = 16 * d.KT, ldT = L.ldTc;
    const int nk = d.NK, NPa = d.NPa, NP = N * po;
    const int tid = SRH_TID, nt = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nt >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    for (int e = tid; e < ldG; e += nt) {
        double v = 0.0;
        if (e < NP) {
            const int k = e / po + 1, a = e - (k - 1) * po;
            for (int j = 0; j < n; ++j) v = fma(c.Co[(size_t)a * n + j], x[(size_t)k * n + j], v);
        }
        L.yfg[e] = v;
    }
    for (int e = tid; e < nk * ld; e += nt) L.panel[e] = 0.0;
    // gT_times runs its lanes past the end of a row (times zeros of y): finite values behind the last row
    for (int e = tid; e < YPAD; e += nt) gh[goff(N, m, NP) + e] = 0.0;
    QPLds P{};
    P.AB = L.panel; P.idxl = L.idxl; P.psel = -1;
    const int MT = NPa >> 4;
    const int KS = (n + 3) >> 2;
    const int Tsplit = half_split_tile(KT);
    constexpr int KSMAX = NSEL > 0 ? (NSEL + 3) / 4 : 32;
    for (int pass = 0; pass < 2; ++pass) {
        const int T0 = pass == 0 ? Tsplit : 0, T1 = pass == 0 ? KT : Tsplit;
        if (T1 <= T0) continue;
        const int c0 = 16 * T0, c1 = min(16 * T1, NP);                  // this pass's columns [c0, c1)
        const int jstart = min(N - 1, (c1 - 1) / po);                   // the last stage that reaches them
        __syncthreads();
        for (int e = tid; e < nk * ldT; e += nt) L.B[e] = 0.0;
        __syncthreads();
        (void)qp::panel_load(d, dyn, P, jstart);
        for (int e = tid; e < po * n; e += nt) {
            const int a = e / n, r = e - a * n, i = jstart * po + a;
            if (i >= c0 && i < c1) L.B[r * ldT + (i - c0)] = c.Co[(size_t)a * n + r];
        }
        __syncthreads();
        for (int j = jstart; j >= 0; --j) {
            const int t_first = max(T0, (j * po) >> 4);
            const int count = (T1 - t_first) * MT;
            const int len = NP - po * j, gj = goff(j, m, NP);
            constexpr int RMAX = CONDENSE_SLOTS;             // item slots per wave: (T1 - T0) MT <= 4 * 5 items over 4 waves (scp_host.h)
            wg::qp_d4 acc[RMAX];
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                acc[r] = {0.0, 0.0, 0.0, 0.0};
                const int it = wave + nw * r;
                if (it < count) {
                    const int ti = t_first + it / MT, ci = it - (it / MT) * MT;
                    double aop[KSMAX], bop[KSMAX];
#pragma unroll
                    for (int s = 0; s < KSMAX; ++s) {
                        aop[s] = s < KS ? L.panel[(4 * s + kk) * ld + 16 * ci + l16] : 0.0;
                        bop[s] = s < KS ? L.B[(4 * s + kk) * ldT + 16 * (ti - T0) + l16] : 0.0;
                    }
#pragma unroll
                    for (int s = 0; s < KSMAX; ++s)
                        if (s < KS) acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[s], bop[s], acc[r], 0, 0, 0);
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RMAX; ++r) {
                const int it = wave + nw * r;
                if (it < count) {
                    const int ti = t_first + it / MT, ci = it - (it / MT) * MT;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int row = 16 * ci + kk + 4 * q, i = 16 * ti + l16;
                        if (i >= po * j && i < c1) {                 // columns of the output stages k > j ("born") inside this pass
                            if (row < n) L.B[row * ldT + (i - c0)] = acc[r][q];
                            else if (row < n + m) gh[gj + (row - n) * len + (i - po * j)] = acc[r][q];
                        }
                    }
                }
            }
            if (j > 0) {
                for (int e = tid; e < po * n; e += nt) {
                    const int a = e / n, r = e - a * n, i = (j - 1) * po + a;
                    if (i >= c0 && i < c1) L.B[r * ldT + (i - c0)] = c.Co[(size_t)a * n + r];
                }
                (void)qp::panel_load(d, dyn, P, j - 1);
            }
            __syncthreads();
        }
    }
}

// The condensation of a horizon that lies in ONE region (idx[0] = ... = idx[N-1]: A_j = A, B_j = B).  The block of Theta_j that belongs
// to output stage k is then C_o A^(k-j-1) -- it depends on k - j only -- and G is block-Toeplitz: packed row (j, b) is the first
// NP - 2 j entries of one vector g_b, g_b[2 t + a] = (C_o A^t B)[a, b].  The general recursion recomputes, at every stage and for every
// older output stage, numbers an earlier stage has produced for the newest one.  Here the recursion runs for the two columns of
// output stage N alone: one 16-column tile of Theta^T (the columns sit at the lanes they have in tile KT - 1), one MFMA item per
// wave and stage, the panel loaded once and its operand kept in registers, Theta^T double buffered (one barrier per stage); the
// packed rows are then copies of g.  Every number goes through the k-steps, operands and order the general recursion gives the
// column of output stage N, and an output column of an MFMA product does not depend on its neighbours: the packed G has the same
// bits.  yf, the pad behind G and the stores (L2 head / LDS by lean_j0; the half-size layout: all in L2) as condense() leaves them.
constexpr int TOEP_PITCH = 17;         // row pitch of the one-tile Theta^T
__host__ __device__ inline bool toeplitz_fits(const QPDims &d, int nwaves, int ldTc) {
    return d.po == 2 && d.NPa / 16 <= nwaves && 2 * d.NK * TOEP_PITCH + d.m * d.N * d.po <= d.NK * ldTc;
}
template <int MSEL, int NSEL>
__device__ __forceinline__ void condense_single(const QPDims &d, const QPConst &c, const QPDyn &dyn, cgptr x, gptr gh, Lds &L) {
    const int N = d.N, n = d.n, m = d.m, po = d.po, ld = d.ld, ldG = 16 * d.KT;
    const int nk = d.NK, NPa = d.NPa, NP = N * po, j0 = d.lean_j0;
    const int tid = SRH_TID, nt = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, nw = nt >> 6;
    const int l16 = lane & 15, kk = lane >> 4;
    constexpr int TP = TOEP_PITCH;
    const bool half = d.lean_half != 0;
    for (int e = tid; e < ldG; e += nt) {
        double v = 0.0;
        if (e < NP) {
            const int k = e / po + 1, a = e - (k - 1) * po;
            for (int j = 0; j < n; ++j) v = fma(c.Co[(size_t)a * n + j], x[(size_t)k * n + j], v);
        }
        if (half) L.yfg[e] = v; else L.yf[e] = v;
    }
    lptr gl = L.B + 2 * nk * TP;                       // g_b[0 .. NP) for b < m, behind the two Theta^T buffers
    for (int e = tid; e < 2 * nk * TP; e += nt) L.B[e] = 0.0;
    for (int e = tid; e < nk * ld; e += nt) L.panel[e] = 0.0;
    const int goff0 = goff(j0, m, NP);
    for (int e = tid; e < YPAD; e += nt) gh[goff0 + e] = 0.0;
    __syncthreads();
    QPLds P{};
    P.AB = L.panel; P.idxl = L.idxl; P.psel = -1;
    const int MT = NPa >> 4;
    const int KS = (n + 3) >> 2;
    const int lc0 = (NP - po) & 15;                    // lane of column (N, 0) in its tile
    (void)qp::panel_load(d, dyn, P, N - 1);
    for (int e = tid; e < po * n; e += nt) { const int a = e / n, r = e - a * n; L.B[r * TP + lc0 + a] = c.Co[(size_t)a * n + r]; }
    __syncthreads();
    constexpr int KSMAX = NSEL > 0 ? (NSEL + 3) / 4 : 32;
    const bool item = wave < MT;                       // row tile `wave` of [A | B]^T
    double aop[KSMAX];
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) aop[s] = (item && s < KS) ? L.panel[(4 * s + kk) * ld + 16 * wave + l16] : 0.0;
    const int ca = l16 - lc0;
    const bool born = ca >= 0 && ca < po;
    lptr cur = L.B, nxt = L.B + nk * TP;
    for (int j = N - 1; j >= 0; --j) {
        if (item) {
            wg::qp_d4 acc = {0.0, 0.0, 0.0, 0.0};
            double bop[KSMAX];
#pragma unroll
            for (int s = 0; s < KSMAX; ++s) bop[s] = s < KS ? cur[(4 * s + kk) * TP + l16] : 0.0;
#pragma unroll
            for (int s = 0; s < KSMAX; ++s)
                if (s < KS) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[s], bop[s], acc, 0, 0, 0);
            if (born) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = 16 * wave + kk + 4 * q;
                    if (row < n) nxt[row * TP + l16] = acc[q];
                    else if (row < n + m) gl[(row - n) * NP + po * (N - 1 - j) + ca] = acc[q];
                }
            }
        }
        __syncthreads();
        lptr t = cur; cur = nxt; nxt = t;
    }
    if (half) for (int e = tid; e < m * NP; e += nt) L.gtoep[e] = gl[e];       // (the Gram fills of this G read g instead of the packed rows)
    // expansion: row (j, b) <- g_b[0 .. NP - 2 j), a wave per row
    for (int r = wave; r < N * m; r += nw) {
        const int j = r / m, b = r - j * m, len = NP - po * j, at = goff(j, m, NP) + b * len;
        for (int e = lane; e < len; e += 64) {
            const double v = gl[b * NP + e];
            if (j < j0) gh[at + e] = v; else L.Gt[at - goff0 + e] = v;
        }
    }
    __syncthreads();
}

// Whether this QP's horizon lies in one region (all N entries of the region sequence in L.idxl equal) and the plan allows the
// single-region condensation (QPDims::lean_toeplitz; explicit per-stage matrices -- no region index -- never qualify).  Uniform over
// the workgroup; counts the QP in the plan's counter (QPConst::single_qps).  Called between two barriers of the caller's preamble;
// L.red is free there.
__device__ __forceinline__ bool single_region(const QPDims &d, const QPConst &c, const QPDyn &dyn, Lds &L) {
    if (dyn.idx == nullptr || !d.lean_toeplitz || !toeplitz_fits(d, (int)blockDim.x >> 6, L.ldTc)) return false;
    const int tid = SRH_TID, nt = blockDim.x;
    liptr f = (liptr)L.red;
    int uni = 1;
    const int first = L.idxl[0];
    for (int k = tid; k < d.N; k += nt) uni = uni && (L.idxl[k] == first);
    if (tid == 0) f[0] = 1;
    __syncthreads();
    if (!uni) f[0] = 0;
    __syncthreads();
    const bool single = __builtin_amdgcn_readfirstlane(f[0]) != 0;
    if (single && tid == 0 && c.single_qps) __hip_atomic_fetch_add(c.single_qps, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return single;
}

// ------------------------------------------------------------------ products with G
// Row (j, b) of the packed G^T starts at goff(j) + b (NP - 2 j); with R(j, b) = that start - 2 j, element i sits at R + i and
//     R(j + 1, b) = R(j, b) + m (NP - 2 j) - 2 b - 2
// -- the loops below walk the stages with two integer additions instead of re-deriving the offsets.

// The same product for a kernel instantiation whose horizon NF and first LDS-resident stage J0F are compile-time constants
// (same thread mapping as g_times below: thread = (column, input class), partial sums of the classes through LDS).  The
// stage loop is unrolled completely: element (j, b, i) of the packed store sits at
//     goff(j) - 2 j  +  (b NP + i)  -  2 j b
// -- an immediate, a per-lane base, and a term that only needs one subtraction of the wave-uniform 2 b per stage -- so a stage
// costs an address subtraction, two LDS reads (G and u, the latter at an immediate offset from a per-wave base) and one FMA,
// plus a select in the triangular part; g_times spends about ten instructions per stage on the same (index arithmetic of
// the run-time loop, clamps and masks of its eight-stage trips).  Stages in blocks of sixteen; a block no lane of the wave
// needs is skipped, a block every lane needs whole runs without the selects.  C2: 7.9 k -> 5.5 k clocks, C5: 15.7 k -> 11.6 k.
template <int MSEL, bool HALF, int NF, class GP>
__device__ __forceinline__ void g_times_tasks(const GP &g, Lds &L, clptr uv, lptr yv, int ldG, Waves<HALF> &W);
template <int MSEL, bool HALF, int NF, int J0F, class GP>
__device__ __forceinline__ void g_times_fixed(const GP &g, Lds &L, clptr uv, lptr yv, int ldG, Waves<HALF> &W) {
    if constexpr (J0F == NF) { g_times_tasks<MSEL, HALF, NF>(g, L, uv, yv, ldG, W); return; }      // the half-size layout
    constexpr int M = MSEL, CW = 128, NP = 2 * NF;
    constexpr int BLK = 16;                 // stages per block: 16 + 16 loads in flight (8: 6.2 k clocks at C2, 16: 5.5 k)
    constexpr int goff0 = M * (J0F * NP - J0F * (J0F - 1));
    const int tid = W.tid, nt = W.nt;
    const int GR = nt / CW, col = tid % CW, grp = __builtin_amdgcn_readfirstlane(tid / CW);
    const int cc = col < NP ? col : NP - 1;
    const int jlast = col < NP ? cc >> 1 : -1;                        // last stage that reaches this lane's column
    const int c_lo = col & ~63, c_hi = min(NP - 1, col | 63);
    const int jall = __builtin_amdgcn_readfirstlane((col | 63) < NP ? c_lo >> 1 : -1);      // every lane of the wave: stages 0 .. jall
    const int jany = __builtin_amdgcn_readfirstlane(c_lo < NP ? c_hi >> 1 : -1);            // some lane of the wave: stages 0 .. jany
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = grp; b < M; b += GR) {                               // wave-uniform
        clptr pu = uv + b;
        // stages [JB, JE) from `pg` (pointing at element (0, b, column) of its store minus SHIFT), MASK: triangular part
        auto block = [&](auto pg, auto JB_, auto JE_, auto SHIFT_, auto MASK, auto TOEP) {
            constexpr int JB = decltype(JB_)::value, JE = decltype(JE_)::value, SHIFT = decltype(SHIFT_)::value;
            constexpr bool masked = decltype(MASK)::value, toep = decltype(TOEP)::value;
            double gv[JE - JB], uu[JE - JB];
#pragma unroll
            for (int j = JB; j < JE; ++j) {
                if constexpr (toep) gv[j - JB] = pg[-2 * j];            // g_b[column - 2 j]
                else gv[j - JB] = pg[(M * (j * NP - j * (j - 1)) - 2 * j - SHIFT) - 2 * j * b];
                uu[j - JB] = pu[j * M];
            }
#pragma unroll
            for (int j = JB; j < JE; ++j) {
                if constexpr (masked) acc[j & 3] = fma(j <= jlast ? gv[j - JB] : 0.0, uu[j - JB], acc[j & 3]);
                else acc[j & 3] = fma(gv[j - JB], uu[j - JB], acc[j & 3]);
            }
        };
        auto span = [&](auto pg, auto LO_, auto HI_, auto SHIFT_, auto TOEP) {   // compile-time range [LO, HI) in blocks of BLK
            constexpr int LO = decltype(LO_)::value, HI = decltype(HI_)::value;
            srh_static_for<0, (HI - LO + BLK - 1) / BLK>([&](auto K_) {
                constexpr int JB = LO + decltype(K_)::value * BLK, JE = JB + BLK < HI ? JB + BLK : HI;
                if (JB <= jany) {                                     // uniform
                    if (JE - 1 <= jall) block(pg, std::integral_constant<int, JB>{}, std::integral_constant<int, JE>{}, SHIFT_, std::false_type{}, TOEP);
                    else block(pg, std::integral_constant<int, JB>{}, std::integral_constant<int, JE>{}, SHIFT_, std::true_type{}, TOEP);
                }
            });
        };
        if constexpr (J0F > 0) {
            constexpr std::integral_constant<int, (J0F < NF ? J0F : NF)> HEAD{};
            if (g.gto != nullptr) span(g.gto + (b * NP + cc), std::integral_constant<int, 0>{}, HEAD, std::integral_constant<int, 0>{}, std::true_type{});
            else span(g.gh + (b * NP + cc), std::integral_constant<int, 0>{}, HEAD, std::integral_constant<int, 0>{}, std::false_type{});
        }
        if constexpr (J0F < NF) span(g.gt + (b * NP + cc), std::integral_constant<int, J0F>{}, std::integral_constant<int, NF>{}, std::integral_constant<int, goff0>{}, std::false_type{});
    }
    lptr part = L.part;
    part[grp * CW + col] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    W.sync();
    if (tid < ldG) {
        double s = 0.0;
        if (tid < NP) for (int q = 0; q < GR; ++q) s += part[q * CW + tid];
        yv[tid] = s;
    }
    W.sync();
}

// The same product for the half-size layout (J0F == NF: every packed row in the L2 block), dealt by (column, chain) TASKS -- the schedule
// stated next to the roster functions above (gu_rounds .. gu_index_outside).  With a thread per column, g_times_fixed runs the wave of
// the columns 64 .. 127 (36 live lanes at NP = 100) through all NF stages and every block of it through the selects of the triangle's
// edge: 50 + 32 stage slots per input on the two waves of an input class for 25.5 full ones.  Here a lane owns ONE of the four chains of
// a column: it sees that chain's operands in that chain's order (the inputs in turn, the stages c, c + 4, .. ascending inside each, one
// accumulator kept across the inputs), the quad forms (a0 + a1) + (a2 + a3) -- the additions of g_times_fixed, a pair sum commutes -- and
// `part`, the sum over the input classes and both syncs stay: the same bits.  A wave runs its rounds one after the other; a round and an
// input are one round trip: every load of the round (at most 13) and its reads of u before the first FMA.  Only a round's last two steps
// meet the triangle's edge: there a lane outside reads element (0, b, i) and skips the FMA, every earlier step runs bare.  The Toeplitz
// generators are read at immediate offsets from one address per lane and input (- 8 doubles per step), the packed rows along gu_index_packed.
// One difference to g_times_fixed: a lane outside the triangle executed fma(0.0, u, acc) there and picked up a NaN from a non-finite u
// (which only occurs behind a failed pivot, L.flag[1] == 0, when the product is discarded); here it executes nothing.  Finite data:
// every bit the same.
template <int MSEL, bool HALF, int NF, class GP>
__device__ __forceinline__ void g_times_tasks(const GP &g, Lds &L, clptr uv, lptr yv, int ldG, Waves<HALF> &W) {
    constexpr int M = MSEL, CW = 64 * GU_WAVES, NP = 2 * NF, NR = gu_rounds(NP);
    const int tid = W.tid, nt = W.nt;
    const int GR = nt / CW, grp = __builtin_amdgcn_readfirstlane(tid / CW), wv = __builtin_amdgcn_readfirstlane((tid % CW) >> 6);
    const int lane = tid & 63, c = lane & 3;
    const bool toep = g.gto != nullptr;                               // (uniform)
    lptr part = L.part + grp * CW;
    clptr pu0 = uv + c * M;
    srh_static_for<0, NR>([&](auto R_) {
        constexpr int r = NR - 1 - decltype(R_)::value;               // a wave's longest round first
        constexpr int S = gu_round_steps(NP, r), SE = gu_first_edge_step(NP, r);
        if (wv != gu_round_wave(NP, r)) return;                       // uniform
        const int i = gu_lane_col(NP, r, lane), jlast = i >> 1;
        // byte offsets from the store's (uniform) base in one 32-bit register per lane: a step of the walk of gu_index_packed is the
        // step's constant plus the lane's - 8 (8 M c + 8 b), a step along the generators - 64
        const unsigned at_p = 8u * (unsigned)gu_index_packed(M, NP, c, 0, 0, i), at_t = 8u * (unsigned)gu_index_toeplitz(NP, c, 0, 0, i);
        double acc = 0.0;
        auto input = [&](cgptr src, int b, auto TOEP) {
            constexpr bool tp = decltype(TOEP)::value;
            clptr pu = pu0 + b;
            const unsigned e0 = 8u * (unsigned)gu_index_outside(NP, b, i);
            unsigned e = tp ? at_t + 8u * (unsigned)(b * NP) : at_p + 8u * (unsigned)(b * (NP - 2 * c));
            const unsigned ndq = 0u - 8u * (unsigned)(8 * M * c + 8 * b);
            double gv[S], uu[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (s > 0) e = tp ? e - 64u : e + ndq + 8u * (unsigned)(gu_walk_e(M, NP, s) - gu_walk_e(M, NP, s - 1));
                const unsigned es = (s >= SE && c + 4 * s > jlast) ? e0 : e;
                gv[s] = *(cgptr)((const __attribute__((address_space(1))) char *)src + es);
                uu[s] = pu[4 * M * s];
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double t = fma(gv[s], uu[s], acc);
                if (s >= SE) acc = c + 4 * s <= jlast ? t : acc;
                else acc = t;
            }
        };
        for (int b0 = grp; b0 < M; b0 += GR) {                        // uniform
            // (b opaque in every trip: left to itself the compiler turns each step's offset into an induction variable of this loop,
            // 2 S registers and a multiplication per step in front of every round)
            int b = b0;
            asm volatile("" : "+s"(b));
            if (toep) input(g.gto, b, std::true_type{});
            else input(g.gh, b, std::false_type{});
        }
        acc = wg::group_sum<4>(acc);                                  // lane 0 of the quad: (a0 + a1) + (a2 + a3)
        if (gu_lane_stores(NP, r, lane)) part[i] = acc;
    });
    W.sync();
    if (tid < ldG) {
        double s = 0.0;
        if (tid < NP) for (int q = 0; q < GR; ++q) s += L.part[q * CW + tid];
        yv[tid] = s;
    }
    W.sync();
}

// yv[i] = sum_{rows (j,b), 2 j <= i} G^T[(j,b)][i] uv[(j,b)]: thread = (column, input class b mod 4).  Stages j <= jlo (the
// last stage that reaches EVERY column of the wave) need no mask; lanes read past "their" rows only inside LDS / the L2
// block (the select discards what they get).  8 loads of G and of u per trip before the FMAs.
template <int MSEL, bool HALF, class GP>
__device__ __forceinline__ void g_times(const QPDims &d, const GP &g, Lds &L, clptr uv, lptr yv, Waves<HALF> &W) {
    if constexpr (GP::NF > 0) { g_times_fixed<MSEL, HALF, GP::NF, GP::J0F>(g, L, uv, yv, 16 * d.KT, W); return; }
    constexpr int M = MSEL, CH = 8, CW = 128;
    const int ldG = 16 * d.KT, NP = g.NP, N = d.N, tid = W.tid, nt = W.nt;
    const int GR = nt / CW, col = tid % CW, grp = tid / CW;          // GR = 4
    const int cc = col < NP ? col : NP - 1;
    const int jcnt = col < NP ? min(N, cc / 2 + 1) : 0;              // stages that reach this column
    // wave-uniform: stages that reach every column of the wave / any column of the wave
    const int c_lo = col & ~63, c_hi = min(NP - 1, col | 63);
    const int jall = __builtin_amdgcn_readfirstlane((col | 63) < NP ? min(N, c_lo / 2 + 1) : 0);
    const int jany = __builtin_amdgcn_readfirstlane(c_lo < NP ? min(N, c_hi / 2 + 1) : 0);
    const int goff0 = goff(g.j0, M, NP);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};            // four independent chains (a dependent f64 FMA issues every ~13 clocks)
    for (int b = grp; b < M; b += GR) {
        // stages [jb, je) of input b; MASK: lanes past their last stage contribute zero
        auto pass = [&](auto src, int jb, int je, auto MASK) {
            constexpr bool masked = decltype(MASK)::value;
            int R = goff(jb, M, NP) + b * (NP - 2 * jb) - 2 * jb + cc, dl = M * (NP - 2 * jb) - 2 * b - 2;
            for (int j0 = jb; j0 < je; j0 += CH) {
                double gv[CH], uu[CH];
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    gv[t] = src[R];
                    uu[t] = uv[min(j0 + t, N - 1) * M + b];
                    R += dl; dl -= 2 * M;
                }
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    const int j = j0 + t;
                    bool ok = j < je;                                 // uniform: the tail of the last trip
                    if constexpr (masked) ok = ok && j < jcnt;
                    acc[t & 3] = fma(ok ? gv[t] : 0.0, uu[t], acc[t & 3]);     // (what masked lanes read may be anything)
                }
            }
        };
        auto span = [&](auto src, int lo, int hi) {                   // stages [lo, hi) of one store
            const int mid = max(lo, min(hi, jall));
            if (mid > lo) pass(src, lo, mid, std::false_type{});
            if (hi > mid) pass(src, mid, hi, std::true_type{});
        };
        span(g.gh, 0, min(g.j0, jany));
        span(g.gt - goff0, g.j0, jany);
    }
    lptr part = L.part;                                     // GR * CW slots: 512 for the workgroup, 256 for a half set
    part[grp * CW + col] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    W.sync();
    if (tid < ldG) {
        double s = 0.0;
        if (tid < NP) for (int q = 0; q < GR; ++q) s += part[q * CW + tid];
        yv[tid] = s;
    }
    W.sync();
}
template <int MSEL, class GP>
__device__ __forceinline__ void g_times(const QPDims &d, const GP &g, Lds &L, clptr uv, lptr yv) {
    auto W = all_waves();
    g_times<MSEL, false>(d, g, L, uv, yv, W);
}

// out1[row] = sum_{i >= 2 j} G^T[row][i] y1[i]  (and out2 with y2 when y2 != null): 8 lanes per row, 64 rows per pass; the
// L2-resident rows (stages < j0) in passes of their own.  No masks: y1 / y2 must be zero from index NP up to NP + YPAD - 1
// (the lanes run to the length of the longest row of the pass; what they read of G past the end of a row is the next
// rows' data -- finite -- times those zeros).
// GRP > 0: the trip count of a row is the one of a pass of GRP rows, whatever the wave set's own pass -- the trip count decides which
// of the two chains a term lands in, so a product on all waves with GRP = the rows per pass of the Newton front's set has the front's
// bits entry by entry (converged_early).  GRP divides the set's rows per pass and is a multiple of 8 (uniform over a wave).
template <int MSEL, bool HALF, int GRP = 0, class GP>
__device__ __forceinline__ void gT_times(const QPDims &d, const GP &g, Lds &L, clptr y1, clptr y2, lptr out1, lptr out2, Waves<HALF> &W) {
    constexpr int M = MSEL;
    const int NP = g.NP, nm = d.N * M, tid = W.tid, nt = W.nt;
    const int g8 = tid & 7, rpp = nt / 8;
    const int goff0 = goff(g.j0, M, NP);
    auto rows = [&](auto src, int rb, int re, auto TWO, bool toep = false) {   // rows [rb, re) from `src` (indexed by the global offset; toep: by b NP + i - 2 j)
        constexpr bool two = decltype(TWO)::value;
        for (int r0 = rb; r0 < re; r0 += rpp) {
            const int r = r0 + (tid >> 3), rc = r < re ? r : re - 1;
            const int j = rc / M, b = rc - j * M, len = NP - 2 * j;
            const int at = (toep ? b * NP : goff(j, M, NP) + b * len) + g8;
            clptr p1 = y1 + 2 * j + g8, p2 = (two ? y2 : y1) + 2 * j + g8;
            int nq = (NP - 2 * (r0 / M) + 7) >> 3;                   // trips of the longest row of this pass (uniform)
            if constexpr (GRP > 0) nq = (NP - 2 * ((rb + (r - rb) / GRP * GRP) / M) + 7) >> 3;      // ... of the pass of GRP rows
            double a1 = 0.0, a2 = 0.0, c1 = 0.0, c2 = 0.0;         // two chains per output
            int q = 0;
            for (; q + 4 <= nq; q += 4) {
                double gv[4], ya[4], yb[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) { gv[t] = src[at + 8 * (q + t)]; ya[t] = p1[8 * (q + t)]; if (two) yb[t] = p2[8 * (q + t)]; }
                a1 = fma(gv[0], ya[0], a1); c1 = fma(gv[1], ya[1], c1); a1 = fma(gv[2], ya[2], a1); c1 = fma(gv[3], ya[3], c1);
                if (two) { a2 = fma(gv[0], yb[0], a2); c2 = fma(gv[1], yb[1], c2); a2 = fma(gv[2], yb[2], a2); c2 = fma(gv[3], yb[3], c2); }
            }
            for (; q < nq; ++q) {
                const double gq = src[at + 8 * q];
                a1 = fma(gq, p1[8 * q], a1);
                if (two) a2 = fma(gq, p2[8 * q], a2);
            }
            a1 += c1; a2 += c2;
            a1 = wg::group_sum<8>(a1);
            if (two) a2 = wg::group_sum<8>(a2);
            if (g8 == 0 && r < re) { out1[r] = a1; if (two) out2[r] = a2; }
        }
    };
    // Rows [0, re) of a single-region G from its Toeplitz generators, half-size layout (the only one that keeps generators: g.gto is
    // set by ipm_box4 alone; J0F == NF > 0, every row L2-resident): entry q of row (j, b) at lane g8 is
    // g_b[g8 + 8 q] whatever j, and b = (tid >> 3) % M in every pass (M divides the 8 rows of a wave, so every set's rows per pass), so a
    // thread's entries -- at most QMAX = ceil(NP / 8) -- are loaded ONCE per product into a register array that is indexed at compile time
    // only, and the passes run from registers and LDS alone: no address arithmetic and no vector-memory load per trip (DESIGN section 45:
    // the products are bound by the instructions they issue).  A lane past the last row keeps its own b: its sums are never stored.  The
    // FMAs are those of `rows`, term by term: blocks of four alternate the two chains while q + 4 <= nq, the remainder trips feed the
    // first chain; nq is wave-uniform, every guard on it is a scalar branch.
    auto rows_toeplitz = [&](int re, auto TWO) {
        constexpr bool two = decltype(TWO)::value;
        // NPF = g.NP: a fixed-horizon instantiation only runs problems with d.N == GP::NF (lean.hip: lean_matches), as g_times_fixed assumes
        constexpr int NPF = 2 * (GP::NF > 0 ? GP::NF : 1), QMAX = (NPF + 7) / 8, KB = (QMAX + 3) / 4;
        double gv[QMAX];
        auto trips = [&](int r0, int r) {                          // of the longest row of the pass (of the pass of GRP rows)
            int nq = (NPF - 2 * (r0 / M) + 7) >> 3;
            if constexpr (GRP > 0) nq = (NPF - 2 * (r / GRP * GRP / M) + 7) >> 3;
            return __builtin_amdgcn_readfirstlane(nq);
        };
        {   // the first pass has the wave's longest rows: entries 0 .. nq - 1, rounded up to whole blocks of four (what the last block
            // holds behind them repeats entry nq - 1: nothing is read that `rows` does not read)
            const int at = ((tid >> 3) % M) * NPF + g8, nq = trips(0, tid >> 3);
            srh_static_for<0, KB>([&](auto K_) {
                constexpr int q0 = 4 * decltype(K_)::value;
                if (q0 < nq) srh_static_for<q0, (q0 + 4 < QMAX ? q0 + 4 : QMAX)>([&](auto Q_) {
                    constexpr int q = decltype(Q_)::value;
                    gv[q] = g.gto[at + 8 * min(q, nq - 1)];
                });
            });
        }
        for (int r0 = 0; r0 < re; r0 += rpp) {
            const int r = r0 + (tid >> 3), rc = r < re ? r : re - 1;
            const int j = rc / M, nq = trips(r0, r);
            clptr p1 = y1 + 2 * j + g8, p2 = (two ? y2 : y1) + 2 * j + g8;
            double a1 = 0.0, a2 = 0.0, c1 = 0.0, c2 = 0.0;
            srh_static_for<0, KB>([&](auto K_) {
                constexpr int q0 = 4 * decltype(K_)::value;
                if (q0 + 4 <= nq) {
                    if constexpr (q0 + 4 <= QMAX) {
                        double ya[4], yb[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) { ya[t] = p1[8 * (q0 + t)]; if (two) yb[t] = p2[8 * (q0 + t)]; }
                        a1 = fma(gv[q0], ya[0], a1); c1 = fma(gv[q0 + 1], ya[1], c1); a1 = fma(gv[q0 + 2], ya[2], a1); c1 = fma(gv[q0 + 3], ya[3], c1);
                        if (two) { a2 = fma(gv[q0], yb[0], a2); c2 = fma(gv[q0 + 1], yb[1], c2); a2 = fma(gv[q0 + 2], yb[2], a2); c2 = fma(gv[q0 + 3], yb[3], c2); }
                    }
                } else {
                    srh_static_for<q0, (q0 + 3 < QMAX ? q0 + 3 : QMAX)>([&](auto Q_) {
                        constexpr int q = decltype(Q_)::value;
                        if (q < nq) {
                            a1 = fma(gv[q], p1[8 * q], a1);
                            if (two) a2 = fma(gv[q], p2[8 * q], a2);
                        }
                    });
                }
            });
            a1 += c1; a2 += c2;
            a1 = wg::group_sum<8>(a1);
            if (two) a2 = wg::group_sum<8>(a2);
            if (g8 == 0 && r < re) { out1[r] = a1; if (two) out2[r] = a2; }
        }
        // every entry named as read (an empty statement; the loads have long landed): the compiler guards a register that a later
        // request overwrites with a wait for loads into it that it cannot see retired -- the entries no row of this wave used
        srh_static_for<0, QMAX>([&](auto Q_) { const double e = gv[decltype(Q_)::value]; asm volatile("" :: "v"(e)); });
    };
    const int rh = min(nm, g.j0 * M);
    const bool toep = g.gto != nullptr;                             // (uniform) the L2-resident rows read from their generators
    cgptr head = toep ? g.gto : g.gh;
    auto product = [&](auto TWO) {
        if (rh > 0) {
            if constexpr (GP::NF > 0 && GP::J0F == GP::NF) {         // the half-size layout
                static_assert(8 % M == 0, "rows_toeplitz: M must divide the 8 rows of a wave (b = (tid >> 3) % M in every pass)");
                if (toep) rows_toeplitz(rh, TWO);
                else rows(head, 0, rh, TWO, false);
            } else rows(head, 0, rh, TWO, toep);
        }
        if (nm > rh) rows(g.gt - goff0, rh, nm, TWO);
    };
    if (y2) product(std::true_type{});
    else product(std::false_type{});
    W.sync();
}
template <int MSEL, class GP>
__device__ __forceinline__ void gT_times(const QPDims &d, const GP &g, Lds &L, clptr y1, clptr y2, lptr out1, lptr out2) {
    auto W = all_waves();
    gT_times<MSEL, false>(d, g, L, y1, y2, out1, out2, W);
}

// ------------------------------------------------------------------ Gram matrix K = I + Ls^T (G D^-1 G^T) Ls -> upper tiles
// One task = up to 4 tiles (I, J0 .. J0 + nJ - 1) of one tile row: the A operand (columns 16 I .. of the packed rows) is
// shared by the tiles of the task; k-steps = 4 packed rows = the inputs 4 sub .. 4 sub + 3 of one stage, and a tile row only
// runs over the stages that reach it: 2 j < 16 (I + 1).  Stages with 2 j <= 16 I reach every lane of the tile row (no
// masks); the last seven are triangular.  sched: per wave 4 tasks x {I, J0, nJ, 0} (host-built, longest first onto the
// least loaded SIMD; nJ = 0: no more tasks).
// STAGE (the half-size layout, where every packed row has its home in the L2 block): the K-tile area L.B is dead when a Gram fill
// starts -- the factor of the iteration before has been used, every tile is rewritten here -- so the rows of the stages >= g.j0 are
// copied into it once (g.gt == L.B, from gsrc) and the tiles read them from LDS instead of once per tile row and column they meet
// from L2.  The tiles walk the stages in the same ascending order: same bits.  An epilogue must not write a tile into L.B while
// another wave still reads staged rows there: the accumulators of ALL tiles of a wave stay in registers (GRAM_SLOTS tasks of at most
// 4, 3, 1 tiles: 8 accumulators) THROUGH the epilogues, which touch registers, L.Ls and L.ks only; one barrier ("every wave has read its
// last staged row" and "L.ks is complete" at once), then each tile is stored once, already scaled -- no raw tile in L.B, no scaling pass
// over the 28 tiles, one barrier less per fill.  Register arrays want compile-time indices, so the tasks are not
// pulled here: c.gram_sched is the static table [wave][slot] of scp_host.h:lean_gram_slots.
// STAGE with gtoep != null (wave-uniform; the packed G is the expansion of the Toeplitz generators g_b, ql::condense_single): operand
// element (j, b, i) of the packed rows is g_b[i - 2 j].  The four vectors are staged instead of the rows -- each behind TOEP_FRONT zeros,
// for the lanes of a triangular stage that sit before its first column (masked as in the packed form; the index must only be
// addressable) and in front of zeros up to the pitch (the padding columns i >= NP of the last tile) -- and EVERY stage reads LDS: no
// L2 head, ~3 loads per thread instead of 59.  Same stages in the same order into the same accumulators: same bits.
constexpr int GRAM_SLOTS = 3;          // per wave of a staged Gram fill: {I, J0, nJ, 0} with nJ <= 4, 3, 1 (nJ = 0: slot not used)
constexpr int TOEP_FRONT = 16;
__host__ __device__ inline int toep_pitch(int KT) { return TOEP_FRONT + 16 * KT + 16; }
template <int MSEL, bool STAGE, class GP>
__device__ __forceinline__ void gram_t(const QPDims &d, const QPConst &c, const GP &g, Lds &L, cgptr gsrc = nullptr, cgptr gtoep = nullptr) {
    static_assert(MSEL == 4 || MSEL == 8, "lean Gram: n_u = 4 or 8");
    constexpr int M = MSEL, SPS = M / 4;                       // k-steps per stage
    const int N = d.N, KT = d.KT, NP = g.NP;
    const int tid = SRH_TID, nt = blockDim.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l16 = lane & 15, kk = lane >> 4;
    const int goff0 = goff(g.j0, M, NP);
    lptr w2 = L.tc;                                            // 1 / D per packed row
    lapc::Laps<6> gl;          // 1/D pass + barrier, descriptors, products, epilogue, barrier, scaling + barrier (STAGE: scaled store + barrier)
    // The tile tasks are PULLED: the list (longest first, scp_host.h) goes into LDS beside a counter, a wave that has finished a task
    // takes the next one -- the static assignment of round 5a left the busiest wave 40 % behind the first one to finish whatever
    // cost model placed the tasks (the waves of a SIMD share its MFMA pipe, the L2 head of G is slower than its LDS tail, ...).
    // The list lives in the reduction scratch of the products (L.part: free during the Gram fill).  Which wave computes a tile
    // does not change its bits.
    liptr tl = (liptr)L.part;                                  // [0] next task, [4 + 4 t ..] = {I, J0, nJ, 0} of task t
    if (tid < GRAM_TASKS * 4) tl[4 + tid] = c.gram_sched[tid];
    if (tid == 0) tl[0] = 0;
    for (int e = tid; e < N * M; e += nt) { const double s = L.Ldi[e]; w2[e] = s * s; }
    const int TGP = toep_pitch(KT);
    if constexpr (STAGE) {                                     // (packed offsets of a stage are multiples of 4: 16-byte pieces)
        if (gtoep != nullptr) {
            for (int e = tid; e < M * TGP; e += nt) {
                const int b = e / TGP, col = e - b * TGP - TOEP_FRONT;
                L.B[e] = (col >= 0 && col < NP) ? gtoep[b * NP + col] : 0.0;
            }
        } else {
            const int nq = (goff(N, M, NP) - goff0) >> 1;
            const double2 *s2 = (const double2 *)(gsrc + goff0);
            double2 *d2 = (double2 *)(lptr)g.gt;
#pragma unroll 4
            for (int e = tid; e < nq; e += nt) d2[e] = s2[e];
        }
    }
    __syncthreads();
    gl.lap(0);
    constexpr int NACC = STAGE ? 8 : 4;
    wg::qp_d4 acc[NACC];
    // ---- the products of one task: tiles (I, J0 .. J0 + nJ - 1) into acc[BASE ..], nJ <= CAP
    auto products = [&](int I, int J0, int nJ, auto BASE, auto CAP, auto TOEP) {
        constexpr int base = decltype(BASE)::value, cap = decltype(CAP)::value;
        constexpr bool toep = decltype(TOEP)::value;          // operands from the staged Toeplitz generators
        const int jend = min(N, 8 * (I + 1));                  // stages with 2 j < 16 (I + 1)
        const int jfull = min(jend, 8 * I + 1);                // stages with 2 j <= 16 I: every lane of the row is live
        const int ia = 16 * I + l16;
        const bool diag0 = J0 == I;                            // tile 0 of the task is the diagonal tile
        const int dJ = 16 * (J0 - I);                          // B operand of tile t: 16 (dJ / 16 + t) doubles behind A's
        // stages [jb, je) from `src` (indexed by the global packed offset); MASK: triangular part of the tile row; NJ tiles.
        // No masks for the padding columns i >= NP of the last tile row / column: what they read (finite or not) only
        // reaches the padding rows / columns of K, which are overwritten below.  1 / D goes onto the shared A operand.
        auto run = [&](auto src, int jb, int je, auto MASK, auto NJ) {
            constexpr bool masked = decltype(MASK)::value;
            constexpr int nj = decltype(NJ)::value;
            int R = goff(jb, M, NP) + kk * (NP - 2 * jb) - 2 * jb + ia;           // R(jb, b = kk) + column of the A operand
            int dl = M * (NP - 2 * jb) - 2 * kk - 2;
            if constexpr (toep) { R = kk * TGP + TOEP_FRONT + ia - 2 * jb; dl = -2; }      // g_b[i - 2 j], b = kk
#ifndef SRH_GRAM_KS
#define SRH_GRAM_KS 4
#endif
            constexpr int UN = SRH_GRAM_KS / SPS;                            // stages per full trip: SRH_GRAM_KS k-steps
            auto trip = [&](int j0, auto UNS) {                              // UNS stages = UNS * SPS k-steps
                constexpr int uns = decltype(UNS)::value, KS = uns * SPS;
                double av[KS], bv[KS][nj];
#pragma unroll
                for (int us = 0; us < uns; ++us) {
                    const int j = j0 + us;
#pragma unroll
                    for (int sub = 0; sub < SPS; ++sub) {
                        const int u = us * SPS + sub;
                        const int base = R + 4 * sub * (toep ? TGP : NP - 2 * j);
                        av[u] = src[base] * w2[j * M + 4 * sub + kk];
#pragma unroll
                        for (int t = 0; t < nj; ++t) bv[u][t] = src[base + dJ + 16 * t];
                        if constexpr (masked) {
                            const bool va = ia >= 2 * j;
                            av[u] = va ? av[u] : 0.0;
                            if (diag0) bv[u][0] = va ? bv[u][0] : 0.0;
                        }
                    }
                    R += dl;
                    if constexpr (!toep) dl -= 2 * M;
                }
#pragma unroll
                for (int u = 0; u < KS; ++u)
#pragma unroll
                    for (int t = 0; t < nj; ++t)
                        acc[base + t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u][t], acc[base + t], 0, 0, 0);
            };
            int j0 = jb;
            for (; j0 + UN <= je; j0 += UN) trip(j0, std::integral_constant<int, UN>{});
            for (; j0 < je; ++j0) trip(j0, std::integral_constant<int, 1>{});
        };
        // four ranges: {L2 head, LDS} x {full, triangular}
        auto task_body = [&](auto NJ) {
            if constexpr (toep) {                                  // two ranges: full, triangular
                if (jfull > 0) run((clptr)L.B, 0, jfull, std::false_type{}, NJ);
                if (jend > jfull) run((clptr)L.B, jfull, jend, std::true_type{}, NJ);
                return;
            }
            const int hf = min(jfull, g.j0), he = min(jend, g.j0);
            if (hf > 0) run(g.gh, 0, hf, std::false_type{}, NJ);
            if (he > hf) run(g.gh, hf, he, std::true_type{}, NJ);
            if (jfull > g.j0) run(g.gt - goff0, g.j0, jfull, std::false_type{}, NJ);
            if (jend > max(jfull, g.j0)) run(g.gt - goff0, max(jfull, g.j0), jend, std::true_type{}, NJ);
        };
        if constexpr (cap >= 4) { if (nJ == 4) { task_body(std::integral_constant<int, 4>{}); return; } }
        if constexpr (cap >= 3) { if (nJ == 3) { task_body(std::integral_constant<int, 3>{}); return; } }
        if constexpr (cap >= 2) { if (nJ == 2) { task_body(std::integral_constant<int, 2>{}); return; } }
        task_body(std::integral_constant<int, 1>{});
    };
    // ---- Ls on both sides, + I, raw tile to the store; the diagonal feeds the Jacobi scaling
    // (the factors of the rows are the same for every tile of the task; the row r ^ 1 of an output stage sits in the neighbouring
    // row of 16 lanes: wg::xor16, two v_permlane16_swap instead of a ds_bpermute round trip; the scale factors of the Jacobi
    // scaling only where the tile is a diagonal one -- round 5: 13 k of the 40 k clocks of a Gram fill were this epilogue)
    // STORE false (the staged fill): the finished raw tile stays in its accumulator -- registers, L.Ls and L.ks only, nothing goes to L.B
    auto epilogue = [&](int I, int J0, int nJ, auto BASE, auto CAP, auto STORE) {
        constexpr int base = decltype(BASE)::value, cap = decltype(CAP)::value;
        constexpr bool store = decltype(STORE)::value;
        double la0[4], la2[4], la3[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gi = 16 * I + kk + 4 * q, ka = min(gi >> 1, N - 1);
            clptr La = L.Ls + (size_t)ka * 4;
            la0[q] = La[0]; la2[q] = La[2]; la3[q] = La[3];
        }
        const bool ar0 = (kk & 1) == 0;                                  // row of the output stage: 16 I + 4 q are even
#pragma unroll
        for (int t = 0; t < cap; ++t) {
            if (t >= nJ) continue;
            const int J = J0 + t;
            const int gjc = 16 * J + l16, kb = min(gjc >> 1, N - 1), bc = gjc & 1;
            clptr Lb = L.Ls + (size_t)kb * 4;
            const double cb_own = bc == 0 ? Lb[0] : Lb[3], cb_oth = bc == 0 ? Lb[2] : 0.0;
            lptr T = L.B + (size_t)qpc::tile_index(I, J, KT) * TSZ;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = kk + 4 * q, gi = 16 * I + r;
                double v = (gi < NP && gjc < NP) ? acc[base + t][q] : 0.0;  // padding rows / columns: exactly the identity
                const double vp = wg::dpp_mov<0xB1>(v);                 // the other column of the output stage
                v = fma(vp, cb_oth, v * cb_own);                        // (Ky Ls)
                const double vr = wg::xor16(v);                         // the other row of the output stage (kk ^ 1)
                v = ar0 ? fma(la2[q], vr, la0[q] * v) : la3[q] * v;     // Ls^T (Ky Ls)
                if (I == J) {                                           // (the whole wave)
                    const bool dg = r == l16;
                    v += dg ? 1.0 : 0.0;
                    const double ri = qpc::rsq3(dg ? v : 1.0);
                    if (dg) L.ks[gi] = ri;
                }
                if constexpr (store) T[r * TS + l16] = v;
                else acc[base + t][q] = v;
            }
        }
    };
    // ---- the staged fill's store: the tiles a wave kept in registers go to L.B once, already scaled to a unit diagonal -- the two
    // multiplications of the scaling pass below in its association (T *= ks_I[r] * sc), behind the barrier that publishes L.ks
    auto store_scaled = [&](int I, int J0, int nJ, auto BASE, auto CAP) {
        constexpr int base = decltype(BASE)::value, cap = decltype(CAP)::value;
        double ki[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ki[q] = L.ks[16 * I + kk + 4 * q];
#pragma unroll
        for (int t = 0; t < cap; ++t) {
            if (t >= nJ) continue;
            const int J = J0 + t;
            lptr T = L.B + (size_t)qpc::tile_index(I, J, KT) * TSZ;
            const double sc = L.ks[16 * J + l16];
#pragma unroll
            for (int q = 0; q < 4; ++q) T[(kk + 4 * q) * TS + l16] = acc[base + t][q] * (ki[q] * sc);
        }
    };
    constexpr std::integral_constant<int, 0> B0{};
    constexpr std::integral_constant<int, 4> C4{};
    if constexpr (!STAGE) {
        while (true) {
            int tnext = 0;
            if (lane == 0) tnext = __hip_atomic_fetch_add(tl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            tnext = __builtin_amdgcn_readfirstlane(tnext);
            if (tnext >= GRAM_TASKS) break;
            const int I = __builtin_amdgcn_readfirstlane(tl[4 + 4 * tnext]), J0 = __builtin_amdgcn_readfirstlane(tl[5 + 4 * tnext]),
                      nJ = __builtin_amdgcn_readfirstlane(tl[6 + 4 * tnext]);
            gl.lap(1);
            if (nJ == 0) break;
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = {0.0, 0.0, 0.0, 0.0};
            products(I, J0, nJ, B0, C4, std::false_type{});
            gl.lap(2);
            epilogue(I, J0, nJ, B0, C4, std::true_type{});
            gl.lap(3);
        }
        __syncthreads();
        gl.lap(4);
        // ---- symmetric scaling to a unit diagonal (see qpc::gram for why it matters): the upper tiles over the waves
        for (int t = wave, I = 0, rowlen = KT; t < KT * (KT + 1) / 2; t += nt >> 6) {
            int tt = t;
            I = 0; rowlen = KT;
            while (tt >= rowlen) { tt -= rowlen; ++I; --rowlen; }
            const int J = I + tt;
            lptr T = L.B + (size_t)qpc::tile_index(I, J, KT) * TSZ;
            const double sc = L.ks[16 * J + l16];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int r = kk + 4 * q; T[r * TS + l16] *= L.ks[16 * I + r] * sc; }
        }
    } else {
        constexpr std::integral_constant<int, 4> B1{};
        constexpr std::integral_constant<int, 7> B2{};
        constexpr std::integral_constant<int, 3> C3{};
        constexpr std::integral_constant<int, 1> C1{};
        int sI[GRAM_SLOTS], sJ[GRAM_SLOTS], sn[GRAM_SLOTS];
#pragma unroll
        for (int s = 0; s < GRAM_SLOTS; ++s) {
            const int e = 4 + 4 * (GRAM_SLOTS * wave + s);
            sI[s] = __builtin_amdgcn_readfirstlane(tl[e]); sJ[s] = __builtin_amdgcn_readfirstlane(tl[e + 1]); sn[s] = __builtin_amdgcn_readfirstlane(tl[e + 2]);
        }
        gl.lap(1);
#pragma unroll
        for (int t = 0; t < NACC; ++t) acc[t] = {0.0, 0.0, 0.0, 0.0};
        if (gtoep != nullptr) {
            if (sn[0] > 0) products(sI[0], sJ[0], sn[0], B0, C4, std::true_type{});
            if (sn[1] > 0) products(sI[1], sJ[1], sn[1], B1, C3, std::true_type{});
            if (sn[2] > 0) products(sI[2], sJ[2], sn[2], B2, C1, std::true_type{});
        } else {
            if (sn[0] > 0) products(sI[0], sJ[0], sn[0], B0, C4, std::false_type{});
            if (sn[1] > 0) products(sI[1], sJ[1], sn[1], B1, C3, std::false_type{});
            if (sn[2] > 0) products(sI[2], sJ[2], sn[2], B2, C1, std::false_type{});
        }
        gl.lap(2);
        if (sn[0] > 0) epilogue(sI[0], sJ[0], sn[0], B0, C4, std::false_type{});
        if (sn[1] > 0) epilogue(sI[1], sJ[1], sn[1], B1, C3, std::false_type{});
        if (sn[2] > 0) epilogue(sI[2], sJ[2], sn[2], B2, C1, std::false_type{});
        gl.lap(3);
        __syncthreads();                                       // every wave has read its last staged row and published its part of L.ks: L.B takes the tiles
        gl.lap(4);
        if (sn[0] > 0) store_scaled(sI[0], sJ[0], sn[0], B0, C4);
        if (sn[1] > 0) store_scaled(sI[1], sJ[1], sn[1], B1, C3);
        if (sn[2] > 0) store_scaled(sI[2], sJ[2], sn[2], B2, C1);
    }
    __syncthreads();
    gl.lap(5);
    if constexpr (lapc::ON) {                                  // wave 0's laps to the mailbox, every wave's products and epilogue to the per-wave sums
        if (tid == 0) {
            for (int i = 0; i < 4; ++i) L.Qu[lapc::MAIL_GRAM + i] += (double)gl[i];
            L.Qu[lapc::MAIL_GRAM_BARRIER] += (double)gl[4]; L.Qu[lapc::MAIL_GRAM_STORE] += (double)gl[5];
        }
        if (lane == 0 && blockIdx.x == 0) { lapc::WaveLaps::add(wave, gl[2]); lapc::WaveLaps::add(8 + wave, gl[3]); }
    }
}
template <int MSEL, class GP>
__device__ __forceinline__ void gram(const QPDims &d, const QPConst &c, const GP &g, Lds &L) { gram_t<MSEL, false>(d, c, g, L); }

// ------------------------------------------------------------------ tile Cholesky on one wave set, without set-wide barriers
// qpc::tile_cholesky synchronises the whole workgroup twice per tile row; its critical path is wave 0 (a 16 x 16 factorisation
// per row, ~4.7 k clocks each) and every barrier on that path is paid in full.  Here wave 0 of the set never waits for a
// barrier: the dependencies are three monotone counters in LDS (F[0]: trailing updates finished, one arrival per worker and
// row; F[1]: inverses of the diagonal tiles published by wave 0; F[2]: panel tiles of a row written, one arrival per wave),
//     wave 0:   [wait: the updates of the rows before are in]  R_J,J+1 = Rinv_J^T K_J,J+1   -> F[2]
//               K_J+1,J+1 -= R_J,J+1^T R_J,J+1;  chol16                                     -> F[1]
//     workers:  [wait F[1]: Rinv_J; wait F[0]: the rows before]  their panel tiles R_JJ'    -> F[2]
//               [wait F[2]: the whole panel]  their trailing tiles                           -> F[0]
// and what wave 0 waits for (the workers' trailing updates of the row before) has normally finished long before it asks: the
// workers run one row behind, beside the factorisation of the next diagonal tile.  A wave's LDS writes reach the LDS before
// its own later arrival (the LDS queue of a wave is in order), the fences keep the compiler from moving accesses across.
// No early exit on a failed pivot (NaNs are harmless, the caller tests L.flag[1] after the halves have joined).
__device__ __forceinline__ void set_signal(liptr c) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if ((SRH_TID & 63) == 0) __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// SLEEP: the workers' waits (one row behind wave 0, long): s_sleep between polls -- same time as polling back to back
// (58.7 vs 58.7-59.2 ms per 4096 rollouts), fewer instructions issued beside the wave that factorises
template <bool SLEEP = false>
__device__ __forceinline__ void set_wait(liptr c, int v) {
    if ((SRH_TID & 63) == 0) { while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) { if (SLEEP) __builtin_amdgcn_s_sleep(4); } }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ wg::qp_d4 panel_tile(Lds &L, int KT, int J, int Jp, int l16, int kk) {      // R_JJ' = Rinv_J^T K_JJ' (returned as well)
    clptr Ri = rinv_tile(L, J, KT);
    lptr T = L.B + (size_t)qpc::tile_index(J, Jp, KT) * TSZ;
    double av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { av[s] = Ri[(4 * s + kk) * TS + l16]; bv[s] = T[(4 * s + kk) * TS + l16]; }
    wg::qp_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) T[(kk + 4 * qd) * TS + l16] = acc[qd];
    return acc;
}
// T <- T - P^T P with P in the registers panel_tile() returned: the accumulator layout of the MFMA (lane (l16, kk): rows kk + 4 q) IS its
// operand layout (k-step s: row 4 s + kk) -- the same products in the same order as qpc::tile_update(T, P, P), without reading P back
__device__ __forceinline__ void tile_update_reg(lptr T, const wg::qp_d4 &P, int l16, int kk) {
    wg::qp_d4 acc;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) acc[qd] = T[(kk + 4 * qd) * TS + l16];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-P[s], P[s], acc, 0, 0, 0);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) T[(kk + 4 * qd) * TS + l16] = acc[qd];
}
// F: three LDS counters, zero on entry.  Returns nothing: L.flag[1] = 1 iff every pivot was positive (valid after the caller's barrier).
// wave: this wave's place in the protocol (0: the chain, w >= 1: worker w - 1); nwk0, roster: the row roster (roster_nwk and the targets next to
// it) -- roster 0 is nwk0 workers in every row.  Every branch on them is scalar: they are uniform over the wave.
__device__ __forceinline__ void tile_cholesky_set(const QPDims &d, Lds &L, int wave, int lane, int nwk0, liptr F, liptr Fnext, int roster = 0) {
    const int KT = d.KT;
    const int l16 = lane & 15, kk = lane >> 4;
    liptr Ftrail = F, Frinv = F + 1, Fpanel = F + 2;
    if (wave == 0) {
        lapc::Laps<lapc::CH_END> cl;
        bool ok = qpc::chol16<false>(L.B, rinv_tile(L, 0, KT));
        cl.lap(lapc::CH_FACTOR);
        set_signal(Frinv);
        cl.lap(lapc::CH_SIGNALS);
        for (int J = 0; J + 1 < KT; ++J) {
            set_wait(Fnext, roster_next_target(J));                // (J, J + 1) and (J + 1, J + 1) carry the updates of row J - 1
            cl.lap(lapc::CH_WAIT);
            const wg::qp_d4 P = panel_tile(L, KT, J, J + 1, l16, kk);
            cl.lap(lapc::CH_PANEL);
            set_signal(Fpanel);
            cl.lap(lapc::CH_SIGNALS);
            lptr T = L.B + (size_t)qpc::tile_index(J + 1, J + 1, KT) * TSZ;
            __builtin_amdgcn_wave_barrier();
            tile_update_reg(T, P, l16, kk);
            __builtin_amdgcn_wave_barrier();
            cl.lap(lapc::CH_UPDATE);
            ok = qpc::chol16<false>(T, rinv_tile(L, J + 1, KT)) && ok;
            cl.lap(lapc::CH_FACTOR);
            set_signal(Frinv);
            cl.lap(lapc::CH_SIGNALS);
        }
        if (lane == 0) L.flag[1] = ok ? 1 : 0;
        if constexpr (lapc::ON) { if (lane == 0) for (int i = 0; i < lapc::CH_END; ++i) L.Qu[lapc::MAIL_CHAIN + i] = (double)cl[i]; }
    } else {
        const int worker = wave - 1;
        for (int J = 0; J + 1 < KT; ++J) {
            const int nwk = roster_nwk(roster, nwk0, J);
            if (!roster_works(roster, nwk0, worker, J)) continue;    // not in this row's roster: no counter touched
            set_wait<true>(Frinv, J + 1);
            set_wait<true>(Ftrail, roster_trail_target(roster, nwk0, J));
            for (int Jp = roster_panel_first(worker, J); Jp < KT; Jp += nwk) panel_tile(L, KT, J, Jp, l16, kk);      // (J, J + 1) is the chain's
            set_signal(Fpanel);
            set_wait<true>(Fpanel, roster_panel_target(roster, nwk0, J));
            // tiles 1 .. ntr-1 over the workers (roster_trailing_tile): the chain does not wait for the whole trailing update of a row
            // (20 tiles in row 0), only for the two early tiles, each announced on its own
            const int ntr = roster_ntr(KT, J);
            for (int t = worker + 1; t < ntr; t += nwk) {
                int I, Kc;
                bool first;
                roster_trailing_tile(KT, J, t, I, Kc, first);
                qpc::tile_update(L.B + (size_t)qpc::tile_index(I, Kc, KT) * TSZ, L.B + (size_t)qpc::tile_index(J, I, KT) * TSZ,
                                 L.B + (size_t)qpc::tile_index(J, Kc, KT) * TSZ, l16, kk);
                if (first) set_signal(Fnext);
            }
            set_signal(Ftrail);
        }
    }
}

// ------------------------------------------------------------------ K^-1 v with the factor in unit-block-diagonal form
// qpc::k_solve substitutes through the 2 KT block rows on one wave with a diagonal solve, two LDS round trips and four
// ds_bpermute sums per block row (23 k clocks per right-hand side, two or three per factorisation).  Here the factor is
// rewritten once per factorisation as R = Dh Uh, Dh = blockdiag(R_JJ), Uh_IJ = Rinv_I R_IJ (unit block diagonal, in place
// of R_IJ: one MFMA product per tile, all waves), so that
//     K^-1 v = Uh^-1 ( Dh^-1 Dh^-T ( Uh^-T v ) )
// and both block substitutions have NO diagonal solve: right-looking on one wave, the partial sums of every block row that
// is still open live in registers (the updates of the rows further down are independent work that covers the latency of
// the one LDS round trip per step), the 4 partial sums of an entry sit in one quad (two DPP adds).  The block-diagonal
// scaling in the middle is one tile per wave.  (An explicit inverse T = R^-1 with x = T T^T v was measured as well: 2.5 k
// clocks per solve, but its residual costs the interior point an iteration on some QPs -- slower overall.)
__device__ __forceinline__ void unit_tiles(const QPDims &d, Lds &L) {
    const int KT = d.KT, tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l16 = lane & 15, kk = lane >> 4, noff = KT * (KT - 1) / 2;
    for (int t = wave; t < noff; t += (int)(blockDim.x >> 6)) {
        int tt = t, I = 0;
        while (tt >= KT - 1 - I) { tt -= KT - 1 - I; ++I; }
        const int J = I + 1 + tt;
        lptr T = L.B + (size_t)qpc::tile_index(I, J, KT) * TSZ;
        clptr Ri = rinv_tile(L, I, KT);
        double av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) { av[s] = Ri[l16 * TS + 4 * s + kk]; bv[s] = T[(4 * s + kk) * TS + l16]; }
        wg::qp_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) T[(kk + 4 * q) * TS + l16] = acc[q];
    }
    __syncthreads();
}

// v <- K^-1 v (scaled K; v: 16 KT doubles of LDS).  KT <= 8; KTC > 0 fixes KT at compile time (no branch between the tile
// updates of a step: their LDS reads are issued together instead of one tile at a time).
template <int KTC>
__device__ __forceinline__ void k_solve_unit_impl(const QPDims &d, Lds &L, lptr v) {
    constexpr int KMAX = KTC > 0 ? KTC : 8;
    const int KT = KTC > 0 ? KTC : d.KT, tid = SRH_TID, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int c = lane >> 2, part = lane & 3;
    const int sw = serial_wave(L);
    if (wave == sw) {                                                    // y = Uh^-T v
        double acc[KMAX];
#pragma unroll
        for (int J = 0; J < KMAX; ++J) acc[J] = 0.0;
#pragma unroll
        for (int I = 0; I < KMAX; ++I) {
            if (KTC > 0 || I < KT) {
                const double yI = v[16 * I + c] - wg::group_sum<4>(acc[I]);
                __builtin_amdgcn_wave_barrier();
                if (part == 0) v[16 * I + c] = yI;
                __builtin_amdgcn_wave_barrier();
                const double y0 = v[16 * I + 4 * part], y1 = v[16 * I + 4 * part + 1], y2 = v[16 * I + 4 * part + 2], y3 = v[16 * I + 4 * part + 3];
#pragma unroll
                for (int J = I + 1; J < KMAX; ++J) {
                    if (KTC > 0 || J < KT) {
                        clptr T = L.B + (size_t)qpc::tile_index(I, J, KT) * TSZ + (4 * part) * TS + c;
                        acc[J] = fma(T[0], y0, fma(T[TS], y1, fma(T[2 * TS], y2, fma(T[3 * TS], y3, acc[J]))));
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int J = wave; J < KT; J += (int)(blockDim.x >> 6)) {            // w_J = Rinv_J (Rinv_J^T y_J): a tile per wave (4-wave workgroups: two rounds)
        clptr Ri = rinv_tile(L, J, KT);
        double t = 0.0;
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) t = fma(Ri[(4 * part + kq) * TS + c], v[16 * J + 4 * part + kq], t);
        t = wg::group_sum<4>(t);
        __builtin_amdgcn_wave_barrier();
        if (part == 0) v[16 * J + c] = t;
        __builtin_amdgcn_wave_barrier();
        double w = 0.0;
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) w = fma(Ri[c * TS + 4 * part + kq], v[16 * J + 4 * part + kq], w);
        w = wg::group_sum<4>(w);
        __builtin_amdgcn_wave_barrier();
        if (part == 0) v[16 * J + c] = w;
    }
    __syncthreads();
    if (wave == sw) {                                                    // x = Uh^-1 w
        double acc[KMAX];
#pragma unroll
        for (int J = 0; J < KMAX; ++J) acc[J] = 0.0;
#pragma unroll
        for (int Jp = KMAX - 1; Jp >= 0; --Jp) {
            if (KTC > 0 || Jp < KT) {
                const double xJ = v[16 * Jp + c] - wg::group_sum<4>(acc[Jp]);
                __builtin_amdgcn_wave_barrier();
                if (part == 0) v[16 * Jp + c] = xJ;
                __builtin_amdgcn_wave_barrier();
                const double x0 = v[16 * Jp + 4 * part], x1 = v[16 * Jp + 4 * part + 1], x2 = v[16 * Jp + 4 * part + 2], x3 = v[16 * Jp + 4 * part + 3];
#pragma unroll
                for (int J = 0; J < Jp; ++J) {
                    clptr T = L.B + (size_t)qpc::tile_index(J, Jp, KT) * TSZ + c * TS + 4 * part;
                    acc[J] = fma(T[0], x0, fma(T[1], x1, fma(T[2], x2, fma(T[3], x3, acc[J]))));
                }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void k_solve_unit(const QPDims &d, Lds &L, lptr v) {
    if (d.KT == 7) k_solve_unit_impl<7>(d, L, v);            // N p_o = 100: the benchmark horizons
    else k_solve_unit_impl<0>(d, L, v);
}

// Newton direction (qpc::newton_solve with the products from the packed store), in two halves:
//   front (needs the gradients, D, Ls and the scaling ks of K -- NOT the factor): t = -D^-1 (g_u + G^T g_y), the reduced dual
//          residual max |g_ud + G^T g_yd| when gyd != null (into L.Qu[0]), yc = ks Ls^T G t;  runs on any wave set
//   back  (needs the factor): v = K^-1 yc, du = t - D^-1 G^T Ls ks v, dy = G du
// keep_gt / reuse_gt (problems without state rows: the y-space gradient g_y = L.ya is the cost's alone and does not change between
// the predictor and the corrector of an iteration): the predictor leaves G^T g_y in L.tb (free once the dual residual has been
// taken), the corrector reads it there instead of repeating the product.
template <int MSEL, bool HALF, class GP>
__device__ __forceinline__ void newton_front(const QPDims &d, const GP &g, Lds &L, clptr gyd, Waves<HALF> &W, Prof &pf,
                                             bool keep_gt = false, bool reuse_gt = false) {
    const int N = d.N, nm = N * d.m, ldG = 16 * d.KT, tid = W.tid, nt = W.nt;
    pf.lap(lapc::NT_GRADIENTS);
    if (!reuse_gt) gT_times<MSEL, HALF>(d, g, L, L.ya, gyd, L.du, gyd ? L.tc : (lptr) nullptr, W);
    clptr gty = reuse_gt ? (clptr)L.tb : (clptr)L.du;
    pf.lap(lapc::NT_GT1);
    if (gyd) {
        double r = 0.0;
        for (int e = tid; e < nm; e += nt) r = fmax(r, fabs(L.tb[e] + L.tc[e]));
        r = wg::wave_max(r);
        if ((tid & 63) == 0) L.red[W.wave] = r;
    }
    for (int e = tid; e < nm; e += nt) {                                                                            // t = -D^-1 g (diagonal D)
        const double sd = L.Ldi[e], gt = gty[e];
        L.ta[e] = -(L.ta[e] + gt) * (sd * sd);
        if (keep_gt) L.tb[e] = gt;
    }
    W.sync();
    if (gyd && tid == 0) { double r = L.red[0]; for (int i = 1; i < W.nw; ++i) r = fmax(r, L.red[i]); L.Qu[0] = r; }
    pf.lap(lapc::NT_RHS);
    g_times<MSEL, HALF>(d, g, L, L.ta, L.yb, W);
    pf.lap(lapc::NT_G1);
    // yc = ks (Ls^T yb) per output stage (p_o = 2, Ls lower: out_0 = L00 v0 + L10 v1, out_1 = L11 v1); padding zeroed
    for (int k = tid; k < ldG / 2; k += nt) {
        double o0 = 0.0, o1 = 0.0;
        if (k < N) {
            clptr Lk = L.Ls + (size_t)k * 4;
            const double v0 = L.yb[2 * k], v1 = L.yb[2 * k + 1];
            o0 = fma(Lk[2], v1, Lk[0] * v0) * L.ks[2 * k];
            o1 = Lk[3] * v1 * L.ks[2 * k + 1];
        }
        L.yc[2 * k] = o0; L.yc[2 * k + 1] = o1;
    }
    W.sync();
}

template <int MSEL, class GP>
__device__ __forceinline__ void newton_back(const QPDims &d, const GP &g, Lds &L, Prof &pf) {
    const int N = d.N, nm = N * d.m, ldG = 16 * d.KT, tid = SRH_TID, nt = blockDim.x;
    k_solve_unit(d, L, L.yc);
    // yd = Ls (ks v) per output stage: out_0 = L00 v0, out_1 = L10 v0 + L11 v1.
    // dy: with w = ks v the solved system reads (I + Ls^T Ky Ls) w = Ls^T yb, Ky = G D^-1 G^T, yb = G t, so that
    //     dy = G du = yb - Ky Ls w = Ls^-T w
    // -- one 2 x 2 back substitution per output stage instead of the product G du (d.ls_pd: every Ls_k is invertible; what the
    // two forms differ by is the residual of the K solve)
    const bool dy_here = d.ls_pd != 0;
    for (int k = tid; k < ldG / 2; k += nt) {
        double o0 = 0.0, o1 = 0.0, e0 = 0.0, e1 = 0.0;
        if (k < N) {
            clptr Lk = L.Ls + (size_t)k * 4;
            const double v0 = L.yc[2 * k] * L.ks[2 * k], v1 = L.yc[2 * k + 1] * L.ks[2 * k + 1];
            o0 = Lk[0] * v0;
            o1 = fma(Lk[3], v1, Lk[2] * v0);
            e1 = v1 / Lk[3];
            e0 = fma(-Lk[2], e1, v0) / Lk[0];
        }
        L.yd[2 * k] = o0; L.yd[2 * k + 1] = o1;
        if (dy_here) { L.dy[2 * k] = e0; L.dy[2 * k + 1] = e1; }
    }
    __syncthreads();
    pf.lap(lapc::NT_KSOLVE);
    gT_times<MSEL>(d, g, L, L.yd, (clptr) nullptr, L.du, (lptr) nullptr);
    pf.lap(lapc::NT_GT2);
    for (int e = tid; e < nm; e += nt) { const double sd = L.Ldi[e]; L.du[e] = L.ta[e] - L.du[e] * (sd * sd); }
    __syncthreads();
    pf.lap(lapc::NT_DU);
    if (!dy_here) g_times<MSEL>(d, g, L, L.du, L.dy);
    pf.lap(lapc::NT_G2);
}

// the whole solve on the whole workgroup (the general-row interior point; corrector solves)
template <int MSEL, class GP>
__device__ __forceinline__ void newton_solve(const QPDims &d, const GP &g, Lds &L, clptr gyd, double *rd, Prof &pf, bool reuse_gt = false) {
    auto W = all_waves();
    newton_front<MSEL, false>(d, g, L, gyd, W, pf, false, reuse_gt);
    if (gyd) *rd = L.Qu[0];
    newton_back<MSEL>(d, g, L, pf);
}
// (profile builds) the Gram fill's per-wave sums of a workgroup of nw waves
__device__ __forceinline__ void print_gram_wave_laps(int nw) {
    printf("lean gram per wave (cumulative) products:");
    for (int i = 0; i < nw; ++i) printf(" %lld", lapc::WaveLaps::get(i));
    printf("  epilogue:");
    for (int i = 0; i < nw; ++i) printf(" %lld", lapc::WaveLaps::get(8 + i));
    printf("\n");
}
// what the two wave sets of a split Newton system left in the lap mailbox, into the launch array (behind the join's barrier; read LDS:
// call it behind `if constexpr (lapc::ON)`)
__device__ __forceinline__ void split_mail_fold(Lds &L, lapc::Launch &prof) {
    prof.add(lapc::SPLIT_FACTOR, (long long)L.Qu[lapc::MAIL_SPLIT_FACTOR]); prof.add(lapc::SPLIT_FRONT, (long long)L.Qu[lapc::MAIL_SPLIT_FRONT]);
    for (int i = 0; i < lapc::CH_END; ++i) prof.add(lapc::CHAIN_WAIT + i, (long long)L.Qu[lapc::MAIL_CHAIN + i]);
}

// The condensation (G, free response) depends on the linearisation only: when the region sequence of this QP equals
// the one G was built from (a rejected SCP step: only delta / omega change, gusto.py:341 `update(full=new)`; or an
// accepted step whose trajectory stays in the same regions) it is still in LDS / the L2 block.  `x0` does not change
// inside a solve; the single-QP kernel (no region index) always condenses.  `from`: the sequence G was built from (L.goff, the half-size
// layout's L.goffg; L.flag[2] != 0: there is one).  The vote goes through L.flag[3] (__syncthreads_and brings static LDS of its own: the
// carve uses all 160 KB) behind two barriers; a caller that uses L.flag[3] for something else afterwards adds its own.
template <class IP>
__device__ __forceinline__ bool same_regions(const QPDyn &dyn, Lds &L, IP from, int N, int tid, int nt) {
    if (dyn.idx == nullptr) return false;
    int same = L.flag[2];
    for (int k = tid; k < N; k += nt) same = same && (from[k] == L.idxl[k]);
    if (tid == 0) L.flag[3] = 1;
    __syncthreads();
    if (!same) L.flag[3] = 0;
    __syncthreads();
    return L.flag[3] != 0;
}

// Lower Cholesky factor (row-major in Lk) of a symmetric positive SEMI-definite 2 x 2 block in closed form (oracle/condensed_ipm.py:
// chol_psd): a pivot that has cancelled to nothing -- 1e-14 of the larger diagonal entry -- gets a zero column.
__device__ __forceinline__ void chol2_psd(double S00, double S01, double S11, lptr Lk) {
    const double dmax = fmax(fabs(S00), fabs(S11));
    const double l00 = S00 > 1e-14 * dmax ? sqrt(S00) : 0.0;
    const double l10 = l00 > 0.0 ? S01 / l00 : 0.0;
    const double v = fma(-l10, l10, S11);
    const double l11 = v > 1e-14 * dmax ? sqrt(v) : 0.0;
    Lk[0] = l00; Lk[1] = 0.0; Lk[2] = l10; Lk[3] = l11;
}

__device__ __forceinline__ void reduce2(double &a, int opa, double &b, int opb, lptr scratch);      // (with ipm_box's helpers below)
// The stopping test of the predictor pass BEFORE its Newton system (ipm_rule.h, PRED; oracle/condensed_ipm.py:286-292 tests there
// too): mu and rp come out of the rows phase, the dual residual rd = max |g_ud + G^T g_yd| needs one product and neither K nor its
// factor.  Where the two conditions without rd hold (ipm::may_converge: the last iteration or two of a QP) the product runs on the
// whole workgroup into L.tc, as newton_front leaves it there, and rd is taken by the same maximum; if the test holds the caller stops
// with status 0 and builds no system.  Otherwise the pass goes on as it was: the front repeats the product.  GRP: rows per pass of the
// front's wave set -- rd has the bits the front gives (gT_times), so no verdict moves.  Called by every thread behind the barrier of
// the rows phase; the answer is uniform.  EARLY_NO_GATE: no product was made (always under QPDims::ipm_late_stop); EARLY_GO_ON: the
// product was made and the test failed; EARLY_STOP: converged.
enum { EARLY_NO_GATE = 0, EARLY_GO_ON = 1, EARLY_STOP = 2 };
template <int MSEL, int GRP, class GP>
__device__ __forceinline__ int converged_early(const QPDims &d, const GP &g, Lds &L, double mu, double rp, double sd, double sp, double &rd) {
    rd = 0.0;
    if (d.ipm_late_stop || !ipm::may_converge(mu, rp, sp, d.tol)) return EARLY_NO_GATE;
    auto W = all_waves();
    gT_times<MSEL, false, GRP>(d, g, L, L.yg, (clptr) nullptr, L.tc, (lptr) nullptr, W);
    const int nm = d.N * d.m;
    double r = 0.0, dummy = 0.0;
    for (int e = W.tid; e < nm; e += W.nt) r = fmax(r, fabs(L.tb[e] + L.tc[e]));
    reduce2(r, 1, dummy, 0, L.red);
    rd = r;
    return ipm::converged(mu, r, rp, sd, sp, d.tol) ? EARLY_STOP : EARLY_GO_ON;
}

// ------------------------------------------------------------------ the QP without its trust-region rows
// Results: w.u, and -- after the final rollout of solve_qp below -- w.x.  Returns 0 optimal, 1 max iterations, 2 numerical failure.
template <int MSEL, int NSEL>
__device__ __forceinline__ int ipm(const QPDims &dfull, const QPConst &c, const QPDyn &dyn, const QPData &q, gptr work_base,
                                   Lds &L, QPLds &Lq, int *iters_out, QPWork &wout, lapc::Launch &prof) {
    int tid = SRH_TID;                                       // re-read at the top of every interior-point iteration (dev_la.h: SRH_TID)
    const int nt = blockDim.x;
    QPDims d = dfull;
    drop_trust_region_rows(d);
    QPWork w;
    qp_carve(w, work_base, d);
    wout = w;
    gptr gh = work_base + dfull.qc_off;
    const int N = d.N, m = d.m, po = d.po, nm = N * m, ldG = 16 * d.KT, NP = N * po;
    GPack g{(cgptr)gh, (clptr)(L.Gt), d.lean_j0, m, NP};
    Prof pf;
    lapc::Clock lp;
    for (int e = tid; e < nm; e += nt) { w.u[e] = 0.0; L.u[e] = 0.0; }
    static_assert(YPAD == 48, "the carve reserves 48 doubles behind ya, yd, yg");
    for (int e = tid; e < YPAD; e += nt) { L.ya[ldG + e] = 0.0; L.yd[ldG + e] = 0.0; L.yg[ldG + e] = 0.0; }
    for (int e = tid; e <= N; e += nt) w.s[e] = 0.0;
    for (int k = tid; k < N; k += nt) L.idxl[k] = dyn.idx ? dyn.idx[k] : k;
    for (int e = tid; e < d.nU * m; e += nt) L.UA[e] = c.UA[e];
    for (int e = tid; e < (d.nX + d.nXf) * po; e += nt) L.Tx[e] = e < d.nX * po ? c.Tx[e] : c.Txf[e - d.nX * po];
    __syncthreads();
    const bool reuse = same_regions(dyn, L, L.goff, N, tid, nt);
    if (!reuse) {
    rollout<MSEL, NSEL>(d, dyn, q.x0, (cgptr) nullptr, w.x, L);
    lp.lap(prof, lapc::QP_SETUP);
    condense<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
    for (int k = tid; k < N; k += nt) L.goff[k] = L.idxl[k];
    if (tid == 0) L.flag[2] = 1;
    }
    for (int e = tid; e < ldG; e += nt) { L.y[e] = L.yf[e]; L.dy[e] = 0.0; }
    __syncthreads();
    lp.lap(prof, lapc::QP_CONDENSE);
    bool rv[QR], ru[QR];
    int rk[QR], rr[QR];
    double rh[QR], rt[QR], rlam[QR], rrg[QR], rrc[QR], rdt[QR], rdl[QR];
#pragma unroll
    for (int qi = 0; qi < QR; ++qi) {
        const int e = tid + nt * qi, nxs = N * d.RX;
        rt[qi] = rlam[qi] = rrg[qi] = rrc[qi] = rdt[qi] = rdl[qi] = 0.0;
        if (e < nxs) {
            rk[qi] = e / d.RX + 1; rr[qi] = e - (rk[qi] - 1) * d.RX; ru[qi] = false;
            rv[qi] = rr[qi] < qp::xrows_of(d, rk[qi]);
        } else {
            const int e2 = e - nxs;
            ru[qi] = true; rv[qi] = e2 < N * d.nU;
            rk[qi] = rv[qi] ? e2 / d.nU : 0; rr[qi] = rv[qi] ? e2 - rk[qi] * d.nU : 0;
        }
        rh[qi] = rv[qi] ? qp::row_h(d, c, q, ru[qi], rk[qi], rr[qi]) : 0.0;
    }
    auto row_val = [&](int qi, clptr vy, clptr vu) {
        double acc = 0.0;
        if (!ru[qi]) { for (int a = 0; a < po; ++a) acc = fma(L.Tx[rr[qi] * po + a], vy[(rk[qi] - 1) * po + a], acc); }
        else { for (int j = 0; j < m; ++j) acc = fma(L.UA[rr[qi] * m + j], vu[rk[qi] * m + j], acc); }
        return acc;
    };
    int status = 1, it = 0;
    enum { INIT = 0, PRED = 1, CORR = 2 };
    int mode = INIT;
    double mu = 0.0, rp = 0.0, sig = 0.0, sd = 1.0, sp = 1.0, dreg = 0.0;
    bool near_opt = false;
    while (true) {
        tid = SRH_TID;
        lp.lap(prof, lapc::QP_STEPS);
        double musum = 0.0, rpm = 0.0;
#pragma unroll
        for (int qi = 0; qi < QR; ++qi) {
            if (!rv[qi]) continue;
            const int e = tid + nt * qi;
            double D, rho;                                  // of this row, to L2 for the stage sums
            if (mode == INIT) {
                ipm::init_row(row_val(qi, L.y, L.u) - rh[qi], 1.0, D, rho, rlam[qi]);
                w.D[e] = D; w.rho[e] = rho;
            } else if (mode == PRED) {
                ipm::pred_row(row_val(qi, L.y, L.u) - rh[qi], rt[qi], rlam[qi], dreg, rrg[qi], D, rho, musum, rpm);
                w.D[e] = D; w.rho[e] = rho; w.lam[e] = rlam[qi];
            } else {
                ipm::corr_row(rt[qi], rlam[qi], rrg[qi], rdt[qi], rdl[qi], sig, mu, dreg, rrc[qi], rho);
                w.rho[e] = rho;
            }
        }
        if (mode == PRED) {
            mu = wg::reduce(musum, 0, L.red) / d.ng;
            rp = wg::reduce(rpm, 1, L.red);
        }
        __syncthreads();
        lp.lap(prof, lapc::QP_ROWS);
        // converged already?  Then no system (converged_early; the gradients of the dual residual as below, the front's own partition)
        if (mode == PRED && !d.ipm_late_stop && ipm::may_converge(mu, rp, sp, d.tol)) {
            qpc::gradients(d, c, q, L, w.lam, L.tb, L.yg);
            double rde;
            if (converged_early<MSEL, 0>(d, g, L, mu, rp, sd, sp, rde) == EARLY_STOP) {
                if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rde; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
                status = 0;
                break;
            }
        }
        double rd = 0.0;
        bool ok = true;
        if (mode != CORR) {
            ok = qpc::stage_factors(d, c, w.D, L);
            lp.lap(prof, lapc::QP_STAGE_FACTORS);
            if (ok) {
                gram<MSEL>(d, c, g, L);
                lp.lap(prof, lapc::QP_GRAM);
                ok = qpc::tile_cholesky(d, L);
                if (ok) unit_tiles(d, L);
                lp.lap(prof, lapc::QP_CHOLESKY);
            }
        }
        pf.restart();
        if (ok) {
            if (mode == PRED) qpc::gradients(d, c, q, L, w.lam, L.tb, L.yg);
            qpc::gradients(d, c, q, L, w.rho, L.ta, L.ya);
            newton_solve<MSEL>(d, g, L, mode == PRED ? (clptr)L.yg : (clptr) nullptr, &rd, pf);
        }
        lp.lap(prof, lapc::QP_NEWTON);
        if (mode == INIT) {
            if (ipm::stops(ipm::verdict_system(ok), status)) break;
            for (int e = tid; e < nm; e += nt) L.u[e] += L.du[e];
            for (int e = tid; e < ldG; e += nt) L.y[e] += L.dy[e];
            __syncthreads();
            if (ipm::stops(ipm::verdict_no_rows(d.ng), status)) break;
            double zmin = INFINITY, zmax = -INFINITY;
#pragma unroll
            for (int qi = 0; qi < QR; ++qi) {
                if (!rv[qi]) continue;
                const double gq = row_val(qi, L.y, L.u) - rh[qi];
                rrg[qi] = gq;
                zmin = fmin(zmin, gq); zmax = fmax(zmax, gq);
            }
            zmin = wg::reduce(zmin, 2, L.red);
            zmax = wg::reduce(zmax, 1, L.red);
            const ipm::Shift sh = ipm::start_shift(zmin, zmax);
#pragma unroll
            for (int qi = 0; qi < QR; ++qi) ipm::start_cold(rrg[qi], sh, rt[qi], rlam[qi]);
            qp::residual_scales(d, c, q, tid, nt, sd, sp, dreg, [&](double &a, double &b) { a = wg::reduce(a, 1, L.red); b = wg::reduce(b, 1, L.red); });
            mode = PRED;
            continue;
        }
        double amax = 1e300;
        if (ok) {
#pragma unroll
            for (int qi = 0; qi < QR; ++qi) {
                if (!rv[qi]) continue;
                ipm::direction(mode == PRED, rt[qi], rlam[qi], rrg[qi], rrc[qi], row_val(qi, L.dy, L.du), dreg, rdl[qi], rdt[qi]);
                ipm::step_bound(rt[qi], rlam[qi], rdt[qi], rdl[qi], amax);
            }
        }
        amax = wg::reduce(amax, 2, L.red);
        if (mode == PRED) {
            if (ipm::stops(ipm::verdict_failed(ok, mu, rd, near_opt), status)) break;
            if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rd; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
            if (ipm::stops(ipm::verdict_converged(mu, rd, rp, sd, sp, d.tol, it, d.max_iter, near_opt), status)) break;
            const double a_aff = ipm::step_affine(amax);
            double ma = 0.0;
#pragma unroll
            for (int qi = 0; qi < QR; ++qi)
                if (rv[qi]) ma += ipm::affine_term(rt[qi], rlam[qi], rdt[qi], rdl[qi], a_aff);
            const double mu_aff = wg::reduce(ma, 0, L.red) / d.ng;
            sig = ipm::centring(mu_aff, mu);
            if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[5] = a_aff; gd[6] = sig; }
            mode = CORR;
            continue;
        }
        if (ipm::stops(ipm::verdict_system(ok), status)) break;
        const double a = ipm::step_length(amax);
        if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[7] = a; }
        for (int e = tid; e < nm; e += nt) L.u[e] += a * L.du[e];
        for (int e = tid; e < ldG; e += nt) L.y[e] += a * L.dy[e];
#pragma unroll
        for (int qi = 0; qi < QR; ++qi) ipm::advance(a, rdt[qi], rdl[qi], rt[qi], rlam[qi]);
        __syncthreads();
        ++it;
        mode = PRED;
    }
    __syncthreads();
    for (int e = tid; e < nm; e += nt) w.u[e] = L.u[e];
    __syncthreads();
    pf.fold(prof);
    if (iters_out) *iters_out = it;
    return status;
}

// ------------------------------------------------------------------ the same interior point, rows next to their sums
// ipm() above keeps qpc::solve's row handling: every inequality row in the registers of "some" thread, its weight D and
// gradient shift rho through L2 arrays, then stage_factors / gradients re-read them per stage -- three L2 round trips and
// ~35 k clocks per Newton system that do no arithmetic to speak of.  ipm_box() maps the rows so that the sums are LOCAL:
//   * input rows: the reference's HyperRectangle layout (rows 2 b and 2 b + 1 bound input b, utils.py:390-414): thread
//     (k, b) owns both, so D_kb = 2 R_bb + a0^2 D0 + a1^2 D1 and the input gradient need no other thread;
//   * state rows of stage k: GX = 1, 2, 4 or 8 adjacent lanes; S_k = S* + sum_r D_r t_r t_r^T and the output gradient by
//     DPP sums, the 2 x 2 (semidefinite) Cholesky factor in closed form by the first lane.
// Same iteration, same quantities (sums in another order: rounding-level differences).  QPDims::lean == 2 selects it.
__device__ __forceinline__ void reduce2(double &a, int opa, double &b, int opb, lptr scratch) {
    auto wr = [](double v, int op) { return op == 0 ? wg::wave_sum(v) : (op == 1 ? wg::wave_max(v) : wg::wave_min(v)); };
    const double wa = wr(a, opa), wb = wr(b, opb);
    const int wave = __builtin_amdgcn_readfirstlane(SRH_TID >> 6), nw = blockDim.x >> 6;
    __syncthreads();
    if ((SRH_TID & 63) == 0) { scratch[wave] = wa; scratch[8 + wave] = wb; }
    __syncthreads();
    auto comb = [](double x, double y, int op) { return op == 0 ? x + y : (op == 1 ? fmax(x, y) : fmin(x, y)); };
    double ra = scratch[0], rb = scratch[8];
    for (int i = 1; i < nw; ++i) { ra = comb(ra, scratch[i], opa); rb = comb(rb, scratch[8 + i], opb); }
    a = ra; b = rb;
}

template <int G>
__device__ __forceinline__ double gsum(double v) {
    if constexpr (G == 1) return v;
    else if constexpr (G == 2) return v + wg::dpp_mov<0xB1>(v);
    else return wg::group_sum<G>(v);
}

template <int MSEL, int NSEL, int GX, int NST = 0, int J0SEL = 0>
__device__ __forceinline__ int ipm_box(const QPDims &dfull, const QPConst &c, const QPDyn &dyn, const QPData &q, gptr work_base,
                                       Lds &L, int *iters_out, QPWork &wout, lapc::Launch &prof, int warm_mode = 0) {
    // warm_mode: 0 cold start, 1 warm start (below), 2 warm start whose multipliers are replaced by +inf -- a test knob
    // (GustoPar::poison_warm, SRH_LEAN_POISON_WARM=1 at plan creation) that makes the warm attempt fail so that the caller's cold
    // retry runs under a test
    const bool warm = warm_mode != 0, poison = warm_mode == 2;
    int tid = SRH_TID;                                       // re-read at the top of every interior-point iteration (dev_la.h: SRH_TID)
    const int nt = blockDim.x;
    QPDims d = dfull;
    drop_trust_region_rows(d);
    QPWork w;
    qp_carve(w, work_base, d);
    wout = w;
    gptr gh = work_base + dfull.qc_off;
    const int N = d.N, m = d.m, nm = N * m, ldG = 16 * d.KT, NP = 2 * N, nz = d.nz;
    GPackT<NST, J0SEL> g{(cgptr)gh, (clptr)(L.Gt), d.lean_j0, m, NP};
    Prof pf;
    lapc::Clock lp, split;                     // (declared here, re-armed where they start: an object in a nested scope moved two PHIs of the product kernel)
    // warm (round 4): the previous QP of this SCP solve left its minimiser in w.u and its multipliers in w.lam -- this QP differs
    // by its linearisation point only and shares most of the active set: the interior point starts from that point (u as it
    // is, slacks from THIS QP's rows, multipliers kept, both at least WARM_FLOOR from zero) and skips the initial Newton system.
    // 7-9 interior-point iterations instead of 15-18 at C2 / C5, same minimiser (oracle/condensed_ipm.py: solve(warm=...)).
    if (warm) { for (int e = tid; e < nm; e += nt) L.u[e] = w.u[e]; }
    else { for (int e = tid; e < nm; e += nt) { w.u[e] = 0.0; L.u[e] = 0.0; } }
    for (int e = tid; e < ldG + YPAD; e += nt) { L.ya[e] = 0.0; L.yd[e] = 0.0; L.yg[e] = 0.0; }     // padding stays zero for good
    for (int e = tid; e <= N; e += nt) w.s[e] = 0.0;
    for (int k = tid; k < N; k += nt) L.idxl[k] = dyn.idx ? dyn.idx[k] : k;
    if constexpr (lapc::ON) { if (tid < 16) L.Qu[tid] = 0.0; }       // (the lap mailbox)
    if (tid < 5) L.flag[3 + tid] = 0;                          // counters of the two wave sets (Waves, tile_cholesky_set; [3]: idle between the region tests of two QPs)
    __syncthreads();
    const bool reuse = same_regions(dyn, L, L.goff, N, tid, nt);
    if (dyn.idx != nullptr) {
        __syncthreads();
        if (tid == 0) L.flag[3] = 0;                           // tile_cholesky_set's early-tile counter from here on
    }
    if (!reuse) {
        const bool single = single_region(d, c, dyn, L);
        rollout<MSEL, NSEL>(d, dyn, q.x0, (cgptr) nullptr, w.x, L);
        lp.lap(prof, lapc::QP_SETUP);
        if (single) condense_single<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
        else condense<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
        for (int k = tid; k < N; k += nt) L.goff[k] = L.idxl[k];
        if (tid == 0) L.flag[2] = 1;
    }
    if (warm) {                                               // y = y_free + G u
        __syncthreads();
        g_times<MSEL>(d, g, L, L.u, L.dy);
        for (int e = tid; e < ldG; e += nt) { L.y[e] = L.yf[e] + L.dy[e]; }
        __syncthreads();
        for (int e = tid; e < ldG; e += nt) L.dy[e] = 0.0;
    } else {
        for (int e = tid; e < ldG; e += nt) { L.y[e] = L.yf[e]; L.dy[e] = 0.0; }
    }
    __syncthreads();
    lp.lap(prof, lapc::QP_CONDENSE);
    // ---- this thread's rows
    const bool isu = tid < nm;
    const int tx = tid - nm;
    const bool isx = tx >= 0 && tx < N * GX;
    const int ku = isu ? tid / m : 0, bu = isu ? tid - ku * m : 0;
    const int kx = isx ? tx / GX + 1 : 1, rx = isx ? tx - (kx - 1) * GX : 0;        // stage 1..N, row slot
    const int nrk = d.nX + (kx == N ? d.nXf : 0);
    const bool xrow = isx && rx < nrk;                                               // the slot holds a state row
    const bool xlead = isx && rx == 0;                                               // first lane of the stage group
    double ca[2] = {0.0, 0.0}, rh[2] = {0.0, 0.0};                                   // row coefficients / right-hand sides
    if (isu) {
        ca[0] = c.UA[(size_t)(2 * bu) * m + bu]; ca[1] = c.UA[(size_t)(2 * bu + 1) * m + bu];
        rh[0] = c.Ub[2 * bu]; rh[1] = c.Ub[2 * bu + 1];
    } else if (xrow) {
        cgptr T = rx < d.nX ? c.Tx + (size_t)rx * 2 : c.Txf + (size_t)(rx - d.nX) * 2;
        ca[0] = T[0]; ca[1] = T[1];
        rh[0] = rx < d.nX ? c.Xb[rx] : c.Xfb[rx - d.nX];
    }
    const double r2bb = isu ? c.R2[bu * m + bu] : 0.0;
    const double udv = (isu && q.ud) ? q.ud[(size_t)ku * m + bu] : 0.0;
    // constant part of the output gradient of this stage (lead lane): -Cz2 z_k (- Czf2 zf at k = N)
    double gc0 = 0.0, gc1 = 0.0, s00 = 0.0, s01 = 0.0, s11 = 0.0;
    if (xlead) {
        cgptr S = (kx == N) ? c.ScN : c.Sc;
        s00 = S[0]; s01 = S[1]; s11 = S[3];
        if (q.z) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Cz2[b], q.z[(size_t)kx * nz + b], gc0); gc1 = fma(-c.Cz2[nz + b], q.z[(size_t)kx * nz + b], gc1); }
        if (kx == N && c.Qzf && q.zf) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Czf2[b], q.zf[b], gc0); gc1 = fma(-c.Czf2[nz + b], q.zf[b], gc1); }
    }
    const int nrow = isu ? 2 : (xrow ? 1 : 0);
    const int lslot = isu ? 2 * tid : 2 * nm + (kx - 1) * (d.nX + d.nXf) + rx;       // this thread's rows in w.lam (NR = N (nX + nXf) + N nU entries)
    double rt[2] = {0.0, 0.0}, rlam[2] = {0.0, 0.0}, rrg[2] = {0.0, 0.0}, rrc[2] = {0.0, 0.0}, rdt[2] = {0.0, 0.0}, rdl[2] = {0.0, 0.0};
    // a_row . (y, u) for row slot s2
    auto row_val = [&](int s2, clptr vy, clptr vu) -> double {
        if (isu) return ca[s2] * vu[tid];
        return fma(ca[1], vy[(kx - 1) * 2 + 1], ca[0] * vy[(kx - 1) * 2]);
    };
    int status = 1, it = 0;
    enum { INIT = 0, PRED = 1, CORR = 2 };
    int mode = INIT;
    double mu = 0.0, rp = 0.0, sig = 0.0, sd = 1.0, sp = 1.0, dreg = 0.0;
    bool near_opt = false;
    const bool ya_const = d.nX + d.nXf == 0;                  // no state rows: L.ya is the same in the predictor and the corrector (newton_front)
    auto scales = [&]() { qp::residual_scales(d, c, q, tid, nt, sd, sp, dreg, [&](double &a, double &b) { reduce2(a, 1, b, 1, L.red); }); };
    if (warm && d.ng > 0) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if (s2 >= nrow) continue;
            ipm::start_warm(row_val(s2, L.y, L.u) - rh[s2], [&] { return w.lam[lslot + s2]; }, poison, rt[s2], rlam[s2]);
        }
        scales();
        mode = PRED;
    }
    while (true) {
        tid = SRH_TID;
        lp.lap(prof, lapc::QP_STEPS);
        // ---------------- rows -> weights, gradient shifts, and their per-stage sums, all in place
        double musum = 0.0, rpm = 0.0;
        double Dw[2] = {0.0, 0.0}, rho[2] = {0.0, 0.0};
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if (s2 >= nrow) continue;
            if (mode == INIT) ipm::init_row(row_val(s2, L.y, L.u) - rh[s2], 1.0, Dw[s2], rho[s2], rlam[s2]);
            else if (mode == PRED) ipm::pred_row(row_val(s2, L.y, L.u) - rh[s2], rt[s2], rlam[s2], dreg, rrg[s2], Dw[s2], rho[s2], musum, rpm);
            else ipm::corr_row(rt[s2], rlam[s2], rrg[s2], rdt[s2], rdl[s2], sig, mu, dreg, rrc[s2], rho[s2]);
        }
        if (isu) {
            const double du0 = r2bb * (L.u[tid] - udv);
            if (mode != CORR) {
                double v = fma(ca[0] * Dw[0], ca[0], r2bb);
                v = fma(ca[1] * Dw[1], ca[1], v);
                L.Ldi[tid] = 1.0 / sqrt(v);
            }
            L.ta[tid] = fma(ca[1], rho[1], fma(ca[0], rho[0], du0));
            if (mode == PRED) L.tb[tid] = fma(ca[1], rlam[1], fma(ca[0], rlam[0], du0));
        }
        if (isx) {                                           // whole stage groups: the DPP sums see every lane of a group
            const double y0 = L.y[(kx - 1) * 2], y1 = L.y[(kx - 1) * 2 + 1];
            if (mode != CORR) {
                const double a00 = gsum<GX>(ca[0] * Dw[0] * ca[0]), a01 = gsum<GX>(ca[0] * Dw[0] * ca[1]), a11 = gsum<GX>(ca[1] * Dw[0] * ca[1]);
                if (xlead) chol2_psd(s00 + a00, s01 + a01, s11 + a11, L.Ls + (size_t)(kx - 1) * 4);
            }
            const double r0 = gsum<GX>(ca[0] * rho[0]), r1 = gsum<GX>(ca[1] * rho[0]);
            double l0 = 0.0, l1 = 0.0;
            if (mode == PRED) { l0 = gsum<GX>(ca[0] * rlam[0]); l1 = gsum<GX>(ca[1] * rlam[0]); }
            if (xlead) {
                const double c0 = fma(s01, y1, s00 * y0) + gc0, c1 = fma(s11, y1, s01 * y0) + gc1;
                L.ya[(kx - 1) * 2] = c0 + r0; L.ya[(kx - 1) * 2 + 1] = c1 + r1;
                if (mode == PRED) { L.yg[(kx - 1) * 2] = c0 + l0; L.yg[(kx - 1) * 2 + 1] = c1 + l1; }
            }
        }
        if (mode == PRED) {
            reduce2(musum, 0, rpm, 1, L.red);
            mu = musum / d.ng;
            rp = rpm;
        }
        __syncthreads();
        lp.lap(prof, lapc::QP_ROWS);
        // ---------------- converged already?  Then no system (converged_early; 32: the rows per pass of the front's four waves)
        if (mode == PRED) {
            double rde;                                        // (not rd: nothing of the early test stays live through the system)
            const int early = converged_early<MSEL, 32>(d, g, L, mu, rp, sd, sp, rde);
            if (early != EARLY_NO_GATE) { lp.lap(prof, lapc::EARLY_TEST); if (early == EARLY_GO_ON) prof.add(lapc::N_EARLY_FOR_NOTHING); }
            if (early == EARLY_STOP) {
                if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rde; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
                status = 0;
                break;
            }
        }
        // ---------------- Newton system
        double rd = 0.0;
        bool ok = true;
        if (mode != CORR) {
            lp.lap(prof, lapc::QP_STAGE_FACTORS);
            gram<MSEL>(d, c, g, L);
            lp.lap(prof, lapc::QP_GRAM);
            // the factorisation (waves 0-3: a chain of one-wave 16 x 16 factorisations) beside the half of the Newton solve that
            // does not need the factor (waves 4-7), see Waves
            const clptr gyd = mode == PRED ? (clptr)L.yg : (clptr) nullptr;
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            pf.restart();
            split.restart();
            auto W = half_waves(L.flag + 4);
            if (half_of_wave(wv) == 0) {
                tile_cholesky_set(d, L, W.wave, W.tid & 63, W.nw - 1, L.flag + 5, L.flag + 3);
                if constexpr (lapc::ON) { if (tid == 0) L.Qu[lapc::MAIL_SPLIT_FACTOR] = (double)split.since(); }
            } else {
                newton_front<MSEL, true>(d, g, L, gyd, W, pf, ya_const && mode == PRED);
                if constexpr (lapc::ON) { if (W.tid == 0) L.Qu[lapc::MAIL_SPLIT_FRONT] = (double)split.since(); }
            }
            __syncthreads();
            if constexpr (lapc::ON) split_mail_fold(L, prof);
            ok = L.flag[1] != 0;
            if (tid < 5) L.flag[3 + tid] = 0;                  // the factorising half's early-tile counter, the product half's arrival counter and the factorising half's three, for the next split
            if (gyd) rd = L.Qu[0];
            if (ok) unit_tiles(d, L);
            lp.lap(prof, lapc::QP_CHOLESKY);
            pf.restart();
            if (ok) newton_back<MSEL>(d, g, L, pf);
        } else {
            pf.restart();
            newton_solve<MSEL>(d, g, L, (clptr) nullptr, &rd, pf, ya_const);
        }
        lp.lap(prof, lapc::QP_NEWTON);
        // ---------------- use the direction
        if (mode == INIT) {
            if (ipm::stops(ipm::verdict_system(ok), status)) break;
            for (int e = tid; e < nm; e += nt) L.u[e] += L.du[e];
            for (int e = tid; e < ldG; e += nt) L.y[e] += L.dy[e];
            __syncthreads();
            if (ipm::stops(ipm::verdict_no_rows(d.ng), status)) break;
            double zmin = INFINITY, zmax = -INFINITY;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (s2 >= nrow) continue;
                const double gq = row_val(s2, L.y, L.u) - rh[s2];
                rrg[s2] = gq;
                zmin = fmin(zmin, gq); zmax = fmax(zmax, gq);
            }
            reduce2(zmin, 2, zmax, 1, L.red);
            const ipm::Shift sh = ipm::start_shift(zmin, zmax);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) ipm::start_cold(rrg[s2], sh, rt[s2], rlam[s2]);
            scales();
            mode = PRED;
            continue;
        }
        double amax = 1e300, dummy = 0.0;
        if (ok) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (s2 >= nrow) continue;
                ipm::direction(mode == PRED, rt[s2], rlam[s2], rrg[s2], rrc[s2], row_val(s2, L.dy, L.du), dreg, rdl[s2], rdt[s2]);
                ipm::step_bound(rt[s2], rlam[s2], rdt[s2], rdl[s2], amax);
            }
        }
        lp.lap(prof, lapc::STEP_ROWS);
        reduce2(amax, 2, dummy, 0, L.red);
        lp.lap(prof, lapc::STEP_AMAX);
        if (mode == PRED) {
            if (ipm::stops(ipm::verdict_failed(ok, mu, rd, near_opt), status)) break;
            if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rd; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
            if (ipm::stops(ipm::verdict_converged(mu, rd, rp, sd, sp, d.tol, it, d.max_iter, near_opt), status)) break;
            const double a_aff = ipm::step_affine(amax);
            double ma = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                if (s2 < nrow) ma += ipm::affine_term(rt[s2], rlam[s2], rdt[s2], rdl[s2], a_aff);
            lp.lap(prof, lapc::STEP_MU_ROWS);
            reduce2(ma, 0, dummy, 0, L.red);
            lp.lap(prof, lapc::STEP_MU_AFF);
            const double mu_aff = ma / d.ng;
            sig = ipm::centring(mu_aff, mu);
            if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[5] = a_aff; gd[6] = sig; }
            mode = CORR;
            continue;
        }
        if (ipm::stops(ipm::verdict_system(ok), status)) break;
        const double a = ipm::step_length(amax);
        if (q.dbg && tid == 0) { gptr gd = q.dbg + 8 * it; gd[7] = a; }
        for (int e = tid; e < nm; e += nt) L.u[e] += a * L.du[e];
        for (int e = tid; e < ldG; e += nt) L.y[e] += a * L.dy[e];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) ipm::advance(a, rdt[s2], rdl[s2], rt[s2], rlam[s2]);
        __syncthreads();
        ++it;
        mode = PRED;
    }
    __syncthreads();
    for (int e = tid; e < nm; e += nt) w.u[e] = L.u[e];
    if (status == 0) {                                        // what the next QP of this solve starts from (warm)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) if (s2 < nrow) w.lam[lslot + s2] = rlam[s2];
    }
    __syncthreads();
    pf.fold(prof, it, warm);
    if constexpr (lapc::ON) {
        if (tid == 0 && blockIdx.x == 0) {
            printf("lean gram laps (this QP, wave 0): 1/D+barrier %.0f descriptors %.0f products %.0f epilogue %.0f barrier %.0f scaling+barrier %.0f\n",
                   L.Qu[lapc::MAIL_GRAM], L.Qu[lapc::MAIL_GRAM + 1], L.Qu[lapc::MAIL_GRAM + 2], L.Qu[lapc::MAIL_GRAM + 3], L.Qu[lapc::MAIL_GRAM_BARRIER], L.Qu[lapc::MAIL_GRAM_STORE]);
            print_gram_wave_laps(8);
        }
    }
    if (iters_out) *iters_out = it;
    return status;
}

// ------------------------------------------------------------------ ipm_box for the HALF-SIZE workgroup (4 waves, <= 80 KB of LDS)
// The same iteration as ipm_box() -- same starting points, weights, stopping rule, warm start, same phase order -- for a workgroup of 256
// threads that shares its CU with a second rollout (QPDims::lean_half, lean.hip: the <.., N, N, ..> instantiations).  What differs:
//   * a thread owns BOTH an input (its two box rows) and a state-row slot (ipm_box gives them to different threads: N m + N GX <= 512);
//     the per-stage sums of the state rows are the same DPP sums over GX adjacent lanes;
//   * the free response yf and the region sequence of the condensation come from the problem's L2 block (Lds::yfg / goffg), every packed
//     row of G from there as well (lean_j0 = N; the Gram fill stages the rows that fit the K-tile area there first: gram_t<.., STAGE>), the
//     inverses of the diagonal tiles sit in the tiles' own places (rinv_tile);
//   * the condensation runs in two column passes (condense_half), rollouts take two row passes (rollout<.., WG = 4>).
// Sums over rows are taken in another order than ipm_box's (reduce2 over 4 waves, two roles per thread): rounding-level differences.
template <int MSEL, int NSEL, int GX, int NST = 0, int J0SEL = 0>
__device__ __forceinline__ int ipm_box4(const QPDims &dfull, const QPConst &c, const QPDyn &dyn, const QPData &q, gptr work_base,
                                        Lds &L, int *iters_out, QPWork &wout, lapc::Launch &prof, int warm_mode = 0) {
    const bool warm = warm_mode != 0, poison = warm_mode == 2;
    int tid = SRH_TID;                                       // re-read at the top of every interior-point iteration (dev_la.h: SRH_TID)
    const int nt = blockDim.x;
    QPDims d = dfull;
    drop_trust_region_rows(d);
    QPWork w;
    qp_carve(w, work_base, d);
    wout = w;
    gptr gh = work_base + dfull.qc_off;
    const int N = d.N, m = d.m, nm = N * m, ldG = 16 * d.KT, NP = 2 * N, nz = d.nz;
    GPackT<NST, J0SEL> g{(cgptr)gh, (clptr)(L.Gt), d.lean_j0, m, NP};
    // the Gram fill's own pack: the stages >= gram_stage_j0 staged in the K-tile area (gram_t)
    const GPack gg{(cgptr)gh, (clptr)(L.B), gram_stage_j0(d), m, NP};
    Prof pf;
    lapc::Clock lp, split, front;                     // (declared here, re-armed where they start: an object in a nested scope moved two PHIs of the product kernel)
    if constexpr (lapc::ON) { if (tid < 15) L.Qu[tid] = 0.0; }       // (the lap mailbox; [15] is the serial wave's)
    // (printed by profile builds) Gram fills of this QP, its condensation (0 kept from the QP before, 1 general, 2 single-region) and the clocks of it
    lapc::Counters<3> qinfo;
    enum { NGRAM, COND_MODE, COND_CLK };
    if (warm) { for (int e = tid; e < nm; e += nt) L.u[e] = w.u[e]; }
    else { for (int e = tid; e < nm; e += nt) { w.u[e] = 0.0; L.u[e] = 0.0; } }
    for (int e = tid; e < ldG + L.ypad; e += nt) { L.ya[e] = 0.0; L.yd[e] = 0.0; L.yg[e] = 0.0; }     // padding stays zero for good
    for (int e = tid; e <= N; e += nt) w.s[e] = 0.0;
    for (int k = tid; k < N; k += nt) L.idxl[k] = dyn.idx ? dyn.idx[k] : k;
    if (tid < 5) L.flag[3 + tid] = 0;                          // counters of the two wave sets (Waves, tile_cholesky_set)
    __syncthreads();
    const bool reuse = same_regions(dyn, L, L.goffg, N, tid, nt);
    if (dyn.idx != nullptr) {
        __syncthreads();
        if (tid == 0) L.flag[3] = 0;                           // tile_cholesky_set's early-tile counter from here on
    }
    if (!reuse) {
        const bool single = single_region(d, c, dyn, L);
        rollout<MSEL, NSEL, false, 4>(d, dyn, q.x0, (cgptr) nullptr, w.x, L);
        lp.lap(prof, lapc::QP_SETUP);
        if (single) condense_single<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
        else condense_half<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
        // (behind the constant: the product build must not see a second `single ? 2 : 1` in front of the one below)
        if constexpr (lapc::ON) { qinfo.add(COND_MODE, single ? 2 : 1); qinfo.add(COND_CLK, lp.since()); }
        for (int k = tid; k < N; k += nt) L.goffg[k] = L.idxl[k];
        if (tid == 0) L.flag[2] = single ? 2 : 1;              // 2: the packed G is the expansion of L.gtoep (kept over the QPs that reuse it)
        __syncthreads();
    }
    const bool toep = __builtin_amdgcn_readfirstlane(L.flag[2]) == 2;
    g.gto = toep ? (cgptr)L.gtoep : (cgptr) nullptr;           // the products read the generators (3.2 KB) instead of the packed rows (82 KB)                         // (uniform: written before a barrier, by this QP or the one that condensed)
    if (warm) {                                               // y = y_free + G u
        __syncthreads();
        g_times<MSEL>(d, g, L, L.u, L.dy);
        for (int e = tid; e < ldG; e += nt) { L.y[e] = L.yfg[e] + L.dy[e]; }
        __syncthreads();
        for (int e = tid; e < ldG; e += nt) L.dy[e] = 0.0;
    } else {
        for (int e = tid; e < ldG; e += nt) { L.y[e] = L.yfg[e]; L.dy[e] = 0.0; }
    }
    __syncthreads();
    lp.lap(prof, lapc::QP_CONDENSE);
    // ---- this thread's rows: the two box rows of input `tid`, and one state-row slot
    const bool isu = tid < nm;
    const bool isx = tid < N * GX;
    const int ku = isu ? tid / m : 0, bu = isu ? tid - ku * m : 0;
    const int kx = isx ? tid / GX + 1 : 1, rx = isx ? tid - (kx - 1) * GX : 0;        // stage 1..N, row slot
    const int nrk = d.nX + (kx == N ? d.nXf : 0);
    const bool xrow = isx && rx < nrk;                                               // the slot holds a state row
    const bool xlead = isx && rx == 0;                                               // first lane of the stage group
    double cu[2] = {0.0, 0.0}, hu[2] = {0.0, 0.0}, cx[2] = {0.0, 0.0}, hx = 0.0;
    if (isu) {
        cu[0] = c.UA[(size_t)(2 * bu) * m + bu]; cu[1] = c.UA[(size_t)(2 * bu + 1) * m + bu];
        hu[0] = c.Ub[2 * bu]; hu[1] = c.Ub[2 * bu + 1];
    }
    if (xrow) {
        cgptr T = rx < d.nX ? c.Tx + (size_t)rx * 2 : c.Txf + (size_t)(rx - d.nX) * 2;
        cx[0] = T[0]; cx[1] = T[1];
        hx = rx < d.nX ? c.Xb[rx] : c.Xfb[rx - d.nX];
    }
    const double r2bb = isu ? c.R2[bu * m + bu] : 0.0;
    const double udv = (isu && q.ud) ? q.ud[(size_t)ku * m + bu] : 0.0;
    double gc0 = 0.0, gc1 = 0.0, s00 = 0.0, s01 = 0.0, s11 = 0.0;
    if (xlead) {
        cgptr S = (kx == N) ? c.ScN : c.Sc;
        s00 = S[0]; s01 = S[1]; s11 = S[3];
        if (q.z) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Cz2[b], q.z[(size_t)kx * nz + b], gc0); gc1 = fma(-c.Cz2[nz + b], q.z[(size_t)kx * nz + b], gc1); }
        if (kx == N && c.Qzf && q.zf) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Czf2[b], q.zf[b], gc0); gc1 = fma(-c.Czf2[nz + b], q.zf[b], gc1); }
    }
    const int lsu = 2 * tid, lsx = 2 * nm + (kx - 1) * (d.nX + d.nXf) + rx;           // this thread's rows in w.lam (layout of ipm_box)
    double tu[2] = {0.0, 0.0}, lu[2] = {0.0, 0.0}, gu[2] = {0.0, 0.0}, ru[2] = {0.0, 0.0}, dtu[2] = {0.0, 0.0}, dlu[2] = {0.0, 0.0};
    double txr = 0.0, lxr = 0.0, gxr = 0.0, rcx = 0.0, dtx = 0.0, dlx = 0.0;
    auto yval = [&](clptr vy) -> double { return fma(cx[1], vy[(kx - 1) * 2 + 1], cx[0] * vy[(kx - 1) * 2]); };
    int status = 1, it = 0;
    enum { INIT = 0, PRED = 1, CORR = 2 };
    int mode = INIT;
    double mu = 0.0, rp = 0.0, sig = 0.0, sd = 1.0, sp = 1.0, dreg = 0.0;
    bool near_opt = false;
    const bool ya_const = d.nX + d.nXf == 0;                  // no state rows: L.ya is the same in the predictor and the corrector (newton_front)
    auto scales = [&]() { qp::residual_scales(d, c, q, tid, nt, sd, sp, dreg, [&](double &a, double &b) { reduce2(a, 1, b, 1, L.red); }); };
    if (warm && d.ng > 0) {
        if (isu) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) ipm::start_warm(cu[s2] * L.u[tid] - hu[s2], [&] { return w.lam[lsu + s2]; }, poison, tu[s2], lu[s2]);
        }
        if (xrow) ipm::start_warm(yval(L.y) - hx, [&] { return w.lam[lsx]; }, poison, txr, lxr);
        scales();
        mode = PRED;
    }
    while (true) {
        tid = SRH_TID;
        lp.lap(prof, lapc::QP_STEPS);
        // ---------------- rows -> weights, gradient shifts, and their per-stage sums, all in place
        double musum = 0.0, rpm = 0.0;
        double Du[2] = {0.0, 0.0}, rhu[2] = {0.0, 0.0}, Dx = 0.0, rhx = 0.0;
        if (isu) {
            const double uv = L.u[tid];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                if (mode == INIT) ipm::init_row(cu[s2] * uv - hu[s2], 1.0, Du[s2], rhu[s2], lu[s2]);
                else if (mode == PRED) ipm::pred_row(cu[s2] * uv - hu[s2], tu[s2], lu[s2], dreg, gu[s2], Du[s2], rhu[s2], musum, rpm);
                else ipm::corr_row(tu[s2], lu[s2], gu[s2], dtu[s2], dlu[s2], sig, mu, dreg, ru[s2], rhu[s2]);
            }
        }
        if (xrow) {
            if (mode == INIT) ipm::init_row(yval(L.y) - hx, 1.0, Dx, rhx, lxr);
            else if (mode == PRED) ipm::pred_row(yval(L.y) - hx, txr, lxr, dreg, gxr, Dx, rhx, musum, rpm);
            else ipm::corr_row(txr, lxr, gxr, dtx, dlx, sig, mu, dreg, rcx, rhx);
        }
        if (isu) {
            const double du0 = r2bb * (L.u[tid] - udv);
            if (mode != CORR) {
                double v = fma(cu[0] * Du[0], cu[0], r2bb);
                v = fma(cu[1] * Du[1], cu[1], v);
                L.Ldi[tid] = 1.0 / sqrt(v);
            }
            L.ta[tid] = fma(cu[1], rhu[1], fma(cu[0], rhu[0], du0));
            if (mode == PRED) L.tb[tid] = fma(cu[1], lu[1], fma(cu[0], lu[0], du0));
        }
        if (isx) {                                           // whole stage groups: the DPP sums see every lane of a group
            const double y0 = L.y[(kx - 1) * 2], y1 = L.y[(kx - 1) * 2 + 1];
            if (mode != CORR) {
                const double a00 = gsum<GX>(cx[0] * Dx * cx[0]), a01 = gsum<GX>(cx[0] * Dx * cx[1]), a11 = gsum<GX>(cx[1] * Dx * cx[1]);
                if (xlead) chol2_psd(s00 + a00, s01 + a01, s11 + a11, L.Ls + (size_t)(kx - 1) * 4);
            }
            const double r0 = gsum<GX>(cx[0] * rhx), r1 = gsum<GX>(cx[1] * rhx);
            double l0 = 0.0, l1 = 0.0;
            if (mode == PRED) { l0 = gsum<GX>(cx[0] * (xrow ? lxr : 0.0)); l1 = gsum<GX>(cx[1] * (xrow ? lxr : 0.0)); }
            if (xlead) {
                const double c0 = fma(s01, y1, s00 * y0) + gc0, c1 = fma(s11, y1, s01 * y0) + gc1;
                L.ya[(kx - 1) * 2] = c0 + r0; L.ya[(kx - 1) * 2 + 1] = c1 + r1;
                if (mode == PRED) { L.yg[(kx - 1) * 2] = c0 + l0; L.yg[(kx - 1) * 2 + 1] = c1 + l1; }
            }
        }
        if (mode == PRED) {
            reduce2(musum, 0, rpm, 1, L.red);
            mu = musum / d.ng;
            rp = rpm;
        }
        __syncthreads();
        lp.lap(prof, lapc::QP_ROWS);
        // ---------------- converged already?  Then no system (converged_early; 16: the rows per pass of the front's two waves)
        if (mode == PRED) {
            double rde;                                        // (not rd: nothing of the early test stays live through the system)
            const int early = converged_early<MSEL, 16>(d, g, L, mu, rp, sd, sp, rde);
            if (early != EARLY_NO_GATE) { lp.lap(prof, lapc::EARLY_TEST); if (early == EARLY_GO_ON) prof.add(lapc::N_EARLY_FOR_NOTHING); }      // the early product's own lap; products paid for nothing
            if (early == EARLY_STOP) { status = 0; break; }
        }
        // ---------------- Newton system
        double rd = 0.0;
        bool ok = true;
        if (mode != CORR) {
            gram_t<MSEL, true>(d, c, gg, L, (cgptr)gh, toep ? (cgptr)L.gtoep : (cgptr) nullptr);
            lp.lap(prof, lapc::QP_GRAM);
            qinfo.add(NGRAM);
            // the factorisation (waves 0-1: a chain of one-wave 16 x 16 factorisations) beside the half of the Newton solve that
            // does not need the factor (waves 2-3), see Waves.  Under a row roster (QPDims::lean_roster, roster_nwk) waves 2 and 3 are
            // workers 1 and 2 of the factorisation as well, in the rows behind (code > 0) or in front of (code < 0) their Newton front:
            // the front touches no K tile and synchronises on L.flag[4] between its two waves only, so both orders are legal.
            // (wave indices after the ^ sw of the serial wave; every branch below is on a value uniform over the wave)
            const clptr gyd = mode == PRED ? (clptr)L.yg : (clptr) nullptr;
            const int sw = serial_wave(L);
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6) ^ sw;
            const int rc = __builtin_amdgcn_readfirstlane(d.lean_roster);
            auto W = half_waves(L.flag + 4, sw);
            pf.restart();
            split.restart();
            if (wv == 0) {
                tile_cholesky_set(d, L, 0, tid & 63, 1, L.flag + 5, L.flag + 3, rc);
                if constexpr (lapc::ON) { if ((tid & 63) == 0) L.Qu[lapc::MAIL_SPLIT_FACTOR] = (double)split.since(); }          // the chain, up to its last signal
            } else {
                const bool has_front = wv >= 2, rows_first = wv == 1 || rc < 0, has_rows = wv == 1 || rc != 0;
#pragma unroll 1
                for (int ph = 0; ph < 2; ++ph) {
                    if ((ph == 0) == rows_first) {
                        if (has_rows) tile_cholesky_set(d, L, wv, tid & 63, 1, L.flag + 5, L.flag + 3, rc);
                    } else if (has_front) {
                        front.restart();
                        pf.restart(front);
                        newton_front<MSEL, true>(d, g, L, gyd, W, pf, ya_const && mode == PRED);
                        if constexpr (lapc::ON) { if (W.tid == 0) L.Qu[lapc::MAIL_SPLIT_FRONT] = (double)front.since(); }       // the front alone, on its two waves
                    }
                }
            }
            __syncthreads();
            if constexpr (lapc::ON) split_mail_fold(L, prof);
            ok = L.flag[1] != 0;
            if (tid < 5) L.flag[3 + tid] = 0;
            if (gyd) rd = L.Qu[0];
            lp.lap(prof, lapc::QP_CHOLESKY);
            if (ok) unit_tiles(d, L);
            lp.lap(prof, lapc::UNIT_TILES);                                        // (unit_tiles and its barrier alone; the factorisation up to the join is lap 5)
            pf.restart();
            if (ok) newton_back<MSEL>(d, g, L, pf);
        } else {
            pf.restart();
            newton_solve<MSEL>(d, g, L, (clptr) nullptr, &rd, pf, ya_const);
        }
        lp.lap(prof, lapc::QP_NEWTON);
        // ---------------- use the direction
        if (mode == INIT) {
            if (ipm::stops(ipm::verdict_system(ok), status)) break;
            for (int e = tid; e < nm; e += nt) L.u[e] += L.du[e];
            for (int e = tid; e < ldG; e += nt) L.y[e] += L.dy[e];
            __syncthreads();
            if (ipm::stops(ipm::verdict_no_rows(d.ng), status)) break;
            double zmin = INFINITY, zmax = -INFINITY;
            if (isu) {
                const double uv = L.u[tid];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) { gu[s2] = cu[s2] * uv - hu[s2]; zmin = fmin(zmin, gu[s2]); zmax = fmax(zmax, gu[s2]); }
            }
            if (xrow) { gxr = yval(L.y) - hx; zmin = fmin(zmin, gxr); zmax = fmax(zmax, gxr); }
            reduce2(zmin, 2, zmax, 1, L.red);
            const ipm::Shift sh = ipm::start_shift(zmin, zmax);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) ipm::start_cold(gu[s2], sh, tu[s2], lu[s2]);
            ipm::start_cold(gxr, sh, txr, lxr);
            scales();
            mode = PRED;
            continue;
        }
        double amax = 1e300, dummy = 0.0;
        if (ok) {
            if (isu) {
                const double duv = L.du[tid];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    ipm::direction(mode == PRED, tu[s2], lu[s2], gu[s2], ru[s2], cu[s2] * duv, dreg, dlu[s2], dtu[s2]);
                    ipm::step_bound(tu[s2], lu[s2], dtu[s2], dlu[s2], amax);
                }
            }
            if (xrow) {
                ipm::direction(mode == PRED, txr, lxr, gxr, rcx, yval(L.dy), dreg, dlx, dtx);
                ipm::step_bound(txr, lxr, dtx, dlx, amax);
            }
        }
        reduce2(amax, 2, dummy, 0, L.red);
        if (mode == PRED) {
            if (ipm::stops(ipm::verdict(ok, mu, rd, rp, sd, sp, d.tol, it, d.max_iter, near_opt), status)) break;
            const double a_aff = ipm::step_affine(amax);
            double ma = 0.0;
            if (isu) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) ma += ipm::affine_term(tu[s2], lu[s2], dtu[s2], dlu[s2], a_aff);
            }
            if (xrow) ma += ipm::affine_term(txr, lxr, dtx, dlx, a_aff);
            reduce2(ma, 0, dummy, 0, L.red);
            const double mu_aff = ma / d.ng;
            sig = ipm::centring(mu_aff, mu);
            mode = CORR;
            continue;
        }
        if (ipm::stops(ipm::verdict_system(ok), status)) break;
        const double a = ipm::step_length(amax);
        for (int e = tid; e < nm; e += nt) L.u[e] += a * L.du[e];
        for (int e = tid; e < ldG; e += nt) L.y[e] += a * L.dy[e];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) ipm::advance(a, dtu[s2], dlu[s2], tu[s2], lu[s2]);
        ipm::advance(a, dtx, dlx, txr, lxr);
        __syncthreads();
        ++it;
        mode = PRED;
    }
    __syncthreads();
    for (int e = tid; e < nm; e += nt) w.u[e] = L.u[e];
    if (status == 0) {                                        // what the next QP of this solve starts from (warm)
        if (isu) { w.lam[lsu] = lu[0]; w.lam[lsu + 1] = lu[1]; }
        if (xrow) w.lam[lsx] = lxr;
    }
    __syncthreads();
    pf.fold(prof, it, warm);
    if constexpr (lapc::ON) {
        if (tid == 0 && blockIdx.x == 0) {
            printf("lean condense (this QP): mode %d clocks %lld interior-point iterations %d status %d\n", (int)qinfo[COND_MODE], qinfo[COND_CLK], it, status);
            printf("lean gram laps (this QP, wave 0, %d fills): 1/D+staging+barrier %.0f descriptors %.0f products %.0f epilogue A %.0f barrier %.0f store+barrier %.0f\n",
                   (int)qinfo[NGRAM], L.Qu[lapc::MAIL_GRAM], L.Qu[lapc::MAIL_GRAM + 1], L.Qu[lapc::MAIL_GRAM + 2], L.Qu[lapc::MAIL_GRAM + 3], L.Qu[lapc::MAIL_GRAM_BARRIER], L.Qu[lapc::MAIL_GRAM_STORE]);
            print_gram_wave_laps(4);
        }
    }
    if (iters_out) *iters_out = it;
    return status;
}

// ------------------------------------------------------------------ short horizons: the interior point on ONE wave
// The reference's closed-loop drivers replan N = 5 (examples/diamond/diamond.py:309-316) and N = 3 (examples/hardware/diamond.py:
// 393-399): N p_o <= 16 outputs -- K is ONE 16 x 16 tile -- and N n_u <= 64 inputs.  ipm_box() spends ~80 k clocks per interior-point
// iteration on such a problem (profiles/r05_lean_phase_clocks.json: N = 5) although nothing in it is larger than a tile: some 35
// workgroup barriers, each with seven waves that have nothing to do.  Here the iteration runs on wave 0 alone, without a single
// workgroup barrier (the other waves wait at the one behind it):
//   * lane e < N m owns input e = (stage, input): its value, its two box rows and their slacks / multipliers, its row of G^T
//     (16 registers) -- G^T y is a lane-local dot product with the 16 broadcast entries of y;
//   * lane l < N GX also owns a state-row slot (stage, slot) like the state-row threads of ipm_box (per-stage sums by DPP);
//   * lane (i, kk) of 16 x 4 holds G in the MFMA layout G^T[4 s + kk][i], s < N m / 4: G u = one FMA per k-step + the sum over kk,
//     and Ky = G D^-1 G^T is N m / 4 MFMA instructions whose A and B operands are THE SAME registers;
//   * y-space vectors live in LDS (16 entries), exchanged under a wave-level fence (the LDS queue of a wave is in order).
// Same iteration as ipm_box (same starting points, weights, stopping rule, warm start): sums in another order, rounding-level
// differences.  Requirements (lean_matches): KT == 1, N m <= 64, N GX <= 64, the whole packed G in LDS (lean_j0 == 0).
// what one wave needs between an LDS write and the read of it by another lane: nothing from the hardware (the LDS queue of a
// wave is in order), only that the compiler keeps the accesses on their sides -- a wavefront-scope fence waits for no counter
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MSEL, int NSEL, int GX>
__device__ __forceinline__ int ipm_wave(const QPDims &dfull, const QPConst &c, const QPDyn &dyn, const QPData &q, gptr work_base,
                                        Lds &L, int *iters_out, QPWork &wout, lapc::Launch &prof, int warm_mode = 0) {
    static_assert(MSEL == 4 || MSEL == 8, "one-wave interior point: n_u = 4 or 8");
    const bool warm = warm_mode != 0, poison = warm_mode == 2;
    int tid = SRH_TID;                                       // re-read at the top of every interior-point iteration (dev_la.h: SRH_TID)
    const int nt = blockDim.x;
    QPDims d = dfull;
    drop_trust_region_rows(d);
    QPWork w;
    qp_carve(w, work_base, d);
    wout = w;
    gptr gh = work_base + dfull.qc_off;
    constexpr int M = MSEL, SMAX = 2 * M;                      // k-steps of a product with G: N m / 4 <= 8 m / 4 (N <= 8)
    const int N = d.N, nm = N * M, ldG = 16, NP = 2 * N, nz = d.nz;
    lapc::Clock lp;
    // ---- the preamble of ipm_box: starting point, condensation (all waves)
    if (warm) { for (int e = tid; e < nm; e += nt) L.u[e] = w.u[e]; }
    else { for (int e = tid; e < nm; e += nt) { w.u[e] = 0.0; L.u[e] = 0.0; } }
    for (int e = tid; e < ldG + YPAD; e += nt) { L.ya[e] = 0.0; L.yd[e] = 0.0; L.yg[e] = 0.0; }
    for (int e = tid; e <= N; e += nt) w.s[e] = 0.0;
    for (int k = tid; k < N; k += nt) L.idxl[k] = dyn.idx ? dyn.idx[k] : k;
    __syncthreads();
    const bool reuse = same_regions(dyn, L, L.goff, N, tid, nt);
    if (!reuse) {
        rollout<MSEL, NSEL>(d, dyn, q.x0, (cgptr) nullptr, w.x, L);
        lp.lap(prof, lapc::QP_SETUP);
        condense<MSEL, NSEL>(d, c, dyn, w.x, gh, L);
        for (int k = tid; k < N; k += nt) L.goff[k] = L.idxl[k];
        if (tid == 0) L.flag[2] = 1;
    }
    __syncthreads();
    lp.lap(prof, lapc::QP_CONDENSE);
    int status = 1, it = 0;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave == 0) {
        int lane = tid, i16 = lane & 15, kk = lane >> 4;          // re-derived at the top of every iteration (SRH_TID)
        const int S = nm >> 2;                                     // k-steps of the products with G (n_u is a multiple of 4)
        // ---- G in registers, twice: by input row (gR) and in the MFMA operand layout (gM)
        const bool isu = lane < nm;
        const int ku = isu ? lane / M : 0, bu = isu ? lane - ku * M : 0;
        auto g_at = [&](int e, int i) -> double {                 // G^T[e][i] from the packed rows (structural zeros: i < 2 j)
            const int j = e / M, b = e - j * M;
            return (i >= 2 * j && i < NP) ? L.Gt[goff(j, M, NP) + b * (NP - 2 * j) + (i - 2 * j)] : 0.0;
        };
        double gR[16], gM[SMAX];
#pragma unroll
        for (int i = 0; i < 16; ++i) gR[i] = isu ? g_at(lane, i) : 0.0;
#pragma unroll
        for (int s2 = 0; s2 < SMAX; ++s2) gM[s2] = s2 < S ? g_at(4 * s2 + kk, i16) : 0.0;
        // ---- this lane's rows: the two box rows of input `lane`, and one state-row slot
        const bool isx = lane < N * GX;
        const int kx = isx ? lane / GX + 1 : 1, rx = isx ? lane - (kx - 1) * GX : 0;
        const int nrk = d.nX + (kx == N ? d.nXf : 0);
        const bool xrow = isx && rx < nrk, xlead = isx && rx == 0;
        double cu[2] = {0.0, 0.0}, hu[2] = {0.0, 0.0}, cx[2] = {0.0, 0.0}, hx = 0.0;
        if (isu) {
            cu[0] = c.UA[(size_t)(2 * bu) * M + bu]; cu[1] = c.UA[(size_t)(2 * bu + 1) * M + bu];
            hu[0] = c.Ub[2 * bu]; hu[1] = c.Ub[2 * bu + 1];
        }
        if (xrow) {
            cgptr T = rx < d.nX ? c.Tx + (size_t)rx * 2 : c.Txf + (size_t)(rx - d.nX) * 2;
            cx[0] = T[0]; cx[1] = T[1];
            hx = rx < d.nX ? c.Xb[rx] : c.Xfb[rx - d.nX];
        }
        const double r2bb = isu ? c.R2[bu * M + bu] : 0.0;
        const double udv = (isu && q.ud) ? q.ud[(size_t)ku * M + bu] : 0.0;
        double gc0 = 0.0, gc1 = 0.0, s00 = 0.0, s01 = 0.0, s11 = 0.0;
        if (xlead) {
            cgptr Sm = (kx == N) ? c.ScN : c.Sc;
            s00 = Sm[0]; s01 = Sm[1]; s11 = Sm[3];
            if (q.z) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Cz2[b], q.z[(size_t)kx * nz + b], gc0); gc1 = fma(-c.Cz2[nz + b], q.z[(size_t)kx * nz + b], gc1); }
            if (kx == N && c.Qzf && q.zf) for (int b = 0; b < nz; ++b) { gc0 = fma(-c.Czf2[b], q.zf[b], gc0); gc1 = fma(-c.Czf2[nz + b], q.zf[b], gc1); }
        }
        const int lsu = 2 * lane, lsx = 2 * nm + (kx - 1) * (d.nX + d.nXf) + rx;           // this lane's rows in w.lam (layout of ipm_box)
        double u_r = isu ? L.u[lane] : 0.0, du_r = 0.0, ldi = 0.0, w2 = 0.0, ta_r = 0.0, tb_r = 0.0;
        double tu[2] = {0.0, 0.0}, lu[2] = {0.0, 0.0}, gu[2] = {0.0, 0.0}, ru[2] = {0.0, 0.0}, dtu[2] = {0.0, 0.0}, dlu[2] = {0.0, 0.0};
        double tx = 0.0, lx = 0.0, gx = 0.0, rcx = 0.0, dtx = 0.0, dlx = 0.0;
        // y = y_free (+ G u when warm), dy = 0: lanes (i, kk) with the sum over kk
        auto g_times_w = [&](clptr uv) -> double {              // (G uv)[i16] on every lane; uv: N m entries of LDS
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < SMAX; s2 += 2) {
                if (s2 < S) a0 = fma(gM[s2], uv[4 * s2 + kk], a0);
                if (s2 + 1 < S) a1 = fma(gM[s2 + 1], uv[4 * (s2 + 1) + kk], a1);
            }
            double a = a0 + a1;
            a += __shfl_xor(a, 16, 64);
            a += __shfl_xor(a, 32, 64);
            return a;
        };
        {
            double y0 = L.yf[i16];
            if (warm) y0 += g_times_w(L.u);
            if (lane < 16) { L.y[lane] = lane < NP ? y0 : 0.0; L.dy[lane] = 0.0; }
        }
        wave_fence();
        auto yval = [&](clptr vy) -> double { return fma(cx[1], vy[(kx - 1) * 2 + 1], cx[0] * vy[(kx - 1) * 2]); };
        enum { INIT = 0, PRED = 1, CORR = 2 };
        int mode = INIT;
        double mu = 0.0, rp = 0.0, sig = 0.0, sd = 1.0, sp = 1.0, dreg = 0.0;
        bool near_opt = false;
        auto scales = [&]() { qp::residual_scales(d, c, q, lane, 64, sd, sp, dreg, [](double &a, double &b) { a = wg::wave_max(a); b = wg::wave_max(b); }); };
        if (warm && d.ng > 0) {
            if (isu) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) ipm::start_warm(cu[s2] * u_r - hu[s2], [&] { return w.lam[lsu + s2]; }, poison, tu[s2], lu[s2]);
            }
            if (xrow) ipm::start_warm(yval(L.y) - hx, [&] { return w.lam[lsx]; }, poison, tx, lx);
            scales();
            mode = PRED;
        }
        while (true) {
            tid = SRH_TID; lane = tid; i16 = lane & 15; kk = lane >> 4;
            // ---------------- rows -> weights, gradient shifts, per-stage sums
            double musum = 0.0, rpm = 0.0;
            double Du[2] = {0.0, 0.0}, rhu[2] = {0.0, 0.0}, Dx = 0.0, rhx = 0.0;
            if (isu) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    if (mode == INIT) ipm::init_row(cu[s2] * u_r - hu[s2], 1.0, Du[s2], rhu[s2], lu[s2]);
                    else if (mode == PRED) ipm::pred_row(cu[s2] * u_r - hu[s2], tu[s2], lu[s2], dreg, gu[s2], Du[s2], rhu[s2], musum, rpm);
                    else ipm::corr_row(tu[s2], lu[s2], gu[s2], dtu[s2], dlu[s2], sig, mu, dreg, ru[s2], rhu[s2]);
                }
                const double du0 = r2bb * (u_r - udv);
                if (mode != CORR) {
                    double v = fma(cu[0] * Du[0], cu[0], r2bb);
                    v = fma(cu[1] * Du[1], cu[1], v);
                    ldi = 1.0 / sqrt(v);
                    w2 = ldi * ldi;
                    L.tc[lane] = w2;                             // for the A operands of the Gram product
                }
                ta_r = fma(cu[1], rhu[1], fma(cu[0], rhu[0], du0));
                if (mode == PRED) tb_r = fma(cu[1], lu[1], fma(cu[0], lu[0], du0));
            }
            if (xrow) {
                if (mode == INIT) ipm::init_row(yval(L.y) - hx, 1.0, Dx, rhx, lx);
                else if (mode == PRED) ipm::pred_row(yval(L.y) - hx, tx, lx, dreg, gx, Dx, rhx, musum, rpm);
                else ipm::corr_row(tx, lx, gx, dtx, dlx, sig, mu, dreg, rcx, rhx);
            }
            {   // whole stage groups (every lane executes the DPP sums; lanes without a row contribute zeros)
                const double y0 = isx ? L.y[(kx - 1) * 2] : 0.0, y1 = isx ? L.y[(kx - 1) * 2 + 1] : 0.0;
                if (mode != CORR) {
                    const double a00 = gsum<GX>(cx[0] * Dx * cx[0]), a01 = gsum<GX>(cx[0] * Dx * cx[1]), a11 = gsum<GX>(cx[1] * Dx * cx[1]);
                    if (xlead) chol2_psd(s00 + a00, s01 + a01, s11 + a11, L.Ls + (size_t)(kx - 1) * 4);
                }
                const double r0 = gsum<GX>(cx[0] * rhx), r1 = gsum<GX>(cx[1] * rhx);
                double l0 = 0.0, l1 = 0.0;
                if (mode == PRED) { l0 = gsum<GX>(cx[0] * lx); l1 = gsum<GX>(cx[1] * lx); }
                if (xlead) {
                    const double c0 = fma(s01, y1, s00 * y0) + gc0, c1 = fma(s11, y1, s01 * y0) + gc1;
                    L.ya[(kx - 1) * 2] = c0 + r0; L.ya[(kx - 1) * 2 + 1] = c1 + r1;
                    if (mode == PRED) { L.yg[(kx - 1) * 2] = c0 + l0; L.yg[(kx - 1) * 2 + 1] = c1 + l1; }
                }
            }
            if (mode == PRED) {
                mu = wg::wave_sum(musum) / d.ng;
                rp = wg::wave_max(rpm);
            }
            wave_fence();
            // ---------------- converged already?  Then no system (ipm_rule.h, PRED; converged_early): the dual residual by the very
            // product and maximum of the Newton direction below
            if (mode == PRED && !d.ipm_late_stop && ipm::may_converge(mu, rp, sp, d.tol)) {
                double gtd = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) gtd = fma(gR[i], L.yg[i], gtd);
                const double rde = wg::wave_max(isu ? fabs(tb_r + gtd) : 0.0);
                if (ipm::converged(mu, rde, rp, sd, sp, d.tol)) {
                    if (q.dbg && lane == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rde; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
                    status = 0;
                    break;
                }
            }
            // ---------------- K = I + Ls^T (G D^-1 G^T) Ls, scaled to a unit diagonal, and its factor (one tile)
            bool ok = true;
            if (mode != CORR) {
                wg::qp_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s2 = 0; s2 < SMAX; ++s2)
                    if (s2 < S) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gM[s2] * L.tc[4 * s2 + kk], gM[s2], acc, 0, 0, 0);
                const int kb = min(i16 >> 1, N - 1), bc = i16 & 1;
                clptr Lb = L.Ls + (size_t)kb * 4;
                const double cb_own = bc == 0 ? Lb[0] : Lb[3], cb_oth = bc == 0 ? Lb[2] : 0.0;
                double kv[4];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int r = kk + 4 * qd, ka = min(r >> 1, N - 1), ar = r & 1;
                    clptr La = L.Ls + (size_t)ka * 4;
                    double v = (r < NP && i16 < NP) ? acc[qd] : 0.0;
                    const double vp = wg::dpp_mov<0xB1>(v);
                    v = fma(vp, cb_oth, v * cb_own);
                    const double vr = wg::xor16(v);
                    v = ar == 0 ? fma(La[2], vr, La[0] * v) : La[3] * v;
                    const bool dg = r == i16;
                    v += dg ? 1.0 : 0.0;
                    const double ri = qpc::rsq3(dg ? v : 1.0);
                    if (dg) L.ks[r] = ri;
                    kv[qd] = v;
                }
                wave_fence();
                const double sc = L.ks[i16];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) { const int r = kk + 4 * qd; L.B[r * TS + i16] = kv[qd] * (L.ks[r] * sc); }
                wave_fence();
                // (the padding rows / columns of a short horizon are the identity: only the leading N p_o pivots do anything)
                ok = NP <= 6 ? qpc::chol16<false, 6>(L.B, L.Rinv) : (NP <= 10 ? qpc::chol16<false, 10>(L.B, L.Rinv) : qpc::chol16<false>(L.B, L.Rinv));
                wave_fence();
            }
            // ---------------- Newton direction
            double rd = 0.0;
            if (ok) {
                double gty = 0.0, gtd = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) gty = fma(gR[i], L.ya[i], gty);
                if (mode == PRED) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) gtd = fma(gR[i], L.yg[i], gtd);
                    rd = wg::wave_max(isu ? fabs(tb_r + gtd) : 0.0);
                }
                const double tt = -(ta_r + gty) * w2;
                if (isu) L.ta[lane] = tt;
                wave_fence();
                const double yb = g_times_w(L.ta);
                {   // yc = ks Ls^T yb per output stage
                    const double yo = wg::dpp_mov<0xB1>(yb);
                    const int k = i16 >> 1;
                    double o = 0.0;
                    if (k < N) {
                        clptr Lk = L.Ls + (size_t)k * 4;
                        o = (i16 & 1) == 0 ? fma(Lk[2], yo, Lk[0] * yb) * L.ks[i16] : Lk[3] * yb * L.ks[i16];
                    }
                    if (lane < 16) L.yc[lane] = o;
                }
                wave_fence();
                {   // v = K^-1 yc = Rinv (Rinv^T yc)   (k_solve_unit, one tile)
                    const int cc = lane >> 2, part = lane & 3;
                    double t = 0.0;
#pragma unroll
                    for (int kq = 0; kq < 4; ++kq) t = fma(L.Rinv[(4 * part + kq) * TS + cc], L.yc[4 * part + kq], t);
                    t = wg::group_sum<4>(t);
                    wave_fence();
                    if (part == 0) L.yc[cc] = t;
                    wave_fence();
                    double wv = 0.0;
#pragma unroll
                    for (int kq = 0; kq < 4; ++kq) wv = fma(L.Rinv[cc * TS + 4 * part + kq], L.yc[4 * part + kq], wv);
                    wv = wg::group_sum<4>(wv);
                    wave_fence();
                    if (part == 0) L.yc[cc] = wv;
                    wave_fence();
                }
                if (lane < 8) {                                   // yd = Ls (ks v), dy = Ls^-T (ks v) per output stage
                    const int k = lane;
                    double o0 = 0.0, o1 = 0.0, e0 = 0.0, e1 = 0.0;
                    if (k < N) {
                        clptr Lk = L.Ls + (size_t)k * 4;
                        const double v0 = L.yc[2 * k] * L.ks[2 * k], v1 = L.yc[2 * k + 1] * L.ks[2 * k + 1];
                        o0 = Lk[0] * v0;
                        o1 = fma(Lk[3], v1, Lk[2] * v0);
                        e1 = v1 / Lk[3];
                        e0 = fma(-Lk[2], e1, v0) / Lk[0];
                    }
                    L.yd[2 * k] = o0; L.yd[2 * k + 1] = o1;
                    if (d.ls_pd) { L.dy[2 * k] = e0; L.dy[2 * k + 1] = e1; }
                }
                wave_fence();
                double gyd = 0.0;
#pragma unroll
                for (int i = 0; i < 16; ++i) gyd = fma(gR[i], L.yd[i], gyd);
                du_r = tt - gyd * w2;
                if (!d.ls_pd) {                                   // dy = G du
                    if (isu) L.ta[lane] = du_r;
                    wave_fence();
                    const double dyv = g_times_w(L.ta);
                    if (lane < 16) L.dy[lane] = lane < NP ? dyv : 0.0;
                    wave_fence();
                }
            }
            // ---------------- use the direction
            if (mode == INIT) {
                if (ipm::stops(ipm::verdict_system(ok), status)) break;
                u_r += du_r;
                if (lane < 16) L.y[lane] += L.dy[lane];
                wave_fence();
                if (ipm::stops(ipm::verdict_no_rows(d.ng), status)) break;
                double zmin = INFINITY, zmax = -INFINITY;
                if (isu) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) { gu[s2] = cu[s2] * u_r - hu[s2]; zmin = fmin(zmin, gu[s2]); zmax = fmax(zmax, gu[s2]); }
                }
                if (xrow) { gx = yval(L.y) - hx; zmin = fmin(zmin, gx); zmax = fmax(zmax, gx); }
                zmin = wg::wave_min(zmin); zmax = wg::wave_max(zmax);
                const ipm::Shift sh = ipm::start_shift(zmin, zmax);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) ipm::start_cold(gu[s2], sh, tu[s2], lu[s2]);
                ipm::start_cold(gx, sh, tx, lx);
                scales();
                mode = PRED;
                continue;
            }
            double amax = 1e300;
            if (ok) {
                if (isu) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        ipm::direction(mode == PRED, tu[s2], lu[s2], gu[s2], ru[s2], cu[s2] * du_r, dreg, dlu[s2], dtu[s2]);
                        ipm::step_bound(tu[s2], lu[s2], dtu[s2], dlu[s2], amax);
                    }
                }
                if (xrow) {
                    ipm::direction(mode == PRED, tx, lx, gx, rcx, yval(L.dy), dreg, dlx, dtx);
                    ipm::step_bound(tx, lx, dtx, dlx, amax);
                }
            }
            amax = wg::wave_min(amax);
            if (mode == PRED) {
                if (ipm::stops(ipm::verdict_failed(ok, mu, rd, near_opt), status)) break;
                if (q.dbg && lane == 0) { gptr gd = q.dbg + 8 * it; gd[0] = mu; gd[1] = rd; gd[2] = rp; gd[3] = sd; gd[4] = sp; }
                if (ipm::stops(ipm::verdict_converged(mu, rd, rp, sd, sp, d.tol, it, d.max_iter, near_opt), status)) break;
                const double a_aff = ipm::step_affine(amax);
                double ma = 0.0;
                if (isu) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) ma += ipm::affine_term(tu[s2], lu[s2], dtu[s2], dlu[s2], a_aff);
                }
                if (xrow) ma += ipm::affine_term(tx, lx, dtx, dlx, a_aff);
                const double mu_aff = wg::wave_sum(ma) / d.ng;
                sig = ipm::centring(mu_aff, mu);
                if (q.dbg && lane == 0) { gptr gd = q.dbg + 8 * it; gd[5] = a_aff; gd[6] = sig; }
                mode = CORR;
                continue;
            }
            if (ipm::stops(ipm::verdict_system(ok), status)) break;
            const double a = ipm::step_length(amax);
            if (q.dbg && lane == 0) { gptr gd = q.dbg + 8 * it; gd[7] = a; }
            u_r += a * du_r;
            if (lane < 16) L.y[lane] += a * L.dy[lane];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) ipm::advance(a, dtu[s2], dlu[s2], tu[s2], lu[s2]);
            ipm::advance(a, dtx, dlx, tx, lx);
            wave_fence();
            ++it;
            mode = PRED;
        }
        // ---- results: the minimiser, and (converged) the multipliers the next QP of this solve starts from
        if (isu) {
            w.u[lane] = u_r;
            if (status == 0) { w.lam[lsu] = lu[0]; w.lam[lsu + 1] = lu[1]; }
        }
        if (xrow && status == 0) w.lam[lsx] = lx;
        if (lane == 0) { L.red[0] = (double)status; L.red[1] = (double)it; }
    }
    __syncthreads();
    status = (int)L.red[0];
    it = (int)L.red[1];
    __syncthreads();
    lp.lap(prof, lapc::QP_NEWTON);
    prof.count_qp(it, warm);
    if (iters_out) *iters_out = it;
    return status;
}

// Objective of the minimiser (qp::objective, locp.py:218-263): e = H x - z by one thread per (stage, output) -- 60 products each --
// instead of one thread walking the n_z n_x = 360 products of its stage (28 k clocks per QP whatever the horizon:
// profiles/r05_lean_phase_clocks.json), then one thread per stage for the small quadratic forms: the same sums in the same order.
// Round 5: x may be the LDS copy the rollout left (XP = clptr), and the output matrix goes through LDS as well (hs: n_z n_x doubles
// behind that copy): a thread's 60 products then read LDS only -- from global memory they were 60 loads issued one product at a time.
template <typename XP>
__device__ __forceinline__ double objective_par(const QPDims &d, const QPConst &c, const QPData &q, XP x, cgptr u, cgptr s, gptr ez, QPLds &L, bool hl = false, lptr hs = nullptr) {
    const int n = d.n, nz = d.nz, m = d.m, N = d.N;
    // hl: objective_lds_doubles(d) doubles of LDS at hs: the output matrix, the weights Qz / Qzf / R and the output errors -- the second
    // phase's n_z^2 + n_u^2 products then read LDS as well (from global memory: one dependent load per product on a handful of threads)
    lptr Hl = hs, Qzl = Hl + (size_t)nz * n, Qfl = Qzl + nz * nz, Rl = Qfl + nz * nz, ezl = Rl + m * m;
    if (hl) {
        for (int e = SRH_TID; e < nz * n; e += blockDim.x) Hl[e] = c.H[e];
        for (int e = SRH_TID; e < nz * nz; e += blockDim.x) { Qzl[e] = c.Qz[e]; Qfl[e] = c.Qzf ? c.Qzf[e] : 0.0; }
        for (int e = SRH_TID; e < m * m; e += blockDim.x) Rl[e] = c.R[e];
        __syncthreads();
    }
    for (int e = SRH_TID; e < (N + 1) * nz; e += blockDim.x) {
        const int k = e / nz, a = e - k * nz;
        double v = q.z ? -q.z[e] : 0.0;
        if (hl) {
#pragma unroll 12
            for (int j = 0; j < n; ++j) v = fma(Hl[a * n + j], x[(size_t)k * n + j], v);       // (twelve products' reads in flight: a thread walks 60 of them)
        } else {
#pragma unroll 12
            for (int j = 0; j < n; ++j) v = fma(c.H[a * n + j], x[(size_t)k * n + j], v);
        }
        ez[e] = v;
        if (hl) ezl[e] = v;
    }
    __syncthreads();
    double acc = 0.0;
    for (int k = SRH_TID; k <= N; k += blockDim.x) {
        double e[16];
        if (hl) { for (int a = 0; a < nz; ++a) e[a] = ezl[(size_t)k * nz + a]; }
        else { for (int a = 0; a < nz; ++a) e[a] = ez[(size_t)k * nz + a]; }
        for (int a = 0; a < nz; ++a)
            for (int b = 0; b < nz; ++b) acc = fma(e[a] * (hl ? (double)Qzl[a * nz + b] : (double)c.Qz[a * nz + b]), e[b], acc);
        if (k == N && c.Qzf) {
            for (int a = 0; a < nz; ++a) e[a] += (q.z ? q.z[(size_t)k * nz + a] : 0.0) - (q.zf ? q.zf[a] : 0.0);
            for (int a = 0; a < nz; ++a)
                for (int b = 0; b < nz; ++b) acc = fma(e[a] * (hl ? (double)Qfl[a * nz + b] : (double)c.Qzf[a * nz + b]), e[b], acc);
        }
        if (k < N) {
            double ue[16];
            for (int a = 0; a < m; ++a) ue[a] = u[(size_t)k * m + a] - (q.ud ? q.ud[(size_t)k * m + a] : 0.0);
            for (int a = 0; a < m; ++a)
                for (int b = 0; b < m; ++b) acc = fma(ue[a] * (hl ? (double)Rl[a * m + b] : (double)c.R[a * m + b]), ue[b], acc);
        }
        if (d.tr) acc += q.omega * s[k];
    }
    return wg::reduce(acc, 0, L.red);
}
__host__ __device__ inline size_t objective_lds_doubles(const QPDims &d) { return (size_t)d.nz * d.n + 2 * (size_t)d.nz * d.nz + (size_t)d.m * d.m + (size_t)(d.N + 1) * d.nz; }

// The QP as the SCP loop needs it: condensed interior point, states by a rollout of the minimiser, objective, trust-region
// test.  Returns 0 when the result IS the minimiser of the full QP (converged, inside the trust region); anything else
// means "hand this QP to the fused kernel" (status of the interior point, or 100 = minimiser outside the trust region).
template <int MSEL, int NSEL, int GXSEL, int NST = 0, int J0SEL = 0>
__device__ __forceinline__ int solve_qp(const QPDims &dfull, const QPConst &c, const QPDyn &dyn, const QPData &q, gptr work_base,
                                        Lds &L, double *J_out, int *iters_out, QPWork &wout, lapc::Launch &prof, int warm = 0) {
    const int tid = SRH_TID, nt = blockDim.x;
    QPLds Lq{};
    Lq.v1 = L.v1; Lq.v2 = L.v2; Lq.Qu = L.Qu; Lq.part = L.part; Lq.red = L.red; Lq.idxl = L.idxl; Lq.flag = L.flag;
    int it = 0;
    int st;
    // GXSEL > 0: box-structured input rows, rows next to their sums, GXSEL lanes per stage for the state rows (one variant per
    // kernel: both interior points in one kernel thrash the instruction cache -- measured -8 % on everything)
    // NST < 0: the short-horizon instantiations (one tile of K): the interior point on one wave
    // NST > 0 and J0SEL == NST: the half-size workgroup (4 waves, every packed row of G in L2)
    constexpr bool HALFWG = NST > 0 && J0SEL == NST;
    if constexpr (NST < 0) st = ipm_wave<MSEL, NSEL, GXSEL>(dfull, c, dyn, q, work_base, L, &it, wout, prof, warm);
    else if constexpr (HALFWG) st = ipm_box4<MSEL, NSEL, GXSEL, NST, J0SEL>(dfull, c, dyn, q, work_base, L, &it, wout, prof, warm);
    else if constexpr (GXSEL > 0) st = ipm_box<MSEL, NSEL, GXSEL, NST, J0SEL>(dfull, c, dyn, q, work_base, L, &it, wout, prof, warm);
    else st = ipm<MSEL, NSEL>(dfull, c, dyn, q, work_base, L, Lq, &it, wout, prof);
    if (iters_out) *iters_out = it;
    if (st != 0) return st;
    lapc::Clock tail;
    QPDims d0 = dfull;
    d0.tr = 0;
    QPWork w = wout;
    const int N = d0.N, n = d0.n;
    const double s0 = qp::slack0(dfull, c, q, Lq);
    for (int k = tid; k < N; k += nt) L.idxl[k] = dyn.idx ? dyn.idx[k] : k;
    for (int e = tid; e <= N; e += nt) w.s[e] = (e == 0) ? s0 : 0.0;
    __syncthreads();
    lptr xs = L.B;                                        // (N + 1) n_x doubles at the start of the Theta^T area: free from here on
    rollout<MSEL, NSEL, true, HALFWG ? 4 : 8>(d0, dyn, q.x0, (cgptr)w.u, w.x, L, xs);
    __syncthreads();
    tail.lap(prof, lapc::TAIL_ROLLOUT);
    // (with x and H read from global memory the Diamond fixed layouts were better off with the one-thread-per-stage form -- 54.5 against
    // 55.0 ms per 4096 rollouts --; with the rollout's LDS copy of the trajectory every layout takes the form below)
    double J;
#ifdef SRH_LEAN_OBJECTIVE_SERIAL
    if constexpr (NST <= 0 || MSEL == 8) J = objective_par(d0, c, q, (cgptr)w.x, w.u, w.s, w.ez, Lq);
    else J = qp::objective(d0, c, q, w.x, w.u, w.s, Lq);
#else
    // (the output matrix behind the trajectory copy when the Theta^T area has the room: always at the shipped shapes)
    const bool hfit = (size_t)(N + 1) * n + objective_lds_doubles(d0) <= (size_t)d0.NK * (16 * (size_t)d0.KT + 1);
    J = objective_par(d0, c, q, (clptr)xs, w.u, w.s, w.ez, Lq, hfit, xs + (size_t)(N + 1) * n);
#endif
    bool inside = true;
    if (dfull.tr) {
        double md = 0.0;
        for (int e = tid + n; e < (N + 1) * n; e += nt) md = fmax(md, fabs(c.xs[e % n] * (xs[e] - q.xk[e])));
        md = wg::reduce(md, 1, L.red);
        inside = md <= q.delta;
        J += q.omega * s0;
    }
    tail.lap(prof, lapc::TAIL_OBJECTIVE);
    if (J_out) *J_out = J;
    return inside ? 0 : 100;
}

}  // namespace ql

