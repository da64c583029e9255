// Lap clocks of the SCP / QP kernels (locp_dev.h, locp_cond.h, locp_lean.h, gusto.hip, lean.hip): shader clocks per phase, printed by
// a build with -DSRH_PROFILE (tools/build_lean.sh).  The macro is tested HERE and nowhere else: everything below is plain C++ over the
// constant lapc::ON, so the product build parses and type-checks every profile statement -- and compiles none: with ON false every
// type here is empty and every member does nothing (the kernels inline all of it), the product's instructions are those of a source
// without a single lap.  A statement that must not even be evaluated in the product build (a printf, a read of the LDS mailbox) goes
// behind `if constexpr (lapc::ON)`, never into the arguments of a member call.
//
// To add a lap: name its slot in the enum that owns it (Slot for the per-launch array; the small local arrays -- Gram fill, factor
// chain, SCP loop, Riccati -- are indexed by the order of their print), call lap(slot) behind the phase, print it next to its neighbours.
// Declare a new clock at the top of the function body and restart() it where it starts -- an (empty) object declared in a nested
// scope, and a value computed only to be passed to add(), have both changed the product's register allocation -- and compare the kept
// assembly (csrc/<unit>.s) of the product build with the one from before the change.
#pragma once
#include <type_traits>

namespace lapc {

#ifdef SRH_PROFILE
constexpr bool ON = true;
#else
constexpr bool ON = false;
#endif

// The per-launch counters of the lean kernels (lean.hip prints them; ql::solve_qp and the interior points below it fill them).
// Clocks unless marked as a count.
enum Slot : int {
    QP_SETUP = 0,           // set-up + zero-input rollout
    QP_ROWS,                // rows: weights, gradient shifts, their sums
    QP_CONDENSE,
    QP_STAGE_FACTORS,
    QP_GRAM,
    QP_CHOLESKY,            // (box interior points: the split up to its join, see SPLIT_*)
    QP_NEWTON,              // gradients + Newton solve
    QP_STEPS,               // from the direction to the top of the next iteration
    NT_GRADIENTS = 8,       // the Newton solve (Prof: newton_front 8-11, newton_back 12-15)
    NT_GT1, NT_RHS, NT_G1, NT_KSOLVE, NT_GT2, NT_DU, NT_G2,
    NT_END,
    SPLIT_FACTOR = 16,      // the split Newton system: the factorising wave set ...
    SPLIT_FRONT,            // ... and the front of the solve beside it
    STEP_ROWS = 18, STEP_AMAX, STEP_MU_ROWS, STEP_MU_AFF,
    TAIL_ROLLOUT = 22,      // solve_qp behind the interior point: rollout of the minimiser,
    TAIL_OBJECTIVE,         // objective + trust-region test
    N_IPM_ITERS = 24,       // COUNT: interior-point iterations
    N_QPS,                  // COUNT: QPs
    N_WARM_QPS,             // COUNT: of them warm started
    CHAIN_WAIT = 27,        // the factor chain on wave 0 (tile_cholesky_set)
    CHAIN_PANEL, CHAIN_UPDATE, CHAIN_FACTOR, CHAIN_SIGNALS,
    UNIT_TILES = 32,        // half-size workgroup: unit_tiles and its barrier
    EARLY_TEST = 33,        // the early stopping test's product and maximum
    N_EARLY_FOR_NOTHING,    // COUNT: early products after which the iteration went on
    NSLOT                   // length of the array (35)
};
static_assert(NT_END == SPLIT_FACTOR && NSLOT == 35, "the slot numbers are what lean.hip prints and tools/probes parse");

// The factor chain's own laps, in the order of CHAIN_WAIT .. CHAIN_SIGNALS
enum Chain : int { CH_WAIT, CH_PANEL, CH_UPDATE, CH_FACTOR, CH_SIGNALS, CH_END };

// Where one wave's laps wait in the LDS mailbox (ql::Lds::Qu, 16 doubles) for the thread that folds or prints them.
// [0] is the Newton front's dual residual and [15] the serial wave's pick: not laps.
enum Mail : int { MAIL_SPLIT_FACTOR = 2, MAIL_SPLIT_FRONT = 3, MAIL_GRAM = 4 /* ..7 */, MAIL_CHAIN = 8 /* ..12 */, MAIL_GRAM_BARRIER = 13, MAIL_GRAM_STORE = 14 };

// ---- N counters, zero at construction
template <int N, bool P = ON> struct Counters {
    long long t[N];
    __device__ __forceinline__ Counters() { for (int i = 0; i < N; ++i) t[i] = 0; }
    __device__ __forceinline__ void add(int slot, long long v = 1) { t[slot] += v; }
    __device__ __forceinline__ long long operator[](int slot) const { return t[slot]; }
};
template <int N> struct Counters<N, false> {
    __device__ __forceinline__ void add(int, long long = 1) {}
    __device__ __forceinline__ long long operator[](int) const { return 0; }
};

// ---- the clock value of the last lap
template <bool P = ON> struct ClockT {
    long long last;
    __device__ __forceinline__ ClockT() : last(clock64()) {}
    __device__ __forceinline__ void restart() { last = clock64(); }
    __device__ __forceinline__ void restart(const ClockT &c) { last = c.last; }
    __device__ __forceinline__ long long since() const { return clock64() - last; }      // (does not re-arm)
    template <class C> __device__ __forceinline__ void lap(C &c, int slot) { const long long now = clock64(); c.add(slot, now - last); last = now; }
};
template <> struct ClockT<false> {
    __device__ __forceinline__ ClockT() {}
    __device__ __forceinline__ void restart() {}
    __device__ __forceinline__ void restart(const ClockT &) {}
    __device__ __forceinline__ long long since() const { return 0; }
    template <class C> __device__ __forceinline__ void lap(C &, int) {}
};
using Clock = ClockT<>;

// ---- counters with their own clock
template <int N> struct Laps : Counters<N>, Clock {
    __device__ __forceinline__ void lap(int slot) { Clock::lap(static_cast<Counters<N> &>(*this), slot); }
    __device__ __forceinline__ void lap_sync(int slot) { if constexpr (ON) __syncthreads(); lap(slot); }      // a lap that ends at a barrier of its own
};

// ---- the per-launch array (one per thread; thread 0 of workgroup 0 prints)
struct Launch : Counters<NSLOT> {
    __device__ __forceinline__ void count_qp(int it, bool warm) { add(N_IPM_ITERS, it); add(N_QPS); add(N_WARM_QPS, warm ? 1 : 0); }
};

// ---- the sub-laps of the Newton solves of one QP (slots NT_*), passed through newton_front / newton_back / newton_solve
struct Prof : Laps<NT_END> {
    __device__ __forceinline__ void fold(Launch &p) const { for (int i = NT_GRADIENTS; i < NT_END; ++i) p.add(i, (*this)[i]); }
    __device__ __forceinline__ void fold(Launch &p, int it, bool warm) const { fold(p); p.count_qp(it, warm); }    // ... and the QP is counted
};

static_assert(ON || (std::is_empty<Clock>::value && std::is_empty<Laps<8>>::value && std::is_empty<Launch>::value && std::is_empty<Prof>::value),
              "the product build carries no lap state");

// ---- per-wave clocks of the Gram fill (products [wave], epilogue [8 + wave]), cumulative over workgroup 0 of every launch.
// (a variable template: the product build never names an instance, so none exists)
template <bool P> __device__ long long g_wave_laps[16];
template <bool P = ON> struct WaveLapsT {
    static __device__ __forceinline__ void add(int i, long long v) { if constexpr (P) g_wave_laps<P>[i] += v; }
    static __device__ __forceinline__ long long get(int i) { if constexpr (P) return g_wave_laps<P>[i]; else return 0; }
};
using WaveLaps = WaveLapsT<>;

}  // namespace lapc
