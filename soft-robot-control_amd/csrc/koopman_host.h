// Host-side Koopman lift handle (owns the observable table, the scaling vectors and the measurement ring in HBM) and the launcher of
// its lift kernels, shared by koopman.hip / koopman_loop.hip.  The kernels themselves are koopman.hip's (koop_lift_fn).
#pragma once
#include "common.h"

enum { KP_ZETA = 0, KP_RECORD = 1, KP_RING = 2 };
constexpr int KP_NT = 256;               // threads of the lift kernel (4 waves)

struct KoopLiftArgs {
    int64_t rows;                 // output rows
    int nz, P, Nw;                // zeta dimension, observables, output columns (rows of W, or P without W)
    int ny, m, delay, slots, head;
    int nlev, has_const;          // degree levels of the table, constant observable last
    const double *zeta;           // KP_ZETA: (rows x nz)
    const double *y, *u;          // KP_RECORD: (T x ny), (T x m); row r is sample r + delay
    const double *ring;           // KP_RING: (rows x slots x (ny + m)) scaled samples, newest in slot `head`
    const double *yoff, *yfac, *uoff, *ufac;   // KP_RECORD only: (ny), (ny), (m), (m)
    const int32_t *par, *var, *lev;            // recurrence psi[k] = psi[par[k]] * zeta[var[k]] (par < 0: 1); lev (nlev + 1)
    const double *W;              // (Nw x P) or NULL
    double *out;                  // (rows x Nw)
    int TR, ld;                   // rows per block (multiple of 16), LDS row stride of psi (>= P rounded up to 4)
};

struct skoop {
    int ny, m, delay, degree, dmd, nz, P, Nw;
    int64_t batch;
    bool has_w = false;
    int nlev = 0;
    srh::DevBuf par, var, lev, W, scale, ring, stage;
    int slots = 0, head = -1;
    int64_t count = 0;            // samples pushed (the ring holds the last `slots` of them)
    hipStream_t stream = nullptr;
    double *pin = nullptr;        // batch x (ny + m) push staging
    hipEvent_t pushed = nullptr;  // the last push's H2D copy (the pinned block is rewritten only after it)
    bool push_pending = false;    // a push was enqueued after the last synchronisation of the stream
    int64_t host_waits = 0;       // blocking waits the handle's calls made (event / stream synchronisations)
    int TR = 64, ld = 0;          // lift tile: rows per workgroup, LDS row stride of psi
    size_t lds = 0;               // dynamic LDS of a lift launch (the kernels' limits are raised once, at creation)
};

// the lift kernel of a mode (koopman.hip: the instances live there; not among the library's dynamic symbols)
__attribute__((visibility("hidden"))) const void *koop_lift_fn(int mode, bool has_w);

static int koop_launch_lift(const skoop *h, int mode, const KoopLiftArgs &base, hipStream_t st) {
    KoopLiftArgs a = base;
    if (a.rows <= 0) return SRH_OK;
    a.nz = h->nz; a.P = h->P; a.Nw = h->has_w ? h->Nw : h->P;
    a.ny = h->ny; a.m = h->m; a.delay = h->delay; a.slots = h->slots;
    a.nlev = h->nlev; a.has_const = h->dmd ? 0 : 1;
    a.par = h->par.as<int32_t>(); a.var = h->var.as<int32_t>(); a.lev = h->lev.as<int32_t>();
    a.W = h->has_w ? h->W.as<double>() : nullptr;
    a.ld = h->ld;
    a.TR = h->TR;
    const unsigned grid = (unsigned)srh::cdiv(a.rows, h->TR);
    void *args[] = {&a};
    SRH_CHECK_HIP(hipLaunchKernel(koop_lift_fn(mode, h->has_w), dim3(grid), dim3(KP_NT), args, h->lds, st));
    return SRH_OK;
}
