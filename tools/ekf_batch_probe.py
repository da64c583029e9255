"""Batched-filter probe (csrc/observer.hip, sekf_batch_step): B extended Kalman filters on the C2 Diamond shape (workloads.diamond_c2:
n_x = 60, n_u = 4, tables at dt_sim = 0.01), five measured nodes (n_y = 30), W = 100 I, V = I, for B in {1, 256, 4096}.

Two contenders over the same numbers, alternated step by step in one process:
  (a) sekf_batch_step: one upload, one launch of B workgroups, one copy back, one wait;
  (b) what the library offered before for the same work: B one-filter handles stepped in turn (sekf_step: one launch and one wait
      each).  (b) runs twice per step (b, b2): the difference of the two medians is the spread.
Both go through ctypes directly (no observer object in between).  Before timing, members 0, 1 and B - 1 of (a) are checked bit for bit
against their handles of (b).  Per step: host clock around work that ends in the call's own wait; 3 warm-up + 20 timed steps (at
B = 4096 the one-filter handles take 3 timed steps: 4096 waits each); median, min, max.

    python tools/ekf_batch_probe.py [--out profiles/ekf_batch_probe.json] [--batches 1,256,4096]

Needs the GPU.  Every number is a measurement of this run; DESIGN.md section 26 quotes them."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd')):
    sys.path.insert(0, p)

DT_SIM, WARM, TIMED, TIMED_HANDLES_4096 = 0.01, 3, 20, 3
NODES = [1354, 200, 600, 1000, 1500]


def build(w):
    from sofacontrol_amd.measurement_models import linearModel
    from sofacontrol_amd.tpwl.tpwl import TPWLATV
    n_f, r = w['U'].shape
    num_nodes = n_f // 3
    Hf = linearModel(nodes=[NODES[0]], num_nodes=num_nodes).C.tocsr()
    Cf = linearModel(nodes=NODES, num_nodes=num_nodes).C.tocsr()
    data = dict(w['tab'], rom_info=dict(type='POD', U=w['U'], q_ref=w['q_ref'], v_ref=w['v_ref']))
    model = TPWLATV(data=data, params=dict(tpwl_method='nn', dist_weights={'q': 1.0, 'v': 0.0}), Hf=Hf, Cf=Cf, discr_method='zoh')
    tab = model.tpwl_dict
    Ad, Bd, dd = model.discretize_batch(np.stack(tab['A_c']), np.stack(tab['B_c']), np.stack(tab['d_c']), DT_SIM)
    model.handle_for(DT_SIM, tables=(Ad, Bd, dd))
    return model


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(len(v)))


def probe(B, model, seed=0, handles=True):
    """handles=False: contender (a) alone (tools/ekf_handle_ab.py times it on two builds of the library)."""
    from sofacontrol_amd import _lib
    lib, f64, dptr = _lib.lib(), _lib.f64, _lib.dptr
    n, m, ny = model.get_state_dim(), model.get_input_dim(), model.C.shape[0]
    mh = model.handle_for(DT_SIM)
    Cm, yr = f64(model.C), f64(model.y_ref)
    S0, W, V = np.eye(n), 100.0 * np.eye(n), np.eye(ny)
    rng = np.random.default_rng(seed)
    steps = WARM + TIMED
    x0 = 0.5 * rng.standard_normal((B, n))
    u = rng.uniform(0.0, 300.0, (steps, B, m))
    y = yr + x0 @ Cm.T + 0.05 * rng.standard_normal((steps, B, ny))
    hb = C.c_void_p()
    _lib.check(lib.sekf_batch_create(C.byref(hb), mh, dptr(Cm), dptr(yr), C.c_int(ny), dptr(S0), dptr(W), dptr(V), C.c_int64(B)), 'sekf_batch_create')
    _lib.check(lib.sekf_batch_set_state(hb, dptr(x0), None), 'sekf_batch_set_state')
    hs = []
    for b in range(B if handles else 0):
        h = C.c_void_p()
        _lib.check(lib.sekf_create(C.byref(h), mh, dptr(Cm), dptr(yr), C.c_int(ny), dptr(S0), dptr(W), dptr(V)), 'sekf_create')
        _lib.check(lib.sekf_set_state(h, dptr(x0[b]), None), 'sekf_set_state')
        hs.append(h)
    xb, x1 = np.empty((B, n)), np.empty((B, n))
    up = [[(dptr(u[k, b]), dptr(y[k, b]), dptr(x1[b])) for b in range(len(hs))] for k in range(steps)]
    timed_handles = TIMED_HANDLES_4096 if B >= 4096 else TIMED
    ta, tb, tb2, equal = [], [], [], True
    for k in range(steps):
        t0 = time.perf_counter()
        _lib.check(lib.sekf_batch_step(hb, dptr(u[k]), dptr(y[k]), dptr(xb)), 'sekf_batch_step')
        t1 = time.perf_counter()
        if k >= WARM:
            ta.append(1e3 * (t1 - t0))
        if not handles:
            continue
        if k == 0:                          # the first step of every handle, and the comparison
            for b in range(B):
                _lib.check(lib.sekf_step(hs[b], up[k][b][0], up[k][b][1], None, None, None, up[k][b][2]), 'sekf_step')
            equal = all(np.array_equal(xb[b], x1[b]) for b in {0, min(1, B - 1), B - 1})
            continue
        if k < WARM - 1 or k >= WARM + timed_handles:
            continue
        for times in (tb, tb2):             # the same inputs twice: what is timed does not depend on the state
            t2 = time.perf_counter()
            for b in range(B):
                rc = lib.sekf_step(hs[b], up[k][b][0], up[k][b][1], None, None, None, up[k][b][2])
                if rc:
                    _lib.check(rc, 'sekf_step')
            t3 = time.perf_counter()
            if k >= WARM:
                times.append(1e3 * (t3 - t2))
    st = np.empty(B, dtype=np.int32)
    _lib.check(lib.sekf_batch_get_state(hb, None, None, _lib.iptr(st)), 'sekf_batch_get_state')
    for h in hs:
        lib.sekf_destroy(h)
    lib.sekf_batch_destroy(hb)
    if not handles:
        return dict(batch=B, failed_filters=int(st.sum()), batched_ms_per_step=stat(ta))
    a, b1, b2 = stat(ta), stat(tb), stat(tb2)
    spread = abs(b1['median'] - b2['median'])
    D = 8
    return dict(batch=B, members_equal_their_handles_bit_for_bit=bool(equal), failed_filters=int(st.sum()),
                batched_ms_per_step=a, handles_ms_per_step=b1, handles_repeat_ms_per_step=b2, handles_spread_ms=spread,
                batched_not_above_handles_by_more_than_the_spread=bool(a['median'] <= b1['median'] + spread),
                batched_us_per_filter_step=1e3 * a['median'] / B, handles_us_per_filter_step=1e3 * b1['median'] / B,
                waits_per_step=dict(batched=1, handles=B),
                pcie_bytes_per_step=dict(up=B * (m + ny) * D, down=B * n * D + B * 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ekf_batch_probe.json'))
    ap.add_argument('--batches', default='1,256,4096')
    args = ap.parse_args()
    import workloads as wl
    model = build(wl.diamond_c2())
    res = dict(shape=dict(n_x=model.get_state_dim(), n_u=model.get_input_dim(), n_y=int(model.C.shape[0]), dt_sim=DT_SIM, warm_up_steps=WARM,
                          timed_steps=TIMED, timed_steps_handles_at_4096=TIMED_HANDLES_4096),
               note='ms per fused predict + update step of all B filters: host clock around calls that end in their own wait; the '
                    'contenders alternate step by step; B = 1 and B = 4096 are reported, B = 256 is judged',
               results=[])
    for B in [int(v) for v in args.batches.split(',')]:
        res['results'].append(probe(B, model))
        print(json.dumps(res['results'][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
