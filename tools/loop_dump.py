"""Bit-level dump of the five closed-loop units (csrc/gusto_loop.hip, gusto_ssm_loop.hip, rompc_loop.hip, koopman_loop.hip, ilqr_loop.hip
and the host shell they share, csrc/gusto_loop_host.h with mpc_loop_host.h and loop_observed_host.h) and of the TPWL rollout kernels
(csrc/tpwl.hip) for comparing two builds of the library (SRH_LIB_PATH selects one).

Runs the loops of the test suites at their own smallest shapes through scp.closed_loop / scp.closed_loop_ssm and records every array
that comes back, raw:
  - TPWL (tests/test_gusto_loop_gpu.py: cl_cases.LOOPS 'frac' and 'zf-u', g6 model, B = 3): reset(x0, 0.1), run(2, W), run(2, W),
    run(4, record_x=False), then _advance once on the last plan;
  - observed TPWL (tests/test_gusto_loop_observer_gpu.py: the g6 loop, n_y = 6, B = 3): reset_observed, run_observed(2, W, V) twice, then
    _advance_observed on the case 'g6-frac-3' of clobs_cases.CASES;
  - SSM (tests/test_gusto_ssm_loop_gpu.py: 'hw' and 'frac', B = 3, observe True and False): reset with v0, run(2, W, V) twice, and the
    stand-alone advance on one entry of ssm_loop_cases.ADVANCE;
  - ROMPC (tests/test_rompc_loop_gpu.py: 'frac' and 'zf-u', g6 model, B = 3): reset(x0, x_hat0, 0.1), run(2, W, V) twice, then _chain (first
    and later period) and _advance alone on the entries 'g6-frac-10', 'r36-5-10', 'm8-frac-10' and 'g6-replay' of rompc_loop_cases.ADVANCE;
  - Koopman (tests/test_koopman_loop_gpu.py: '5-1' and '1-3', the shipped model on the r36 plant, B = 3): reset, run(2, W, V) twice, then
    _fixup (first and later period) and _advance alone on the entries 'r36-ship-5-1', 'm8-w-1-1', 'g6-dmd-5-1' and 'r36-ship-replay' of
    koopman_loop_cases.ADVANCE, and the re-projected _advance of tests/test_koopman_reproject_gpu.py (n_y = 3, 'box+1', B = 3, replay);
  - iLQR (tests/test_ilqr_loop_gpu.py: 'g6-r5-tail' (r = 5) and 'g6-r1' of ilqr_loop_cases.ADVANCE, 'obs-r5-mismatch' of OBSERVED): _advance
    alone, a run split in two in the middle of a controller step without and with an observer, last_policy and stats behind each;
  - rollout (tests/test_tpwl_rollout_staged_gpu.py: every entry of SHAPES -- staged with the held table, staged with the wave search,
    plain above 64 KB -- and the velocity-weighted model): X and Z of the staged handle and of the plain one;
after every run also last_inputs(), last_plan() and stats().  The host-side refusals are recorded as text, message for message: run
before reset, periods * n_keep over the cap, last_inputs before a period, the observed run without an observer, the SSM model mismatch,
the later-period shift without a previous plan, a QP with a trust region or input-rate rows handed to the two linear MPC creates, the
iLQR run without a policy and the observers of another batch or model.

    python tools/loop_dump.py --out dumps/new        writes <out>.bin (the records, raw) and <out>.json (their index)
    python tools/loop_dump.py --compare A B --log profiles/x.log    compares two dumps record by record, byte for byte; exit 1 on a difference

One dump per process.  Needs the GPU (not for --compare)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tests')]

T_START = 0.1
RESULT_FIELDS = ('x', 'z', 'u', 'iters', 'status', 'J', 't', 'x_hat', 'y', 'ekf_status')


class Records(list):
    def array(self, name, a):
        self.append((name, b'' if a is None else np.ascontiguousarray(a).tobytes()))

    def arrays(self, label, d):
        for k, a in d.items():
            self.array('%s/%s' % (label, k), a)

    def after_run(self, label, cl, r, fields=RESULT_FIELDS):
        self.arrays(label, {f: getattr(r, f) for f in fields})
        self.arrays(label + '/last_inputs', cl.last_inputs())
        self.arrays(label + '/last_plan', dict(zip(('xopt', 'uopt'), cl.last_plan())))
        self.append((label + '/stats', json.dumps(cl.stats(), sort_keys=True).encode()))

    def refusal(self, label, call):
        try:
            call()
            text = 'NOT REFUSED'
        except RuntimeError as e:
            text = str(e)
        self.append(('refusal/' + label, text.encode()))


def dump_tpwl(rec):
    import cl_cases as cc
    import test_gusto_loop_gpu as tl
    for name in ('frac', 'zf-u'):
        cl, gu, inp = tl.make_loop(name, 3)
        label = 'tpwl/' + name
        if name == 'frac':
            rec.refusal('tpwl/run_before_reset', lambda: cl.run(1))
        cl.reset(inp['x0'], T_START)
        if name == 'frac':
            rec.refusal('tpwl/last_inputs_before_a_period', lambda: cl.last_inputs())
        for q in range(2):
            rec.after_run('%s/run2_%d' % (label, q), cl, cl.run(2, W=inp['W'][2 * q:2 * q + 2]))
        cl.reset(inp['x0'], T_START)
        rec.after_run(label + '/run4_no_x', cl, cl.run(cc.PERIODS, record_x=False))
        xo, uo = cl.last_plan()
        rec.arrays(label + '/advance', dict(zip(('X', 'Z', 'U', 'idx_plant', 'idx_gain'), cl._advance(xo, uo, cl.last_inputs()['x0']))))
    cl, gu, inp = tl.make_loop('frac', 3, max_steps_per_run=30)
    cl.reset(inp['x0'], T_START)
    rec.refusal('tpwl/over_the_cap', lambda: cl.run(4))
    # the library's own answer to an observed run on a loop without an observer (the class refuses earlier, with its own message)
    from sofacontrol_amd import _lib
    d, i = np.empty(1), np.empty(1, dtype=np.int32)
    rec.refusal('tpwl/observed_run_without_an_observer/class', lambda: cl.run_observed(1))
    rec.refusal('tpwl/observed_run_without_an_observer/library', lambda: _lib.check(_lib.lib().sgusto_loop_run_observed(
        cl._h, C.c_int(1), None, None, None, _lib.dptr(d), _lib.dptr(d), _lib.iptr(i), _lib.iptr(i), _lib.dptr(d), _lib.dptr(d), _lib.dptr(d),
        _lib.iptr(i)), 'sgusto_loop_run_observed'))


def dump_observed(rec):
    import clobs_cases as oc
    import test_gusto_loop_observer_gpu as to
    from sofacontrol_amd.scp.closed_loop import ClosedLoopBatch
    cl, inp = to.make_loop('g6', (0, 1, 2))
    rec.refusal('observed/run_before_reset', lambda: cl.run_observed(1))
    cl.reset_observed(inp['x0'], inp['x_hat0'], T_START)
    rec.refusal('observed/last_inputs_before_a_period', lambda: cl.last_inputs())
    for q in range(2):
        rec.after_run('observed/g6/run2_%d' % q, cl, cl.run_observed(2, W=inp['W'][2 * q:2 * q + 2], V=inp['V'][2 * q:2 * q + 2]))
    rec.refusal('observed/over_the_cap', lambda: cl.run_observed(17))
    cs = [c for c in oc.CASES if c[0] == 'g6-frac-3'][0]
    name, mname, same, dt_sim, n_keep = cs[:5]
    tp, gm = to.planner(mname)
    c = oc.case(cs)
    cl = ClosedLoopBatch(to.make_gusto(mname, oc.B, np.zeros((oc.B, gm.n_x))), tp, dt_sim, n_keep, K=c['K'], observer=to.make_observer(mname, same, oc.B))
    rec.arrays('observed/advance/' + name, cl._advance_observed(c['xopt'], c['uopt'], c['x'], c['x_hat'], c['W'], c['V']))
    rec.refusal('observed/run_behind_the_advance', lambda: cl.run_observed(1))


def dump_ssm(rec):
    import ssm_cases as sc
    import ssm_loop_cases as slc
    import test_gusto_ssm_loop_gpu as ts
    from test_ssm_gpu import product_ssm
    from sofacontrol_amd.scp import closed_loop_ssm
    for name in ts.LOOPS:
        for observe in (True, False):
            cl, gu, inp = ts.make_loop(name, 3, observe=observe)
            label = 'ssm/%s/%s' % (name, 'estimate' if observe else 'state')
            if name == 'hw' and observe:
                rec.refusal('ssm/run_before_reset', lambda: cl.run(1))
            cl.reset(inp['x0'], T_START, v0=inp['v0'])
            if name == 'hw' and observe:
                rec.refusal('ssm/last_inputs_before_a_period', lambda: cl.last_inputs())
            for q in range(2):
                rec.after_run('%s/run2_%d' % (label, q), cl, cl.run(2, W=inp['W'][2 * q:2 * q + 2], V=inp['V'][2 * q:2 * q + 2]))
    cl, gu, inp = ts.make_loop('frac', 3, max_steps_per_run=30)
    cl.reset(inp['x0'], T_START)
    rec.refusal('ssm/over_the_cap', lambda: cl.run(8))
    hw = ts.make_gusto('hw', 3, ts.inputs('hw', 3)['x0'])
    rec.refusal('ssm/model_mismatch', lambda: closed_loop_ssm.SSMClosedLoopBatch(hw, ts.models('frac')[1], 0.02, 2))
    case = slc.ADVANCE[1]
    s, method, dt_sim, dt, N, nk = case
    planner = product_ssm(sc.oracle_model(sc.model(s)), discr='fe')
    pm = sc.oracle_model(slc.plant_model(s))
    plant = product_ssm(pm, discrete=True) if method == 'map' else product_ssm(pm, discr=method)
    i = slc.inputs(case)
    got = closed_loop_ssm.advance(plant, planner, dt_sim, N, i['j'], i['theta'], i['uopt'], i['x'], W=i['W'], V=i['V'])
    rec.arrays('ssm/advance/' + slc.case_id(case), got)


def dump_rompc(rec):
    import rompc_loop_cases as rc
    import test_rompc_loop_gpu as tr
    for name in tr.LOOPS:
        cl, inp = tr.make_loop(name, 3)
        label = 'rompc/' + name
        if name == 'frac':
            rec.refusal('rompc/run_before_reset', lambda: cl.run(1))
        cl.reset(inp['x0'], inp['x_hat0'], T_START)
        for q in range(2):
            rec.after_run('%s/run2_%d' % (label, q), cl, cl.run(2, W=inp['W'][2 * q:2 * q + 2], V=inp['V'][2 * q:2 * q + 2]), tr.FIELDS + ('t',))
    from sofacontrol_amd import _lib
    create_refusals(rec, 'srompc', cl, lambda h, prob: _lib.lib().srompc_loop_create(
        C.byref(h), cl.observer._h, C.cast(C.byref(prob), C.c_void_p), _lib.dptr(cl._A), _lib.dptr(cl._B), _lib.dptr(cl._d), C.c_double(cl.dt),
        cl.plant.handle_for(cl.dt_sim), C.c_double(cl.dt_sim), C.c_int(cl.n_keep), C.c_int64(cl.max_steps_per_run)))
    for name in ('g6-frac-10', 'r36-5-10', 'm8-frac-10', 'g6-replay'):
        case = [c for c in rc.ADVANCE if c[0] == name][0]
        c, cl = rc.advance_case(case), tr.advance_loop(case)
        rec.arrays('rompc/advance/' + name, cl._advance(c['xopt'], c['uopt'], c['x'], c['x_hat'], W=c['W'], V=c['V'], X_plant=c['X_plant']))
        if name != 'g6-replay':
            k = rc.chain_case(case[2], cl.N, cl.n_x, cl.n_u, case[-1])
            for first in (True, False):
                got = cl._chain(k['xsol'], k['usol'], k['x0'], k['status'], None if first else k['xprev'], None if first else k['uprev'], first=first)
                rec.arrays('rompc/chain/%s_%s' % (name, 'first' if first else 'later'), dict(zip(('xopt', 'uopt', 'x0_next'), got)))
            if name == 'g6-frac-10':
                rec.refusal('rompc/later_chain_without_a_previous_plan', lambda: cl._chain(k['xsol'], k['usol'], k['x0'], k['status'], first=False))


def create_refusals(rec, label, cl, create):
    """The library's answers to a QP the resident linear MPC loops do not offer: create(problem) is the class's own create call."""
    from sofacontrol_amd import _lib
    for field, value in (('tr_active', 1), ('ndU', 1)):
        prob = type(cl.problem())()
        C.pointer(prob)[0] = cl.problem()
        setattr(prob, field, value)
        h = C.c_void_p()
        rec.refusal('%s/create_%s' % (label, field), lambda: _lib.check(create(h, prob), label + '_loop_create'))
        assert not h.value


def dump_koopman(rec):
    import koopman_loop_cases as kc
    import koopman_reproject_cases as qc
    import test_koopman_loop_gpu as tk
    import test_koopman_reproject_gpu as tq
    from sofacontrol_amd import _lib
    for name in tk.LOOPS:
        cl, inp = tk.make_loop(name, 3)
        label = 'koopman/' + name
        if name == '5-1':
            rec.refusal('koopman/run_before_reset', lambda: cl.run(1))
        tk.reset(cl, inp, T_START)
        if name == '5-1':
            rec.refusal('koopman/last_inputs_before_a_period', lambda: cl.last_inputs())
        for q in range(2):             # (three periods of noise: the second run reads periods 1 and 2)
            rec.after_run('%s/run2_%d' % (label, q), cl, cl.run(2, W=inp['W'][q:q + 2], V=inp['V'][q:q + 2]), tk.FIELDS + ('t',))
    rec.refusal('koopman/over_the_cap', lambda: cl.run(17))
    p = cl.plant.handle_for(cl.dt_sim)
    create_refusals(rec, 'skoop', cl, lambda h, prob: _lib.lib().skoop_loop_create(
        C.byref(h), cl.lift._h, C.cast(C.byref(prob), C.c_void_p), _lib.dptr(cl._A), _lib.dptr(cl._Bm), C.c_double(kc.TS), p, _lib.dptr(cl._C),
        _lib.dptr(cl._yref), _lib.dptr(cl.u0), C.c_double(cl.dt_sim), C.c_int(cl.rollout_horizon), C.c_int64(cl.max_steps_per_run)))
    for name in ('r36-ship-5-1', 'm8-w-1-1', 'g6-dmd-5-1', 'r36-ship-replay'):
        case = [c for c in kc.ADVANCE if c[0] == name][0]
        c, cl, h = kc.advance_case(case), tk.advance_loop(case), kc.history(case, case[5])
        sim = case[8] == 'sim'
        cl.reset(x0=c['x'] if sim else None, y0=None if sim else c['Y_plant'][:, 0], y_hist=h['y_hist'], u_hist=h['u_hist'], u_prev0=h['u_prev0'],
                 v0=h['v0'] if sim else None)
        rec.arrays('koopman/advance/' + name, cl._advance(c['uopt'], c['x'] if sim else None, W=c['W'], V=c['V'], Y_plant=c['Y_plant'],
                                                          U_applied=c['U_applied']))
        rec.array('koopman/advance/%s/ring' % name, tk.ring_of(cl.lift)[0])
        if name == 'r36-ship-5-1':
            rec.refusal('koopman/run_behind_the_advance', lambda: cl.run(1))
        if sim:
            s = kc.spec(case[2])
            k = kc.fixup_case(case[5], s['n_lift'], s['m'], case[-1])
            k['status'][0] = 5 if case[5] == 1 else 0
            for first in (True, False):
                got = cl._fixup(k['xsol'], k['usol'], k['x0'], k['status'], None if first else k['xprev'], None if first else k['uprev'], first=first)
                rec.arrays('koopman/fixup/%s_%s' % (name, 'first' if first else 'later'), dict(zip(('xopt', 'uopt'), got)))
            if name == 'r36-ship-5-1':
                rec.refusal('koopman/later_fixup_without_a_previous_plan', lambda: cl._fixup(k['xsol'], k['usol'], k['x0'], k['status'], first=False))
    ny, rows, B = 3, 'box+1', 3
    s = qc.spec(ny)
    nk = qc.N * qc.R
    Yp, _ = qc.replay_samples(ny, rows, B, nk)
    cl = tq.replay_loop(ny, B, qc.N, tq.Ypoly(*qc.polyhedron(ny, rows)))
    rng = np.random.default_rng(31 + ny)
    y_hist = s['y_offset'] + s['y_factor'] * rng.uniform(-1.0, 1.0, (B, 1, ny))
    u_hist, u_prev0 = rng.uniform(0.0, 100.0, (B, 1, qc.M)), rng.uniform(0.0, 100.0, (B, qc.M))
    cl.reset(y0=Yp[:, 0], y_hist=y_hist, u_hist=u_hist, u_prev0=u_prev0)
    rec.arrays('koopman/advance/reprojected-3-box+1', cl._advance(rng.uniform(-1.0, 1.0, (B, qc.N, qc.M)), Y_plant=Yp))


def dump_ilqr(rec):
    import ilqr_loop_cases as ic
    import test_ilqr_loop_gpu as ti
    from sofacontrol_amd.lqr.closed_loop import ILQRClosedLoopBatch
    from sofacontrol_amd.tpwl.observer import DiscreteEKFObserverBatch

    def after(label, cl, r):
        rec.arrays(label, {f: getattr(r, f) for f in ('x', 'z', 'u', 'x_hat', 'y', 'ekf_status', 't')})
        rec.arrays(label + '/last_policy', dict(zip(('x_bar', 'u_bar', 'K'), cl.last_policy())))
        rec.append((label + '/stats', json.dumps(cl.stats(), sort_keys=True).encode()))

    bare = ILQRClosedLoopBatch(ti.ilqr_of('g6', 12), ti.plant('g6'), 0.05, 3, max_steps_per_run=10)
    rec.refusal('ilqr/run_before_reset', lambda: bare.run(1))
    bare.reset(ic.advance_case(ic.ADVANCE[0])['x'])
    rec.refusal('ilqr/run_without_a_policy', lambda: bare.run(1))
    rec.refusal('ilqr/last_policy_without_a_policy', lambda: bare.last_policy())
    for name in ('g6-r5-tail', 'g6-r1'):
        case = [c for c in ic.ADVANCE if c[0] == name][0]
        S = case[5]
        cl, c = ti.make_loop(case, max_steps_per_run=S)
        rec.arrays('ilqr/advance/' + name, dict(zip(('X', 'Z', 'U', 'idx'), cl._advance(c['x'], S, W=c['W']))))
        cl.reset(c['x'])
        k = 7 if case[4] > 1 else S // 2           # (r = 5: the held input crosses the run boundary)
        cut = lambda a, lo, hi: None if a is None else a[lo:hi]
        after('ilqr/%s/run_%d' % (name, k), cl, cl.run(k, W=cut(c['W'], 0, k)))
        after('ilqr/%s/run_%d' % (name, S - k), cl, cl.run(S - k, W=cut(c['W'], k, S)))
        if name == 'g6-r1':
            rec.refusal('ilqr/over_the_cap', lambda: cl.run(S + 1))
    cs = [c for c in ic.OBSERVED if c[0] == 'obs-r5-mismatch'][0]
    steps = cs[3]
    cl, c = ti.make_observed(cs)
    cl.reset(c['x'], c['x_hat'])
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]
    after('ilqr/%s/run_7' % cs[0], cl, cl.run(7, W=cut(c['W'], 0, 7), V=cut(c['V'], 0, 7)))
    after('ilqr/%s/run_%d' % (cs[0], steps - 7), cl, cl.run(steps - 7, W=cut(c['W'], 7, steps), V=cut(c['V'], 7, steps)))
    # the library's own answers to an observer of another batch and of another model width (the class may refuse earlier, in its own words)
    from sofacontrol_amd import _lib
    import clobs_cases as oc
    ms = oc.measurement('g6')
    four = DiscreteEKFObserverBatch(ti.filter_model(True), 4, Sigma0=ms['Sigma0'], W=ms['W'], V=ms['V'])
    rec.refusal('ilqr/observer_of_another_batch', lambda: _lib.check(_lib.lib().silqr_loop_set_observer(cl._h, four._h), 'silqr_loop_set_observer'))
    r36, _ = ti.make_loop([c for c in ic.ADVANCE if c[0] == 'r36-r5'][0])
    three = DiscreteEKFObserverBatch(ti.filter_model(True), 3, Sigma0=ms['Sigma0'], W=ms['W'], V=ms['V'])
    rec.refusal('ilqr/observer_of_another_model', lambda: _lib.check(_lib.lib().silqr_loop_set_observer(r36._h, three._h), 'silqr_loop_set_observer'))


def dump_rollout(rec):
    import test_tpwl_rollout_staged_gpu as tg
    cases = [('-'.join(map(str, s)), tg.shape_case(*s), path) for s, path in tg.SHAPES] + [('6-3-12-12-3-wv', tg.shape_case(6, 3, 12, 12, 3, w_v=0.5), (True, False))]
    for name, c, path in cases:
        batch, N = c['u'].shape[0], c['u'].shape[1]
        plan = c['staged'].plan(N, batch)
        kind = 'plain' if not plan['staged'] else 'held' if plan['held'] else 'wave'
        assert (plan['staged'], plan['held']) == path, (name, plan)
        rec.append(('rollout/%s/%s/plan' % (kind, name), json.dumps(plan, sort_keys=True).encode()))
        for which in ('staged', 'plain'):
            rec.arrays('rollout/%s/%s/%s_handle' % (kind, name, which), dict(zip(('X', 'Z'), c[which].rollout(c['x0'], c['u']))))


def dump(out):
    from sofacontrol_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    _lib.set_device(0)
    rec = Records()
    dump_tpwl(rec)
    dump_observed(rec)
    dump_ssm(rec)
    dump_rompc(rec)
    dump_koopman(rec)
    dump_ilqr(rec)
    dump_rollout(rec)
    index, off = [], 0
    with open(out + '.bin', 'wb') as f:
        for name, b in rec:
            f.write(b)
            index.append(dict(name=name, offset=off, bytes=len(b), sha256=hashlib.sha256(b).hexdigest()))
            off += len(b)
    refusals = {name: b.decode() for name, b in rec if name.startswith('refusal/')}
    with open(out + '.json', 'w') as f:
        json.dump(dict(library=os.path.relpath(_lib.LIB_PATH, ROOT), refusals=refusals, records=index), f, indent=0)
    print('loop_dump: %d records (%d refusals), %d bytes -> %s.bin (library %s)' % (len(index), len(refusals), off, out, os.path.relpath(_lib.LIB_PATH, ROOT)))


def compare(a, b, log):
    ja, jb = (json.load(open(p + '.json')) for p in (a, b))
    ba, bb = (open(p + '.bin', 'rb').read() for p in (a, b))
    lines = ['loop_dump --compare', 'A: %s (library %s)' % (a, ja['library']), 'B: %s (library %s)' % (b, jb['library'])]
    same_index = [r['name'] for r in ja['records']] == [r['name'] for r in jb['records']]
    lines.append('records: %d / %d, same names in the same order: %s' % (len(ja['records']), len(jb['records']), same_index))
    per_group, differing = {}, []
    if same_index:
        for ra, rb in zip(ja['records'], jb['records']):
            equal = ba[ra['offset']:ra['offset'] + ra['bytes']] == bb[rb['offset']:rb['offset'] + rb['bytes']]
            parts = ra['name'].split('/')
            group = '/'.join(parts[:1 if parts[0] == 'refusal' else 2 if parts[0] == 'rollout' else 4 if parts[0] == 'ssm' and parts[1] != 'advance' else 3])
            t = per_group.setdefault(group, [0, 0, 0])
            t[0] += 1
            t[1] += 0 if equal else 1
            t[2] += ra['bytes']
            if not equal:
                differing.append(ra['name'])
    for group, (total, bad, size) in per_group.items():
        lines.append('%-44s %3d records, %7d bytes, %s' % (group, total, size, 'identical' if bad == 0 else '%d DIFFER' % bad))
    lines.append('refusals, message for message:')
    for name, text in ja['refusals'].items():
        lines.append('  %-52s %s' % (name[len('refusal/'):], 'same: ' + text if jb['refusals'].get(name) == text else
                                     'DIFFER: %r / %r' % (text, jb['refusals'].get(name))))
    ok = same_index and not differing and ba == bb and ja['refusals'] == jb['refusals'] and 'NOT REFUSED' not in ja['refusals'].values()
    lines += ['first differing records: %s' % differing[:8]] if differing else []
    lines.append('whole files (%d / %d bytes) identical: %s' % (len(ba), len(bb), ba == bb))
    lines.append('RESULT: %s' % ('identical, byte for byte' if ok else 'DIFFERENT'))
    print('\n'.join(lines))
    if log:
        with open(log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--log')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.log))
    if not args.out:
        ap.error('need --out or --compare')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dump(args.out)


if __name__ == '__main__':
    main()
