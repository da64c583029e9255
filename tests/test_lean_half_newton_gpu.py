"""The Newton system of the half-size lean workgroup (ql::ipm_box4, instantiation <4, 60, 4, 50, 50, 4>): the staged Gram
fill keeps every tile in registers through its epilogue, joins "the staged rows are read" and "the scale factors are published" in ONE
barrier and stores each tile once, already scaled.  It is a reordering of the same arithmetic: a race on the merged barrier does not fail
loudly (the interior point corrects an inexact Newton step and converges anyway), so the cases ask for EQUALITY between runs and between
batch sizes, for the untouched full-size kernel's result at the tolerance tests/test_lean_half_gram_gpu.py uses for that pair, and for the
oracle's at the 1e-7 of tests/test_lean_toeplitz_gpu.py on both addressing forms of the fill.  BASELINE C2, solves capped at 5 SCP
iterations.  (The same cases covered the in-factor conversion of the unit tiles, which was measured and not adopted.)
(No failed-pivot case: K = I + Ls^T G D^-1 G^T Ls has no input that makes a pivot fail, and the suite has no knob that forces one on
the lean path.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HALF, FULL = (4, 60, 4, 50, 50, 4), (4, 60, 4, 50, 7, 4)
FIELDS = ('xopt', 'uopt', 'zopt', 'iters', 'status')


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def result(g):
    return {f: np.array(getattr(g, f)).copy() for f in FIELDS}


def plan(monkeypatch, half, w, gm, xc, fc, x0, u_init, x_init, z):
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    monkeypatch.setenv('SRH_LEAN_HALF', '1' if half else '0')
    g = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']), X=Polyhedron(w['XA'], w['Xb']),
              x_char=xc, f_char=fc, convg_thresh=1e-3, batch=x0.shape[0], max_trace=0, max_gusto_iters=5, first_solve_cap=5)
    assert g.kernel_info['lean'] == (HALF if half else FULL), g.kernel_info
    return g


def test_merged_barrier_of_the_staged_fill_does_not_race(monkeypatch):
    """600 rollouts (more than CUs: co-resident workgroups) solved three times: every output array identical.  The first 8 solved alone
    equal their rows of the 600 bit for bit."""
    import workloads as wl
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2()
    B, S = 600, 8
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    g = plan(monkeypatch, 1, w, gm, xc, fc, x0, u_init, x_init, z)
    runs = []
    for _ in range(3):
        g.solve_batch(x0, u_init, x_init, z=z)
        assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0
        runs.append(result(g))
    for k in (1, 2):
        print('solve %d vs solve 0: max |dx| %g |du| %g |dz| %g' % ((k,) + tuple(float(np.abs(runs[k][f] - runs[0][f]).max()) for f in FIELDS[:3])))
    for k in (1, 2):
        for f in FIELDS:
            assert np.array_equal(runs[k][f], runs[0][f]), (k, f)
    gs = plan(monkeypatch, 1, w, gm, xc, fc, x0[:S], u_init[:S], x_init[:S], z[:S])
    gs.solve_batch(x0[:S], u_init[:S], x_init[:S], z=z[:S])
    small = result(gs)
    print('batch of 8 vs its rows of the 600: max |dx| %g |du| %g' % (np.abs(small['xopt'] - runs[0]['xopt'][:S]).max(),
                                                                     np.abs(small['uopt'] - runs[0]['uopt'][:S]).max()))
    for f in FIELDS:
        assert np.array_equal(small[f], runs[0][f][:S]), f


def test_half_size_against_the_untouched_full_size_kernel(monkeypatch):
    """The same 64 rollouts on the half-size kernel and on the full-size one (pulled tasks, separate scaling pass):
    equal SCP iteration counts, trajectories within the 1e-8 of tests/test_lean_half_gram_gpu.py (measured there: 8.7e-15)."""
    import workloads as wl
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2()
    gm, xc, fc, x0, u_init, x_init, z = problem(w, 64, 2, 1354)
    res = {}
    for half in (1, 0):
        g = plan(monkeypatch, half, w, gm, xc, fc, x0, u_init, x_init, z)
        g.solve_batch(x0, u_init, x_init, z=z)
        assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0
        res[half] = result(g)
    ex, eu = rel(res[1]['xopt'], res[0]['xopt']), rel(res[1]['uopt'], res[0]['uopt'])
    print('half-size vs full-size, 64 rollouts: rel x %.2e u %.2e' % (ex, eu))
    assert np.array_equal(res[1]['iters'], res[0]['iters'])
    assert ex <= 1e-8 and eu <= 1e-8, (ex, eu)


@pytest.mark.parametrize('points', [1, 64])
def test_both_addressing_forms_of_the_fill_against_the_oracle(points, monkeypatch):
    """points = 1: a one-point TPWL table, every QP is single-region and every fill reads the Toeplitz generators (the counter shows one
    condensation per rollout, the rest reuse it).  points = 64 (the C2 table): the counter reports fewer single-region QPs than there are
    QPs, so general condensations -- and fills from the staged packed rows -- occur.  The first two rollouts of each against oracle.gusto
    around the numpy statement of the lean interior point: equal SCP iteration counts, trajectories within 1e-7."""
    import bench
    import workloads as wl
    from oracle import gusto as ogusto
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2(P=1) if points == 1 else wl.diamond_c2()
    B = 8
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    if points == 1:        # (the characteristic values of a one-point table are zero: scale with those of the 64-point table of C2)
        xc, fc = bench.build_model(wl.diamond_c2(), 1354)[1].get_characteristic_vals()
    g = plan(monkeypatch, 1, w, gm, xc, fc, x0, u_init, x_init, z)
    g.solve_batch(x0, u_init, x_init, z=z)
    assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0
    single, qps = int(g.kernel_info['single_region_qps']), int(g.iters.sum())
    print('%d-point table: %d single-region condensations, %d QPs in %d rollouts' % (points, single, qps, B))
    if points == 1:
        assert single == B, single
    else:
        assert B <= single < qps, (single, qps)
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    for b in range(2):
        xe, ue, ze, tr = ogusto.solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], w['N'], w['dt'], w['Qz'], w['R'], x0[b], u_init[b], x_init[b],
                                      z=z[b], U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3,
                                      qp_solver='condensed_ipm', max_gusto_iters=5)
        ex, eu = rel(g.xopt[b], xe), rel(g.uopt[b], ue)
        print('%d-point table, rollout %d against oracle.gusto: rel x %.2e u %.2e, SCP iterations %d / %d' % (points, b, ex, eu, int(g.iters[b]), len(tr)))
        assert int(g.iters[b]) == len(tr)
        assert ex <= 1e-7 and eu <= 1e-7, (ex, eu)
