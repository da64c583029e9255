"""The single-region condensation of the lean kernels (ql::condense_single): when every stage of a QP's horizon lies
in ONE TPWL region the condensed matrix G is block-Toeplitz and is built from one chain of N products -- the recursion restricted to
the columns of output stage N -- and expanded into the packed rows, instead of the full adjoint recursion.  Each number goes through
the same MFMA k-steps in the same order as in the general recursion, so the packed G must have the SAME BITS.  A wrong G does not fail
loudly (the SCP loop converges on an inexact model anyway), so these cases ask for EQUALITY against a plan created under
SRH_LEAN_NO_TOEPLITZ=1 (general recursion always), and they check through `kernel_info['single_region_qps']` that the path under test
actually ran (and, where the case is about it, that it did not)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ('xopt', 'uopt', 'zopt', 'iters', 'status', 'costs')


def rel(a, b):
    return float(np.abs(a - b).max() / max(1e-12, np.abs(b).max()))


def regions(w, X):
    """Region of every stage k = 0 .. N - 1 of the trajectories X (B x (N + 1) x n) by the oracle's nearest-point rule."""
    from oracle import tpwl as otpwl
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    return np.stack([otpwl.nearest_points(model, x[:w['N']]) for x in X])


def uniform(idx):
    return (idx == idx[:, :1]).all(axis=1)


def plan(monkeypatch, knob, half, w, gm, xc, fc, x0, u_init, x_init, z, cap=5, with_X=True):
    """A resident GuSTO plan for the batch, created with / without SRH_LEAN_NO_TOEPLITZ=1 (read when the plan is created)."""
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    monkeypatch.setenv('SRH_LEAN_HALF', '1' if half else '0')
    if knob:
        monkeypatch.setenv('SRH_LEAN_NO_TOEPLITZ', '1')
    else:
        monkeypatch.delenv('SRH_LEAN_NO_TOEPLITZ', raising=False)
    X = Polyhedron(w['XA'], w['Xb']) if with_X else None
    g = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0, u_init, x_init, z=z, U=Polyhedron(w['UA'], w['Ub']), X=X, x_char=xc, f_char=fc,
              convg_thresh=1e-3, batch=x0.shape[0], max_trace=0, max_gusto_iters=cap, first_solve_cap=cap)
    monkeypatch.delenv('SRH_LEAN_NO_TOEPLITZ', raising=False)
    return g


def result(g):
    return {f: np.array(getattr(g, f)).copy() for f in FIELDS}


def assert_identical(a, b, what):
    for f in FIELDS:
        if a[f].dtype.kind == 'f':
            print('%s: %s max |difference| %g' % (what, f, float(np.abs(a[f] - b[f]).max())))
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.mark.parametrize('half', [1, 0])
def test_single_region_condensation_equals_the_general_one_at_c2(half, monkeypatch):
    """BASELINE C2, 64 rollouts, solves capped at 5 SCP iterations, on the half-size (<4, 60, 4, 50, 50, 4>) and the full-size
    (<4, 60, 4, 50, 7, 4>) lean kernel.  Premise (oracle): every initial guess lies in one region -- the first QP of every rollout takes
    the single-region path -- and the final trajectory of at least one rollout crosses regions.  Then: all results of the normal plan
    and of the SRH_LEAN_NO_TOEPLITZ=1 plan are identical arrays; the normal plan counted at least 64 single-region QPs and fewer than
    there were QPs (both paths ran), the knob plan none."""
    import workloads as wl
    from test_gusto_bench_shapes_gpu import problem, oracle_solve
    w = wl.diamond_c2()
    B = 64
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    assert uniform(regions(w, x_init)).all()
    crosses = 0
    for b in range(8):
        xe = oracle_solve(w, xc, fc, x0[b], u_init[b], x_init[b], z[b], 5)[0]
        crosses += int(not uniform(regions(w, xe[None]))[0])
    print('oracle: %d of the first 8 final trajectories cross regions' % crosses)
    assert crosses >= 1
    res, single = {}, {}
    for knob in (False, True):
        g = plan(monkeypatch, knob, half, w, gm, xc, fc, x0, u_init, x_init, z)
        assert g.kernel_info['lean'] == ((4, 60, 4, 50, 50, 4) if half else (4, 60, 4, 50, 7, 4)), g.kernel_info
        g.solve_batch(x0, u_init, x_init, z=z)
        res[knob], single[knob] = result(g), int(g.kernel_info['single_region_qps'])
    qps = int(res[False]['iters'].sum())
    print('half %d: single-region QPs %d of %d SCP iterations (knob plan: %d)' % (half, single[False], qps, single[True]))
    assert_identical(res[False], res[True], 'C2 half %d' % half)
    assert B <= single[False] < qps, (single[False], qps)
    assert single[True] == 0, single[True]


def test_one_point_table_every_qp_is_single_region(monkeypatch):
    """A TPWL table with ONE point (an LTI model through the TPWL plan): every QP of every solve is single-region; the first one
    condenses by the restricted recursion, the later ones keep its G (region sequence unchanged).  Equal to the knob plan bit for bit
    (both kernel sizes), and to oracle.gusto.solve around the numpy statement of the lean interior point within 1e-7 -- the bound
    tests/test_lean_gpu.py uses for the lean kernel against that statement."""
    import bench
    import workloads as wl
    from oracle import gusto as ogusto
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2(P=1)
    B = 8
    gm, _, _, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    # (the characteristic values of a one-point table are zero: scale with those of the 64-point table of C2)
    xc, fc = bench.build_model(wl.diamond_c2(), 1354)[1].get_characteristic_vals()
    assert (regions(w, x_init) == 0).all()
    for half in (1, 0):
        res, single = {}, {}
        for knob in (False, True):
            g = plan(monkeypatch, knob, half, w, gm, xc, fc, x0, u_init, x_init, z)
            assert g.kernel_info['lean'] == ((4, 60, 4, 50, 50, 4) if half else (4, 60, 4, 50, 7, 4)), g.kernel_info
            g.solve_batch(x0, u_init, x_init, z=z)
            assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0
            res[knob], single[knob] = result(g), int(g.kernel_info['single_region_qps'])
        assert_identical(res[False], res[True], 'one-point table, half %d' % half)
        assert single[False] == B and single[True] == 0, single          # one condensation per rollout, the rest reuse it
        model = dict(w['tab'], w_q=1.0, w_v=0.0)
        for b in range(2):
            xe, ue, ze, tr = ogusto.solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], w['N'], w['dt'], w['Qz'], w['R'], x0[b], u_init[b],
                                          x_init[b], z=z[b], U=(w['UA'], w['Ub']), X=(w['XA'], w['Xb']), x_char=xc, f_char=fc,
                                          convg_thresh=1e-3, qp_solver='condensed_ipm', max_gusto_iters=5)
            ex, eu = rel(res[False]['xopt'][b], xe), rel(res[False]['uopt'][b], ue)
            print('one-point table, half %d, rollout %d against oracle.gusto: rel x %.2e u %.2e, SCP iterations %d / %d'
                  % (half, b, ex, eu, int(res[False]['iters'][b]), len(tr)))
            assert int(res[False]['iters'][b]) == len(tr)
            assert ex <= 1e-7 and eu <= 1e-7, (ex, eu)


def test_detection_edges_keep_the_general_path(monkeypatch):
    """Horizons that are NOT single-region must not take the restricted recursion, wherever the odd stage sits.  C2, 8 rollouts:
    0, 1 as they are (single-region); 2, 3 with x0 scaled by 20 -- by the oracle the zero-input guess then starts in another region and
    is back in region 0 from stage 1 on (a change at the first stage that comes from the dynamics); 4, 5 with stage 0 of the guess, and
    6, 7 with stage N - 1 of the guess (the last one the region sequence has) replaced by a far table point: the only change at the
    first / at the last stage, constructed.  Premises asserted with the oracle's nearest points.  With one QP per rollout
    (max_gusto_iters = 0) the counter shows exactly the two unmodified rollouts; with the cap of 5 all results equal the knob plan's."""
    import workloads as wl
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2()
    N, r = w['N'], w['r']
    B = 8
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    x0, x_init = x0.copy(), x_init.copy()
    x0[2:4] *= 20.0
    from oracle import tpwl as otpwl
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    for b in (2, 3):
        x_init[b] = otpwl.rollout(model, w['Ad'], w['Bd'], w['dd'], x0[b], np.zeros((N, w['m'])))
    far = np.concatenate((np.zeros(r), w['tab']['q'][5]))
    x_init[4:6, 0] = far
    x_init[6:8, N - 1] = far
    idx = regions(w, x_init)
    assert uniform(idx[:2]).all()
    for b in (2, 3, 4, 5):
        assert idx[b, 0] != idx[b, 1] and (idx[b, 1:] == idx[b, 1]).all(), (b, idx[b])
    for b in (6, 7):
        assert idx[b, N - 1] != idx[b, 0] and (idx[b, :N - 1] == idx[b, 0]).all(), (b, idx[b])
    for half in (1, 0):
        g = plan(monkeypatch, False, half, w, gm, xc, fc, x0, u_init, x_init, z, cap=0)
        g.solve_batch(x0, u_init, x_init, z=z)
        assert (g.iters == 1).all(), g.iters
        assert int(g.kernel_info['single_region_qps']) == 2, g.kernel_info
        res = {}
        for knob in (False, True):
            g = plan(monkeypatch, knob, half, w, gm, xc, fc, x0, u_init, x_init, z)
            g.solve_batch(x0, u_init, x_init, z=z)
            res[knob] = result(g)
        assert_identical(res[False], res[True], 'detection edges, half %d' % half)


def test_repeated_solves_on_one_plan_are_identical(monkeypatch):
    """Three solve_batch calls on one half-size plan, 600 rollouts (pairs share a CU): identical arrays and the same counter each time
    -- neither the marker of a kept condensation nor the counter carries state across launches that changes a result."""
    import workloads as wl
    from test_gusto_bench_shapes_gpu import problem
    w = wl.diamond_c2()
    B = 600
    gm, xc, fc, x0, u_init, x_init, z = problem(w, B, 2, 1354)
    g = plan(monkeypatch, False, 1, w, gm, xc, fc, x0, u_init, x_init, z)
    assert g.kernel_info['lean'] == (4, 60, 4, 50, 50, 4), g.kernel_info
    runs = []
    for _ in range(3):
        g.solve_batch(x0, u_init, x_init, z=z)
        runs.append((result(g), int(g.kernel_info['single_region_qps'])))
    print('600 rollouts: single-region QPs per solve', [s for _, s in runs], 'of', int(runs[0][0]['iters'].sum()))
    for k in (1, 2):
        assert_identical(runs[k][0], runs[0][0], 'solve %d against solve 0' % k)
        assert runs[k][1] == runs[0][1]
    assert runs[0][1] >= B
