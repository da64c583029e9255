"""The products with the condensed map G of the lean interior points (ql::gT_times in csrc/locp_lean.h).  In the
half-size fixed-horizon kernel (<4, 60, 4, 50, 50, 4>, the only layout that keeps the Toeplitz generators of a single-region QP) a
product G^T y loads the thread's generator entries once and runs every row pass from registers and LDS; the FMAs keep their operands,
their chains and their place in them.  A plan created under SRH_LEAN_NO_TOEPLITZ=1 condenses every QP by the general recursion and its
products read the packed rows: EQUAL results of the two plans, and the suite's 1e-7 against oracle.gusto around the numpy statement of
the lean interior point with equal SCP iteration counts, are what every case asks for.

WHICH CASES RUN THE REGISTER PATH: the N = 50 half-size cases (one-point table: every product of every QP; 64-point table: both kinds
of QP in one solve) and the 600-rollout case.  A row of stage j has ceil((100 - 2 j) / 8) trips of 8 lanes, so every trip count from 13
(one remainder trip behind three blocks of four) down to 1 occurs inside each of them, as does the last pass that is not full (200 rows
= 6 x 32 + 8), on the front's two waves (GRP = 16 in the early stopping test) and on the whole workgroup.

EVERYTHING ELSE IS A REGRESSION GUARD on loops this change leaves alone; there the two plans differ in the condensation only.  The
shorter horizons (N = 9: the smallest of the box kernels, NP = 18 > 16; 12; 16; 20; 28) run the run-time-horizon kernel
<4, 60, 4, 0, 0, 0>: fixed-horizon instantiations exist at N = 50 only (lean.hip: SRH_LEAN_VARIANTS).  The full-size kernels -- C2 on
<4, 60, 4, 50, 7, 4>, C5 with its eight inputs on <8, 60, 1, 50, 24, 0> -- and the general-row form keep no generators, so the M = 8 and
L2-head-plus-LDS cases the issue lists cannot reach the register path.  Every case asserts through kernel_info['kernel'] which kernel
answered and that it is not the one-wave form (NST = -1)."""
import numpy as np
import pytest

from test_gusto_bench_shapes_gpu import problem, rel
from test_lean_half_newton_gpu import FULL, HALF

pytestmark = pytest.mark.gpu

CAP = 5
FIELDS = ('xopt', 'uopt', 'zopt', 'iters', 'status', 'costs')
RUNTIME = (4, 60, 4, 0, 0, 0)
_cache = {}


def shape(name, N=50, points=64):
    """(workload, model, scales, 8 rollouts), built once per shape and left unchanged"""
    key = (name, N, points)
    if key not in _cache:
        import bench
        import workloads as wl
        if name == 'c5':
            w = wl.trunk_c5()
            tip, seed = w['tip_node'], 9
        else:
            w, tip, seed = wl.diamond_c2(N=N, P=points), 1354, 2
        gm, xc, fc, x0, u_init, x_init, z = problem(w, 8, seed, tip)
        if points == 1:       # the characteristic values of a one-point table are zero: scale with those of the 64-point table of C2
            xc, fc = bench.build_model(wl.diamond_c2(), 1354)[1].get_characteristic_vals()
        _cache[key] = (w, gm, xc, fc, x0, u_init, x_init, z)
    return _cache[key]


def make(monkeypatch, prob, B, half=None, no_toeplitz=False, no_box=False):
    """A resident plan for the first B rollouts of `prob`; the knobs are read when the plan is created"""
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    w, gm, xc, fc, x0, u_init, x_init, z = prob
    for var, val in (('SRH_LEAN_HALF', None if half is None else str(half)), ('SRH_LEAN_NO_TOEPLITZ', '1' if no_toeplitz else None),
                     ('SRH_QP_NO_BOX', '1' if no_box else None)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)
    X = Polyhedron(w['XA'], w['Xb']) if w['XA'] is not None else None
    g = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0[:B], u_init[:B], x_init[:B], z=z[:B], U=Polyhedron(w['UA'], w['Ub']), X=X,
              x_char=xc, f_char=fc, convg_thresh=1e-3, batch=B, max_trace=0, max_gusto_iters=CAP, first_solve_cap=CAP)
    for var in ('SRH_LEAN_HALF', 'SRH_LEAN_NO_TOEPLITZ', 'SRH_QP_NO_BOX'):
        monkeypatch.delenv(var, raising=False)
    return g


def solve(g, prob, B):
    w, gm, xc, fc, x0, u_init, x_init, z = prob
    g.solve_batch(x0[:B], u_init[:B], x_init[:B], z=z[:B])
    return {f: np.array(getattr(g, f)).copy() for f in FIELDS}


def box_kernel(info, lean=None):
    """a lean box kernel answered (not the fused kernel, not the one-wave form), the expected one where the case names it"""
    if info['family'] != 'lean':
        pytest.skip('the lean path refuses this size: %s' % (info,))
    assert info['kernel'] == 'lean<%d, %d, %d, %d, %d, %d>' % info['lean'] and info['lean'][3] != -1, info
    if lean is not None:
        assert info['lean'] == lean, info


def assert_identical(a, b, what):
    for f in FIELDS:
        if a[f].dtype.kind == 'f':
            print('%s: %s max |difference| %g' % (what, f, float(np.abs(a[f] - b[f]).max())))
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


def both_paths(monkeypatch, name, N, points, half, lean, no_box=False):
    """8 rollouts under the default plan and under SRH_LEAN_NO_TOEPLITZ=1, solved once per session and shared"""
    key = ('paths', name, N, points, half, no_box)
    if key not in _cache:
        prob = shape(name, N, points)
        res = {}
        for knob in (False, True):
            g = make(monkeypatch, prob, 8, half=half, no_toeplitz=knob, no_box=no_box)
            box_kernel(g.kernel_info, lean)
            out = solve(g, prob, 8)
            info = g.kernel_info
            assert info['handed_over'] == 0, info
            print('%s N %d, %d table points, half %s, no Toeplitz %d: %s, SCP iterations %s, single-region QPs %d' %
                  (name, N, points, half, knob, info['kernel'], out['iters'].tolist(), info['single_region_qps']))
            res[knob] = (out, int(info['single_region_qps']))
        _cache[key] = res
    return _cache[key]


def oracle(prob, b):
    from oracle import gusto as ogusto
    w, gm, xc, fc, x0, u_init, x_init, z = prob
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    X = (w['XA'], w['Xb']) if w['XA'] is not None else None
    return ogusto.solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], w['N'], w['dt'], w['Qz'], w['R'], x0[b], u_init[b], x_init[b], z=z[b],
                        U=(w['UA'], w['Ub']), X=X, x_char=xc, f_char=fc, convg_thresh=1e-3, qp_solver='condensed_ipm', max_gusto_iters=CAP)


def assert_oracle(got, prob, rollouts, what):
    """equal SCP iteration counts and the suite's 1e-7 (tests/test_lean_gpu.py, test_lean_toeplitz_gpu.py, test_ipm_early_stop_gpu.py)"""
    for b in rollouts:
        xe, ue, ze, tr = oracle(prob, b)
        ex, eu = rel(got['xopt'][b], xe), rel(got['uopt'][b], ue)
        print('%s rollout %d against oracle.gusto: rel x %.2e u %.2e, SCP iterations %d / %d' % (what, b, ex, eu, int(got['iters'][b]), len(tr)))
        assert int(got['iters'][b]) == len(tr)
        assert ex <= 1e-7 and eu <= 1e-7, (ex, eu)


# (N, half, the instantiation that must answer): the half-size and the full-size fixed-horizon kernels at N = 50, the run-time horizon below
HORIZONS = [(9, None, RUNTIME), (12, None, RUNTIME), (16, None, RUNTIME), (20, None, RUNTIME), (28, None, RUNTIME), (50, 1, HALF), (50, 0, FULL)]


@pytest.mark.parametrize('points', [1, 64])
@pytest.mark.parametrize('N,half,lean', HORIZONS)
def test_generator_path_equals_packed_row_path(N, half, lean, points, monkeypatch):
    """One-point table: every QP is single-region, every product of the default plan reads the generators.  C2 table (64 points):
    single-region and general QPs in one solve.  The default plan and the SRH_LEAN_NO_TOEPLITZ=1 plan give identical arrays; the
    knob plan never took the single-region path, the default plan at N = 50 at least once per rollout.  Only (50, half-size) runs the
    register path; the other rows compare the two condensations on unchanged product loops (module docstring)."""
    res = both_paths(monkeypatch, 'c2', N, points, half, lean)
    assert_identical(res[False][0], res[True][0], 'N %d, %d points, half %s' % (N, points, half))
    assert res[True][1] == 0, res[True][1]
    if N == 50:               # (the first QP of every C2 rollout is single-region: tests/test_lean_toeplitz_gpu.py asserts the premise)
        assert res[False][1] >= 8, res[False][1]


@pytest.mark.parametrize('points', [1, 64])
@pytest.mark.parametrize('N,half,lean', HORIZONS)
def test_horizons_against_the_oracle(N, half, lean, points, monkeypatch):
    """the first two rollouts of every case above against oracle.gusto"""
    got = both_paths(monkeypatch, 'c2', N, points, half, lean)[False][0]
    assert_oracle(got, shape('c2', N, points), (0, 1), 'N %d, %d points, half %s' % (N, points, half))


def test_eight_inputs_c5(monkeypatch):
    """C5 (Trunk, n_u = 8, no state rows), lean<8, 60, 1, 50, 24, 0>, a full-size kernel: it keeps no generators, its products are the
    unchanged loops (rows of the stages >= 24 from LDS).  Regression guard: single-region condensation against the general one, and two
    rollouts against the oracle."""
    res = both_paths(monkeypatch, 'c5', 50, 64, None, (8, 60, 1, 50, 24, 0))
    assert_identical(res[False][0], res[True][0], 'C5')
    assert res[False][1] >= 8 and res[True][1] == 0, (res[False][1], res[True][1])
    assert_oracle(res[False][0], shape('c5'), (0, 1), 'C5')


def test_general_row_form(monkeypatch):
    """SRH_QP_NO_BOX=1: the rows keep ql::ipm's general handling (GX = 0) on a run-time-horizon kernel, whose Newton front runs on the
    whole workgroup (GRP = 0) with the unchanged loops.  Regression guard at C2, N = 50: the two condensations give equal results, two
    rollouts against the oracle."""
    res = both_paths(monkeypatch, 'c2', 50, 64, None, None, no_box=True)
    prob = shape('c2', 50, 64)
    g = make(monkeypatch, prob, 8, no_box=True)
    assert g.kernel_info['lean'][2] == 0, g.kernel_info
    assert_identical(res[False][0], res[True][0], 'general rows')
    assert_oracle(res[False][0], prob, (0, 1), 'general rows')


def test_600_rollouts_three_times_and_their_first_8_alone(monkeypatch):
    """600 C2 rollouts on the default plan (above the CU count: the half-size workgroup, two per CU) three times: identical arrays.
    Their first 8 on a plan of their own -- on the same kernel, SRH_LEAN_HALF=1: a batch of 8 would pick the full-size workgroup, whose
    sums differ in rounding -- equal those rows bit for bit: no product reads another rollout's registers, rows or generators."""
    import workloads as wl
    w = wl.diamond_c2()
    prob = (w,) + tuple(problem(w, 600, 2, 1354))
    g = make(monkeypatch, prob, 600)
    box_kernel(g.kernel_info, HALF)
    runs = [solve(g, prob, 600) for _ in range(3)]
    for k in (1, 2):
        assert_identical(runs[k], runs[0], 'solve %d against solve 0' % k)
    g8 = make(monkeypatch, prob, 8, half=1)
    box_kernel(g8.kernel_info, HALF)
    first = solve(g8, prob, 8)
    for f in FIELDS:
        assert np.array_equal(first[f], runs[0][f][:8]), f
