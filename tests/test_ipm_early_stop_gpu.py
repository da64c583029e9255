"""The lean interior points test convergence BEFORE they build the predictor's Newton system (csrc/ipm_rule.h: ipm::may_converge /
ipm::converged; ql::converged_early in csrc/locp_lean.h), as oracle/condensed_ipm.py:286-292 does: the final pass of every QP no longer
fills, factors and solves a system whose only use was to find the iterate converged.  The dual residual of the early test is the very
product and maximum the Newton front takes, so no verdict moves: against SRH_IPM_LATE_STOP=1 (read when a plan's constants are built:
the former order) every output is EQUAL -- trajectories, SCP iteration counts, status, costs -- on each lean form at its smallest
shape: the half-size workgroup (C2, <4, 60, 4, 50, 50, 4>), the full-size workgroup at C2 (SRH_LEAN_HALF=0) and at C5 (n_u = 8), the
one-wave form of the drivers' horizons (N = 3 without state rows, N = 5 with them; one rollout and eight), the general-row form, and a
QP without inequality rows.  The one place the two orders may differ -- a factorisation that breaks down at an iterate that already passes the strict test --
has no knob in the suite.  Solves capped at 5 SCP iterations."""
import numpy as np
import pytest

from test_gusto_bench_shapes_gpu import problem, rel
from test_lean_half_newton_gpu import FIELDS, FULL, HALF

pytestmark = pytest.mark.gpu

CAP = 5
_cache = {}


def shape(name):
    """(workload, tip node, seed, 8 rollouts of it), built once per shape"""
    if name not in _cache:
        import workloads as wl
        if name == 'c2':
            w, tip, seed = wl.diamond_c2(), 1354, 2
        elif name == 'c5':
            w = wl.trunk_c5()
            tip, seed = w['tip_node'], 9
        elif name == 'n3':
            w, tip, seed = wl.diamond_c2(N=3, dt=0.1, with_X=False), 1354, 2
        elif name == 'n5':
            w, tip, seed = wl.diamond_c2(N=5, dt=0.05, with_X=True), 1354, 2
        else:
            raise KeyError(name)
        _cache[name] = (w,) + tuple(problem(w, 8, seed, tip))
    return _cache[name]


def make(monkeypatch, name, B, late, half=None, rows=True, no_box=False, **kw):
    """A plan for the first B rollouts of `name`, its constants built under SRH_IPM_LATE_STOP=late (None: unset)"""
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    w, gm, xc, fc, x0, u_init, x_init, z = shape(name)
    if late is None:
        monkeypatch.delenv('SRH_IPM_LATE_STOP', raising=False)
    else:
        monkeypatch.setenv('SRH_IPM_LATE_STOP', str(late))
    if half is None:
        monkeypatch.delenv('SRH_LEAN_HALF', raising=False)
    else:
        monkeypatch.setenv('SRH_LEAN_HALF', str(half))
    if no_box:
        monkeypatch.setenv('SRH_QP_NO_BOX', '1')
    else:
        monkeypatch.delenv('SRH_QP_NO_BOX', raising=False)
    U = Polyhedron(w['UA'], w['Ub']) if rows else None
    X = Polyhedron(w['XA'], w['Xb']) if (rows and w['XA'] is not None) else None
    return GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0[:B], u_init[:B], x_init[:B], z=z[:B], U=U, X=X, x_char=xc, f_char=fc,
                 convg_thresh=1e-3, batch=B, max_trace=0, max_gusto_iters=CAP, first_solve_cap=CAP, **kw)


def solve(g, name, B):
    w, gm, xc, fc, x0, u_init, x_init, z = shape(name)
    g.solve_batch(x0[:B], u_init[:B], x_init[:B], z=z[:B])
    out = {f: np.array(getattr(g, f)).copy() for f in FIELDS}
    out['costs'] = np.array(g.costs).copy()
    return out


def both_orders(monkeypatch, name, B, half=None, lean=None, rows=True, no_box=False):
    """the same B rollouts under the early test and under SRH_IPM_LATE_STOP=1 (each solved once per session, shared, left unchanged)"""
    key = ('orders', name, B, half, rows, no_box)
    if key not in _cache:
        res = {}
        for late in (None, 1):
            g = make(monkeypatch, name, B, late, half=half, rows=rows, no_box=no_box)
            info = g.kernel_info
            assert info['family'] == 'lean', info
            if lean is not None:
                assert info['lean'] == lean, info
            assert info['ipm_late_stop'] == (1 if late else 0), info
            res[late] = solve(g, name, B)
            assert g.kernel_info['handed_over'] == 0, g.kernel_info
            print('%s, %d rollouts, late stop %s: kernel %s, SCP iterations %s, status %s' %
                  (name, B, late, info['kernel'], res[late]['iters'].tolist(), res[late]['status'].tolist()))
        _cache[key] = res
    return _cache[key]


def assert_equal(res):
    early, late = res[None], res[1]
    for f in FIELDS + ('costs',):
        assert np.array_equal(early[f], late[f]), (f, float(np.abs(np.asarray(early[f], dtype=float) - late[f]).max()))
    assert (early['status'] == 0).all(), early['status']


def test_half_size_workgroup_c2(monkeypatch):
    """8 C2 rollouts (N = 50, r = 30, U box + X box) on the half-size kernel: both condensation kinds, cold first QPs and warm later ones"""
    assert_equal(both_orders(monkeypatch, 'c2', 8, half=1, lean=HALF))


def test_full_size_workgroup_c2(monkeypatch):
    """the same 8 rollouts with SRH_LEAN_HALF=0: ql::ipm_box, eight waves, the front on four of them"""
    assert_equal(both_orders(monkeypatch, 'c2', 8, half=0, lean=FULL))


def test_full_size_workgroup_c5(monkeypatch):
    """8 rollouts of C5 (Trunk, n_u = 8, no state rows): ql::ipm_box with the kept G^T g_y of problems without state rows"""
    assert_equal(both_orders(monkeypatch, 'c5', 8))


@pytest.mark.parametrize('name,B', [('n3', 1), ('n3', 8), ('n5', 1), ('n5', 8)])
def test_one_wave_form(name, B, monkeypatch):
    """the drivers' horizons (N = 3 without X rows, N = 5 with them): ql::ipm_wave, one rollout and a batch of 8"""
    assert_equal(both_orders(monkeypatch, name, B))


def test_general_row_form(monkeypatch):
    """SRH_QP_NO_BOX=1 (read when the constants are built): the rows keep ql::ipm's general handling, lean<4, 60, 0, ..>; N = 5 with X rows"""
    res = both_orders(monkeypatch, 'n5', 8, no_box=True, lean=(4, 60, 0, 0, 0, 0))
    assert_equal(res)


def test_qp_without_inequality_rows(monkeypatch):
    """no U, no X: the QP is solved by its starting system (ipm::verdict_no_rows) and never reaches a predictor pass -- unchanged"""
    res = {}
    for late in (None, 1):
        g = make(monkeypatch, 'n3', 2, late, rows=False)
        res[late] = solve(g, 'n3', 2)
        print('no rows, late stop %s: %s, SCP iterations %s' % (late, g.kernel_info, res[late]['iters'].tolist()))
    assert_equal(res)


def test_qp_converged_at_iteration_0_of_a_warm_start(monkeypatch):
    """keep_solver_state=True and the same problem solved twice: the first QP of the second solve starts from the converged minimiser and
    multipliers of the first solve's last QP -- the early test can hold in the very first predictor pass, before any system of that QP
    exists.  Both solves equal the late order's."""
    res = {}
    for late in (None, 1):
        g = make(monkeypatch, 'c2', 8, late, half=1, keep_solver_state=True)
        assert g.kernel_info['lean'] == HALF and g.kernel_info['ipm_late_stop'] == (1 if late else 0), g.kernel_info
        res[late] = [solve(g, 'c2', 8) for _ in range(2)]
        assert g.kernel_info['handed_over'] == 0, g.kernel_info
    for k in range(2):
        assert_equal({None: res[None][k], 1: res[1][k]})


def oracle(name, b):
    from oracle import gusto as ogusto
    w, gm, xc, fc, x0, u_init, x_init, z = shape(name)
    model = dict(w['tab'], w_q=1.0, w_v=0.0)
    X = (w['XA'], w['Xb']) if w['XA'] is not None else None
    return ogusto.solve(model, w['Ad'], w['Bd'], w['dd'], w['H'], w['N'], w['dt'], w['Qz'], w['R'], x0[b], u_init[b], x_init[b], z=z[b],
                        U=(w['UA'], w['Ub']), X=X, x_char=xc, f_char=fc, convg_thresh=1e-3, qp_solver='condensed_ipm', max_gusto_iters=CAP)


@pytest.mark.parametrize('name,b', [('c2', b) for b in range(8)] + [('n5', 0), ('n5', 1)])
def test_against_the_oracle(name, b, monkeypatch):
    """oracle.gusto around the numpy statement of the lean interior point (which tests before the system): equal SCP iteration counts,
    trajectories within the 1e-7 of tests/test_lean_half_newton_gpu.py / test_lean_toeplitz_gpu.py"""
    got = both_orders(monkeypatch, name, 8, half=1 if name == 'c2' else None, lean=HALF if name == 'c2' else None)[None]
    xe, ue, ze, tr = oracle(name, b)
    ex, eu = rel(got['xopt'][b], xe), rel(got['uopt'][b], ue)
    print('%s rollout %d against oracle.gusto: rel x %.2e u %.2e, SCP iterations %d / %d' % (name, b, ex, eu, int(got['iters'][b]), len(tr)))
    assert int(got['iters'][b]) == len(tr)
    assert ex <= 1e-7 and eu <= 1e-7, (ex, eu)


@pytest.mark.parametrize('value', ['0', '2', 'yes', ''])
def test_only_the_value_1_keeps_the_late_order(value, monkeypatch):
    """kernel_info reports the knob; any value but 1 counts as 0 (as an illegal SRH_LEAN_ROSTER code counts as 0) and gives the default's
    results"""
    ref = both_orders(monkeypatch, 'n5', 8)[None]
    g = make(monkeypatch, 'n5', 8, value)
    assert g.kernel_info['ipm_late_stop'] == 0, g.kernel_info
    got = solve(g, 'n5', 8)
    for f in FIELDS + ('costs',):
        assert np.array_equal(got[f], ref[f]), f
