"""The row roster of the half-size lean workgroup's tile factorisation (ql::ipm_box4 / ql::tile_cholesky_set, instantiation
<4, 60, 4, 50, 50, 4>): under SRH_LEAN_ROSTER=<code> waves 2 and 3 work in some tile rows of the factorisation beside or
behind their Newton front.  Every roster deals the same MFMA products to other waves and every tile still receives its updates in
ascending row order, so K's factor and with it every output is bit-identical: the cases ask for EQUALITY between codes, between runs,
between batch sizes and between the two places of the serial wave.  BASELINE C2 (KT = 7: legal codes 1 .. 5 of either sign), solves
capped at 5 SCP iterations.  The counter protocol itself is replayed on the host in tests/test_lean_roster_cpu.py."""
import numpy as np
import pytest

from test_lean_half_newton_gpu import FIELDS, HALF, result

pytestmark = pytest.mark.gpu

_cache = {}


def problem8():
    """8 rollouts of C2 and the 600 they are the first rows of (built once)"""
    if 'p' not in _cache:
        import workloads as wl
        from test_gusto_bench_shapes_gpu import problem
        w = wl.diamond_c2()
        _cache['p'] = (w,) + tuple(problem(w, 600, 2, 1354))
    return _cache['p']


def plan(monkeypatch, code, B, serial_wave=None):
    """A half-size plan for the first B rollouts, created under SRH_LEAN_ROSTER=code (None: the default) and, when given,
    SRH_LEAN_SERIAL_WAVE; both are read when the plan is created."""
    from sofacontrol_amd.scp.gusto import GuSTO
    from sofacontrol_amd.utils import Polyhedron
    w, gm, xc, fc, x0, u_init, x_init, z = problem8()
    monkeypatch.setenv('SRH_LEAN_HALF', '1')
    if code is None:
        monkeypatch.delenv('SRH_LEAN_ROSTER', raising=False)
    else:
        monkeypatch.setenv('SRH_LEAN_ROSTER', str(code))
    if serial_wave is None:
        monkeypatch.delenv('SRH_LEAN_SERIAL_WAVE', raising=False)
    else:
        monkeypatch.setenv('SRH_LEAN_SERIAL_WAVE', str(serial_wave))
    g = GuSTO(gm, w['N'], w['dt'], w['Qz'], w['R'], x0[:B], u_init[:B], x_init[:B], z=z[:B], U=Polyhedron(w['UA'], w['Ub']),
              X=Polyhedron(w['XA'], w['Xb']), x_char=xc, f_char=fc, convg_thresh=1e-3, batch=B, max_trace=0, max_gusto_iters=5, first_solve_cap=5)
    assert g.kernel_info['lean'] == HALF, g.kernel_info
    return g


def solve(g, B):
    w, gm, xc, fc, x0, u_init, x_init, z = problem8()
    g.solve_batch(x0[:B], u_init[:B], x_init[:B], z=z[:B])
    assert (g.status == 0).all() and g.kernel_info['handed_over'] == 0, g.kernel_info
    return result(g)


def code0(monkeypatch):
    """the 8 rollouts under code 0 (solved once, shared and left unchanged)"""
    if 'c0' not in _cache:
        g = plan(monkeypatch, 0, 8)
        res = solve(g, 8)
        assert g.kernel_info['lean_roster'] == 0
        single, qps = int(g.kernel_info['single_region_qps']), int(g.iters.sum())
        print('8 rollouts, code 0: %d single-region condensations in %d QPs' % (single, qps))
        assert 8 <= single < qps, (single, qps)              # both condensation kinds occur
        _cache['c0'] = res
    return _cache['c0']


@pytest.mark.parametrize('code', [0, 1, 3, 5, -1, -2, -5])
def test_codes_agree(code, monkeypatch):
    """8 rollouts under SRH_LEAN_ROSTER=code: every output array equal to code 0's, nothing handed over, the code reported"""
    ref = code0(monkeypatch)
    g = plan(monkeypatch, code, 8)
    got = solve(g, 8)
    assert g.kernel_info['lean_roster'] == code, g.kernel_info
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), (code, f)


def test_an_out_of_range_code_is_ignored(monkeypatch):
    """KT = 7: the legal range is 1 .. 5; SRH_LEAN_ROSTER=6 counts as 0"""
    ref = code0(monkeypatch)
    g = plan(monkeypatch, 6, 8)
    got = solve(g, 8)
    assert g.kernel_info['lean_roster'] == 0, g.kernel_info
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), f


def test_co_resident_workgroups_and_the_serial_wave_on_wave_2(monkeypatch):
    """The default code, 600 rollouts (more than CUs: two workgroups per CU) solved three times: every array identical; the first 8
    solved alone equal their rows of the 600; the same 600 under SRH_LEAN_SERIAL_WAVE=1 (a workgroup that finds its wave 0 in the second
    wave slot runs its serial chain on wave 2, and the roster's waves are counted from there) equal the run without it."""
    B, S = 600, 8
    g = plan(monkeypatch, None, B)
    runs = [solve(g, B) for _ in range(3)]
    for k in (1, 2):
        for f in FIELDS:
            assert np.array_equal(runs[k][f], runs[0][f]), (k, f)
    gs = plan(monkeypatch, None, S)
    small = solve(gs, S)
    assert gs.kernel_info['lean_roster'] == g.kernel_info['lean_roster']
    for f in FIELDS:
        assert np.array_equal(small[f], runs[0][f][:S]), f
    gw = plan(monkeypatch, None, B, serial_wave=1)
    other = solve(gw, B)
    for f in FIELDS:
        assert np.array_equal(other[f], runs[0][f]), f
