"""Without a GPU: the refusals of the measurement re-projection (Y=) of the batched closed loops that happen before any device call, and
the surface the feature adds (entries of the library, their declarations, the seeds of the GPU cases).

Y must be a Polyhedron made with with_reproject=True -- the reference refuses to project onto any other -- of at most 16 dimensions and
64 rows, finite, with as many columns as the loop has measurements; each refusal names the class and carries the numbers."""
import os
import re
import types

import numpy as np
import pytest

import koopman_reproject_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def poly(A, b, with_reproject=True):
    from sofacontrol_amd.utils import Polyhedron
    return Polyhedron(A, b, with_reproject=with_reproject)


def koopman_loop(Y, ny=3):
    """set_reproject of a loop that has no handle: Y is examined before the library is called."""
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    cl = KoopmanClosedLoopBatch.__new__(KoopmanClosedLoopBatch)
    cl.n_y, cl._h = ny, None
    return cl.set_reproject(Y)


BOX3 = (np.kron(np.eye(3), np.array([[1.0], [-1.0]])), np.ones(6))


def test_Y_must_be_a_polyhedron():
    with pytest.raises(RuntimeError, match=r'KoopmanClosedLoopBatch: Y must be a Polyhedron\(A, b, with_reproject=True\), got tuple'):
        koopman_loop(BOX3)


def test_Y_without_reproject_is_refused_by_name():
    with pytest.raises(RuntimeError, match='KoopmanClosedLoopBatch: Y was made without with_reproject=True'):
        koopman_loop(poly(*BOX3, with_reproject=False))


def test_Y_columns_must_match_the_measurements():
    with pytest.raises(RuntimeError, match=r'KoopmanClosedLoopBatch: Y needs A of shape \(rows, n_y = 2\).*got A \(6, 3\) and b \(6,\)'):
        koopman_loop(poly(*BOX3), ny=2)
    with pytest.raises(RuntimeError, match=r'got A \(6, 3\) and b \(5,\)'):
        koopman_loop(poly(BOX3[0], np.ones(5)))


def test_limits_carry_the_numbers():
    with pytest.raises(RuntimeError, match=r'n_y <= 16 and 1 <= rows <= 64 \(got n_y = 17, rows = 2\)'):
        koopman_loop(poly(np.ones((2, 17)), np.ones(2)), ny=17)
    with pytest.raises(RuntimeError, match=r'n_y <= 16 and 1 <= rows <= 64 \(got n_y = 3, rows = 65\)'):
        koopman_loop(poly(np.ones((65, 3)), np.ones(65)))
    with pytest.raises(RuntimeError, match=r'got n_y = 3, rows = 0'):
        koopman_loop(poly(np.ones((0, 3)), np.ones(0)))


def test_non_finite_Y_names_the_row():
    A, b = BOX3[0].copy(), BOX3[1].copy()
    A[4, 1] = np.nan
    with pytest.raises(RuntimeError, match=r'KoopmanClosedLoopBatch: Y is not finite \(row 4'):
        koopman_loop(poly(A, b))
    A, b = BOX3[0].copy(), BOX3[1].copy()
    b[2] = np.inf
    with pytest.raises(RuntimeError, match=r'Y is not finite \(row 2'):
        koopman_loop(poly(A, b))


def test_constructors_keep_their_parameter_lists():
    """Y is set behind the constructor (set_reproject, as the library's *_set_reproject): no constructor grows a parameter."""
    import inspect
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    for fn in (KoopmanClosedLoopBatch.__init__, SSMClosedLoopBatch.__init__, SSMClosedLoopBatch.on_plant):
        assert 'Y' not in inspect.signature(fn).parameters
    for cls in (KoopmanClosedLoopBatch, SSMClosedLoopBatch):
        assert list(inspect.signature(cls.set_reproject).parameters) == ['self', 'Y']


def test_no_Y_passes_the_check():
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanClosedLoopBatch
    assert KoopmanClosedLoopBatch._check_reproject(None, 3) is None
    A, b = KoopmanClosedLoopBatch._check_reproject(poly(*BOX3), 3)
    assert A.shape == (6, 3) and b.shape == (6,) and A.flags['C_CONTIGUOUS'] and A.dtype == np.float64


def ssm_loop(Y, observe=True, n_o=3, tpwl=False):
    """set_reproject of an SSM loop (either plant kind) that has no handle: Y is examined before the library is called."""
    from sofacontrol_amd.scp.closed_loop_ssm import SSMClosedLoopBatch
    cl = SSMClosedLoopBatch.__new__(SSMClosedLoopBatch)
    cl.n_o, cl.observe, cl._h, cl.n_plant = n_o, observe, None, (8 if tpwl else None)
    return cl.set_reproject(Y)


@pytest.mark.parametrize('tpwl', (False, True), ids=('ssm-plant', 'tpwl-plant'))
def test_ssm_loops_refuse_the_same_things(tpwl):
    with pytest.raises(RuntimeError, match='SSMClosedLoopBatch: Y was made without with_reproject=True'):
        ssm_loop(poly(*BOX3, with_reproject=False), tpwl=tpwl)
    with pytest.raises(RuntimeError, match=r'SSMClosedLoopBatch: Y must be a Polyhedron\(A, b, with_reproject=True\), got list'):
        ssm_loop([1, 2], tpwl=tpwl)
    with pytest.raises(RuntimeError, match=r'SSMClosedLoopBatch: Y needs A of shape \(rows, n_y = 4\)'):
        ssm_loop(poly(*BOX3), n_o=4, tpwl=tpwl)
    with pytest.raises(RuntimeError, match=r'n_y <= 16 and 1 <= rows <= 64 \(got n_y = 3, rows = 70\)'):
        ssm_loop(poly(np.ones((70, 3)), np.ones(70)), tpwl=tpwl)
    A = BOX3[0].copy(); A[0, 0] = np.inf
    with pytest.raises(RuntimeError, match=r'Y is not finite \(row 0'):
        ssm_loop(poly(A, BOX3[1]), tpwl=tpwl)


def test_ssm_loop_refuses_Y_without_a_measurement():
    with pytest.raises(RuntimeError, match='SSMClosedLoopBatch: Y together with observe=False is refused'):
        ssm_loop(poly(*BOX3), observe=False)


def test_stand_alone_advance_entries_name_themselves():
    from sofacontrol_amd.scp import closed_loop_ssm
    with pytest.raises(RuntimeError, match='advance_tpwl: Y was made without with_reproject=True'):
        closed_loop_ssm._Y_arrays('advance_tpwl', poly(*BOX3, with_reproject=False), 3)
    A, b, rows = closed_loop_ssm._Y_arrays('advance', poly(*BOX3), 3)
    assert rows == 6 and A.shape == (6, 3)


ENTRIES = ('spoly_project_status', 'skoop_loop_set_reproject', 'skoop_loop_run_reprojected', 'skoop_loop_advance_reprojected',
           'sgusto_ssm_loop_set_reproject', 'sgusto_ssm_loop_run_reprojected', 'sgusto_ssm_loop_advance_reprojected',
           'sgusto_ssm_loop_advance_tpwl_reprojected')


@pytest.mark.parametrize('name', ENTRIES)
def test_entries_are_declared_and_exported(name):
    from sofacontrol_amd import _lib
    assert hasattr(_lib.lib(), name), 'the library does not export %s' % name
    with open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')) as f:
        assert re.search(r'^int %s\(' % name, f.read(), flags=re.M), 'include/sofacontrol_hip.h does not declare %s' % name


def test_result_fields_are_none_without_Y():
    from sofacontrol_amd.baselines.koopman.closed_loop import KoopmanLoopResult
    from sofacontrol_amd.scp.closed_loop import ClosedLoopResult
    for r in (KoopmanLoopResult(*[None] * 8), ClosedLoopResult(*[None] * 7)):
        assert r.y_used is None and r.proj is None


def test_replay_samples_keep_clear_of_the_faces():
    """The condition on closeness to a face, on the CPU, for every one-launch case (their samples are given, not simulated)."""
    for ny in rc.NY:
        for rows in rc.ROWS:
            A, b = rc.polyhedron(ny, rows)
            assert A.shape[1] == ny and A.shape[0] == {'one': 1, 'box+1': 2 * ny + 1, '64': 64}[rows]
            for B in (1, 3):
                Y, kinds = rc.replay_samples(ny, rows, B, rc.N * rc.R)
                share = rc.check_sides(A, b, Y)
                assert 0.0 < share < 1.0, (ny, rows, B, share)
                if rc.box_face(A, b) is not None:
                    assert (kinds[:, 1:] == 'face').any() and (kinds[:, 1:] == 'ulp').any()
