"""CPU: the continuous-time LQR surface exists -- `sric_care` declared in include/sofacontrol_hip.h and exported by the built
library, lqr.care / care_batch / CLQR and controllers.StateCLQR with the reference's class relations (sofacontrol/lqr/lqr.py:57,
sofacontrol/tpwl/controllers.py:440-444)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sric_care_is_declared_and_exported():
    from sofacontrol_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'sofacontrol_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'^int\s+sric_care\s*\(const double \*A, const double \*B, int64_t batch, int n_x, int n_u,', src, flags=re.M)
    assert hasattr(_lib.lib(), 'sric_care')


def test_python_surface_and_class_relations():
    import sofacontrol_amd.lqr.lqr as lqr
    from sofacontrol_amd.tpwl import controllers
    from sofacontrol_amd.tpwl.controllers import StateCLQR          # what a port of a reference driver imports
    assert callable(lqr.care) and callable(lqr.care_batch)
    assert issubclass(lqr.CLQR, lqr.DLQR) and lqr.CLQR is not lqr.DLQR
    assert lqr.CLQR.compute_gain_matrix is not lqr.DLQR.compute_gain_matrix
    assert lqr.CLQR.compute_policy is lqr.DLQR.compute_policy
    assert issubclass(StateCLQR, controllers.StateDLQR)
    assert StateCLQR.LQR_type is lqr.CLQR and controllers.StateDLQR.LQR_type is lqr.DLQR
    assert StateCLQR.compute_input is controllers.StateDLQR.compute_input


def test_sric_care_refuses_bad_dimensions_without_a_gpu():
    """The argument checks come before any device call."""
    import ctypes as C
    import numpy as np
    from sofacontrol_amd import _lib
    A, B, Q, R = np.eye(2), np.ones((2, 17)), np.eye(2), np.eye(17)
    K, P = np.empty((17, 2)), np.empty((2, 2))
    rc = _lib.lib().sric_care(_lib.dptr(A), _lib.dptr(B), C.c_int64(1), C.c_int(2), C.c_int(17), _lib.dptr(Q), _lib.dptr(R),
                              C.c_double(1e-14), C.c_int(100), _lib.dptr(K), _lib.dptr(P), None)
    assert rc == -1 and b'sric_care: bad dimensions' in _lib.lib().srh_last_error()
