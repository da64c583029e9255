"""Seeded problems of the batched filter (sekf_batch_*, DiscreteEKFObserverBatch), shared by tests/test_ekf_batch_surface_cpu.py
(input conditions, no GPU) and tests/test_ekf_batch_gpu.py.

One shape per kernel path.  The shape's model, C, y_ref, W, V and Sigma0 are those of tests/ekf_cases.py (first scaling, table
form); every member of a batch gets its own state resets, inputs and measurements, drawn from seed + member with the recipe of
ekf_cases.case, and runs the schedule of ekf_cases.operations: reset at every fourth step, fused calls at even steps, a predict-only
call followed by an update-only call at odd ones.  The long-double reference, the float64 oracle and the tolerance rule are
ekf_cases' own (LongDoubleFilter, OracleFilter, tolerance)."""
import numpy as np

import ekf_cases as ec

SHAPES = [('valu', 8, 6, 4), ('mfma0', 34, 15, 16), ('mfma60', 60, 30, 4), ('wide', 72, 30, 4)]
SMALL = 3                                   # every member is compared
LARGE = 260                                 # more workgroups than the MI355X has CUs (256): a CU takes a second one
LARGE_MEMBERS = (0, 1, 255, 256, 259)
FAILING = 1                                 # the member that is handed an indefinite covariance in the isolation test

_MEMBERS = {}


def member(shape, b):
    """The case of member b: ekf_cases.case(shape) with its own resets, u and y (cached; read-only)."""
    key = (tuple(shape), b)
    if key not in _MEMBERS:
        base = ec.case(ec.spec(shape))
        n, ny, m, steps = base['n'], base['ny'], base['m'], base['steps']
        rng = np.random.default_rng(base['seed'] + b)
        pts = np.hstack([base['model']['v'], base['model']['q']])
        u = rng.uniform(0.0, 300.0, (steps, m))
        point = [(ec.POINTS - 1 - k // 4 + b) % ec.POINTS for k in range(steps)]          # members start on different table points
        y = base['y_ref'] + pts[point] @ base['C'].T + 0.05 * rng.standard_normal((steps, ny))
        resets = {k: pts[point[k]] + 1e-3 * rng.standard_normal(n) for k in range(0, steps, 4)}
        c = dict(base)
        c.update(u=u, y=y, resets=resets, member=b)
        _MEMBERS[key] = c
    return _MEMBERS[key]


_REFS = {}


def reference(shape, b):
    """(long-double trajectory, the filter that made it -- picks, margins --, e_oracle) of member b, as ekf_cases.reference."""
    key = (tuple(shape), b)
    if key not in _REFS:
        c = member(shape, b)
        ref = ec.LongDoubleFilter(c)
        traj = ec.run(c, ref)
        e_oracle = max(max(e) for e in ec.errors(ec.run(c, ec.OracleFilter(c)), traj))
        _REFS[key] = (traj, ref, e_oracle)
    return _REFS[key]


def batch_operations(shape, members):
    """The common schedule of the members as batched operations: ('reset', k, X (B x n)) | ('step', k, U (B x m) or None,
    Y (B x ny) or None).  Every member has the same sequence of operation kinds."""
    per = [ec.operations(member(shape, b)) for b in members]
    out = []
    for ops in zip(*per):
        kind, k = ops[0][0], ops[0][1]
        assert all(o[0] == kind and o[1] == k for o in ops)
        if kind == 'reset':
            out.append(('reset', k, np.stack([o[2] for o in ops])))
        else:
            u = None if ops[0][2] is None else np.stack([o[2] for o in ops])
            y = None if ops[0][3] is None else np.stack([o[3] for o in ops])
            out.append(('step', k, u, y))
    return out
