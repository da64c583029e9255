"""Seeded cases of the batched SSM closed loop, shared by tests/test_ssm_loop_reference_cpu.py (which measures the float64 chain against
the long-double one without a GPU) and tests/test_gusto_ssm_loop_gpu.py (which runs ssm_loop_advance_kernel on them).

Planner = workloads.ssm_model(n, m, rom order, ssm order, seed=500 + n) (tests/ssm_cases.model); the plant is the planner with its
nonlinear R columns (and those of its discrete map) and its W moved 2 % towards the model of seed 900 + n: another model of the same
shape, near enough that the controller's W_map still inverts its output.  x0 = 0.3 N(0, 1), plan inputs 0.5 N(0, 1), W and V at 1e-3,
all from default_rng(7000 + n + n_keep), B = 3 members.  Tolerance: the project's rule, ssm_cases.tolerance = max(100 e_oracle, 1e-13) with
e_oracle <= 1e-11 asserted.  Whatever the functions return is cached: treat it as read-only."""
import numpy as np

import cl_cases as cc
import ssm_cases as sc
import ssm_loop_reference as slr

B = 3
MIX = 0.02
# (shape (n, m, rom order, ssm order), plant method, dt_sim, dt, N, n_keep)
ADVANCE = [
    ((1, 1, 7, 7), 'fe', 0.01, 0.05, 12, 10),        # the highest order, ld = 1
    ((2, 3, 4, 1), 'bil', 0.03, 0.05, 12, 10),       # n_u > n_x, linear maps, fractional dt / dt_sim
    ((5, 5, 3, 3), 'fe', 0.01, 0.05, 12, 60),        # odd n, the longest allowed n_keep
    ((6, 4, 3, 2), 'be', 0.01, 0.02, 3, 4),          # the hardware driver's shape
    ((6, 4, 3, 2), 'be', 0.02, 0.02, 3, 3),          # n_keep dt_sim == N dt
    ((9, 4, 2, 2), 'be', 0.03, 0.05, 12, 10),        # EP2 inverse
    ((12, 8, 2, 2), 'be', 0.01, 0.05, 12, 10),       # EP4, eight inputs
    ((16, 4, 2, 1), 'bil', 0.05, 0.05, 12, 1),       # the last of EP4, n_keep = 1
    ((10, 8, 3, 2), 'map', 0.01, 0.05, 12, 10),      # C3, the discrete map
]
FIELDS = ('X', 'Z', 'U', 'Y', 'Xhat')


def case_id(c):
    return '%s-%s@%g-N%d-k%d' % (sc.shape_id(c[0]), c[1], c[2], c[4], c[5])


@sc.cached
def plant_model(s):
    """The plant's float64 coefficient arrays of a shape (a new dict: the planner's stays as it is)."""
    import workloads
    n, m, ro, so = s
    d, o = sc.model(s), workloads.ssm_model(n, m, ro, so, seed=900 + n)
    p = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    p['R'][:, n:] += MIX * (o['R'][:, n:] - d['R'][:, n:])
    p['Rd'][:, n:] += MIX * (o['Rd'][:, n:] - d['Rd'][:, n:])
    p['W'] += MIX * (o['W'] - d['W'])
    return p


@sc.cached
def inputs(c):
    """dict uopt (B, N, m), x (B, n), W (n_keep, B, n), V (n_keep, B, n), j, theta (n_keep) of a case."""
    (n, m, _, _), _, dt_sim, dt, N, nk = c
    rng = np.random.default_rng(7000 + n + nk)
    _, _, j, theta = cc.direct_schedule(N, dt, dt_sim, nk, 0.0, 0)
    return dict(x=0.3 * rng.standard_normal((B, n)), uopt=0.5 * rng.standard_normal((B, N, m)), W=1e-3 * rng.standard_normal((nk, B, n)),
                V=1e-3 * rng.standard_normal((nk, B, n)), j=np.asarray(j), theta=np.asarray(theta))


def chain(c, dtype):
    """The chain of every member in `dtype`: {field: (B, n_keep, .)}."""
    s, method, dt_sim = c[0], c[1], c[2]
    make = sc.reference_model if dtype is slr.LD else sc.oracle_model
    plant, planner = make(plant_model(s)), make(sc.model(s))
    i = inputs(c)
    out = [slr.advance(plant, planner, method, dt_sim, i['uopt'][b], i['x'][b], i['j'], i['theta'], i['W'][:, b], i['V'][:, b], dtype)
           for b in range(B)]
    return {f: np.stack([o[k] for o in out]) for k, f in enumerate(FIELDS)}


@sc.cached
def reference(c):
    """(the long-double chain, {field: e_oracle} of the float64 chain over all members and sub-steps)."""
    ref, f64 = chain(c, slr.LD), chain(c, np.float64)
    return ref, {f: slr.err(f64[f], ref[f]) for f in FIELDS}
