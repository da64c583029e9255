"""Seeded continuous-time LQR test problems shared by tests/test_care_reference_cpu.py (which checks every case's certificate
and input condition without a GPU) and tests/test_care_gpu.py (which runs care_sda_kernel on them).

Every case is three different (A, B) pairs under one (Q, R): member 0 is the single solve, the stack is the batched one.  Member
0 draws its matrices in the order the family's recipe lists them; the other members' (A, B) follow.

Tolerance rule (tests/test_lqr_exact_gpu.py): tol = max(100 e_yardstick, 1e-13) with e_yardstick the error of
scipy.linalg.solve_continuous_are against the long-double reference on the same inputs, e_yardstick <= 1e-11 asserted; error
measure max|a - b| / max(1, max|b|)."""
import numpy as np
import scipy.linalg

import care_reference as cr
from helpers import golden_problem
from lq_cases import RICCATI_SHAPES

E_YARDSTICK_MAX = 1e-11
MEMBERS = 3

RAND_SHAPES = list(RICCATI_SHAPES)             # (n_x, n_u); 64 and 78 use the HBM slots
FEM_SHAPES = [(1, 1), (3, 2), (36, 8), (30, 4), (39, 4)]       # (r, n_u), n_x = 2 r; (36, 8) is the shipped basis size
UNSTABLE_SHAPES = [(7, 3), (33, 16)]
# seeds of the `unstable` family replaced because the default one (13000 + 100 n + m) left a member with a stable open loop: with
# these every member has an eigenvalue of A in the right half plane and holds the certificate and the input condition
# (tests/test_care_reference_cpu.py asserts all three)
UNSTABLE_SEEDS = {(7, 3): 15703}

CONTROLLER = ('controller', 8, 3)              # one member: `controller_case` below
CASES = ([('rand', n, m) for n, m in RAND_SHAPES] + [('fem', r, m) for r, m in FEM_SHAPES] +
         [('unstable', n, m) for n, m in UNSTABLE_SHAPES])
ALL_CASES = CASES + [CONTROLLER]               # what tests/test_care_reference_cpu.py certifies


def case_id(case):
    return '%s-%d-%d' % case


def _rand_pair(n, m, rng):
    K = rng.standard_normal((n, n)) / np.sqrt(n)
    A = (K - K.T) + np.diag(rng.uniform(-1.0, 0.3, n))
    return A, rng.standard_normal((n, m))


def rand_case(n, m, seed=None, shift=0.0):
    """A = skew + diag(U(-1, 0.3)) (+ shift I), B = randn, Q = G G'/n + I, R = 0.5 (I + 0.1 11')."""
    rng = np.random.default_rng(11000 + 100 * n + m if seed is None else seed)
    pairs = [_rand_pair(n, m, rng)]
    G = rng.standard_normal((n, n))
    pairs += [_rand_pair(n, m, rng) for _ in range(MEMBERS - 1)]
    A = np.stack([p[0] for p in pairs]) + shift * np.eye(n)
    return A, np.stack([p[1] for p in pairs]), G @ G.T / n + np.eye(n), 0.5 * (np.eye(m) + 0.1 * np.ones((m, m)))


def _fem_pair(r, m, rng):
    V, _ = np.linalg.qr(rng.standard_normal((r, r)))
    Kq = V @ np.diag(np.logspace(0, 2, r)) @ V.T
    D = 0.02 * Kq + 0.2 * np.eye(r)
    A = np.block([[-D, -Kq], [np.eye(r), np.zeros((r, r))]])
    return A, np.concatenate([rng.standard_normal((r, m)), np.zeros((r, m))])


def fem_case(r, m, seed=None, members=MEMBERS):
    """The lightly damped second-order shape of a TPWL point, x = [v; q]: A = [[-D, -Kq], [I, 0]], B = [randn; 0],
    Q = 100 C'C + 1e-2 I with C = [0 | randn(min(3, r), r)], R = 1e-2 diag(U(0.5, 2))."""
    rng = np.random.default_rng(12000 + 100 * r + m if seed is None else seed)
    pairs = [_fem_pair(r, m, rng)]
    C = np.concatenate([np.zeros((min(3, r), r)), rng.standard_normal((min(3, r), r))], axis=1)
    R = 1e-2 * np.diag(rng.uniform(0.5, 2.0, m))
    pairs += [_fem_pair(r, m, rng) for _ in range(members - 1)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), 100.0 * C.T @ C + 1e-2 * np.eye(2 * r), R


def unstable_case(n, m, seed=None):
    """The `rand` family with A + 0.5 I: an unstable open loop."""
    seed = UNSTABLE_SEEDS.get((n, m), 13000 + 100 * n + m) if seed is None else seed
    return rand_case(n, m, seed=seed, shift=0.5)


def controller_case():
    """The operating point of the StateCLQR test: point 2 of the synthetic TPWL model tests/test_controllers_gpu.py builds its
    StateDLQR on, under the `rand` family's costs.  Returns the model pieces (for helpers.product_tpwl), the point's index, Q, R."""
    model, U, q_ref, v_ref, Hf = golden_problem(4, 3, 7, 20, 40, q_scale=0.05)
    G = np.random.default_rng(5).standard_normal((8, 8))
    return (model, U, q_ref, v_ref, Hf), 2, G @ G.T / 8 + np.eye(8), 0.5 * (np.eye(3) + 0.1 * np.ones((3, 3)))


def inputs(case):
    if case == CONTROLLER:
        (model, *_), k, Q, R = controller_case()
        return model['A_c'][k][None], model['B_c'][k][None], Q, R
    family, a, b = case
    return {'rand': rand_case, 'fem': fem_case, 'unstable': unstable_case}[family](a, b)


def tolerance(e_yardstick):
    assert e_yardstick <= E_YARDSTICK_MAX, e_yardstick
    return max(100.0 * e_yardstick, 1e-13)


_PREPARED = {}


def prepared(case):
    """The inputs of a case and, per member, the long-double reference (X, K), its doubling steps, its certificate figures
    and the yardstick's error -- computed once per case and shared by every test; nothing modifies it."""
    if case not in _PREPARED:
        A, B, Q, R = inputs(case)
        members = []
        for k in range(A.shape[0]):
            X, steps = cr.care(A[k], B[k], Q, R)
            Xs = scipy.linalg.solve_continuous_are(A[k], B[k], Q, R)
            res, res_scipy, re_max = cr.certificate(A[k], B[k], Q, R, X, Xs)
            members.append(dict(X=X, K=cr.gain(B[k], R, X), steps=steps, res=res, res_scipy=res_scipy, re_max=re_max,
                                e_yardstick=cr.err(Xs, X)))
        _PREPARED[case] = (A, B, Q, R, members)
    return _PREPARED[case]
