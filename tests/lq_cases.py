"""Seeded, well conditioned linear-quadratic test problems shared by tests/test_lq_reference_cpu.py (which checks the
input condition e_oracle <= 1e-11 without a GPU) and tests/test_lqr_exact_gpu.py (which runs the kernels on them).

Conditioning ("Exact LQ tests"): R = 0.5 (I + 0.1 11'), Q = G G' + I, Qf = 10 Q.  With R = 1e-3 I against a
rank-deficient Q of size 100 -- the inputs of the golden-vector tests -- the float64 recursion of oracle/lqr.py is itself
only good to ~1e-5 and cannot tell a kernel that is wrong in the seventh digit from a right one."""
import numpy as np

from oracle import lqr as olqr, tpwl as otpwl

DT = 0.05
LDS_LIMIT = 160 * 1024
NT = 512

# (r, n_u, n_z, N) with n_x = 2 r: the path and the edge each one reaches (paths by `ilqr_path` below)
ILQR_SHAPES = [
    (1, 1, 1, 1),        # smallest of everything; ilqr_gain_t<1>; one stage
    (5, 4, 6, 10),       # generic instantiation, MFMA-1
    (5, 4, 6, 513),      # more stages than threads: the strided expected-decrease sum
    (9, 7, 6, 5),        # n_x + n_u = 25: not a multiple of 16, one panel short of two
    (17, 3, 16, 5),      # n_x + n_u = 37: just over two 16-row panels; n_z = 16
    (30, 4, 6, 15),      # fixed <0, 60, 4>, MFMA-1 (n_x + n_u = 64 fills the panel: the largest n_x MFMA-1 takes at n_u = 4)
    (30, 8, 6, 15),      # fixed <0, 60, 8> -- by the LDS formula this one is MFMA-2 (three 80 x 81 panels do not fit)
    (24, 16, 16, 5),     # chol16 branch (n_u > 8) on MFMA-1: (48, 16) is the largest n_x MFMA-1 accepts at n_u = 16
    (31, 2, 6, 5),       # (62, 2): the largest n_x MFMA-1 accepts at all
    (31, 9, 6, 5),       # chol16 on MFMA-2; the B block (columns 62..70) spans the tile boundary at 64 in ilqr_mm
    (30, 16, 16, 3),     # (60, 16): the largest n_x MFMA-2 accepts at n_u = 16; B block columns 60..75
    (32, 16, 16, 5),     # (64, 16): neither MFMA layout fits -- default dispatch lands on the VALU pass without staging
    (33, 5, 6, 5),       # MFMA-2, generic instantiation
    (36, 4, 6, 15),      # MFMA-2, fixed <0, 72, 4>
    (36, 7, 6, 3),       # the largest n_u MFMA-2 accepts at n_x = 72 (n_u = 8 is refused there: see the refusal test)
    (38, 4, 6, 3),       # (76, 4): the largest n_x MFMA-2 accepts at n_u = 4 (78 is refused)
]
# the same under SRH_ILQR_NO_MFMA: three staged ([A|B] in LDS) and the largest n_x that fits only without staging
VALU_SHAPES = [(5, 4, 6, 10), (17, 3, 16, 5), (30, 8, 6, 15), (37, 4, 6, 5)]


def lqr_lds_doubles(n, m, nn=0):
    """csrc/lqr.hip: lqr_lds_doubles."""
    nn = nn or n * n
    return 3 * nn + 2 * n * m + 2 * 256 + 2 * m * n + 4 * n + 32 + 16 + 4


def ilqr_path(n, m, no_mfma=False, ssm_tail=None):
    """The dispatch of ilqr_impl (csrc/lqr.hip), restated from its LDS formulas: 'mfma1', 'mfma2', 'valu_staged',
    'valu_unstaged' or 'refused' (TPWL model; `ssm_tail`: the extra doubles of an SSM model, see ssm_ilqr_path).
    This is a hand copy -- the library exports nothing that names the path, and tests may add no export.  The refusal
    tests check the copy against the kernel's own refusals; between two refusal sizes a change of the kernel's LDS layout
    would mislabel paths (in the log and in test_ilqr_paths_and_refusal_sizes) without a test noticing, so whoever changes
    lqr_lds_doubles, `tail` or the mf_lds formulas in lqr.hip changes them here."""
    tail = 20 + 16 * n + 16 + NT + 16 + n + (ssm_tail or 0)
    NPa = (n + m + 15) & ~15
    ldp = NPa + 1
    off = lqr_lds_doubles(n, m, 256) + tail
    mf1 = (off + 3 * NPa * ldp + 16 * ldp + 16 * n + 16) * 8
    mf2 = (off + (n + m + ((n + 3) & ~3) + 16) * ldp + 16 * n + 16) * 8
    if not no_mfma and mf1 <= LDS_LIMIT:
        return 'mfma1'
    if not no_mfma and mf2 <= LDS_LIMIT:
        return 'mfma2'
    valu = (lqr_lds_doubles(n, m) + tail) * 8
    if ssm_tail is not None:                                   # SSM models always stage (A_t, B_t): it is part of their tail
        return 'valu_staged' if valu <= LDS_LIMIT else 'refused'
    if valu + 8 * (n * n + n * m + n) <= LDS_LIMIT:
        return 'valu_staged'
    return 'valu_unstaged' if valu <= LDS_LIMIT else 'refused'


def ssm_ilqr_path(n, m, no, Er, ns, dense_jacobian=False, no_mfma=False):
    """ilqr_path for an SSM model with exponent table Er (nr x n) of the reduced dynamics and ns output monomials:
    the tail adds the per-step (A, B, d), ssm::work_doubles and ssm::lds_tab_doubles with the compact-list capacity of
    ssm::jacobian_list_cap (csrc/ssm_dev.h) -- the same kind of hand copy as ilqr_path."""
    Er = np.asarray(Er)
    nr = Er.shape[0]
    assert Er.shape == (nr, n)
    jcap = 0 if dense_jacobian else max(int((Er[g::4, j] > 0).sum()) for j in range(n) for g in range(4))
    work = max(nr, ns) + max(nr * n, ns * no) + 4 * n + 4 * n * (n | 1) + n + 4
    ints = 2 * nr * n + 2 * nr + 2 * ns * no + 2 * ns + 3 * 4 * n * jcap
    tab = n * nr + no * ns + n * 16 + (ints + 1) // 2 + 8
    return ilqr_path(n, m, no_mfma, ssm_tail=n * n + n * m + n + work + tab)


# seeds replaced because the default one left the optimal trajectory inside a single TPWL region (the CPU test asserts
# that the nearest-point search picks more than one point on every case with more than one stage)
ILQR_SEEDS = {(9, 7, 6, 5): 1, (36, 7, 6, 3): 2}


def costs(m, nz, rng):
    G = rng.standard_normal((nz, nz))
    Q = G @ G.T + np.eye(nz)
    R = 0.5 * (np.eye(m) + 0.1 * np.ones((m, m)))
    return Q, R, 10.0 * Q


def ilqr_case(r, m, nz, N, seed=None, n_points=6, q_scale=0.003):
    """One affine map behind a TPWL table of `n_points` points: every point carries point 0's (A_c, B_c, d_c) but its own
    q, so the nearest-point search still chooses while the dynamics are x+ = A x + B u + d.  Returns a dict with the
    model pieces (for helpers.product_tpwl), the costs, targets, x0 and a warm start."""
    seed = ILQR_SEEDS.get((r, m, nz, N), 1000 * r + 10 * m + nz) if seed is None else seed
    rng = np.random.default_rng(seed)
    model = otpwl.synthetic_model(r, m, n_points, seed=seed)
    for key in ('A_c', 'B_c', 'd_c'):
        model[key][1:] = model[key][0]
    model['B_c'] *= 20.0                       # inputs of size ~1 move the outputs by ~0.1: u, K are O(1), not O(1e-3)
    model['q'] = model['q'] * q_scale          # the points lie within the reach of the trajectory
    n_f = 60
    U, _ = np.linalg.qr(rng.standard_normal((n_f, r)))
    q_ref = rng.uniform(-1.0, 1.0, n_f)
    v_ref = 0.01 * rng.standard_normal(n_f)
    Hf = rng.standard_normal((nz, 2 * n_f))
    H = Hf @ np.kron(np.eye(2), U)
    z_ref = Hf @ np.concatenate([v_ref, q_ref])
    Q, R, Qf = costs(m, nz, rng)
    z_target = z_ref + 0.05 * rng.standard_normal((N + 1, nz))
    x0 = 1e-2 * rng.standard_normal(2 * r)
    u_warm = rng.standard_normal((N, m))
    model['q'][0] = x0[r:]                     # the first step picks point 0, later ones whichever random point is nearest
    return dict(r=r, m=m, nz=nz, N=N, model=model, U=U, q_ref=q_ref, v_ref=v_ref, Hf=Hf, H=H, z_ref=z_ref, Q=Q, R=R,
                Qf=Qf, z_target=z_target, x0=x0, u_warm=u_warm)


def oracle_newton_step(A, B, d, H, z_ref, c, u_warm=None):
    """One iteration of the float64 oracle (oracle/lqr.py) on the affine map (A, B, d): max_iter = 0, no input-variation
    cost, no line search, no regularisation.  Returns x, u, K, cost."""
    n, m = B.shape
    o = olqr.ILQRGeneric(lambda x, u: (A, B, d), lambda x: H @ x + z_ref, H, n, m, c['Q'], c['R'], c['Qf'], c['N'])
    o.p.max_iter = 0
    o.p.include_input_var_constraint = o.p.do_linesearch = o.p.regularize = False
    x, u, K = o.solve(c['x0'], c['z_target'], u_warm)
    assert len(o.trace) == 2
    return x, u, K, o.trace[-1][1]


def orthogonal(n, rng):
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return Qm


# (n_x, n_u) of the TV-LQR / fixed-point DARE tests: inner dimensions of `mm` below, on and past its unroll by 8, n_u
# on both sides of 8, and (78, 4): the largest n_x the kernels' LDS carve accepts at n_u = 4 (79 is refused)
RICCATI_SHAPES = [(1, 1), (2, 2), (7, 3), (8, 8), (9, 1), (17, 9), (33, 16), (64, 5), (78, 4)]


def tvlqr_case(n, m, steps, seed=None):
    rng = np.random.default_rng(7000 + 100 * n + 10 * m + steps if seed is None else seed)
    A = np.stack([0.95 * orthogonal(n, rng) for _ in range(steps)])
    B = rng.standard_normal((steps, n, m))
    G = rng.standard_normal((n, n))
    return A, B, G @ G.T + np.eye(n), 0.5 * (np.eye(m) + 0.1 * np.ones((m, m)))


# seeds of the fixed-point DARE cases: chosen so that ||L - L_old||_F of the reference's last two iterations is at least
# 1 % away from tol = 1e-4 (tests/test_lq_reference_cpu.py asserts it): an iteration count that flips is the kernel's doing
DARE_SEEDS = {(33, 16): 1}            # the default seed stops member 0 at 1.008e-4, inside the margin


def dare_case(n, m, seed=None):
    """Three different (A, B) = (0.9 orthogonal, randn) under one (Q, R): member 0 is the single solve, the stack is the
    batched one.  Returns A (3, n, n), B (3, n, m), Q, R."""
    seed = DARE_SEEDS.get((n, m), 9000 + 100 * n + m) if seed is None else seed
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    A = np.stack([0.9 * orthogonal(n, rng) for _ in range(3)])
    B = rng.standard_normal((3, n, m))
    return A, B, G @ G.T + np.eye(n), 0.5 * (np.eye(m) + 0.1 * np.ones((m, m)))


def dare_modes_case(n, m, rho, rank_q, seed):
    """The doubling DARE tests' problem (tests/test_lqr_gpu.py, tests/test_rompc_gpu.py): a diagonalisable A whose slowest mode
    sits at |lambda| = rho, randn B, a state cost of rank `rank_q`, R = 1e-2 diag(0.5 .. 2).  Returns A, B, Q, R."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, n))
    lam = rho * rng.uniform(0.3, 1.0, n)
    lam[0] = rho
    A = np.real(V @ np.diag(lam) @ np.linalg.inv(V))
    B = rng.standard_normal((n, m))
    Cq = rng.standard_normal((rank_q, n))
    return A, B, Cq.T @ Cq, np.diag(rng.uniform(0.5, 2.0, m)) * 1e-2
