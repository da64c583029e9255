"""Extended-precision statement of the SSM polynomial reduced model behind csrc/ssm.hip and csrc/ssm_dev.h (test
infrastructure only).

Plain numpy in np.longdouble (80-bit on x86: eps 1.1e-19; np.linalg has no long-double path, hence the hand-written
Gauss-Jordan inverse; no np.power on long double: monomials by repeated multiplication).  Nothing here imports the package
under test or the float64 oracle: oracle/ssm.py is *measured* against this module (tests/test_ssm_reference_cpu.py), and that
measured error sets the tolerance of the kernels (tests/test_ssm_exact_gpu.py).

The model (sofacontrol/SSM/ssm.py):  f(x, u) = R phi_r(x) + B u,  z = W phi_s(x) + z_ref,  x = V phi_s(z - z_ref), phi the
monomials of degree 1 .. order -- graded, within a degree lexicographic with x1 first (ssm.py:158-164)."""
from itertools import combinations_with_replacement

import numpy as np

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def err(a, b):
    """The project's error measure: max|a - b| / max(1, max|b|), b the reference (as lq_reference.err)."""
    a, b = ld(a), ld(b)
    return float(np.abs(a - b).max() / max(LD(1), np.abs(b).max()))


def exponents(dim, order):
    """Exponent table (n_mon, dim).  A monomial of degree g is a multiset of g variable indices; the multisets in
    lexicographic order of their sorted index tuples are the monomials with the highest power of x1 first."""
    rows = []
    for deg in range(1, order + 1):
        for combo in combinations_with_replacement(range(dim), deg):
            e = [0] * dim
            for i in combo:
                e[i] += 1
            rows.append(e)
    return np.array(rows, dtype=np.int64).reshape(-1, dim)


def phi(E, x):
    """phi_j = prod_i x_i^E[j, i] by repeated multiplication."""
    x = ld(x)
    out = np.ones(E.shape[0], dtype=LD)
    for i in range(E.shape[1]):
        for p in range(int(E[:, i].max(initial=0))):
            out = np.where(E[:, i] > p, out * x[i], out)
    return out


def dphi(E, x):
    """(n_mon, dim): d phi_j / d x_i = E[j, i] * (the monomial with exponents E[j] - 1_i), zero where E[j, i] = 0."""
    D = np.zeros(E.shape, dtype=LD)
    for i in range(E.shape[1]):
        Ei = E.copy()
        Ei[:, i] = np.maximum(Ei[:, i] - 1, 0)
        D[:, i] = ld(E[:, i]) * phi(Ei, x)
    return D


def make_model(n, m, n_o, rom_order, ssm_order, R, B, W, V, z_ref, Rd=None, Bd=None):
    """W (n_o x n_s) is only usable where n_o == n (the reduced -> observed map takes a reduced state)."""
    Er, Es = exponents(n, rom_order), exponents(n_o, ssm_order)
    opt = lambda a: None if a is None else ld(a)
    mdl = dict(n=n, m=m, n_o=n_o, Er=Er, Es=Es, R=ld(R), B=ld(B), W=opt(W), V=ld(V), z_ref=ld(z_ref), Rd=opt(Rd), Bd=opt(Bd))
    assert mdl['R'].shape == (n, Er.shape[0]) and mdl['B'].shape == (n, m) and mdl['V'].shape == (n, Es.shape[0])
    return mdl


def dynamics(model, x, u, discrete=False):
    R, B = (model['Rd'], model['Bd']) if discrete else (model['R'], model['B'])
    return R @ phi(model['Er'], x) + B @ ld(u)


def continuous_jacobians(model, x, u, discrete=False):
    """A = R dphi, B, d = f - A x - B u (of the discrete map's coefficients when `discrete`)."""
    R, B = (model['Rd'], model['Bd']) if discrete else (model['R'], model['B'])
    x, u = ld(x), ld(u)
    A = R @ dphi(model['Er'], x)
    f = R @ phi(model['Er'], x) + B @ u
    return A, B.copy(), f - A @ x - B @ u


def inverse(M):
    """Gauss-Jordan inverse with partial pivoting; the pivot of column k is the FIRST row i >= k with the largest |M[i, k]|.
    Returns (inverse, rows exchanged).  A zero pivot raises (np.linalg.inv raises LinAlgError on a singular matrix)."""
    M = ld(M).copy()
    n = M.shape[0]
    inv = np.eye(n, dtype=LD)
    swaps = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))          # argmax returns the first maximum
        if M[p, k] == 0:
            raise np.linalg.LinAlgError('inverse: singular matrix (zero pivot in column %d)' % k)
        if p != k:
            M[[k, p]] = M[[p, k]]
            inv[[k, p]] = inv[[p, k]]
            swaps += 1
        d = M[k, k]
        M[k] = M[k] / d
        inv[k] = inv[k] / d
        for i in range(n):
            if i != k:
                f = M[i, k]
                M[i] = M[i] - f * M[k]
                inv[i] = inv[i] - f * inv[k]
    return inv, swaps


def discretize(A_c, B_c, d_c, dt, method):
    """ssm.py:279-301."""
    n = A_c.shape[0]
    I, dt = np.eye(n, dtype=LD), LD(dt)
    if method == 'fe':
        return I + dt * A_c, dt * B_c, dt * d_c
    if method == 'be':
        A_d = inverse(I - dt * A_c)[0]
    elif method == 'bil':
        A_d = (I + dt / 2 * A_c) @ inverse(I - dt / 2 * A_c)[0]
    else:
        raise RuntimeError('self.discr_method must be in [fe, be, bil, zoh]')
    sep = inverse(A_c)[0] @ (A_d - I)
    return A_d, sep @ B_c, sep @ d_c


def jacobians(model, x, u, dt=None, method=None):
    """method: None (continuous) | 'fe' | 'be' | 'bil' | 'map' (Jacobians of the discrete map, no discretisation)."""
    if method == 'map':
        return continuous_jacobians(model, x, u, discrete=True)
    A, B, d = continuous_jacobians(model, x, u)
    return (A, B, d) if method is None else discretize(A, B, d, dt, method)


def observe(model, x):
    """C_map without z_ref."""
    assert model['n_o'] == model['n']
    return model['W'] @ phi(model['Es'], x)


def observer_jacobians(model, x):
    """H = W dphi_s, c = z - H x."""
    assert model['n_o'] == model['n']
    H = model['W'] @ dphi(model['Es'], x)
    return H, observe(model, x) - H @ ld(x)


def reduce(model, z):
    """x = V phi_s(z - z_ref), z of dimension n_o."""
    return model['V'] @ phi(model['Es'], ld(z) - model['z_ref'])


def rollout(model, x0, u, dt, method, with_z=True):
    """x_{i+1} = A_d x_i + B_d u_i + d_d, re-linearised at every (x_i, u_i); z_i = C_map(x_i) + z_ref."""
    u = ld(u)
    N = u.shape[0]
    x = np.zeros((N + 1, model['n']), dtype=LD)
    x[0] = ld(x0)
    for i in range(N):
        A, B, d = jacobians(model, x[i], u[i], dt, method)
        x[i + 1] = A @ x[i] + B @ u[i] + d
    z = np.stack([observe(model, xi) for xi in x]) + model['z_ref'] if with_z else None
    return x, z
