"""Extended-precision statements of the linear-quadratic problems behind csrc/lqr.hip (test infrastructure only).

Plain numpy in np.longdouble (80-bit on x86: eps 1.1e-19; np.linalg has no long-double path, hence the hand-written
Cholesky).  Nothing here imports the package under test or the float64 oracle: the float64 statements in oracle/lqr.py
are *measured* against this module (tests/test_lq_reference_cpu.py), and that measured error sets the tolerance of the
kernels (tests/test_lqr_exact_gpu.py)."""
import numpy as np

LD = np.longdouble


def ld(a):
    return np.asarray(a, dtype=LD)


def err(a, b):
    """The project's error measure: max|a - b| / max(1, max|b|), b the reference."""
    a, b = ld(a), ld(b)
    return float(np.abs(a - b).max() / max(LD(1), np.abs(b).max()))


def chol_solve(S, B):
    """S^-1 B for a small symmetric positive definite S (m <= 16): Cholesky S = L L^T, two triangular solves."""
    S, B = ld(S), ld(B)
    m = S.shape[0]
    assert S.shape == (m, m) and m <= 16
    vec = B.ndim == 1
    Y = B.reshape(m, -1).copy()
    L = np.zeros((m, m), dtype=LD)
    for i in range(m):
        for j in range(i + 1):
            s = S[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                if not s > 0:
                    raise np.linalg.LinAlgError('chol_solve: matrix is not positive definite')
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    for i in range(m):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y[:, 0] if vec else Y.reshape(B.shape)


def sym(P):
    return (P + P.T) / 2


def lq_tracking(A, B, d, H, z_ref, Q, R, Qf, z_target, x0, N):
    """Exact minimiser of  sum_{t<N} 1/2 |H x_t + z_ref - z*_t|^2_Q + 1/2 u_t' R u_t  +  1/2 |H x_N + z_ref - z*_N|^2_Qf
    subject to x+ = A x + B u + d: affine Riccati recursion, Joseph-form P update, symmetrised every step.
    Returns x (N+1, n), u (N, m), K (N, m, n), cost -- all long double."""
    A, B, d, H, Q, R, Qf, x0 = ld(A), ld(B), ld(d), ld(H), ld(Q), ld(R), ld(Qf), ld(x0)
    c = ld(z_ref)[None, :] - ld(z_target)                      # z - z* = H x + c_t
    n, m = B.shape
    P = sym(H.T @ Qf @ H)
    p = H.T @ (Qf @ c[N])
    HQH = sym(H.T @ Q @ H)
    K = np.zeros((N, m, n), dtype=LD)
    k = np.zeros((N, m), dtype=LD)
    for t in range(N - 1, -1, -1):
        PB = P @ B
        Quu = sym(R + B.T @ PB)
        g = p + P @ d                                          # gradient of V_{t+1} at A x + B u + d, x = 0, u = 0
        K[t] = -chol_solve(Quu, PB.T @ A)
        k[t] = -chol_solve(Quu, B.T @ g)
        Acl = A + B @ K[t]
        e = B @ k[t] + d
        p = H.T @ (Q @ c[t]) + K[t].T @ (R @ k[t]) + Acl.T @ (P @ e + p)
        P = sym(HQH + K[t].T @ R @ K[t] + Acl.T @ P @ Acl)
    x = np.zeros((N + 1, n), dtype=LD)
    u = np.zeros((N, m), dtype=LD)
    x[0] = x0
    cost = LD(0)
    for t in range(N):
        u[t] = K[t] @ x[t] + k[t]
        dz = H @ x[t] + c[t]
        cost += dz @ Q @ dz / 2 + u[t] @ R @ u[t] / 2
        x[t + 1] = A @ x[t] + B @ u[t] + d
    dz = H @ x[N] + c[N]
    cost += dz @ Qf @ dz / 2
    return x, u, K, cost


def tvlqr(A, B, Q, R):
    """oracle/lqr.py:tvlqr line for line in long double: per-step (A_i, B_i) in forward time order, terminal P = Q.
    Returns K (n, m, nx), P (n + 1, nx, nx) in forward order."""
    A, B, Q, R = ld(A), ld(B), ld(Q), ld(R)
    n = A.shape[0]
    P = [Q]
    K = []
    for i in reversed(range(n)):
        Ki = -chol_solve(R + B[i].T @ P[-1] @ B[i], B[i].T @ P[-1] @ A[i])
        K.append(Ki)
        Acl = A[i] + B[i] @ Ki
        P.append(Q + Ki.T @ R @ Ki + Acl.T @ P[-1] @ Acl)
    return np.flip(np.asarray(K), axis=0), np.flip(np.asarray(P), axis=0)


def fixed_point_dare(A, B, Q, R, tol=1e-4, max_iter=100000):
    """oracle/lqr.py:solve_riccati in long double.  Returns L, P, the iteration count and (||L - L_old||_F of the
    iteration before the last, of the last): the distance of both from `tol` says whether a float64 evaluation can
    legitimately stop one iteration earlier or later."""
    A, B, Q, R = ld(A), ld(B), ld(Q), ld(R)
    n, m = B.shape
    P = np.zeros((n, n), dtype=LD)
    L = np.zeros((m, n), dtype=LD)
    Lold = np.full((m, n), np.inf, dtype=LD)
    it = 0
    steps = [np.inf, np.inf]
    while it < max_iter:
        dist = np.sqrt(((L - Lold) ** 2).sum()) if it > 0 else LD(np.inf)
        steps = [steps[1], float(dist)]
        if not dist > tol:
            break
        Lold = L
        S = R + B.T @ P @ B
        BPA = B.T @ P @ A
        P = A.T @ P @ A - BPA.T @ chol_solve(S, BPA) + Q
        L = -chol_solve(R + B.T @ P @ B, B.T @ P @ A)
        it += 1
    return L, P, it, tuple(steps)


def kkt_tracking(A, B, d, H, z_ref, Q, R, Qf, z_target, x0, N):
    """The same problem as lq_tracking as one dense float64 KKT system (tiny sizes only): x (N+1, n), u (N, m)."""
    A, B, d, H = (np.asarray(v, dtype=np.float64) for v in (A, B, d, H))
    n, m = B.shape
    c = np.asarray(z_ref)[None, :] - np.asarray(z_target)
    nv = N * (n + m)                                          # w = (u_0, x_1, u_1, x_2, ..., u_{N-1}, x_N)
    Hq = np.zeros((nv, nv)); g = np.zeros(nv)
    E = np.zeros((N * n, nv)); b = np.zeros(N * n)
    iu = lambda t: t * (n + m)
    ix = lambda t: (t - 1) * (n + m) + m                      # t >= 1
    for t in range(N):
        Hq[iu(t):iu(t) + m, iu(t):iu(t) + m] = R
    for t in range(1, N + 1):
        W = Qf if t == N else Q
        Hq[ix(t):ix(t) + n, ix(t):ix(t) + n] = H.T @ W @ H
        g[ix(t):ix(t) + n] = H.T @ W @ c[t]
    for t in range(N):                                        # x_{t+1} - A x_t - B u_t = d
        r0 = t * n
        E[r0:r0 + n, ix(t + 1):ix(t + 1) + n] = np.eye(n)
        E[r0:r0 + n, iu(t):iu(t) + m] = -B
        if t == 0:
            b[r0:r0 + n] = d + A @ x0
        else:
            E[r0:r0 + n, ix(t):ix(t) + n] = -A
            b[r0:r0 + n] = d
    KKT = np.block([[Hq, E.T], [E, np.zeros((N * n, N * n))]])
    w = np.linalg.solve(KKT, np.concatenate([-g, b]))[:nv]
    x = np.zeros((N + 1, n)); u = np.zeros((N, m))
    x[0] = x0
    for t in range(N):
        u[t] = w[iu(t):iu(t) + m]
        x[t + 1] = w[ix(t + 1):ix(t + 1) + n]
    return x, u
