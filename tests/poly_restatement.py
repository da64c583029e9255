"""csrc/poly.hip restated line by line in float64 numpy, for what cannot be read off the device: iteration counts, and what the
algorithm (as opposed to the kernel) does on a case.  Same start, the same two Newton solves per iteration, step rule and shifted
Cholesky (wg::chol_factor); it differs from the kernel in reduction order and FMA contraction.

  rule='feasible'   the exit the kernel had before the closing step: stop at mu <= 1e-13 scale with both residuals <= 1e-10 scale,
                    and after 60 iterations accept any iterate that is feasible to 1e-6 scale.
  rule='certified'  the kernel as it is: once mu <= 1e-9 scale and both residuals <= 1e-6 scale, every iteration tries the closing
                    step (`closing`), and only its certified point is a result.

`project` returns (p, status, interior-point iterations, closing rounds of the successful attempt or -1)."""
import numpy as np

MAX_ITER = 60
IDENT_MU, IDENT_RES, CERT_TOL, DEPENDENT, CLOSING_ROUNDS = 1e-9, 1e-6, 1e-12, 1e-18, 16


def chol_shifted(M):
    n = M.shape[0]
    dmax = np.abs(np.diag(M)).max()
    shift = 0.0
    for _ in range(8):
        Lc = np.zeros_like(M)
        ok = True
        for i in range(n):
            for j in range(i + 1):
                v = M[i, j] + (shift if i == j else 0.0) - Lc[i, :j] @ Lc[j, :j]
                if i == j:
                    if not v > 0.0:
                        ok = False
                        break
                    Lc[i, i] = np.sqrt(v)
                else:
                    Lc[i, j] = v / Lc[j, j]
            if not ok:
                break
        if ok:
            return Lc
        shift = 1e-14 * dmax if shift == 0.0 else shift * 100.0
    return None


def affine_hull_step(A, b, x, in_w):
    """Pivoted modified Gram-Schmidt over the rows of the set: (p, rows taken, their multipliers)."""
    rows, n = A.shape
    z, na2 = A.copy(), (A * A).sum(axis=1)
    h = np.zeros((rows, n))
    taken = np.zeros(rows, dtype=bool)
    p, sel, c, R = x.copy(), [], [], np.zeros((n, n))
    for k in range(n):
        cand = np.where(in_w & ~taken & (na2 > 0), (z * z).sum(axis=1) / np.where(na2 > 0, na2, 1.0), -1.0)
        j = int(np.argmax(cand))
        if not cand[j] > DEPENDENT:
            break
        nz = np.sqrt(z[j] @ z[j])
        q = z[j] / nz
        ck = (A[j] @ p - b[j]) / nz
        R[:k, k], R[k, k] = h[j, :k], nz
        p = p - ck * q
        taken[j] = True
        sel.append(j)
        c.append(ck)
        for _ in range(2):
            g = z @ q
            z = z - np.outer(g, q)
            h[:, k] += g
    lam = np.zeros(len(sel))
    for i in range(len(sel) - 1, -1, -1):
        lam[i] = (c[i] - R[i, i + 1:len(sel)] @ lam[i + 1:]) / R[i, i]
    return p, sel, lam


def closing(A, b, x, lam, s, scale):
    """(certified point or None, rounds)."""
    in_w = lam >= s
    tol = CERT_TOL * scale
    for rnd in range(CLOSING_ROUNDS):
        p, sel, l = affine_hull_step(A, b, x, in_w)
        if sel and not l.min() >= -tol:
            in_w[sel[int(np.argmin(l))]] = False
            continue
        v = A @ p - b
        j = int(np.argmax(v))
        if not np.isfinite(p).all():
            return None, rnd
        if not v[j] > tol:
            return p, rnd
        if in_w[j]:
            return None, rnd
        in_w[j] = True
    return None, CLOSING_ROUNDS


def project(A, b, x, rule='certified'):
    rows, n = A.shape
    scale = max(1.0, np.abs(x).max(), np.abs(b).max())
    p = x.copy()
    viol = A @ p - b
    if not viol.max() > 0:
        return x.copy(), 0, 0, -1
    s, lam = np.maximum(-viol, 1e-2 * scale), np.maximum(viol, 1e-2 * scale)

    def newton(rd, rp, rc):
        with np.errstate(all='ignore'):                 # an empty polyhedron drives s to zero and d to infinity: status 2, as on the device
            d = lam / s
            Lc = chol_shifted(np.eye(n) + (A.T * d) @ A)
            if Lc is None:
                return None
            dp = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, rd + A.T @ (d * rp - rc / s)))
            dlam = d * (A @ dp + rp) - rc / s
            return dp, dlam, -(rc + s * dlam) / lam

    def max_step(v, dv):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(dv < 0, -v / dv, np.inf).min()

    it, st, rpn = 0, 0, np.inf
    while True:
        rd, rp = p - x + A.T @ lam, A @ p + s - b
        rdn, rpn, mu = np.abs(rd).max(), np.abs(rp).max(), (s * lam).sum() / rows
        if rule == 'certified':
            if mu <= IDENT_MU * scale and rpn <= IDENT_RES * scale and rdn <= IDENT_RES * scale:
                pw, rounds = closing(A, b, x, lam, s, scale)
                if pw is not None:
                    return pw, 0, it, rounds
            if it >= MAX_ITER:
                return p, 1, it, -1
        else:
            if mu <= 1e-13 * scale and rpn <= 1e-10 * scale and rdn <= 1e-10 * scale:
                break
            if it >= MAX_ITER:
                st = 1
                break
        r = newton(rd, rp, s * lam)
        if r is None:
            st = 2
            break
        dpa, dla, dsa = r
        aa = min(1.0, max_step(s, dsa), max_step(lam, dla))
        mua = ((s + aa * dsa) * (lam + aa * dla)).sum() / rows
        r = newton(rd, rp, s * lam + dsa * dla - (mua / mu) ** 3 * mu)
        if r is None:
            st = 2
            break
        dp, dl, dsv = r
        al = min(1.0, 0.99 * min(max_step(s, dsv), max_step(lam, dl)))
        p, s, lam = p + al * dp, s + al * dsv, lam + al * dl
        it += 1
    if rule == 'feasible' and st != 0 and np.isfinite(p).all() and (A @ p - b).max() <= 1e-6 * scale and rpn <= 1e-6 * scale:
        st = 0
    return p, st, it, -1


if __name__ == '__main__':
    import poly_cases as pc
    import poly_reference as pr
    for rule in ('feasible', 'certified'):
        print('rule=%s: interior-point iterations (float64 restatement) and worst |p - p*|_2 / scale per family' % rule)
        fam = {}
        for c in pc.cases():
            for x, r in zip(c.X, pc.certified(c)):
                if not (c.A @ x - c.b).max() > 0:
                    continue
                p, st, it, rounds = project(c.A, c.b, x, rule)
                d = p.astype(np.longdouble) - r.p
                fam.setdefault(c.family, []).append((it, float(np.sqrt((d * d).sum())) / pr.scale_of(c.b, x), st, rounds, c.key))
        for f, v in fam.items():
            slow = sorted({k for it, _, _, _, k in v if it > 40})
            print('  %-11s %3d points outside: iterations mean %4.1f max %2d, worst error %.2e, failures %d%s%s'
                  % (f, len(v), np.mean([t[0] for t in v]), max(t[0] for t in v), max(t[1] for t in v), sum(t[2] != 0 for t in v),
                     ', closing rounds max %d' % max(t[3] for t in v) if rule == 'certified' else '',
                     ', more than 40 iterations in %s' % slow if slow else ''))
