"""The cases of the polyhedron projection's exact tests (csrc/poly.hip, spoly_project): named, seeded families, each the smallest
shape that reaches the edge it is listed for.  A case is one polyhedron (A, b) and a handful of points X; `cases()` lists every case
the reference must certify, `FAILURES` the ones on which the call must fail.  tests/test_poly_reference_cpu.py certifies all of
them without a GPU; tests/test_poly_exact_gpu.py runs the kernel on them.

The bounds (poly_reference.py has the derivation), relative to scale = max(1, |x|_inf, |b|_inf), the kernel's own:
  CONTRACT        1e-9: every certified case whatever its margin (pr.CONTRACT).
  WELL_SEPARATED  for the cases whose margin (smallest active multiplier or inactive slack) is at least 1e-3 scale: eight times the
                  worst error measured on the MI355X over exactly those cases (profiles/poly_exact.log), the headroom being for
                  reduction order across compiler versions."""
import numpy as np

import poly_reference as pr

WELL_SEPARATED_MARGIN = 1e-3
WELL_SEPARATED_MEASURED = 1.058e-15     # worst |p - p*|_2 / scale over the 147 well-separated points (profiles/poly_exact.log)
WELL_SEPARATED = 8.5e-15                # eight times that


class Case:
    def __init__(self, key, A, b, X, p_star=None, lam_star=None, margin=None):
        self.key = key
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
        # constructed cases: the solution, its multipliers (rows x points -> points x rows) and the margin each point claims
        self.p_star, self.lam_star, self.margin = p_star, lam_star, margin

    @property
    def family(self):
        return self.key.split('/')[0]


def box(n, ub=1.0, lb=-1.0):
    """Rows +e_i, -e_i alternating, b = [ub, -lb, ...] (HyperRectangle's layout)."""
    return np.kron(np.eye(n), np.array([[1.0], [-1.0]])), np.tile([ub, -lb], n)


def box_and_facets(n, rows, rng):
    """The first `rows` rows of: the box [-0.5, 1]^n, then random facets a.p <= 0.8 .. 1.3 (the origin is strictly inside)."""
    A, b = box(n, 1.0, -0.5)
    extra = max(0, rows - 2 * n)
    if extra:
        A = np.vstack([A, rng.standard_normal((extra, n))])
        b = np.concatenate([b, 0.8 + rng.uniform(0, 0.5, extra)])
    return A[:rows], b[:rows]


# ---------------------------------------------------------------------------------------------------- 1. limits of the wave
LIMIT_N = (1, 2, 15, 16)
LIMIT_ROWS = (1, 2, 63, 64)


def limits():
    out = []
    for n in LIMIT_N:
        for rows in LIMIT_ROWS + ((10,) if n >= 15 else ()):       # rows < n: 1, 2 and 10 rows in 15 / 16 dimensions
            rng = np.random.default_rng(7000 + 100 * n + rows)
            A, b = box_and_facets(n, rows, rng)
            X = rng.uniform(-2.5, 2.5, (3, n))
            out.append(Case('limits/n%d_r%d' % (n, rows), A, b, X))
    for n in (15, 16):                                              # no idle lane at n = 16: more points, looking for slow ones
        rng = np.random.default_rng(7900 + n)
        A, b = box_and_facets(n, 64, rng)
        out.append(Case('limits/full_n%d' % n, A, b, rng.uniform(-2.5, 2.5, (12, n))))
    return out


# -------------------------------------------------------------------------------------------------------- 2. margin ladder
LADDER = (1.0, 1e-3, 1e-6, 1e-9, 0.0)
LADDER_SLACK = (1e-3, 1e-6, 1e-9)


def ladder():
    """The box [-1, 1]^3.  Multipliers: p* = (1, 1, 0.0) with rows x0 <= 1, x1 <= 1 active, lam* = (1, l): x = (2, 1 + l, 0.0);
    l = 0 is the weakly active corner.  Slacks: p* = (1, 1 - d, 0.0) with row x0 <= 1 alone active: x = (2, 1 - d, 0.0)."""
    A, b = box(3)
    X, P, LAM, M = [], [], [], []
    for l in LADDER:
        le = (1.0 + l) - 1.0                  # the multiplier of the float64 point: l to one rounding of 1 + l
        X.append([2.0, 1.0 + l, 0.0]); P.append([1.0, 1.0, 0.0]); LAM.append([1.0, 0, le, 0, 0, 0]); M.append(le)
    for d in LADDER_SLACK:
        X.append([2.0, 1.0 - d, 0.0]); P.append([1.0, 1.0 - d, 0.0]); LAM.append([1.0, 0, 0, 0, 0, 0]); M.append(1.0 - (1.0 - d))
    return [Case('ladder/box3', A, b, X, np.array(P), np.array(LAM), np.array(M))]


# ------------------------------------------------------------------------------- 3. barely outside and on the boundary
ULP1 = float(np.nextafter(1.0, 2.0))


def boundary():
    """The box [-1, 1]^2.  `outside`: violations 1e-3, 1e-9, 1e-15 and one ulp of the face x0 <= 1, and of the vertex (1, 1).
    `on`: points on a face, at a vertex and inside, with -0.0 coordinates: viol == 0, so they must come back bit for bit."""
    A, b = box(2)
    outside = [[1 + 1e-3, 0.3], [1 + 1e-9, 0.3], [1 + 1e-15, 0.0], [ULP1, 0.3], [1 + 1e-9, -0.0], [ULP1, ULP1], [1 + 1e-9, 1 + 1e-15],
               [-1 - 1e-9, -0.0]]
    expect = [[1, 0.3], [1, 0.3], [1, 0.0], [1, 0.3], [1, -0.0], [1, 1], [1, 1], [-1, -0.0]]
    on = [[1.0, 0.3], [1.0, 1.0], [-1.0, 1.0], [1.0, -0.0], [-0.0, -0.0], [-0.0, 0.5], [0.0, -1.0]]
    return [Case('boundary/outside', A, b, outside, np.array(expect, dtype=np.float64)), Case('boundary/on', A, b, on, np.array(on))]


# ---------------------------------------------------------------------------------------------------- 4. degenerate geometry
def degenerate():
    out = []
    rng = np.random.default_rng(7400)
    # twenty facets through one vertex of R^3: integer normals with a positive component along (1, 1, 1), a dyadic vertex
    v0 = np.array([0.5, -0.25, 0.75])
    N = []
    while len(N) < 20:
        a = rng.integers(-4, 5, 3).astype(np.float64)
        if a.sum() > 0 and not any(np.array_equal(a, q) for q in N):
            N.append(a)
    A = np.array(N)
    X = np.array([v0 + 0.7, v0 + [2.0, 0.1, -0.3], v0 + [0.05, 0.9, 0.4], v0 - [0.2, 0.1, 0.3]])
    out.append(Case('degenerate/vertex20', A, A @ v0, X))
    # every row twice
    A, b = box_and_facets(4, 10, rng)
    out.append(Case('degenerate/duplicated', np.repeat(A, 2, axis=0), np.repeat(b, 2), rng.uniform(-2.5, 2.5, (4, 4))))
    # a . p <= c and -a . p <= -c: the plane a . p = c inside a box, no strict interior
    a = np.array([1.0, 2.0, -1.0])
    A, b = box(3, 2.0, -2.0)
    out.append(Case('degenerate/equality', np.vstack([a, -a, A]), np.concatenate([[0.5, -0.5], b]),
                    [[1.5, 1.0, -1.0], [-1.0, -1.0, 1.5], [3.0, 0.0, 0.0], [0.25, 0.125, 0.0]]))
    # a slab of width 1e-9
    out.append(Case('degenerate/slab', np.vstack([a, -a, A]), np.concatenate([[0.5, -0.5 + 1e-9], b]),
                    [[1.5, 1.0, -1.0], [-1.0, -1.0, 1.5], [3.0, 0.0, 0.0]]))
    # a sharp wedge y <= -1e4 |x| with its apex at the origin
    out.append(Case('degenerate/wedge', [[1.0, 1e-4], [-1.0, 1e-4]], [0.0, 0.0],
                    [[0.0, 1.0], [0.5, 0.0], [1e-5, 1e-9], [-0.3, -1000.0], [1e-3, -5.0]]))
    return out


# --------------------------------------------------------------------------------------------------------------- 5. scale
SMALL_BOXES = (0.02, 1e-4, 1e-6, 1e-8)


def scale():
    out = []
    A, b = box(3)
    out.append(Case('scale/far_points', A, b, [[1e6, -3e5, 0.2], [1e3, 2.0, -1e6], [-1e6, -1e6, 1e6], [30.0, 0.5, -0.5]]))
    rng = np.random.default_rng(7500)
    A, b = box(4, 1.0, -0.5)
    f = np.logspace(-3, 3, 8)
    out.append(Case('scale/row_norms', A * f[:, None], b * f, rng.uniform(-2.5, 2.5, (4, 4))))
    for h in SMALL_BOXES:           # scale is floored at 1: the contract is 1e-9 absolute here, a tenth of the last box
        A, b = box(3, h, -h)
        out.append(Case('scale/box_%g' % h, A, b, h * np.array([[2.0, 0.3, -0.4], [1.5, -3.0, 1.0], [1.0 + 1e-3, 0.0, 0.0], [40.0, 40.0, -40.0]])))
    return out


# --------------------------------------------------------------------------------------------------------------- 6. batch
def batch():
    """n = 5, the box and three facets; 65 points, the even ones inside (the origin is strictly inside), the odd ones outside."""
    rng = np.random.default_rng(7600)
    A, b = box_and_facets(5, 13, rng)
    X = rng.uniform(-2.5, 2.5, (65, 5))
    X[0::2] = rng.uniform(-0.2, 0.2, X[0::2].shape)
    assert (X[0::2] @ A.T - b).max() < 0 and ((X[1::2] @ A.T - b).max(axis=1) > 0).all()
    return [Case('batch/n5_r13', A, b, X)]


# ------------------------------------------------------------------------------------------------------------ 7. failures
def empty():
    """x <= -1 and x >= 1."""
    return np.array([[1.0], [-1.0]]), np.array([-1.0, -1.0])


FAILURES = ('empty', 'empty_in_batch', 'nan', 'inf', 'nan_in_batch', 'inf_in_batch')


def failure(name):
    """(A, b, X, index of the point the message must name, word the message must hold)."""
    if name == 'empty':
        A, b = empty()
        return A, b, np.array([[3.0]]), 0, 'empty'
    if name == 'empty_in_batch':            # the second coordinate is boxed, the first has no admissible value; every point fails: the first is named
        A = np.array([[1.0, 0], [-1.0, 0], [0, 1.0], [0, -1.0]])
        return A, np.array([-1.0, -1.0, 1.0, 1.0]), np.array([[0.0, 3.0], [2.0, 0.5]]), 0, 'empty'
    A, b = box(2)
    bad = np.nan if name.startswith('nan') else -np.inf
    if name.endswith('in_batch'):
        X = np.array([[0.1, 0.2], [3.0, 0.5], [0.3, bad], [2.0, 2.0]])
        return A, b, X, 2, 'finite'
    return A, b, np.array([[bad, 0.5]]), 0, 'finite'


def cases():
    return limits() + ladder() + boundary() + degenerate() + scale() + batch()


def n_points():
    return sum(len(c.X) for c in cases())


_certified = {}


def certified(case):
    """[pr.Projection] of every point of the case, computed once and shared."""
    if case.key not in _certified:
        _certified[case.key] = [pr.project(case.A, case.b, x) for x in case.X]
    return _certified[case.key]


def bound_for(case, i):
    """The asserted |p - p*|_2 of point i, absolute."""
    sc = pr.scale_of(case.b, case.X[i])
    rel = WELL_SEPARATED if certified(case)[i].margin >= WELL_SEPARATED_MARGIN * sc else pr.CONTRACT
    return rel * sc
