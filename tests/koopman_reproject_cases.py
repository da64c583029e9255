"""Seeded cases of the measurement re-projection inside the batched closed-loop Koopman MPC (Y= of KoopmanClosedLoopBatch,
koop_loop_advance_kernel<true> of csrc/koopman_loop.hip), shared by tests/test_koopman_reproject_gpu.py and
tests/test_loop_reproject_cpu.py.

Shapes, the smallest at which the code can go wrong: n_y in {1, 3, 16}, Y of 1 row, of a box plus one oblique facet, of 64 rows, B in
{1, 3}, N = 3, r = 2 simulation steps per controller step, the 8-state plant 'g6' of cl_cases, two or three periods.  The models are
seeded synthetic Koopman models in the manner of koopman_loop_cases.spec (one delay, degree 2, W to 12 rows, the plant's three inputs).

Y lives in raw measurement coordinates.  The replay cases use the box [-0.5, 1]^n of poly_cases, so that "on the face" (1.0 or -0.5 in
one coordinate, zeros elsewhere) and "one ulp outside" are exact in every arithmetic; every other sample is asserted to be at least EDGE
scale from every face."""
import numpy as np

import cl_cases as cc
import koopman_loop_cases as kc
import koopman_loop_reference as kr
import poly_cases as pc

TS, N, R = 0.05, 3, 2
DT_SIM = TS / R
M = 3                                   # the inputs of the plant 'g6'
EDGE = 1e-9                             # no sample that is not on a face exactly may be nearer to one, relative to scale
ULP1 = float(np.nextafter(1.0, 2.0))
NY = (1, 3, 16)
ROWS = ('one', 'box+1', '64')
_cache = {}


def spec(ny):
    """A Koopman model of n_y measurements in the layout of koopman_loop_cases.spec."""
    if ('spec', ny) in _cache:
        return _cache[('spec', ny)]
    rng = np.random.default_rng(7700 + ny)
    d, deg, nw = 1, 2, 12
    nzeta = ny * (d + 1) + M * d
    P = len(kr.exponents(nzeta, deg, False))
    W = np.linalg.qr(rng.standard_normal((P, nw)))[0].T
    A = rng.standard_normal((nw, nw))
    A *= 0.9 / np.abs(np.linalg.eigvals(A)).max()
    s = dict(n_y=ny, m=M, delays=d, degree=deg, dmd=False, W=W, A=A, B=0.1 * rng.standard_normal((nw, M)),
             H=rng.standard_normal((ny, nw)) / np.sqrt(nw), y_offset=rng.uniform(-2.0, 2.0, ny), y_factor=rng.uniform(0.5, 3.0, ny),
             u_offset=rng.uniform(20.0, 60.0, M), u_factor=rng.uniform(30.0, 80.0, M), n_psi=P, n_lift=nw, nzeta=nzeta)
    _cache[('spec', ny)] = s
    return s


def polyhedron(ny, rows):
    """(A, b) of Y in n_y dimensions: 'one' the half space y_0 <= 1, 'box+1' the box [-0.5, 1]^n and one oblique facet, '64' the box
    and seeded facets up to 64 rows (poly_cases.box_and_facets: the origin is strictly inside)."""
    rng = np.random.default_rng(7800 + 10 * ny + ROWS.index(rows))
    if rows == 'one':
        A = np.zeros((1, ny)); A[0, 0] = 1.0
        return A, np.array([1.0])
    if rows == 'box+1':
        return pc.box_and_facets(ny, 2 * ny + 1, rng)
    return pc.box_and_facets(ny, 64, rng)


def scale_of(b, y):
    return max(1.0, float(np.abs(y).max()), float(np.abs(b).max()))


def side(A, b, y):
    """max(A y - b) / scale in float64, numpy's A @ y as the reference's `contains` forms it."""
    return float((A @ y - b).max()) / scale_of(b, y)


def box_face(A, b):
    """(coordinate i, bound v, the value one ulp beyond it) of a face y_i = v of the box rows of Y on which the point v e_i lies strictly
    inside every other row, or None (Y has no box rows, or the seeded facets cut every such point off)."""
    ny = A.shape[1]
    for i in range(ny):
        for v, beyond in ((1.0, ULP1), (-0.5, float(np.nextafter(-0.5, -1.0)))):
            y = np.zeros(ny); y[i] = v
            res = A @ y - b
            on = np.nonzero(res == 0.0)[0]
            if len(on) == 1 and np.count_nonzero(A[on[0]]) == 1 and (np.delete(res, on) < -1e-3).all():
                return i, v, beyond
    return None


def replay_samples(ny, rows, B, n_keep):
    """(Y_plant (B, n_keep + 1, n_y), kinds (B, n_keep + 1)) for the one-launch tests: per member a seeded mix of samples inside, far
    outside (one, two, all coordinates beyond the box), exactly on a face of the box ('face') and one ulp beyond it ('ulp'; both only
    where box_face finds such a face, 'one' otherwise).  Row 0 is where the launch starts (not read)."""
    A, b = polyhedron(ny, rows)
    face = box_face(A, b)
    rng = np.random.default_rng(7900 + 100 * ny + 10 * ROWS.index(rows) + B)
    Y = np.zeros((B, n_keep + 1, ny))
    kinds = np.empty((B, n_keep + 1), dtype=object)
    order = ['inside', 'one', 'face', 'ulp', 'all', 'two']
    for m in range(B):
        for s in range(n_keep + 1):
            kind = order[(s + m) % len(order)]
            if kind in ('face', 'ulp') and face is None:
                kind = 'one'
            y = rng.uniform(-0.2, 0.2, ny)
            if kind == 'one':
                y[0] = 1.0 + rng.uniform(0.3, 2.0)
            elif kind == 'two':
                y[0] = 1.0 + rng.uniform(0.3, 2.0); y[-1] = -0.5 - rng.uniform(0.3, 2.0)
            elif kind == 'all':
                y = np.where(rng.uniform(size=ny) < 0.5, 1.0 + rng.uniform(0.3, 2.0, ny), -0.5 - rng.uniform(0.3, 2.0, ny))
            elif kind in ('face', 'ulp'):
                y = np.zeros(ny); y[face[0]] = face[1] if kind == 'face' else face[2]
            Y[m, s], kinds[m, s] = y, kind
    return Y, kinds


def exact_edge(A, b, y):
    """True where a sample sits on (or one ulp beyond) a face in a way every arithmetic agrees on: one non-zero coordinate, and the rows
    within EDGE of it have a single entry +-1."""
    near = np.abs(A @ y - b) < EDGE * scale_of(b, y)
    return np.count_nonzero(y) <= 1 and all(np.count_nonzero(A[i]) == 1 and abs(A[i]).max() == 1.0 for i in np.nonzero(near)[0])


def check_sides(A, b, Y):
    """Assert the issue's condition on a record of raw samples (any leading shape): none has 0 < |max(A y - b)| < EDGE scale, unless it
    is one of the exact edge samples.  Returns the share of samples outside."""
    out = 0
    flat = np.reshape(Y, (-1, Y.shape[-1]))
    for y in flat:
        if not np.isfinite(y).all():
            continue
        v = side(A, b, y)
        assert v == 0.0 or abs(v) >= EDGE or exact_edge(A, b, y), ('a sample within rounding of a face', y, v)
        out += v > 0.0
    return out / max(1, len(flat))


# ------------------------------------------------------------------------------------------------------------- whole loops
LOOP_NY, LOOP_B, PERIODS, RH = 3, 3, 3, 2          # n_keep = RH R = 4 sub-steps per period


def loop_inputs(B=LOOP_B):
    """The plant 'g6' measured by a seeded C with three rows, the histories, the noise and the target of the whole-loop tests.
    Members 0..2 are the same for every B and differ."""
    s = spec(LOOP_NY)
    mdl = cc.model('g6')['model']
    rng = np.random.default_rng(8100)
    nb, nk = 3, RH * R
    n = 2 * cc.MODELS['g6'][0]
    x0 = np.concatenate((np.zeros((nb, n // 2)), mdl['q'][:nb] + 0.02 * rng.standard_normal((nb, n // 2))), axis=1)
    Cm = s['y_factor'][:, None] * kc.measurement('g6', LOOP_NY, 0)[0]
    T = 60
    t = TS * np.arange(T)
    z = 0.3 * np.stack([np.sin(2 * np.pi * t / 1.5 + p) for p in (0.0, 1.0, 2.0)], axis=1)
    inp = dict(x0=x0, C=Cm, y_ref=s['y_offset'].copy(), phase=np.array([-0.2, 0.37, 1.0]), t=t, z=z,
               y_hist=s['y_offset'] + 0.3 * s['y_factor'] * rng.standard_normal((nb, 1, LOOP_NY)), u_hist=rng.uniform(20.0, 80.0, (nb, 1, M)),
               u_prev0=rng.uniform(20.0, 80.0, (nb, M)), v0=0.3 * s['y_factor'] * rng.standard_normal((nb, LOOP_NY)),
               V=0.3 * s['y_factor'] * rng.standard_normal((PERIODS, nk, nb, LOOP_NY)))
    per_member = ('x0', 'phase', 'y_hist', 'u_hist', 'u_prev0', 'v0')
    return {k: (np.ascontiguousarray(v[:, :, :B]) if k == 'V' else (v[:B] if k in per_member else v)) for k, v in inp.items()}


def member_of(inp, m):
    per_member = ('x0', 'phase', 'y_hist', 'u_hist', 'u_prev0', 'v0')
    return {k: (np.ascontiguousarray(v[:, :, m:m + 1]) if k == 'V' else (v[m:m + 1] if k in per_member else v)) for k, v in inp.items()}


def loop_polyhedron(half=0.5):
    """Y of the whole loops: the box y_ref +- half y_factor and the oblique facet sum((y - y_ref) / y_factor) <= 1.5 half, in raw
    coordinates: the noise of loop_inputs (0.3 y_factor) puts a good share of the samples outside."""
    s = spec(LOOP_NY)
    A = np.kron(np.eye(LOOP_NY), np.array([[1.0], [-1.0]]))
    b = np.ravel([[s['y_offset'][i] + half * s['y_factor'][i], -(s['y_offset'][i] - half * s['y_factor'][i])] for i in range(LOOP_NY)])
    a = 1.0 / s['y_factor']
    return np.vstack([A, a[None]]), np.append(b, 1.5 * half + a @ s['y_offset'])


def containing_polyhedron():
    """A Y that contains every sample of the whole loops by a wide margin."""
    A, b = loop_polyhedron(half=1e3)
    return A, b


def empty_polyhedron():
    """y_0 <= -1e3 and y_0 >= 1e3 in three dimensions: no sample has a projection."""
    A = np.zeros((2, LOOP_NY)); A[0, 0], A[1, 0] = 1.0, -1.0
    return A, np.array([-1e3, -1e3])
