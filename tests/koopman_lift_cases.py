"""Cases and seeded data of the exact Koopman lift tests (tests/test_koopman_lift_reference_cpu.py, tests/test_koopman_lift_exact_gpu.py).
Every case is named by what it is the smallest to reach in koop_prepare_launch / koop_lift_kernel; (P, ld, TR, LDS bytes) are written out
here and checked against koopman_lift_reference.tile_model by the CPU test.

INTEGER DATA.  zeta entries in {-3..3}, W entries in {-8..8}; the last zeta variable has magnitude 3 and the last column (k = P - 1) and
last row of W magnitude 8, so the end of every index range carries weight; zeta rows pairwise distinct wherever 2 * 7^(nz - 1) >= rows.
|psi| <= 3^4 = 81, so |sum| <= 1001 * 81 * 8 = 648 648 < 2^20: every partial sum of W psi is an integer far below 2^53 and the product
is exact in any order.
REAL DATA.  zeta uniform in [-1.5, 1.5]; W standard normal, its columns scaled by 10^uniform(-2, 2) (four decades)."""
import functools
import itertools

import numpy as np

import koopman_lift_reference as kr

# name: (nz, degree, dmd, P, ld, TR, lds_bytes)
LIFT_CASES = {
    'one_observable':        (1, 1, True, 1, 4, 64, 2560),        # one observable, one level, no constant
    'one_variable_4_levels': (1, 4, False, 5, 8, 64, 5120),       # one variable through four levels
    'const_beside_padding':  (3, 1, False, 4, 8, 64, 7680),       # P % 4 == 0: ld = P + 4, the constant beside the padding
    'small_dmd':             (3, 2, True, 9, 12, 64, 7680),
    'shipped':               (10, 2, False, 66, 68, 64, 40960),   # the shipped model
    'last_tr64':             (13, 2, False, 105, 108, 64, 64000),  # last TR = 64, last under 64 KiB
    'first_tr32':            (14, 2, False, 120, 124, 32, 35840),  # first TR = 32, P % 4 == 0
    'first_over_64k':        (20, 2, False, 231, 232, 32, 66560),  # first launch over 64 KiB
    'first_tr16':            (21, 2, True, 252, 256, 16, 35840),   # first TR = 16, P % 4 == 0
    'widest_zeta':           (64, 1, False, 65, 68, 32, 35840),    # nz = 64: TR drops because of nz, not P
    'widest_zeta_dmd':       (64, 1, True, 64, 68, 32, 35840),
    'degree3_near_cap':      (16, 3, False, 969, 972, 16, 128000),
    'widest_near_cap':       (43, 2, False, 990, 992, 16, 133120),  # the largest request
    'most_observables':      (10, 4, False, 1001, 1004, 16, 130560),
    'most_observables_dmd':  (10, 4, True, 1000, 1004, 16, 130560),
}
REFUSED = [(44, 2), (11, 4)]                     # more than 1024 observables
FULL_ROWS = {64: 'shipped', 32: 'first_tr32', 16: 'first_tr16'}     # one case per TR class runs every row count
W_CASES = ['shipped', 'first_tr32', 'first_tr16', 'most_observables', 'most_observables_dmd']
NW_LIST = (1, 15, 16, 17, 33)                    # and P
KINDS = ('int', 'real')

# (n_y, m, delays, degree, dmd): nz = 1, 10, 7, 17, 60; TR = 64, 64, 16, 32, 64
RECORD_CASES = {
    'no_input_column': (1, 1, 0, 4, False),
    'shipped':         (3, 4, 1, 2, False),
    'two_delays_tr16': (1, 2, 2, 4, False),
    'three_delays_tr32': (2, 3, 3, 2, False),
    'nz60':            (4, 4, 7, 1, False),
}
# (n_y, m, delays, degree, dmd, with_w): nz = 2, 6, 10, 14 (TR = 32), and a TR = 16 handle; W on one handle of each TR class
RING_CASES = {
    'delays0': (2, 2, 0, 2, False, False),
    'delays1': (2, 2, 1, 2, True, False),
    'delays1_w': (2, 2, 1, 2, False, True),
    'delays2': (2, 2, 2, 2, False, False),
    'delays3_tr32': (2, 2, 3, 2, False, False),
    'delays3_tr32_w': (2, 2, 3, 2, False, True),
    'delays2_tr16_w': (1, 2, 2, 4, False, True),
}


def case(name):
    nz, degree, dmd, P, ld, TR, lds = LIFT_CASES[name]
    return dict(name=name, nz=nz, degree=degree, dmd=dmd, P=P, ld=ld, TR=TR, lds=lds)


def rows_of(name):
    TR = LIFT_CASES[name][5]
    if FULL_ROWS[TR] == name:
        return sorted({1, 15, 16, 17, TR - 1, TR, TR + 1, 2 * TR + 1})
    return sorted({1, 17, TR + 1})


def w_rows_of(name):
    TR = LIFT_CASES[name][5]
    return sorted({1, 15, TR - 1, TR + 1})


def nw_of(name):
    P = LIFT_CASES[name][3]
    return [n for n in NW_LIST if n <= P] + [P]


def _seed(*key):
    """A seed that depends on the key's text alone (Python's hash of a string changes from process to process)."""
    return sum((i + 1) * ord(c) for i, c in enumerate('|'.join(str(k) for k in key)))


def distinct_int_rows(rng, rows, ncols, pinned):
    """(rows, ncols) integers in {-3..3}, the `pinned` columns in {-3, 3}; pairwise distinct rows wherever the shape has room."""
    free = [c for c in range(ncols) if c not in pinned]
    room = 7 ** len(free) * 2 ** len(pinned)
    out = np.empty((rows, ncols))
    if room <= 20000:
        combos = np.array(list(itertools.product(*[([-3, 3] if c in pinned else range(-3, 4)) for c in range(ncols)])), dtype=float)
        pick = rng.permutation(room)[:min(rows, room)]
        out[:len(pick)] = combos[pick]
        if rows > room:
            out[room:] = combos[rng.integers(0, room, rows - room)]
        return out
    seen = set()
    r = 0
    while r < rows:
        v = rng.integers(-3, 4, ncols).astype(float)
        for c in pinned:
            v[c] = rng.choice([-3.0, 3.0])
        if tuple(v) in seen:
            continue
        seen.add(tuple(v))
        out[r] = v
        r += 1
    return out


@functools.lru_cache(maxsize=None)
def zeta(name, kind):
    """The master zeta rows of a lift case (the most rows the case runs); a run of R rows takes the first R."""
    nz = LIFT_CASES[name][0]
    R = max(rows_of(name) + w_rows_of(name))
    rng = np.random.default_rng(_seed('zeta', name, kind))
    Z = distinct_int_rows(rng, R, nz, [nz - 1]) if kind == 'int' else rng.uniform(-1.5, 1.5, (R, nz))
    Z.setflags(write=False)
    return Z


def make_w(Nw, P, kind, key):
    rng = np.random.default_rng(_seed('W', Nw, P, kind, key))
    if kind == 'int':
        W = rng.integers(-8, 9, (Nw, P)).astype(float)
        W[:, P - 1] = rng.choice([-8.0, 8.0], Nw)
        W[Nw - 1, :] = rng.choice([-8.0, 8.0], P)
    else:
        W = rng.standard_normal((Nw, P)) * 10.0 ** rng.uniform(-2.0, 2.0, P)
    return W


@functools.lru_cache(maxsize=None)
def w_of(name, Nw, kind):
    W = make_w(Nw, LIFT_CASES[name][3], kind, name)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def exps(nz, degree, dmd):
    E = kr.exponents(nz, degree, dmd)
    E.setflags(write=False)
    return E


@functools.lru_cache(maxsize=None)
def psi_of(name, kind, ld):
    """psi of the master zeta rows: float64 twin (ld False) or long double (ld True)."""
    c = case(name)
    out = kr.psi(zeta(name, kind), exps(c['nz'], c['degree'], c['dmd']), np.longdouble if ld else np.float64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def w_reference(name, Nw, kind):
    """(expected, bound) of the master rows: int -> (float64 psi @ W^T, None); real -> (long-double psi W^T, w_bound)."""
    c = case(name)
    W = w_of(name, Nw, kind)
    if kind == 'int':
        return kr.project(psi_of(name, kind, False), W, np.float64), None
    pl = psi_of(name, kind, True)
    return kr.project(pl, W, np.longdouble), kr.w_bound(pl, W, c['P'], c['degree'])


# ------------------------------------------------------------------------------------------------------------ records and ring samples
def scales(n_y, m, kind, key):
    """(y_offset, y_factor, u_offset, u_factor): integer data -- powers of two and integer offsets, so that (raw - off) / fac is again
    the integer it was made from; real data -- factors that are no powers of two."""
    rng = np.random.default_rng(_seed('scale', n_y, m, kind, key))
    if kind == 'int':
        return (rng.integers(-5, 6, n_y).astype(float), 2.0 ** rng.integers(-2, 3, n_y), rng.integers(-5, 6, m).astype(float),
                2.0 ** rng.integers(-2, 3, m))
    return (rng.uniform(-1, 1, n_y), rng.uniform(0.55, 2.9, n_y), rng.uniform(-1, 1, m), rng.uniform(0.55, 2.9, m))


def samples(count, n_y, m, delays, kind, scale, key):
    """`count` raw samples [y | u] whose scaled values are integer data ({-3..3}, pairwise distinct rows where there is room, the column
    that ends zeta of magnitude 3) or real data (uniform in [-1.5, 1.5] before the scaling is undone)."""
    rng = np.random.default_rng(_seed('samples', count, n_y, m, delays, kind, key))
    yo, yf, uo, uf = scale
    if kind == 'int':
        pinned = [n_y + m - 1] + ([n_y - 1] if delays == 0 else [])
        S = distinct_int_rows(rng, count, n_y + m, pinned)
    else:
        S = rng.uniform(-1.5, 1.5, (count, n_y + m))
    return S[:, :n_y] * yf + yo, S[:, n_y:] * uf + uo


def record_dims(name):
    n_y, m, delays, degree, dmd = RECORD_CASES[name]
    nz = n_y * (delays + 1) + m * delays
    P = kr.n_psi(nz, degree, dmd)
    return dict(n_y=n_y, m=m, delays=delays, degree=degree, dmd=dmd, nz=nz, P=P, TR=kr.tile_model(nz, P)[1])


def record_lengths(name):
    d = record_dims(name)
    return [d['delays'], d['delays'] + 1, d['delays'] + d['TR'], d['delays'] + d['TR'] + 1]


def ring_dims(name):
    n_y, m, delays, degree, dmd, with_w = RING_CASES[name]
    nz = n_y * (delays + 1) + m * delays
    P = kr.n_psi(nz, degree, dmd)
    return dict(n_y=n_y, m=m, delays=delays, degree=degree, dmd=dmd, with_w=with_w, nz=nz, P=P, TR=kr.tile_model(nz, P)[1])
