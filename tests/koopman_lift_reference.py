"""Reference statement of the Koopman lift (csrc/koopman.hip: koop_lift_kernel in its three zeta modes, launched by koop_launch_lift of
csrc/koopman_host.h): the delay embedding and scaling of get_zeta / scale_down (sofacontrol/baselines/koopman/koopman_utils.py:30-47,
104-107), the monomial observables of get_lifting_function (156-175) and the optional projection W psi.  The same code runs in np.float64
(the twin that the device must meet bit for bit) and in np.longdouble (the reference of the derived bound of W psi).  It imports neither the
package nor oracle/.

WHAT IS EXACT.  An observable is a product of zeta entries and nothing else, multiplied in one fixed order, so IEEE double arithmetic gives
one answer: `psi(.., np.float64)` and the device agree in every bit or one of them is wrong.  The scaling is one subtraction and one
division, the same.  Only W psi is a sum, and only there does the order (the MFMA's, four k per step, fused or not) matter: on integer data
small enough every partial sum is an integer below 2^53 and the order is immaterial again; on real data `w_bound` holds for every order."""
import numpy as np

from koopman_loop_reference import exponents, scale_down  # noqa: F401  (one statement of the observables' order for every Koopman test)

U = 2.0 ** -53          # unit roundoff of float64
KP_MAX_NZ, KP_MAX_DEG, KP_MAX_PSI = 64, 4, 1024     # the limits of skoop_create
LDS_TARGET = 64 * 1024  # the tile is halved until it fits this, down to 16 rows
LDS_UNIT = 2560         # srh::lds_request rounds a request up to whole units of this many bytes
LDS_CU = 160 * 1024


def factors(E):
    """Per observable the variables it multiplies, in the order it multiplies them: ascending index, each repeated by its exponent."""
    return [[i for i in range(E.shape[1]) for _ in range(int(e[i]))] for e in E]


def psi(Z, E, dtype):
    """(rows, n_psi) observables of the zeta rows Z (rows, nzeta) for the exponent rows E of `exponents`.

    Observable k is the product of its variables in ascending index order, each repeated by its exponent, multiplied left to right:
    z1^2 z3 is (z1 * z1) * z3.  The constant (an all-zero exponent row) is exactly 1.  This is the order that par[] / var[] of skoop_create
    produce: var[k] is the LAST non-zero variable of row k and par[k] the observable with the same exponents and one removed from that
    variable, so psi[k] = psi[par[k]] * zeta[var[k]] unrolls, level by level, to the ascending left-to-right product; a degree-1
    observable is 1.0 * z = z, exactly.  With dtype np.float64 every product rounds as the kernel's does (a double multiplication has one
    answer), so the result is the kernel's bit for bit; with np.longdouble it is the reference of `w_bound`."""
    Z = np.asarray(Z, dtype=dtype)
    out = np.empty((Z.shape[0], len(E)), dtype=dtype)
    for k, f in enumerate(factors(E)):
        if not f:
            out[:, k] = dtype(1)
            continue
        acc = Z[:, f[0]].copy()
        for v in f[1:]:
            acc = acc * Z[:, v]
        out[:, k] = acc
    return out


def zeta_record(y, u, delays, scale, dtype):
    """(T - delays, nzeta) rows [y_t, y_{t-1} .. y_{t-d}, u_{t-1} .. u_{t-d}] for t = delays .. T - 1 of a raw record y (T, n_y), u (T, m);
    scale = (y_offset, y_factor, u_offset, u_factor), applied as (v - off) / fac -- scale_down, the kernel's two operations in its order."""
    yo, yf, uo, uf = scale
    ys, us = scale_down(y, yo, yf, dtype), scale_down(u, uo, uf, dtype)
    T = ys.shape[0]
    rows = []
    for t in range(delays, T):
        rows.append(np.concatenate([ys[t]] + [ys[t - j] for j in range(1, delays + 1)] + [us[t - j] for j in range(1, delays + 1)]))
    nz = ys.shape[1] * (delays + 1) + us.shape[1] * delays
    return np.array(rows, dtype=dtype).reshape(len(rows), nz)


def zeta_ring(pushed, delays, scale, dtype):
    """(batch, nzeta) zeta of every member after the pushes `pushed`: the chronological list of (y (batch, n_y), u (batch, m)) raw samples
    given to `push`, oldest first (at least delays + 1 of them).  Built from that list alone -- the newest sample is the last entry, sample
    t - j the entry j before it -- and not from any model of slots and heads."""
    yo, yf, uo, uf = scale
    ys = [scale_down(np.atleast_2d(p[0]), yo, yf, dtype) for p in pushed]
    us = [scale_down(np.atleast_2d(p[1]), uo, uf, dtype) for p in pushed]
    assert len(pushed) >= delays + 1
    return np.concatenate([ys[-1]] + [ys[-1 - j] for j in range(1, delays + 1)] + [us[-1 - j] for j in range(1, delays + 1)], axis=1)


def lds_request(nbytes):
    """srh::lds_request (csrc/common.h): whole 2560-byte units, capped at the 160 KiB of a CU."""
    r = (nbytes + LDS_UNIT - 1) // LDS_UNIT * LDS_UNIT
    return r if r < LDS_CU else (nbytes if nbytes > LDS_CU else LDS_CU)


def tile_model(nz, P):
    """(ld, TR, lds_bytes) of a handle, restating koop_prepare_launch: ld = P rounded up to 4, plus 4 where that equals P; TR = 64 halved
    while TR * 8 * (ld + nz) exceeds 64 KiB, down to 16; the request is that product through lds_request."""
    ld = (P + 3) // 4 * 4
    if ld == P:
        ld += 4
    row_bytes = 8 * (ld + nz)
    TR = 64
    while TR > 16 and TR * row_bytes > LDS_TARGET:
        TR //= 2
    return ld, TR, lds_request(TR * row_bytes)


def n_psi(nz, degree, dmd):
    c = 1
    for i in range(1, degree + 1):
        c = c * (nz + i) // i
    return c - 1 + (0 if dmd else 1)


def project(P_, W, dtype):
    """psi W^T in `dtype` (numpy's own summation order)."""
    return np.asarray(P_, dtype=dtype) @ np.asarray(W, dtype=dtype).T


def w_bound(psi_ld, W, P, degree):
    """Elementwise bound (P + 4 + degree) 2^-53 (|psi| |W|^T) on |computed - exact| of out = psi W^T, for the kernel and for any other
    float64 evaluation that sums at most P + 4 terms per entry.  psi_ld: the long-double observables (rows, P); W (Nw, P) float64.

    Derivation, with u = 2^-53 and out_rj = sum_k psi_rk W_jk:
      * the computed psi_k is a product of `degree` factors at the most, so it carries at most degree - 1 roundings:
        |psi~_k - psi_k| <= ((1 + u)^(degree - 1) - 1) |psi_k|;
      * each term psi~_k W_jk is rounded once as a product (not at all when the multiply is fused into the add) and then passes through
        at most ld <= P + 4 additions -- the kernel's k loop adds ld terms to an accumulator that starts at zero -- whatever their
        order: a sum of n terms formed by any n - 1 or n additions perturbs each term by at most (1 + u)^n - 1 relative [Higham,
        Accuracy and Stability of Numerical Algorithms, Sec. 4.2];
      * the padding columns P .. ld - 1 hold exact zeros on both operands: they add 0.0, which rounds nothing, and ld > P always, so
        at most P + 3 of those additions can round;
      * together at most (degree - 1) + 1 + (P + 3) roundings per term: (1 + u)^(P + 3 + degree) - 1 <= (P + 3 + degree) u + second
        order, and with P + 3 + degree <= 1031 the second-order part is below 1031^2 u^2 < 2e-10 u;
      * the long-double reference (u_ld = 2^-64 = 2^-11 u) errs by at most (P + degree) u_ld on the same |psi| |W|^T: below
        1028 * 2^-11 u < 0.51 u.
    The factor P + 4 + degree leaves one whole u for the last two items, which need 0.51 u.  Nothing here is measured."""
    a = np.abs(np.asarray(psi_ld, dtype=np.longdouble)) @ np.abs(np.asarray(W, dtype=np.longdouble)).T
    return (P + 4 + degree) * np.longdouble(U) * a


# ------------------------------------------------------------------------------------------------ the comparisons the device test makes
def same_bits(got, ref):
    """Equal in every bit pattern that matters: same shape, same values, NaN where NaN (np.array_equal with equal_nan)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return got.shape == ref.shape and bool(np.array_equal(got, ref, equal_nan=True))


def bound_fraction(got, ref_ld, bound):
    """Largest |got - ref| / bound over the entries (0 / 0 counts as 0; an error where the bound is 0 as inf; NaN as inf)."""
    got = np.asarray(got, dtype=np.longdouble)
    if got.shape != np.shape(ref_ld):
        return float('inf')
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref_ld)
    bound = np.asarray(bound, dtype=np.longdouble)
    frac = np.where(err == 0, np.longdouble(0), err / np.where(bound > 0, bound, np.longdouble(1)))
    frac = np.where((bound == 0) & (err != 0), np.longdouble(np.inf), frac)
    frac = np.where(np.isnan(err), np.longdouble(np.inf), frac)
    return float(frac.max())


def inside(got, ref_ld, bound):
    return bound_fraction(got, ref_ld, bound) <= 1.0
