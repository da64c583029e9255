"""CPU: sgusto_ssm_rate_rows_fit -- the rule by which the SSM GuSTO plan takes input-rate rows dU into its one-wave QP in the space of
the inputs (csrc/locp_dense_u.h: qdu::limit) -- on its boundaries.  Host arithmetic only: no GPU is touched."""
import ctypes as C
import itertools

import pytest


def fit(N, n_x, n_u, n_z, nU, nX, nXf, ndU):
    from sofacontrol_amd import _lib
    fits = C.c_int(-1)
    _lib.check(_lib.lib().sgusto_ssm_rate_rows_fit(C.c_int(N), C.c_int(n_x), C.c_int(n_u), C.c_int(n_z), C.c_int(nU), C.c_int(nX),
                                                   C.c_int(nXf), C.c_int(ndU), C.byref(fits)), 'sgusto_ssm_rate_rows_fit')
    assert fits.value in (0, 1)
    return bool(fits.value)


def applies_without_rate_rows(N, n, m, nz, nU, nX, nXf):
    """qdu::applies as it stood before rate rows existed."""
    stage = N * n * (n + m + 1) + nz * n + nX * n
    return (N * m <= 16 and N * nz <= 48 and N * (nU + nX) <= 64 and nXf == 0 and n <= 64 and N <= 8 and nz <= 16 and m <= 16 and
            stage <= 6144)


def test_hardware_shape_fits_with_forty_rows():
    # n_x = 6 + 6 carried outputs, n_u = 4, N = 3: 3 * 8 input rows + 2 * 8 rate rows
    assert fit(3, 12, 4, 6, 8, 0, 0, 8)
    assert 3 * 8 + 2 * 8 == 40


def test_row_budget_of_sixty_four():
    assert fit(4, 12, 4, 6, 8, 2, 0, 8)            # 4 * (8 + 2) + 3 * 8 = 64
    assert not fit(4, 12, 4, 6, 8, 3, 0, 8)        # 4 * (8 + 3) + 3 * 8 = 68
    assert fit(4, 12, 4, 6, 8, 3, 0, 6)            # 44 + 18 = 62
    assert fit(3, 12, 4, 6, 0, 0, 0, 32) and not fit(3, 12, 4, 6, 0, 0, 0, 33)      # rate rows alone: 2 * 32 = 64
    assert fit(1, 12, 4, 6, 8, 0, 0, 1000)         # N = 1: no stage pair, no rate row


def test_input_tile_and_terminal_rows():
    assert not fit(5, 12, 4, 6, 8, 0, 0, 8)        # N n_u = 20 > 16
    assert not fit(5, 12, 4, 6, 8, 0, 0, 0)
    assert fit(4, 12, 4, 6, 8, 0, 0, 8)            # N n_u = 16
    for nXf in (1, 2):
        assert not fit(3, 12, 4, 6, 8, 0, nXf, 8)
        assert not fit(3, 12, 4, 6, 8, 0, nXf, 0)


def test_without_rate_rows_the_rule_is_the_old_one():
    shapes = itertools.product((1, 3, 4, 5, 8, 9), (6, 12, 40, 64, 65), (2, 4, 5, 16), (3, 6, 16, 17), (0, 8, 16, 17), (0, 2, 9), (0, 1))
    n = 0
    for N, nx, m, nz, nU, nX, nXf in shapes:
        assert fit(N, nx, m, nz, nU, nX, nXf, 0) == applies_without_rate_rows(N, nx, m, nz, nU, nX, nXf), (N, nx, m, nz, nU, nX, nXf)
        n += 1
    assert n > 1000


def test_bad_arguments_are_refused():
    from sofacontrol_amd import _lib
    assert _lib.lib().sgusto_ssm_rate_rows_fit(C.c_int(3), C.c_int(12), C.c_int(4), C.c_int(6), C.c_int(8), C.c_int(0), C.c_int(0),
                                               C.c_int(8), None) != 0
    assert b'sgusto_ssm_rate_rows_fit' in _lib.lib().srh_last_error()
    fits = C.c_int(0)
    assert _lib.lib().sgusto_ssm_rate_rows_fit(C.c_int(3), C.c_int(12), C.c_int(4), C.c_int(6), C.c_int(8), C.c_int(0), C.c_int(0),
                                               C.c_int(-1), C.byref(fits)) != 0
