"""Expected values of the discretisation kernel's exact tests, in multiprecision arithmetic (needs mpmath; about a minute).

Usage:  python tests/golden/make_golden_discretize.py          (writes tests/golden/g24_discretize.npz)

For every case of tests/discretize_cases.fixture_cases(): `<key>/Ad`, `<key>/Bd`, `<key>/dd` (with the batch dimension), the
statement of tests/discretize_reference.mp_discretize at 60 digits rounded once to float64; for the zoh cases also `<key>/s`, the
squarings of the published rule, and `<key>/nrm`, the 1-norm of the augmented matrix.  The inputs are regenerated from their seeds and
are not stored.  The GPU box never runs this script."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import discretize_cases as dc  # noqa: E402
import discretize_reference as dr  # noqa: E402


def entries(key, method, dt, A, B, d):
    """The fixture's arrays of one case."""
    out = {}
    res = [dr.mp_discretize(A[b], B[b], d[b], dt, method) for b in range(A.shape[0])]
    for i, o in enumerate(('Ad', 'Bd', 'dd')):
        out['%s/%s' % (key, o)] = np.stack([r[i] for r in res])
    if method == 'zoh':
        Ms = [dr.augmented(A[b], B[b], d[b], dt) for b in range(A.shape[0])]
        out[key + '/s'] = np.array([dr.squarings(M) for M in Ms], dtype=np.int32)
        out[key + '/nrm'] = np.array([dr.norm1(M) for M in Ms])
    return out


def main():
    out = {}
    for c in dc.fixture_cases():
        t0 = time.time()
        out.update(entries(*c))
        print('%-24s %s  n %d m %d batch %d  %.1f s' % (c[0], c[1], c[4].shape[1], c[4].shape[2], c[3].shape[0], time.time() - t0))
    np.savez(dc.GOLDEN, **out)
    print('wrote %s: %d arrays, %d bytes' % (dc.GOLDEN, len(out), os.path.getsize(dc.GOLDEN)))


if __name__ == '__main__':
    main()
