"""Dump what spoly_project answers on every family of tests/poly_cases.py, and compare two dumps bit for bit.

  SRH_LIB_PATH=<build A>/libsofacontrol_hip.so python tools/poly_dump.py --out dumps/poly_a.npz
  python tools/poly_dump.py --out dumps/poly_b.npz                    (the in-tree library)
  python tools/poly_dump.py --compare dumps/poly_a.npz dumps/poly_b.npz

A dump holds, per case, the points of the whole batch in one call and of every point alone, and per failure of pc.FAILURES the return
code and the message.  The comparison prints one line per family and ends with RESULT: identical / DIFFERENT (exit status 1).
profiles/poly_wave_unit_bits.log is such a comparison: the stand-alone kernel before and after its body moved into csrc/poly_dev.h."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def spoly(A, b, X):
    from sofacontrol_amd import _lib
    lib = _lib.lib()
    A, b, X = (np.ascontiguousarray(v, dtype=np.float64) for v in (A, b, X))
    out = np.full(X.shape, -7.25e77)
    rc = lib.spoly_project(_lib.dptr(A), _lib.dptr(b), C.c_int(A.shape[0]), C.c_int(X.shape[1]), _lib.dptr(X), C.c_int64(X.shape[0]),
                           _lib.dptr(out))
    return rc, (lib.srh_last_error().decode(errors='replace') if rc != 0 else ''), out


def dump(path):
    import poly_cases as pc
    from sofacontrol_amd import _lib
    rec = {'library': np.array(os.path.relpath(_lib.LIB_PATH, ROOT))}
    for c in pc.cases():
        rc, msg, out = spoly(c.A, c.b, c.X)
        assert rc == 0, (c.key, msg)
        rec[c.key + '#batch'] = out
        rec[c.key + '#alone'] = np.stack([spoly(c.A, c.b, x[None])[2][0] for x in c.X])
    for name in pc.FAILURES:
        A, b, X, _, _ = pc.failure(name)
        rc, msg, _ = spoly(A, b, X)
        rec['failure/' + name + '#rc'] = np.array(rc)
        rec['failure/' + name + '#message'] = np.array(msg)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **rec)
    print('poly_dump: %d records from %s -> %s' % (len(rec) - 1, rec['library'], path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    print('poly_dump --compare')
    print('A: %s (library %s)' % (pa, a['library']))
    print('B: %s (library %s)' % (pb, b['library']))
    ka, kb = [k for k in a.files if k != 'library'], [k for k in b.files if k != 'library']
    print('records: %d / %d, same names in the same order: %s' % (len(ka), len(kb), ka == kb))
    same = ka == kb
    fam = {}
    for k in ka:
        if k not in b.files:
            continue
        va, vb = a[k], b[k]
        eq = va.shape == vb.shape and va.dtype == vb.dtype and va.tobytes() == vb.tobytes()
        f = fam.setdefault(k.split('/')[0], [0, 0, 0, True])
        f[0] += 1; f[1] += va.nbytes; f[2] += int(va.size if va.dtype == np.float64 else 0); f[3] = f[3] and eq
        if not eq:
            print('  DIFFERENT: %s' % k)
    for name, (n, nbytes, doubles, eq) in fam.items():
        print('%-12s %4d records, %8d bytes, %6d doubles, %s' % (name, n, nbytes, doubles, 'identical' if eq else 'DIFFERENT'))
        same = same and eq
    for k in ka:
        if k.endswith('#message') and k in b.files:
            print('  %-32s %s: %s' % (k[:-8], 'same' if str(a[k]) == str(b[k]) else 'DIFFERENT', a[k]))
    print('RESULT: %s' % ('identical, bit for bit' if same else 'DIFFERENT'))
    return 0 if same else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out or os.path.join(ROOT, 'dumps', 'poly.npz'))
