"""Bit-level dump of the filter kernels (csrc/observer.hip) for comparing two builds of the library (SRH_LIB_PATH selects one).

Runs the 12-step schedules of tests/ekf_cases.py through the C ABI: every entry of SPECS (all four kernel paths at both scalings,
and the explicit (A_d, B_d, d_d) cases) and NO_MFMA_SPECS under SRH_EKF_NO_MFMA=1.  Each case steps a single handle (sekf_step) and,
on the table form, a batch of 3 (sekf_batch_step; member b gets the case's inputs shifted by b), and records x, Sigma and the status
(the single handle's return code, the batch's status words) after every call.

    python tools/ekf_dump.py --out dumps/new         writes <out>.bin (the records, raw) and <out>.json (their index)
    python tools/ekf_dump.py --compare A B --log profiles/x.log    compares two dumps record by record, byte for byte; exit 1 on a difference

One dump per process.  Needs the GPU (not for --compare)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'soft-robot-control_amd'), os.path.join(ROOT, 'tests')]

BATCH = 3


def dump_case(s, label, records):
    import ekf_cases as ec
    from sofacontrol_amd import _lib
    lib, f64, dptr = _lib.lib(), _lib.f64, _lib.dptr
    c = ec.case(s)
    n, m, ny = c['n'], c['m'], c['ny']
    tp, _ = ec.product_filter(c)
    mh = tp.handle_for(ec.DT)
    Cm, yr, S0, W, V = (f64(c[k]) for k in ('C', 'y_ref', 'Sigma0', 'W', 'V'))
    create_args = (mh, dptr(Cm), dptr(yr), C.c_int(ny), dptr(S0), dptr(W), dptr(V))

    def record(kind, call, x, Sg, status):
        for name, a in (('x', x), ('Sigma', Sg), ('status', np.asarray(status, dtype=np.int32))):
            records.append(('%s/%s/call%02d/%s' % (label, kind, call, name), np.ascontiguousarray(a).tobytes()))

    ops = ec.operations(c)
    h = C.c_void_p()
    _lib.check(lib.sekf_create(C.byref(h), *create_args), 'sekf_create')
    path = C.c_int()
    _lib.check(lib.sekf_handle_plan(h, C.byref(path), None, None), 'sekf_handle_plan')
    x, Sg, xo, call = np.empty(n), np.empty((n, n)), np.empty(n), 0
    for op in ops:
        if op[0] == 'reset':
            _lib.check(lib.sekf_set_state(h, dptr(f64(op[2])), None), 'sekf_set_state')
            continue
        u, y = (None if v is None else f64(v) for v in op[2:4])
        A, B, d = (None, None, None) if op[4] is None else (f64(a) for a in op[4])
        rc = lib.sekf_step(h, dptr(u) if u is not None else None, dptr(y) if y is not None else None, dptr(A) if A is not None else None,
                           dptr(B) if B is not None else None, dptr(d) if d is not None else None, dptr(xo))
        _lib.check(lib.sekf_get_state(h, dptr(x), dptr(Sg)), 'sekf_get_state')
        record('single', call, np.concatenate((x, xo)), Sg, [rc])
        call += 1
    lib.sekf_destroy(h)
    if c['form'] != 'table':
        return path.value
    hb = C.c_void_p()
    _lib.check(lib.sekf_batch_create(C.byref(hb), *create_args, C.c_int64(BATCH)), 'sekf_batch_create')
    shift = np.arange(BATCH)[:, None]
    xb, Sb, xob, st, call = np.empty((BATCH, n)), np.empty((BATCH, n, n)), np.empty((BATCH, n)), np.empty(BATCH, dtype=np.int32), 0
    for op in ops:
        if op[0] == 'reset':
            _lib.check(lib.sekf_batch_set_state(hb, dptr(f64(op[2][None] + 1e-4 * shift)), None), 'sekf_batch_set_state')
            continue
        u = None if op[2] is None else f64(op[2][None] + 1.0 * shift)
        y = None if op[3] is None else f64(op[3][None] + 0.01 * shift)
        rc = lib.sekf_batch_step(hb, dptr(u) if u is not None else None, dptr(y) if y is not None else None, dptr(xob))
        _lib.check(lib.sekf_batch_get_state(hb, dptr(xb), dptr(Sb), _lib.iptr(st)), 'sekf_batch_get_state')
        record('batch%d' % BATCH, call, np.concatenate((xb, xob)), Sb, [rc] + st.tolist())
        call += 1
    lib.sekf_batch_destroy(hb)
    return path.value


def dump(out):
    import ekf_cases as ec
    from sofacontrol_amd import _lib
    assert _lib.device_count() >= 1, 'no GPU visible'
    _lib.set_device(0)
    records, paths = [], {}
    os.environ.pop('SRH_EKF_NO_MFMA', None)
    for s in ec.SPECS:
        paths[ec.spec_id(s)] = dump_case(s, ec.spec_id(s), records)
    os.environ['SRH_EKF_NO_MFMA'] = '1'              # read when a filter is created
    for s in ec.NO_MFMA_SPECS:
        paths['no_mfma/' + ec.spec_id(s)] = dump_case(s, 'no_mfma/' + ec.spec_id(s), records)
    os.environ.pop('SRH_EKF_NO_MFMA')
    index, off = [], 0
    with open(out + '.bin', 'wb') as f:
        for name, b in records:
            f.write(b)
            index.append(dict(name=name, offset=off, bytes=len(b), sha256=hashlib.sha256(b).hexdigest()))
            off += len(b)
    with open(out + '.json', 'w') as f:
        json.dump(dict(library=os.path.relpath(_lib.LIB_PATH, ROOT), kernel_path_of_case=paths, records=index), f, indent=0)
    print('ekf_dump: %d cases, %d records, %d bytes -> %s.bin (library %s)' % (len(paths), len(index), off, out, os.path.relpath(_lib.LIB_PATH, ROOT)))


def compare(a, b, log):
    ja, jb = (json.load(open(p + '.json')) for p in (a, b))
    ba, bb = (open(p + '.bin', 'rb').read() for p in (a, b))
    lines = ['ekf_dump --compare', 'A: %s (library %s)' % (a, ja['library']), 'B: %s (library %s)' % (b, jb['library'])]
    same_index = [r['name'] for r in ja['records']] == [r['name'] for r in jb['records']]
    lines.append('records: %d / %d, same names in the same order: %s' % (len(ja['records']), len(jb['records']), same_index))
    lines.append('kernel path of every case equal: %s' % (ja['kernel_path_of_case'] == jb['kernel_path_of_case']))
    per_case, differing = {}, []
    if same_index:
        for ra, rb in zip(ja['records'], jb['records']):
            equal = ba[ra['offset']:ra['offset'] + ra['bytes']] == bb[rb['offset']:rb['offset'] + rb['bytes']]
            case = ra['name'].rsplit('/', 3)[0]
            t = per_case.setdefault(case, [0, 0])
            t[0] += 1
            t[1] += 0 if equal else 1
            if not equal:
                differing.append(ra['name'])
    for case, (total, bad) in per_case.items():
        lines.append('%-44s path %d: %3d records, %s' % (case, ja['kernel_path_of_case'][case], total,
                                                        'identical' if bad == 0 else '%d DIFFER' % bad))
    ok = same_index and not differing and ba == bb and ja['kernel_path_of_case'] == jb['kernel_path_of_case']
    lines += ['first differing records: %s' % differing[:8]] if differing else []
    lines.append('whole files (%d / %d bytes) identical: %s' % (len(ba), len(bb), ba == bb))
    lines.append('RESULT: %s' % ('identical, byte for byte' if ok else 'DIFFERENT'))
    print('\n'.join(lines))
    if log:
        with open(log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--log')
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.log))
    if not args.out:
        ap.error('need --out or --compare')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dump(args.out)


if __name__ == '__main__':
    main()
