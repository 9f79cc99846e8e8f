#!/usr/bin/env python
"""Rebuilding a loaded map's bag-of-words side (KeyFrame::ComputeBoW and KeyFrameDatabase::add for every keyframe, the loops of
Osmap::rebuild), per keyframe against in bulk, in the same run -> profiles/map_load_bench.txt.

Map: 500 and 2 000 keyframes of 2 000 synthetic descriptors each (vocabulary nodes' descriptors with 5 % of the bits flipped,
every seventh pure noise), a k = 10, L = 5 synthetic vocabulary, levelsup 4.  Timed on a host clock around calls that end in a
device synchronise, the median of `--reps` rounds after one warm-up round:
  per keyframe   orbfe_bow_transform + orbfe_kfdb_add for each keyframe (2 n submissions and waits)
  bulk           one orbfe_bow_transform_batch + one orbfe_kfdb_add_batch
Both routes go through the C ABI with arrays prepared beforehand (ctypes), so the Python binding's marshalling is in neither.
The two routes' BowVectors are compared before anything is timed."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_DESC = 2000


def descriptors(rng, image, n):
    rec = np.frombuffer(image, np.uint8, offset=4).reshape(-1, 45)
    pick = rec[rng.integers(0, len(rec), n), 5:37].copy()
    bits = np.unpackbits(pick, axis=1)
    out = np.packbits(bits ^ (rng.random(bits.shape) < 0.05), axis=1)
    out[::7] = rng.integers(0, 256, (len(out[::7]), 32), dtype=np.uint8)
    return np.ascontiguousarray(out)


class Outputs:
    """per-keyframe output arrays of both calls, and the pointer tables of the bulk one"""

    def __init__(self, n_kf, n):
        self.ids = np.zeros((n_kf, n), np.uint32)
        self.vals = np.zeros((n_kf, n), np.float64)
        self.fvn = np.zeros((n_kf, n), np.uint32)
        self.fvo = np.zeros((n_kf, n + 1), np.uint32)
        self.fvf = np.zeros((n_kf, n), np.uint32)
        self.nw = np.zeros(n_kf, np.int32)
        self.nn = np.zeros(n_kf, np.int32)
        self.tab = np.array([[a[k].ctypes.data for k in range(n_kf)] for a in (self.ids, self.vals, self.fvn, self.fvo, self.fvf)], np.uint64)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def run(api, image, n_kf, reps, rng):
    L = api.load_library()
    voc = api.Vocabulary(image)
    n_words = voc.info()['n_words']
    desc = [descriptors(rng, image, N_DESC) for _ in range(n_kf)]
    dptr = np.array([d.ctypes.data for d in desc], np.uint64)
    n = np.full(n_kf, N_DESC, np.int32)
    keys = np.arange(1, n_kf + 1, dtype=np.uint64)
    a, b = Outputs(n_kf, N_DESC), Outputs(n_kf, N_DESC)

    def per_keyframe(db):
        for k in range(n_kf):
            rc = L.orbfe_bow_transform(voc.h, vp(desc[k]), N_DESC, 0, 4, vp(a.ids[k]), vp(a.vals[k]), C.byref(C.c_int.from_buffer(a.nw, 4 * k)),
                                       vp(a.fvn[k]), vp(a.fvo[k]), vp(a.fvf[k]), C.byref(C.c_int.from_buffer(a.nn, 4 * k)), None, None)
            rc = rc or L.orbfe_kfdb_add(db.h, int(keys[k]), vp(a.ids[k]), vp(a.vals[k]), int(a.nw[k]))
            assert rc == 0, L.orbfe_last_error()

    def bulk(db):
        rc = L.orbfe_bow_transform_batch(voc.h, 4, n_kf, vp(dptr), vp(n), vp(n), vp(b.tab[0]), vp(b.tab[1]), vp(b.nw), vp(b.tab[2]), vp(b.tab[3]),
                                         vp(b.tab[4]), vp(b.nn), None, None)
        rc = rc or L.orbfe_kfdb_add_batch(db.h, n_kf, vp(keys), vp(b.tab[0]), vp(b.tab[1]), vp(b.nw))
        assert rc == 0, L.orbfe_last_error()

    times = {}
    for name, fn in (('per keyframe', per_keyframe), ('bulk', bulk)):
        t = []
        for r in range(reps + 1):
            db = api.KeyFrameDatabase(n_words, 0, n_kf, n_kf * N_DESC)
            t0 = time.perf_counter()
            fn(db)
            t.append((time.perf_counter() - t0) * 1e3)
            if r == 0:
                size = db.size()
            db.close()
        times[name] = (float(np.median(t[1:])), min(t[1:]), max(t[1:]), size)
    assert a.nw.tolist() == b.nw.tolist() and a.nn.tolist() == b.nn.tolist()
    for k in range(n_kf):
        w = int(a.nw[k])
        assert a.ids[k, :w].tobytes() == b.ids[k, :w].tobytes() and a.vals[k, :w].tobytes() == b.vals[k, :w].tobytes(), k
    assert times['per keyframe'][3] == times['bulk'][3]
    voc.close()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keyframes', type=int, nargs='+', default=[500, 2000])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'map_load_bench.txt'))
    args = ap.parse_args()
    from os1_amd import api
    from os1_amd.synth import synth_vocabulary
    assert api.device_count() >= 1, 'no GPU visible'
    image = synth_vocabulary(5, 10, 5)
    lines = ['# tools/map_load_bench.py: KeyFrame::ComputeBoW + KeyFrameDatabase::add for every keyframe of a loaded map (%d descriptors each,'
             % N_DESC, '# k = 10, L = 5 vocabulary, levelsup 4), host clock, median of %d rounds (min .. max), ms' % args.reps,
             '# per keyframe: orbfe_bow_transform + orbfe_kfdb_add per keyframe; bulk: one orbfe_bow_transform_batch + one orbfe_kfdb_add_batch',
             'keyframes  per_keyframe_ms               bulk_ms                       ratio  entries']
    for n_kf in args.keyframes:
        t = run(api, image, n_kf, args.reps, np.random.default_rng(n_kf))
        p, b = t['per keyframe'], t['bulk']
        lines.append('%9d  %8.2f (%8.2f .. %8.2f)  %8.2f (%8.2f .. %8.2f)  %5.2f  %d' % (n_kf, p[0], p[1], p[2], b[0], b[1], b[2], p[0] / b[0], p[3][1]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
