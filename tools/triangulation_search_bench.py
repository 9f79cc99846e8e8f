#!/usr/bin/env python
"""The SearchForTriangulation loop of one LocalMapping::CreateNewMapPoints, two ways in the same run ->
profiles/triangulation_search_bench.txt.

Job (tests/triangulation_batch_util.bench_job): 1 current keyframe against 20 neighbours, 2 000 keypoints each, FeatureVectors
of about 100 nodes of uneven size, about half of every keyframe's keypoints flagged as having a MapPoint.  Timed through the C
ABI with arrays prepared beforehand (ctypes), host clock, median and 90th percentile of `--reps` rounds after a warm-up:
  single calls   20 x orbfe_search_for_triangulation on host arrays, check_orientation = 0
  batch call     1 x orbfe_search_for_triangulation_frames_batch on resident frames (built beforehand, as the keyframes of a
                 running map are), and the same followed by the host-side orbfe_triangulation_finish calls
The rows of the two routes are compared before anything is timed.  Bytes: what each route puts into its upload image / reads
back, from the array sizes.  No threshold: the numbers are the result."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def stats(ms):
    s = np.sort(ms)
    return float(s[len(s) // 2]), float(s[min(len(s) - 1, int(np.ceil(0.9 * len(s))) - 1)])


def common(fv1, fv2):
    """number of vocabulary nodes with features on both sides"""
    live = lambda fv: set(int(i) for i, a, b in zip(fv[0], fv[1][:-1], fv[1][1:]) if b > a)
    return len(live(fv1) & live(fv2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--neighbours', type=int, default=20)
    ap.add_argument('--keypoints', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'triangulation_search_bench.txt'))
    args = ap.parse_args()
    from os1_amd import api
    import triangulation_batch_util as T
    assert api.device_count() >= 1, 'no GPU visible'
    L = api.load_library()
    job = T.bench_job(args.neighbours, args.keypoints)
    kf1, nbs = job['kf1'], job['nb']
    n1 = len(kf1['kps'])
    m = api.Matcher(0)
    f1 = api.Frame.from_host(m, kf1['kps'], kf1['desc'], T.BOUNDS)
    f2 = [api.Frame.from_host(m, nb['kps'], nb['desc'], T.BOUNDS) for nb in nbs]
    m.synchronize()
    fv1 = [np.ascontiguousarray(a, np.uint32) for a in kf1['fv']]
    fv2 = [[np.ascontiguousarray(a, np.uint32) for a in nb['fv']] for nb in nbs]
    F = [np.ascontiguousarray(nb['F12'], np.float32) for nb in nbs]
    pairs = np.zeros((len(nbs), n1, 2), np.int32)
    nm = np.zeros(len(nbs), np.int32)
    nmp = [C.cast(nm.ctypes.data + 4 * j, C.POINTER(C.c_int)) for j in range(len(nbs))]

    def single():
        for j, nb in enumerate(nbs):
            rc = L.orbfe_search_for_triangulation(m.h, vp(kf1['kps']), vp(kf1['desc']), vp(kf1['has']), n1, vp(fv1[0]), vp(fv1[1]), vp(fv1[2]), len(fv1[0]),
                                                  vp(nb['kps']), vp(nb['desc']), vp(nb['has']), len(nb['kps']), vp(fv2[j][0]), vp(fv2[j][1]), vp(fv2[j][2]),
                                                  len(fv2[j][0]), vp(F[j]), nb['ex'], nb['ey'], vp(nb['sf']), vp(nb['s2']), len(nb['sf']), 0, vp(pairs[j]),
                                                  nmp[j])
            assert rc == 0, L.orbfe_last_error()

    arr, _keep = m._tri_neighbours([T.neighbour_arg(f, nb) for f, nb in zip(f2, nbs)])
    raw = np.full((len(nbs), n1), -1, np.int32)

    def batch():
        rc = L.orbfe_search_for_triangulation_frames_batch(m.h, f1.h, vp(kf1['has']), vp(fv1[0]), vp(fv1[1]), vp(fv1[2]), len(fv1[0]), len(nbs),
                                                           C.cast(arr, C.c_void_p), vp(raw))
        assert rc == 0, L.orbfe_last_error()

    out2 = np.zeros((n1, 2), np.int32)
    n2c = C.c_int(0)

    def batch_finish():
        batch()
        for j, nb in enumerate(nbs):
            rc = L.orbfe_triangulation_finish(vp(raw[j]), n1, vp(kf1['has']), vp(kf1['has']), 1, vp(kf1['kps']), vp(nb['kps']), len(nb['kps']), vp(out2), C.byref(n2c))
            assert rc == 0

    single()                                                   # warm-up: buffers grow here; and the comparison
    batch()
    total = 0
    for j in range(len(nbs)):
        assert T.raw_from_pairs(pairs[j][:nm[j]], n1).tobytes() == raw[j].tobytes(), 'neighbour %d: the two routes differ' % j
        total += int(nm[j])
    res = {}
    for name, fn in (('single calls', single), ('batch call', batch), ('batch call + finish', batch_finish)):
        fn()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = stats(ms)
    nf1 = int(fv1[1][-1])
    up_single = sum((28 + 32 + 1) * (n1 + len(nb['kps'])) + 4 * (nf1 + int(fv[1][-1])) + 24 * common(fv1, fv) for nb, fv in zip(nbs, fv2))
    recs = sum(common(fv1, fv) for fv in fv2)
    up_batch = 208 * len(nbs) + 24 * recs + n1 + 4 * nf1 + sum(len(nb['kps']) + 4 * int(fv[1][-1]) for nb, fv in zip(nbs, fv2))
    down = 4 * n1 * len(nbs)
    lines = ['# tools/triangulation_search_bench.py: the SearchForTriangulation loop of one CreateNewMapPoints -- 1 keyframe x %d neighbours, %d keypoints'
             % (len(nbs), n1), '# each, %d (neighbour, common node) records, %d raw matches in all -- as %d orbfe_search_for_triangulation calls on host arrays and as ONE'
             % (recs, total, len(nbs)), '# orbfe_search_for_triangulation_frames_batch call on resident frames; host clock, %d rounds after a warm-up, ms.  Bytes: the upload image of' % args.reps,
             '# each route (the single calls read theirs in place from page-locked memory when every node fits LDS) and the rows read back.',
             'route                       median_ms    p90_ms   submissions   KB_up   KB_down']
    fmt = '%-26s %10.3f %9.3f %13d %7.1f %9.1f'
    lines.append(fmt % ('single calls', res['single calls'][0], res['single calls'][1], len(nbs), up_single / 1e3, down / 1e3))
    lines.append(fmt % ('batch call', res['batch call'][0], res['batch call'][1], 1, up_batch / 1e3, down / 1e3))
    lines.append(fmt % ('batch call + %d x finish' % len(nbs), res['batch call + finish'][0], res['batch call + finish'][1], 1, up_batch / 1e3, down / 1e3))
    lines.append('# single / batch (medians): %.2f; with the host-side finish of every row (orientation check on): %.2f'
                 % (res['single calls'][0] / res['batch call'][0], res['single calls'][0] / res['batch call + finish'][0]))
    print('\n'.join(lines), flush=True)
    for f in [f1] + f2:
        f.close()
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
