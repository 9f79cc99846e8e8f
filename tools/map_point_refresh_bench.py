#!/usr/bin/env python
"""One orbfe_local_map_refresh_rows call against the route it replaces, in the same run -> profiles/map_point_refresh_bench.txt.

Scene (seeded): 30 resident keyframes of 2 000 keypoints, 2 000 MapPoints with 2-40 observations each (uniform; a keyframe
observes a MapPoint once, so a draw above the number of keyframes is clamped to it), no bad keyframe,
a table of 2 048 rows.  Both routes leave the same rows in their table (checked once, byte for byte, before anything is timed).
  new   LocalMap.refresh_rows(DESCRIPTOR | NORMAL_DEPTH) with the four host outputs: one upload of 8 bytes per observation and 16
        per MapPoint, k_refresh_map_points, one download of 24 bytes per MapPoint; the call returns after a stream synchronise
  enq   the same call without host outputs (returns once enqueued) followed by Matcher.synchronize()
  old   the parent's entry points: a host gather of the observed descriptor rows (numpy fancy indexing out of the keyframes'
        host arrays), Matcher.distinctive_descriptors (orbfe_distinctive_descriptors: upload of 32 bytes per observation, k_distinctive,
        download of 4 bytes per MapPoint), the single-core C++ restatement of UpdateNormalAndDepth per MapPoint
        (tests/cpp/map_point_refresh_ref.cpp mpr_refresh_rows with what = NORMAL_DEPTH on a host copy of the table, built -O3),
        LocalMap.set_rows of descriptor, normal, min and max, Matcher.synchronize()
Method: a host clock (time.perf_counter) around work that ends in a device synchronise; `--warmup` untimed rounds, then `--reps`
rounds in which the routes ALTERNATE (new, enq, old, new, ...), so that drift of the shared host hits all alike; median, min
and max per route.  The Python binding is inside every figure.  PCIe bytes are counted from the shapes."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
f32 = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mps', type=int, default=2000)
    ap.add_argument('--kfs', type=int, default=30)
    ap.add_argument('--kps', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import subprocess
    import map_point_refresh_util as U
    from os1_amd import api
    assert api.device_count() >= 1, 'needs a GPU'
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, 'mpr_o3.so')
    subprocess.check_call(['g++', '-std=c++17', '-O3', '-ffp-contract=off', '-fPIC', '-shared', U.REF_SRC, '-o', so])
    import ctypes as C
    ref = U.build_ref(tmp)                                # the tests' build: what "equal" compares with
    fast = C.CDLL(so)                                     # the -O3 build: what is timed
    fast.mpr_refresh_rows.argtypes = ref.mpr_refresh_rows.argtypes

    rng = np.random.default_rng(a.seed)
    kfs = [U.KF(rng, a.kps) for _ in range(a.kfs)]
    cap = 1 << int(np.ceil(np.log2(a.mps)))
    table = np.zeros((cap, 64), np.uint8)
    tf = table.view(f32).reshape(cap, 16)
    tf[:, 0:3] = np.stack([rng.uniform(-4, 4, cap), rng.uniform(-3, 3, cap), rng.uniform(3, 9, cap)], 1).astype(f32)
    obs, refs = [], []
    for _ in range(a.mps):
        n = int(rng.integers(2, 41))
        slots = np.sort(rng.choice(a.kfs, min(n, a.kfs), replace=False))
        o = [(int(s), int(rng.integers(0, a.kps)), False) for s in slots]
        obs.append(o)
        refs.append((o[0][0], o[0][1]))
    b = U.Batch(rng.permutation(cap)[:a.mps], obs, refs)
    total = int(b.offs[-1])
    all_rows = np.arange(cap, dtype=np.int32)

    m = api.Matcher(0)
    bounds = (0.0, 640.0, 0.0, 480.0)
    frames = [api.Frame.from_host(m, k.kps, k.desc, bounds) for k in kfs]
    Ow = np.stack([k.Ow for k in kfs]).astype(f32)
    new_map, old_map = api.LocalMap(m, cap), api.LocalMap(m, cap)
    for lm in (new_map, old_map):
        lm.set_rows(all_rows, pos=tf[:, 0:3])
    host_table = table.copy()
    dp = (C.c_void_p * len(kfs))(*[k.desc.ctypes.data for k in kfs])
    op = (C.c_void_p * len(kfs))(*[k.oct.ctypes.data for k in kfs])
    seg = b.offs

    def new(outputs=True):
        r = new_map.refresh_rows(3, frames, Ow, b.rows, b.offs, b.kf, b.kp, b.fl, b.ref_kf, b.ref_kp, scale_factors=U.SF, outputs=outputs)
        if not outputs:
            m.synchronize()
        return r

    def old():
        lists = [kfs_desc[b.kf[seg[p]:seg[p + 1]], b.kp[seg[p]:seg[p + 1]]] for p in range(a.mps)]      # the host gather
        best = m.distinctive_descriptors(lists)
        desc = np.stack([lists[p][best[p]] for p in range(a.mps)])
        nrm = np.zeros((a.mps, 3), f32)
        mn, mx = np.zeros(a.mps, f32), np.zeros(a.mps, f32)
        fast.mpr_refresh_rows(U._p(host_table), 2, len(kfs), C.cast(dp, C.c_void_p), C.cast(op, C.c_void_p), U._p(Ow), U._p(U.SF), U.NLEVELS,
                              a.mps, U._p(b.rows), U._p(b.offs), U._p(b.kf), U._p(b.kp), U._p(b.fl), U._p(b.ref_kf), U._p(b.ref_kp), None,
                              U._p(nrm), U._p(mn), U._p(mx))
        old_map.set_rows(b.rows, normal=nrm, min_raw=mn, max_raw=mx, desc=desc)
        m.synchronize()

    kfs_desc = np.stack([k.desc for k in kfs])          # [kf][kp][32]: what the application holds as pKF->mDescriptors
    new()
    old()
    same = new_map.download_rows(all_rows).tobytes() == old_map.download_rows(all_rows).tobytes()
    want = U.ref_refresh(ref, table, 3, kfs, b)[0]
    same = same and new_map.download_rows(all_rows).tobytes() == want.tobytes()
    routes = (('new', new), ('enq', lambda: new(False)), ('old', old))
    for _ in range(a.warmup):
        for _, fn in routes:
            fn()
    t = {k: [] for k, _ in routes}
    for _ in range(a.reps):
        for k, fn in routes:
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    up_new, down_new = 8 * total + 16 * a.mps + 4 + 28 * a.kfs, 24 * a.mps + 4
    up_old, down_old = 32 * total + 4 * (a.mps + 1) + 80 * a.mps, 4 * a.mps
    lines = ['# %d MapPoints, %d observations (2-40 each), %d keyframes x %d keypoints; seed %d' % (a.mps, total, a.kfs, a.kps, a.seed),
             '# host clock around calls that end in a stream synchronise; %d warm-up rounds, %d timed rounds, routes alternating' % (a.warmup, a.reps),
             '# rows of both tables equal each other and the CPU restatement: %s' % ('yes' if same else 'NO'),
             '# route | median_ms (min..max) | PCIe bytes up | PCIe bytes down']
    for k, up, down in (('new', up_new, down_new), ('enq', up_new, 0), ('old', up_old, down_old)):
        lines.append('%7s | %8.3f (%.3f..%.3f) | %10d | %8d' % (k, np.median(t[k]), np.min(t[k]), np.max(t[k]), up, down))
    text = '\n'.join(lines) + '\n'
    print(text, end='', flush=True)
    if a.out:
        open(a.out, 'w').write(text)
    for f in frames:
        f.close()
    new_map.close()
    old_map.close()
    m.close()
    assert same


if __name__ == '__main__':
    main()
