#!/usr/bin/env python
"""The counting loop of KeyFrame::UpdateConnections for every keyframe of a map, on the host against one
orbfe_covisibility_counts call, in the same run -> profiles/covisibility_bench.txt.

Map: 500 and 2 000 keyframes of 2 000 keypoint entries each, 800 of them MapPoints on average (the rest -1), every MapPoint
observed by 2 to 12 keyframes out of the 21 around a random centre.  Timed, the median of `--reps` rounds after one warm-up:
  host loop    tests/cpp/covisibility_ref.cpp covis_ref_loop_ms: per keyframe a std::map<KeyFrame*, int>, per MapPoint a copy of
               its std::map<KeyFrame*, size_t> of observations, one core, structures built beforehand
  GPU call     one orbfe_covisibility_counts through the C ABI with arrays prepared beforehand (ctypes), on a host clock; the
               call's own split (orbfe_debug_covis_ms): argument check + staging on the host, the kernel (stream events), the rest
               (copies up and down, waits, the assembly of the output CSR)
both for the full counters and for the map load's (subj_limit[k] = k + 1).  Then one Tracking::UpdateLocalKeyFrames-sized call:
1 subject (a Frame, nobody excluded) of 2 000 entries whose MapPoints lie in the 2 000-keyframe map, with only those MapPoints'
observations sent.  The two routes' outputs are compared before anything is timed.  No threshold: the numbers are the result."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ENTRIES = 2000
MP_PER_KF = 800
WINDOW = 10


def synth_map(n_kf, rng):
    """(obs_offsets, obs_kf, subj_self, subj_offsets, subj_mp): subjects are the keyframes in slot order."""
    n_mp = n_kf * MP_PER_KF // 7
    centre = rng.integers(0, n_kf, n_mp)
    want = rng.integers(2, 13, n_mp)
    slots = centre[:, None] + np.arange(-WINDOW, WINDOW + 1)[None, :]
    keys = rng.random(slots.shape)
    keys[(slots < 0) | (slots >= n_kf)] = 2.0                    # outside the map: never among the smallest
    order = np.argsort(keys, axis=1)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(slots.shape[1])[None, :].repeat(n_mp, 0), axis=1)
    take = (rank < want[:, None]) & (keys < 2.0)
    mp_of, col = np.nonzero(take)                                # row-major: MapPoint by MapPoint, slots ascending
    obs_kf = slots[mp_of, col].astype(np.int32)
    obs_offsets = np.zeros(n_mp + 1, np.int32)
    obs_offsets[1:] = np.cumsum(take.sum(1))
    by_kf = np.argsort(obs_kf, kind='stable')
    per_kf = np.bincount(obs_kf, minlength=n_kf)
    assert per_kf.max() <= ENTRIES, per_kf.max()
    subj_mp = np.full((n_kf, ENTRIES), -1, np.int32)
    start = np.concatenate([[0], np.cumsum(per_kf)])
    pos = np.arange(len(obs_kf)) - start[obs_kf[by_kf]]
    subj_mp[obs_kf[by_kf], pos] = mp_of[by_kf]
    subj_offsets = (np.arange(n_kf + 1, dtype=np.int64) * ENTRIES).astype(np.int32)
    return obs_offsets, obs_kf, np.arange(n_kf, dtype=np.int32), subj_offsets, np.ascontiguousarray(subj_mp.reshape(-1))


def frame_case(n_kf, obs_offsets, obs_kf, rng):
    """one Frame of ENTRIES entries: MapPoints picked among those of a stretch of keyframes, their observations only"""
    far = np.abs(obs_kf[obs_offsets[:-1]].astype(np.int64) - n_kf // 2)          # by the MapPoint's first observer
    pick = np.sort(rng.choice(np.argsort(far, kind='stable')[:2 * ENTRIES], ENTRIES, replace=False))
    counts = (obs_offsets[pick + 1] - obs_offsets[pick]).astype(np.int64)
    offs = np.zeros(ENTRIES + 1, np.int32)
    offs[1:] = np.cumsum(counts)
    kf = np.concatenate([obs_kf[obs_offsets[p]:obs_offsets[p + 1]] for p in pick]).astype(np.int32)
    return offs, kf, np.array([-1], np.int32), np.array([0, ENTRIES], np.int32), np.arange(ENTRIES, dtype=np.int32)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def measure(api, U, ref, m, n_kf, arrays, limit, reps):
    """-> dict of times (ms) and sizes for one case"""
    oo, ok, ss, so, sm = arrays
    L = api.load_library()
    n_mp, n_subj = len(oo) - 1, len(ss)
    cap = api.covisibility_bound(n_kf, oo, so, sm, limit)
    offs = np.zeros(n_subj + 1, np.int32)
    kf, cnt = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
    need = C.c_int(0)

    def call():
        rc = L.orbfe_covisibility_counts(m.h, n_kf, n_mp, vp(oo), vp(ok), n_subj, vp(ss), vp(limit), vp(so), vp(sm), vp(offs), vp(kf), vp(cnt), cap,
                                         C.byref(need))
        assert rc == 0, L.orbfe_last_error()

    call()                                                        # warm-up: buffers grow here; and the comparison
    c = U.Case.__new__(U.Case)
    c.n_kf, c.obs_offsets, c.obs_kf, c.subj_self, c.subj_offsets, c.subj_mp, c.subj_limit = n_kf, oo, ok, ss, so, sm, limit
    rc, want_need = U.ref_counts(ref, c, cap=0)
    assert want_need == need.value, (want_need, need.value)
    if n_subj * n_kf <= 4000 * 2000:
        w = U.ref_counts(ref, c)
        assert np.array_equal(w[0], offs) and np.array_equal(w[1], kf[:need.value]) and np.array_equal(w[2], cnt[:need.value])
    wall, split = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        split.append(m.covis_ms())
    i = int(np.argsort(wall)[len(wall) // 2])
    chk = C.c_longlong(0)
    host = ref.covis_ref_loop_ms(n_kf, n_mp, vp(oo), vp(ok), n_subj, vp(ss), vp(limit), vp(so), vp(sm), reps, C.byref(chk))
    assert host >= 0 and chk.value == int(cnt[:need.value].sum())
    return dict(host=host, gpu=wall[i], gpu_min=min(wall), gpu_max=max(wall), staging=split[i][0], kernel=split[i][1],
                rest=split[i][2] - split[i][0] - split[i][1], entries=need.value, obs=int(oo[-1]), bytes_up=4 * (len(oo) + len(ok) + 2 * n_subj + len(so) + len(sm)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keyframes', type=int, nargs='+', default=[500, 2000])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'covisibility_bench.txt'))
    args = ap.parse_args()
    import tempfile
    from os1_amd import api
    import covisibility_util as U
    assert api.device_count() >= 1, 'no GPU visible'
    ref = U.build_ref(tempfile.mkdtemp(prefix='covis_bench_'))
    m = api.Matcher(0)
    lines = ['# tools/covisibility_bench.py: the counting loop of KeyFrame::UpdateConnections for every keyframe of a synthetic map (%d entries per'
             % ENTRIES, '# keyframe, about %d of them MapPoints with 2..12 observations), host loop (std::map, one core) against ONE orbfe_covisibility_counts call;'
             % MP_PER_KF, '# host clock, median of %d rounds after a warm-up, ms.  gpu = staging (check + arena fill on the host) + kernel (stream events) + rest' % args.reps,
             '# (copies, waits, output assembly).  ratio = host / gpu: above 1 the GPU call is faster.  Neither figure holds the walk over the',
             '# KeyFrame / MapPoint objects that writes the index arrays down (include/orbfe/Covisibility.h does it once per batch; not timed here).',
             'case                 keyframes  subjects  observations   entries_out  MB_up   host_ms     gpu_ms (min .. max)            staging   kernel     rest   ratio']
    fmt = '%-20s %9d %9d %13d %13d %6.1f %9.2f %10.2f (%8.2f .. %8.2f) %9.2f %8.3f %8.2f %7.2f'
    last = None
    for n_kf in args.keyframes:
        arrays = synth_map(n_kf, np.random.default_rng(n_kf))
        last = (n_kf, arrays)
        for name, limit in (('full counters', None), ('map load (limit k+1)', np.arange(1, n_kf + 1, dtype=np.int32))):
            r = measure(api, U, ref, m, n_kf, arrays, limit, args.reps)
            lines.append(fmt % (name, n_kf, n_kf, r['obs'], r['entries'], r['bytes_up'] / 1e6, r['host'], r['gpu'], r['gpu_min'], r['gpu_max'],
                                r['staging'], r['kernel'], r['rest'], r['host'] / r['gpu']))
            print(lines[-1], flush=True)
    n_kf, (oo, ok, _, _, _) = last
    r = measure(api, U, ref, m, n_kf, frame_case(n_kf, oo, ok, np.random.default_rng(1)), None, max(args.reps, 21))
    lines.append(fmt % ('one frame (Tracking)', n_kf, 1, r['obs'], r['entries'], r['bytes_up'] / 1e6, r['host'], r['gpu'], r['gpu_min'], r['gpu_max'],
                        r['staging'], r['kernel'], r['rest'], r['host'] / r['gpu']))
    print(lines[-1], flush=True)
    if r['host'] < r['gpu']:
        lines.append('# one frame: the one-subject call is SLOWER than the host loop (%.3f ms against %.3f ms): per-frame callers keep the host loop.'
                     % (r['gpu'], r['host']))
    else:
        lines.append('# one frame: the one-subject call is faster than the host loop (%.3f ms against %.3f ms).' % (r['gpu'], r['host']))
    print(lines[-1], flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
