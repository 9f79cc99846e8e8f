#!/usr/bin/env python
"""The counting loop of LocalMapping::KeyFrameCulling for one job, on the host against one orbfe_redundant_observations call, in
the same run -> profiles/keyframe_culling_bench.txt.

Job (tests/keyframe_culling_util.culling_job, seeded): 100 local keyframes of 1 000 keypoint entries each, the MapPoints observed
by 2 to 40 keyframes of the 200 around them, levels 0..7.  Timed, the median of `--reps` rounds after one warm-up:
  host loop    tests/cpp/keyframe_culling_ref.cpp kfcull_ref_loop_ms: per (keyframe, MapPoint) a copy of the MapPoint's
               std::map<KeyFrame*, size_t> of observations and the observers' octaves through mvKeysUn, one core, structures built
               beforehand
  write-down   kfcull_ref_writedown_ms: the arrays of the call from the same structures, the way include/orbfe/KeyFrameCulling.h
               writes them (every distinct MapPoint's map read once), one core
  GPU call     one orbfe_redundant_observations through the C ABI with arrays prepared beforehand (ctypes), on a host clock; the
               call's own split (orbfe_debug_culling_ms): argument check + staging on the host, the kernel (stream events), the rest
               (copies up and down, the wait)
and the same three for a recount of the job's last 50 keyframes, as after a cull in the middle of the list: a job with one recount
costs the two rows together.  The two routes' outputs are compared before anything is timed.  No threshold: the numbers are the
result; the one that matters is write-down + call against the host loop."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure(U, ref, m, c, reps):
    got = m.redundant_observations(*c.args())                     # warm-up: buffers grow here; and the comparison
    want = U.ref_counts(ref, c)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    wall, split = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.redundant_observations(*c.args())
        wall.append((time.perf_counter() - t0) * 1e3)
        split.append(m.culling_ms())
    i = int(np.argsort(wall)[len(wall) // 2])
    host, chk = U.ref_loop_ms(ref, c, reps)
    assert chk == int(want[1].sum()), (chk, int(want[1].sum()))
    down, _ = U.ref_writedown_ms(ref, c, reps)
    e0, e1 = int(c.subj_offsets[0]), int(c.subj_offsets[-1])
    return dict(host=host, down=down, gpu=wall[i], gpu_min=min(wall), gpu_max=max(wall), staging=split[i][0], kernel=split[i][1],
                rest=split[i][2] - split[i][0] - split[i][1], entries=int((c.subj_mp[e0:e1] >= 0).sum()), obs=int(c.obs_offsets[-1]),
                redundant=int(want[1].sum()), bytes_up=4 * (2 * len(c.obs_offsets) + c.n_subj * 2) + 5 * (len(c.obs_kf) + e1 - e0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--subjects', type=int, default=100)
    ap.add_argument('--entries', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'keyframe_culling_bench.txt'))
    args = ap.parse_args()
    from os1_amd import api
    import keyframe_culling_util as U
    assert api.device_count() >= 1, 'no GPU visible'
    ref = U.build_ref(tempfile.mkdtemp(prefix='kfcull_bench_'))
    m = api.Matcher(0)
    job = U.culling_job(n_subj=args.subjects, entries=args.entries)
    half = args.subjects // 2
    recount = job.but(subj_self=job.subj_self[half:].copy(), subj_offsets=job.subj_offsets[half:].copy())
    lines = ['# tools/keyframe_culling_bench.py: the counting loop of LocalMapping::KeyFrameCulling for one job (%d local keyframes x %d entries, MapPoints'
             % (args.subjects, args.entries), '# with 2..40 observations), host loop (a std::map copy per keyframe and MapPoint, one core) against the write-down of the arrays (one core) + ONE',
             '# orbfe_redundant_observations call; host clock, median of %d rounds after a warm-up, ms.  gpu = staging (check + arena fill on the host) +' % args.reps,
             '# kernel (stream events) + rest (copies, wait).  ratio = host / (write-down + gpu): above 1 the batched route is faster.  A job with one',
             '# recount costs the two rows together; the host loop costs its first row whatever is culled.',
             'case                  subjects  MapPoint_entries  observations  redundant  MB_up   host_ms  writedown_ms     gpu_ms (min .. max)          staging   kernel     rest   ratio']
    fmt = '%-20s %9d %17d %13d %10d %6.2f %9.2f %13.2f %10.3f (%7.3f .. %7.3f) %9.3f %8.3f %8.3f %7.2f'
    rows = []
    for name, c in (('whole job', job), ('recount, second half', recount)):
        r = measure(U, ref, m, c, args.reps)
        rows.append(r)
        lines.append(fmt % (name, c.n_subj, r['entries'], r['obs'], r['redundant'], r['bytes_up'] / 1e6, r['host'], r['down'], r['gpu'], r['gpu_min'],
                            r['gpu_max'], r['staging'], r['kernel'], r['rest'], r['host'] / (r['down'] + r['gpu'])))
        print(lines[-1], flush=True)
    both = sum(r['down'] + r['gpu'] for r in rows)
    lines.append('# a job with one recount: %.2f ms (write-down + call, twice) against %.2f ms for the host loop' % (both, rows[0]['host']))
    print(lines[-1], flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
