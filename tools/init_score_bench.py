#!/usr/bin/env python
"""One orbfe_score_init_hypotheses_kps / _frames call against the single-core time of the reference restatement's two scoring
loops (tests/cpp/init_score_ref.cpp, built -O3 here) on the same matches and hypotheses, in the same run
-> profiles/init_score_bench.txt.

K = 200 hypotheses per model (mMaxIterations), N = 100, 500 and 2 000 matches of the general scene of the tests.  Timed, each as
the median of `--reps` calls after warm-up, on a host clock around calls that end in a device synchronise (the C calls block):
  kps      one orbfe_score_init_hypotheses_kps: host compaction, upload of points and hypotheses, two kernels
           (k_init_score over 400 workgroups, k_init_select), results read from page-locked memory; Python binding included
  frames   one orbfe_score_init_hypotheses_frames on two resident frames: upload of matches12 and hypotheses, k_init_gather,
           the same two kernels
  ref_h    the restatement's FindHomography loop from the hypothesis on: 200 x CheckHomography
  ref_f    the restatement's FindFundamental loop from the hypothesis on: 200 x CheckFundamental
  ref_2thr max(ref_h, ref_f): the reference runs the two loops on two threads and joins both (Initializer.cc:104-109)
The 8-point solves (cv::SVD) are in neither side's time.  The kernels' own durations come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool with --no-ref."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='100,500,2000')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--no-ref', action='store_true', help='GPU side only (for a profiler run)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import init_score_util as U
    from os1_amd import api
    assert api.device_count() >= 1, 'needs a GPU'
    tmp = tempfile.mkdtemp()
    check = U.build_ref(tmp)                                                        # the tests' build: what "equal" compares with
    lib = None if a.no_ref else U.build_ref(tmp, flags=('-O3', '-ffp-contract=off'), name='init_score_ref_o3.so')
    scene = U.make_scene(False, U.SCENE_SEEDS['general'])
    H21, H12, F21 = U.random_hypotheses(scene, U.K_MAX, 1)
    m = api.Matcher(0)
    rng = np.random.default_rng(0)
    bounds = (0.0, 640.0, 0.0, 480.0)
    lines = ['# K = %d per model; median ms of %d calls (min..max)' % (U.K_MAX, a.reps),
             '#     N | kps_ms (min..max) | frames_ms (min..max) | ref_h_ms ref_f_ms ref_2thr_ms | equal']
    for n in (int(s) for s in a.sizes.split(',')):
        pts = scene['pts'][:n]
        k1, k2, m12 = U.keypoint_form(pts, n)
        f1 = m.frame(k1, rng.integers(0, 256, (len(k1), 32), dtype=np.uint8), bounds)
        f2 = m.frame(k2, rng.integers(0, 256, (len(k2), 32), dtype=np.uint8), bounds)
        kps = median_ms(lambda: m.score_init_hypotheses_kps(k1, k2, m12, U.SIGMA, H21, H12, F21), a.reps)
        frs = median_ms(lambda: m.score_init_hypotheses_frames(f1, f2, m12, U.SIGMA, H21, H12, F21), a.reps)
        got = m.score_init_hypotheses_frames(f1, f2, m12, U.SIGMA, H21, H12, F21)
        try:
            U.assert_same(got, U.ref_find(check, pts, U.SIGMA, H21, H12, F21), 'n=%d' % n)
            equal = 'bit-equal'
        except AssertionError as e:
            equal = 'DIFFERENT (%s)' % e
        rh = rf = float('nan')
        if lib is not None:
            rh = median_ms(lambda: U.ref_find(lib, pts, U.SIGMA, H21, H12, None), a.reps)[0]
            rf = median_ms(lambda: U.ref_find(lib, pts, U.SIGMA, None, None, F21), a.reps)[0]
        f1.close()
        f2.close()
        lines.append('%7d | %7.3f (%.3f..%.3f) | %7.3f (%.3f..%.3f) | %8.3f %8.3f %8.3f | %s' % (
            n, kps[0], kps[1], kps[2], frs[0], frs[1], frs[2], rh, rf, max(rh, rf), equal))
        print(lines[-1], flush=True)
    m.close()
    text = '\n'.join(lines) + '\n'
    if a.out:
        open(a.out, 'w').write(text)
    assert 'DIFFERENT' not in text


if __name__ == '__main__':
    main()
