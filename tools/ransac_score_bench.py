#!/usr/bin/env python
"""One orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses call against the single-core time of the restatement's scoring
loop (tests/cpp/ransac_score_ref.cpp, rsr_score_sim3 / rsr_score_pnp: CheckInliers once per hypothesis) on the same arrays, in the
same run -> profiles/ransac_score_bench.txt.

Four job sizes, segments x hypotheses per segment x correspondences per segment, for both models:
  round     10 x 5 x 100      one round of the reference's round-robin (LoopClosing.cc:286-346, Tracking.cc:1030-1060)
  whole     10 x 300 x 100    every hypothesis of every candidate at once
  large     10 x 300 x 1000
  refine     1 x 1 x 100      a single PnPsolver::Refine (or one Sim3 hypothesis)
Timed, each as the median of `--reps` calls after warm-up, on a host clock, through ctypes on both sides with the arrays already
in their final layout:
  gpu_ms    the C call: argument check, staging into page-locked memory, one upload, one kernel, the wait, the copy to the caller's
            arrays (the call blocks until the results are written)
  ref_ms    the restatement's loop over the same hypotheses on one core, counts and packed words written the same way
The minimal-set solves are in neither side's time."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

JOBS = (('round', 10, 5, 100), ('whole', 10, 300, 100), ('large', 10, 300, 1000), ('refine', 1, 1, 100))


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def job(U, model, n_seg, per_seg, n):
    make = U.make_sim3 if model == 'sim3' else U.make_pnp
    parts = [make(500 + s, n, per_seg) for s in range(n_seg)]
    seg_off = np.arange(n_seg + 1, dtype=np.int32) * n
    hyp_seg = np.tile(np.arange(n_seg, dtype=np.int32), per_seg)      # interleaved, as a round-robin hands them over
    hyp = np.stack([parts[s][2][k] for k in range(per_seg) for s in range(n_seg)])
    return U.Call(model, np.concatenate([p[0] for p in parts]), np.stack([p[1] for p in parts]), hyp, seg_off, hyp_seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import ransac_score_util as U
    from os1_amd import api
    assert api.device_count() >= 1, 'needs a GPU'
    ref = U.build_ref(tempfile.mkdtemp())
    m = api.Matcher(0)
    L, p = m.L, U._p
    lines = ['# median ms of %d calls (min..max); segments x hypotheses per segment x correspondences per segment' % a.reps,
             '# model job    shape          | gpu_ms (min..max)        | ref_ms (min..max)        | gpu/ref | equal']
    for model in ('sim3', 'pnp'):
        for name, n_seg, per_seg, n in JOBS:
            c = job(U, model, n_seg, per_seg, n)
            K = len(c.hyp)
            nw = sum(U.words_of(c.n_of(k)) for k in range(K))
            out = [(np.zeros(K, np.int32), np.zeros(nw, np.uint64)) for _ in range(2)]
            if model == 'sim3':
                T12, T21 = c.T12, c.T21
                gpu = lambda: L.orbfe_score_sim3_hypotheses(m.h, n_seg, p(c.seg_off), p(c.corr), p(c.cams), K, p(c.hyp_seg), p(T12), p(T21),
                                                            p(out[0][0]), None, p(out[0][1]))
                cpu = lambda: ref.rsr_score_sim3(n_seg, p(c.seg_off), p(c.corr), p(c.cams), K, p(c.hyp_seg), p(T12), p(T21), p(out[1][0]), None,
                                                 p(out[1][1]))
            else:
                gpu = lambda: L.orbfe_score_pnp_hypotheses(m.h, n_seg, p(c.seg_off), p(c.corr), p(c.cams), K, p(c.hyp_seg), p(c.hyp), p(out[0][0]),
                                                           None, p(out[0][1]))
                cpu = lambda: ref.rsr_score_pnp(n_seg, p(c.seg_off), p(c.corr), p(c.cams), K, p(c.hyp_seg), p(c.hyp), p(out[1][0]), None, p(out[1][1]))
            assert gpu() == 0 and cpu() == 0
            g = median_ms(gpu, a.reps)
            r = median_ms(cpu, a.reps)
            equal = 'bit-equal' if np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) else 'DIFFERENT'
            lines.append('%-5s %-6s %3d x %3d x %4d | %8.3f (%.3f..%.3f) | %8.3f (%.3f..%.3f) | %7.2f | %s' % (
                model, name, n_seg, per_seg, n, g[0], g[1], g[2], r[0], r[1], r[2], g[0] / r[0], equal))
            print(lines[-1], flush=True)
    m.close()
    text = '\n'.join(lines) + '\n'
    if a.out:
        open(a.out, 'w').write(text)
    assert 'DIFFERENT' not in text


if __name__ == '__main__':
    main()
