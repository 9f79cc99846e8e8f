#!/usr/bin/env python
"""A blocking 1080p / 2 000-feature extraction plus the resident frame built from it, for a 5-coefficient pinhole camera:
  gpu    orbfe_extractor_set_camera: k_undistort behind the descriptor kernel, orbfe_frame_create_from_extract without coordinates
  host   the route before it: extract, orbfe_undistort_pinhole on the returned keypoints, orbfe_frame_create_from_extract with the
         8 bytes per keypoint uploaded
Median of --reps calls after warm-up on a host clock; each call ends with the frame's descriptors being complete on the device.
-> profiles/undistort_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAM = (517.306408, 516.469215, 318.643040 * 3, 255.313989 * 2.25, (0.262383, -0.953104, -0.005358, 0.002628, 1.163314))


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
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'undistort_bench.txt'))
    a = ap.parse_args()
    from os1_amd import api
    from os1_amd import stream_workload as sw
    assert api.device_count() >= 1, 'needs a GPU'
    fx, fy, cx, cy, dist = CAM
    img = api.PinnedArray((sw.H, sw.W))
    img.a[:] = sw.StreamFrames(sw.stream_seed(0), pool=1).frame(0)
    bounds = api.compute_image_bounds(sw.W, sw.H, 0, fx, fy, cx, cy, dist)
    gpu = api.Extractor(sw.NFEAT, sw.SCALE, sw.NLEVELS, sw.INI_TH, sw.MIN_TH, 0)
    gpu.set_camera(fx, fy, cx, cy, dist)
    host = api.Extractor(sw.NFEAT, sw.SCALE, sw.NLEVELS, sw.INI_TH, sw.MIN_TH, 0)

    def run_gpu():
        k, d, xy = gpu.extract_undistorted(img.a)
        fr = api.Frame.from_extract(gpu, 0, bounds)
        fr.descriptors_device()
        return xy

    def run_host():
        k, d = host(img.a)
        xy = api.undistort_pinhole(np.stack([k['x'], k['y']], 1), fx, fy, cx, cy, dist)
        fr = api.Frame.from_extract(host, 0, bounds, xy)
        fr.descriptors_device()
        return xy

    equal = run_gpu().tobytes() == run_host().tobytes()
    g, h = median_ms(run_gpu, a.reps), median_ms(run_host, a.reps)
    lines = ['# tools/undistort_bench.py: blocking 1080p / 2000-feature extraction + resident frame for a 5-coefficient camera; median ms of %d calls (min..max)' % a.reps,
             'gpu   %.3f (%.3f..%.3f)' % g, 'host  %.3f (%.3f..%.3f)' % h, 'xy_un equal: %s' % equal]
    print('\n'.join(lines))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
