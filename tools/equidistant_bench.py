#!/usr/bin/env python
"""A blocking extraction plus the resident frame built from it, for the Sony AS-20 equidistant fisheye camera, at 1080p / 2 000
features and at 3840 x 2160 / 4 000 features (BASELINE.json config 5):
  gpu    orbfe_extractor_set_camera_equidistant: k_undistort_equidistant behind the descriptor kernel, the host settle,
         orbfe_frame_create_from_extract without coordinates
  host   the route before it: extract, download, orbfe_undistort_equidistant on the returned keypoints, orbfe_frame_create_from_extract
         with the 8 bytes per keypoint uploaded
and k_undistort_equidistant against k_undistort (a 5-coefficient pinhole camera) on the frame's keypoints and on 262 144 points,
as the time of one orbfe_extractor_undistort call: upload, kernel, download and wait are the same in both, the equidistant call adds
the clearing and the download of its 256-byte undecided list.  With --kernels-only the script only issues those calls, for a run under a
kernel tracer.  Median of --reps calls after warm-up on a host clock.  -> profiles/equidistant_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SONY_720P = (732.0, 732.0, 613.0, 385.0)     # scaled with the image width (x 1.5, x 3)
PINHOLE_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
SIZES = ((1920, 1080, 2000, 1.5), (3840, 2160, 4000, 3.0))


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
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'equidistant_bench.txt'))
    a = ap.parse_args()
    from os1_amd import api
    from os1_amd import stream_workload as sw
    assert api.device_count() >= 1, 'needs a GPU'
    lines = ['# tools/equidistant_bench.py: median ms of %d calls (min..max)' % a.reps]
    for w, h, nfeat, s in SIZES:
        cam = tuple(v * s for v in SONY_720P)
        fx, fy, cx, cy = cam
        gpu = api.Extractor(nfeat, sw.SCALE, sw.NLEVELS, sw.INI_TH, sw.MIN_TH, 0)
        gpu.set_camera_equidistant(*cam)
        host = api.Extractor(nfeat, sw.SCALE, sw.NLEVELS, sw.INI_TH, sw.MIN_TH, 0)
        pin = api.Extractor(nfeat, sw.SCALE, sw.NLEVELS, sw.INI_TH, sw.MIN_TH, 0)
        pin.set_camera(fx, fy, cx, cy, PINHOLE_DIST)
        img = api.PinnedArray((h, w))
        img.a[:] = sw.StreamFrames(sw.stream_seed(0), w, h, pool=1).frame(0)
        bounds = api.compute_image_bounds(w, h, 1, fx, fy, cx, cy, ())

        def run_gpu():
            k, d, xy = gpu.extract_undistorted(img.a)
            api.Frame.from_extract(gpu, 0, bounds).descriptors_device()
            return xy

        def run_host():
            k, d = host(img.a)
            xy = api.undistort_equidistant(np.stack([k['x'], k['y']], 1), fx, fy, cx, cy)
            api.Frame.from_extract(host, 0, bounds, xy).descriptors_device()
            return xy

        k, _ = host(img.a)
        pts = np.stack([k['x'], k['y']], 1).astype(np.float32)
        rng = np.random.RandomState(1)
        big = np.stack([rng.uniform(0, w, 262144), rng.uniform(0, h, 262144)], 1).astype(np.float32)
        if a.kernels_only:
            for _ in range(a.reps):
                for p in (pts, big):
                    gpu.undistort(p)
                    pin.undistort(p)
            continue
        equal = run_gpu().tobytes() == run_host().tobytes()
        lines.append('%dx%d / %d features (%d keypoints), Sony AS-20 x %.1f' % (w, h, nfeat, len(pts), s))
        lines.append('  extraction + resident frame   gpu   %.3f (%.3f..%.3f)' % median_ms(run_gpu, a.reps))
        lines.append('  extraction + resident frame   host  %.3f (%.3f..%.3f)' % median_ms(run_host, a.reps))
        lines.append('  xy_un equal: %s' % equal)
        for name, p in (('%d keypoints' % len(pts), pts), ('262144 points', big)):
            lines.append('  undistort call, %-15s equidistant %.3f (%.3f..%.3f)' % ((name,) + median_ms(lambda: gpu.undistort(p), a.reps)))
            lines.append('  undistort call, %-15s pinhole     %.3f (%.3f..%.3f)' % ((name,) + median_ms(lambda: pin.undistort(p), a.reps)))
        s3 = gpu.equidistant_stats()
        lines.append('  settled on the host over the whole run: %d points, %d changed' % (s3[0], s3[1]))
    if a.kernels_only:
        return
    print('\n'.join(lines))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
