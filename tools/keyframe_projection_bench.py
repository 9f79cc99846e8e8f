"""Keyframe-side projection search timings on a resident 1080p keyframe (2 000 features), one JSON line per size:

  LocalMapping   Fuse(pKF, vpMapPoints, th = 3): about 1 500 fuse candidates, chi-square gate
  LoopClosing    Fuse(pKF, Scw, vpPoints, th = 4) over 10 000 and 30 000 loop MapPoints

  fused            orbfe_search_projected_keyframe_frame: k_project_keyframe + window search + bookkeeping, one submission;
                   reads 5 bytes per MapPoint (row, flag byte) over PCIe
  host_projection  the route it replaces, first half: the projection loop on the host as orb_shim.hpp's projectIntoKeyFrame
                   does it (the restated arithmetic of tests/cpp/project_keyframe_ref.cpp, no cv::Mat temporaries) and the
                   copy of each valid point's 32-byte descriptor into the sources' array
  projected_frame  second half: orbfe_search_projected_frame on those arrays (page-locked); reads 49 bytes per MapPoint
  replaced_route   host_projection + projected_frame, timed as one call

Median, p10 and p90 over >= 200 warm blocking calls (every call returns with its results).  The fused call's results are
checked against the replaced route's before anything is timed.

  usage: python tools/keyframe_projection_bench.py [--iters 300] [--out profiles/keyframe_projection_bench.json] [--only-fused]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from os1_amd import api  # noqa: E402
import keyframe_projection_util as K  # noqa: E402


def stats(ts):
    a = np.array(ts)
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4),
                p90_ms=round(float(np.percentile(a, 90)), 4), n=len(a))


def timed(fn, iters, warm=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def pinned(a):
    p = api.PinnedArray(a.shape, a.dtype)
    p.a[:] = a
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-fused', action='store_true', help='the fused call only (for a kernel trace)')
    a = ap.parse_args()
    W, H = 1920, 1080
    ex = api.Extractor(2000, 1.2, 8, 20, 7)
    kA, dA, kB, dB, sf = K.SP.frames(W, H, 2000, extractor=ex)
    ex.close()
    m = api.Matcher(0)
    ref = K.build_ref(tempfile.mkdtemp())
    sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=9)
    kf = m.frame(kB, dB, sc['bounds'])
    M = sc['M']
    lm = api.LocalMap(m, M)
    lm.set_rows(np.arange(M), sc['tab']['pos'], sc['tab']['normal'], sc['tab']['min'], sc['tab']['max'], sc['tab']['desc'])
    is2 = (1.0 / (np.asarray(sf, np.float32) ** 2)).astype(np.float32)
    results = []
    for name, fn, n, th in (('LocalMapping', K.FUSE, 1500, 3.0), ('LoopClosing', K.FUSE_SCW, 10000, 4.0),
                            ('LoopClosing', K.FUSE_SCW, 30000, 4.0)):
        d = K.make_case(ref, fn, sc, th)['dirs'][0]
        rng = np.random.default_rng(n)
        pick = rng.integers(0, len(d['rows']), n)          # the case's points, drawn n times (a loop's MapPoints repeat places)
        rows_h, flags_h = np.ascontiguousarray(d['rows'][pick]), np.ascontiguousarray(d['flags'][pick])
        rows, fl = pinned(rows_h), pinned(flags_h)
        acam = K.api_projection(api, d['pr'])
        inv = is2 if d['chi2'] else None
        r = dict(config='1080p', thread=name, function=fn, n_points=n, n_keypoints=int(len(kB)), th=th,
                 bytes_per_call=dict(fused=5 * n, replaced_route=49 * n))
        fused = lambda: m.search_projected_keyframe(kf, lm, acam, rows.a, fl.a, sf, th, inv_sigma2=inv, max_dist=d['max_dist'])  # noqa: E731
        res = fused()
        r['nmatches'], r['n_valid'] = res['nmatches'], res['n_valid']
        r['fused'] = stats(timed(fused, a.iters))
        if not a.only_fused:
            desc = sc['tab']['desc']
            buf = {k: pinned(v) for k, v in dict(uv=np.zeros((n, 2), np.float32), ra=np.zeros(n, np.float32), lv=np.zeros(n, np.int32),
                                                 va=np.zeros(n, np.uint8), desc=np.zeros((n, 32), np.uint8)).items()}

            def host_projection():
                p = K.ref_project(ref, sc['tab'], rows_h, flags_h, d['pr'], sc['bounds'], sf, th)
                buf['uv'].a[:], buf['ra'].a[:], buf['lv'].a[:], buf['va'].a[:] = p['uv'], p['radius'], p['level'], p['valid']
                v = np.flatnonzero(p['valid'])
                buf['desc'].a[v] = desc[rows_h[v]]         # pMP->GetDescriptor() of every point that survives
                return p

            def projected_frame():
                return m.search_projected(kf, None, None, buf['uv'].a, buf['ra'].a, buf['lv'].a, buf['va'].a, buf['desc'].a,
                                          inv_sigma2=inv, max_dist=d['max_dist'])

            def replaced_route():
                host_projection()
                return projected_frame()
            n2, bi2, bd2 = replaced_route()
            assert n2 == res['nmatches'] and (bi2 == res['best_idx']).all() and (bd2 == res['best_dist']).all()
            r['host_projection'] = stats(timed(host_projection, a.iters))
            r['projected_frame'] = stats(timed(projected_frame, a.iters))
            r['replaced_route'] = stats(timed(replaced_route, a.iters))
            r['fused_wins'] = bool(r['fused']['median_ms'] < r['replaced_route']['median_ms'])
        print(json.dumps(r), flush=True)
        results.append(r)
    for h in (lm, kf):
        h.close()
    m.close()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
