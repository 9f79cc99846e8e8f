"""Local-map projection + SearchLocalPoints timings on a resident 1080p frame (orbfe_search_local_points_frame and the
calls it replaces), one JSON line per configuration.

  fused        orbfe_search_local_points_frame: k_project_local_map + window search + bookkeeping, one submission
  two_step     orbfe_project_local_map, then orbfe_search_by_projection_frame_rows
  rows_only    orbfe_search_by_projection_frame_rows with the projection's fields precomputed (what the caller had before)
  host_loop    the projection restated on the host (tests/cpp/is_in_frustum_ref.cpp): restated arithmetic, no cv::Mat --
               NOT the reference's cost, which adds locked cv::Mat clones and temporaries per MapPoint

Median and p90 over >= 200 warm calls; every call returns with its results (a sync per call).

  usage: python tools/local_map_bench.py [--iters 300] [--out profiles/local_map_bench.json] [--only-fused]"""
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
from os1_amd.synth import shifted, synth  # noqa: E402
import local_map_util as U  # noqa: E402


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_us=round(float(np.median(a)), 2), p90_us=round(float(np.percentile(a, 90)), 2), n=len(a))


def timed(fn, iters, warm=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-fused', action='store_true', help='the fused call only (for a kernel trace)')
    a = ap.parse_args()
    W, H = 1920, 1080
    A = synth(11, W, H)
    B = shifted(A, 3, -2, 12)
    ex = api.Extractor(2000, 1.2, 8, 20, 7)
    kA, dA = ex(A)
    kB, dB = ex(B)
    sf = ex.tables()['sf']
    ex.close()
    m = api.Matcher(0)
    bounds = (0.0, float(W), 0.0, float(H))
    frame = m.frame(kB, dB, bounds)
    ref = U.build_ref(tempfile.mkdtemp())
    results = []
    for n_mp in (3000, 10000):
        camA = U.camera(W, H)
        mp = U.triangulate(kA, dA, sf, n_mp, camA, seed=n_mp)
        cam = U.moved_camera(W, H, 3, -2, 8.0, seed=1)
        acam = U.api_camera(api, cam)
        rows = np.arange(n_mp, dtype=np.int32)
        flags = U.flags_for(n_mp, seed=2, bad=0.0, skip=0.0)
        occ = np.zeros(len(kB), np.uint8)
        lm = api.LocalMap(m, n_mp)
        lm.set_rows(rows, mp['pos'], mp['normal'], mp['min'], mp['max'], mp['desc'])
        pin = {k: api.PinnedArray(v.shape, v.dtype) for k, v in dict(rows=rows, flags=flags, occ=occ).items()}
        pin['rows'].a[:] = rows
        pin['flags'].a[:] = flags
        pin['occ'].a[:] = occ
        r = dict(config='1080p', n_mp=n_mp, th=1.0)
        fused = lambda: m.search_local_points(frame, lm, acam, pin['rows'].a, pin['flags'].a, pin['occ'].a, sf, 1.0)  # noqa: E731
        res = fused()
        r['nmatches'], r['n_in_view'] = res['nmatches'], res['n_in_view']
        r['fused'] = stats(timed(fused, a.iters))
        if not a.only_fused:
            proj = m.project_local_map(frame, lm, acam, rows, flags)
            tab = api.DescTable(n_mp)
            tab.host.a[:] = mp['desc']
            tab.upload(m, 0, n_mp)
            pf = {k: api.PinnedArray(v.shape, v.dtype) for k, v in dict(xy=proj['proj_xy'], lv=proj['level'], vc=proj['view_cos'],
                                                                        fl=U.oracle_flags(proj, flags)).items()}
            pf['xy'].a[:] = proj['proj_xy']
            pf['lv'].a[:] = proj['level']
            pf['vc'].a[:] = proj['view_cos']
            pf['fl'].a[:] = U.oracle_flags(proj, flags)

            def two_step():
                p = m.project_local_map(frame, lm, acam, pin['rows'].a, pin['flags'].a)
                return m.search_by_projection_rows(frame, sf, pin['occ'].a, p['proj_xy'], p['level'], p['view_cos'],
                                                   U.oracle_flags(p, flags), tab, pin['rows'].a, 1.0, 0.8)

            def rows_only():
                return m.search_by_projection_rows(frame, sf, pin['occ'].a, pf['xy'].a, pf['lv'].a, pf['vc'].a, pf['fl'].a, tab,
                                                   pin['rows'].a, 1.0, 0.8)
            assert two_step()[0] == rows_only()[0] == res['nmatches']
            r['two_step'] = stats(timed(two_step, a.iters))
            r['rows_only'] = stats(timed(rows_only, a.iters))
            r['host_loop_restated_arithmetic_no_cvMat'] = stats(timed(lambda: U.ref_project(ref, mp, rows, flags, cam, bounds),
                                                                      a.iters))
            tab.free()
        lm.close()
        print(json.dumps(r), flush=True)
        results.append(r)
    frame.close()
    m.close()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
