"""Last-frame / keyframe projection search timings on resident 1080p frames (2 000 features; the sources are the last frame's
keypoints, about half of them with a MapPoint), one JSON line per mode.

  uv_frame     orbfe_search_by_projection_uv_frame on PREPARED page-locked arrays: the existing route from the projection on --
               what is left of it once the host projection loop (not timed here) has run; reads 50 bytes per source over PCIe
  fused        orbfe_search_by_projection_sources_frame: k_project_sources + window search + bookkeeping, one submission;
               reads 5 bytes per source (row, flag byte) over PCIe
  facade       (--facade) the C++ facade end to end, host projection loop included, old function against new
               (tests/cpp/source_projection_test.cpp in `time` mode, as tools/facade_timing.py does for the other searches)

Median, p10 and p90 over >= 200 warm blocking calls (every call returns with its results).

  usage: python tools/source_projection_bench.py [--iters 300] [--out profiles/source_projection_bench.json] [--only-fused] [--facade]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from os1_amd import api  # noqa: E402
import local_map_util as U  # noqa: E402
import source_projection_util as S  # noqa: E402


def stats(ts):
    a = np.array(ts) * 1e3
    return dict(median_us=round(float(np.median(a)), 2), p10_us=round(float(np.percentile(a, 10)), 2),
                p90_us=round(float(np.percentile(a, 90)), 2), n=len(a))


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


def facade(W, H):
    import source_projection_facade as F
    from os1_amd.synth import shifted, synth
    with tempfile.TemporaryDirectory() as d:
        exe = F.compile_test(os.path.join(d, 'source_projection_test'))
        base = synth(71, W, H)
        for k in range(2):
            shifted(base, -3 * k, k, 700 + k).tofile(os.path.join(d, 'f%03d.gray' % k))
        open(os.path.join(d, 'meta.txt'), 'w').write('%d %d %d %d %d %d\n' % (W, H, 2, 2000, -3, 1))
        r = subprocess.run([exe, d, 'time'], capture_output=True, text=True, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith('timing ')]
        assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads(line[0][len('timing '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only-fused', action='store_true', help='the fused call only (for a kernel trace)')
    ap.add_argument('--facade', action='store_true')
    a = ap.parse_args()
    W, H = 1920, 1080
    ex = api.Extractor(2000, 1.2, 8, 20, 7)
    kA, dA, kB, dB, sf = S.frames(W, H, 2000, extractor=ex)
    ex.close()
    m = api.Matcher(0)
    ref = S.build_ref(tempfile.mkdtemp())
    results = []
    for mode, name, th, max_dist in ((S.LAST_FRAME, 'last_frame', 15.0, 100), (S.KEYFRAME, 'keyframe', 10.0, 100)):
        sc = S.scene(kA, dA, kB, sf, W, H, seed=9, occupied=0.0)
        flags = S.flags_of(sc, mode)
        src = m.frame(kA, dA, sc['bounds'])
        cur = m.frame(kB, dB, sc['bounds'])
        n = len(sc['tab']['pos'])
        lm = api.LocalMap(m, n)
        lm.set_rows(np.arange(n), sc['tab']['pos'], sc['tab']['normal'], sc['tab']['min'], sc['tab']['max'], sc['tab']['desc'])
        acam = U.api_camera(api, sc['cam'])
        rows, fl, occ = pinned(sc['rows']), pinned(flags), pinned(sc['st']['occ'])
        r = dict(config='1080p', mode=name, n_src=int(len(kA)), sources_with_mappoint=int((sc['st']['absent'] == 0).sum()), th=th,
                 bytes_per_call=dict(fused=5 * len(kA), uv_frame=50 * len(kA)))
        fused = lambda: m.search_by_projection_sources(cur, src, lm, acam, mode, rows.a, fl.a, occ.a, sf, th, max_dist, True)  # noqa: E731
        res = fused()
        r['nmatches'], r['n_valid'] = res['nmatches'], res['n_valid']
        r['fused'] = stats(timed(fused, a.iters))
        if not a.only_fused:
            proj = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode)
            p = {k: pinned(np.ascontiguousarray(v)) for k, v in dict(uv=proj['uv'], lv=proj['level'], va=proj['valid'],
                                                                     ang=kA['angle'].astype(np.float32),
                                                                     desc=sc['tab']['desc'][sc['rows']]).items()}
            uv_frame = lambda: m.search_by_projection_uv(cur, None, None, sf, occ.a, p['uv'].a, p['lv'].a, p['ang'].a, fl.a,  # noqa: E731
                                                         p['va'].a, p['desc'].a, th, max_dist, mode == S.KEYFRAME, True)
            n2, a2 = uv_frame()
            assert n2 == res['nmatches'] and (a2 == res['kp_assigned']).all()
            r['uv_frame'] = stats(timed(uv_frame, a.iters))
            r['host_loop_restated_arithmetic_no_cvMat'] = stats(timed(
                lambda: S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode), a.iters))
        for h in (lm, cur, src):
            h.close()
        print(json.dumps(r), flush=True)
        results.append(r)
    m.close()
    if a.facade:
        f = dict(config='1080p', mode='facade_last_frame', **facade(W, H))
        print(json.dumps(f), flush=True)
        results.append(f)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
