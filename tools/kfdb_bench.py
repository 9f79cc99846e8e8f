#!/usr/bin/env python
"""One orbfe_kfdb_query against the single-core time of the reference restatement (tests/cpp/kfdb_ref.cpp) on the same map, in the
same run -> profiles/kfdb_bench.txt.

Map: 500, 2 000 and 8 000 keyframes of about 1 200 words each, drawn from 10^6 words with p(w) ~ 1 / (w + 1000): a few thousand
frequent words that most keyframes hold and a long tail, the skew a tf-idf vocabulary gives.  The query is a frame that revisits
one keyframe (half of its words) plus fresh draws.  Timed, each as the median of `--reps` calls after warm-up, on a host clock around
calls that end in a device synchronise:
  query     one orbfe_kfdb_query (upload of the query, k_kfdb_query over every keyframe, host sort of the sharing keyframes)
  ref_walk  the restatement's inverted-file walk alone (KeyFrameDatabase.cc:207-222 on std::list / std::map), no scores
  ref_reloc the restatement's whole DetectRelocalizationCandidates (walk, scores of the keyframes above 0.8 max, accumulation)
  add/erase one orbfe_kfdb_add / orbfe_kfdb_erase (mean over the map's keyframes)
The kernel's own duration comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_WORDS = 1000000


def draw(rng, n):
    u = rng.random(int(n * 1.4))
    w = np.floor(1000.0 * np.power(1.0 + N_WORDS / 1000.0, u) - 1000.0).astype(np.int64)
    w = np.unique(np.clip(w, 0, N_WORDS - 1))
    if len(w) > n:
        w = np.sort(rng.choice(w, n, replace=False))
    v = rng.uniform(0.2, 9.0, len(w))
    return w.astype(np.uint32), v / np.sum(v)


def median_ms(fn, reps, warmup=3):
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
    ap.add_argument('--sizes', default='500,2000,8000')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-ref', action='store_true', help='GPU side only (for a profiler run)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import kfdb_util as K
    from os1_amd import api
    assert api.device_count() >= 1, 'needs a GPU'
    lib = None if a.no_ref else K.build_ref(tempfile.mkdtemp())
    lines = ['# keyframes words/kf query_words sharing | query_ms (min..max) | ref_walk_ms ref_reloc_ms | add_us erase_us | equal']
    for n in (int(s) for s in a.sizes.split(',')):
        rng = np.random.default_rng(n)
        kfs = [draw(rng, 1200) for _ in range(n)]
        fresh = draw(rng, 700)
        qw = np.union1d(kfs[n // 3][0][::2], fresh[0]).astype(np.uint32)
        qv = rng.uniform(0.2, 9.0, len(qw))
        qv /= np.sum(qv)
        entries = sum(len(w) for w, _ in kfs)
        db = api.KeyFrameDatabase(N_WORDS, K.L1, n, entries)
        t0 = time.perf_counter()
        for i, (w, v) in enumerate(kfs):
            db.add(i, w, v)
        add_us = (time.perf_counter() - t0) * 1e6 / n
        q_ms = median_ms(lambda: db.query(qw, qv), a.reps)
        keys, common, scores = db.query(qw, qv)
        walk_ms = reloc_ms = float('nan')
        equal = 'not checked'
        if lib is not None:
            scene = dict(n_words=N_WORDS, scoring=K.L1, kfs=[dict(index=i, id=i, words=w, values=v, connected=set(), covisible=[], bad=False)
                                                              for i, (w, v) in enumerate(kfs)])
            ref = K.Ref(lib, scene)
            for i in range(n):
                ref.step(('add', i))
            C = K.C
            out, com = np.zeros(n, np.int32), np.zeros(n, np.int32)
            walk_ms = median_ms(lambda: lib.kref_sharing(ref.h, K._p(qw), K._p(qv), len(qw), K._p(out), K._p(com), None, n), a.reps)[0]
            fid = [10]

            def reloc():
                fid[0] += 1
                lib.kref_detect_reloc(ref.h, fid[0], K._p(qw), K._p(qv), len(qw), K._p(out), n)
            reloc_ms = median_ms(reloc, a.reps)[0]
            rk, rc, rs = ref.sharing(qw, qv)
            equal = 'bit-equal' if (keys.tolist() == rk.tolist() and common.tolist() == rc.tolist()
                                    and scores.view(np.uint64).tolist() == rs.view(np.uint64).tolist()) else 'DIFFERENT'
            ref.close()
        t0 = time.perf_counter()
        for i in range(n):
            db.erase(i)
        erase_us = (time.perf_counter() - t0) * 1e6 / n
        db.close()
        lines.append('%6d %6.0f %5d %6d | %8.3f (%.3f..%.3f) | %9.3f %9.3f | %7.1f %7.2f | %s' % (
            n, entries / n, len(qw), len(keys), q_ms[0], q_ms[1], q_ms[2], walk_ms, reloc_ms, add_us, erase_us, equal))
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if a.out:
        open(a.out, 'w').write(text)
    assert 'DIFFERENT' not in text


if __name__ == '__main__':
    main()
