#!/usr/bin/env python3
"""Writes tests/golden/triangulation_batch_outputs.npz: the inputs of the multi-neighbour jobs of tests/triangulation_batch_util.py
and what oracle/_ref/libos1_matcher.so -- the reference's own src/ORBmatcher.cc compiled by oracle/Makefile -- returns for them:
the raw row of every neighbour (SearchForTriangulation without the orientation check, the flags at loop entry) and the pairs of
the loop of LocalMapping.cc:207-232 with the current keyframe's flags evolving, for both settings of the orientation check.
Arrays only.  Refuses to write unless the library is there and says it is the reference build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import os1_matcher_ref_util as R  # noqa: E402
import triangulation_batch_util as T  # noqa: E402
from oracle.pyoracle import Oracle, build  # noqa: E402


def main():
    build()
    assert R.have_lib(), 'oracle/_ref/libos1_matcher.so missing: run make -C oracle where the reference exists'
    o = Oracle()
    ref = R.RefBackend(o)          # asserts os1_matcher_is_reference_build()
    out = {}
    for name, spec in T.JOBS.items():
        job = T.make_job(spec)
        raw = T.ref_raw_rows(ref, job)
        seq = {ori: T.ref_sequence(ref, job, bool(ori)) for ori in (0, 1)}
        assert (raw == T.ref_raw_rows(o, job)).all() and all(seq[ori] == T.ref_sequence(o, job, bool(ori)) for ori in (0, 1)), 'oracle and reference disagree'
        print('%s: %d keypoints against %s; raw matches per neighbour %s; loop pairs %s (no check) %s (orientation check)' % (
            name, len(job['kf1']['kps']), [len(nb['kps']) for nb in job['nb']], [int((r >= 0).sum()) for r in raw],
            [n for n, _ in seq[0]], [n for n, _ in seq[1]]))
        out.update(T.pack(name, job, raw, seq))
    np.savez_compressed(T.GOLDEN, **out)
    print('wrote %s: %d arrays, %d bytes' % (os.path.relpath(T.GOLDEN, ROOT), len(out), os.path.getsize(T.GOLDEN)))


if __name__ == '__main__':
    main()
