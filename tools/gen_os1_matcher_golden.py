#!/usr/bin/env python3
"""Writes tests/golden/os1_matcher_outputs.npz: the results of every scene of tests/os1_matcher_ref_util.registry() as computed by
oracle/_ref/libos1_matcher.so, the reference's own src/ORBmatcher.cc compiled by oracle/Makefile.  Recorded results only -- match
indices, counts, bookkeeping arrays, the updated vbPrevMatched -- for checkouts that cannot build the library.  Refuses to write
unless the library is there and says it is the reference build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import keyframe_projection_util as KP  # noqa: E402
import os1_matcher_ref_util as R  # noqa: E402
import source_projection_util as SP  # noqa: E402
from oracle.pyoracle import Oracle, build  # noqa: E402


def main():
    build()
    assert R.have_lib(), 'oracle/_ref/libos1_matcher.so missing: run make -C oracle where the reference exists'
    o = Oracle()
    SP.bind_oracle(o)
    KP.bind_oracle(o)
    ref = R.RefBackend(o)          # asserts os1_matcher_is_reference_build()
    whole = R.Whole(ref.L)
    out, skipped = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for key, runner in R.registry(KP.build_ref(tmp)):
            try:
                res = runner(ref, whole)
            except R.Unmappable:
                skipped.append(key)
                continue
            for field, v in res.items():
                v = np.asarray(v)
                small = v.dtype.kind in 'iu' and (v.size == 0 or (v.min() >= -2 ** 31 and v.max() < 2 ** 31))
                out['%s|%s' % (key, field)] = v.astype(np.int32) if small else v
    out[R.UNMAPPED] = np.array(skipped)
    np.savez_compressed(R.GOLDEN, **out)
    print('%s: %d arrays of %d scenes (%d array-form scenes no member expresses), %d bytes' %
          (os.path.relpath(R.GOLDEN, ROOT), len(out), len({k.rsplit("|", 1)[0] for k in out if "|" in k}), len(skipped), os.path.getsize(R.GOLDEN)))


if __name__ == '__main__':
    main()
