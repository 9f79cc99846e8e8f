#!/usr/bin/env python3
"""Writes tests/golden/os1_initializer_outputs.npz: the scores of every hypothesis, the winner, its score and its inlier mask for
every case of tests/init_score_util's N / K sweep, and the scores and masks of the boundary set, as computed by
oracle/_ref/libos1_initializer.so, the reference's own src/Initializer.cc (CheckHomography / CheckFundamental) compiled by
oracle/Makefile.  Recorded results only.  Refuses to write unless the library is there and says it is the reference build."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import init_score_util as U  # noqa: E402
from oracle.pyoracle import build  # noqa: E402


def main():
    build()
    assert U.have_os1(), 'oracle/_ref/libos1_initializer.so missing: run make -C oracle where the reference exists'
    with tempfile.TemporaryDirectory() as d:
        out = U.golden_records(U.build_ref(d))          # the restatement only places the crafted hypotheses in their sets
    np.savez_compressed(U.GOLDEN, **out)
    size = os.path.getsize(U.GOLDEN)
    print('%s: %d arrays of %d cases, %d bytes' % (os.path.relpath(U.GOLDEN, ROOT), len(out), len({k.rsplit("|", 1)[0] for k in out}), size))
    assert size <= 480 * 1024


if __name__ == '__main__':
    main()
