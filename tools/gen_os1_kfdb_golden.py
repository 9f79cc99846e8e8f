#!/usr/bin/env python3
"""Writes tests/golden/os1_kfdb_outputs.npz: for every scene of tests/kfdb_util (the seeded ones and the crafted decision-boundary
ones) the candidate list of every query step and all six members of every keyframe after every step, as computed by
oracle/_ref/libos1_kfdb.so, the reference's own src/KeyFrameDatabase.cc compiled by oracle/Makefile.  Recorded results only; the
scenes are recipes.  Refuses to write unless the library is there and says it is the reference build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import kfdb_util as K  # noqa: E402
from oracle.pyoracle import build  # noqa: E402


def main():
    build()
    assert K.have_os1(), 'oracle/_ref/libos1_kfdb.so missing: run make -C oracle where the reference exists'
    out = K.golden_records()          # the binding asserts os1kfdb_is_reference_build()
    np.savez_compressed(K.GOLDEN, **out)
    size = os.path.getsize(K.GOLDEN)
    print('%s: %d arrays of %d scenes, %d bytes' % (os.path.relpath(K.GOLDEN, ROOT), len(out), len({k.split("|")[0] for k in out}), size))
    assert size <= 480 * 1024


if __name__ == '__main__':
    main()
