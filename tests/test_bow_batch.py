"""CPU side of the map-load bulk calls (orbfe_bow_transform_batch, orbfe_kfdb_add_batch): the header as C with the new
declarations; the library's exports and the binding; the argument checks that need no device; the host-side bookkeeping
(set-offset table, capacity check, all-or-nothing overflow, the keyframe database's duplicate / overflow pre-check and placement)
as a stand-alone program under the address and undefined-behaviour sanitizers; and the two shim overloads on a stub KeyFrame
type over a host back end.  The GPU side is tests/test_gpu_bow_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bow_batch_util as B


def test_header_compiles_as_c_with_the_new_declarations(tmp_path):
    p = str(tmp_path / 't.c')
    open(p, 'w').write('#include "orbfe.h"\nint main(void) { return (int)sizeof(&orbfe_bow_transform_batch) - (int)sizeof(&orbfe_kfdb_add_batch); }\n')
    for std in ('c99', 'c11'):
        subprocess.check_call(['gcc', '-x', 'c', '-std=' + std, '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I' + os.path.join(B.ROOT, 'include'), p])
    subprocess.check_call(['g++', '-x', 'c++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', '-I' + os.path.join(B.ROOT, 'include'), p])


def test_library_exports_the_two_calls_and_the_binding_matches_the_header():
    from os1_amd import api
    L = api.load_library()
    hdr = open(os.path.join(B.ROOT, 'include', 'orbfe.h')).read()
    for name, n in dict(orbfe_bow_transform_batch=15, orbfe_kfdb_add_batch=6).items():
        assert len(getattr(L, name).argtypes) == n
        m = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert m and len(m.group(1).split(',')) == n, name
    assert api.Vocabulary.transform_batch and api.KeyFrameDatabase.add_batch and api.BowBatchOutputs


def test_null_handles_and_negative_counts_are_refused_before_any_device_work():
    from os1_amd import api
    L = api.load_library()
    one = np.zeros(1, np.int32)
    ptrs = np.zeros(1, np.uint64)
    assert L.orbfe_bow_transform_batch(None, 4, 1, *[ptrs.ctypes.data_as(C.c_void_p)] * 12) == -1
    assert L.orbfe_last_error()
    assert L.orbfe_kfdb_add_batch(None, 1, ptrs.ctypes.data_as(C.c_void_p), ptrs.ctypes.data_as(C.c_void_p), ptrs.ctypes.data_as(C.c_void_p),
                                  one.ctypes.data_as(C.c_void_p)) == -1


def test_host_side_bookkeeping_under_the_sanitizers(tmp_path):
    """set-offset table and the wave search over it, capacity checks, all-or-nothing; the keyframe database's pre-check and placement
    against a simulation of single adds -- a program of its own, the sanitizers linked into it"""
    B.run(B.compile_plan_test(str(tmp_path / 'plan_asan'), sanitize=True))


def test_shim_overloads_on_the_host_back_end(tmp_path):
    """ComputeBoW(voc, vector) equals the one-keyframe overload keyframe by keyframe, sends the three keyframes without vectors in ONE
    call and leaves the computed one alone; KeyFrameDatabaseT::add(vector) equals single adds"""
    B.run(B.compile_shim_test(str(tmp_path / 'shim_host'), host_backend=True))


def test_keyframe_database_header_still_compiles_against_the_reference_names(tmp_path):
    import kfdb_facade as F
    F.syntax_check(str(tmp_path / 'kfdb_header.o'))
