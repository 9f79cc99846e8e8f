"""CPU: the pieces of the device local map that need no GPU -- the glibc logf restatement PredictScale runs on
(os1_amd/csrc/glibc_logf.h) against the host libm, the reference restatement of the projection, and the C++ facade's
SearchLocalPoints (include/orbfe/orb_shim.hpp) compiling and linking against the C ABI."""
import numpy as np

import local_map_facade as F
import local_map_util as U


def test_logf_restatement_dense_range():
    from os1_amd import api
    assert api.logf_host_mismatches(0x3d800000, 0x457fffff) == 0     # every float in [2^-4, 2^12): 134 M values


def test_logf_restatement_all_positive_floats_strided():
    from os1_amd import api
    assert api.logf_host_mismatches(0x00000000, 0x7f800000, 97) == 0  # zero .. inf, every 97th pattern


def test_logf_restatement_special_values():
    from os1_amd import api
    assert api.logf_host_mismatches(0x00000000, 0x00000000) == 0     # -inf
    assert api.logf_host_mismatches(0x00000001, 0x007fffff) == 0     # every subnormal
    assert api.logf_host_mismatches(0x3f800000, 0x3f800000) == 0     # log(1) = +0
    assert api.logf_host_mismatches(0x7f800000, 0x7f800000) == 0     # inf


def test_reference_projection_builds_and_predicts_levels(tmp_path):
    """the reference restatement on the ulp-sensitive case: seen from where it was made, a MapPoint's predicted level is the
    level its mfMaxDistance was made with, whenever libm's logf makes it so"""
    L = U.build_ref(tmp_path)
    W, H = 1920, 1080
    cam = U.camera(W, H)
    sf = np.array([1.2 ** i for i in range(8)], np.float32)
    for i in range(1, 8):
        sf[i] = np.float32(sf[i - 1] * np.float32(1.2))
    mp = U.edge_points(cam, (0.0, W, 0.0, H), sf)
    n = len(mp['pos'])
    r = U.ref_project(L, mp, np.arange(n, dtype=np.int32), np.zeros(n, np.uint8), cam, (0.0, W, 0.0, H))
    lv = r['level'][-8:]
    ratio = mp['max'][-8:] / np.float32(10.0)                        # dist = 10 exactly
    want = [int(np.ceil(U.logf(ratio[i]) / U.logf(1.2))) for i in range(8)]
    assert r['in_view'][-8:].all() and list(lv) == want
    assert all(lv[i] in (i, i + 1) for i in range(8))
    # where a one-ulp error of the log would move the level: the quotient lands within a few ulps of an integer
    q = np.array([U.logf(ratio[i]) / U.logf(1.2) for i in range(8)], np.float32)
    assert (np.abs(q - np.round(q)) < 1e-5).all()
    assert r['in_view'][0] == 0 and r['in_view'][1] == 0           # behind the camera


def test_search_local_points_facade_compiles_and_links(tmp_path):
    exe = F.compile_test(str(tmp_path / 'local_map_test'))
    import os
    assert os.path.exists(exe)
