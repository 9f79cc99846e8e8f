"""The source projection (orbfe_project_sources / orbfe_search_by_projection_sources_frame) without a GPU: the reference
restatement tests/cpp/project_sources_ref.cpp is pinned to the oracle's whole-function restatements orc_sbp_frame /
orc_sbp_keyframe (src/ORBmatcher.cc:1292-1552), the C++ facade test compiles and links, the library exports the calls.
The fused cases of tests/test_gpu_source_projection.py are run here on the CPU (oracle extractor, restatement, oracle
search) so that the conditions they assert on the oracle's output are known to hold before a GPU is involved."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import source_projection_util as S


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp('spref'))


@pytest.fixture(scope='module')
def oracle():
    from oracle.pyoracle import Oracle
    o = Oracle()
    S.bind_oracle(o)
    return o


_FRAMES = {}


def _frames(W, H, nfeat):
    if (W, H, nfeat) not in _FRAMES:
        _FRAMES[(W, H, nfeat)] = S.frames(W, H, nfeat)
    return _FRAMES[(W, H, nfeat)]


@pytest.mark.parametrize('W,H,nfeat', [(1920, 1080, 2000), (640, 480, 500)])
@pytest.mark.parametrize('mode', [S.LAST_FRAME, S.KEYFRAME])
def test_restatement_and_array_search_reproduce_whole_function_oracle(ref, oracle, mode, W, H, nfeat):
    kA, dA, kB, dB, sf = _frames(W, H, nfeat)
    info = dict(pruned=0)
    for th, max_dist in S.CASES[mode]:
        for check_ori in (True, False):
            sc = S.scene(kA, dA, kB, sf, W, H, seed=S.case_seed(mode, th, W))
            want = S.checked_oracle_case(ref, oracle, sc, mode, kA, kB, dB, sf, th, max_dist, check_ori, W, info)
            # the restatement's sources through the oracle's array-form search: the same keypoints, the same count
            proj = want['proj']
            n2, a2 = oracle.search_by_projection_uv(kB, dB, sc['bounds'], sf, sc['st']['occ'], proj['uv'], proj['level'], kA['angle'],
                                                    want['flags'], proj['valid'], sc['tab']['desc'][sc['rows']], th, max_dist,
                                                    mode == S.KEYFRAME, check_ori)
            assert n2 == want['nmatches']
            assert (S.cur_mp_from_assigned(want['before'], a2, sc['rows']) == want['cur_mp']).all()
    assert info['pruned'] > 0   # the rotation check cleared a slot in at least one case of this mode


def test_edge_sources_behind_the_camera(ref):
    """the projection test's scene holds a point behind the camera that LAST_FRAME rejects and KEYFRAME keeps"""
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(W, H, 2000)
    sc, edge = S.edge_sources(S.scene(kA, dA, kB, sf, W, H, seed=5), sf)
    S.assert_edges(ref, sc, edge, kA, sf)


def test_facade_test_compiles_and_links(tmp_path):
    import source_projection_facade as F
    exe = F.compile_test(str(tmp_path / 'source_projection_test'))
    assert os.path.exists(exe)


def test_library_exports_the_calls_with_the_documented_arguments():
    from os1_amd import api
    L = api.load_library()
    assert len(L.orbfe_project_sources.argtypes) == 13
    assert len(L.orbfe_search_by_projection_sources_frame.argtypes) == 21
    # the same counts in the header's declarations
    hdr = open(os.path.join(S.ROOT, 'include', 'orbfe.h')).read()
    for name, n in (('orbfe_project_sources', 13), ('orbfe_search_by_projection_sources_frame', 21)):
        m = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert m and len(m.group(1).split(',')) == n
    assert isinstance(L.orbfe_project_sources, C._CFuncPtr)
    assert api.SRC_LAST_FRAME == 0 and api.SRC_KEYFRAME == 1
