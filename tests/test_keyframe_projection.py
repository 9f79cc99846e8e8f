"""The keyframe projection (orbfe_project_keyframe / orbfe_search_projected_keyframe_frame) without a GPU: the reference
restatement tests/cpp/project_keyframe_ref.cpp is pinned to the oracle's whole-function restatements orc_sbp_scw / orc_fuse /
orc_fuse_scw / orc_search_by_sim3 (src/ORBmatcher.cc:285-398, 806-1290) -- restatement, then the oracle's array-form search,
then each function's bookkeeping replay reproduce the return value and every output array exactly -- the C++ facade test
compiles and links, the library exports the calls.  The fused cases of tests/test_gpu_keyframe_projection.py are run here on
the CPU so that the conditions they rely on are known to hold on the oracle's output before a GPU is involved."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keyframe_projection_util as K


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kpref'))


@pytest.fixture(scope='module')
def oracle():
    from oracle.pyoracle import Oracle
    o = Oracle()
    K.bind_oracle(o)
    return o


_FRAMES = {}


def _frames(W, H, nfeat):
    if (W, H, nfeat) not in _FRAMES:
        _FRAMES[(W, H, nfeat)] = K.SP.frames(W, H, nfeat)
    return _FRAMES[(W, H, nfeat)]


@pytest.mark.parametrize('W,H,nfeat', [(1920, 1080, 2000), (640, 480, 500)])
@pytest.mark.parametrize('fn', K.FUNCS)
def test_restatement_search_and_replay_reproduce_whole_function_oracle(ref, oracle, fn, W, H, nfeat):
    kA, dA, kB, dB, sf = _frames(W, H, nfeat)
    info = {}
    for th in K.CASES[fn]:
        sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=K.case_seed(fn, th, W))
        K.checked_oracle_case(ref, oracle, fn, sc, th, kA, dA, kB, dB, sf, W, info)
    K.assert_branches(fn, info)


def test_every_th_of_the_issue_occurs_and_the_sim3_scale_is_not_one():
    assert {float(t) for ths in K.CASES.values() for t in ths} == {3.0, 4.0, 7.5, 10.0}
    assert K.SIM3_SCALE != 1 and K.SCW_SCALE != 1


def test_edge_points(ref):
    W, H = 1920, 1080
    sf = _frames(W, H, 2000)[4]
    cam = K.U.camera(W, H)
    Kc = np.float32([cam['fx'], cam['fy'], cam['cx'], cam['cy'], cam['lsf']])
    bounds = (0.0, float(W), 0.0, float(H))
    tab, names = K.edge_points(bounds, Kc, sf)
    out = K.assert_edges(ref, tab, names, bounds, Kc, sf)
    # the float and the double form of invz give the same projection of every edge point ...
    K.check_projection(out[False], out[True])


def test_float_and_double_invz_are_the_same_function():
    """The reference spells invz as a float division in SearchByProjection(Scw) and Fuse and as a double division rounded to
    float in Fuse(Scw) and SearchBySim3, and kernel and restatement keep both spellings.  No input tells them apart: a double
    carries 53 >= 2*24 + 2 bits, so rounding the double quotient to float is the correctly rounded float quotient (double
    rounding is innocuous for division at these widths).  The search below covers every mantissa; it finds no z, so this test
    asserts the count is 0 where a differing z had been expected."""
    assert K.invz_forms_differ() == 0


def test_facade_test_compiles_and_links(tmp_path):
    import keyframe_projection_facade as F
    exe = F.compile_test(str(tmp_path / 'keyframe_projection_test'))
    assert os.path.exists(exe)


def test_library_exports_the_calls_with_the_documented_arguments():
    from os1_amd import api
    L = api.load_library()
    assert len(L.orbfe_project_keyframe.argtypes) == 15
    assert len(L.orbfe_search_projected_keyframe_frame.argtypes) == 22
    hdr = open(os.path.join(K.ROOT, 'include', 'orbfe.h')).read()
    for name, n in (('orbfe_project_keyframe', 15), ('orbfe_search_projected_keyframe_frame', 22)):
        m = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert m and len(m.group(1).split(',')) == n
    assert isinstance(L.orbfe_project_keyframe, C._CFuncPtr)
    # the Python struct has the header's fields, in order
    m = re.search(r'typedef struct OrbfeKeyFrameProjection \{(.*?)\} OrbfeKeyFrameProjection;', hdr, re.S)
    fields = [f.strip().split('[')[0] for decl in re.findall(r'(?:float|int) ([^;]*);', m.group(1)) for f in decl.split(',')]
    assert fields == [f[0] for f in api.KeyFrameProjection._fields_]
    assert C.sizeof(api.KeyFrameProjection) == 4 * (9 + 3 + 1 + 9 + 3 + 3 + 4 + 1 + 3)
