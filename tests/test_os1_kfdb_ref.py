"""The keyframe database's decision logic pinned to the reference's own compiled src/KeyFrameDatabase.cc (oracle/_ref/libos1_kfdb.so,
built by oracle/Makefile where the reference exists; oracle/os1_kfdb_wrap.cpp).  For every scene -- the seeded ones and the crafted
decision-boundary families A to F of tests/kfdb_util.py -- and every step: the reference object == tests/cpp/kfdb_ref.cpp == the
Python restatement, on the candidate list and on all six members of every keyframe (score bits as uint32).  Every comparison is
exact.  Where the library is absent the same assertions run against the recorded results of tests/golden/os1_kfdb_outputs.npz
(tools/gen_os1_kfdb_golden.py); where both exist the recording is held to the library.

Each crafted scene carries a literal expectation written from the reference text, and a witness: the Python restatement with the
scene's named comparison flipped must not reproduce the scene."""
import numpy as np
import pytest

import kfdb_util as K

F32 = np.float32
ALL = list(K.every_scene())
CRAFTED = list(K.crafted())


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kfdbref'))


def _reference(name):
    """(results, members) of the reference's object code: computed now where the library is built, else the recording"""
    if K.have_os1():
        ref = K.os1_ref(K.every_scene()[name])
        out = K.trace(ref, K.every_scene()[name])
        ref.close()
        return out
    return K.golden()[name]


def test_reference_source():
    print('\nos1 kfdb reference: %s' % ('oracle/_ref/libos1_kfdb.so' if K.have_os1() else 'tests/golden/os1_kfdb_outputs.npz'))
    g = K.golden()
    assert g is not None, 'tests/golden/os1_kfdb_outputs.npz is missing: run tools/gen_os1_kfdb_golden.py'
    assert sorted(g) == sorted(ALL)
    if K.have_os1():
        rec = K.golden_records()
        z = np.load(K.GOLDEN)
        assert set(rec) == set(z.files) and all(rec[k].tobytes() == z[k].tobytes() and rec[k].dtype == z[k].dtype for k in rec), \
            'the golden is stale: run tools/gen_os1_kfdb_golden.py'


@pytest.mark.parametrize('name', ALL)
def test_reference_object_equals_both_restatements(lib, name):
    scene = K.every_scene()[name]
    want_res, want_mem = _reference(name)
    assert (want_res, want_mem) == K.golden()[name]
    assert len(want_res) == len(scene['steps'])
    ref, py = K.Ref(lib, scene), K.PyRef(scene)
    for i, st in enumerate(scene['steps']):
        a, b = ref.step(st), py.step(st)
        assert a == want_res[i] and b == want_res[i], (name, i, st[0], a, b, want_res[i])
        assert ref.members() == want_mem[i], (name, i, st[0], 'kfdb_ref.cpp')
        assert py.members() == want_mem[i], (name, i, st[0], 'PyRef')
    ref.close()
    assert any(r for r in want_res if r is not None) or name in ('max5', 'max10'), 'a scene in which no query returns anything'


@pytest.mark.parametrize('name', CRAFTED)
def test_crafted_scene_literal_and_witness(name):
    scene = K.crafted()[name]
    res, mem = _reference(name)
    assert [r for r in res if r is not None] == scene['literal']
    assert scene['witness'] or name == 'A_maxc01'        # maxCommonWords 1: minCommonWords 0, nobody is listed with 0 words
    for w in scene['witness']:
        got = K.trace(K.PyRef(scene, flip=[w]), scene)
        assert got != (res, mem), '%s: flipping %s changes nothing' % (name, w)
    assert scene['n_words'] <= 1000 and len(scene['kfs']) <= 32 and all(len(k['words']) <= 64 for k in scene['kfs'])
    for k in scene['kfs']:       # dyadic, not normalised: every value is a multiple of 2^-25 below 2
        v = k['values'] * 2.0 ** 25
        assert (v == np.rint(v)).all() and (np.abs(k['values']) <= 1).all()


def test_min_common_words_is_an_integer_or_truncates():
    """int minCommonWords = maxCommonWords*0.8f for maxCommonWords 1..40, from the reference's members: the keyframe with exactly
    minCommonWords words is listed and NOT scored, the one with one more is scored."""
    integer = []
    for maxc in K.MAXC_RANGE:
        scene = K.crafted()['A_maxc%02d' % maxc]
        nm = scene['named']
        prod = F32(maxc) * F32(0.8)
        assert nm['minc'] == int(prod) == (4 * maxc) // 5
        if float(prod) == int(prod):
            integer.append(maxc)
        res, mem = _reference('A_maxc%02d' % maxc)
        for step, (wi, si) in ((-2, (4, 5)), (-1, (1, 2))):          # after the relocalisation step, after the loop step
            m = mem[step]
            assert m[nm['at_max']][wi] == maxc and m[nm['at_max']][si] == int(F32(maxc / 64.0).view(np.uint32))
            if nm['at_min'] is not None:
                assert m[nm['at_min']][wi] == nm['minc'] and m[nm['at_min']][si] == 0
            if nm['above_min'] is not None:
                assert m[nm['above_min']][wi] == nm['minc'] + 1 and m[nm['above_min']][si] == int(F32((nm['minc'] + 1) / 64.0).view(np.uint32))
    # the float product is an integer exactly for the multiples of 5; every other maxc truncates
    assert integer == [m for m in K.MAXC_RANGE if m % 5 == 0]


def test_boundary_values_are_what_the_scenes_say():
    assert F32(0.75) * F32(0.5) == F32(0.375)
    assert F32(0.75) * K.ulps(0.5, 1) == K.ulps(0.375, 2) and 0.75 * float(K.ulps(0.5, 1)) < float(K.ulps(0.375, 2))   # the tie rounds up
    assert F32(F32(0.5) + F32(2.0 ** -25)) == F32(0.5) and F32(F32(2.0 ** -25) + F32(2.0 ** -25)) + F32(0.5) == K.ulps(0.5, 1)
    sc = K.crafted()['B_min_score']
    assert [float(st[2]) for st in sc['steps'] if st[0] == 'loop'] == [float(sc['named']['s']), float(K.ulps(sc['named']['s'], 1)),
                                                                      float(K.ulps(sc['named']['s'], -1))]
