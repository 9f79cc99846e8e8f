"""-m gpu: the crafted boundary scenes of tests/bow_boundary_util.py through every call form that admits hand-written rows --
host arrays on the default route ('host'), the upload route (ORBFE_BOW_ZEROCOPY=0, 'upload'), as the middle member of a
three-keyframe search_by_bow_batch call ('batch') and, for the two SearchByBoW kinds, with the descriptor rows of side 1, of
side 2 or of both read from a resident frame built from the same host rows ('res1', 'res2', 'res12'; a scene with an empty side
has no resident form for it: a frame of no keypoints has no rows).  SearchForTriangulation takes host arrays only, so 'tri' scenes run
'host' and 'upload'.  Every result equals BOTH the hand-stated expectation and the CPU oracle's, bit for bit; a failure names
the boundary."""
import numpy as np
import pytest

from bow_boundary_util import BY_NAME, SCENES, companions, expected, merge_batch, overflow_inp, run
from search_boundary_util import make_kps

pytestmark = pytest.mark.gpu

ORBFE_ERR_OVERFLOW = -5
CASES = [(s, f) for s in SCENES for f in ('host', 'upload')]
CASES += [(s, 'batch') for s in SCENES if s.kind != 'tri']
CASES += [(s, f) for s in SCENES if s.kind != 'tri' for f, need in (('res1', ('desc1',)), ('res2', ('desc2',)), ('res12', ('desc1', 'desc2')))
          if all(len(s.inp[k]) for k in need)]
BOUNDS = (0.0, 640.0, 0.0, 480.0)


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def matcher(api):
    return api.Matcher()


_oracle_result = {}


def _batch(matcher, kind, members):
    """[(nmatches, matches12 with side-2 indices relative to the member's own side 2)] of the members searched in ONE call."""
    sides, d2, a2, v2, fv2, base = merge_batch(kind, members)
    i = members[0]
    got = matcher.search_by_bow_batch(sides, d2, a2, v2, fv2, i['ratio'], i['ori'], kind == 'kf_kf')
    out = []
    for (n, m), b, mem in zip(got, base, members):
        m = np.asarray(m, np.int64)
        assert ((m < 0) | ((m >= b) & (m < b + len(mem['desc2'])))).all(), 'a match outside the member\'s own side 2'
        out.append((int(n), [int(v) - b if v >= 0 else -1 for v in m]))
    return out


@pytest.mark.parametrize('scene,form', CASES, ids=['%s-%s' % (s.name, f) for s, f in CASES])
def test_boundary(scene, form, api, matcher, oracle, monkeypatch):
    if scene.name not in _oracle_result:
        _oracle_result[scene.name] = run(scene, oracle)
    want = expected(scene)
    assert _oracle_result[scene.name] == want
    i = scene.inp
    if form == 'upload':
        monkeypatch.setenv('ORBFE_BOW_ZEROCOPY', '0')
    if form in ('host', 'upload'):
        assert run(scene, matcher) == want
        return
    if form == 'batch':
        (ca, ea), (cb, eb) = companions(scene.kind)
        for c in (ca, cb):
            c['ratio'], c['ori'] = i['ratio'], i['ori']
        got = _batch(matcher, scene.kind, [ca, i, cb])
        assert got[1] == want and got[0] == ea and got[2] == eb
        return
    frames = {k: api.Frame.from_host(matcher, make_kps([(1.0, 1.0, 0)] * len(i[k])), i[k], BOUNDS)
              for k in (('desc1',) if form == 'res1' else ('desc2',) if form == 'res2' else ('desc1', 'desc2'))}
    try:
        got = run(scene, matcher, desc1=frames['desc1'].descriptors_device() if 'desc1' in frames else None,
                  desc2=frames['desc2'].descriptors_device() if 'desc2' in frames else None)
        assert got == want
    finally:
        for f in frames.values():
            f.close()


LARGE = ['claimed_was_best_in_257x257_kff', 'claimed_was_second_in_300x2049_kfk', 'conflict_earlier_accepts_one_group_kff',
         'topk_seven_taken_ratio_decided_by_the_eighth_other_group_kfk', 'claimed_was_tie_in_front_in_12289x257_kff']
OTHERS = {'kf_frame': ['claimed_was_irrelevant_kff', 'many_common_nodes_kff'], 'kf_kf': ['invalid_candidate_not_second_kfk', 'claims_chain_of_three_kfk']}


@pytest.mark.parametrize('name', LARGE)
@pytest.mark.parametrize('position', [0, 1, 2])
def test_large_node_scene_as_each_keyframe_of_a_batch(name, position, matcher):
    """The large route's matches12 index carries base1: the same large-node scene as keyframe 0, 1 and 2 of a three-keyframe call; the other
    two keyframes are different (small) scenes with their own hand-stated expectations.  All at ratio 0.7, orientation check off."""
    members = [BY_NAME[n] for n in OTHERS[BY_NAME[name].kind]]
    members.insert(position, BY_NAME[name])
    assert all(m.inp['ratio'] == 0.7 and not m.inp['ori'] for m in members)
    assert _batch(matcher, members[0].kind, [m.inp for m in members]) == [expected(m) for m in members]


@pytest.mark.parametrize('kind', ['kf_frame', 'kf_kf', 'tri'])
def test_node_of_65536_features_is_refused_and_the_matcher_stays_usable(kind, api, matcher):
    inp = overflow_inp(kind)
    s = BY_NAME['th_low_0_in_%s_lone' % {'kf_frame': 'kff', 'kf_kf': 'kfk', 'tri': 'tri'}[kind]]
    probe = type(s)('overflow', 'G', kind, inp, (0, {}), None)
    with pytest.raises(api.OrbfeError) as e:
        run(probe, matcher)
    assert e.value.code == ORBFE_ERR_OVERFLOW
    assert run(s, matcher) == expected(s)
