"""-m gpu: the crafted boundary scenes of tests/search_boundary_util.py through every call form that admits hand-written
keypoints -- host arrays, a resident frame built from host arrays, the marshalled upload route (ORBFE_FRAME_ZEROCOPY=0),
page-locked query arrays (one scene per family) and, for the list-length family, the switches of the bookkeeping kernel.
Every result equals BOTH the hand-stated expectation and the CPU oracle's, bit for bit; a failure names the boundary."""
import pytest

from search_boundary_util import BY_NAME, SCENES, expected, run

pytestmark = pytest.mark.gpu

FRAME_KINDS = ('mp', 'uv', 'proj')
PINNED = ['edge_abs_dx_eq_r_is_out_mp', 'column_run_65_proj', 'list_length_0_to_8_chain_by_claim_proj', 'tie_three_first_in_grid_order_uv',
          'ratio_0p6_3_5_same_level', 'viewcos_at_float_0p998_radius_2p5', 'histogram_30_3_keeps_small_uv']
CASES = [(s, 'host') for s in SCENES]
CASES += [(s, f) for s in SCENES if s.kind in FRAME_KINDS for f in ('frame', 'upload')]
CASES += [(BY_NAME[n], 'pinned') for n in PINNED]
CASES += [(s, f) for s in SCENES if s.family == 'C' for f in ('generic', 'one_round')]


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def matcher(api):
    return api.Matcher()


_oracle_result = {}


@pytest.mark.parametrize('scene,form', CASES, ids=['%s-%s' % (s.name, f) for s, f in CASES])
def test_boundary(scene, form, api, matcher, oracle, monkeypatch):
    if scene.name not in _oracle_result:
        _oracle_result[scene.name] = run(scene, oracle)
    want = expected(scene)
    assert _oracle_result[scene.name] == want
    first, pin, keep = None, None, []
    if form == 'upload':                       # before the frame is built: the switch selects the frame's build route as well
        monkeypatch.setenv('ORBFE_FRAME_ZEROCOPY', '0')
    if form != 'host':
        first = api.Frame.from_host(matcher, scene.inp['kps'], scene.inp['desc'], scene.inp['bounds'])
    if form == 'generic':
        monkeypatch.setenv('ORBFE_RESOLVE_GENERIC', '1')
    elif form == 'one_round':
        monkeypatch.setenv('ORBFE_RESOLVE_MAX_ROUNDS', '1')
    elif form == 'pinned':
        def pin(a):
            p = api.PinnedArray(a.shape, a.dtype)
            p.a[...] = a
            keep.append(p)
            return p.a
    got = run(scene, matcher, first, pin)
    assert got == want
    if scene.kind in FRAME_KINDS and len(scene.inp['qdesc']) and len(scene.inp['kps']):
        # tables of the bookkeeping kernel: in LDS (these problems are tiny) unless the switch sends them to global scratch
        assert matcher.resolve_route() == (0 if form == 'generic' else 2)
        if scene.family == 'C' and 'chain' in scene.name:
            # every cluster is a chain of queries that lose their best keypoint to an earlier one: never settled in one round
            assert matcher.resolve_rounds() == -1 if form == 'one_round' else matcher.resolve_rounds() >= 3
    if first is not None:
        first.close()
