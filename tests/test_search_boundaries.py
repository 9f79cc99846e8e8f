"""Decision boundaries of the windowed searches on crafted frames (tests/search_boundary_util.py), on the CPU: every scene's
witness holds -- the scene really sits on the boundary its name states -- and the oracle gives the hand-stated result.  The GPU
counterpart is tests/test_gpu_search_boundaries.py; both compare for equality only."""
import pytest

from search_boundary_util import RATIO_CASES, SCENES, chi2_cases, chi2_product_cases, expected, ratio_differs_in_double, ratio_product_is_exact_tie, run


@pytest.mark.parametrize('scene', SCENES, ids=lambda s: s.name)
def test_witness(scene):
    assert bool(scene.witness()) is True


@pytest.mark.parametrize('scene', SCENES, ids=lambda s: s.name)
def test_oracle_gives_the_hand_stated_result(scene, oracle):
    assert run(scene, oracle) == expected(scene)


def test_scene_set_is_complete():
    fam = {f: [s for s in SCENES if s.family == f] for f in 'ABCDEFG'}
    assert all(len(v) >= 8 for v in fam.values())
    assert len({s.name for s in SCENES}) == len(SCENES)
    # sizes stay small: a frame of at most about 300 keypoints, a call of at most a few hundred queries
    for s in SCENES:
        i = s.inp
        assert len(i.get('kps', i.get('kps2', []))) <= 300
        assert len(i.get('qdesc', i.get('desc1', []))) <= 300
    # 0.6f * 5 and 0.8f * 125 are round-to-even ties that land on 3 / 100; 0.9f * 10 and 0.9f * 100 round up onto 9 / 90, and a
    # comparison widened to double sees them below
    assert ratio_product_is_exact_tie(0.6, 3, 5) and ratio_product_is_exact_tie(0.8, 100, 125)
    assert ratio_differs_in_double(0.9, 9, 10) and ratio_differs_in_double(0.9, 90, 100)
    assert len(RATIO_CASES) == 13
    c = chi2_cases()
    assert sum(1 for x in c if x[3]) >= 2 and sum(1 for x in c if not x[3]) >= 2
    assert len(chi2_product_cases()) >= 2
