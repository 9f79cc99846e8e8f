"""Decision boundaries of the vocabulary-guided searches on crafted feature sets (tests/bow_boundary_util.py), on the CPU: every
scene's witness holds -- the scene really sits on the boundary its name states --, the oracle gives the hand-stated result, and
the constants the scenes of family G are sized to are the ones in os1_amd/csrc/orbfe_bow.hip.  The GPU counterpart is
tests/test_gpu_bow_boundaries.py; both compare for equality only."""
import os
import re

import pytest

from bow_boundary_util import (CONSTANTS, SCENES, epipole_fma_cases, expected, line_fma_cases, line_general_cases, line_t_cases, ratio_float_pairs,
                               run)


@pytest.mark.parametrize('scene', SCENES, ids=lambda s: s.name)
def test_witness(scene):
    assert bool(scene.witness()) is True


@pytest.mark.parametrize('scene', SCENES, ids=lambda s: s.name)
def test_oracle_gives_the_hand_stated_result(scene, oracle):
    assert run(scene, oracle) == expected(scene)


def test_constants_are_the_kernel_files():
    """A retuned constant asks for retuned scenes: the sizes of family G are stated against these values."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'os1_amd', 'csrc', 'orbfe_bow.hip')).read()
    for name, want in CONSTANTS.items():
        m = re.findall(r'constexpr\s+int\s+(?:[A-Za-z_0-9]+\s*=\s*[0-9]+\s*,\s*)*%s\s*=\s*([0-9]+)' % name, src)
        assert m == [str(want)], (name, m)


def test_scene_set_is_complete():
    assert len({s.name for s in SCENES}) == len(SCENES)
    fam = {f: [s for s in SCENES if s.family == f] for f in 'ABCDEFG'}
    assert all(len(v) >= 20 for v in fam.values())
    for f in 'ABCDFG':
        assert {s.kind for s in fam[f]} == {'kf_frame', 'kf_kf', 'tri'}
    p = ratio_float_pairs()
    assert len(p['i']) == 25 and p['ii'] == []
    assert [c[1] for c in line_t_cases()] == [0, 5, 7]
    assert len(line_general_cases()) >= 2
    assert len(line_fma_cases('num')) >= 2 and len(line_fma_cases('den')) >= 2 and len(line_fma_cases('abc')) >= 1
    assert len(epipole_fma_cases()) >= 2
