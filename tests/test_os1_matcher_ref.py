"""The twelve ORBmatcher members pinned to the reference's own compiled src/ORBmatcher.cc (oracle/_ref/libos1_matcher.so, built by
oracle/Makefile where the reference exists; tests/os1_matcher_ref_util.py).  For every scene three results are compared and every
field must be equal -- integers, index arrays, float bits: the reference object's, the oracle's restatement's and, where the scene
has one, its hand-stated literal.  Where the library is absent the same assertions run against the recorded results of
tests/golden/os1_matcher_outputs.npz (tools/gen_os1_matcher_golden.py); where both exist the golden is held to the library.

A disagreement in the arithmetic tests below is a defect of the cv::Mat stand-in, not a finding about the searches."""
import numpy as np
import pytest

import bow_boundary_util as BB
import keyframe_projection_util as KP
import os1_matcher_ref_util as R
import search_boundary_util as SB
import source_projection_util as SP

UNMAPPABLE_REASONS = ('outside the image bounds', 'outside the pyramid', 'max_dist !=', 'max_dist >= 256', 'two radii on one level', 'skipped but not claimed',
                      'claim and gate together', 'an empty side', 'two queries end on one keypoint', 'a gate other than')


@pytest.fixture(scope='module')
def kp_L(tmp_path_factory):
    return KP.build_ref(tmp_path_factory.mktemp('os1_ref_kp'))


@pytest.fixture(scope='module')
def ref(oracle):
    SP.bind_oracle(oracle)
    KP.bind_oracle(oracle)
    be = R.RefBackend(oracle) if R.have_lib() else None
    print('\nos1 matcher reference: %s' % ('oracle/_ref/libos1_matcher.so' if be else 'tests/golden/os1_matcher_outputs.npz'))
    assert be is not None or R.golden() is not None, 'neither oracle/_ref/libos1_matcher.so nor tests/golden/os1_matcher_outputs.npz'
    return be


@pytest.fixture(scope='module')
def reg(kp_L):
    return dict(R.registry(kp_L))


def reference_result(key, runner, ref):
    """the reference's result of a scene: the library's (held against the golden where both exist) or the golden's"""
    g = R.golden()
    if ref is None:
        assert g is not None and key in g, 'no recorded result for %s' % key
        return g[key]
    got = runner(ref, R.Whole(ref.L))
    if g is not None:
        assert key in g, 'the golden has no %s: run tools/gen_os1_matcher_golden.py' % key
        assert R.same(got, g[key]), 'golden and library differ on %s: %s' % (key, R.diff(got, g[key]))
    return got


KEYS = [k for k, _ in R.registry()]


@pytest.mark.parametrize('key', KEYS)
def test_reference_oracle_and_literal_agree(key, reg, ref, oracle):
    runner = reg[key]
    whole = R.Whole(oracle.L)
    try:
        orc = runner(oracle, whole)
    except R.Unmappable as e:
        # no member expresses this array-form scene; its literal stays held to the array form (tests/test_search_boundaries.py)
        assert key.startswith('b:') and any(r in str(e) for r in UNMAPPABLE_REASONS), str(e)
        s = SB.BY_NAME[key[2:]]
        assert s.kind in ('uv', 'proj') and SB.run(s, oracle) == SB.expected(s)
        g = R.golden()
        assert g is None or (key not in g and key in R.golden_unmapped())
        return
    want = reference_result(key, runner, ref)
    assert R.same(orc, want), 'oracle and reference differ on %s: %s' % (key, R.diff(orc, want))
    if key.startswith('b:'):
        name = key[2:]
        s = SB.BY_NAME.get(name) or BB.BY_NAME[name]
        lit = R.boundary_result(s, (SB.expected if isinstance(s, SB.Scene) else BB.expected)(s))
        have = {k: want[k] for k in lit}
        assert R.same(have, lit), 'literal and reference differ on %s: %s' % (key, R.diff(have, lit))
        assert s.witness()


def test_scene_counts(reg, oracle):
    """what the registry holds, and how many of the array-form scenes a whole member expresses"""
    whole = R.Whole(oracle.L)
    n = dict(mapped=0, unmapped=0)
    for s in SB.SCENES:
        if s.kind in ('uv', 'proj'):
            try:
                R.run_boundary(s, oracle, whole)
                n['mapped'] += 1
            except R.Unmappable:
                n['unmapped'] += 1
    kinds = {}
    for s in R.BOUNDARY:
        kinds[s.kind] = kinds.get(s.kind, 0) + 1
    print('\nboundary scenes by kind: %s; uv / proj expressed by a member: %d, not: %d; other scenes: %d' %
          (kinds, n['mapped'], n['unmapped'], len(reg) - len(R.BOUNDARY)))
    assert n['mapped'] > 0 and set(kinds) == {'mp', 'uv', 'proj', 'init', 'kf_frame', 'kf_kf', 'tri'}
    assert len(R.KP_CASES) == 8 and len(R.SP_CASES) == 5 and len(R.EDGE_CASES) == 4 and len(R.SIM3_TH_HIGH) == 6


def test_seeded_scenes_are_not_vacuous(reg, oracle):
    for key, runner in reg.items():
        if key.split(':')[0] not in ('sp', 'kp', 'mp', 'init'):
            continue
        r = runner(oracle, None)
        n = int(r['n'] if 'n' in r else r['ret'])
        assert n >= 10, (key, n)
    i = R.init_seeded()
    assert len(i['kps1']) == 300
    sb = R.sp_scene(SP.LAST_FRAME, 2151, False)['st']
    assert sb['occ'].any() and sb['bad'].any() and sb['already'].any() and (sb['nObs'] == 0).any()


# ---- the literals of the scenes that have no boundary-scene literal ---------------------------------------------------------------
@pytest.mark.parametrize('d1,d2,found', R.SIM3_TH_HIGH)
def test_search_by_sim3_accepts_at_th_high_in_both_directions(d1, d2, found, reg, ref):
    """`bestDist<=TH_HIGH` at src/ORBmatcher.cc:1185 (keyframe 1 -> 2) and :1265 (2 -> 1): 100 is accepted, 101 is not, and a match needs both"""
    key = 'sim3_th_high:%d:%d' % (d1, d2)
    want = reference_result(key, reg[key], ref)
    assert SB.hamming(SB.row(d1), SB.row(0)) == d1 and SB.hamming(SB.row(d2), SB.row(0)) == d2
    assert int(want['ret']) == found and [int(v) for v in want['m12']] == ([1] if found else [-1])


def test_edge_points_land_on_the_side_the_reference_text_puts_them(reg, ref):
    """Fuse(KeyFrame, Scw) on the edge scene: a candidate that passes every test ends with an observation (idx >= 0) or, where its
    keypoint holds a MapPoint, in vpReplacePoint.  Stated from the text: depth `<0.0f` (:979) with z = +-0 projecting to nothing finite,
    IsInImage half-open (KeyFrame.cc:678-681), `dist3D<minDistance || dist3D>maxDistance` (:1000), `PO.dot(Pn)<0.5*dist3D` (:1006)."""
    S, case = R.edge_case(KP.FUSE_SCW, 4.0)
    want = reference_result('edge:' + KP.FUSE_SCW, reg['edge:' + KP.FUSE_SCW], ref)
    E, names = S['E'], S['names']
    rep = {int(p): int(r) for p, r in zip(case['points'], want['replace'])}
    passed = {n for n, i in names.items() if want['idx'][i] >= 0 or rep.get(i, -1) >= 0}
    expect = {'u_minX', 'v_minY', 'dist_on_max', 'dist_on_min', 'dot_on_half', 'invz_probe'} | {'level_%d' % l for l in range(8) if l != 3}   # (level_3 is bad)
    assert passed == expect, sorted(passed ^ expect)
    twins = {n for n, i in names.items() if want['idx'][E + i] >= 0 or rep.get(E + i, -1) >= 0}
    assert twins == (expect | {'level_3'}) - {'level_5'}                               # (the twin of level_5 is bad)


def test_descriptor_distance_and_helper_literals(reg, ref):
    dd = reference_result('dd', reg['dd'], ref)
    tab, known, rnd = R.dd_pairs()
    assert [int(v) for v in dd['known']] == [abs(a - b) for a, b in known] == [int(v) for v in dd['known_rows']]
    pop = [int(np.unpackbits(np.bitwise_xor(rnd[i], rnd[i + 1])).sum()) for i in range(0, 200, 2)]
    assert [int(v) for v in dd['rnd']] == pop == [int(v) for v in dd['rnd_rows']] and pop[0] == 256
    h = reference_result('helpers', reg['helpers'], ref)
    assert np.asarray(h['radius'], np.int64).astype(np.uint32).view(np.float32).tolist() == [2.5, 4.0, 2.5, 2.5, 4.0, 4.0]
    assert [int(v) for v in h['maxima'][len(SB.HIST_COUNTS)]] == [-1, -1, -1]          # an empty histogram keeps nothing


def test_one_gemm_is_not_a_product_and_an_add(oracle):
    """the inputs of the arithmetic scene tell `A*b+c` as one gemm from a product followed by an add, and the transposed path from the
    plain one (else 'arith' could not tell a stand-in that got the form wrong)"""
    differ = sum(np.float32(np.float32(A[0, 0] * b[0] + A[0, 1] * b[1] + A[0, 2] * b[2]) + c[0]).tobytes() != oracle.cv_small('gemm', A, b, 1.0, c, 1.0)[:1].tobytes()
                 or oracle.cv_small('gemmT', A, b, -1.0).tobytes() != oracle.cv_small('gemm', np.ascontiguousarray(A.T), b, -1.0).tobytes()
                 for A, b, c in R.arith_inputs())
    assert differ >= 5
