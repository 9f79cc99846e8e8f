"""-m gpu: the HIP searches compared DIRECTLY with the reference's own compiled src/ORBmatcher.cc (oracle/_ref/libos1_matcher.so;
tests/os1_matcher_ref_util.py), field for field, with no oracle in between: the host-array forms and the resident-frame forms on
every boundary scene a member expresses, on 500 projected MapPoints (two 256-lane blocks, the second partial) and on the dense-tie
SearchForInitialization scene, and the fused projection+search forms (k_project_sources: search_by_projection_sources;
k_project_keyframe: search_projected_keyframe with the bookkeeping replay, also on edge MapPoints and on SearchBySim3's TH_HIGH; orbfe_search_local_points_frame) on the seeded scenes.
Where the library cannot be loaded the recorded results of tests/golden/os1_matcher_outputs.npz stand in; with neither, the module
fails.  It never skips, and prints once which of the two it compared against."""
import numpy as np
import pytest

import bow_boundary_util as BB
import keyframe_projection_util as KP
import local_map_util as U
import os1_matcher_ref_util as R
import search_boundary_util as SB
import source_projection_util as SP

pytestmark = pytest.mark.gpu

FRAME_KINDS = ('mp', 'uv', 'proj')
CASES = [(s, 'host') for s in R.BOUNDARY] + [(s, 'frame') for s in R.BOUNDARY if isinstance(s, SB.Scene) and s.kind in FRAME_KINDS]


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def matcher(api):
    m = api.Matcher(0)
    yield m
    m.close()


@pytest.fixture(scope='module')
def kp_L(tmp_path_factory):
    return KP.build_ref(tmp_path_factory.mktemp('os1_ref_kp_gpu'))


@pytest.fixture(scope='module')
def ref(oracle):
    SP.bind_oracle(oracle)
    KP.bind_oracle(oracle)
    be = None
    if R.have_lib():
        try:
            be = R.RefBackend(oracle)
        except OSError:
            be = None
    assert be is not None or R.golden() is not None, 'neither oracle/_ref/libos1_matcher.so nor tests/golden/os1_matcher_outputs.npz'
    print('\nos1 matcher reference on the GPU side: compared against %s' %
          ('the library oracle/_ref/libos1_matcher.so' if be else 'the golden tests/golden/os1_matcher_outputs.npz'))
    return be


@pytest.fixture(scope='module')
def reg(kp_L):
    return dict(R.registry(kp_L))


_want = {}


def reference(key, reg, ref):
    """the reference's result of a registry scene (library, else golden); None where no member expresses the scene"""
    if key not in _want:
        if ref is not None:
            try:
                _want[key] = reg[key](ref, R.Whole(ref.L))
            except R.Unmappable:
                _want[key] = None
        else:
            g = R.golden()
            assert key in g or key in R.golden_unmapped(), 'the golden has no %s: run tools/gen_os1_matcher_golden.py' % key
            _want[key] = g.get(key)
    return _want[key]


@pytest.mark.parametrize('scene,form', CASES, ids=['%s-%s' % (s.name, f) for s, f in CASES])
def test_boundary_scene_equals_the_reference_object(scene, form, api, matcher, reg, ref):
    run = SB.run if isinstance(scene, SB.Scene) else BB.run
    first = api.Frame.from_host(matcher, scene.inp['kps'], scene.inp['desc'], scene.inp['bounds']) if form == 'frame' else None
    try:
        res = run(scene, matcher, first) if first is not None else run(scene, matcher)
        got = R.boundary_result(scene, res)
        if getattr(scene, 'kind', '') == 'init':
            i = scene.inp
            got['prev'] = np.asarray(matcher.search_for_initialization(i['kps1'], i['desc1'], i['kps2'], i['desc2'], i['bounds'], i['prev'], i['window'],
                                                                       i['ratio'], i['ori'])[2], np.float32)
    finally:
        if first is not None:
            first.close()
    want = reference('b:' + scene.name, reg, ref)
    if want is None:      # an array-form scene no member expresses: the hand-stated literal is all there is to hold it to
        assert scene.kind in ('uv', 'proj')
        want = R.boundary_result(scene, SB.expected(scene))
    assert R.same(got, want), '%s (%s): %s' % (scene.name, form, R.diff(got, want))


@pytest.mark.parametrize('form', ['host', 'frame'])
def test_500_map_points_two_blocks(form, api, matcher, reg, ref):
    i = R.mp_seeded()
    assert len(i['level']) == 500
    first = api.Frame.from_host(matcher, i['kps'], i['desc'], i['bounds']) if form == 'frame' else i['kps']
    try:
        n, a = matcher.search_by_projection(first, i['desc'], i['bounds'], i['sf'], i['occ'], i['xy'], i['level'], i['viewcos'], i['flags'], i['qdesc'],
                                            i['th'], i['ratio'])
    finally:
        if form == 'frame':
            first.close()
    got = dict(n=np.int64(n), a=np.asarray(a, np.int64))
    want = reference('mp:seeded', reg, ref)
    assert R.same(got, want), R.diff(got, want)
    assert int(want['n']) > 50


def test_search_for_initialization_dense_ties(matcher, reg, ref):
    i = R.init_seeded()
    n, m, prev = matcher.search_for_initialization(i['kps1'], i['desc1'], i['kps2'], i['desc2'], i['bounds'], i['prev'], i['window'], i['ratio'], i['ori'])
    got = dict(n=np.int64(n), a=np.asarray(m, np.int64), prev=np.asarray(prev, np.float32))
    want = reference('init:seeded', reg, ref)
    assert R.same(got, want), R.diff(got, want)


def _table(api, matcher, tab):
    n = len(tab['pos'])
    lm = api.LocalMap(matcher, n)
    lm.set_rows(np.arange(n), tab['pos'], tab['normal'], tab['min'], tab['max'], tab['desc'])
    return lm


@pytest.mark.parametrize('mode,seed,th,max_dist,edges', R.SP_CASES)
def test_fused_source_projection_equals_the_reference_object(mode, seed, th, max_dist, edges, api, matcher, reg, ref):
    """k_project_sources + search (orbfe_search_by_projection_sources_frame) against SearchByProjection(Frame, Frame / KeyFrame)"""
    kA, dA, kB, dB, sf = R.frames()
    sc = R.sp_scene(mode, seed, edges)
    flags = SP.flags_of(sc, mode)
    if mode == SP.LAST_FRAME:
        flags[np.arange(sc['n']) % 17 == 3] |= SP.MP_SKIP          # mvbOutlier of run_sp
    src, cur = matcher.frame(kA, dA, sc['bounds']), matcher.frame(kB, dB, sc['bounds'])
    lm = _table(api, matcher, sc['tab'])
    try:
        got = matcher.search_by_projection_sources(cur, src, lm, U.api_camera(api, sc['cam']), mode, sc['rows'], flags, sc['st']['occ'], sf, th,
                                                   max_dist, True)
    finally:
        lm.close()
        cur.close()
        src.close()
    want = reference('sp:%d:%d:%g:%d:%d' % (mode, seed, th, max_dist, edges), reg, ref)
    before = np.where(sc['st']['occ'] != 0, len(sc['tab']['pos']), -1).astype(np.int64)       # an occupied keypoint holds the extra MapPoint (run_sp)
    have = dict(n=np.int64(got['nmatches']), before=before, cur=SP.cur_mp_from_assigned(before, got['kp_assigned'], sc['rows']).astype(np.int64))
    assert R.same(have, want), R.diff(have, want)


def _keyframe_side(api, matcher, fn, sc, case, views, th):
    """the member through k_project_keyframe + search per direction and the bookkeeping replay: run_kp's dict"""
    kA, dA, kB, dB, sf = views
    frames = dict(A=matcher.frame(kA, dA, sc['bounds']), B=matcher.frame(kB, dB, sc['bounds']))
    lm = _table(api, matcher, sc['tab'])
    is2 = (1.0 / (np.asarray(sf, np.float32) ** 2)).astype(np.float32)
    try:
        best = [matcher.search_projected_keyframe(frames[d['to']], lm, KP.api_projection(api, d['pr']), d['rows'], d['flags'], sf, float(th),
                                                  kp_skip=d['kp_skip'], claim=d['claim'], inv_sigma2=is2 if d['chi2'] else None, chi2=5.99,
                                                  max_dist=d['max_dist'])['best_idx'] for d in case['dirs']]
    finally:
        lm.close()
        for f in frames.values():
            f.close()
    return {k: np.asarray(v).astype(np.int64) for k, v in KP.replay(fn, case, best).items() if k != 'disagree'}     # (a diagnostic of replay's)


@pytest.mark.parametrize('fn,seed,th', R.KP_CASES)
def test_fused_keyframe_projection_equals_the_reference_object(fn, seed, th, api, matcher, kp_L, reg, ref):
    """k_project_keyframe + search (orbfe_search_projected_keyframe_frame) and the bookkeeping that follows it against
    SearchByProjection(KeyFrame, Scw), both Fuse overloads and SearchBySim3: return value, slots, vpReplacePoint, bad / nObs / idxInKF"""
    sc = R.kp_scene(seed)
    have = _keyframe_side(api, matcher, fn, sc, KP.make_case(kp_L, fn, sc, th), R.frames(), th)
    want = reference('kp:%s:%d:%g' % (fn, seed, th), reg, ref)
    assert int(want['ret']) >= 10
    assert R.same(have, want), R.diff(have, want)


@pytest.mark.parametrize('fn,th', R.EDGE_CASES)
def test_fused_keyframe_projection_on_edge_points(fn, th, api, matcher, reg, ref):
    """the same route on the edge MapPoints under the identity pose (z = +-0, u / v on each bound, dist3D on and past both invariance
    bounds, the viewing cosine on 0.5, every level), every predicted level inside the pyramid"""
    S, case = R.edge_case(fn, th)
    have = _keyframe_side(api, matcher, fn, S['sc'], case, S['views'], th)
    want = reference('edge:%s' % fn, reg, ref)
    assert R.same(have, want), R.diff(have, want)


@pytest.mark.parametrize('d1,d2,found', R.SIM3_TH_HIGH)
def test_search_by_sim3_at_th_high(d1, d2, found, api, matcher, reg, ref):
    """max_dist = TH_HIGH of the k_project_keyframe route: one candidate per direction at exactly 100 / 101"""
    S, case = R.sim3_th_high_case(d1, d2)
    have = _keyframe_side(api, matcher, KP.SIM3, S['sc'], case, S['views'], 4.0)
    want = reference('sim3_th_high:%d:%d' % (d1, d2), reg, ref)
    assert R.same(have, want), R.diff(have, want)
    assert int(have['ret']) == found


def test_fused_local_points_equals_the_reference_object(api, matcher, oracle, ref):
    """orbfe_search_local_points_frame: the call's own projection (mTrackProjX / Y, mnTrackScaleLevel, mTrackViewCos, mbTrackInView) is
    handed to the reference's SearchByProjection(Frame, MapPoints, th), whose result the fused search must equal.  500 MapPoints and 25
    repeats: two 256-lane blocks and a partial third.  The inputs of the member come from the GPU, so no golden can stand in: without
    the library the oracle's restatement of that member does, which tests/test_os1_matcher_ref.py holds to the library and the golden."""
    kA, dA, kB, dB, sf = R.frames()
    W, H, n_mp = 640, 480, 500
    mp = U.triangulate(kA, dA, sf, n_mp, U.camera(W, H), seed=31)
    cam = U.moved_camera(W, H, 3, -2, 8.0, seed=32)
    rng = np.random.default_rng(33)
    rows = np.concatenate([rng.permutation(n_mp), rng.integers(0, n_mp, n_mp // 20)]).astype(np.int32)
    flags = U.flags_for(len(rows), seed=34)
    occ = (rng.random(len(kB)) < 0.1).astype(np.uint8)
    bounds = (0.0, float(W), 0.0, float(H))
    member = ref or oracle
    print('\nfused local points: the member is run by %s' % ('the library' if ref else "the oracle's restatement (no library: the inputs come from the GPU, no golden can hold them)"))
    frame = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, mp)
    try:
        for th in (1.0, 5.0):
            fused = matcher.search_local_points(frame, lm, U.api_camera(api, cam), rows, flags, occ, sf, th)
            inv = fused['in_view'] == 1
            assert inv.sum() > n_mp // 4 and ((fused['level'][inv] >= 0) & (fused['level'][inv] < len(sf))).all()
            n, a = member.search_by_projection(kB, dB, bounds, sf, occ, fused['proj_xy'], np.where(inv, fused['level'], 0), fused['view_cos'],
                                               U.oracle_flags(fused, flags), mp['desc'][rows], th, 0.8)
            assert fused['nmatches'] == n and n > 20
            assert (np.asarray(fused['kp_assigned']) == np.asarray(a)).all()
    finally:
        lm.close()
        frame.close()
    # ... and with local_map_util.edge_points (isInFrustum's edges: behind the camera, on and one float beyond each bound, 0.8 * min /
    # 1.2 * max +- 1 ulp, viewing cosines at 0.5 and around 0.998) under the identity camera.  Edge points that are in view with a level
    # outside the pyramid are left out: the call refuses them (test_gpu_local_map.py), and the member would index mvScaleFactors there.
    camA = U.camera(W, H)
    E = U.edge_points(camA, bounds, sf)
    ne = len(E['pos'])
    E['desc'] = dB[np.arange(ne) % len(dB)].copy()
    tab = U.concat(mp, E)
    frame = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, tab)
    try:
        rows_e = np.concatenate([n_mp + np.arange(ne), rng.permutation(n_mp)[:200]]).astype(np.int32)
        fl_e = np.concatenate([np.full(ne, 8, np.uint8), U.flags_for(200, seed=35)])
        proj = matcher.project_local_map(frame, lm, U.api_camera(api, camA), rows_e, fl_e)
        keep = ~((proj['in_view'] == 1) & ((proj['level'] < 0) | (proj['level'] >= len(sf))))
        edge_kept = keep[:ne]
        assert edge_kept.sum() >= ne // 2 and (proj['in_view'][:ne][edge_kept] == 1).any() and (proj['in_view'][:ne][edge_kept] == 0).any()
        rows_e, fl_e = rows_e[keep], fl_e[keep]
        for th in (1.0, 5.0):
            fused = matcher.search_local_points(frame, lm, U.api_camera(api, camA), rows_e, fl_e, occ, sf, th)
            inv = fused['in_view'] == 1
            n, a = member.search_by_projection(kB, dB, bounds, sf, occ, fused['proj_xy'], np.where(inv, fused['level'], 0), fused['view_cos'],
                                               U.oracle_flags(fused, fl_e), tab['desc'][rows_e], th, 0.8)
            assert fused['nmatches'] == n and n > 5
            assert (np.asarray(fused['kp_assigned']) == np.asarray(a)).all()
    finally:
        lm.close()
        frame.close()
