"""-m gpu: the projection loops of SearchByProjection(CurrentFrame, LastFrame, th) and (CurrentFrame, pKF, sAlreadyFound, th,
ORBdist) on the device (orbfe_project_sources) and fused with the search (orbfe_search_by_projection_sources_frame), bit-exact
against the reference restatement tests/cpp/project_sources_ref.cpp (src/ORBmatcher.cc:1313-1347, 1441-1479), the CPU oracle's
whole-function restatements orc_sbp_frame / orc_sbp_keyframe, and the existing two-step route (host arrays ->
orbfe_search_by_projection_uv_frame)."""

import numpy as np
import pytest

import local_map_util as U
import source_projection_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return S.build_ref(tmp_path_factory.mktemp('spref'))


@pytest.fixture(scope='module')
def oracle():
    from oracle.pyoracle import Oracle
    o = Oracle()
    S.bind_oracle(o)
    return o


@pytest.fixture(scope='module')
def matcher(api):
    m = api.Matcher(0)
    yield m
    m.close()


_FRAMES = {}


def _frames(api, W, H, nfeat):
    """the GPU extractor's keypoints (the CPU file runs the same cases on the oracle extractor's)"""
    if (W, H, nfeat) not in _FRAMES:
        ex = api.Extractor(nfeat, 1.2, 8, 20, 7)
        _FRAMES[(W, H, nfeat)] = S.frames(W, H, nfeat, extractor=ex)
        ex.close()
    return _FRAMES[(W, H, nfeat)]


def _table(api, matcher, tab):
    n = len(tab['pos'])
    lm = api.LocalMap(matcher, n)
    lm.set_rows(np.arange(n), tab['pos'], tab['normal'], tab['min'], tab['max'], tab['desc'])
    return lm


@pytest.mark.parametrize('pose', ['identity', 'moved'])
@pytest.mark.parametrize('mode', [S.LAST_FRAME, S.KEYFRAME])
def test_projection_parity(api, matcher, ref, mode, pose):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(api, W, H, 2000)
    sc, edge = S.edge_sources(S.scene(kA, dA, kB, sf, W, H, seed=5), sf)
    S.assert_edges(ref, sc, edge, kA, sf)   # a point behind the camera: rejected in LAST_FRAME mode, kept in KEYFRAME mode
    cam = sc['camA'] if pose == 'identity' else sc['cam']
    flags = S.flags_of(sc, mode)
    src = matcher.frame(kA, dA, sc['bounds'])
    cur = matcher.frame(kB, dB, sc['bounds'])
    lm = _table(api, matcher, sc['tab'])
    got = matcher.project_sources(cur, src, lm, U.api_camera(api, cam), mode, sc['rows'], flags)
    want = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], cam, sc['bounds'], mode)
    S.check_projection(got, want)
    assert want['n_valid'] > len(kA) // 6
    skipmask = S.MP_SKIP | (S.MP_BAD if mode == S.KEYFRAME else 0)
    assert not want['valid'][(flags & skipmask) != 0].any()
    if mode == S.LAST_FRAME:
        v = want['valid'] == 1
        assert (want['level'][v] == kA['octave'][v]).all()
        assert want['valid'][(flags & (S.MP_SKIP | S.MP_BAD)) == S.MP_BAD].any()   # isBad() is not asked in this mode
    lm.close()
    cur.close()
    src.close()


def _two_step(matcher, cur, sc, mode, kA, sf, proj, flags, th, max_dist, check_ori):
    """the existing route: host arrays -> orbfe_search_by_projection_uv_frame on the resident frame"""
    return matcher.search_by_projection_uv(cur, None, None, sf, sc['st']['occ'], proj['uv'], proj['level'], kA['angle'], flags,
                                           proj['valid'], sc['tab']['desc'][sc['rows']], th, max_dist, mode == S.KEYFRAME, check_ori)


def _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, check_ori, W, info):
    want = S.checked_oracle_case(ref, oracle, sc, mode, kA, kB, dB, sf, th, max_dist, check_ori, W, info)
    got = matcher.search_by_projection_sources(cur, src, lm, U.api_camera(api, sc['cam']), mode, sc['rows'], want['flags'],
                                               sc['st']['occ'], sf, th, max_dist, check_ori)
    S.check_projection(got, want['proj'])
    assert got['nmatches'] == want['nmatches']
    assert (S.cur_mp_from_assigned(want['before'], got['kp_assigned'], sc['rows']) == want['cur_mp']).all()
    n2, a2 = _two_step(matcher, cur, sc, mode, kA, sf, want['proj'], want['flags'], th, max_dist, check_ori)
    assert got['nmatches'] == n2 and (got['kp_assigned'] == a2).all()
    return got


@pytest.mark.parametrize('W,H,nfeat', [(640, 480, 500), (1920, 1080, 2000)])
@pytest.mark.parametrize('mode', [S.LAST_FRAME, S.KEYFRAME])
def test_fused_equals_oracle_and_two_step(api, matcher, ref, oracle, mode, W, H, nfeat):
    kA, dA, kB, dB, sf = _frames(api, W, H, nfeat)
    info = dict(pruned=0)
    cleared = 0
    for th, max_dist in S.CASES[mode]:
        sc = S.scene(kA, dA, kB, sf, W, H, seed=S.case_seed(mode, th, W))
        src = matcher.frame(kA, dA, sc['bounds'])
        cur = matcher.frame(kB, dB, sc['bounds'])
        lm = _table(api, matcher, sc['tab'])
        for check_ori in (True, False):
            got = _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, check_ori, W, info)
            cleared += int((got['kp_assigned'] == -2).sum())
        lm.close()
        cur.close()
        src.close()
    assert info['pruned'] > 0 and cleared > 0   # the rotation check cleared a slot (-2) in at least one case of this mode


@pytest.mark.parametrize('mode', [S.LAST_FRAME, S.KEYFRAME])
def test_row_updates_between_calls_and_second_call(api, matcher, ref, oracle, mode):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(api, W, H, 2000)
    th, max_dist = S.CASES[mode][1] if mode == S.LAST_FRAME else S.CASES[mode][0]
    sc = S.scene(kA, dA, kB, sf, W, H, seed=77 + mode)
    src = matcher.frame(kA, dA, sc['bounds'])
    cur = matcher.frame(kB, dB, sc['bounds'])
    lm = _table(api, matcher, sc['tab'])
    info = dict(pruned=0)
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, True, W, info)
    rng = np.random.default_rng(78)
    n = len(sc['tab']['pos'])
    r1 = rng.choice(n, n // 20, replace=False).astype(np.int32)          # 5 % of the MapPoints move
    sc['tab']['pos'][r1] = (sc['tab']['pos'][r1] * np.float32(1.002)).astype(np.float32)
    lm.set_rows(r1, pos=sc['tab']['pos'][r1])
    r2 = rng.choice(n, n // 20, replace=False).astype(np.int32)          # 5 % of the descriptors are recomputed
    sc['tab']['desc'][r2] = rng.integers(0, 256, (len(r2), 32), dtype=np.uint8)
    lm.set_rows(r2, desc=sc['tab']['desc'][r2])
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, True, W, info)
    # the same frame a second time with 2*th, nothing sent in between
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, 2 * th, max_dist, True, W, info)
    lm.close()
    cur.close()
    src.close()


def test_errors_leave_everything_usable(api, ref, oracle):
    W, H = 640, 480
    kA, dA, kB, dB, sf = _frames(api, W, H, 500)
    mode = S.KEYFRAME
    th, max_dist = S.CASES[mode][0]
    sc = S.scene(kA, dA, kB, sf, W, H, seed=S.case_seed(mode, th, W))
    matcher, other = api.Matcher(0), api.Matcher(0)
    src = matcher.frame(kA, dA, sc['bounds'])
    cur = matcher.frame(kB, dB, sc['bounds'])
    lm = _table(api, matcher, sc['tab'])
    acam = U.api_camera(api, sc['cam'])
    flags = S.flags_of(sc, mode)
    occ = sc['st']['occ']
    info = dict(pruned=0)

    def fails(fn, *a):
        with pytest.raises(api.OrbfeError) as e:
            fn(*a)
        assert e.value.code == -1   # ORBFE_ERR_INVALID
    # the source frame's size is not n_src
    fails(matcher.project_sources, cur, src, lm, acam, mode, sc['rows'][:-1], flags[:-1])
    fails(matcher.search_by_projection_sources, cur, src, lm, acam, mode, sc['rows'][:-1], flags[:-1], occ, sf, th, max_dist)
    # a matcher that does not own the map
    ocur, osrc = other.frame(kB, dB, sc['bounds']), other.frame(kA, dA, sc['bounds'])
    fails(other.project_sources, ocur, osrc, lm, acam, mode, sc['rows'], flags)
    fails(other.search_by_projection_sources, ocur, osrc, lm, acam, mode, sc['rows'], flags, occ, sf, th, max_dist)
    # a projected row outside the table (a skipped source may carry anything)
    i = int(np.flatnonzero((flags & (S.MP_SKIP | S.MP_BAD)) == 0)[3])
    j = int(np.flatnonzero((flags & S.MP_SKIP) != 0)[3])
    bad_rows = sc['rows'].copy()
    bad_rows[i] = len(sc['tab']['pos'])
    fails(matcher.project_sources, cur, src, lm, acam, mode, bad_rows, flags)
    fails(matcher.search_by_projection_sources, cur, src, lm, acam, mode, bad_rows, flags, occ, sf, th, max_dist)
    fails(matcher.search_by_projection_sources, cur, src, lm, acam, S.LAST_FRAME, bad_rows, S.flags_of(sc, S.LAST_FRAME), occ, sf, th)
    ok_rows = sc['rows'].copy()
    ok_rows[j] = 1 << 30
    S.check_projection(matcher.project_sources(cur, src, lm, acam, mode, ok_rows, flags),
                       S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode))
    # a bad mode
    fails(matcher.project_sources, cur, src, lm, acam, 2, sc['rows'], flags)
    # KEYFRAME mode: a valid source whose predicted level is >= nlevels (mfMaxDistance = dist * 1.2^9)
    proj = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode)
    s = int(np.flatnonzero(proj['valid'] == 1)[5])
    row = int(sc['rows'][s])
    d = U._norm((sc['tab']['pos'][row] - sc['cam']['Ow'])[None].astype(np.float32))[0]
    keep = sc['tab']['min'][row], sc['tab']['max'][row]
    sc['tab']['min'][row], sc['tab']['max'][row] = 0.0, d * np.float32(1.2 ** 9)
    lm.set_rows([row], min_raw=np.float32([0.0]), max_raw=np.float32([sc['tab']['max'][row]]))
    want = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode)
    assert want['valid'][s] == 1 and want['level'][s] >= len(sf)
    S.check_projection(matcher.project_sources(cur, src, lm, acam, mode, sc['rows'], flags), want)   # reported as it is
    nm = None
    with pytest.raises(api.OrbfeError) as e:
        nm = matcher.search_by_projection_sources(cur, src, lm, acam, mode, sc['rows'], flags, occ, sf, th, max_dist)
    assert e.value.code == -1 and nm is None
    # the C call's nmatches is 0 on that failure
    import ctypes as C
    rows32, occ8, sf32 = np.ascontiguousarray(sc['rows'], np.int32), np.ascontiguousarray(occ, np.uint8), np.ascontiguousarray(sf, np.float32)
    assigned = np.full(len(kB), -1, np.int32)
    cnm, cnv = C.c_int(7), C.c_int(7)
    rc = matcher.L.orbfe_search_by_projection_sources_frame(matcher.h, cur.h, src.h, lm.h, C.byref(acam), mode, U._p(rows32), U._p(flags),
                                                            len(rows32), U._p(sf32), len(sf32), U._p(occ8), th, int(max_dist), 1, None, None,
                                                            None, U._p(assigned), C.byref(cnm), C.byref(cnv))
    assert rc == -1 and cnm.value == 0
    # the next valid call on the same handles succeeds and is exact
    sc['tab']['min'][row], sc['tab']['max'][row] = keep
    lm.set_rows([row], min_raw=np.float32([keep[0]]), max_raw=np.float32([keep[1]]))
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, True, W, info)
    # LAST_FRAME mode: refused up front when the source frame holds an octave the pyramid does not have
    fails(matcher.search_by_projection_sources, cur, src, lm, acam, S.LAST_FRAME, sc['rows'], S.flags_of(sc, S.LAST_FRAME), occ, sf[:4], th)
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, S.LAST_FRAME, kA, kB, dB, sf, 15.0, S.TH_HIGH, True, W, info)
    # no sources at all / an empty current frame
    e0 = matcher.frame(kA[:0], dA[:0], sc['bounds'])
    r = matcher.search_by_projection_sources(cur, e0, lm, acam, mode, sc['rows'][:0], flags[:0], occ, sf, th, max_dist)
    assert r['nmatches'] == 0 and r['n_valid'] == 0 and (r['kp_assigned'] == -1).all()
    r = matcher.search_by_projection_sources(e0, src, lm, acam, mode, sc['rows'], flags, occ[:0], sf, th, max_dist)
    assert r['nmatches'] == 0 and r['n_valid'] == proj['n_valid']
    for h in (e0, lm, cur, src, ocur, osrc):
        h.close()
    other.close()
    matcher.close()


def test_out_of_range_level_in_the_second_block(api, matcher, ref, oracle):
    """KEYFRAME mode on the 500-feature frame: two 256-lane blocks, the second one partial.  Two valid sources of the second
    block predict a level >= nlevels (mfMaxDistance = dist * 1.2^9): the fused call fails naming the lower of them, the
    projection alone reports both as they are, and with the two taken out (no MapPoint: ORBFE_MP_SKIP) the fused call equals
    the oracle.  (In LAST_FRAME mode the level is the source's octave, refused up front.)"""
    W, H = 640, 480
    kA, dA, kB, dB, sf = _frames(api, W, H, 500)
    mode = S.KEYFRAME
    th, max_dist = S.CASES[mode][0]
    sc = S.scene(kA, dA, kB, sf, W, H, seed=S.case_seed(mode, th, W))
    n = sc['n']
    assert 256 < n <= 512
    flags = S.flags_of(sc, mode)
    proj = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode)
    named_once = np.bincount(sc['rows'], minlength=n)[sc['rows']] == 1
    cand = np.flatnonzero((proj['valid'] == 1) & named_once & (np.arange(n) >= 256))
    assert len(cand) >= 4
    lo, hi = int(cand[1]), int(cand[3])
    for s in (hi, lo):
        row = int(sc['rows'][s])
        d = U._norm((sc['tab']['pos'][row] - sc['cam']['Ow'])[None].astype(np.float32))[0]
        sc['tab']['min'][row], sc['tab']['max'][row] = 0.0, d * np.float32(1.2 ** 9)
    src = matcher.frame(kA, dA, sc['bounds'])
    cur = matcher.frame(kB, dB, sc['bounds'])
    lm = _table(api, matcher, sc['tab'])
    acam = U.api_camera(api, sc['cam'])
    want = S.ref_project(ref, sc['tab'], sc['rows'], flags, kA['octave'], sc['cam'], sc['bounds'], mode)
    outside = (want['valid'] == 1) & ((want['level'] < 0) | (want['level'] >= len(sf)))
    assert np.flatnonzero(outside).tolist() == [lo, hi]
    with pytest.raises(api.OrbfeError) as e:
        matcher.search_by_projection_sources(cur, src, lm, acam, mode, sc['rows'], flags, sc['st']['occ'], sf, th, max_dist)
    assert e.value.code == -1
    assert 'source %d: predicted level outside [0, %d)' % (lo, len(sf)) in str(e.value)
    S.check_projection(matcher.project_sources(cur, src, lm, acam, mode, sc['rows'], flags), want)
    sc['st']['absent'][[lo, hi]] = 1
    assert (S.flags_of(sc, mode)[[lo, hi]] & S.MP_SKIP).all()
    _check_fused(api, matcher, ref, oracle, cur, src, lm, sc, mode, kA, kB, dB, sf, th, max_dist, True, W, dict(pruned=0))
    lm.close()
    cur.close()
    src.close()


def test_facade_sequence(api, tmp_path):
    """tests/cpp/source_projection_test.cpp: a tracking-shaped sequence through orb_shim.hpp's SearchByProjectionLastFrame /
    SearchByProjectionKeyFrame, every call equal to orc_sbp_frame / orc_sbp_keyframe, rows sent only for changed MapPoints,
    no frame uploaded"""
    import source_projection_facade as F
    exe = F.compile_test(str(tmp_path / 'source_projection_test'))
    stats = F.run(exe, tmp_path)
    assert stats['last_calls'] == 5 and stats['kf_calls'] == 4
    assert stats['matches_last'] > 25 * 5 and stats['matches_kf'] > 0
