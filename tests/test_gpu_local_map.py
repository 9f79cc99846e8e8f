"""-m gpu: the local map on the device -- Frame::isInFrustum over the local MapPoints (orbfe_project_local_map) and that
projection fused with SearchByProjection(F, vpLocalMapPoints, th) (orbfe_search_local_points_frame), bit-exact against the
reference restatement tests/cpp/is_in_frustum_ref.cpp (src/Frame.cc:151-207, src/MapPoint.cc:358-379,
src/Tracking.cc:798-814, host libm logf) and the CPU oracle's SearchByProjection (src/ORBmatcher.cc:45-132)."""

import numpy as np
import pytest

import local_map_util as U
from os1_amd.synth import shifted, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('lmref'))


@pytest.fixture(scope='module')
def matcher(api):
    m = api.Matcher(0)
    yield m
    m.close()


_PAIRS = {}


def _pair(api, W, H, nfeat, seed=11):
    """frame A (the MapPoints' source), frame B = A shifted by (3, -2) px: keypoints, descriptors, scale factors"""
    key = (W, H, nfeat, seed)
    if key not in _PAIRS:
        A = synth(seed, W, H)
        B = shifted(A, 3, -2, seed + 1)
        ex = api.Extractor(nfeat, 1.2, 8, 20, 7)
        kA, dA = ex(A)
        kB, dB = ex(B)
        sf = ex.tables()['sf']
        ex.close()
        _PAIRS[key] = (kA, dA, kB, dB, sf)
    return _PAIRS[key]


def _check_projection(got, want):
    assert got['n_in_view'] == want['n_in_view']
    assert (got['in_view'] == want['in_view']).all()
    assert got['proj_xy'].tobytes() == want['proj_xy'].tobytes()
    assert (got['level'] == want['level']).all()
    assert got['view_cos'].tobytes() == want['view_cos'].tobytes()


def _table(api, matcher, mp):
    lm = api.LocalMap(matcher, len(mp['pos']))
    lm.set_rows(np.arange(len(mp['pos'])), mp['pos'], mp['normal'], mp['min'], mp['max'], mp['desc'])
    return lm


def test_device_logf_matches_host_libm(api, matcher, ref):
    rng = np.random.default_rng(5)
    bits = np.concatenate([np.arange(0x3d800000, 0x45800000, 13, dtype=np.uint32),        # [2^-4, 2^12) every 13th float
                           rng.integers(1, 0x7f800000, 2_000_000, dtype=np.uint32),        # all positive floats
                           np.arange(0, 0x00800000, 4099, dtype=np.uint32),                # subnormals
                           np.array([0x3f800000, 0x7f800000, 0x00000001, 0x007fffff], np.uint32)])
    x = bits.view(np.float32)
    sf = _pair(api, 640, 480, 500)[4]
    x = np.concatenate([x, sf, (sf * np.float32(1.0000001)).astype(np.float32)])
    got = matcher.logf(x)
    want = np.zeros_like(x)
    ref.ref_logf_array(U._p(x), len(x), U._p(want))
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, 'device logf differs at %r' % [(float(x[i]), float(got[i]), float(want[i])) for i in bad[:5]]


@pytest.mark.parametrize('pose', ['identity', 'moved'])
def test_projection_parity(api, matcher, ref, pose):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _pair(api, W, H, 2000)
    camA = U.camera(W, H)
    mp = U.concat(U.triangulate(kA, dA, sf, 3000, camA, seed=1), U.edge_points(camA, (0.0, W, 0.0, H), sf))
    n = len(mp['pos'])
    cam = camA if pose == 'identity' else U.moved_camera(W, H, 3, -2, 8.0, seed=2)
    rng = np.random.default_rng(3)
    rows = np.concatenate([rng.permutation(n), rng.integers(0, n, 300)]).astype(np.int32)   # every row, some repeated
    flags = U.flags_for(len(rows), seed=4)
    flags[rows >= 3000] &= np.uint8(~(2 | 16) & 0xff)       # the edge points are always projected
    frame = matcher.frame(kB, dB, (0.0, W, 0.0, H))
    lm = _table(api, matcher, mp)
    got = matcher.project_local_map(frame, lm, U.api_camera(api, cam), rows, flags)
    want = U.ref_project(ref, mp, rows, flags, cam, (0.0, W, 0.0, H))
    _check_projection(got, want)
    assert want['n_in_view'] > 1000
    if pose == 'identity':   # the ulp-sensitive case is common: predicted level == the octave mfMaxDistance was made with
        lv = want['level'][(want['in_view'] == 1) & (rows < 3000)]
        assert len(lv) > 1000 and (lv >= 0).all()
    # the edge points did what they are there for: some in view, some out, levels outside the pyramid among them
    e = rows >= 3000
    assert want['in_view'][e].any() and not want['in_view'][e].all()
    assert (want['level'][e & (want['in_view'] == 1)] >= len(sf)).any()
    # skipped and bad MapPoints are never in view
    assert not want['in_view'][(flags & (2 | 16)) != 0].any()
    lm.close()
    frame.close()


def _fused_case(api, matcher, ref, oracle, W, H, nfeat, n_mp, th, seed):
    kA, dA, kB, dB, sf = _pair(api, W, H, nfeat)
    camA = U.camera(W, H)
    mp = U.triangulate(kA, dA, sf, n_mp, camA, seed=seed)
    cam = U.moved_camera(W, H, 3, -2, 8.0, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    rows = np.concatenate([rng.permutation(n_mp), rng.integers(0, n_mp, n_mp // 20)]).astype(np.int32)
    flags = U.flags_for(len(rows), seed=seed + 3)
    occ = (rng.random(len(kB)) < 0.1).astype(np.uint8)
    bounds = (0.0, float(W), 0.0, float(H))
    frame = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, mp)
    acam = U.api_camera(api, cam)
    want = U.ref_project(ref, mp, rows, flags, cam, bounds)
    inv = want['in_view'] == 1
    assert inv.sum() > n_mp // 3
    assert ((want['level'][inv] >= 0) & (want['level'][inv] < len(sf))).all()
    fused = matcher.search_local_points(frame, lm, acam, rows, flags, occ, sf, th)
    _check_projection(fused, want)
    # two steps: the projection, then the rows search on the same descriptors
    proj = matcher.project_local_map(frame, lm, acam, rows, flags)
    _check_projection(proj, want)
    tab = api.DescTable(n_mp)
    tab.host.a[:] = mp['desc']
    tab.upload(matcher, 0, n_mp)
    mflags = U.oracle_flags(proj, flags)
    n2, a2 = matcher.search_by_projection_rows(frame, sf, occ, proj['proj_xy'], proj['level'], proj['view_cos'], mflags, tab, rows,
                                               th, 0.8)
    on, oa = oracle.search_by_projection(kB, dB, bounds, sf, occ, want['proj_xy'], want['level'], want['view_cos'],
                                         U.oracle_flags(want, flags), mp['desc'][rows], th, 0.8)
    assert fused['nmatches'] == n2 == on and on > 50
    assert (fused['kp_assigned'] == a2).all() and (a2 == oa).all()
    tab.free()
    return frame, lm, mp, cam, rows, flags, occ, sf, bounds


@pytest.fixture(scope='module')
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.mark.parametrize('th', [1.0, 5.0])
def test_fused_equals_two_step_and_oracle_3000(api, matcher, ref, oracle, th):
    frame, lm, *_ = _fused_case(api, matcher, ref, oracle, 1920, 1080, 2000, 3000, th, seed=21)
    lm.close()
    frame.close()


def test_fused_equals_two_step_and_oracle_config5(api, matcher, ref, oracle):
    frame, lm, *_ = _fused_case(api, matcher, ref, oracle, 3840, 2160, 4000, 10000, 1.0, seed=31)
    lm.close()
    frame.close()


def test_row_updates_between_calls(api, matcher, ref, oracle):
    frame, lm, mp, cam, rows, flags, occ, sf, bounds = _fused_case(api, matcher, ref, oracle, 1920, 1080, 2000, 3000, 1.0, seed=41)
    rng = np.random.default_rng(42)
    n = len(mp['pos'])
    acam = U.api_camera(api, cam)
    # moved points (positions only), new normals (normals only), new descriptors (descriptors only): NULL fields keep their values
    r1 = rng.choice(n, 200, replace=False).astype(np.int32)
    mp['pos'][r1] = (mp['pos'][r1] * np.float32(1.01)).astype(np.float32)
    lm.set_rows(r1, pos=mp['pos'][r1])
    r2 = rng.choice(n, 200, replace=False).astype(np.int32)
    mp['normal'][r2] = -mp['normal'][r2]
    lm.set_rows(r2, normal=mp['normal'][r2])
    r3 = rng.choice(n, 300, replace=False).astype(np.int32)
    mp['desc'][r3] = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    lm.set_rows(r3, desc=mp['desc'][r3])
    r4 = rng.choice(n, 100, replace=False).astype(np.int32)
    mp['max'][r4] = (mp['max'][r4] * np.float32(0.95)).astype(np.float32)
    mp['min'][r4] = (mp['min'][r4] * np.float32(0.5)).astype(np.float32)
    lm.set_rows(r4, min_raw=mp['min'][r4], max_raw=mp['max'][r4])
    want = U.ref_project(ref, mp, rows, flags, cam, bounds)
    got = matcher.search_local_points(frame, lm, acam, rows, flags, occ, sf, 1.0)
    _check_projection(got, want)
    kB, dB = _pair(api, 1920, 1080, 2000)[2:4]
    on, oa = oracle.search_by_projection(kB, dB, bounds, sf, occ, want['proj_xy'], want['level'], want['view_cos'],
                                         U.oracle_flags(want, flags), mp['desc'][rows], 1.0, 0.8)
    assert got['nmatches'] == on and (got['kp_assigned'] == oa).all()
    assert not (want['in_view'][np.isin(rows, r2)]).any()   # turned normals: viewing cosine < 0.5
    lm.close()
    frame.close()


def test_edges(api, matcher, ref, oracle):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _pair(api, W, H, 2000)
    camA = U.camera(W, H)
    mp = U.triangulate(kA, dA, sf, 500, camA, seed=51)
    bounds = (0.0, float(W), 0.0, float(H))
    frame = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, mp)
    occ = np.zeros(len(kB), np.uint8)
    acam = U.api_camera(api, camA)
    rows = np.arange(500, dtype=np.int32)
    flags = np.zeros(500, np.uint8)
    # n_mp = 0
    r = matcher.search_local_points(frame, lm, acam, rows[:0], flags[:0], occ, sf, 1.0)
    assert r['nmatches'] == 0 and r['n_in_view'] == 0 and (r['kp_assigned'] == -1).all()
    assert matcher.project_local_map(frame, lm, acam, rows[:0], flags[:0])['n_in_view'] == 0
    # everything culled: the camera looks away
    away = U.camera(W, H, U.rotation((0, 1, 0), np.pi), np.zeros(3, np.float32))
    r = matcher.search_local_points(frame, lm, U.api_camera(api, away), rows, flags, occ, sf, 1.0)
    assert r['nmatches'] == 0 and r['n_in_view'] == 0 and not r['in_view'].any() and (r['kp_assigned'] == -1).all()
    # rows outside the table: refused by set_rows and by the calls (unless the MapPoint is skipped or bad)
    with pytest.raises(api.OrbfeError):
        lm.set_rows([500], pos=np.zeros((1, 3), np.float32))
    with pytest.raises(api.OrbfeError):
        lm.set_rows([3, 3], pos=np.zeros((2, 3), np.float32))
    bad_rows = rows.copy()
    bad_rows[7] = 500
    with pytest.raises(api.OrbfeError):
        matcher.project_local_map(frame, lm, acam, bad_rows, flags)
    with pytest.raises(api.OrbfeError):
        matcher.search_local_points(frame, lm, acam, bad_rows, flags, occ, sf, 1.0)
    skip = flags.copy()
    skip[7] = 16
    want = U.ref_project(ref, mp, np.where(bad_rows == 500, 0, bad_rows), skip, camA, bounds)
    _check_projection(matcher.project_local_map(frame, lm, acam, bad_rows, skip), want)
    # a predicted level >= nlevels: MapPoint 9 seen from far closer than its depth range says (mfMaxDistance = dist * 1.2^9)
    PO = mp['pos'][9] - camA['Ow']
    d = U._norm(PO[None])[0]
    lm.set_rows([9], min_raw=np.float32([0.0]), max_raw=np.float32([d * np.float32(1.2 ** 9)]))
    mp['min'][9] = 0.0
    mp['max'][9] = d * np.float32(1.2 ** 9)
    want = U.ref_project(ref, mp, rows, flags, camA, bounds)
    got = matcher.project_local_map(frame, lm, acam, rows, flags)
    _check_projection(got, want)
    assert got['in_view'][9] == 1 and got['level'][9] >= len(sf)
    with pytest.raises(api.OrbfeError) as e:
        matcher.search_local_points(frame, lm, acam, rows, flags, occ, sf, 1.0)
    assert e.value.code == -1
    # the matcher stays usable: the same call without that MapPoint equals the oracle
    fl2 = flags.copy()
    fl2[9] = 2
    want = U.ref_project(ref, mp, rows, fl2, camA, bounds)
    got = matcher.search_local_points(frame, lm, acam, rows, fl2, occ, sf, 1.0)
    _check_projection(got, want)
    on, oa = oracle.search_by_projection(kB, dB, bounds, sf, occ, want['proj_xy'], want['level'], want['view_cos'],
                                         U.oracle_flags(want, fl2), mp['desc'][rows], 1.0, 0.8)
    assert got['nmatches'] == on and (got['kp_assigned'] == oa).all()
    lm.close()
    frame.close()


def test_out_of_range_level_in_the_second_block(api, matcher, ref, oracle):
    """500 MapPoints are two 256-lane blocks, the second one partial.  MapPoints 300 and 270 predict a level >= nlevels
    (mfMaxDistance = dist * 1.2^9): the fused call fails naming the lowest of them, the projection alone reports both as they
    are, and with the two skipped the fused call equals the oracle."""
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _pair(api, W, H, 2000)
    camA = U.camera(W, H)
    mp = U.triangulate(kA, dA, sf, 500, camA, seed=51)
    for i in (300, 270):
        d = U._norm((mp['pos'][i] - camA['Ow'])[None])[0]
        mp['min'][i] = 0.0
        mp['max'][i] = d * np.float32(1.2 ** 9)
    bounds = (0.0, float(W), 0.0, float(H))
    frame = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, mp)
    occ = np.zeros(len(kB), np.uint8)
    acam = U.api_camera(api, camA)
    rows = np.arange(500, dtype=np.int32)
    flags = np.zeros(500, np.uint8)
    want = U.ref_project(ref, mp, rows, flags, camA, bounds)
    outside = (want['in_view'] == 1) & ((want['level'] < 0) | (want['level'] >= len(sf)))
    assert np.flatnonzero(outside).tolist() == [270, 300]
    with pytest.raises(api.OrbfeError) as e:
        matcher.search_local_points(frame, lm, acam, rows, flags, occ, sf, 1.0)
    assert e.value.code == -1
    assert 'MapPoint 270: predicted level outside [0, %d)' % len(sf) in str(e.value)
    _check_projection(matcher.project_local_map(frame, lm, acam, rows, flags), want)
    fl2 = flags.copy()
    fl2[[270, 300]] = 16
    want = U.ref_project(ref, mp, rows, fl2, camA, bounds)
    got = matcher.search_local_points(frame, lm, acam, rows, fl2, occ, sf, 1.0)
    _check_projection(got, want)
    on, oa = oracle.search_by_projection(kB, dB, bounds, sf, occ, want['proj_xy'], want['level'], want['view_cos'],
                                         U.oracle_flags(want, fl2), mp['desc'][rows], 1.0, 0.8)
    assert got['nmatches'] == on and on > 0 and (got['kp_assigned'] == oa).all()
    lm.close()
    frame.close()


def test_search_local_points_facade_sequence(api, tmp_path, ref, oracle):
    """tests/cpp/local_map_test.cpp: a tracking-shaped sequence through orb_shim.hpp's SearchLocalPoints"""
    import local_map_facade as F
    exe = F.compile_test(str(tmp_path / 'local_map_test'))
    F.run_and_check(api, exe, tmp_path, ref, oracle)
