"""-m gpu: the projection loops of SearchByProjection(KeyFrame*, Scw), Fuse, Fuse(Scw) and SearchBySim3 on the device
(orbfe_project_keyframe) and fused with the projected search (orbfe_search_projected_keyframe_frame), bit-exact against the
reference restatement tests/cpp/project_keyframe_ref.cpp (src/ORBmatcher.cc:316-357, 833-873, 973-1015, 1122-1155, 1202-1235),
the CPU oracle's whole-function restatements orc_sbp_scw / orc_fuse / orc_fuse_scw / orc_search_by_sim3, and the two-step
route (orbfe_project_keyframe -> orbfe_search_projected_frame).  Every comparison is ==."""

import numpy as np
import pytest

import keyframe_projection_util as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kpref'))


@pytest.fixture(scope='module')
def oracle():
    from oracle.pyoracle import Oracle
    o = Oracle()
    K.bind_oracle(o)
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
        _FRAMES[(W, H, nfeat)] = K.SP.frames(W, H, nfeat, extractor=ex)
        ex.close()
    return _FRAMES[(W, H, nfeat)]


def _table(api, matcher, tab):
    n = len(tab['pos'])
    lm = api.LocalMap(matcher, n)
    lm.set_rows(np.arange(n), tab['pos'], tab['normal'], tab['min'], tab['max'], tab['desc'])
    return lm


def _inv_sigma2(sf):
    sf = np.asarray(sf, np.float32)
    return (1.0 / (sf * sf)).astype(np.float32)


def _fused(api, matcher, frames, lm, d, sf, th):
    return matcher.search_projected_keyframe(frames[d['to']], lm, K.api_projection(api, d['pr']), d['rows'], d['flags'], sf, float(th),
                                             kp_skip=d['kp_skip'], claim=d['claim'], inv_sigma2=_inv_sigma2(sf) if d['chi2'] else None,
                                             chi2=5.99, max_dist=d['max_dist'])


def _two_step(api, matcher, frames, lm, sc, d, sf, th):
    """orbfe_project_keyframe, then host arrays -> orbfe_search_projected_frame on the resident keyframe"""
    proj = matcher.project_keyframe(frames[d['to']], lm, K.api_projection(api, d['pr']), d['rows'], d['flags'], sf, float(th))
    sdesc = sc['tab']['desc'][np.where(proj['valid'] == 1, d['rows'], 0)]
    res = matcher.search_projected(frames[d['to']], None, None, proj['uv'], proj['radius'], proj['level'], proj['valid'], sdesc,
                                   kp_skip=d['kp_skip'], claim=d['claim'], inv_sigma2=_inv_sigma2(sf) if d['chi2'] else None, chi2=5.99,
                                   max_dist=d['max_dist'])
    return proj, res


def _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, th, kA, dA, kB, dB, sf, W, info):
    c = K.checked_oracle_case(ref, oracle, fn, sc, th, kA, dA, kB, dB, sf, W, info)
    best = []
    for d, want_proj, cpu_best in zip(c['case']['dirs'], c['projs'], c['best']):
        got = _fused(api, matcher, frames, lm, d, sf, th)
        K.check_projection(got, want_proj)
        assert (got['best_idx'] == cpu_best).all()
        assert got['nmatches'] == int((cpu_best >= 0).sum())
        proj2, (n2, bi2, bd2) = _two_step(api, matcher, frames, lm, sc, d, sf, th)
        K.check_projection(proj2, want_proj)
        assert got['nmatches'] == n2 and (got['best_idx'] == bi2).all() and (got['best_dist'] == bd2).all()
        best.append(got['best_idx'])
    K.same_outputs(K.replay(fn, c['case'], best), c['want'])          # the whole function, through the fused call
    return c


def test_projection_parity_on_edge_points(api, matcher, ref):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(api, W, H, 2000)
    cam = K.U.camera(W, H)
    Kc = np.float32([cam['fx'], cam['fy'], cam['cx'], cam['cy'], cam['lsf']])
    bounds = (0.0, float(W), 0.0, float(H))
    tab, names = K.edge_points(bounds, Kc, sf)
    want = K.assert_edges(ref, tab, names, bounds, Kc, sf)
    kf = matcher.frame(kB, dB, bounds)
    lm = _table(api, matcher, tab)
    n = len(tab['pos'])
    I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for dbl in (False, True):
        pr = K.projection(I3, z3, Kc, Ow=z3, invz_double=dbl)
        got = matcher.project_keyframe(kf, lm, K.api_projection(api, pr), np.arange(n), np.zeros(n, np.uint8), sf, 4.0)
        K.check_projection(got, want[dbl])
    # the Sim3 form on the same points: the norm of the transformed point, no viewing-angle test, a second transform
    sR = (I3 * np.float32(1.05)).astype(np.float32)             # (dist3D = 10.5: inside dot_below_half's 0.8f*8 .. 1.2f*9)
    pr = K.projection(I3, z3, Kc, sR=sR, t2=np.float32([0.01, -0.02, 0.03]), invz_double=True, angle=False, dist_point=True)
    w3 = K.ref_project(ref, tab, np.arange(n), np.zeros(n, np.uint8), pr, bounds, sf, 7.5)
    assert w3['valid'][names['dot_below_half']] == 1
    K.check_projection(matcher.project_keyframe(kf, lm, K.api_projection(api, pr), np.arange(n), np.zeros(n, np.uint8), sf, 7.5), w3)
    lm.close()
    kf.close()


@pytest.mark.parametrize('W,H,nfeat', [(640, 480, 500), (1920, 1080, 2000)])
@pytest.mark.parametrize('fn', K.FUNCS)
def test_fused_equals_oracle_and_two_step(api, matcher, ref, oracle, fn, W, H, nfeat):
    kA, dA, kB, dB, sf = _frames(api, W, H, nfeat)
    info = {}
    for th in K.CASES[fn]:
        sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=K.case_seed(fn, th, W))
        frames = dict(A=matcher.frame(kA, dA, sc['bounds']), B=matcher.frame(kB, dB, sc['bounds']))
        lm = _table(api, matcher, sc['tab'])
        _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, th, kA, dA, kB, dB, sf, W, info)
        lm.close()
        for f in frames.values():
            f.close()
    K.assert_branches(fn, info)


def test_row_updates_between_calls_and_second_call(api, matcher, ref, oracle):
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(api, W, H, 2000)
    fn, th = K.FUSE_SCW, 4.0
    sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=91)
    frames = dict(A=matcher.frame(kA, dA, sc['bounds']), B=matcher.frame(kB, dB, sc['bounds']))
    lm = _table(api, matcher, sc['tab'])
    info = {}
    _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, th, kA, dA, kB, dB, sf, W, info)
    rng = np.random.default_rng(92)
    n = sc['nA']
    r1 = rng.choice(n, n // 20, replace=False).astype(np.int32)          # 5 % of the MapPoints move
    sc['tab']['pos'][r1] = (sc['tab']['pos'][r1] * np.float32(1.002)).astype(np.float32)
    lm.set_rows(r1, pos=sc['tab']['pos'][r1])
    r2 = rng.choice(n, n // 20, replace=False).astype(np.int32)          # 5 % of the descriptors are recomputed
    sc['tab']['desc'][r2] = rng.integers(0, 256, (len(r2), 32), dtype=np.uint8)
    lm.set_rows(r2, desc=sc['tab']['desc'][r2])
    _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, th, kA, dA, kB, dB, sf, W, info)
    # the same keyframe a second time with another th and another function, nothing sent in between
    _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, 10.0, kA, dA, kB, dB, sf, W, info)
    _check_case(api, matcher, ref, oracle, frames, lm, K.SIM3, sc, 7.5, kA, dA, kB, dB, sf, W, info)
    lm.close()
    for f in frames.values():
        f.close()


def test_more_points_than_one_bookkeeping_chunk(api, matcher, ref, oracle):
    """> 2 048 points with claim = 1: the bookkeeping kernel runs several chunks, a keypoint claimed in one is taken in the next"""
    W, H = 1920, 1080
    kA, dA, kB, dB, sf = _frames(api, W, H, 2000)
    sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=93)
    case = K.make_case(ref, K.SBP_SCW, sc, 10)
    d = dict(case['dirs'][0])
    rng = np.random.default_rng(94)
    order = np.concatenate([rng.permutation(len(d['rows'])) for _ in range(3)])
    d['rows'], d['flags'] = d['rows'][order], d['flags'][order]
    assert len(order) > 2 * 2048
    frames = dict(B=matcher.frame(kB, dB, sc['bounds']))
    lm = _table(api, matcher, sc['tab'])
    want_proj = K.ref_project(ref, sc['tab'], d['rows'], d['flags'], d['pr'], sc['bounds'], sf, 10)
    nm, bi, bd = K.cpu_search(oracle, d, want_proj, sc, kB, dB, sf)
    got = _fused(api, matcher, frames, lm, d, sf, 10)
    K.check_projection(got, want_proj)
    assert got['nmatches'] == nm and (got['best_idx'] == bi).all() and (got['best_dist'] == bd).all()
    hit = bi[bi >= 0]
    assert len(hit) > 500 and len(np.unique(hit)) == len(hit)           # claimed once each
    proj2, (n2, bi2, bd2) = _two_step(api, matcher, frames, lm, sc, d, sf, 10)
    assert n2 == nm and (bi2 == bi).all()
    lm.close()
    frames['B'].close()


def test_errors_leave_everything_usable(api, ref, oracle):
    W, H = 640, 480
    kA, dA, kB, dB, sf = _frames(api, W, H, 500)
    fn, th = K.FUSE, 3.0
    sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=K.case_seed(fn, th, W))
    matcher, other = api.Matcher(0), api.Matcher(0)
    frames = dict(A=matcher.frame(kA, dA, sc['bounds']), B=matcher.frame(kB, dB, sc['bounds']))
    lm = _table(api, matcher, sc['tab'])
    info = {}
    d = K.make_case(ref, fn, sc, th)['dirs'][0]
    acam = K.api_projection(api, d['pr'])
    rows, flags = d['rows'], d['flags']

    def fails(f, *a, **kw):
        with pytest.raises(api.OrbfeError) as e:
            f(*a, **kw)
        assert e.value.code == -1   # ORBFE_ERR_INVALID
    # a matcher that does not own the map
    okf = other.frame(kB, dB, sc['bounds'])
    fails(other.project_keyframe, okf, lm, acam, rows, flags, sf, th)
    fails(other.search_projected_keyframe, okf, lm, acam, rows, flags, sf, th)
    # a projected row outside the table (a flagged point may carry anything: the cases' NULL candidates carry 1 << 30)
    assert ((flags & K.MP_SKIP) != 0).any() and (rows[(flags & K.MP_SKIP) != 0] == 1 << 30).any()
    i = int(np.flatnonzero(flags == 0)[3])
    bad_rows = rows.copy()
    bad_rows[i] = sc['M']
    fails(matcher.project_keyframe, frames['B'], lm, acam, bad_rows, flags, sf, th)
    fails(matcher.search_projected_keyframe, frames['B'], lm, acam, bad_rows, flags, sf, th)
    bad_rows[i] = -1
    fails(matcher.search_projected_keyframe, frames['B'], lm, acam, bad_rows, flags, sf, th)
    # more than 32 levels; the viewing-angle test without a camera centre
    fails(matcher.project_keyframe, frames['B'], lm, acam, rows, flags, np.ones(33, np.float32), th)
    pr = dict(d['pr'])
    pr['dist_point'] = True
    fails(matcher.project_keyframe, frames['B'], lm, K.api_projection(api, pr), rows, flags, sf, th)
    # LEVEL CONTRACT: a valid point whose predicted level is >= nlevels (mfMaxDistance = dist * 1.2^9)
    proj = K.ref_project(ref, sc['tab'], rows, flags, d['pr'], sc['bounds'], sf, th)
    s = int(np.flatnonzero(proj['valid'] == 1)[5])
    row = int(rows[s])
    dist = K.U._norm((sc['tab']['pos'][row] - d['pr']['Ow'])[None].astype(np.float32))[0]
    keep = sc['tab']['min'][row], sc['tab']['max'][row]
    sc['tab']['min'][row], sc['tab']['max'][row] = 0.0, dist * np.float32(1.2 ** 9)
    lm.set_rows([row], min_raw=np.float32([0.0]), max_raw=np.float32([sc['tab']['max'][row]]))
    want = K.ref_project(ref, sc['tab'], rows, flags, d['pr'], sc['bounds'], sf, th)
    assert want['valid'][s] == 1 and want['level'][s] >= len(sf) and want['radius'][s] == 0
    K.check_projection(matcher.project_keyframe(frames['B'], lm, acam, rows, flags, sf, th), want)   # reported as it is
    res = None
    with pytest.raises(api.OrbfeError) as e:
        res = matcher.search_projected_keyframe(frames['B'], lm, acam, rows, flags, sf, th, inv_sigma2=_inv_sigma2(sf))
    assert e.value.code == -1 and res is None
    # the C call's nmatches is 0 on that failure
    import ctypes as C
    rows32, sf32 = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(sf, np.float32)
    bi = np.full(len(rows32), -1, np.int32)
    cnm, cnv = C.c_int(7), C.c_int(7)
    rc = matcher.L.orbfe_search_projected_keyframe_frame(matcher.h, frames['B'].h, lm.h, C.byref(acam), K._p(rows32), K._p(flags),
                                                         len(rows32), K._p(sf32), len(sf32), th, None, 0, None, 5.99, 50, None, None,
                                                         None, K._p(bi), None, C.byref(cnm), C.byref(cnv))
    assert rc == -1 and cnm.value == 0
    # the next valid calls on the same handles succeed and are exact
    sc['tab']['min'][row], sc['tab']['max'][row] = keep
    lm.set_rows([row], min_raw=np.float32([keep[0]]), max_raw=np.float32([keep[1]]))
    _check_case(api, matcher, ref, oracle, frames, lm, fn, sc, th, kA, dA, kB, dB, sf, W, info)
    # n = 0 / an empty keyframe
    r = matcher.search_projected_keyframe(frames['B'], lm, acam, rows[:0], flags[:0], sf, th)
    assert r['nmatches'] == 0 and r['n_valid'] == 0 and len(r['best_idx']) == 0
    assert matcher.project_keyframe(frames['B'], lm, acam, rows[:0], flags[:0], sf, th)['n_valid'] == 0
    e0 = matcher.frame(kB[:0], dB[:0], sc['bounds'])
    r = matcher.search_projected_keyframe(e0, lm, acam, rows, flags, sf, th)
    assert r['nmatches'] == 0 and (r['best_idx'] == -1).all() and r['n_valid'] == proj['n_valid']
    for h in (e0, lm, okf, frames['A'], frames['B']):
        h.close()
    other.close()
    matcher.close()


def test_out_of_range_level_in_the_second_block(api, matcher, ref, oracle):
    """Fuse on the 500-feature frames: two 256-lane blocks, the second one partial.  Two valid points of the second block
    predict a level >= nlevels (mfMaxDistance = dist * 1.2^9): the fused call fails naming the lower of them, the projection
    alone reports both as they are, and with the two flagged ORBFE_MP_SKIP the fused call equals the oracle."""
    W, H = 640, 480
    kA, dA, kB, dB, sf = _frames(api, W, H, 500)
    fn, th = K.FUSE, 3.0
    sc = K.scene(kA, dA, kB, dB, sf, W, H, seed=K.case_seed(fn, th, W))
    d = K.make_case(ref, fn, sc, th)['dirs'][0]
    rows, flags = d['rows'], d['flags']
    n = len(rows)
    assert 256 < n <= 512
    proj = K.ref_project(ref, sc['tab'], rows, flags, d['pr'], sc['bounds'], sf, th)
    named_once = np.array([(rows == r).sum() == 1 for r in rows])
    cand = np.flatnonzero((proj['valid'] == 1) & named_once & (np.arange(n) >= 256))
    assert len(cand) >= 4
    lo, hi = int(cand[1]), int(cand[3])
    for s in (hi, lo):
        row = int(rows[s])
        dist = K.U._norm((sc['tab']['pos'][row] - d['pr']['Ow'])[None].astype(np.float32))[0]
        sc['tab']['min'][row], sc['tab']['max'][row] = 0.0, dist * np.float32(1.2 ** 9)
    frames = dict(B=matcher.frame(kB, dB, sc['bounds']))
    lm = _table(api, matcher, sc['tab'])
    want = K.ref_project(ref, sc['tab'], rows, flags, d['pr'], sc['bounds'], sf, th)
    outside = (want['valid'] == 1) & ((want['level'] < 0) | (want['level'] >= len(sf)))
    assert np.flatnonzero(outside).tolist() == [lo, hi]
    with pytest.raises(api.OrbfeError) as e:
        _fused(api, matcher, frames, lm, d, sf, th)
    assert e.value.code == -1
    assert 'MapPoint %d: predicted level outside [0, %d)' % (lo, len(sf)) in str(e.value)
    K.check_projection(matcher.project_keyframe(frames['B'], lm, K.api_projection(api, d['pr']), rows, flags, sf, float(th)), want)
    d2 = dict(d)
    d2['flags'] = flags.copy()
    d2['flags'][[lo, hi]] |= K.MP_SKIP
    want = K.ref_project(ref, sc['tab'], rows, d2['flags'], d['pr'], sc['bounds'], sf, th)
    nm, bi, bd = K.cpu_search(oracle, d2, want, sc, kB, dB, sf)
    got = _fused(api, matcher, frames, lm, d2, sf, th)
    K.check_projection(got, want)
    assert got['nmatches'] == nm and nm > 0 and (got['best_idx'] == bi).all() and (got['best_dist'] == bd).all()
    lm.close()
    frames['B'].close()


def test_facade_sequence(api, tmp_path):
    """tests/cpp/keyframe_projection_test.cpp: the four new shim templates on facade_pose_test's mock model, every call equal to
    the oracle's whole function and to the host-projection template it stands in for"""
    import keyframe_projection_facade as F
    exe = F.compile_test(str(tmp_path / 'keyframe_projection_test'))
    stats = F.run(exe)
    assert stats['sbp_scw'] > 100 and stats['fuse'] > 100 and stats['fuse_scw'] > 100 and stats['sim3'] > 60
    assert stats['rows_sent'] > 0
