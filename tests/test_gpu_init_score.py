"""orbfe_score_init_hypotheses* on the GPU against the restatement tests/cpp/init_score_ref.cpp, bit for bit: scores (NaN by
class), winners, winning scores and both masks over the shape sweep with the crafted hypotheses, the three entry points on the
same data, argument errors, the C++ facade and a chain from extraction through SearchForInitialization."""
import ctypes as C

import numpy as np
import pytest

import init_score_util as U

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('init_score_ref'))


@pytest.fixture(scope='module')
def scenes(ref):
    return U.scenes(ref)


@pytest.fixture(scope='module')
def matcher():
    from os1_amd import api
    m = api.Matcher(0)
    yield m
    m.close()


def _models(H21, H12, F21):
    return (('both', H21, H12, F21), ('h', H21, H12, None), ('f', None, None, F21))


@pytest.mark.parametrize('n', U.SWEEP_N)
def test_shape_sweep(ref, scenes, matcher, n):
    """Every N with K in {1, 3, 200}, both models / H only / F only, on both scenes; the K = 200 set holds every crafted hypothesis,
    the K = 3 set a NaN score in front of a tie, and the 'nothing' set has no score above 0."""
    for s, sets in scenes:
        pts = s['pts'][:n]
        for name in ('k1', 'k3', 'k200', 'nothing'):
            for tag, H21, H12, F21 in _models(*sets[name]):
                want = U.ref_find(ref, pts, U.SIGMA, H21, H12, F21)
                got = matcher.score_init_hypotheses(pts, U.SIGMA, H21, H12, F21)
                U.assert_same(got, want, '%s n=%d %s %s' % (s['name'], n, name, tag))
                assert got.n_matches == n
                if tag == 'h':
                    assert got.scores_f is None and got.best_f is None
        if n == U.N_MAX:   # the crafted cases did what they were built for, on the GPU's own numbers
            g = matcher.score_init_hypotheses(pts, U.SIGMA, *sets['k200'])
            assert g.best_h == U.I_TIE_LO and g.best_f == U.I_TIE_LO
            assert np.isnan(g.scores_h[U.I_ZERO_H12]) and np.isnan(g.scores_f[U.I_ZERO_F]) and np.isnan(g.scores_f[U.I_TINY_F])
            assert np.isfinite(g.scores_h[U.I_INF_H21])
            g = matcher.score_init_hypotheses(pts, U.SIGMA, *sets['nothing'])
            assert g.best_h == -1 and g.best_f == -1 and g.score_h == 0 and g.score_f == 0
            assert not g.inliers_h.any() and not g.inliers_f.any()


def test_inf_hypothesis_wins_and_rejects_its_match(ref, scenes, matcher):
    """The H21 with a match on its line at infinity, alone.  It wins (its H12 is the best hypothesis', so the first term of most
    matches counts), and the mask that comes back is its own: the match on the line is rejected by an infinite distance; the
    other matches are rejected by finite ones, because a line at infinity that crosses the image throws every point far away."""
    s, sets = scenes[0]
    H21, H12, _ = sets['k200']
    pts = s['pts'][:257]
    a, b = H21[[U.I_INF_H21]], H12[[U.I_INF_H21]]
    want = U.ref_find(ref, pts, U.SIGMA, a, b, None)
    got = matcher.score_init_hypotheses(pts, U.SIGMA, a, b, None)
    U.assert_same(got, want, 'inf')
    assert want.best_h == 0 and got.best_h == 0 and got.score_h > 0 and np.isfinite(got.score_h)
    assert not got.inliers_h[U.INF_MATCH] and not want.inliers_h.any()


def test_three_entry_points_agree(ref, scenes, matcher):
    from os1_amd import api
    for (s, sets), n in zip(scenes, (U.LDS_CHUNK + 1, 300)):
        pts = s['pts'][:n]
        k1, k2, m12 = U.keypoint_form(pts, 3)
        assert (m12 < 0).sum() == 37
        xy1, xy2 = np.stack([k1['x'], k1['y']], 1), np.stack([k2['x'], k2['y']], 1)
        assert np.array_equal(U.ref_compact(ref, xy1, xy2, m12), pts)
        rng = np.random.default_rng(1)
        bounds = (0.0, 640.0, 0.0, 480.0)
        f1 = matcher.frame(k1, rng.integers(0, 256, (len(k1), 32), dtype=np.uint8), bounds)
        f2 = matcher.frame(k2, rng.integers(0, 256, (len(k2), 32), dtype=np.uint8), bounds)
        try:
            for tag, H21, H12, F21 in _models(*sets['k200']):
                want = U.ref_find(ref, pts, U.SIGMA, H21, H12, F21)
                a = matcher.score_init_hypotheses(pts, U.SIGMA, H21, H12, F21)
                b = matcher.score_init_hypotheses_kps(k1, k2, m12, U.SIGMA, H21, H12, F21)
                c = matcher.score_init_hypotheses_frames(f1, f2, m12, U.SIGMA, H21, H12, F21)
                for got, form in ((a, 'pts'), (b, 'kps'), (c, 'frames')):
                    U.assert_same(got, want, '%s %s %s' % (s['name'], form, tag))
                    assert got.n_matches == n
            # no match at all
            none = np.full(len(k1), -1, np.int32)
            for got in (matcher.score_init_hypotheses_kps(k1, k2, none, U.SIGMA, *sets['k3']),
                        matcher.score_init_hypotheses_frames(f1, f2, none, U.SIGMA, *sets['k3'])):
                assert got.n_matches == 0 and got.best_h == -1 and got.best_f == -1 and got.score_h == 0 and got.score_f == 0
                assert (got.scores_h == 0).all() and (got.scores_f == 0).all() and len(got.inliers_h) == 0
        finally:
            f1.close()
            f2.close()


def test_argument_errors_leave_outputs_untouched(scenes, matcher):
    from os1_amd import api
    L = api.load_library()
    s, sets = scenes[0]
    H21, H12, F21 = sets['k3']
    pts = np.ascontiguousarray(s['pts'][:65])
    k1, k2, m12 = U.keypoint_form(pts, 3)
    rng = np.random.default_rng(2)
    bounds = (0.0, 640.0, 0.0, 480.0)
    f1 = matcher.frame(k1, rng.integers(0, 256, (len(k1), 32), dtype=np.uint8), bounds)
    f2 = matcher.frame(k2, rng.integers(0, 256, (len(k2), 32), dtype=np.uint8), bounds)
    p = U._p

    def outs():
        o = [np.full(8, 7.5, f32), np.full(8, 7.5, f32), np.full(1, 77, np.int32), np.full(1, 77, np.int32), np.full(1, 7.5, f32),
             np.full(1, 7.5, f32), np.full(len(k1), 9, np.uint8), np.full(len(k1), 9, np.uint8)]
        return o, [x.copy() for x in o]

    def call(form, K, h21, h12, f21_, m=None, fa=None, fb=None):
        o, before = outs()
        nm = C.c_int(-5)
        tail = [U.SIGMA, K, p(h21), p(h12), p(f21_)] + [p(x) for x in o]
        if form == 'pts':
            rc = L.orbfe_score_init_hypotheses(matcher.h, p(pts), len(pts), *tail)
        elif form == 'kps':
            rc = L.orbfe_score_init_hypotheses_kps(matcher.h, p(k1), len(k1), p(k2), len(k2), p(m), *tail, C.byref(nm))
        else:
            rc = L.orbfe_score_init_hypotheses_frames(matcher.h, fa.h, fb.h, p(m), *tail, C.byref(nm))
        assert rc == -1, (form, rc)
        assert b'invalid' in L.orbfe_last_error()
        assert all(np.array_equal(x, y) for x, y in zip(o, before)) and nm.value == -5, form

    try:
        for form in ('pts', 'kps', 'frames'):
            kw = dict(m=m12, fa=f1, fb=f2)
            call(form, 0, H21, H12, F21, **kw)          # n_hyp < 1
            call(form, -3, H21, H12, F21, **kw)
            call(form, 3, H21, None, F21, **kw)         # only one of H21 / H12
            call(form, 3, None, H12, F21, **kw)
            call(form, 3, None, H12, None, **kw)
        for form in ('kps', 'frames'):
            for v in (len(k2), -2, 1 << 30):            # a matches12 index outside [-1, n2)
                bad = m12.copy()
                bad[len(bad) // 2] = v
                call(form, 3, H21, H12, F21, m=bad, fa=f1, fb=f2)
        if api.device_count() >= 2:                     # frames on another device than the matcher (needs a second GPU)
            other = api.Matcher(1)
            g1 = other.frame(k1, rng.integers(0, 256, (len(k1), 32), dtype=np.uint8), bounds)
            try:
                call('frames', 3, H21, H12, F21, m=m12, fa=g1, fb=f2)
                call('frames', 3, H21, H12, F21, m=m12, fa=f1, fb=g1)
            finally:
                g1.close()
                other.close()
        # and the handle still works
        got = matcher.score_init_hypotheses_frames(f1, f2, m12, U.SIGMA, H21, H12, F21)
        assert got.n_matches == len(pts)
    finally:
        f1.close()
        f2.close()


def test_facade(ref, scenes, tmp_path):
    exe = U.compile_facade(str(tmp_path / 'init_score_test'))
    files = []
    for (s, sets), n, name in zip(scenes, (U.LDS_CHUNK + 1, 300), ('k200', 'k3')):
        pts = s['pts'][:n]
        k1, k2, m12 = U.keypoint_form(pts, 4)
        pairs = np.stack([np.nonzero(m12 >= 0)[0], m12[m12 >= 0]], 1)
        xy1, xy2 = np.stack([k1['x'], k1['y']], 1), np.stack([k2['x'], k2['y']], 1)
        files.append(U.write_scene(str(tmp_path / ('%s.bin' % s['name'])), xy1, xy2, pairs, U.SIGMA, *sets[name]))
    s, sets = scenes[1]
    k1, k2, m12 = U.keypoint_form(s['pts'][:64], 5)
    pairs = np.stack([np.nonzero(m12 >= 0)[0], m12[m12 >= 0]], 1)
    xy1, xy2 = np.stack([k1['x'], k1['y']], 1), np.stack([k2['x'], k2['y']], 1)
    files.append(U.write_scene(str(tmp_path / 'f_only.bin'), xy1, xy2, pairs, U.SIGMA, None, None, sets['k200'][2]))
    files.append(U.write_scene(str(tmp_path / 'nothing.bin'), xy1, xy2, pairs, U.SIGMA, *sets['nothing']))
    lines = U.run_facade(exe, files)
    assert lines[-2] == 'scenes 4 mismatches 0'


def test_chain_from_extraction(ref, matcher):
    """Two shifted synthetic VGA frames: extract, SearchForInitialization, resident frames, score on the frames with the search's
    own matches12; the restatement gets the keypoints as the frames hold them."""
    from os1_amd import api
    from os1_amd.synth import shifted, synth
    A = synth(1, 640, 480)
    B = shifted(A, -6, 2, 1)
    ex = api.Extractor(1000, 1.2, 8, 20, 7, device=0)
    (k1, d1), (k2, d2) = ex(A), ex(B)
    bounds = (0.0, 640.0, 0.0, 480.0)
    prev = np.stack([k1['x'], k1['y']], 1)
    nm, m12, _ = matcher.search_for_initialization(k1, d1, k2, d2, bounds, prev, 100, 0.9, True)
    assert nm >= 100
    f1, f2 = matcher.frame(k1, d1, bounds), matcher.frame(k2, d2, bounds)
    try:
        dk1, dk2 = f1.download()[0], f2.download()[0]
        pts = U.ref_compact(ref, np.stack([dk1['x'], dk1['y']], 1), np.stack([dk2['x'], dk2['y']], 1), m12)
        assert len(pts) == nm
        H21, H12, F21 = U.random_hypotheses({'pts': pts}, 50, 9) if nm >= 257 else U.random_hypotheses({'pts': np.tile(pts, (3, 1))}, 50, 9)
        want = U.ref_find(ref, pts, U.SIGMA, H21, H12, F21)
        got = matcher.score_init_hypotheses_frames(f1, f2, m12, U.SIGMA, H21, H12, F21)
        U.assert_same(got, want, 'chain')
        assert got.n_matches == nm and got.best_h >= 0 and got.inliers_h.sum() > nm // 2   # a pure shift: a homography fits
    finally:
        f1.close()
        f2.close()
        ex.close()
