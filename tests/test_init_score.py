"""Initialiser scoring without a GPU: the C++ restatement (tests/cpp/init_score_ref.cpp) and the numpy restatement
(tests/init_score_util.py) agree bit for bit on every scene; the scenes are sharp enough for the GPU tests that rely on them
(a reordered or double-accumulated sum, a contracted multiply-add and every crafted hypothesis show in the expected values);
the C++ side compiles against the stubs."""
import os
import subprocess

import numpy as np
import pytest

import init_score_util as U

ROOT = U.ROOT
CPP = os.path.join(ROOT, 'tests', 'cpp')
f32 = np.float32


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('init_score_ref'))


@pytest.fixture(scope='module')
def scenes(ref):
    return U.scenes(ref)


@pytest.fixture(scope='module')
def full(ref, scenes):
    """The restatement's results on the whole of each scene with the K_MAX set."""
    return [U.ref_find(ref, s['pts'], U.SIGMA, *sets['k200']) for s, sets in scenes]


def test_chunk_constant_matches_the_kernel():
    assert U.kernel_constant('kChunk') == U.LDS_CHUNK


def test_restatements_agree(ref, scenes):
    for s, sets in scenes:
        for name, (H21, H12, F21) in sets.items():
            for n in (U.N_MAX, 257, 8, 1, 0) if name == 'k200' else (U.N_MAX, 65):
                pts = s['pts'][:n]
                a = U.ref_find(ref, pts, U.SIGMA, H21, H12, F21)
                b = U.np_find(pts, U.SIGMA, H21, H12, F21)
                what = '%s %s n=%d' % (s['name'], name, n)
                # scores as uint32; NaN scores (crafted) by class
                U.assert_same(b, a, what)
                fin = ~np.isnan(a.scores_h)
                assert (U.bits(a.scores_h)[fin] == U.bits(b.scores_h)[fin]).all(), what
                fin = ~np.isnan(a.scores_f)
                assert (U.bits(a.scores_f)[fin] == U.bits(b.scores_f)[fin]).all(), what


def test_scenes_have_a_model_that_fits(scenes, full):
    (planar, _), (general, _) = scenes
    rp, rg = full
    # planar scene: some homography explains most good matches; general scene: some fundamental matrix does
    assert rp.inliers_h.sum() > 0.8 * planar['good'].sum()
    assert rg.inliers_f.sum() > 0.8 * general['good'].sum()
    assert rg.inliers_h.sum() < 0.5 * general['good'].sum()
    for s, r in ((planar, rp), (general, rg)):
        wrong = (~s['good']).mean()
        assert 0.25 < wrong < 0.35
        assert r.inliers_f[~s['good']].mean() < 0.2


def _sums(scene, sets, model):
    H21, H12, F21 = sets['k200']
    seq, pair, dbl = [], [], []
    for k in range(U.K_MAX):
        c1, c2, _ = U.np_terms_h(scene['pts'], H21[k], H12[k], U.SIGMA) if model == 'h' else U.np_terms_f(scene['pts'], F21[k], U.SIGMA)
        t = U.interleave(c1, c2)
        with np.errstate(all='ignore'):
            seq.append(U.ordered_sum(t))
            pair.append(f32(np.sum(t, dtype=f32)))                    # numpy's pairwise float sum
            dbl.append(f32(np.sum(t.astype(np.float64))))             # accumulated in double, rounded once
    return np.array(seq, f32), np.array(pair, f32), np.array(dbl, f32)


@pytest.mark.parametrize('model', ['h', 'f'])
def test_summation_order_shows(scenes, model):
    for s, sets in scenes:
        seq, pair, dbl = _sums(s, sets, model)
        fin = np.isfinite(seq)
        assert (U.bits(seq)[fin] != U.bits(pair)[fin]).any(), '%s: a pairwise sum gives the same bits everywhere' % s['name']
        assert (U.bits(seq)[fin] != U.bits(dbl)[fin]).any(), '%s: a double-accumulated sum gives the same bits everywhere' % s['name']


def test_crafted_hypotheses(ref, scenes, full):
    for (s, sets), r in zip(scenes, full):
        H21, H12, F21 = sets['k200']
        pts = s['pts']
        # tie: the copies score the same bits and the lowest index wins
        for sc, best in ((r.scores_h, r.best_h), (r.scores_f, r.best_f)):
            assert U.bits(sc)[U.I_TIE_LO] == U.bits(sc)[U.I_BEST] == U.bits(sc)[U.I_TIE_HI]
            assert sc[U.I_BEST] == np.nanmax(sc) and best == U.I_TIE_LO
        # an all-zero H12: NaN, never the winner although it stands in front of the winner
        assert np.isnan(r.scores_h[U.I_ZERO_H12]) and U.I_ZERO_H12 < r.best_h
        # a point on H21's line at infinity: an infinite distance, the match is rejected, the score stays finite
        inl = np.ones(len(pts), np.uint8)
        sc = ref.isr_check_homography(U._p(pts), len(pts), U._p(H21[U.I_INF_H21]), U._p(H12[U.I_INF_H21]), U.SIGMA, U._p(inl))
        assert np.isfinite(sc) and inl[U.INF_MATCH] == 0
        with np.errstate(all='ignore'):
            h = H21[U.I_INF_H21]
            p = pts[U.INF_MATCH]
            assert h[6] * p[0] + h[7] * p[1] + h[8] == 0 and np.isinf(f32(np.float64(1.0) / np.float64(h[6] * p[0] + h[7] * p[1] + h[8])))
        # an all-zero F21: 0/0
        assert np.isnan(r.scores_f[U.I_ZERO_F]) and U.I_ZERO_F < r.best_f
        # F21 * 1e-25: the squares underflow to 0, 0/0; a milder scale lands on denormals
        d2, d1 = U.np_terms_f(pts, F21[U.I_TINY_F], U.SIGMA, detail=True)[3:]
        assert (d2 == 0).any() and (d1 == 0).any() and np.isnan(r.scores_f[U.I_TINY_F])
        d2, d1 = U.np_terms_f(pts, F21[U.I_DENORM_F], U.SIGMA, detail=True)[3:]
        tiny = np.finfo(f32).tiny
        assert ((d2 > 0) & (d2 < tiny)).sum() > 100 and ((d1 > 0) & (d1 < tiny)).sum() > 100
        # nothing above 0
        n = U.ref_find(ref, pts, U.SIGMA, *sets['nothing'])
        assert n.best_h == -1 and n.best_f == -1 and n.score_h == 0 and n.score_f == 0
        assert not n.inliers_h.any() and not n.inliers_f.any()
        assert (n.scores_h[:2] == 0).all() and np.isnan(n.scores_h[2]) and n.scores_f[0] == 0 and np.isnan(n.scores_f[1])


def test_contraction_shows(ref, scenes, full, tmp_path):
    if 'fma' not in open('/proc/cpuinfo').read().split():
        pytest.skip('no FMA on this CPU: a contracted build cannot be run')
    fused = U.build_ref(tmp_path, flags=('-O2', '-ffp-contract=fast', '-mfma'), name='init_score_ref_fma.so')
    for (s, sets), r in zip(scenes, full):
        g = U.ref_find(fused, s['pts'], U.SIGMA, *sets['k200'])
        for a, b in ((r.scores_h, g.scores_h), (r.scores_f, g.scores_f)):
            fin = np.isfinite(a) & np.isfinite(b)
            assert (U.bits(a)[fin] != U.bits(b)[fin]).any(), '%s: contraction changes no score' % s['name']


def test_compaction(ref):
    s = U.make_scene(True, 5, n=300)
    k1, k2, m12 = U.keypoint_form(s['pts'], 3)
    assert (m12 < 0).sum() == 37 and len(k2) == len(k1) + 5
    xy1, xy2 = np.stack([k1['x'], k1['y']], 1), np.stack([k2['x'], k2['y']], 1)
    assert np.array_equal(U.ref_compact(ref, xy1, xy2, m12), s['pts'])


def test_header_and_facade_compile():
    """include/orbfe/orb_shim.hpp's ScoreInitializerHypotheses with the reference's types (cv::KeyPoint, cv::Mat of the stubs) and
    with the test program's own types."""
    for defs in (['-DINIT_SCORE_CV_TYPES'], []):
        subprocess.check_call(['g++', '-std=c++17', '-fsyntax-only', '-Wall', '-Werror'] + defs +
                              ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(CPP, 'opencv_stub'),
                               os.path.join(CPP, 'init_score_test.cpp')])
