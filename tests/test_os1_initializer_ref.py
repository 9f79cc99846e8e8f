"""The Initializer's hypothesis scoring pinned to the reference's own compiled src/Initializer.cc (oracle/_ref/libos1_initializer.so,
built by oracle/Makefile where the reference exists; oracle/os1_initializer_wrap.cpp reaches CheckHomography and CheckFundamental and
nothing else).  On the boundary inputs and on the existing crafted hypotheses over the N / K sweep: the reference object ==
tests/cpp/init_score_ref.cpp == the numpy restatement, on scores (bit for bit, NaN by class), winners and both masks.  Where the
library is absent the same assertions run against the recorded results of tests/golden/os1_initializer_outputs.npz
(tools/gen_os1_initializer_golden.py); where both exist the recording is held to the library, and the stub counter is 0 after
every call."""
import numpy as np
import pytest

import init_score_util as U

f32 = np.float32


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('init_score_ref'))


@pytest.fixture(scope='module')
def cases(ref):
    return {c[0]: c[1:] for c in U.sweep_cases(ref)}


def test_reference_source(ref):
    print('\nos1 initializer reference: %s' % ('oracle/_ref/libos1_initializer.so' if U.have_os1() else 'tests/golden/os1_initializer_outputs.npz'))
    g = U.golden()
    assert g is not None, 'tests/golden/os1_initializer_outputs.npz is missing: run tools/gen_os1_initializer_golden.py'
    if U.have_os1():
        rec = U.golden_records(ref)
        z = np.load(U.GOLDEN)
        assert set(rec) == set(z.files) and all(rec[k].tobytes() == z[k].tobytes() and rec[k].dtype == z[k].dtype for k in rec), \
            'the golden is stale: run tools/gen_os1_initializer_golden.py'
        assert U.os1().stub_calls() == 0


def _reference(key, pts, H21, H12, F21):
    if U.have_os1():
        return U.os1_find(pts, U.SIGMA, H21, H12, F21)          # asserts the stub counter
    return U.result_from_fields(U.golden()[key], len(pts))


@pytest.mark.parametrize('n', U.SWEEP_N)
def test_sweep_reference_object_equals_both_restatements(ref, cases, n):
    for scene in ('planar', 'general'):
        for name in ('k1', 'k3', 'k200', 'nothing'):
            key = '%s/n%d/%s' % (scene, n, name)
            pts, H21, H12, F21 = cases[key]
            want = _reference(key, pts, H21, H12, F21)
            U.assert_same(U.result_from_fields(U.golden()[key], len(pts)), want, key + ' recording')
            U.assert_same(U.ref_find(ref, pts, U.SIGMA, H21, H12, F21), want, key + ' init_score_ref.cpp')
            if name != 'k200' or n <= U.LDS_CHUNK + 1:          # the numpy restatement on all but the two largest K = 200 cases per scene
                U.assert_same(U.np_find(pts, U.SIGMA, H21, H12, F21), want, key + ' numpy')


def test_boundary_inputs(ref):
    b = U.boundary_set()
    g = U.golden()['boundary']
    assert g['pts'].tobytes() == b['pts'].tobytes()
    rec = (g['scores_h'], g['masks_h'], g['scores_f'], g['masks_f'])
    witnesses = [('init_score_ref.cpp', U.boundary_masks(U.RefChecks(ref), b)), ('numpy', U.boundary_masks(U.NumpyChecks(), b))]
    if U.have_os1():
        witnesses.append(('reference object', U.boundary_masks(U.os1(), b)))
        assert U.os1().stub_calls() == 0
    for who, (sh, mh, sf, mf) in witnesses:
        assert U.same_scores(sh, rec[0]) and U.same_scores(sf, rec[2]), who
        assert np.array_equal(mh, rec[1]) and np.array_equal(mf, rec[3]), who
    sh, mh, sf, mf = rec
    # H: `chiSquare > th` -- AT the threshold is an inlier that adds +0 twice, one ulp above is rejected, one ulp below adds one ulp of th twice
    c1, c2, inl = U.np_terms_h(b['pts'], b['H21'][U.I_B_IDENT], b['H12'][U.I_B_IDENT], U.SIGMA)
    assert mh[U.I_B_IDENT, [U.M_H_AT, U.M_H_ABOVE, U.M_H_BELOW]].tolist() == [True, False, True]
    assert c1[U.M_H_AT] == 0 and c2[U.M_H_AT] == 0 and c1[U.M_H_ABOVE] == 0
    assert c1[U.M_H_BELOW] == U.TH_H - U._ulp_walk(U.TH_H, -1) > 0
    # F: the same at 3.841f; an inlier AT th adds 5.991f - 3.841f
    c1, c2, inl = U.np_terms_f(b['pts'], b['F21'][U.I_B_SIDE], U.SIGMA)
    assert b['facts']['f_at'] is not None                 # fl(d*d) == 3.841f has a solution: d = 1.959847f
    assert mf[U.I_B_SIDE, [U.M_F_BELOW, U.M_F_ABOVE, U.M_F_AT]].tolist() == [True, False, True]
    assert c1[U.M_F_AT] == c2[U.M_F_AT] == f32(5.991) - f32(3.841) and c1[U.M_F_ABOVE] == 0
    below = f32(b['facts']['f_below'] * b['facts']['f_below'])   # squares of neighbouring floats are about two ulps of th apart
    assert U._ulp_walk(U.TH_F, -3) <= below < U.TH_F and c1[U.M_F_BELOW] == f32(5.991) - below
    # an inlier in one direction only: rejected, and the accepted direction still adds to the score
    c1, c2, inl = U.np_terms_f(b['pts'], b['F21'][U.I_B_ASYM], U.SIGMA)
    assert c1[U.M_F_ONE_DIR] == 0 and c2[U.M_F_ONE_DIR] > 0 and not mf[U.I_B_ASYM, U.M_F_ONE_DIR]
    c1, c2, inl = U.np_terms_h(b['pts'], b['H21'][U.I_B_ONE_DIR], b['H12'][U.I_B_ONE_DIR], U.SIGMA)
    assert (c1 == 0).all() and (c2[[U.M_H_AT, U.M_H_BELOW]] >= 0).all() and c2[10] > 0 and not mh[U.I_B_ONE_DIR].any() and sh[U.I_B_ONE_DIR] > 0
    # w of exactly 0: 1.0 / 0 = inf; den of exactly 0: num * num / 0
    assert not mh[U.I_B_W0_H21, U.M_W0_A] and not mh[U.I_B_W0_H12, U.M_W0_B] and np.isfinite(sh[[U.I_B_W0_H21, U.I_B_W0_H12]]).all()
    den2 = U.np_terms_f(b['pts'], b['F21'][U.I_B_DEN0], U.SIGMA, detail=True)[3]
    assert den2[U.M_DEN0] == 0 and not mf[U.I_B_DEN0, U.M_DEN0]
    assert np.isnan(sf[U.I_B_ZERO]) and mf[U.I_B_ZERO].all()   # 0 * 0 / (0 + 0): NaN > th is false, the NaN is added
