"""CPU side of tests/test_gpu_shared_handles.py: every value the GPU module compares against is produced here, without a device, from
the oracle or from the restatement its call is pinned to (tests/shared_handles_util.py world()), and the scenes are what the GPU
module's docstring says they are -- no expectation is empty, so none of the comparisons there can pass vacuously.

The culling scene: keyframe_culling_util.random_map cut to 8 keyframes of 130 entries keeps every boundary between two subjects
inside a wave (130 k is no multiple of 64 for k < 32) and still holds redundant and non-redundant MapPoints; with 8 keyframes no MapPoint of it can
have more than 8 observers, so the observation lists longer than 64 (the wave route) come from crafted_case(3), which runs beside it."""
import numpy as np
import pytest

import shared_handles_util as SH


@pytest.fixture(scope='module')
def w(tmp_path_factory):
    return SH.world(tmp_path_factory.mktemp('shared_handles'))


def test_window_search_expectations_hold_matches(w):
    assert 256 < len(w.kA) <= 512 and 256 < len(w.kB) <= 512          # more than one block of the build and projection kernels, the last partial
    assert w.sbp['nmatches'] > 50 and 50 < (w.sbp['kp_assigned'] >= 0).sum() <= w.sbp['nmatches']      # (the last MapPoint to take a keypoint stays)
    assert w.local['proj']['n_in_view'] > len(w.local['rows']) // 3
    p = w.projected
    assert p['nmatches'] > 15 and (p['best_idx'] >= 0).sum() == p['nmatches'] and p['inv_sigma2'] is not None
    assert (w.kfproj['best'] == p['best_idx']).all()
    s = w.sources['want']
    assert s['nmatches'] > 25 and s['proj']['n_valid'] > len(w.kA) // 6
    assert w.uv['nmatches'] > 100 and (w.uv['kp_assigned'] == -2).any()      # the rotation check cleared a slot


def test_the_oracle_reproduces_the_recorded_triangulation_rows(w):
    import triangulation_batch_util as TB
    job, raw = w.tri['job'], w.tri['raw']
    assert len(job['nb']) == 3 and all(300 <= len(k['kps']) <= 400 for k in [job['kf1']] + job['nb'])
    assert TB.ref_raw_rows(w.oracle, job).tobytes() == raw.tobytes()
    assert (raw[0] >= 0).any() and (raw[1] == -1).all() and (raw[2] >= 0).any()


def test_refresh_expectation_changes_every_kind_of_field(w):
    r = w.refresh
    b = r['batch']
    before, after = r['table'], r['rows_after']
    touched = b.rows[[len(o) > 0 for o in b.obs_lists]]
    assert (after[touched, 12:32] != before[touched, 12:32]).any(axis=1).all()       # normal, min, max
    assert (after[:, 32:] != before[:, 32:]).any() and (r['best'] >= 0).sum() >= len(b.rows) - 3
    assert after[:, :12].tobytes() == before[:, :12].tobytes()                       # pos is never written
    assert max(len(o) for o in b.obs_lists) == 129 and len(r['kfs']) == 132


def test_init_score_expectation_has_winners(w):
    i = w.init
    assert i['n'] == 300 and (i['m12'] >= 0).sum() == 300
    assert i['want'].best_h >= 0 and i['want'].best_f >= 0 and i['want'].inliers_h.any() and i['want'].inliers_f.any()


def test_the_reduced_culling_map_and_the_crafted_case_keep_their_edges(w):
    import keyframe_culling_util as KC
    c = w.culling
    cut = c['cut']
    assert cut.n_kf == SH.CULL_KF and (np.diff(cut.subj_offsets) == SH.CULL_ENTRIES).all()
    inner = cut.subj_offsets[1:-1]
    assert len(inner) == SH.CULL_KF - 1 and (inner % SH.WAVE != 0).all()             # every subject boundary lies inside a wave
    assert np.diff(cut.obs_offsets).max() <= SH.CULL_KF                              # ... and no list of it can be long:
    assert np.diff(c['crafted'].obs_offsets).max() > KC.LONG                         # the crafted case brings those (65 and 300)
    assert (np.diff(c['crafted'].obs_offsets) == KC.LONG + 1).any()
    n_mps, n_red = c['cut_want']
    assert [a.tolist() for a in KC.np_counts(cut)] == [n_mps.tolist(), n_red.tolist()]
    assert 0 < n_red.sum() < n_mps.sum()
    assert list(zip(c['crafted_want'][0].tolist(), c['crafted_want'][1].tolist())) == c['crafted_hand']


def test_covisibility_database_and_bow_expectations_are_not_empty(w, tmp_path):
    import covisibility_util as CV
    for name in ('special', 'small'):
        offs, kf, cnt = w.covis[name + '_want']
        assert offs[-1] == len(kf) == len(cnt) > 0
    ref = CV.build_ref(tmp_path)
    for name in ('special', 'small'):
        for g, r in zip(w.covis[name + '_want'], CV.ref_counts(ref, w.covis[name])):
            assert np.array_equal(g, r)
    k = w.kfdb
    assert len(k['adds']) > 20
    for name, (keys, common, scores) in k['want'].items():
        assert len(keys) > 3 and (common > 0).all() and (scores > 0).any(), name
    assert set(k['want']['reloc'][0].tolist()) != set(k['want']['reloc2'][0].tolist())
    lens = [len(s) for s in w.bow['sets']]
    assert lens == [63, 0, 65]
    for n, flat in zip(lens, w.bow['want']):
        assert (len(flat[0]) > 0) == (n > 0)
