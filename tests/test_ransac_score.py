"""RANSAC scoring without a GPU: the C++ restatement (tests/cpp/ransac_score_ref.cpp) and the numpy restatement
(tests/ransac_score_util.py) agree bit for bit on the sweep and on the crafted set; the crafted verdicts are the ones that follow
by hand; os1_amd/csrc/ransac_plan.h accepts and refuses what it should, also under the sanitizers; Sim3RansacWalk and
PnPRansacWalk (include/orbfe/RansacScoring.h), driven by the restatement's counts, replay the restated iterate loops on
scripted count sequences; the headers compile as C++11."""
import os
import subprocess

import numpy as np
import pytest

import ransac_score_util as U

ROOT = U.ROOT
CPP = U.CPP


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('ransac_score_ref'))


@pytest.fixture(scope='module')
def walk_exe(tmp_path_factory):
    return U.compile_walk_test(str(tmp_path_factory.mktemp('ransac_walk') / 'ransac_score_test_host'), host=True)


@pytest.mark.parametrize('model', ['sim3', 'pnp'])
def test_restatements_agree_on_the_sweep(ref, model):
    ratios = []
    for n in U.SWEEP_N:
        for K in U.SWEEP_K:
            call = U.sweep_call(model, n, K)
            a = U.ref_score(ref, call)
            U.assert_same(U.np_score(call), a, '%s n=%d K=%d' % (model, n, K))
            assert all(c == m.sum() for c, m in zip(*a))
            if n == 1000 and K == 300:
                ratios = a[0] / n
    call = U.multi_call(model)
    a = U.ref_score(ref, call)
    U.assert_same(U.np_score(call), a, '%s multi' % model)
    assert [len(m) for m in a[1]] == [U.MULTI_N[s] for s in call.hyp_seg]
    # the hypotheses run from the truth (about 70 % of the correspondences are right) to gross (nothing fits)
    assert ratios.max() > 0.6 and ratios.min() == 0 and ((ratios > 0.1) & (ratios < 0.5)).any()


@pytest.mark.parametrize('model', ['sim3', 'pnp'])
def test_crafted_set(ref, model):
    call, want = U.crafted(model)
    counts, masks = U.ref_score(ref, call)
    U.assert_same(U.np_score(call), (counts, masks), model)
    assert np.array_equal(np.stack(masks), want)
    assert list(counts) == [int(want[0].sum()), 0]
    # the arithmetic behind two of the verdicts
    assert U.f32(float(U.BELOW3) ** 2) == np.nextafter(U.f32(9), U.f32(0)) and U.BELOW3 < 3
    assert U.sim3_max_error(U.SIGMA2_L1) == 13 and 13.2 < 9.210 * float(U.SIGMA2_L1) < 13.3
    assert U.pnp_max_error(U.SIGMA2_L1) == U.f32(1.44) * U.f32(5.991)


def test_plan_header_standalone_and_sanitized(tmp_path):
    src = os.path.join(CPP, 'ransac_plan_test.cpp')
    inc = '-I' + os.path.join(ROOT, 'os1_amd', 'csrc')
    for name, flags in (('plain', ['-O1']), ('san', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('ransac_plan_test_' + name))
        subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror'] + flags + [inc, src, '-o', exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == 'PASS', name + ': ' + r.stdout[-2000:] + r.stderr[-2000:]


def test_headers_compile_as_cxx11(tmp_path):
    one = tmp_path / 'only_header.cpp'
    one.write_text('#include "orbfe/RansacScoring.h"\nint main() { return 0; }\n')
    subprocess.check_call(['g++', '-std=c++11', '-fsyntax-only', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(one)])
    subprocess.check_call(['g++', '-std=c++11', '-fsyntax-only', '-Wall', '-Werror', '-DRANSAC_SCORE_HOST', '-I' + os.path.join(ROOT, 'include'),
                           '-I' + os.path.join(ROOT, 'oracle'), '-I' + CPP, os.path.join(CPP, 'ransac_score_test.cpp')])


# ---- the walks on scripted count sequences ----------------------------------------------------------------------------------
N, MIN = 40, 20      # scripted candidates: 40 correspondences; mRansacMinInliers 20 (PnP: max(10, 40 * 0.5))


def _scene(tmp_path, walk_exe, name, model, cands, **kw):
    """Write and run one scene; -> its iterate() lines.  The program has already compared every line with the restated iterate;
    here the scripted counts are checked to be what the restatement computes, and the caller asserts the outcome."""
    path = U.write_scene(str(tmp_path / (name + '.bin')), model, cands, **kw)
    lines, calls = U.run_walk_test(walk_exe, [path])
    assert lines[-2] == 'scenes 1 mismatches 0' and lines[0].startswith('pack:') and lines[0].endswith(' ok')
    return calls[path]


def _scripted(ref, model, counts, refined=(), **kw):
    c = U.scripted_candidate(model, N, counts, refined, **kw)
    for hyp, want in ((c['hyp'], counts), (c['refined'], refined)):
        if len(want):
            got, _ = U.ref_score(ref, U.Call(model, c['corr'], c['cams'], hyp))
            assert list(got) == list(want), 'the scripted counts are not what the restatement computes'
    return c


def test_sim3_walk_tie_takes_the_later_and_equal_to_min_goes_on(ref, walk_exe, tmp_path):
    # a tie at the best: `>=` takes the later hypothesis; nothing is above 20, so the call returns cv::Mat()
    c = _scripted(ref, 'sim3', [10, 15, 15, 12, 3])
    (a,) = _scene(tmp_path, walk_exe, 'tie', 'sim3', [c], max_its=5)
    assert (a['ret'], a['best'], a['its'], a['noMore'], a['nInliers']) == (-1, 2, 5, 1, 0)
    # a count equal to mRansacMinInliers does not stop the loop (`>`); the 25 two iterations later does
    c = _scripted(ref, 'sim3', [20, 5, 25, 40, 40])
    (a,) = _scene(tmp_path, walk_exe, 'equal', 'sim3', [c])
    assert (a['ret'], a['best'], a['its'], a['consumed'], a['noMore'], a['nInliers']) == (2, 2, 3, 3, 0, 25)


def test_sim3_walk_state_across_three_calls_and_exhaustion(ref, walk_exe, tmp_path):
    # three iterate(5) calls: the best of call 1 survives call 2 (a tie in call 2 moves it), call 3 returns at its third hypothesis
    c = _scripted(ref, 'sim3', [3, 18, 7, 0, 1] + [2, 18, 4, 17, 0] + [19, 9, 21, 40, 40])
    a = _scene(tmp_path, walk_exe, 'three', 'sim3', [c])
    assert [(x['ret'], x['best'], x['its'], x['noMore']) for x in a] == [(-1, 1, 5, 0), (-1, 6, 10, 0), (12, 12, 13, 0)]
    # exhaustion: mRansacMaxIts = 12 ends the third call after two hypotheses, with a best but nothing to return
    c = _scripted(ref, 'sim3', [3, 18, 7, 0, 1] + [2, 18, 4, 17, 0] + [19, 9, 40, 40, 40])
    a = _scene(tmp_path, walk_exe, 'exhaust', 'sim3', [c], max_its=12)
    assert [(x['ret'], x['best'], x['its'], x['noMore'], x['consumed']) for x in a] == [(-1, 1, 5, 0, 5), (-1, 6, 10, 0, 5), (-1, 10, 12, 1, 2)]
    # fewer correspondences than mRansacMinInliers: bNoMore at once, nothing consumed
    few = U.scripted_candidate('sim3', 12, [12, 12])
    (a,) = _scene(tmp_path, walk_exe, 'few', 'sim3', [few])
    assert (a['ret'], a['noMore'], a['its'], a['consumed']) == (-1, 1, 0, 0)


def test_pnp_walk_tie_keeps_the_earlier_and_equal_to_min_accepts(ref, walk_exe, tmp_path):
    # two 22s: the strict `>` keeps the first; both call Refine, which fails twice (20 is not > 20, 18); the iterations run out
    # (mRansacMaxIts 6 -- the OR in the loop condition makes iterate(5) run all six) and the best so far is returned
    c = _scripted(ref, 'pnp', [3, 22, 5, 22, 7, 1], refined=[20, 18])
    (a,) = _scene(tmp_path, walk_exe, 'tie', 'pnp', [c], min_inliers=10, max_its=6)
    assert (a['ret'], a['best'], a['its'], a['consumed'], a['noMore'], a['nInliers']) == (1, 1, 6, 6, 1, 22)
    # a count equal to mRansacMinInliers is accepted (`>=`): Refine runs, and its 21 > 20 succeeds
    c = _scripted(ref, 'pnp', [19, 20, 40], refined=[21])
    (a,) = _scene(tmp_path, walk_exe, 'equal', 'pnp', [c], min_inliers=10, max_its=6)
    assert (a['ret'], a['best'], a['its'], a['consumed'], a['noMore'], a['nInliers']) == (-2, 1, 2, 2, 0, 21)


def test_pnp_walk_refine_exhaustion_and_state_across_three_calls(ref, walk_exe, tmp_path):
    # a failing, then a succeeding Refine
    c = _scripted(ref, 'pnp', [25, 3, 24, 40], refined=[19, 30])
    (a,) = _scene(tmp_path, walk_exe, 'refine', 'pnp', [c], min_inliers=10, max_its=6)
    assert (a['ret'], a['best'], a['its'], a['nInliers'], a['noMore']) == (-2, 0, 3, 30, 0)
    # exhaustion without a best: nothing reaches 20
    c = _scripted(ref, 'pnp', [19, 3, 0, 18, 7, 1])
    (a,) = _scene(tmp_path, walk_exe, 'none', 'pnp', [c], min_inliers=10, max_its=6)
    assert (a['ret'], a['best'], a['its'], a['nInliers'], a['noMore']) == (-1, -1, 6, 0, 1)
    # three calls on one solver: call 1 runs mRansacMaxIts = 8 iterations and finds nothing; call 2 runs five more (the OR), a 22
    # with a failing Refine becomes the best and is returned at the end; call 3: a 21 is accepted but is no new best, Refine -- on
    # the mask carried over from call 2 -- succeeds
    c = _scripted(ref, 'pnp', [1, 2, 3, 4, 5, 6, 7, 8] + [9, 22, 3, 2, 1] + [4, 21, 40, 40, 40], refined=[5, 33])
    a = _scene(tmp_path, walk_exe, 'three', 'pnp', [c], min_inliers=10, max_its=8, calls=3)
    assert [(x['ret'], x['best'], x['its'], x['nInliers'], x['noMore'], x['consumed']) for x in a] == \
        [(-1, -1, 8, 0, 1, 8), (9, 9, 13, 22, 1, 5), (-2, 9, 15, 33, 0, 2)]


def test_round_robin_of_three_candidates_on_the_host(ref, walk_exe, tmp_path):
    """The scenes the GPU test runs through the C ABI, with the restatement as the scorer."""
    lines, calls = U.run_walk_test(walk_exe, [U.sim3_round_robin_scene(str(tmp_path / 's.bin')), U.pnp_refine_scene(str(tmp_path / 'p.bin'))])
    assert lines[-2] == 'scenes 2 mismatches 0'
    s, p = (calls[k] for k in sorted(calls, key=lambda k: k.endswith('p.bin')))
    assert {x['cand'] for x in s} == {0, 1, 2} and max(x['round'] for x in s) >= 2 and any(x['ret'] >= 0 for x in s)
    assert any(x['ret'] == -2 for x in p)
