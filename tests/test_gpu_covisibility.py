"""orbfe_covisibility_counts on the GPU against the CPU restatement tests/cpp/covisibility_ref.cpp: all three output arrays,
exactly (integer counting: there is no tolerance), with a np.add.at count as a second, independent check; the overflow report;
every refusal with a live matcher; and the C++ facade on the stub map through the C ABI.

Shapes, each because the kernel can go wrong there (S = the histogram's bins per pass, api.covis_slots_per_pass()):
  n_kf 1, 63, 64, 65                     one bin; either side of a wave of bins in the output sweep
  n_kf S - 1, S, S + 1                   the last bin of a pass, a second pass of one bin; observers at slots 0, S - 1, S, n_kf - 1
  1, 2 and 130 subjects                  more workgroups than fit the CUs' LDS at S bins each in one go
  a subject with no entries / all -1 / a MapPoint without observations / observed only by itself (an empty segment)
  a MapPoint named 300 times             counts above 255, duplicates
  subj_self -1                           no exclusion
  subj_limit 0, k + 1 and n_kf           on the same data
  cap one short of the need              ORBFE_ERR_OVERFLOW with n_needed right; the same call with room then succeeds
  a small map                            40 keyframes of 200 entries, 2 to 12 observations per MapPoint"""
import numpy as np
import pytest

import covisibility_util as U

pytestmark = pytest.mark.gpu


class World:
    pass


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from os1_amd import api
    w = World()
    w.api = api
    w.ref = U.build_ref(tmp_path_factory.mktemp('covis_ref'))
    w.m = api.Matcher(0)
    w.S = api.covis_slots_per_pass()
    w.special, w.names = U.special_case()
    w.want = {}
    yield w
    w.m.close()


def want(w, key, case):
    """the restatement's answer, computed once per case"""
    if key not in w.want:
        w.want[key] = U.ref_counts(w.ref, case)
    return w.want[key]


def check(w, key, case, numpy_too=True):
    got = w.api.covisibility_counts(w.m, *case.args())
    ref = want(w, key, case)
    for name, g, r in zip(('out_offsets', 'out_kf', 'out_count'), got, ref):
        assert g.dtype == np.int32 and np.array_equal(g, r), (key, name)
    if numpy_too:
        for name, g, r in zip(('out_offsets', 'out_kf', 'out_count'), got, U.np_counts(case)):
            assert np.array_equal(g, r), (key, name, 'numpy')
    return got


@pytest.mark.parametrize('n_kf,n_subj', [(1, 1), (63, 2), (64, 130), (65, 130), (65, 1)])
def test_counts_equal_the_restatement(world, n_kf, n_subj):
    c = U.random_case(100 + n_kf + n_subj, n_kf, n_subj, must=(0, n_kf - 1))
    offs, kf, cnt = check(world, ('random', n_kf, n_subj), c)
    if n_kf > 1:
        assert offs[-1] > 0
    for s in range(n_subj):
        seg = kf[offs[s]:offs[s + 1]]
        assert (np.diff(seg) > 0).all() and (cnt[offs[s]:offs[s + 1]] > 0).all()       # ascending slots, non-zero counters only
        assert c.subj_self[s] not in seg.tolist()


@pytest.mark.parametrize('delta', (-1, 0, 1))
def test_pass_boundary(world, delta):
    w = world
    n_kf = w.S + delta
    c = U.random_case(7 + delta, n_kf, 3, n_mp=40, max_obs=10, must=(0, w.S - 1, w.S, n_kf - 1), frames=1.0)
    offs, kf, cnt = check(w, ('boundary', delta), c)
    seen = set(kf.tolist())
    for j in (0, w.S - 1, w.S, n_kf - 1):
        if j < n_kf:
            assert j in seen, j                                                        # both sides of the boundary are hit
    # the same data seen by subjects that ARE the boundary keyframes, and cut by a limit on the boundary
    d = U.Case.__new__(U.Case)
    d.__dict__.update(c.__dict__)
    d.subj_self = np.array([min(w.S - 1, n_kf - 1), min(w.S, n_kf - 1), 0], np.int32)
    d.subj_limit = np.array([n_kf, min(w.S, n_kf), w.S - 1], np.int32)
    offs, kf, cnt = check(w, ('boundary-self', delta), d)
    assert int(d.subj_self[0]) not in kf[offs[0]:offs[1]].tolist() and (kf[offs[1]:offs[2]] < w.S).all() and (kf[offs[2]:offs[3]] < w.S - 1).all()


def test_three_passes_and_many_subjects(world):
    w = world
    n_kf = 2 * w.S + 5
    c = U.random_case(9, n_kf, 130, n_mp=50, entries=(0, 40), max_obs=8, must=(0, w.S - 1, w.S, 2 * w.S - 1, 2 * w.S, n_kf - 1))
    offs, kf, cnt = check(w, 'three-passes', c, numpy_too=False)
    assert {0, w.S - 1, w.S, 2 * w.S - 1, 2 * w.S, n_kf - 1} <= set(kf.tolist())


def test_special_subjects(world):
    w = world
    offs, kf, cnt = check(w, 'special', w.special)
    seg = {n: (kf[offs[s]:offs[s + 1]].tolist(), cnt[offs[s]:offs[s + 1]].tolist()) for s, n in enumerate(w.names)}
    for n in ('no_entries', 'all_skipped', 'zero_observations', 'only_itself'):
        assert seg[n] == ([], []), n
    assert seg['named_300_times'] == ([0, 1, 2, 4, 64, 65, 69], [1, 300, 300, 300, 300, 300, 1])
    assert 3 in seg['frame'][0] and seg['frame'][1][seg['frame'][0].index(3)] == 4     # subj_self -1: nobody excluded


def test_limits_on_the_same_data(world):
    w = world
    base = U.random_case(4, 65, 65, frames=0.0)
    k = np.arange(65, dtype=np.int32)
    full = check(w, ('limit', 'none'), base.with_limits(None))
    same = check(w, ('limit', 'n_kf'), base.with_limits(np.full(65, 65, np.int32)))
    assert all(np.array_equal(a, b) for a, b in zip(full, same))
    zero = check(w, ('limit', 0), base.with_limits(np.zeros(65, np.int32)))
    assert zero[0].tolist() == [0] * 66 and len(zero[1]) == 0
    pred = check(w, ('limit', 'k+1'), base.with_limits(k + 1))
    for s in range(65):
        assert (pred[1][pred[0][s]:pred[0][s + 1]] < s).all()                         # only predecessors (slot s itself is the subject)
    assert 0 < pred[0][-1] < full[0][-1]


def test_overflow_reports_the_need_and_the_matcher_stays_usable(world):
    w = world
    ref = want(w, 'special', w.special)
    need = int(ref[0][-1])
    with pytest.raises(w.api.OrbfeError) as e:
        w.api.covisibility_counts(w.m, *w.special.args(), cap=need - 1)
    assert e.value.code == -5 and e.value.n_needed == need
    with pytest.raises(w.api.OrbfeError) as e:
        w.api.covisibility_counts(w.m, *w.special.args(), cap=0)
    assert e.value.code == -5 and e.value.n_needed == need
    got = w.api.covisibility_counts(w.m, *w.special.args(), cap=need)                  # the identical call with room
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))


def test_small_map(world):
    w = world
    c = U.small_map()
    assert c.n_kf == 40 and (np.diff(c.subj_offsets) == 200).all()
    n_obs = np.diff(c.obs_offsets)
    assert n_obs.min() >= 2 and n_obs.max() <= 12
    offs, kf, cnt = check(w, 'small-map', c)
    assert cnt.max() >= 15 and offs[-1] > 40 * 6
    pred = check(w, 'small-map-load', c.with_limits(np.arange(40, dtype=np.int32) + 1))
    assert pred[0][1] == 0 and pred[0][-1] < offs[-1]                                  # the first keyframe of a load sees nobody
    ms = w.m.covis_ms()
    assert (ms >= 0).all() and ms[2] >= ms[1] > 0


def test_refusals_with_a_live_matcher(world):
    w = world
    c = w.special

    def refused(word, cap=None, **change):
        d = U.Case.__new__(U.Case)
        d.__dict__.update(c.__dict__)
        for k, (i, v) in change.items():
            a = getattr(d, k).copy()
            a[i] = v
            setattr(d, k, a)
        with pytest.raises(w.api.OrbfeError) as e:
            w.api.covisibility_counts(w.m, *d.args(), cap=cap)
        assert e.value.code == -1 and word in str(e.value), e.value

    refused('obs_offsets decreases', obs_offsets=(2, 1))
    refused('subj_offsets decreases', subj_offsets=(3, 10))
    refused('obs_kf[2] = 70', obs_kf=(2, 70))
    refused('obs_kf[0] = -1', obs_kf=(0, -1))
    refused('subj_mp[40] = 6', subj_mp=(40, 6))
    refused('subj_mp[40] = -2', subj_mp=(40, -2))
    refused('subj_self[1] = 70', subj_self=(1, 70))
    refused('subj_self[1] = -2', subj_self=(1, -2))
    refused('negative size', cap=-1)
    for i, v in ((0, 71), (2, -1)):
        lim = np.full(c.n_subj, c.n_kf, np.int32)
        lim[i] = v
        with pytest.raises(w.api.OrbfeError) as e:
            w.api.covisibility_counts(w.m, *c.with_limits(lim).args())
        assert e.value.code == -1 and 'subj_limit[%d] = %d' % (i, v) in str(e.value)
    # no subjects: fine, and empty
    z = np.zeros(0, np.int32)
    offs, kf, cnt = w.api.covisibility_counts(w.m, c.n_kf, c.obs_offsets, c.obs_kf, z, np.zeros(1, np.int32), z)
    assert offs.tolist() == [0] and len(kf) == 0 and len(cnt) == 0
    # no keyframes and no MapPoints, one subject of skipped entries
    offs, kf, cnt = w.api.covisibility_counts(w.m, 0, np.zeros(1, np.int32), z, np.array([-1], np.int32), np.array([0, 3], np.int32),
                                              np.full(3, -1, np.int32))
    assert offs.tolist() == [0, 0] and len(kf) == 0
    # and the matcher still counts
    check(w, 'special', c)


def test_facade_on_the_stub_map(tmp_path):
    U.run(U.compile_facade(str(tmp_path / 'covis_gpu'), host_backend=False))
