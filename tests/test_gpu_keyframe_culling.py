"""orbfe_redundant_observations on the GPU (Matcher.redundant_observations) against the CPU restatement
tests/cpp/keyframe_culling_ref.cpp: both output arrays, exactly (integer counting: there is no tolerance), with hand-worked figures
and a numpy count as further checks; every refusal with a live matcher; the grow-only buffers; and the C++ facade on the stub maps
through the C ABI.

Shapes, each because the kernel can go wrong there (keyframe_culling_util.crafted_case, th_obs 1 and 3):
  subjects of 0, 1, 63, 64, 65, 130 entries     a wave and a workgroup not filled, filled, one over; empty subjects in the bisection
  all entries -1                                 nothing to add, no atomic
  10 + 7 + 64 entries                            two and three subjects inside one wave: the per-segment totals
  MapPoints of 0, th_obs, th_obs + 1 observations   not looked at / looked at
  64, 65, 300 observations                       the lane route's longest list, the wave route's shortest, several steps of 64
  observers at level + 1, level + 2, 0, 255      the level test, in int: 255 + 1 does not wrap
  the subject first, last, absent; subj_self -1  the exclusion, on both routes
  exactly th_obs qualifying, one the subject     th_obs - 1 others: not redundant
  qualifying observers late in a long list       the wave route's last, partly filled step
  a MapPoint named twice                         counts twice
  mp_nobs given, NULL, disagreeing with the CSR  Observations() decides, the CSR is counted
  rebased CSRs                                   offsets[0] > 0, junk in front that must not be read
  a random map                                   40 keyframes of 300 entries, 2 to 30 observations, levels 0..7
  covisibility and culling calls interleaved     the staging the two calls share, over buffers that are too large and that regrow"""
import numpy as np
import pytest

import keyframe_culling_util as U

pytestmark = pytest.mark.gpu


class World:
    pass


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from os1_amd import api
    w = World()
    w.api = api
    w.ref = U.build_ref(tmp_path_factory.mktemp('kfcull_ref'))
    w.m = api.Matcher(0)
    w.want = {}
    yield w
    w.m.close()


def pairs(counts):
    return list(zip(counts[0].tolist(), counts[1].tolist()))


def want(w, key, case):
    """the restatement's answer, computed once per case"""
    if key not in w.want:
        w.want[key] = U.ref_counts(w.ref, case)
    return w.want[key]


def check(w, key, case, matcher=None):
    got = (matcher or w.m).redundant_observations(*case.args())
    ref = want(w, key, case)
    for name, g, r in zip(('n_mps', 'n_redundant'), got, ref):
        assert g.dtype == np.int32 and np.array_equal(g, r), (key, name, g.tolist(), r.tolist())
    return got


@pytest.mark.parametrize('th_obs', (1, 3))
def test_crafted_subjects(world, th_obs):
    c, names, hand = U.crafted_case(th_obs)
    got = check(world, ('crafted', th_obs), c)
    assert dict(zip(names, pairs(got))) == dict(zip(names, hand))
    assert pairs(check(world, ('crafted', th_obs), c.rebased())) == hand
    # mp_nobs given and equal to the CSR's lengths: the same answer
    assert pairs(check(world, ('crafted', th_obs), c.but(mp_nobs=np.diff(c.obs_offsets).astype(np.int32)))) == hand


def test_observation_counts_that_disagree_with_the_csr(world):
    c, hand = U.nobs_case()
    assert pairs(check(world, 'nobs', c)) == hand
    assert pairs(check(world, 'nobs-null', c.but(mp_nobs=None))) == [(4, 2)]
    assert pairs(check(world, 'nobs-4', c.but(mp_nobs=np.array([4, 4, 9, 4], np.int32)))) == [(4, 3)]
    assert pairs(check(world, 'nobs-0', c.but(mp_nobs=np.zeros(4, np.int32)))) == [(4, 0)]


@pytest.mark.parametrize('th_obs', (1, 3))
def test_random_map(world, th_obs):
    c = U.random_map(th_obs=th_obs)
    assert c.n_kf == 40 and (np.diff(c.subj_offsets) == 300).all()
    got = check(world, ('map', th_obs), c)
    assert pairs(got) == pairs(U.np_counts(c))
    assert 0 < got[1].sum() < got[0].sum()
    ms = world.m.culling_ms()
    assert (ms >= 0).all() and ms[2] >= ms[1] > 0


def test_two_calls_of_different_size_on_one_matcher_agree_with_fresh_matchers(world):
    w = world
    small, _, _ = U.crafted_case(3)
    big = U.random_map()
    assert len(big.subj_mp) > 4 * len(small.subj_mp)
    m = w.api.Matcher(0)
    try:
        first = check(w, ('crafted', 3), small, matcher=m)          # the buffers are sized for the small call,
        second = check(w, ('map', 3), big, matcher=m)               # grow for the big one,
        third = check(w, ('crafted', 3), small, matcher=m)          # and are larger than the third call needs
    finally:
        m.close()
    for case, got in ((small, first), (big, second), (small, third)):
        f = w.api.Matcher(0)
        try:
            fresh = f.redundant_observations(*case.args())
        finally:
            f.close()
        assert pairs(fresh) == pairs(got)


def test_covisibility_and_culling_calls_interleaved_on_one_matcher(world):
    """The two calls stage the same graph through one piece of code into grow-only buffers of their own.  On one matcher: a larger
    covisibility call, a small culling call, a small covisibility call (its buffers are larger than it needs and hold the first
    call's data), a larger culling call (its buffers regrow).  Larger: 300 MapPoints, 65 keyframes, 5 subjects of 150 entries -- every
    part of the upload arena and covisibility's output arrays are past one 256-byte granule (culling's two output arrays are 4 bytes
    per subject: one granule each up to 64 subjects) -- and MapPoint 0 is seen from all 65 keyframes, so that the wave route of
    k_redundant_observations runs on the restaged data.  All outputs are integers and must equal the numpy counts."""
    import covisibility_util as CU
    w = world
    rng = np.random.default_rng(23)
    n_kf, n_mp = 65, 300
    observers = [[(j, 0) for j in range(n_kf)]]
    for _ in range(n_mp - 1):
        slots = np.sort(rng.choice(n_kf, int(rng.integers(0, 13)), replace=False))
        observers.append(list(zip(slots.tolist(), rng.integers(0, 8, len(slots)).tolist())))
    subjects = []
    for self_ in (0, 17, 64, -1, 3):
        mp = rng.integers(0, n_mp, 150)
        mp[rng.random(150) < 0.1] = -1
        mp[7] = 0
        subjects.append((self_, list(zip(mp.tolist(), rng.integers(0, 8, 150).tolist()))))
    tiny_obs = [[(0, 0), (1, 1), (2, 0), (3, 2)], [(1, 0)], []]
    tiny_subj = [(0, [(0, 1), (1, 0), (-1, 0)]), (-1, [(2, 1), (0, 3)])]

    def covis(n, obs, subj):
        return CU.Case(n, [[j for j, _ in o] for o in obs], [(s, None, [p for p, _ in e]) for s, e in subj])

    big_covis, big_cull = covis(n_kf, observers, subjects), U.Case(n_kf, observers, subjects)
    small_covis, small_cull = covis(4, tiny_obs, tiny_subj), U.Case(4, tiny_obs, tiny_subj)
    assert big_cull.n_mp == 300 and big_cull.n_subj == 5 and small_cull.n_mp == 3 and small_cull.n_subj == 2
    assert np.diff(big_cull.obs_offsets).max() == 65 > U.LONG and len(big_cull.obs_level) > 256 and CU.np_counts(big_covis)[0][-1] > 64
    m = w.api.Matcher(0)
    try:
        got = [w.api.covisibility_counts(m, *big_covis.args()), m.redundant_observations(*small_cull.args()),
               w.api.covisibility_counts(m, *small_covis.args()), m.redundant_observations(*big_cull.args())]
    finally:
        m.close()
    expect = [CU.np_counts(big_covis), U.np_counts(small_cull), CU.np_counts(small_covis), U.np_counts(big_cull)]
    for k, (g, e) in enumerate(zip(got, expect)):
        assert len(g) == len(e)
        for a, b in zip(g, e):
            assert a.dtype == np.int32 and np.array_equal(a, b), (k, a.tolist(), b.tolist())
    assert pairs(got[1]) == [(2, 1), (2, 1)] and got[3][1].sum() > 0      # the small culling call by hand; the larger one finds redundancy


def test_refusals_with_a_live_matcher(world):
    w = world
    c, _, hand = U.crafted_case(3)

    def refused(word, **change):
        d = c.but()
        for k, v in change.items():
            if isinstance(v, tuple):
                a = getattr(d, k).copy()
                a[v[0]] = v[1]
                v = a
            setattr(d, k, v)
        with pytest.raises(w.api.OrbfeError) as e:
            w.m.redundant_observations(*d.args())
        assert e.value.code == -1 and word in str(e.value), e.value

    refused('obs_offsets decreases', obs_offsets=(3, 1))
    refused('subj_offsets decreases', subj_offsets=(3, 100))
    refused('obs_kf[2] = 400', obs_kf=(2, 400))
    refused('obs_kf[0] = -1', obs_kf=(0, -1))
    refused('subj_mp[40] = %d' % c.n_mp, subj_mp=(40, c.n_mp))
    refused('subj_mp[40] = -2', subj_mp=(40, -2))
    refused('subj_self[1] = 400', subj_self=(1, 400))
    refused('subj_self[1] = -2', subj_self=(1, -2))
    refused('th_obs = 0', th_obs=0)
    nobs = np.diff(c.obs_offsets).astype(np.int32)
    nobs[5] = -1
    refused('mp_nobs[5] = -1', mp_nobs=nobs)
    # no subjects: fine, and empty
    z, b = np.zeros(0, np.int32), np.zeros(0, np.uint8)
    a, r = w.m.redundant_observations(c.n_kf, c.obs_offsets, c.obs_kf, c.obs_level, z, np.zeros(1, np.int32), z, b)
    assert len(a) == 0 and len(r) == 0
    # no keyframes and no MapPoints, one subject of skipped entries, one without entries
    a, r = w.m.redundant_observations(0, np.zeros(1, np.int32), z, b, np.array([-1, -1], np.int32), np.array([0, 3, 3], np.int32),
                                      np.full(3, -1, np.int32), np.zeros(3, np.uint8))
    assert a.tolist() == [0, 0] and r.tolist() == [0, 0]
    # and the matcher still counts
    assert pairs(check(w, ('crafted', 3), c)) == hand


def test_facade_on_the_stub_maps(tmp_path):
    U.run(U.compile_facade(str(tmp_path / 'kfcull_gpu'), gpu=True))
