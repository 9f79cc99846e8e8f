"""-m gpu: SearchForTriangulation on resident keyframes, all neighbours of a keyframe in one call
(orbfe_search_for_triangulation_frames_batch, k_bow_triangulate_batch).  The two jobs of tests/triangulation_batch_util.py -- one
keyframe against three neighbours of 300 - 400 keypoints, 8 levels, nodes of 257 (the global-memory route) and of exactly 256
(the last size of the LDS route), a neighbour that shares no node, flags on about half of every side, a table of its own per
neighbour -- row by row against the existing single call, the reference (oracle/_ref/libos1_matcher.so, else the oracle) and
the recorded results; batches of one and of none; the loop of LocalMapping.cc:207-232 with evolving flags; every
SearchForTriangulation boundary scene of tests/bow_boundary_util.py through the one-neighbour resident form; the refusals; and
tests/cpp/triangulation_search_test.cpp, the C++ facade (include/orbfe/TriangulationSearch.h) in a loop that adds MapPoints."""
import numpy as np
import pytest

import triangulation_batch_util as T
from bow_boundary_util import SCENES, expected

pytestmark = pytest.mark.gpu

TRI = [s for s in SCENES if s.kind == 'tri']


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def matcher(api):
    return api.Matcher()


@pytest.fixture(scope='module')
def ref(oracle):
    return T.reference_backend(oracle)


@pytest.fixture(scope='module')
def resident(api, matcher):
    """{job: (job, frame of the current keyframe, [frames of the neighbours])}, built once"""
    out = {}
    for name, (job, _, _) in T.golden().items():
        mk = lambda kf: api.Frame.from_host(matcher, kf['kps'], kf['desc'], T.BOUNDS)
        out[name] = (job, mk(job['kf1']), [mk(nb) for nb in job['nb']])
    yield out
    for _, f1, f2 in out.values():
        for f in [f1] + f2:
            f.close()


_ref_raw = {}


def _reference_rows(name, ref):
    if name not in _ref_raw:
        _ref_raw[name] = T.ref_raw_rows(ref, T.golden()[name][0])
    return _ref_raw[name]


def _single_raw(matcher, kf1, nb):
    n, p = matcher.search_for_triangulation(kf1['kps'], kf1['desc'], kf1['has'], kf1['fv'], nb['kps'], nb['desc'], nb['has'], nb['fv'], nb['F12'],
                                            nb['ex'], nb['ey'], nb['sf'], nb['s2'], False)
    return T.raw_from_pairs(p, len(kf1['kps']))


def test_the_jobs_hold_what_they_are_for():
    (large, lraw, _), (edge, eraw, _) = T.golden()['large'], T.golden()['edge256']
    sizes = lambda kf: {int(i): int(b - a) for i, a, b in zip(kf['fv'][0], kf['fv'][1][:-1], kf['fv'][1][1:])}
    assert sizes(large['kf1'])[10] == T.K_SIDE + 1 and sizes(large['nb'][1])[20] == T.K_SIDE + 1
    assert sizes(edge['kf1'])[10] == T.K_SIDE == sizes(edge['nb'][0])[10]
    assert not set(sizes(large['kf1'])) & set(sizes(large['nb'][0])) and not set(sizes(edge['kf1'])) & set(sizes(edge['nb'][1]))
    for job, raw in ((large, lraw), (edge, eraw)):
        assert all(300 <= len(k['kps']) <= 400 and 0.35 < k['has'].mean() < 0.65 for k in [job['kf1']] + job['nb'])
        assert len({nb['F12'].tobytes() for nb in job['nb']}) == 3 and len({nb['sf'].tobytes() for nb in job['nb']}) == 3
        assert len({(nb['ex'], nb['ey']) for nb in job['nb']}) == 3
    # matches come out of both large nodes and of the 256 x 256 one
    under = lambda kf, node: set(int(v) for v in kf['fv'][2][kf['fv'][1][list(kf['fv'][0]).index(node)]:kf['fv'][1][list(kf['fv'][0]).index(node) + 1]])
    assert any(lraw[1][i] >= 0 for i in under(large['kf1'], 10)) and any(lraw[1][i] >= 0 for i in under(large['kf1'], 20))
    assert any(lraw[2][i] >= 0 for i in under(large['kf1'], 10)) and any(eraw[0][i] >= 0 for i in under(edge['kf1'], 10))


@pytest.mark.parametrize('name', list(T.JOBS))
def test_batch_rows_equal_the_single_call_the_reference_and_the_record(name, resident, matcher, ref):
    job, f1, f2 = resident[name]
    kf1 = job['kf1']
    raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], [T.neighbour_arg(f, nb) for f, nb in zip(f2, job['nb'])])
    assert raw.shape == (3, len(kf1['kps'])) and raw.dtype == np.int32
    want = _reference_rows(name, ref)
    for j, nb in enumerate(job['nb']):
        assert raw[j].tobytes() == _single_raw(matcher, kf1, nb).tobytes(), 'neighbour %d differs from the single call' % j
        assert raw[j].tobytes() == want[j].tobytes(), 'neighbour %d differs from the reference' % j
    assert raw.tobytes() == np.ascontiguousarray(T.golden()[name][1]).tobytes()
    assert (raw[:, kf1['has'] != 0] == -1).all()
    none = 0 if name == 'large' else 1
    assert (raw[none] == -1).all() and (raw[2] >= 0).any()
    # a table row read for the wrong neighbour would show: neighbour 2 searched with neighbour 0's / 1's geometry gives another row
    for other in (0, 1):
        swapped = dict(job['nb'][2], **{k: job['nb'][other][k] for k in ('F12', 'ex', 'ey', 'sf', 's2')})
        assert _single_raw(matcher, kf1, swapped).tobytes() != raw[2].tobytes()


@pytest.mark.parametrize('name', list(T.JOBS))
def test_batches_of_one_and_of_none(name, resident, matcher):
    job, f1, f2 = resident[name]
    kf1 = job['kf1']
    for j, nb in enumerate(job['nb']):
        raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], [T.neighbour_arg(f2[j], nb)])
        assert raw.shape == (1, len(kf1['kps'])) and raw[0].tobytes() == np.ascontiguousarray(T.golden()[name][1][j]).tobytes()
    raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], [])
    assert raw.shape == (0, len(kf1['kps']))
    # the same neighbour three times, in another order than recorded: rows follow the call's order
    order = [2, 0, 2]
    raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], [T.neighbour_arg(f2[j], job['nb'][j]) for j in order])
    assert raw.tobytes() == np.ascontiguousarray(T.golden()[name][1][order]).tobytes()


@pytest.mark.parametrize('name', list(T.JOBS))
@pytest.mark.parametrize('ori', [0, 1])
def test_the_loop_with_evolving_flags(name, ori, resident, matcher, ref, api):
    """raw rows once, with the flags at loop entry; then neighbour after neighbour: finish the row with the flags as they stand, give
    a seeded subset of its pairs a MapPoint.  The reference is called inside the same loop with the evolving flags."""
    job, f1, f2 = resident[name]
    kf1 = job['kf1']
    want = T.ref_sequence(ref, job, bool(ori))
    assert want == T.golden()[name][2][ori]
    raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], [T.neighbour_arg(f, nb) for f, nb in zip(f2, job['nb'])])
    rng = np.random.default_rng(3)
    has1 = kf1['has'].copy()
    for j, nb in enumerate(job['nb']):
        n, p = api.triangulation_finish(raw[j], kf1['has'], has1, ori, kf1['kps'], nb['kps'])
        p = [(int(a), int(b)) for a, b in p]
        assert (n, p) == want[j], 'neighbour %d' % j
        has1[T.triangulated(rng, p)] = 1
    assert has1.sum() > kf1['has'].sum()


@pytest.mark.parametrize('scene', TRI, ids=[s.name for s in TRI])
def test_boundary_scene_on_resident_keyframes(scene, api, matcher):
    i = scene.inp
    f1 = api.Frame.from_host(matcher, i['kps1'], i['desc1'], T.BOUNDS)
    f2 = api.Frame.from_host(matcher, i['kps2'], i['desc2'], T.BOUNDS)
    try:
        n, p = matcher.search_for_triangulation_frames(f1, i['has1'], i['fv1'], (f2, i['has2'], i['fv2'], i['F12'], i['ex'], i['ey'], i['sf'], i['s2']),
                                                       i['kps1'], i['kps2'], i['ori'])
        assert (int(n), [(int(a), int(b)) for a, b in p]) == expected(scene)
    finally:
        f1.close()
        f2.close()


def test_bad_neighbours_are_named_and_nothing_is_written(resident, matcher, api):
    job, f1, f2 = resident['large']
    kf1 = job['kf1']
    good = [T.neighbour_arg(f, nb) for f, nb in zip(f2, job['nb'])]
    L = api.load_library()

    def refused(neigh, word, code=-1):
        h1 = np.ascontiguousarray(kf1['has'])
        fv = [np.ascontiguousarray(a, np.uint32) for a in kf1['fv']]
        arr, keep = matcher._tri_neighbours(neigh)
        out = np.full((len(neigh), len(h1)), -7, np.int32)
        rc = L.orbfe_search_for_triangulation_frames_batch(matcher.h, f1.h, api._p(h1), api._p(fv[0]), api._p(fv[1]), api._p(fv[2]), len(fv[0]), len(neigh),
                                                           api.C.cast(arr, api.C.c_void_p), api._p(out))
        msg = L.orbfe_last_error().decode()
        assert rc == code and (out == -7).all() and word in msg, (rc, msg)
        return msg

    def with_(j, **kw):
        names = ('frame2', 'has', 'fv', 'F12', 'ex', 'ey', 'sf', 's2')
        d = dict(zip(names, good[j]), **kw)
        return good[:j] + [tuple(d[k] for k in names)] + good[j + 1:]

    assert 'neighbour 1' in refused(with_(1, sf=job['nb'][1]['sf'][:7], s2=job['nb'][1]['s2'][:7]), 'octave')      # octave 7 with 7 levels
    bad = [a.copy() for a in job['nb'][2]['fv']]
    bad[2][-1] = len(job['nb'][2]['kps'])
    assert 'neighbour 2' in refused(with_(2, fv=bad), 'feature index')
    bad1 = [a.copy() for a in kf1['fv']]
    bad1[2][0] = len(kf1['kps'])
    with pytest.raises(api.OrbfeError) as e:
        matcher.search_for_triangulation_frames_batch(f1, kf1['has'], bad1, good)
    assert e.value.code == -1 and 'feature index' in str(e.value)
    sf17 = np.cumprod(np.full(17, 1.1, np.float32)).astype(np.float32)
    assert 'neighbour 0' in refused(with_(0, sf=sf17, s2=sf17 * sf17), 'nlevels2')
    # the matcher and the frames stay usable
    raw = matcher.search_for_triangulation_frames_batch(f1, kf1['has'], kf1['fv'], good)
    assert raw.tobytes() == np.ascontiguousarray(T.golden()['large'][1]).tobytes()


@pytest.mark.parametrize('name', list(T.JOBS))
def test_cpp_facade_over_a_loop_that_adds_map_points(name, tmp_path, ref):
    """tests/cpp/triangulation_search_test.cpp: orbfe::TriangulationSearch<KeyFrame>::pairs(i) against orbfe::SearchForTriangulation in a
    loop that adds MapPoints between neighbours (checked inside the program, with the resident cache's counters, the cleared-flag
    fall-back and a cache too small for the batch); the pairs it writes equal the reference's in the same loop."""
    import subprocess
    job = T.golden()[name][0]
    exe = T.facade_compile(str(tmp_path / 'triangulation_search_test'))
    T.facade_write_job(str(tmp_path), job)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'triangulation_search_test ok' in r.stdout, (r.returncode, r.stdout, r.stderr)
    for ori in (0, 1):
        want = T.facade_ref_sequence(ref, job, bool(ori))
        assert sum(len(p) for p in want) > 20
        for i, p in enumerate(want):
            got = np.fromfile(tmp_path / ('pairs_ori%d_nb%d.bin' % (ori, i)), np.int32).reshape(-1, 2)
            assert [(int(a), int(b)) for a, b in got] == p, 'orientation check %d, neighbour %d' % (ori, i)
