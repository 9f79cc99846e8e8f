"""-m gpu: the equidistant (fisheye) camera on the GPU -- k_undistort_equidistant against the host build of equidistant_tan.h, the
settled results against the oracle composition (extract, undistort_equidistant, image_bounds mode 1, search_for_initialization on
mvKeysUn), and the host settle on a camera that makes a keypoint of two frames undecided (tests/golden/equidistant_undecided.npz)."""
import numpy as np
import pytest

import equidistant_util as E
import undistort_stream_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def golden():
    return np.load(E.GOLDEN)


def _extractor(api, cam=E.SONY, nlevels=U.NLEVELS):
    ex = api.Extractor(U.NFEAT, 1.2, nlevels, 20, 7, device=0)
    ex.set_camera_equidistant(*cam)
    return ex


_EXPECT = {}


def expected(oracle, cam, kind='main'):
    """undistort_stream_util.expected with the equidistant model."""
    key = (cam, kind)
    if key not in _EXPECT:
        ex = U.extracted(oracle, kind)
        w, h = (U.W, U.H) if kind == 'main' else (U.STRIP_W, U.STRIP_H)
        xy = [oracle.undistort_equidistant(np.stack([k['x'], k['y']], 1).astype(np.float32), *cam) for k, _ in ex]
        bounds = oracle.image_bounds(w, h, 1, *cam)
        un = []
        for (k, _), p in zip(ex, xy):
            u = k.copy()
            u['x'], u['y'] = p[:, 0], p[:, 1]
            un.append(u)
        _EXPECT[key] = dict(xy_un=xy, bounds=bounds, un=un, pairs={})
    return _EXPECT[key]


def pair(oracle, cam, i, j):
    e = expected(oracle, cam)
    if (i, j) not in e['pairs']:
        ex = U.extracted(oracle)
        n, m12, _ = oracle.search_for_initialization(e['un'][i], ex[i][1], e['un'][j], ex[j][1], e['bounds'], e['xy_un'][i], 100, 0.9, True)
        e['pairs'][(i, j)] = (n, m12.copy())
    return e['pairs'][(i, j)]


def _check_batch(oracle, cam, got, keys, pred, xy):
    kps, desc, n, m12, nm = got
    for i, f in enumerate(keys):
        wk, wd = U.extracted(oracle)[f]
        assert n[i] == len(wk) and kps[i, :n[i]].tobytes() == wk.tobytes() and desc[i, :n[i]].tobytes() == wd.tobytes(), i
        assert xy[i, :n[i]].tobytes() == expected(oracle, cam)['xy_un'][f].tobytes(), i
        p = pred if i == 0 else keys[i - 1]
        if p is None:
            assert nm[i] == 0 and (m12[i] == -1).all(), i
            continue
        wn, wm = pair(oracle, cam, p, f)
        assert nm[i] == wn and (m12[i, :len(wm)] == wm).all() and (m12[i, len(wm):] == -1).all(), (i, p, f)


def test_verdict_equals_the_host_header(api, golden):
    ex = _extractor(api)
    seeded = U.seeded_points()
    gold = np.concatenate([golden['%s_%s' % (a, k)] for a in 'xy' for k in ('upper', 'lower')])
    for pts in [seeded, U.crafted_points('k4'), gold] + [seeded[:n] for n in (0, 1, 63, 64, 65)]:
        got, und = ex.undistort_verdict(pts)
        want, wund = E.verdict(pts, E.SONY) if len(pts) else (pts, np.zeros(0, bool))
        assert got.tobytes() == want.tobytes() and (und == wund).all(), len(pts)
    assert ex.undistort_verdict(gold)[1].all() and ex.undistort_verdict(U.crafted_points('k4'))[1].any()
    assert (ex.equidistant_stats() == 0).all()                  # the raw output: nothing settled


def _settle_counts(oracle, pts, cam):
    """(points the host settles, points whose value it changes) -- from the host header and the oracle's own libm, so that the counts
    hold on a libm whose tan is faithful but not correctly rounded on these inputs."""
    raw, und = E.verdict(pts, cam)
    final = oracle.undistort_equidistant(pts, *cam)
    return int(und.sum()), int(((raw.view(np.uint32) != final.view(np.uint32)).any(1) & und).sum())


def test_points_are_settled_to_the_oracle(api, oracle, golden):
    ex = _extractor(api)
    seeded = U.seeded_points()
    upper = np.concatenate([golden['x_upper'], golden['y_upper']])
    lower = np.concatenate([golden['x_lower'], golden['y_lower']])
    many = np.concatenate([upper] * 5)                          # more undecided points than the list holds: the whole launch is settled
    assert len(many) > 63
    for pts in (seeded, U.crafted_points('k4'), upper, lower, many, seeded[:1], seeded[:0]):
        before = ex.equidistant_stats()
        got = ex.undistort(pts)
        want = oracle.undistort_equidistant(pts, *E.SONY) if len(pts) else pts
        assert got.tobytes() == want.tobytes(), len(pts)
        if len(pts):
            assert got.tobytes() == api.undistort_equidistant(pts, *E.SONY).tobytes()
        d = ex.equidistant_stats() - before
        if pts is seeded:
            assert (d == 0).all()
        if pts is upper or pts is lower:
            assert d[0] == len(pts)                              # every one of them is undecided
            assert tuple(d[:2]) == _settle_counts(oracle, pts, E.SONY)      # (upper: the correctly rounded tan changes every one)
        if pts is many:                                          # the whole launch was settled
            assert d[0] == len(many) and d[1] == 5 * _settle_counts(oracle, upper, E.SONY)[1]


def test_pinhole_refusal_names_the_new_call_and_cameras_can_be_swapped(api, oracle):
    ex = _extractor(api)
    with pytest.raises(api.OrbfeError) as e:
        ex.set_camera(500.0, 500.0, 320.0, 240.0, (), mode=1)
    assert e.value.code == -6 and 'tan' in str(e.value) and 'orbfe_extractor_set_camera_equidistant' in str(e.value)
    pts = U.seeded_points()[:100]
    assert ex.undistort(pts).tobytes() == oracle.undistort_equidistant(pts, *E.SONY).tobytes()       # kept its camera
    fx, fy, cx, cy, dist = U.CAMERAS['k4']
    ex.set_camera(fx, fy, cx, cy, dist)
    k, d, xy = ex.extract_undistorted(U.frames()[0])
    assert xy.tobytes() == U.expected(oracle, 'k4')['xy_un'][0].tobytes()
    with pytest.raises(api.OrbfeError):
        ex.undistort_verdict(pts)
    ex.set_camera_equidistant(*E.SONY)
    k, d, xy = ex.extract_undistorted(U.frames()[0])
    assert xy.tobytes() == expected(oracle, E.SONY)['xy_un'][0].tobytes()


def test_extraction_yields_mvkeysun(api, oracle):
    ex = _extractor(api)
    want = expected(oracle, E.SONY)
    frames = U.frames()
    for f in (0, 2):
        k, d, xy = ex.extract_undistorted(frames[f])
        wk, wd = U.extracted(oracle)[f]
        assert k.tobytes() == wk.tobytes() and d.tobytes() == wd.tobytes()      # unchanged by the camera
        assert xy.tobytes() == want['xy_un'][f].tobytes()
    ex.submit_ptrs([f.ctypes.data for f in frames], U.H, U.W, U.W, False)
    kps, desc, n, xy = ex.collect_undistorted()
    for f in range(U.NFRAMES):
        wk, wd = U.extracted(oracle)[f]
        assert n[f] == len(wk) and kps[f, :n[f]].tobytes() == wk.tobytes() and desc[f, :n[f]].tobytes() == wd.tobytes()
        assert xy[f, :n[f]].tobytes() == want['xy_un'][f].tobytes()


def test_host_quadtree_route(api, oracle):
    frames = U.frames('strip')
    want = expected(oracle, E.SONY, 'strip')
    ex = _extractor(api, nlevels=U.STRIP_LEVELS)
    for f in range(2):
        k, d, xy = ex.extract_undistorted(frames[f])
        wk, wd = U.extracted(oracle, 'strip')[f]
        assert k.tobytes() == wk.tobytes() and d.tobytes() == wd.tobytes()
        assert xy.tobytes() == want['xy_un'][f].tobytes()


def test_resident_frame_takes_mvkeysun_from_the_arena(api, oracle):
    e = expected(oracle, E.SONY)
    ex = _extractor(api)
    ex.extract_undistorted(U.frames()[0])
    own = api.Frame.from_extract(ex, 0, e['bounds'])
    sent = api.Frame.from_extract(ex, 0, e['bounds'], e['xy_un'][0])
    for a, b in zip(own.download(), sent.download()):
        assert a.tobytes() == b.tobytes()
    assert np.stack([own.download()[0]['x'], own.download()[0]['y']], 1).tobytes() == e['xy_un'][0].tobytes()


@pytest.mark.parametrize('multi', [False, True])
def test_stream_matches_on_mvkeysun(api, oracle, multi):
    frames = U.frames()
    st = api.MultiStream(U.NFEAT, 1.2, U.NLEVELS, 20, 7, [0, 0], 2, depth=1) if multi else api.Stream(U.NFEAT, 1.2, U.NLEVELS, 20, 7, 0, 2, depth=2)
    try:
        st.set_camera_equidistant(*E.SONY)
        st.set_matching(expected(oracle, E.SONY)['bounds'])
        pushes = ([0, 1], [2, 1], [0, 1])
        for keys in pushes:
            st.push_ptrs([frames[f].ctypes.data for f in keys], U.H, U.W, U.W, on_device=False)
        pred = None
        for keys in pushes:
            got = st.pop(copy=True)
            _check_batch(oracle, E.SONY, got, keys, pred, st.xy_un())
            pred = keys[-1]
        assert (st.equidistant_stats() == 0).all()             # nothing to settle under this camera (test_equidistant_tan.py)
    finally:
        st.close()


def _settle_camera(golden):
    cx, cy = golden['centres'][0]
    return (E.SONY[0], E.SONY[1], float(cx), float(cy))


def _settle_plan(oracle, cam, pushes):
    """The counters a chain over `pushes` must report: points settled / changed per frame as _settle_counts, and the rows to search
    again -- rows f and f + 1 of a changed frame f, row 0 of the batch after one whose last frame changed."""
    per = {}
    for f, (k, _) in enumerate(U.extracted(oracle)):
        per[f] = _settle_counts(oracle, np.stack([k['x'], k['y']], 1).astype(np.float32), cam)
    settled = changed = rows = 0
    pred = None
    for keys in pushes:
        for i, f in enumerate(keys):
            settled += per[f][0]
            changed += per[f][1]
            p = pred if i == 0 else keys[i - 1]
            if p is not None and (per[p][1] or per[f][1]):
                rows += 1
        pred = keys[-1]
    return settled, changed, rows


def test_settle_patches_results_arena_and_match_rows(api, oracle, golden):
    """A camera that makes one level-0 keypoint of frame 1 (mid-batch) and of frame 2 (the batch's last frame) undecided, with the
    correctly rounded tan on the upper float: the kernel's provisional value is wrong at both.  Two batches of three frames.

    A one-ULP float shift usually leaves the match rows equal either way: what fails without the settle is the xy_un bytes and the
    counters; the rows are compared all the same."""
    cam = _settle_camera(golden)
    px = golden['pixel']
    want = expected(oracle, cam)
    frames = U.frames()
    ex = _extractor(api, cam)
    raw, und = ex.undistort_verdict(px[None])
    final = oracle.undistort_equidistant(px[None], *cam)
    assert und[0] and raw.tobytes() != final.tobytes()         # the raw verdict differs from the final value at that slot
    slots = []
    for f in (1, 2):
        k = U.extracted(oracle)[f][0]
        hit = np.flatnonzero((k['x'] == px[0]) & (k['y'] == px[1]) & (k['octave'] == 0))
        assert len(hit) == 1
        slots.append(int(hit[0]))
        assert want['xy_un'][f][hit[0]].tobytes() == final.tobytes()
    chain = ex.match_chain()
    try:
        out = []
        for keys in ([0, 1, 2], [0, 1, 2]):
            ex.submit_matched_ptrs(chain, [frames[f].ctypes.data for f in keys], U.H, U.W, U.W, False, want['bounds'])
            out.append(ex.collect_undistorted(matched=True))
            if len(out) == 1:                                   # the resident frame of the batch's last frame: the patched arena
                own = api.Frame.from_extract(ex, 2, want['bounds'])
                assert np.stack([own.download()[0]['x'], own.download()[0]['y']], 1).tobytes() == want['xy_un'][2].tobytes()
    finally:
        ex.free_match_chain(chain)
    (k0, d0, n0, xy0, m0, nm0), (k1, d1, n1, xy1, m1, nm1) = out
    _check_batch(oracle, cam, (k0, d0, n0, m0, nm0), [0, 1, 2], None, xy0)
    _check_batch(oracle, cam, (k1, d1, n1, m1, nm1), [0, 1, 2], 2, xy1)
    s = ex.equidistant_stats()
    plan = _settle_plan(oracle, cam, ([0, 1, 2], [0, 1, 2]))
    assert tuple(s) == plan
    assert s[1] >= 4 and s[2] >= 4      # two points per batch changed; rows 1, 2 of both batches, row 0 of the second if frame 0 changed


def test_settle_in_the_stream_runner(api, oracle, golden):
    cam = _settle_camera(golden)
    want = expected(oracle, cam)
    frames = U.frames()
    st = api.Stream(U.NFEAT, 1.2, U.NLEVELS, 20, 7, 0, 3, depth=2)
    try:
        st.set_camera_equidistant(*cam)
        st.set_matching(want['bounds'])
        pushes = ([0, 1, 2], [1, 0, 2], [0, 1, 2])              # both in flight at once: the second batch read a stale carry
        for keys in pushes:
            st.push_ptrs([frames[f].ctypes.data for f in keys], U.H, U.W, U.W, on_device=False)
        pred = None
        for keys in pushes:
            got = st.pop(copy=True)
            _check_batch(oracle, cam, got, keys, pred, st.xy_un())
            pred = keys[-1]
        s = st.equidistant_stats()
        assert tuple(s) == _settle_plan(oracle, cam, pushes) and s[1] >= 6
    finally:
        st.close()


def test_chain_starts_over_when_the_camera_changes(api, oracle, golden):
    """A carry written under another model, or under an equidistant camera with other intrinsics, is no predecessor."""
    frames = U.frames()
    ex = _extractor(api)
    chain = ex.match_chain()
    try:
        def batch(keys, bounds):
            ex.submit_matched_ptrs(chain, [frames[f].ctypes.data for f in keys], U.H, U.W, U.W, False, bounds)
            return ex.collect_undistorted(matched=True)
        eb = expected(oracle, E.SONY)['bounds']
        k, d, n, xy, m12, nm = batch([0, 1], eb)
        wn, wm = pair(oracle, E.SONY, 0, 1)
        assert nm[0] == 0 and nm[1] == wn and (m12[1, :len(wm)] == wm).all()
        ex.set_camera_equidistant(*_settle_camera(golden))          # other intrinsics
        k, d, n, xy, m12, nm = batch([2], eb)
        assert nm[0] == 0 and (m12[0] == -1).all()
        fx, fy, cx, cy, dist = U.CAMERAS['k5']                       # the other model
        ex.set_camera(fx, fy, cx, cy, dist)
        pb = U.expected(oracle, 'k5')['bounds']
        k, d, n, xy, m12, nm = batch([1], pb)
        assert nm[0] == 0 and (m12[0] == -1).all()
        k, d, n, xy, m12, nm = batch([2], pb)                        # ... and the chain goes on under the new camera
        wn, wm = U.pair(oracle, 'k5', 1, 2)
        assert nm[0] == wn and (m12[0, :len(wm)] == wm).all()
        ex.set_camera_equidistant(*E.SONY)                           # back: the pinhole carry is no predecessor either
        k, d, n, xy, m12, nm = batch([0], eb)
        assert nm[0] == 0 and (m12[0] == -1).all()
    finally:
        ex.free_match_chain(chain)
