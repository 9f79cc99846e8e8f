"""-m gpu: Frame::UndistortKeyPoints on the GPU (k_undistort) and the streamed SearchForInitialization on mvKeysUn, bit for bit against
the oracle composition of undistort_stream_util (the conditions that make these comparisons meaningful: test_undistort_stream.py)."""
import numpy as np
import pytest

import undistort_stream_util as U

pytestmark = pytest.mark.gpu

ALL = list(U.CAMERAS)


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


def _extractor(api, cam, nlevels=U.NLEVELS):
    ex = api.Extractor(U.NFEAT, 1.2, nlevels, 20, 7, device=0)
    if cam is not None:
        fx, fy, cx, cy, dist = U.CAMERAS[cam]
        ex.set_camera(fx, fy, cx, cy, dist)
    return ex


@pytest.mark.parametrize('cam', ALL)
def test_point_sweep(api, oracle, cam):
    fx, fy, cx, cy, dist = U.CAMERAS[cam]
    ex = _extractor(api, cam)
    seeded = U.seeded_points()
    for pts in [U.crafted_points(cam), seeded] + [seeded[:n] for n in (0, 1, 63, 64, 65)]:
        got = ex.undistort(pts)
        want = oracle.undistort_pinhole(pts, fx, fy, cx, cy, dist) if len(pts) else pts
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (cam, len(pts))
        if len(pts):
            assert got.tobytes() == api.undistort_pinhole(pts, fx, fy, cx, cy, dist).tobytes()


def test_undistort_needs_a_camera_and_equidistant_is_refused(api, oracle):
    ex = _extractor(api, None)
    with pytest.raises(api.OrbfeError):
        ex.undistort(U.seeded_points()[:4])
    with pytest.raises(api.OrbfeError) as e:
        ex.set_camera(500.0, 500.0, 320.0, 240.0, (), mode=1)
    assert e.value.code == -6 and 'tan' in str(e.value)
    k, d = ex(U.frames()[0])                      # the handle stays usable, and without a camera
    wk, wd = U.extracted(oracle)[0]
    assert k.tobytes() == wk.tobytes() and d.tobytes() == wd.tobytes()
    ex.set_camera(*U.CAMERAS['k4'][:4], U.CAMERAS['k4'][4])
    with pytest.raises(api.OrbfeError):
        ex.set_camera(500.0, 500.0, 320.0, 240.0, (), mode=1)
    k, d, xy = ex.extract_undistorted(U.frames()[0])      # ... and keeps the camera it had
    assert xy.tobytes() == U.expected(oracle, 'k4')['xy_un'][0].tobytes()


@pytest.mark.parametrize('cam', ALL)
def test_extraction_yields_mvkeysun(api, oracle, cam):
    ex = _extractor(api, cam)
    want = U.expected(oracle, cam)
    frames = U.frames()
    for f in (0, 2):                               # the one-frame route
        k, d, xy = ex.extract_undistorted(frames[f])
        wk, wd = U.extracted(oracle)[f]
        assert k.tobytes() == wk.tobytes() and d.tobytes() == wd.tobytes()      # unchanged by the camera
        assert xy.tobytes() == want['xy_un'][f].tobytes()
        if U.is_identity(cam):
            assert xy.tobytes() == np.stack([k['x'], k['y']], 1).tobytes()
    ex.submit_ptrs([f.ctypes.data for f in frames], U.H, U.W, U.W, False)       # the batch route
    kps, desc, n, xy = ex.collect_undistorted()
    for f in range(U.NFRAMES):
        wk, wd = U.extracted(oracle)[f]
        assert n[f] == len(wk) and kps[f, :n[f]].tobytes() == wk.tobytes() and desc[f, :n[f]].tobytes() == wd.tobytes()
        assert xy[f, :n[f]].tobytes() == want['xy_un'][f].tobytes()


def _check_batch(oracle, cam, got, keys, pred, xy=None):
    """got = (kps, desc, n, m12, nm) of frames `keys`; pred = the frame before keys[0] (None: no predecessor)."""
    kps, desc, n, m12, nm = got
    for i, f in enumerate(keys):
        wk, wd = U.extracted(oracle)[f]
        assert n[i] == len(wk) and kps[i, :n[i]].tobytes() == wk.tobytes() and desc[i, :n[i]].tobytes() == wd.tobytes(), (cam, i)
        if xy is not None:
            assert xy[i, :n[i]].tobytes() == U.expected(oracle, cam)['xy_un'][f].tobytes(), (cam, i)
        p = pred if i == 0 else keys[i - 1]
        if p is None:
            assert nm[i] == 0 and (m12[i] == -1).all(), (cam, i)
            continue
        wn, wm = U.pair(oracle, cam, p, f)
        assert nm[i] == wn and (m12[i, :len(wm)] == wm).all() and (m12[i, len(wm):] == -1).all(), (cam, i, p, f)


def _chain_run(api, oracle, cam, feed_raw=False):
    ex = _extractor(api, None if feed_raw else cam)
    chain = ex.match_chain()
    try:
        frames = U.frames()
        bounds = U.expected(oracle, cam)['bounds']
        out = []
        for keys in ([0, 1], [2]):                 # 2 + 1 frames: the second submission's frame 0 is matched against the carry
            ex.submit_matched_ptrs(chain, [frames[f].ctypes.data for f in keys], U.H, U.W, U.W, False, bounds)
            out.append(ex.collect_undistorted(matched=True))
        return out
    finally:
        ex.free_match_chain(chain)


@pytest.mark.parametrize('cam', ALL + [None])
def test_chain_across_two_submissions(api, oracle, cam):
    (k0, d0, n0, xy0, m0, nm0), (k1, d1, n1, xy1, m1, nm1) = _chain_run(api, oracle, cam)
    _check_batch(oracle, cam, (k0, d0, n0, m0, nm0), [0, 1], None, xy0)
    _check_batch(oracle, cam, (k1, d1, n1, m1, nm1), [2], 1, xy1)


@pytest.mark.parametrize('cam', ['k5', 'barrel'])
def test_chain_fed_raw_coordinates_is_told_apart(api, oracle, cam):
    """The same submissions from a handle WITHOUT the camera (raw coordinates, the camera's bounds) do not give the expected vectors."""
    (k0, d0, n0, xy0, m0, nm0), (k1, d1, n1, xy1, m1, nm1) = _chain_run(api, oracle, cam, feed_raw=True)
    differs = False
    for (nm, m12), (p, f) in (((nm0[1], m0[1]), (0, 1)), ((nm1[0], m1[0]), (1, 2))):
        wn, wm = U.pair(oracle, cam, p, f)
        differs = differs or nm != wn or bool((m12[:len(wm)] != wm).any())
    assert differs


@pytest.mark.parametrize('cam', ['k5', 'barrel', 'identity'])
def test_stream_matches_on_mvkeysun(api, oracle, cam):
    frames = U.frames()
    st = api.Stream(U.NFEAT, 1.2, U.NLEVELS, 20, 7, 0, 2, depth=2)
    try:
        fx, fy, cx, cy, dist = U.CAMERAS[cam]
        st.set_camera(fx, fy, cx, cy, dist)
        st.set_matching(U.expected(oracle, cam)['bounds'])
        pushes = ([0, 1], [2, 1], [0, 1])
        for keys in pushes:
            st.push_ptrs([frames[f].ctypes.data for f in keys], U.H, U.W, U.W, on_device=False)
        pred = None
        for keys in pushes:
            got = st.pop(copy=True)
            _check_batch(oracle, cam, got, keys, pred, st.xy_un())
            pred = keys[-1]
        with pytest.raises(api.OrbfeError):
            st.set_camera(500.0, 500.0, 320.0, 240.0, (), mode=1)
    finally:
        st.close()


@pytest.mark.parametrize('cam', ['k5', 'barrel'])
def test_multistream_over_two_runners_matches_on_mvkeysun(api, oracle, cam):
    """Two runners on device 0: every batch boundary is a boundary pair of the host bounce; same bytes as the chain."""
    frames = U.frames()
    st = api.MultiStream(U.NFEAT, 1.2, U.NLEVELS, 20, 7, [0, 0], 2, depth=1)
    try:
        fx, fy, cx, cy, dist = U.CAMERAS[cam]
        st.set_camera(fx, fy, cx, cy, dist)
        st.set_matching(U.expected(oracle, cam)['bounds'])
        pushes = ([0, 1], [2, 1], [0, 1])
        for keys in pushes:
            st.push_ptrs([frames[f].ctypes.data for f in keys], U.H, U.W, U.W, on_device=False)
        pred = None
        for keys in pushes:
            got = st.pop(copy=True)
            _check_batch(oracle, cam, got, keys, pred, st.xy_un())
            pred = keys[-1]
        with pytest.raises(api.OrbfeError):
            st.set_camera(500.0, 500.0, 320.0, 240.0, (), mode=1)
    finally:
        st.close()


def test_host_quadtree_route(api, oracle):
    cam = 'k5'
    frames = U.frames('strip')
    want = U.expected(oracle, cam, 'strip')
    ex = _extractor(api, cam, U.STRIP_LEVELS)
    for f in range(2):
        k, d, xy = ex.extract_undistorted(frames[f])
        wk, wd = U.extracted(oracle, 'strip')[f]
        assert k.tobytes() == wk.tobytes() and d.tobytes() == wd.tobytes()
        assert xy.tobytes() == want['xy_un'][f].tobytes()
    chain = ex.match_chain()
    try:
        ex.cap = max(ex.cap, ex.L.orbfe_extractor_max_keypoints_for_size(ex.h, U.STRIP_H, U.STRIP_W))
        ex.submit_matched_ptrs(chain, [f.ctypes.data for f in frames], U.STRIP_H, U.STRIP_W, U.STRIP_W, False, want['bounds'])
        kps, desc, n, xy, m12, nm = ex.collect_undistorted(matched=True)
    finally:
        ex.free_match_chain(chain)
    wn, wm = want['pairs'][0]
    assert nm[0] == 0 and nm[1] == wn and (m12[1, :len(wm)] == wm).all()
    for f in range(2):
        assert xy[f, :n[f]].tobytes() == want['xy_un'][f].tobytes()


def test_resident_frame_takes_mvkeysun_from_the_arena(api, oracle):
    cam = 'barrel'
    e = U.expected(oracle, cam)
    ex = _extractor(api, cam)
    m = api.Matcher(0)
    k, d, xy = ex.extract_undistorted(U.frames()[0])
    own = api.Frame.from_extract(ex, 0, e['bounds'])                       # nothing sent
    sent = api.Frame.from_extract(ex, 0, e['bounds'], e['xy_un'][0])       # the oracle's coordinates, uploaded
    for a, b in zip(own.download(), sent.download()):
        assert a.tobytes() == b.tobytes()
    assert np.stack([own.download()[0]['x'], own.download()[0]['y']], 1).tobytes() == e['xy_un'][0].tobytes()
    # SearchByProjection against both, and against the oracle on the undistorted keypoints
    rng = np.random.default_rng(3)
    src = rng.integers(0, len(k), 300)
    mxy = (e['xy_un'][0][src] + rng.uniform(-3, 3, (300, 2))).astype(np.float32)
    level = k['octave'][src].astype(np.int32)
    viewcos = np.ones(300, np.float32)
    flags = np.full(300, 1 | 8, np.uint8)
    sf = ex.tables()['sf']
    occ = np.zeros(len(k), np.uint8)
    kun = k.copy()
    kun['x'], kun['y'] = e['xy_un'][0][:, 0], e['xy_un'][0][:, 1]
    want = oracle.search_by_projection(kun, d, e['bounds'], sf, occ, mxy, level, viewcos, flags, d[src], 3.0, 0.8)
    for fr in (own, sent):
        n, a = m.search_by_projection(fr, None, None, sf, occ, mxy, level, viewcos, flags, d[src], 3.0, 0.8)
        assert n == want[0] and (a == want[1]).all()
    assert want[0] > 100
