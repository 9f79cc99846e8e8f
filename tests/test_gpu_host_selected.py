"""-m gpu: what a HOST-selected batch (quadtree.h writing the arena's slots) shares with every other batch since the host quadtree
became a stage of the one submit / collect path: colour input, the fused vocabulary descent, resident frames built from the arena,
and a match chain across batches.  Each on the 1600 x 100 strip (23-29 roots per level: outside the GPU quadtree's limits, and
4 x roots exceeds every level's quota) and at 640 x 480 under ORBFE_HOST_QUADTREE=1.  Everything is compared with equality."""
import ctypes as C

import numpy as np
import pytest

from dbow2_ref_util import voc_image
from oracle.pyoracle import OracleExtractor
from os1_amd.synth import shifted, synth

pytestmark = pytest.mark.gpu

# name -> (cols, rows, nfeatures, nlevels, ORBFE_HOST_QUADTREE, seed)
CASES = {'strip': (1600, 100, 200, 3, None, 82), 'forced': (640, 480, 500, 8, '1', 83)}
# a mild, distorting pinhole model for the strip: |x| <= 1 in normalised coordinates, so 1 + k1 r^2 + k2 r^4 stays near 0.9
STRIP_CAMERA = (800.0, 800.0, 800.0, 50.0, (-0.1, 0.01, 0.0005, -0.0003))
_SHARED = {}


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


def _case(oracle, name):
    """Four frames of the case and the oracle's extraction of each; computed once, never changed."""
    if name not in _SHARED:
        W, H, N, nl, _, seed = CASES[name]
        base = synth(seed, W, H)
        frames = [base] + [shifted(base, 3 * i, -i, 900 + i) for i in range(1, 4)]
        ox = OracleExtractor(N, 1.2, nl, 20, 7, oracle)
        _SHARED[name] = dict(frames=frames, want=[ox.extract(f) for f in frames])
    return _SHARED[name]


def _extractor(api, monkeypatch, name):
    W, H, N, nl, env, _ = CASES[name]
    if env is not None:
        monkeypatch.setenv('ORBFE_HOST_QUADTREE', env)      # read when the handle is created
    ex = api.Extractor(N, 1.2, nl, 20, 7)
    monkeypatch.delenv('ORBFE_HOST_QUADTREE', raising=False)
    ex.cap = max(ex.cap, ex.L.orbfe_extractor_max_keypoints_for_size(ex.h, H, W))
    return ex


def _submit_collect(ex, images, cols):
    """The batch through orbfe_extract_batch_submit / _collect -> [(keypoints, descriptors)] per frame."""
    rows = images[0].shape[0]
    ex.submit_ptrs([im.ctypes.data for im in images], rows, cols, images[0].strides[0], False)
    kps, desc, n = ex.collect()
    return [(kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(len(images))]


def _same(got, want):
    assert len(got) == len(want)
    for (gk, gd), (wk, wd) in zip(got, want):
        assert len(gk) == len(wk) and len(gk) > 50
        assert gk.tobytes() == wk.tobytes() and gd.tobytes() == wd.tobytes()


def _check_colour_input(api, oracle, monkeypatch, name):
    W, H, N, nl, env, seed = CASES[name]
    c = _case(oracle, name)
    rng = np.random.default_rng(seed)
    cols = []
    for g in c['frames'][:2]:
        g = g.astype(np.int32)
        cols.append(np.ascontiguousarray(np.stack([np.clip(g + rng.integers(-30, 31, g.shape), 0, 255), np.clip(g + rng.integers(-10, 11, g.shape), 0, 255),
                                                   np.clip(g + rng.integers(-40, 41, g.shape), 0, 255)], axis=-1).astype(np.uint8)))
    ex = _extractor(api, monkeypatch, name)
    ex.set_input_format('rgb')
    got = _submit_collect(ex, cols, W)
    if name == 'forced':
        # the geometry is inside the GPU quadtree's limits: the product's own grey image, off a handle on that route, through the SAME handle
        gpu = api.Extractor(N, 1.2, nl, 20, 7)
        gpu.set_input_format('rgb')
        grays = []
        for col in cols:
            gpu.extract_color(col)
            grays.append(np.ascontiguousarray(gpu.level(0)))
        ex.set_input_format('gray')
        _same(got, _submit_collect(ex, grays, W))
    else:
        # no crop of a strip with 23 roots is inside them: the oracle's conversion and the oracle's extractor
        ox = OracleExtractor(N, 1.2, nl, 20, 7, oracle)
        _same(got, [ox.extract(oracle.cvt_gray(col, True, 0)) for col in cols])


def _check_fused_vocabulary_descent(api, oracle, monkeypatch, name):
    W, H = CASES[name][:2]
    c = _case(oracle, name)
    v = api.Vocabulary(voc_image('synth3_10_4'))
    ex = _extractor(api, monkeypatch, name)
    ex.set_vocabulary(v, 4)
    got = _submit_collect(ex, c['frames'][:2], W)
    _same(got, c['want'][:2])
    for f, (k, d) in enumerate(got):
        leaf, node = np.zeros(len(k), np.uint32), np.zeros(len(k), np.uint32)
        n = C.c_int(0)
        assert ex.L.orbfe_extract_bow_raw(ex.h, f, leaf.ctypes.data, node.ctypes.data, len(k), C.byref(n)) == 0
        assert n.value == len(k)
        a, b = v.assemble(leaf, node), v.transform(d, 4)
        for x, y in zip((a[0], a[1], *a[2], a[3], a[4]), (b[0], b[1], *b[2], b[3], b[4])):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    ex.set_vocabulary(None)
    v.close()


def _check_resident_frames_from_the_arena(api, oracle, monkeypatch, name):
    W, H = CASES[name][:2]
    c = _case(oracle, name)
    bounds = (0.0, float(W), 0.0, float(H))
    ex = _extractor(api, monkeypatch, name)
    m = api.Matcher(0)
    got = _submit_collect(ex, c['frames'][:2], W)
    _same(got, c['want'][:2])
    own = [api.Frame.from_extract(ex, f, bounds) for f in range(2)]
    sent = [api.Frame.from_host(m, k, d, bounds) for k, d in got]
    down = []
    for a, b in zip(own, sent):
        da, db = a.download(), b.download()
        assert len(a) == len(b)
        for x, y in zip(da, db):
            assert x.tobytes() == y.tobytes()
        down.append((da, db))
    res = []
    for side in (0, 1):
        (k1, d1), (k2, d2) = down[0][side][:2], down[1][side][:2]
        res.append(m.search_for_initialization(k1, d1, k2, d2, bounds, np.stack([k1['x'], k1['y']], 1), 100, 0.9, True))
    assert res[0][0] == res[1][0] and res[0][0] > 20 and res[0][1].tobytes() == res[1][1].tobytes()
    for f in own + sent:
        f.close()


def _chain_expectation(oracle, c, camera, W, H):
    """per frame pair (i - 1, i): the oracle's SearchForInitialization on mvKeysUn, vbPrevMatched := F1's mvKeysUn"""
    key = ('chain', camera is not None)
    if key not in c:
        if camera is None:
            xy = [np.stack([k['x'], k['y']], 1).astype(np.float32) for k, _ in c['want']]
            bounds = np.asarray((0.0, W, 0.0, H), np.float32)
        else:
            fx, fy, cx, cy, dist = camera
            xy = [oracle.undistort_pinhole(np.stack([k['x'], k['y']], 1).astype(np.float32), fx, fy, cx, cy, dist) for k, _ in c['want']]
            bounds = oracle.image_bounds(W, H, 0, fx, fy, cx, cy, dist)
        un = []
        for (k, _), p in zip(c['want'], xy):
            u = k.copy()
            u['x'], u['y'] = p[:, 0], p[:, 1]
            un.append(u)
        pairs = [None]
        for i in range(1, 4):
            n, m12, _ = oracle.search_for_initialization(un[i - 1], c['want'][i - 1][1], un[i], c['want'][i][1], bounds, xy[i - 1], 100, 0.9, True)
            pairs.append((n, m12.copy()))
        c[key] = dict(xy=xy, bounds=bounds, pairs=pairs)
    return c[key]


def _check_match_chain_across_two_batches(api, oracle, monkeypatch, name, camera):
    W, H = CASES[name][:2]
    c = _case(oracle, name)
    e = _chain_expectation(oracle, c, camera, W, H)
    ex = _extractor(api, monkeypatch, name)
    if camera is not None:
        ex.set_camera(*camera[:4], dist=camera[4])
        assert any((a != np.stack([k['x'], k['y']], 1)).any() for a, (k, _) in zip(e['xy'], c['want']))      # the camera does distort
    chain = ex.match_chain()
    total = 0
    try:
        for b in range(2):
            ex.submit_matched_ptrs(chain, [f.ctypes.data for f in c['frames'][2 * b:2 * b + 2]], H, W, W, False, e['bounds'])
            kps, desc, n, xy, m12, nm = ex.collect_undistorted(matched=True)
            for i in range(2):
                g = 2 * b + i
                wk, wd = c['want'][g]
                assert kps[i, :n[i]].tobytes() == wk.tobytes() and desc[i, :n[i]].tobytes() == wd.tobytes()
                assert xy[i, :n[i]].tobytes() == e['xy'][g].tobytes()
                if g == 0:
                    assert nm[i] == 0 and (m12[i] == -1).all()
                    continue
                wn, wm = e['pairs'][g]            # batch 2's frame 0 against batch 1's last frame
                assert nm[i] == wn and (m12[i, :len(wm)] == wm).all() and (m12[i, len(wm):] == -1).all()
                total += wn
    finally:
        ex.free_match_chain(chain)
    assert total > 60


def test_host_selected_batches_take_the_one_path(api, oracle, monkeypatch):
    """One test for all of it (about four seconds): the cases share their frames and the oracle's extraction of them."""
    for name in CASES:
        _check_colour_input(api, oracle, monkeypatch, name)
        _check_fused_vocabulary_descent(api, oracle, monkeypatch, name)
        _check_resident_frames_from_the_arena(api, oracle, monkeypatch, name)
    for name, camera in [('strip', None), ('strip', STRIP_CAMERA), ('forced', None)]:
        _check_match_chain_across_two_batches(api, oracle, monkeypatch, name, camera)

