"""The one launch rule of the window kernel (os1_amd/csrc/window_plan.h, launch_window_match in orbfe_window.hip) on both of its
callers.  One frame of 200 keypoints on bounds 0..640 x 0..480 (64 grid columns of 10 pixels: invW = 0.1), and per call ONE
radius for every query, so the call's widest window, 2 r / 10 + 3 columns, selects the lanes per query: 25 | 25.5 (8 | 16 lanes),
65 | 65.5 (16 | 32), 145 | 145.5 (32 | 64) and 400 (every column of the grid).  A class too narrow for its window would lose the
candidates of the columns beyond its lanes.  Each call goes through

  Matcher.window_candidates                   the host-array route (HostSearch::candidates, orbfe_matcher.hip)
  Matcher.search_projected on a Frame         the resident route (run_search, orbfe_frame.hip)

and must give what the oracle's window query (Frame::GetFeaturesInArea) and descriptor distance give: the ordered candidate
lists with their distances, and the first least distance <= max_dist.  70 queries: more than one block at every class (32, 16, 8
and 4 queries per block) and a multiple of none.

The window kernel's older check, radii from 3 to 400 mixed in ONE call on an extracted frame (_mixed_windows, formerly
test_window_candidates_primitive of tests/test_gpu_parity.py), runs first in the same test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUNDS = (0.0, 640.0, 0.0, 480.0)
RADII = (25.0, 25.5, 65.0, 65.5, 145.0, 145.5, 400.0)
NQ, MAX_DIST = 70, 50


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def scene(api):
    rng = np.random.default_rng(2025)
    n = 200
    k = np.zeros(n, api.KP_DTYPE)
    k['x'] = rng.uniform(0, 640, n).astype(np.float32)
    k['y'] = rng.uniform(0, 480, n).astype(np.float32)
    k['octave'] = rng.integers(0, 4, n)
    k['angle'] = rng.uniform(0, 360, n).astype(np.float32)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    # a query: some keypoint's position moved by up to 24 pixels (inside the smallest window), its level or the next, and its
    # descriptor with a few bits flipped -- a match within max_dist, among the candidates of the other keypoints (about 128 bits
    # away); every fourth query lies anywhere up to 30 pixels outside the bounds with a random descriptor
    src = rng.integers(0, n, NQ)
    xy = np.stack([k['x'][src] + rng.uniform(-24, 24, NQ), k['y'][src] + rng.uniform(-24, 24, NQ)], 1).astype(np.float32)
    level = (k['octave'][src] + rng.integers(0, 2, NQ)).astype(np.int32)
    valid = np.ones(NQ, np.uint8)
    valid[::9] = 0
    qd = d[src].copy()
    for q in range(NQ):
        if q % 4 == 3:
            xy[q] = (rng.uniform(-30, 670), rng.uniform(-30, 510))
            qd[q] = rng.integers(0, 256, 32, dtype=np.uint8)
        else:
            for bit in rng.choice(256, int(rng.integers(0, 30)), replace=False):
                qd[q, bit >> 3] ^= np.uint8(1 << (bit & 7))
    m = api.Matcher()
    return dict(m=m, frame=api.Frame.from_host(m, k, d, BOUNDS), k=k, d=d, xy=xy, level=level, valid=valid, qd=qd, want={})


def _want(scene, oracle, r):
    """per query the oracle's candidate list with distances (None: inactive), computed once per radius"""
    if r not in scene['want']:
        lists = []
        for q in range(NQ):
            if not scene['valid'][q]:
                lists.append(None)
                continue
            lv = int(scene['level'][q])
            idx = oracle.get_features_in_area(scene['k'], BOUNDS, float(scene['xy'][q, 0]), float(scene['xy'][q, 1]), float(r), lv - 1, lv)
            lists.append((idx.tolist(), [oracle.hamming(scene['qd'][q], scene['d'][i]) for i in idx]))
        scene['want'][r] = lists
    return scene['want'][r]


def _host_array_route(scene, oracle, r):
    s, want = scene, _want(scene, oracle, r)
    qr = np.where(s['valid'] != 0, np.float32(r), np.float32(-1.0)).astype(np.float32)
    got = s['m'].window_candidates(s['k'], s['d'], BOUNDS, s['xy'][:, 0], s['xy'][:, 1], qr, s['level'] - 1, s['level'], s['qd'])
    total = 0
    for q in range(NQ):
        idx, dist = got[q]
        w = want[q] if want[q] is not None else ([], [])
        assert idx.tolist() == w[0] and dist.tolist() == w[1], (r, q)
        total += len(w[0])
    assert total > 0


def _resident_route(scene, oracle, r):
    s, want = scene, _want(scene, oracle, r)
    radius = np.full(NQ, r, np.float32)
    nm, bi, bd = s['m'].search_projected(s['frame'], None, None, s['xy'], radius, s['level'], s['valid'], s['qd'], None, False, None, 5.99,
                                         MAX_DIST)
    wi, wd = np.full(NQ, -1, np.int32), np.full(NQ, -1, np.int32)
    for q in range(NQ):
        if want[q] is None or not want[q][0]:
            continue
        best = int(np.argmin(want[q][1]))          # the first least distance in GetFeaturesInArea order
        if want[q][1][best] <= MAX_DIST:
            wi[q], wd[q] = want[q][0][best], want[q][1][best]
    assert bi.tolist() == wi.tolist() and bd.tolist() == wd.tolist(), r
    assert nm == int((wi >= 0).sum()) and nm > 20


def _mixed_windows(api, oracle):
    """orbfe_window_candidates on an extracted 1280 x 720 frame, radii from 3 to 400 mixed in one call with inactive queries and open
    level ranges: per query the GetFeaturesInArea list in reference order with Hamming distances (the GPU half of Fuse /
    SearchBySim3 / SearchByProjection(KeyFrame*, Scw, ...)).  Moved here from tests/test_gpu_parity.py with the kernel it tests."""
    from os1_amd.synth import synth
    k, d = api.Extractor(1500, 1.2, 8, 20, 7)(synth(33, 1280, 720))
    bounds = (0.0, 1280.0, 0.0, 720.0)
    m = api.Matcher()
    rng = np.random.default_rng(9)
    nq = 300
    qx = rng.uniform(-20, 1300, nq).astype(np.float32)
    qy = rng.uniform(-20, 740, nq).astype(np.float32)
    qr = rng.choice([-1.0, 3.0, 7.5, 25.0, 90.0, 400.0], nq).astype(np.float32)
    lv = rng.integers(0, 8, nq)
    qmin = np.where(rng.random(nq) < 0.2, -1, lv - 1).astype(np.int32)
    qmax = np.where(qmin < 0, -1, lv + rng.integers(0, 2, nq)).astype(np.int32)
    qdesc = d[rng.integers(0, len(k), nq)].copy()
    res = m.window_candidates(k, d, bounds, qx, qy, qr, qmin, qmax, qdesc)
    total = 0
    for q in range(nq):
        idx, dist = res[q]
        if qr[q] < 0:
            assert len(idx) == 0
            continue
        want = oracle.get_features_in_area(k, bounds, float(qx[q]), float(qy[q]), float(qr[q]), int(qmin[q]), int(qmax[q]))
        assert idx.tolist() == want.tolist()
        assert dist.tolist() == [oracle.hamming(qdesc[q], d[i]) for i in want]
        total += len(want)
    assert total > 2000


def test_window_kernel_against_the_oracle(api, scene, oracle):
    """One test: the suite runs again for every later change, and these calls share one frame and one reference per radius."""
    _mixed_windows(api, oracle)
    for r in RADII:
        _host_array_route(scene, oracle, r)
        _resident_route(scene, oracle, r)
