"""Shared by tests/test_source_projection.py and tests/test_gpu_source_projection.py: the reference restatement of the source
projection (tests/cpp/project_sources_ref.cpp, built here with g++ -ffp-contract=off), ctypes bindings of the oracle's
whole-function restatements orc_sbp_frame / orc_sbp_keyframe (oracle/orb_oracle_pose.h), and the scenes both files search.

A scene: frames A and B = A shifted by (3, -2) px.  Source i is keypoint i of A (the "last frame" / the keyframe); its
MapPoint is triangulated from that keypoint at a varied depth, with mfMaxDistance = dist * mvScaleFactors[octave] and
mfMinDistance = mfMaxDistance / mvScaleFactors[nlevels - 1] as MapPoint::UpdateNormalAndDepth sets them
(src/MapPoint.cc:315-355).  MapPoint ids are rows of the device table; rows[i] names the MapPoint of source i (a permutation,
a few MapPoints named by two sources).  isBad(), Observations() and membership in sAlreadyFound are states of the MapPoint,
"no MapPoint / outlier" is a state of the source: the flag bytes of the GPU calls and the oracle's arrays are two views of
the same states."""
import ctypes as C
import os
import subprocess

import numpy as np

import local_map_util as U
from oracle.pyoracle import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.path.join(ROOT, 'tests', 'cpp', 'project_sources_ref.cpp')
LAST_FRAME, KEYFRAME = 0, 1
MP_BAD, MP_OBSERVED, MP_SKIP = 2, 8, 16
TH_HIGH = 100

_p = U._p


class OrcView(C.Structure):
    _fields_ = [('kpsUn', C.c_void_p), ('desc', C.c_void_p), ('n', C.c_int), ('bounds', C.c_float * 4), ('fx', C.c_float),
                ('fy', C.c_float), ('cx', C.c_float), ('cy', C.c_float), ('scaleFactors', C.c_void_p),
                ('invLevelSigma2', C.c_void_p), ('nlevels', C.c_int), ('logScaleFactor', C.c_float)]


class OrcPoints(C.Structure):
    _fields_ = [('M', C.c_int), ('pos', C.c_void_p), ('normal', C.c_void_p), ('mfMinDistance', C.c_void_p),
                ('mfMaxDistance', C.c_void_p), ('desc', C.c_void_p), ('bad', C.c_void_p), ('nObs', C.c_void_p),
                ('idxInKF', C.c_void_p)]


def bind_oracle(oracle):
    L = oracle.L
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.orc_sbp_frame.argtypes = [C.POINTER(OrcView), vp, vp, vp, ci, vp, vp, C.POINTER(OrcPoints), vp, cf, ci]
    L.orc_sbp_frame.restype = ci
    L.orc_sbp_keyframe.argtypes = [C.POINTER(OrcView), vp, vp, ci, vp, vp, C.POINTER(OrcPoints), vp, cf, ci, ci]
    L.orc_sbp_keyframe.restype = ci
    return L


def build_ref(outdir):
    so = os.path.join(str(outdir), 'project_sources_ref.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC,
                           '-o', so])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ref_project_sources.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    L.ref_project_sources.restype = C.c_int
    return L


def camera_center(R, t):
    """Ow = -Rcw.t()*tcw as ORBmatcher.cc:1431 computes it: gemm with GEMM_1_T, double products summed in order"""
    Ow = np.zeros(3, np.float32)
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += float(R[k, i]) * float(t[k])
        Ow[i] = np.float32(s * -1.0)
    return Ow


def with_center(cam):
    cam = dict(cam)
    cam['Ow'] = camera_center(cam['Rcw'], cam['tcw'])
    return cam


def tcw16(cam):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = cam['Rcw']
    T[:3, 3] = cam['tcw']
    return np.ascontiguousarray(T)


def ref_project(L, tab, rows, flags, src_octave, cam, bounds, mode):
    rows = np.ascontiguousarray(rows, np.int32)
    flags = np.ascontiguousarray(flags, np.uint8)
    octv = np.ascontiguousarray(src_octave, np.int32)
    n = len(rows)
    va = np.zeros(max(n, 1), np.uint8)
    uv = np.zeros((max(n, 1), 2), np.float32)
    lv = np.zeros(max(n, 1), np.int32)
    ca = U.cam_array(cam)
    b = np.asarray(bounds, np.float32)
    pos, mn, mx = (np.ascontiguousarray(tab[k], np.float32) for k in ('pos', 'min', 'max'))
    cnt = L.ref_project_sources(_p(pos), _p(mn), _p(mx), _p(rows), _p(flags), _p(octv), n, _p(ca), _p(b), mode, _p(va), _p(uv),
                                _p(lv))
    return dict(valid=va[:n], uv=uv[:n], level=lv[:n], n_valid=cnt)


def check_projection(got, want):
    assert got['n_valid'] == want['n_valid']
    assert (got['valid'] == want['valid']).all()
    assert got['uv'].tobytes() == want['uv'].tobytes()
    assert (got['level'] == want['level']).all()


def frames(W, H, nfeat, seed=11, extractor=None):
    """keypoints and descriptors of frame A and of B = A shifted by (3, -2) px, the scale factors.  extractor: an object
    with __call__(image) -> (kps, desc) and tables(); default the CPU oracle's"""
    from os1_amd.synth import shifted, synth
    A = synth(seed, W, H)
    B = shifted(A, 3, -2, seed + 1)
    if extractor is None:
        from oracle.pyoracle import OracleExtractor
        ex = OracleExtractor(nfeat, 1.2, 8, 20, 7)
        kA, dA = ex.extract(A)
        kB, dB = ex.extract(B)
    else:
        ex = extractor
        kA, dA = ex(A)
        kB, dB = ex(B)
    return kA, dA, kB, dB, ex.tables()['sf']


def triangulate_keypoints(kps, desc, sf, cam, seed, z0=8.0):
    """MapPoint j from keypoint j of the frame whose camera is `cam` (identity pose): local_map_util.triangulate's
    construction, one point per keypoint"""
    rng = np.random.default_rng(seed)
    n, nlev = len(kps), len(sf)
    near = rng.random(n) < 0.6
    Z = np.where(near, rng.uniform(z0 * 0.97, z0 * 1.03, n), rng.uniform(2.0, 40.0, n)).astype(np.float32)
    X = ((kps['x'].astype(np.float32) - cam['cx']) * Z / cam['fx']).astype(np.float32)
    Y = ((kps['y'].astype(np.float32) - cam['cy']) * Z / cam['fy']).astype(np.float32)
    pos = np.stack([X, Y, Z], 1).astype(np.float32)
    PO = (pos - cam['Ow']).astype(np.float32)
    dist = U._norm(PO)
    normal = (PO / dist[:, None]).astype(np.float32)
    octv = np.minimum(kps['octave'], nlev - 2)
    mx = (dist * sf[octv]).astype(np.float32)
    mn = (mx / sf[nlev - 1]).astype(np.float32)
    d = desc.copy()
    for i in range(n):                                      # 0-24 bit flips
        for b in rng.integers(0, 256, rng.integers(0, 25)):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(pos=pos, normal=normal, min=mn, max=mx, desc=d)


def scene(kA, dA, kB, sf, W, H, seed, skip=0.5, bad=0.03, obs=0.85, occupied=0.10, shared=0.03, already=0.05):
    """The table (row = MapPoint id), rows[i], the MapPoint / source / keypoint states, both cameras"""
    rng = np.random.default_rng(seed)
    camA = with_center(U.camera(W, H))
    cam = with_center(U.moved_camera(W, H, 3, -2, 8.0, seed=seed + 1))
    n = len(kA)
    pts = triangulate_keypoints(kA, dA, sf, camA, seed + 2)
    # depth ranges that reject the point from the moved camera: 2 % too far (1.2f * max < dist), 2 % too near (0.8f * min > dist)
    dist = U._norm((pts['pos'] - cam['Ow']).astype(np.float32))
    r = rng.random(n)
    far, nearr = r < 0.02, (r >= 0.02) & (r < 0.04)
    pts['max'][far] = (dist[far] * np.float32(0.7)).astype(np.float32)
    pts['min'][far] = (pts['max'][far] * np.float32(0.1)).astype(np.float32)
    pts['min'][nearr] = (dist[nearr] * np.float32(1.5)).astype(np.float32)
    pts['max'][nearr] = (dist[nearr] * np.float32(2.0)).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)              # MapPoint of source i = row perm[i]
    tab = {k: np.zeros_like(v) for k, v in pts.items()}
    for k in pts:
        tab[k][perm] = pts[k]
    rows = perm.copy()
    twice = np.flatnonzero(rng.random(n) < shared)          # these sources name the MapPoint of another source
    rows[twice] = perm[rng.integers(0, n, len(twice))]
    st = dict(bad=(rng.random(n) < bad).astype(np.uint8), nObs=(rng.random(n) < obs).astype(np.int32),
              already=(rng.random(n) < already).astype(np.uint8), absent=(rng.random(n) < skip).astype(np.uint8),
              occ=(rng.random(len(kB)) < occupied).astype(np.uint8))
    return dict(tab=tab, rows=rows, st=st, camA=camA, cam=cam, n=n, bounds=(0.0, float(W), 0.0, float(H)))


def flags_of(S, mode):
    """the GPU calls' flag bytes of scene S"""
    st, rows = S['st'], S['rows']
    fl = np.zeros(S['n'], np.uint8)
    fl[st['nObs'][rows] > 0] |= MP_OBSERVED
    fl[st['bad'][rows] != 0] |= MP_BAD                      # (LAST_FRAME mode does not ask isBad(): the call ignores the bit)
    skip = st['absent'] != 0
    if mode == KEYFRAME:
        skip = skip | (st['already'][rows] != 0)
    fl[skip] |= MP_SKIP
    return fl


def oracle_search(L, S, mode, kA, kB, dB, sf, cam, th, max_dist, check_ori):
    """orc_sbp_frame / orc_sbp_keyframe on scene S: (nmatches, CurrentFrame.mvpMapPoints as ids afterwards, before).  An
    occupied keypoint holds MapPoint M (one extra id with Observations() = 1)."""
    tab, st, rows, n = S['tab'], S['st'], S['rows'], S['n']
    M = n
    kA = np.ascontiguousarray(kA, KP_DTYPE)
    kB = np.ascontiguousarray(kB, KP_DTYPE)
    dB = np.ascontiguousarray(dB, np.uint8)
    sf = np.ascontiguousarray(sf, np.float32)
    is2 = np.ascontiguousarray(1.0 / (sf * sf), np.float32)
    ext = lambda a, v: np.ascontiguousarray(np.concatenate([a, np.asarray(v, a.dtype).reshape((1,) + a.shape[1:])]))
    pos, nrm = ext(tab['pos'], np.zeros(3)), ext(tab['normal'], np.zeros(3))
    mn, mx, desc = ext(tab['min'], [0]), ext(tab['max'], [0]), ext(tab['desc'], np.zeros(32))
    bad, nObs = ext(st['bad'], [0]), ext(st['nObs'], [1])
    idx = np.full(M + 1, -1, np.int32)
    P = OrcPoints(M + 1, _p(pos), _p(nrm), _p(mn), _p(mx), _p(desc), _p(bad), _p(nObs), _p(idx))
    V = OrcView(_p(kB), _p(dB), len(kB), (C.c_float * 4)(*S['bounds']), cam['fx'], cam['fy'], cam['cx'], cam['cy'], _p(sf),
                _p(is2), len(sf), cam['lsf'])
    T = tcw16(cam)
    cur = np.where(st['occ'] != 0, M, -1).astype(np.int32)
    before = cur.copy()
    src_mp = np.where(st['absent'] != 0, -1, rows).astype(np.int32)
    if mode == LAST_FRAME:
        outlier = np.zeros(n, np.uint8)
        nm = L.orc_sbp_frame(C.byref(V), _p(T), _p(kA), _p(kA), n, _p(src_mp), _p(outlier), C.byref(P), _p(cur), th,
                             int(check_ori))
    else:
        already = ext(st['already'], [0])
        nm = L.orc_sbp_keyframe(C.byref(V), _p(T), _p(kA), n, _p(src_mp), _p(already), C.byref(P), _p(cur), th, int(max_dist),
                                int(check_ori))
    return nm, cur, before


def cur_mp_from_assigned(before, assigned, rows):
    """CurrentFrame.mvpMapPoints after the write-back of a kp_assigned vector (source index, -1, -2 = cleared)"""
    cur = before.copy()
    a = np.asarray(assigned)
    hit = a >= 0
    cur[hit] = rows[a[hit]]
    cur[a == -2] = -1
    return cur


def edge_sources(S, sf):
    """Edge MapPoints appended to scene S's table and given to its first sources (always projected): local_map_util.edge_points
    for the identity camera (behind the camera, on and one float beyond each bound, 0.8f * min / 1.2f * max +- 1 ulp,
    mfMaxDistance = dist * sf[l] for every level) plus z = +-0 with x = y = 0 and with x != 0.  Returns the scene's copy and
    the indices of the edge sources."""
    E = U.edge_points(S['camA'], S['bounds'], sf)
    z = [(0.0, 0.0, 0.0), (0.0, 0.0, -0.0), (0.3, 0.0, 0.0), (-0.3, 0.0, 0.0), (0.3, 0.0, -0.0), (0.0, 0.2, -0.0),
         (0.0, 0.0, 1e-30), (0.0, 0.0, -1e-30)]
    Z = dict(pos=np.array(z, np.float32), normal=np.tile(np.float32([0, 0, 1]), (len(z), 1)), min=np.zeros(len(z), np.float32),
             max=np.full(len(z), 60.0, np.float32), desc=np.zeros((len(z), 32), np.uint8))
    E = U.concat(E, Z)
    ne = len(E['pos'])
    assert ne < S['n']
    S2 = dict(S)
    S2['tab'] = U.concat(S['tab'], E)
    S2['rows'] = S['rows'].copy()
    S2['rows'][:ne] = S['n'] + np.arange(ne)
    st = {k: v.copy() for k, v in S['st'].items()}
    st['bad'] = np.concatenate([st['bad'], np.zeros(ne, np.uint8)])
    st['nObs'] = np.concatenate([st['nObs'], np.ones(ne, np.int32)])
    st['already'] = np.concatenate([st['already'], np.zeros(ne, np.uint8)])
    st['absent'][:ne] = 0
    S2['st'] = st
    return S2, np.arange(ne)


# (th, max_dist) of the fused cases: Tracking::TrackWithMotionModel's th = 15 and 30 (and 7, the stereo value) with TH_HIGH;
# Tracking::Relocalization's (10, 100) and (3, 64)
CASES = {LAST_FRAME: [(7.0, TH_HIGH), (15.0, TH_HIGH), (30.0, TH_HIGH)], KEYFRAME: [(10.0, 100), (3.0, 64)]}


def case_seed(mode, th, W):
    return 1000 * (mode + 1) + 10 * int(th) + (1 if W >= 1920 else 0)


def rejected_by_distance(L, sc, flags, src_octave, cam):
    """KEYFRAME mode: sources the 0.8f * min bound alone rejects, sources the 1.2f * max bound alone rejects (the restatement
    run again with that bound out of the way)"""
    base = ref_project(L, sc['tab'], sc['rows'], flags, src_octave, cam, sc['bounds'], KEYFRAME)['valid']
    t1 = dict(sc['tab'])
    t1['min'] = np.zeros_like(t1['min'])
    by_min = ref_project(L, t1, sc['rows'], flags, src_octave, cam, sc['bounds'], KEYFRAME)['valid'] & ~base & 1
    t2 = dict(sc['tab'])
    t2['max'] = np.full_like(t2['max'], 3e38)
    by_max = ref_project(L, t2, sc['rows'], flags, src_octave, cam, sc['bounds'], KEYFRAME)['valid'] & ~base & 1
    return int(by_min.sum()), int(by_max.sum())


def checked_oracle_case(L, oracle, sc, mode, kA, kB, dB, sf, th, max_dist, check_ori, W, info):
    """One fused case on the CPU: the whole-function oracle's result, with the conditions that keep the case from passing
    vacuously asserted on it.  info['pruned'] collects the slots the rotation check cleared."""
    flags = flags_of(sc, mode)
    cam = sc['cam']
    proj = ref_project(L, sc['tab'], sc['rows'], flags, kA['octave'], cam, sc['bounds'], mode)
    v = proj['valid'] == 1
    assert ((proj['level'][v] >= 0) & (proj['level'][v] < len(sf))).all()   # (the oracle indexes mvScaleFactors with it)
    skipmask = MP_SKIP | (MP_BAD if mode == KEYFRAME else 0)
    nonskip = (flags & skipmask) == 0
    assert 3 * v.sum() >= nonskip.sum() > 0
    if mode == KEYFRAME:
        by_min, by_max = rejected_by_distance(L, sc, flags, kA['octave'], cam)
        assert by_min >= 1 and by_max >= 1
    nm, cur, before = oracle_search(oracle.L, sc, mode, kA, kB, dB, sf, cam, th, max_dist, check_ori)
    assert nm > (100 if W >= 1920 else 25), nm
    if check_ori:
        nm0, _, _ = oracle_search(oracle.L, sc, mode, kA, kB, dB, sf, cam, th, max_dist, False)
        info['pruned'] += nm0 - nm
    return dict(nmatches=nm, cur_mp=cur, before=before, proj=proj, flags=flags)


def assert_edges(L, sc, edge, kA, sf):
    """both modes' projections of the edge scene under the identity camera; the scene holds a point behind the camera that
    LAST_FRAME rejects and KEYFRAME keeps, valid and invalid edge sources, and levels outside the pyramid"""
    out = {}
    for mode in (LAST_FRAME, KEYFRAME):
        out[mode] = ref_project(L, sc['tab'], sc['rows'], flags_of(sc, mode), kA['octave'], sc['camA'], sc['bounds'], mode)
    z = sc['tab']['pos'][sc['rows'][edge], 2]
    behind = edge[z < 0]
    lf, kf = out[LAST_FRAME]['valid'], out[KEYFRAME]['valid']
    assert ((lf[behind] == 0) & (kf[behind] == 1)).any()
    assert kf[edge].any() and not kf[edge].all() and lf[edge].any() and not lf[edge].all()
    assert (out[KEYFRAME]['level'][edge][kf[edge] == 1] >= len(sf)).any()
    return out
