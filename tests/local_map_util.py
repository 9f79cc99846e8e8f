"""Shared by tests/test_local_map.py and tests/test_gpu_local_map.py: the reference restatement of the local-map projection
(tests/cpp/is_in_frustum_ref.cpp, built here with g++ -ffp-contract=off) and the scenes the GPU tests project.

A scene: MapPoints triangulated from frame A's keypoints of a synthetic pair at varied depths, with mfMaxDistance =
dist * mvScaleFactors[octave] and mfMinDistance = mfMaxDistance / mvScaleFactors[nlevels - 1] as
MapPoint::UpdateNormalAndDepth sets them (src/MapPoint.cc:315-355), the normal = the unit viewing ray of frame A.  Seen from
frame A's own pose the predicted level lands exactly on the octave (the ulp-sensitive case of PredictScale); from a slightly
moved pose it lands near it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.path.join(ROOT, 'tests', 'cpp', 'is_in_frustum_ref.cpp')

_libm = C.CDLL('libm.so.6')
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x):
    """host libm logf of one float"""
    return np.float32(_libm.logf(float(np.float32(x))))


def build_ref(outdir):
    so = os.path.join(str(outdir), 'is_in_frustum_ref.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC,
                           '-o', so])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ref_search_local_points_projection.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_float, vp, vp, vp, vp]
    L.ref_search_local_points_projection.restype = C.c_int
    L.ref_logf_array.argtypes = [vp, C.c_int, vp]
    L.ref_logf_array.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cam_array(cam):
    """OrbfeCamera fields as 20 floats (the reference restatement's layout)"""
    return np.array(list(cam['Rcw'].ravel()) + list(cam['tcw']) + list(cam['Ow']) +
                    [cam['fx'], cam['fy'], cam['cx'], cam['cy'], cam['lsf']], np.float32)


def ref_project(L, mp, rows, flags, cam, bounds, cos_limit=0.5):
    rows = np.ascontiguousarray(rows, np.int32)
    flags = np.ascontiguousarray(flags, np.uint8)
    n = len(rows)
    iv = np.zeros(max(n, 1), np.uint8)
    xy = np.zeros((max(n, 1), 2), np.float32)
    lv = np.zeros(max(n, 1), np.int32)
    vc = np.zeros(max(n, 1), np.float32)
    ca = cam_array(cam)
    b = np.asarray(bounds, np.float32)
    cnt = L.ref_search_local_points_projection(_p(mp['pos']), _p(mp['normal']), _p(mp['min']), _p(mp['max']), _p(rows),
                                               _p(flags), n, _p(ca), _p(b), float(np.float32(cos_limit)), _p(iv), _p(xy),
                                               _p(lv), _p(vc))
    return dict(in_view=iv[:n], proj_xy=xy[:n], level=lv[:n], view_cos=vc[:n], n_in_view=cnt)


def api_camera(api, cam):
    return api.Camera.make(cam['Rcw'], cam['tcw'], cam['Ow'], cam['fx'], cam['fy'], cam['cx'], cam['cy'], cam['lsf'])


def _norm(v):
    """(float) cv::norm of float rows: double accumulation, sqrt, rounded to float"""
    v = v.astype(np.float64)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]).astype(np.float32)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


def camera(W, H, R=None, t=None):
    """OrbfeCamera values of a Frame with pose [R | t]: Ow = -R^T t as Frame::UpdatePoseMatrices computes it (double
    accumulation, rounded to float)"""
    f = np.float32(0.47 * W)
    R = np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32)
    t = np.zeros(3, np.float32) if t is None else np.asarray(t, np.float32)
    Ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    return dict(Rcw=R, tcw=t, Ow=Ow, fx=f, fy=f, cx=np.float32(W / 2), cy=np.float32(H / 2), lsf=logf(1.2))


def moved_camera(W, H, dx, dy, z0, seed):
    """a pose under which points at depth z0 move by (dx, dy) px (the shift of frame B), plus a small rotation"""
    rng = np.random.default_rng(seed)
    f = np.float32(0.47 * W)
    R = rotation(rng.normal(size=3), 4e-4)
    t = np.array([dx * z0 / f, dy * z0 / f, 0.01], np.float32)
    return camera(W, H, R, t)


def triangulate(kps, desc, sf, n_mp, cam, seed, z0=8.0, max_octave=None):
    """n_mp MapPoints from keypoints of the frame whose camera is `cam` (identity pose); rows of a local map"""
    rng = np.random.default_rng(seed)
    nlev = len(sf)
    max_octave = nlev - 2 if max_octave is None else max_octave
    src = rng.integers(0, len(kps), n_mp)
    near = rng.random(n_mp) < 0.6
    Z = np.where(near, rng.uniform(z0 * 0.97, z0 * 1.03, n_mp), rng.uniform(2.0, 40.0, n_mp)).astype(np.float32)
    x = kps['x'][src].astype(np.float32)
    y = kps['y'][src].astype(np.float32)
    X = ((x - cam['cx']) * Z / cam['fx']).astype(np.float32)
    Y = ((y - cam['cy']) * Z / cam['fy']).astype(np.float32)
    pos = np.stack([X, Y, Z], 1).astype(np.float32)
    PO = (pos - cam['Ow']).astype(np.float32)
    dist = _norm(PO)
    normal = (PO / dist[:, None]).astype(np.float32)
    octv = np.minimum(kps['octave'][src], max_octave)
    mx = (dist * sf[octv]).astype(np.float32)
    mn = (mx / sf[nlev - 1]).astype(np.float32)
    d = desc[src].copy()
    for i in range(n_mp):                                   # 0-24 bit flips
        for b in rng.integers(0, 256, rng.integers(0, 25)):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(pos=pos, normal=normal, min=mn, max=mx, desc=d)


def flags_for(n, seed, bad=0.03, skip=0.05, cand=0.05, obs=0.85):
    rng = np.random.default_rng(seed)
    fl = np.zeros(n, np.uint8)
    fl[rng.random(n) < obs] |= 8
    fl[rng.random(n) < cand] |= 4
    fl[rng.random(n) < bad] |= 2
    fl[rng.random(n) < skip] |= 16
    return fl


def oracle_flags(proj, flags):
    """the MapPoint flags SearchByProjection sees after the projection: mbTrackInView, plCandidato, Observations() > 0"""
    return (proj['in_view'].astype(np.uint8) | (flags & np.uint8(4 | 8))).astype(np.uint8)


def _floats_around(x, k):
    x = np.float32(x)
    out = [x]
    up = dn = x
    for _ in range(k):
        up = np.nextafter(up, np.float32(np.inf), dtype=np.float32)
        dn = np.nextafter(dn, np.float32(-np.inf), dtype=np.float32)
        out += [up, dn]
    return np.array(out, np.float32)


def edge_points(cam, bounds, sf):
    """MapPoints on the edges of isInFrustum for the identity camera `cam` (Pc = P, PO = P): behind the camera, projecting
    on and one float beyond each image bound, at distances 0.8*min and 1.2*max and one float either side, viewing cosines at
    0.5 and around 0.998.  Their predicted levels may lie outside the pyramid (projection tests only)."""
    fx, cx, fy, cy = cam['fx'], cam['cx'], cam['fy'], cam['cy']
    f32 = np.float32
    pos, nrm, mn, mx = [], [], [], []

    def add(p, n=(0, 0, 1), lo=f32(0.5), hi=f32(60.0)):
        pos.append(np.array(p, np.float32)); nrm.append(np.array(n, np.float32)); mn.append(f32(lo)); mx.append(f32(hi))
    Z = f32(10.0)
    add((0.1, 0.2, -5.0))                                   # behind the camera
    add((0.0, 0.0, -1e-7))
    invz = f32(1.0) / Z
    for b, (f, c, axis) in zip(bounds, [(fx, cx, 0), (fx, cx, 0), (fy, cy, 1), (fy, cy, 1)]):
        x0 = f32((f32(b) - c) * Z / f)
        for X in _floats_around(x0, 40):
            u = f32(f32(f * X) * invz) + c
            if abs(float(u) - float(b)) <= 2e-4 * max(1.0, abs(float(b))):
                p = [0.0, 0.0, Z]
                p[axis] = X
                add(p)
    P = (0.0, 0.0, Z)                                       # dist = Z exactly
    for m in _floats_around(Z / f32(1.2), 3):               # 1.2f * max around dist
        add(P, lo=f32(0.5), hi=m)
    for m in _floats_around(Z / f32(0.8), 3):               # 0.8f * min around dist
        add(P, lo=m, hi=f32(1e3))
    for c0 in (f32(0.5), f32(0.998)):                       # viewing cosines
        for c in _floats_around(c0, 3):
            s = f32(np.sqrt(max(0.0, 1.0 - float(c) * float(c))))
            add(P, n=(s, 0.0, c), lo=f32(8.0), hi=f32(9.0))
    # the ulp-sensitive PredictScale: mfMaxDistance = dist * mvScaleFactors[level] for every level
    for lv in range(len(sf)):
        add(P, lo=f32(0.01), hi=f32(Z * sf[lv]))
    return dict(pos=np.array(pos, np.float32), normal=np.array(nrm, np.float32), min=np.array(mn, np.float32),
                max=np.array(mx, np.float32), desc=np.zeros((len(pos), 32), np.uint8))


def concat(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}
