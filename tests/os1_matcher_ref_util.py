"""Shared by tests/test_os1_matcher_ref.py, tests/test_gpu_os1_matcher_ref.py and tools/gen_os1_matcher_golden.py: the ctypes
loader of oracle/_ref/libos1_matcher.so -- the reference's OWN src/ORBmatcher.cc compiled against the stand-ins of oracle/os1_decl/
(oracle/Makefile, oracle/os1_matcher_wrap.cpp) --, the adapters that feed the existing scene formats to it, the scene registry and
the reader of tests/golden/os1_matcher_outputs.npz, the recorded results a checkout without the reference compares against.

Every entry of the library takes the arguments of the oracle's restatement of the same member, so RefBackend IS pyoracle.Oracle with
the functions swapped: Oracle's methods, source_projection_util.oracle_search and keyframe_projection_util.run_oracle all run
unchanged on it.  The two array forms that are no member of ORBmatcher ('uv': a search from the projection on; 'proj': the projected
best-match loop) go through Whole: it builds the pose, camera and MapPoints for which the WHOLE member projects every query exactly
onto its (u, v) and predicts exactly its level, and calls the member -- on the library and, the same way, on the oracle's
whole-function restatement.  A scene no member can express raises Unmappable with the reason.

A scene of the registry is (key, runner): runner(backend) -> {field: array}, everything the member lets a caller observe."""
import ctypes as C
import os

import numpy as np

import bow_boundary_util as BB
import keyframe_projection_util as KP
import search_boundary_util as SB
import source_projection_util as SP
from oracle.pyoracle import KP_DTYPE, Oracle

ROOT = SP.ROOT
LIB = os.path.join(ROOT, 'oracle', '_ref', 'libos1_matcher.so')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'os1_matcher_outputs.npz')
_p = SP._p
OrcView, OrcPoints = SP.OrcView, SP.OrcPoints
F32 = np.float32

# orc_* of the oracle -> os1_* of the library (same arguments)
SAME_ARGS = {'orc_search_by_projection': 'os1_search_by_projection', 'orc_search_for_initialization': 'os1_search_for_initialization',
             'orc_search_by_bow': 'os1_search_by_bow', 'orc_search_by_bow_kf': 'os1_search_by_bow_kf',
             'orc_search_for_triangulation': 'os1_search_for_triangulation', 'orc_hamming': 'os1_descriptor_distance',
             'orc_sbp_frame': 'os1_sbp_frame', 'orc_sbp_keyframe': 'os1_sbp_keyframe', 'orc_sbp_scw': 'os1_sbp_scw', 'orc_fuse': 'os1_fuse',
             'orc_fuse_scw': 'os1_fuse_scw', 'orc_search_by_sim3': 'os1_search_by_sim3'}

def have_lib():
    return os.path.exists(LIB)


class _Alias:
    """the library's functions under the oracle's names"""

    def __init__(self, lib, oracle):
        self._lib = lib
        for o, r in SAME_ARGS.items():
            f = getattr(lib, r)
            f.restype = C.c_int
            at = getattr(getattr(oracle.L, o), 'argtypes', None)
            if at:
                f.argtypes = at
            setattr(self, o, f)


class RefBackend(Oracle):
    """pyoracle.Oracle's methods on the reference's compiled ORBmatcher.cc"""

    def __init__(self, oracle):
        lib = self.lib = C.CDLL(LIB)
        lib.os1_matcher_is_reference_build.restype = C.c_int
        assert lib.os1_matcher_is_reference_build() == 1
        self.L = _Alias(lib, oracle)
        SP.bind_oracle(self)
        KP.bind_oracle(self)
        lib.os1_descriptor_distance_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.os1_radius_by_viewing_cos.argtypes = [C.c_float]
        lib.os1_radius_by_viewing_cos.restype = C.c_float
        lib.os1_compute_three_maxima.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.os1_cv_small.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.POINTER(C.c_double)]
        lib.os1_matcher_constants.argtypes = [C.c_void_p]

    def constants(self):
        v = np.zeros(3, np.int32)
        self.lib.os1_matcher_constants(_p(v))
        return dict(TH_HIGH=int(v[0]), TH_LOW=int(v[1]), HISTO_LENGTH=int(v[2]))

    def hamming_rows(self, rows, ia, ib):
        rows = np.ascontiguousarray(rows, np.uint8)
        return self.lib.os1_descriptor_distance_rows(_p(rows), len(rows), int(ia), int(ib))

    def radius_by_viewing_cos(self, c):
        return float(self.lib.os1_radius_by_viewing_cos(float(c)))

    def compute_three_maxima(self, counts):
        c = np.ascontiguousarray(counts, np.int32)
        ind = np.full(3, -1, np.int32)
        self.lib.os1_compute_three_maxima(_p(c), len(c), _p(ind))
        return [int(v) for v in ind]

    def cv_small(self, op, A, b=None, c=None, s=1.0):
        """the stand-in's arithmetic alone (os1_cv_small of the wrapper)"""
        A = np.ascontiguousarray(A, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        c = None if c is None else np.ascontiguousarray(c, np.float32)
        out, o1 = np.zeros(9, np.float32), C.c_double(0)
        self.lib.os1_cv_small(op, _p(A), None if b is None else _p(b), None if c is None else _p(c), float(s), _p(out), C.byref(o1))
        return o1.value if op in (2, 3) else out[:9 if op in (5, 6, 7) else 3].copy()


def three_maxima_py(counts):
    """ComputeThreeMaxima written out for the literal side (src/ORBmatcher.cc:1554-1595); the oracle keeps its copy in an anonymous
    namespace, reached through every search with an orientation check"""
    m = [0, 0, 0]
    ind = [-1, -1, -1]
    for i, s in enumerate(counts):
        if s > m[0]:
            m, ind = [s, m[0], m[1]], [i, ind[0], ind[1]]
        elif s > m[1]:
            m, ind = [m[0], s, m[1]], [ind[0], i, ind[1]]
        elif s > m[2]:
            m[2], ind[2] = s, i
    if F32(m[1]) < F32(0.1) * F32(m[0]):
        ind[1] = ind[2] = -1
    elif F32(m[2]) < F32(0.1) * F32(m[0]):
        ind[2] = -1
    return ind


class Unmappable(Exception):
    pass


LSF = F32(0.01)     # mfLogScaleFactor of the adapters' camera: level L is predicted from mfMaxDistance = dist * exp(LSF * (L - 0.5))


class Whole:
    """search_by_projection_uv / search_projected of a backend, answered by WHOLE members.  L: an object with the orc_* functions
    (an Oracle's L for the restatements, a RefBackend's L for the library).  Camera: identity pose, fx = fy = 1, cx = cy = 0; the
    MapPoint of query i lies at (u, v, 1): R*p + t = (u*1 + v*0 + 1*0) + 0 is exact, 1/z = 1, fx*x*invz + cx = u."""

    def __init__(self, L):
        self.L = L

    @staticmethod
    def _points(uv, level, sdesc, nsf, need_level):
        n = len(uv)
        pos = np.concatenate([np.asarray(uv, np.float32).reshape(-1, 2), np.ones((n, 1), np.float32)], 1).astype(np.float32)
        dist = SP.U._norm(pos) if n else np.zeros(0, np.float32)
        mx = (dist * np.exp(LSF * (np.asarray(level, np.float32) - F32(0.5))).astype(np.float32)).astype(np.float32)
        if need_level is not None and n:
            got = np.ceil(np.log((mx / dist).astype(np.float32)).astype(np.float32) / LSF)
            ok = (got == np.asarray(level)) & (np.asarray(level) >= 0) & (np.asarray(level) < nsf) & (F32(1.2) * mx >= dist)
            if not ok[need_level].all():
                raise Unmappable('a query level outside the pyramid: the member indexes mvScaleFactors with it')
        nrm = (pos / np.maximum(dist, F32(1e-30))[:, None]).astype(np.float32)
        return dict(pos=pos, normal=nrm, min=np.zeros(n, np.float32), max=mx, desc=np.ascontiguousarray(sdesc, np.uint8).reshape(-1, 32))

    @staticmethod
    def _table(pts, nObs, extra_holder=True):
        """OrcPoints of the query points plus one holder (Observations() = 1) for occupied keypoints; returns (struct, arrays)"""
        ext = lambda a, v: np.ascontiguousarray(np.concatenate([a, np.asarray(v, a.dtype).reshape((1,) + a.shape[1:])]))
        a = dict(pos=ext(pts['pos'], np.zeros(3)), normal=ext(pts['normal'], [0, 0, 1]), min=ext(pts['min'], [0]), max=ext(pts['max'], [0]),
                 desc=ext(pts['desc'], np.zeros(32)), bad=np.zeros(len(nObs) + 1, np.uint8), nObs=ext(np.asarray(nObs, np.int32), [1]),
                 idx=np.full(len(nObs) + 1, -1, np.int32))
        P = OrcPoints(len(a['bad']), _p(a['pos']), _p(a['normal']), _p(a['min']), _p(a['max']), _p(a['desc']), _p(a['bad']), _p(a['nObs']),
                      _p(a['idx']))
        return P, a

    @staticmethod
    def _view(kps, desc, bounds, sf, is2=None):
        keep = [np.ascontiguousarray(kps, KP_DTYPE), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(sf, np.float32),
                np.ascontiguousarray(is2 if is2 is not None else np.ones(len(sf)), np.float32)]
        V = OrcView(_p(keep[0]), _p(keep[1]), len(keep[0]), (C.c_float * 4)(*[float(b) for b in bounds]), 1.0, 1.0, 0.0, 0.0, _p(keep[2]),
                    _p(keep[3]), len(keep[2]), float(LSF))
        return V, keep

    @staticmethod
    def _inside(uv, valid, bounds, closed):
        b = [F32(v) for v in bounds]
        u, v = uv[:, 0], uv[:, 1]
        ok = (u >= b[0]) & (u <= b[1]) & (v >= b[2]) & (v <= b[3]) if closed else (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        if not ok[valid].all():
            raise Unmappable('a query outside the image bounds: the member rejects it before it searches')

    def search_by_projection_uv(self, kps, desc, bounds, sf, occ, src_uv, src_level, src_angle, src_flags, src_valid, src_desc, th, max_dist,
                                skip_any, check_ori):
        uv = np.ascontiguousarray(src_uv, np.float32).reshape(-1, 2)
        n, nk = len(uv), len(kps)
        valid = np.asarray(src_valid) != 0
        level = np.asarray(src_level, np.int32)
        observed = (np.asarray(src_flags) & 8) != 0
        self._inside(uv, valid, bounds, True)
        if ((level[valid] < 0) | (level[valid] >= len(sf))).any():
            raise Unmappable('a query level outside the pyramid: the member indexes mvScaleFactors with it')
        as_keyframe = bool(skip_any) or (observed[valid].all() and max_dist != 100)
        if not as_keyframe and max_dist != 100:
            raise Unmappable('max_dist != TH_HIGH with unobserved sources: neither member has that combination')
        if as_keyframe and max_dist >= 256:
            # bestDist starts at 256 with bestIdx2 = -1 (src/ORBmatcher.cc:1488-1489) and `bestDist<=ORBdist` (:1508) then holds with no
            # candidate at all: the member writes mvpMapPoints[-1].  No caller of the reference passes more than TH_HIGH.
            raise Unmappable('max_dist >= 256: the member writes mvpMapPoints[-1] when no candidate is below 256')
        pts = self._points(uv, level, src_desc, len(sf), valid if as_keyframe else None)
        P, arr = self._table(pts, observed.astype(np.int32))
        V, keep = self._view(kps, desc, bounds, sf)
        T = np.eye(4, dtype=np.float32)
        cur = np.where(np.asarray(occ) != 0, n, -1).astype(np.int32)
        src_mp = np.where(valid, np.arange(n), -1).astype(np.int32)
        src_k = np.zeros(n, KP_DTYPE)
        src_k['octave'], src_k['angle'] = level, np.asarray(src_angle, np.float32)
        if as_keyframe:
            already = np.zeros(n + 1, np.uint8)
            nm = self.L.orc_sbp_keyframe(C.byref(V), _p(T), _p(src_k), n, _p(src_mp), _p(already), C.byref(P), _p(cur), float(th), int(max_dist),
                                         int(check_ori))
        else:
            outl = np.zeros(n, np.uint8)
            nm = self.L.orc_sbp_frame(C.byref(V), _p(T), _p(src_k), _p(src_k), n, _p(src_mp), _p(outl), C.byref(P), _p(cur), float(th), int(check_ori))
        return nm, np.where(cur == n, -1, cur)[:nk]

    def search_projected(self, kps, desc, bounds, uv, radius, level, valid, sdesc, kp_skip=None, claim=False, inv_sigma2=None, chi2=5.99,
                         max_dist=50):
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        n, nk = len(uv), len(kps)
        valid = np.asarray(valid) != 0
        level = np.asarray(level, np.int32)
        radius = np.asarray(radius, np.float32)
        desc = np.ascontiguousarray(desc, np.uint8)
        sdesc = np.ascontiguousarray(sdesc, np.uint8).reshape(-1, 32)
        if n == 0 or nk == 0:
            raise Unmappable('an empty side')
        self._inside(uv, valid, bounds, False)
        d = np.unpackbits(sdesc[:, None, :] ^ desc[None, :, :], axis=2).sum(2)
        lo, hi = min(max_dist, 50), max(max_dist, 50)
        if ((d[valid] > lo) & (d[valid] <= hi)).any():
            raise Unmappable('max_dist != TH_LOW decides a candidate: SearchBySim3 alone accepts up to TH_HIGH, and it searches both ways')
        if ((level[valid] < 0)).any():
            raise Unmappable('a query level outside the pyramid: the member indexes mvScaleFactors with it')
        nlev = int(max(level[valid].max() + 1 if valid.any() else 1, kps['octave'].max() + 1, 1))
        sf = np.ones(nlev, np.float32)
        seen = {}
        for i in np.flatnonzero(valid):
            if seen.setdefault(int(level[i]), radius[i]) != radius[i]:
                raise Unmappable('two radii on one level: the member takes th * mvScaleFactors[level]')
            sf[level[i]] = radius[i]
        pts = self._points(uv, np.where(valid, level, 0), sdesc, nlev, valid)
        P, arr = self._table(pts, np.zeros(n, np.int32))
        arr['bad'][:n] = ~valid                                # an invalid query: a bad MapPoint, skipped by every member
        V, keep = self._view(kps, desc, bounds, sf, inv_sigma2)
        T = np.eye(4, dtype=np.float32)
        pts_id = np.arange(n, dtype=np.int32)
        slot = np.full(nk, -1, np.int32)
        if kp_skip is not None or claim:
            if not claim:
                raise Unmappable('keypoints skipped but not claimed: SearchByProjection(KeyFrame, Scw) always claims')
            if inv_sigma2 is not None:
                raise Unmappable('claim and gate together: no member has both')
            if kp_skip is not None:
                slot[np.asarray(kp_skip) != 0] = n
            nm = self.L.orc_sbp_scw(C.byref(V), _p(T), _p(pts_id), n, C.byref(P), _p(slot), 1)
            bi = np.full(n, -1, np.int32)
            for k in np.flatnonzero((slot >= 0) & (slot < n)):
                bi[slot[k]] = k
        elif inv_sigma2 is not None:
            if chi2 != 5.99:
                raise Unmappable('a gate other than 5.99')
            nm = self.L.orc_fuse(C.byref(V), _p(T), _p(pts_id), n, C.byref(P), _p(slot), 1.0)
            if arr['bad'][:n][valid].any():
                raise Unmappable('two queries end on one keypoint: Fuse replaces one MapPoint by the other')
            bi = arr['idx'][:n].copy()
        else:
            rep = np.full(n, -1, np.int32)
            nm = self.L.orc_fuse_scw(C.byref(V), _p(T), _p(pts_id), n, C.byref(P), _p(slot), 1.0, _p(rep))
            bi = arr['idx'][:n].copy()
            hit = rep >= 0
            bi[hit] = arr['idx'][rep[hit]]
        bd = np.array([d[i, bi[i]] if bi[i] >= 0 else -1 for i in range(n)], np.int32)
        return nm, bi, bd


# ---- the scene registry -------------------------------------------------------------------------------------------------------
def _norm_uv(res):
    """(n, assigned) with the array form's 'pruned' mark (-2) read as what the member leaves: NULL"""
    n, a = res
    return dict(n=np.int64(n), a=np.where(np.asarray(a, np.int64) == -2, -1, np.asarray(a, np.int64)))


def boundary_result(scene, res):
    """run()'s tuple as a dict of arrays"""
    if isinstance(scene, BB.Scene):
        if scene.kind == 'tri':
            return dict(n=np.int64(res[0]), pairs=np.asarray(res[1], np.int64).reshape(-1, 2))
        return dict(n=np.int64(res[0]), m=np.asarray(res[1], np.int64))
    if scene.kind in ('mp', 'init'):
        return dict(n=np.int64(res[0]), a=np.asarray(res[1], np.int64))
    if scene.kind == 'uv':
        return _norm_uv(res)
    return dict(n=np.int64(res[0]), bi=np.asarray(res[1], np.int64), bd=np.asarray(res[2], np.int64))


def run_boundary(scene, be, whole=None):
    """one boundary scene on a backend: members directly, 'uv' / 'proj' through Whole (whole = the Whole of that backend)"""
    if isinstance(scene, BB.Scene):
        return boundary_result(scene, BB.run(scene, be))
    if scene.kind in ('uv', 'proj'):
        return boundary_result(scene, SB.run(scene, whole))
    res = SB.run(scene, be)
    if scene.kind == 'init':     # ... and the vbPrevMatched the call updated
        i = scene.inp
        n, m12, prev = be.search_for_initialization(i['kps1'], i['desc1'], i['kps2'], i['desc2'], i['bounds'], i['prev'], i['window'], i['ratio'], i['ori'])
        out = boundary_result(scene, res)
        out['prev'] = np.asarray(prev, np.float32)
        return out
    return boundary_result(scene, res)


BOUNDARY = [s for s in SB.SCENES if s.kind != 'win'] + list(BB.SCENES)     # ('win' is GetFeaturesInArea alone: no member of ORBmatcher)


def seeded_frames(W=640, H=480, nfeat=400):
    return SP.frames(W, H, nfeat)


_FR = {}


def frames():
    if 'f' not in _FR:
        _FR['f'] = seeded_frames()
    return _FR['f']


def sp_scene(mode, seed, edges):
    kA, dA, kB, dB, sf = frames()
    S = SP.scene(kA, dA, kB, sf, 640, 480, seed)
    if edges:
        # the edge MapPoints under the identity camera (behind it, on and beyond each bound, z = +-0); LAST_FRAME takes the level from
        # the keypoint.  KEYFRAME would predict levels outside the pyramid for some and index mvScaleFactors with them.
        S, _ = SP.edge_sources(S, sf)
        S = dict(S, cam=S['camA'])
    return S


def run_sp(be, mode, seed, th, max_dist, edges=False):
    """source_projection_util.oracle_search with the table as long as the scene's (the edge MapPoints are rows past the sources'):
    an occupied keypoint holds one extra MapPoint with Observations() = 1"""
    kA, dA, kB, dB, sf = frames()
    S = sp_scene(mode, seed, edges)
    cam, tab, st, rows, n = S['cam'], S['tab'], S['st'], S['rows'], S['n']
    M = len(tab['pos'])
    kA, kB = np.ascontiguousarray(kA, KP_DTYPE), np.ascontiguousarray(kB, KP_DTYPE)
    dB, sf = np.ascontiguousarray(dB, np.uint8), np.ascontiguousarray(sf, np.float32)
    is2 = np.ascontiguousarray(1.0 / (sf * sf), np.float32)
    ext = lambda a, v: np.ascontiguousarray(np.concatenate([a, np.asarray(v, a.dtype).reshape((1,) + a.shape[1:])]))
    pos, nrm = ext(tab['pos'], np.zeros(3)), ext(tab['normal'], np.zeros(3))
    mn, mx, desc = ext(tab['min'], [0]), ext(tab['max'], [0]), ext(tab['desc'], np.zeros(32))
    bad, nObs, already = ext(st['bad'], [0]), ext(st['nObs'], [1]), ext(st['already'], [0])
    assert len(bad) == len(nObs) == len(already) == M + 1
    idx = np.full(M + 1, -1, np.int32)
    P = OrcPoints(M + 1, _p(pos), _p(nrm), _p(mn), _p(mx), _p(desc), _p(bad), _p(nObs), _p(idx))
    V = OrcView(_p(kB), _p(dB), len(kB), (C.c_float * 4)(*S['bounds']), cam['fx'], cam['fy'], cam['cx'], cam['cy'], _p(sf), _p(is2), len(sf),
                cam['lsf'])
    T = SP.tcw16(cam)
    cur = np.where(st['occ'] != 0, M, -1).astype(np.int32)
    before = cur.copy()
    src_mp = np.where(st['absent'] != 0, -1, rows).astype(np.int32)
    if mode == SP.LAST_FRAME:
        outlier = (np.arange(n) % 17 == 3).astype(np.uint8)      # mvbOutlier: a few sources are outliers of the last frame
        nm = be.L.orc_sbp_frame(C.byref(V), _p(T), _p(kA), _p(kA), n, _p(src_mp), _p(outlier), C.byref(P), _p(cur), th, 1)
    else:
        nm = be.L.orc_sbp_keyframe(C.byref(V), _p(T), _p(kA), n, _p(src_mp), _p(already), C.byref(P), _p(cur), th, int(max_dist), 1)
    return dict(n=np.int64(nm), cur=cur.astype(np.int64), before=before.astype(np.int64))


def kp_scene(seed):
    kA, dA, kB, dB, sf = frames()
    return KP.scene(kA, dA, kB, dB, sf, 640, 480, seed)


def run_kp(be, fn, sc, case, views=None):
    kA, dA, kB, dB, sf = views or frames()
    out = KP.run_oracle(be, fn, case, sc, kA, dA, kB, dB, sf)
    return {k: np.asarray(v).astype(np.int64) for k, v in out.items()}


def mp_seeded(seed=5, n_mp=500):
    """SearchByProjection(Frame, MapPoints, th): 500 projected MapPoints near frame B's keypoints, with absent, bad, candidate and
    unobserved points and occupied keypoints"""
    kA, dA, kB, dB, sf = frames()
    rng = np.random.default_rng(seed)
    src = rng.integers(0, len(kB), n_mp)
    xy = np.stack([kB['x'][src] + rng.normal(0, 1.5, n_mp), kB['y'][src] + rng.normal(0, 1.5, n_mp)], 1).astype(np.float32)
    level = np.clip(kB['octave'][src] + rng.integers(0, 2, n_mp), 0, len(sf) - 1).astype(np.int32)
    viewcos = rng.choice(np.array([0.5, 0.9979, 0.998, 0.9981, 1.0], np.float32), n_mp)
    flags = (1 * (rng.random(n_mp) < 0.9) + 2 * (rng.random(n_mp) < 0.03) + 4 * (rng.random(n_mp) < 0.05) + 8 * (rng.random(n_mp) < 0.85)).astype(np.uint8)
    qdesc = dB[src].copy()
    for i in range(n_mp):
        for b in rng.integers(0, 256, rng.integers(0, 40)):
            qdesc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    occ = (rng.random(len(kB)) < 0.1).astype(np.uint8)
    return dict(kps=kB, desc=dB, bounds=(0.0, 640.0, 0.0, 480.0), sf=sf, occ=occ, xy=xy, level=level, viewcos=viewcos, flags=flags, qdesc=qdesc,
                th=3.0, ratio=0.8)


def init_seeded(seed=9, n=300):
    """SearchForInitialization on ~300 level-0 keypoints on a 6-pixel lattice whose descriptors come from a palette of eight rows at
    pairwise distances 1..14: every window holds many candidates at equal and near-equal distances (ties of best, of second best, and
    keypoints of frame 2 claimed twice)"""
    rng = np.random.default_rng(seed)
    pal = SB.rows([0, 2, 4, 6, 8, 10, 12, 14])
    g = rng.permutation(24 * 18)[:n]
    x, y = 200.0 + 6.0 * (g % 24), 150.0 + 6.0 * (g // 24)
    k1 = SB.make_kps([(x[i], y[i], 0 if rng.random() < 0.95 else 1, float(rng.choice([0.0, 10.0, 40.0, 200.0]))) for i in range(n)])
    k2 = SB.make_kps([(x[i] + 1.0, y[i] - 1.0, 0, float(rng.choice([0.0, 12.0, 200.0]))) for i in rng.permutation(n)])
    return dict(kps1=k1, desc1=pal[rng.integers(0, 8, n)], kps2=k2, desc2=pal[rng.integers(0, 8, n)], bounds=(0.0, 640.0, 0.0, 480.0),
                prev=np.stack([k1['x'], k1['y']], 1).astype(np.float32), window=10, ratio=0.9, ori=True)


# ---- crafted keyframe-side scenes: edge MapPoints and SearchBySim3 on TH_HIGH ----------------------------------------------------
E_BOUNDS = (0.0, 640.0, 0.0, 480.0)
E_LSF = F32(1.0)     # mfLogScaleFactor of the crafted keyframes: with it every edge point that reaches PredictScale predicts a level
                     # inside the pyramid (a ratio just below 1 gives ceil(-0.18) = 0, the largest ratio 33 gives 4), so the members
                     # index mvScaleFactors in range -- under log(1.2) the same points predict -1 and 10
E_CAM = dict(Rcw=np.eye(3, dtype=np.float32), tcw=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), fx=F32(320.0), fy=F32(240.0),
             cx=F32(320.0), cy=F32(240.0), lsf=E_LSF)
E_SF = np.cumprod(np.array([1.0] + [1.2] * 7, np.float32)).astype(np.float32)
E_K = np.array([E_CAM['fx'], E_CAM['fy'], E_CAM['cx'], E_CAM['cy'], E_LSF], np.float32)
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def _sim3_dirs(case, K):
    """the two GPU calls of a SearchBySim3 case at s12 = 1, R12 = I, t12 = 0 between two identity keyframes (what
    keyframe_projection_util.make_case builds for its scene)"""
    mp1, mp2, m12, idx, bad = case['mp1'], case['mp2'], case['m12'], case['idx'], case['bad']
    already1 = m12 >= 0
    already2 = np.zeros(len(mp2), bool)
    hit = idx[m12[already1]]
    already2[hit[(hit >= 0) & (hit < len(mp2))]] = True
    dirs = []
    for mp, already, to in ((mp1, already1, 'B'), (mp2, already2, 'A')):
        fl = np.zeros(len(mp), np.uint8)
        fl[(mp < 0) | already] = KP.MP_SKIP
        free = (mp >= 0) & (fl == 0)
        fl[free] |= np.where(bad[mp[free]] != 0, KP.MP_BAD, 0).astype(np.uint8)
        dirs.append(dict(pr=KP.projection(I3, Z3, K, sR=I3, t2=Z3, invz_double=True, angle=False, dist_point=True),
                         rows=np.where(mp >= 0, mp, 1 << 30).astype(np.int32), flags=fl, to=to, kp_skip=None, claim=False, chi2=False,
                         max_dist=KP.TH_HIGH))
    return dirs


def _sim3_case(mp1, mp2, m12, idx, bad, nObs, th):
    case = dict(fn=KP.SIM3, th=th, bad=bad, nObs=nObs, mp1=np.asarray(mp1, np.int32), mp2=np.asarray(mp2, np.int32), idx=idx,
                m12=np.asarray(m12, np.int32), s12=F32(1.0), R12=I3.copy(), t12=Z3.copy(), T1=KP.pose16(I3, Z3), T2=KP.pose16(I3, Z3))
    case['dirs'] = _sim3_dirs(case, E_K)
    return case


def _crafted_sc(tab):
    return dict(tab=tab, M=len(tab['pos']), cam=E_CAM, bounds=E_BOUNDS, K=E_K)


def edge_scene():
    """keyframe_projection_util.edge_points under the identity pose, as a scene the four keyframe-side members search.  Edge point i
    (z = +0 / -0 / slightly negative / tiny, u and v on each bound, dist3D on and one float past both invariance bounds, the viewing
    cosine on and one float below 0.5, one point per level, the invz probe) is table row i and again row E + i.  The keyframe holds two
    keypoints per edge point beside its projection: 2i + 1 (octave level - 1, the descriptor of row i) and 2i (octave level, the
    descriptor of row E + i); all descriptors are random, so a point that passes every test finds exactly its own keypoint at distance 0
    and one that is rejected leaves it empty: each edge shows in the return value and the bookkeeping.  Rows 2E.. are holders."""
    tab, names = KP.edge_points(E_BOUNDS, E_K, E_SF)
    E = len(tab['pos'])
    rng = np.random.default_rng(77)
    pos = tab['pos']
    dist = SP.U._norm(pos)
    with np.errstate(all='ignore'):
        lvl = np.ceil(np.log((tab['max'] / dist).astype(np.float32)).astype(np.float32) / E_LSF)
        u = (E_CAM['fx'] * (pos[:, 0] / pos[:, 2]) + E_CAM['cx']).astype(np.float32)
        v = (E_CAM['fy'] * (pos[:, 1] / pos[:, 2]) + E_CAM['cy']).astype(np.float32)
    reach = (pos[:, 2] > 0) & (F32(0.8) * tab['min'] <= dist) & (F32(1.2) * tab['max'] >= dist)        # reaches PredictScale
    assert reach.sum() >= 16 and ((lvl[reach] >= 0) & (lvl[reach] < len(E_SF))).all(), 'an edge point predicts a level outside the pyramid'
    lvl = np.where(reach, lvl, 0).astype(np.int32)
    ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 2000) & (np.abs(v) < 2000)
    u, v = np.where(ok, u, 100.0 + 3 * np.arange(E)), np.where(ok, v, 100.0)
    pts = []
    for i in range(E):
        pts += [(u[i] + 0.5, v[i], int(lvl[i])), (u[i] - 0.5, v[i] + 0.5, max(int(lvl[i]) - 1, 0))]
    kps = SB.make_kps(pts)
    dk = rng.integers(0, 256, (2 * E, 32), dtype=np.uint8)
    H = 6
    hold = {k: np.concatenate([tab[k], tab[k], tab[k][:H]]) for k in tab}
    hold['desc'] = np.concatenate([dk[1::2], dk[0::2], rng.integers(0, 256, (H, 32), dtype=np.uint8)])
    return dict(sc=_crafted_sc(hold), E=E, H=H, names=names, kps=kps, desc=dk, views=(kps, dk, kps, dk, E_SF))


def edge_case(fn, th):
    """one member's call on edge_scene(): every edge row and its twin as candidates, a few bad, six keypoints already holding a holder"""
    S = edge_scene()
    E, H, M = S['E'], S['H'], S['sc']['M']
    rng = np.random.default_rng(78 + KP.FUNCS.index(fn))
    bad = np.zeros(M, np.uint8)
    bad[[S['names']['level_3'], E + S['names']['level_5']]] = 1
    nObs = rng.integers(0, 6, M).astype(np.int32)
    nk = len(S['kps'])
    if fn == KP.SIM3:
        mp1, mp2 = np.full(nk, -1, np.int32), np.full(nk, -1, np.int32)
        mp1[0::2] = np.arange(E)             # keyframe 1 observes row i at keypoint 2i; in keyframe 2 it finds keypoint 2i + 1 ...
        mp2[1::2] = E + np.arange(E)         # ... which observes row E + i, whose descriptor is keypoint 2i's in keyframe 1: they agree
        idx = np.full(M, -1, np.int32)
        idx[mp2[1::2]] = np.arange(1, nk, 2)
        m12 = np.full(nk, -1, np.int32)
        m12[2 * S['names']['level_1']] = E + S['names']['level_1']          # matched before the call: both sides are skipped
        return S, _sim3_case(mp1, mp2, m12, idx, bad, nObs, th)
    slot, idx = np.full(nk, -1, np.int32), np.full(M, -1, np.int32)
    held = [2 * S['names'][n] + 1 for n in ('level_0', 'level_2', 'u_minX', 'dist_on_max', 'dot_on_half', 'invz_probe')]
    slot[held] = 2 * E + np.arange(H)
    idx[2 * E + np.arange(H)] = held
    nObs[2 * E + np.arange(H)] = [1, 5, 1, 5, 3, 2]
    points = np.concatenate([rng.permutation(2 * E), [2 * E, 2 * E + 1]]).astype(np.int32)
    case = dict(fn=fn, th=th, bad=bad, nObs=nObs, points=points, slot=slot, idx=idx)
    fl = np.zeros(len(points), np.uint8)
    K = E_K
    if fn == KP.FUSE:
        points[[3, 11]] = -1
        has = points >= 0
        fl[~has] = KP.MP_SKIP
        fl[has] |= np.where(bad[points[has]] != 0, KP.MP_BAD, 0).astype(np.uint8)
        fl[has] |= np.where((idx[points[has]] >= 0) & (bad[points[has]] == 0), KP.MP_SKIP, 0).astype(np.uint8)
        d = dict(pr=KP.projection(I3, Z3, K, Ow=Z3), kp_skip=None, claim=False, chi2=True)
    else:
        fl[bad[points] != 0] = KP.MP_BAD
        found = np.zeros(M, bool)
        inslot = slot[slot >= 0]
        if fn == KP.SBP_SCW:
            found[inslot] = True
            d = dict(pr=KP.projection(I3, Z3, K, Ow=Z3), kp_skip=(slot >= 0).astype(np.uint8), claim=True, chi2=False)
        else:
            found[inslot[bad[inslot] == 0]] = True
            d = dict(pr=KP.projection(I3, Z3, K, Ow=Z3, invz_double=True), kp_skip=None, claim=False, chi2=False)
        fl[(fl == 0) & found[points]] = KP.MP_SKIP
    case['T'] = KP.pose16(I3, Z3)
    d.update(rows=np.where(points >= 0, points, 1 << 30).astype(np.int32), flags=fl, to='B', max_dist=KP.TH_LOW)
    case['dirs'] = [d]
    return S, case


EDGE_CASES = [(KP.SBP_SCW, 4), (KP.FUSE, 4.0), (KP.FUSE_SCW, 4.0), (KP.SIM3, 4.0)]

# SearchBySim3 on `bestDist<=TH_HIGH` (src/ORBmatcher.cc:1185 for keyframe 1 -> 2, :1265 for 2 -> 1): (d1, d2, found).  Keyframe 1 holds
# one keypoint with row(0) and observes MapPoint 0, whose descriptor is row(d1); keyframe 2 holds one keypoint with row(0) and
# observes MapPoint 1 with row(d2).  Both points lie at (0, 0, 10) before two identity cameras, s12 = 1: each direction has exactly one
# candidate, at distance d1 resp. d2, and the match counts only if both directions accept.
SIM3_TH_HIGH = [(100, 0, 1), (101, 0, 0), (0, 100, 1), (0, 101, 0), (100, 100, 1), (101, 101, 0)]


def sim3_th_high_case(d1, d2):
    tab = dict(pos=np.array([[0, 0, 10], [0, 0, 10]], np.float32), normal=np.array([[0, 0, 1], [0, 0, 1]], np.float32),
               min=np.array([1, 1], np.float32), max=np.array([9, 9], np.float32), desc=SB.rows([d1, d2]))
    k1 = SB.make_kps([(E_CAM['cx'] + 0.5, E_CAM['cy'], 0)])
    k2 = SB.make_kps([(E_CAM['cx'] - 0.5, E_CAM['cy'] + 0.5, 0)])
    d0 = SB.rows([0])
    idx = np.array([-1, 0], np.int32)
    case = _sim3_case([0], [1], [-1], idx, np.zeros(2, np.uint8), np.ones(2, np.int32), 4.0)
    return dict(sc=_crafted_sc(tab), views=(k1, d0, k2, d0, E_SF)), case


SP_CASES = [(SP.LAST_FRAME, 2151, 15.0, 100, False), (SP.LAST_FRAME, 2152, 7.0, 100, False), (SP.LAST_FRAME, 2151, 15.0, 100, True),
            (SP.KEYFRAME, 3101, 10.0, 100, False), (SP.KEYFRAME, 3102, 3.0, 64, False)]
KP_CASES = [(fn, seed, th) for fn in KP.FUNCS for seed, th in zip((41, 42), KP.CASES[fn])]      # two poses (seeds), both th of the caller


def _bits(v):
    return np.frombuffer(np.asarray(v, np.float32).tobytes(), np.uint32).astype(np.int64)


def dd_pairs():
    """DescriptorDistance inputs: rows at known distances (row(a), row(b): |a - b|), all-zero against all-one, random rows"""
    rng = np.random.default_rng(3)
    tab = np.stack([SB.row(n) for n in range(257)])
    known = [(0, 0), (0, 1), (0, 255), (0, 256), (17, 200), (256, 1), (128, 129)]
    rnd = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    rnd[0], rnd[1] = 0, 255
    return tab, known, rnd


def histogram_cases():
    rng = np.random.default_rng(4)
    cases = [c + [0] * (30 - len(c)) for _, c, _ in SB.HIST_COUNTS] + [[0] * 30, [1] * 30, [0] * 29 + [5]]
    return cases + [[int(v) for v in rng.integers(0, 12, 30)] for _ in range(40)]


def viewcos_cases():
    c0 = F32(0.998)
    return [c0, np.nextafter(c0, F32(0)), np.nextafter(c0, F32(2)), F32(1.0), F32(0.5), F32(-1.0)]


def arith_inputs():
    """(A, b, c) for the stand-in's arithmetic: random, and cancelling (A*b lands near -c, the rows of A nearly orthogonal to b)"""
    rng = np.random.default_rng(8)
    out = []
    for _ in range(60):
        out.append((rng.normal(size=(3, 3)), rng.normal(size=3) * 10.0 ** rng.integers(-3, 4), rng.normal(size=3)))
    for _ in range(60):
        b = rng.normal(size=3)
        A = rng.normal(size=(3, 3))
        A -= np.outer(A @ b, b) / (b @ b) * (1 - 1e-6)
        c = -(A.astype(np.float32) @ b.astype(np.float32)) * (1 + rng.normal() * 1e-6)
        out.append((A * 1e3, b, c * 1e3))
    out.append((np.eye(3), np.array([1e30, -1e30, 1.0]), np.zeros(3)))
    out.append((np.eye(3), np.zeros(3), -np.zeros(3)))
    return [(np.float32(A), np.float32(b), np.float32(c)) for A, b, c in out]


def dd_run(be, whole):
    tab, known, rnd = dd_pairs()
    rows = getattr(be, 'hamming_rows', lambda t, a, b: be.hamming(t[a], t[b]))       # DescriptorDistance(D.row(a), D.row(b)) on the library
    return dict(known=np.array([be.hamming(tab[a], tab[b]) for a, b in known], np.int64), known_rows=np.array([rows(tab, a, b) for a, b in known], np.int64),
                rnd=np.array([be.hamming(rnd[i], rnd[i + 1]) for i in range(0, 200, 2)], np.int64),
                rnd_rows=np.array([rows(rnd, i, i + 1) for i in range(0, 200, 2)], np.int64))


def helpers_run(be, whole):
    """ComputeThreeMaxima and RadiusByViewingCos: the library's own, else (the oracle keeps its copies in an anonymous namespace) the
    statements of them written out here"""
    tm = getattr(be, 'compute_three_maxima', three_maxima_py)
    rv = getattr(be, 'radius_by_viewing_cos', lambda c: 2.5 if float(F32(c)) > 0.998 else 4.0)
    out = dict(maxima=np.array([tm(c) for c in histogram_cases()], np.int64), radius=_bits([rv(c) for c in viewcos_cases()]))
    if hasattr(be, 'constants'):
        k = be.constants()
        assert k == dict(TH_HIGH=100, TH_LOW=50, HISTO_LENGTH=30), k
    return out


def arith_run(be, whole):
    """every operator form of the cv::Mat stand-in (os1_cv_small of the wrapper) or, on the oracle, the same form through orc_cv_small
    and plain float arithmetic: A*b+c, A*b, -A*b, -A.t()*b, norm, dot, s*A, (1.0/s)*A.t(), A/s, b-c, KeyFrame::SetPose's -Rwc*tcw"""
    lib = hasattr(be, 'lib')
    v, d = [], []
    for A, b, c in arith_inputs():
        s = F32(abs(float(b[0])) + 0.37)
        inv = F32(1.0 / float(s))
        if lib:
            v += [be.cv_small(0, A, b, c), be.cv_small(0, A, b), be.cv_small(4, A, b), be.cv_small(1, A, b), be.cv_small(5, A, s=s),
                  be.cv_small(6, A, s=s), be.cv_small(7, A, s=s), be.cv_small(8, A, b, c), be.cv_small(9, A, b)]
            d += [be.cv_small(2, A, b), be.cv_small(3, A, b)]
        else:
            v += [be.cv_small('gemm', A, b, 1.0, c, 1.0), be.cv_small('gemm', A, b, 1.0), be.cv_small('gemm', A, b, -1.0),
                  be.cv_small('gemmT', A, b, -1.0), A.ravel() * s, A.T.ravel() * inv, A.ravel() * inv, b - c,
                  be.cv_small('gemm', np.ascontiguousarray(A.T), b, -1.0)]
            d += [be.cv_small('norm', A, b), be.cv_small('dot', A, b)]
    return dict(f32=_bits(np.concatenate([np.asarray(x, np.float32).ravel() for x in v])),
                f64=np.frombuffer(np.asarray(d, np.float64).tobytes(), np.int64).copy())


def registry(kp_L=None):
    """[(key, runner)]; runner(be, whole) -> dict of arrays.  kp_L: the restatement library keyframe_projection_util.make_case asks for
    (KP.build_ref), needed to RUN the 'kp:' scenes, not to list the keys."""
    reg = [('dd', dd_run), ('helpers', helpers_run), ('arith', arith_run)]
    for s in BOUNDARY:
        reg.append(('b:' + s.name, lambda be, whole, s=s: run_boundary(s, be, whole)))
    for mode, seed, th, md, edges in SP_CASES:
        reg.append(('sp:%d:%d:%g:%d:%d' % (mode, seed, th, md, edges), lambda be, whole, a=(mode, seed, th, md, edges): run_sp(be, *a)))
    for fn, seed, th in KP_CASES:
        def runner(be, whole, fn=fn, seed=seed, th=th):
            sc = kp_scene(seed)
            return run_kp(be, fn, sc, KP.make_case(kp_L, fn, sc, th))
        reg.append(('kp:%s:%d:%g' % (fn, seed, th), runner))

    for fn, th in EDGE_CASES:
        def edge_runner(be, whole, fn=fn, th=th):
            S, case = edge_case(fn, th)
            return run_kp(be, fn, S['sc'], case, S['views'])
        reg.append(('edge:%s' % fn, edge_runner))
    for d1, d2, found in SIM3_TH_HIGH:
        def th_runner(be, whole, d1=d1, d2=d2):
            S, case = sim3_th_high_case(d1, d2)
            return run_kp(be, KP.SIM3, S['sc'], case, S['views'])
        reg.append(('sim3_th_high:%d:%d' % (d1, d2), th_runner))

    def mp_run(be, whole):
        i = mp_seeded()
        n, a = be.search_by_projection(i['kps'], i['desc'], i['bounds'], i['sf'], i['occ'], i['xy'], i['level'], i['viewcos'], i['flags'], i['qdesc'],
                                       i['th'], i['ratio'])
        return dict(n=np.int64(n), a=np.asarray(a, np.int64))

    def init_run(be, whole):
        i = init_seeded()
        n, m, prev = be.search_for_initialization(i['kps1'], i['desc1'], i['kps2'], i['desc2'], i['bounds'], i['prev'], i['window'], i['ratio'], i['ori'])
        return dict(n=np.int64(n), a=np.asarray(m, np.int64), prev=np.asarray(prev, np.float32))
    reg.append(('mp:seeded', mp_run))
    reg.append(('init:seeded', init_run))
    return reg


# ---- the golden ---------------------------------------------------------------------------------------------------------------
_G = {}
UNMAPPED = 'unmapped_keys'     # the array-form scenes no member expresses, recorded so that a key MISSING from the golden is told apart


def golden():
    """{key: {field: array}} of tests/golden/os1_matcher_outputs.npz, or None"""
    if 'g' not in _G:
        _G['g'] = None
        if os.path.exists(GOLDEN):
            z = np.load(GOLDEN)
            g = {}
            for name in z.files:
                if name == UNMAPPED:
                    continue
                key, field = name.rsplit('|', 1)
                g.setdefault(key, {})[field] = z[name]
            _G['g'] = g
    return _G['g']


def golden_unmapped():
    z = np.load(GOLDEN)
    return set(str(k) for k in z[UNMAPPED])


def same(a, b):
    """every field equal: integers, index arrays and float bits"""
    if a is None or b is None or set(a) != set(b):
        return False
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).dtype.kind == np.asarray(b[k]).dtype.kind
               and np.asarray(a[k]).astype(np.asarray(b[k]).dtype).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def diff(a, b):
    if a is None or b is None:
        return 'one side is missing'
    return '; '.join('%s: %s != %s' % (k, np.asarray(a.get(k)).ravel()[:12], np.asarray(b.get(k)).ravel()[:12]) for k in sorted(set(a) | set(b))
                     if k not in a or k not in b or not same({k: a[k]}, {k: b[k]}))
