"""Shared by tests/test_keyframe_projection.py and tests/test_gpu_keyframe_projection.py: the reference restatement of the
keyframe projection (tests/cpp/project_keyframe_ref.cpp, built here with g++ -ffp-contract=off), ctypes bindings of the oracle's
whole-function restatements orc_sbp_scw / orc_fuse / orc_fuse_scw / orc_search_by_sim3 (oracle/orb_oracle_pose.h), the scenes
both files search, and each function's bookkeeping replay (what orb_shim.hpp does after the search).

A scene: frames A and B = A shifted by (3, -2) px.  Keyframe B has the moved camera; the MapPoints are triangulated from A's
keypoints (identity camera) at varied depths, so that B sees each near its own copy of that keypoint.  Added to them: twins
(another MapPoint at the same place: two candidates for one keypoint), points behind B's camera or beside its image, points whose normal looks
away, depth ranges that reject the point on either bound, and holders (the MapPoints that sit in keyframe B's slots).  For
SearchBySim3 keyframe A (identity camera) observes the A points and keyframe B a second set triangulated from B's keypoints.
MapPoint ids are rows of the device table."""
import ctypes as C
import os
import subprocess

import numpy as np

import local_map_util as U
import source_projection_util as SP
from oracle.pyoracle import KP_DTYPE

ROOT = SP.ROOT
REF_SRC = os.path.join(ROOT, 'tests', 'cpp', 'project_keyframe_ref.cpp')
MP_BAD, MP_SKIP = 2, 16
TH_LOW, TH_HIGH = 50, 100
SBP_SCW, FUSE, FUSE_SCW, SIM3 = 'sbp_scw', 'fuse', 'fuse_scw', 'sim3'
FUNCS = (SBP_SCW, FUSE, FUSE_SCW, SIM3)
# th of the cases: LoopClosing's SearchByProjection(Scw) th = 10 (an int) and 3; LocalMapping's Fuse th = 3.0 and 7.5;
# LoopClosing::SearchAndFuse's 4 and 10; ComputeSim3's SearchBySim3 th = 7.5 and 10.  Every th of {3, 4, 7.5, 10} occurs.
CASES = {SBP_SCW: [10, 3], FUSE: [3.0, 7.5], FUSE_SCW: [4.0, 10.0], SIM3: [7.5, 10.0]}
SCW_SCALE = np.float32(1.35)
SIM3_SCALE = np.float32(1.1)
REASONS = dict(valid=0, flagged=1, depth=2, image=3, near=4, far=5, angle=6)

_p = U._p
OrcView, OrcPoints = SP.OrcView, SP.OrcPoints


def bind_oracle(oracle):
    L = oracle.L
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    V, P = C.POINTER(OrcView), C.POINTER(OrcPoints)
    L.orc_sbp_scw.argtypes = [V, vp, vp, ci, P, vp, ci]
    L.orc_fuse.argtypes = [V, vp, vp, ci, P, vp, cf]
    L.orc_fuse_scw.argtypes = [V, vp, vp, ci, P, vp, cf, vp]
    L.orc_search_by_sim3.argtypes = [V, vp, vp, V, vp, vp, P, vp, cf, vp, vp, cf]
    for f in (L.orc_sbp_scw, L.orc_fuse, L.orc_fuse_scw, L.orc_search_by_sim3):
        f.restype = ci
    return L


def build_ref(outdir):
    so = os.path.join(str(outdir), 'project_keyframe_ref.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC,
                           '-o', so])
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    L.ref_decompose_scw.argtypes = [vp] * 4
    L.ref_decompose_scw.restype = None
    L.ref_keyframe_center.argtypes = [vp] * 3
    L.ref_keyframe_center.restype = None
    L.ref_sim3_matrices.argtypes = [C.c_float, vp, vp, vp, vp, vp]
    L.ref_sim3_matrices.restype = None
    L.ref_project_keyframe.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, C.c_float, vp,
                                       vp, vp, vp, vp]
    L.ref_project_keyframe.restype = ci
    return L


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def projection(R, t, K, Ow=None, sR=None, t2=None, invz_double=False, angle=True, dist_point=False):
    """one projection loop as a dict (the fields of OrbfeKeyFrameProjection); K = (fx, fy, cx, cy, logScaleFactor)"""
    return dict(R=_f32(R).reshape(3, 3), t=_f32(t), Ow=None if Ow is None else _f32(Ow), sR=None if sR is None else _f32(sR).reshape(3, 3),
                t2=None if t2 is None else _f32(t2), K=_f32(K), invz_double=bool(invz_double), angle=bool(angle), dist_point=bool(dist_point))


def api_projection(api, pr):
    K = pr['K']
    return api.KeyFrameProjection.make(pr['R'], pr['t'], K[0], K[1], K[2], K[3], K[4], Ow=pr['Ow'], sR=pr['sR'], t2=pr['t2'],
                                       invz_in_double=pr['invz_double'], check_viewing_angle=pr['angle'],
                                       distance_from_camera_point=pr['dist_point'])


def ref_project(L, tab, rows, flags, pr, bounds, sf, th):
    rows = np.ascontiguousarray(rows, np.int32)
    flags = np.ascontiguousarray(flags, np.uint8)
    sf = _f32(sf)
    n = len(rows)
    m = max(n, 1)
    va, uv, lv, ra, why = np.zeros(m, np.uint8), np.zeros((m, 2), np.float32), np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros(m, np.uint8)
    pos, nrm, mn, mx = (_f32(tab[k]) for k in ('pos', 'normal', 'min', 'max'))
    b = _f32(bounds)
    Ow = _f32(np.zeros(3)) if pr['Ow'] is None else pr['Ow']
    cnt = L.ref_project_keyframe(_p(pos), _p(nrm), _p(mn), _p(mx), _p(rows), _p(flags), n, _p(pr['R']), _p(pr['t']),
                                 None if pr['sR'] is None else _p(pr['sR']), None if pr['t2'] is None else _p(pr['t2']), _p(Ow),
                                 _p(pr['K']), _p(b), int(pr['invz_double']), int(pr['angle']), int(pr['dist_point']), _p(sf), len(sf),
                                 float(th), _p(va), _p(uv), _p(lv), _p(ra), _p(why))
    return dict(valid=va[:n], uv=uv[:n], level=lv[:n], radius=ra[:n], n_valid=cnt, reason=why[:n])


def check_projection(got, want):
    assert got['n_valid'] == want['n_valid']
    assert (got['valid'] == want['valid']).all()
    assert got['uv'].tobytes() == want['uv'].tobytes()
    assert (got['level'] == want['level']).all()
    if 'radius' in got:
        assert got['radius'].tobytes() == want['radius'].tobytes()


def pose16(R, t, scale=1.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = _f32(R) * np.float32(scale)
    T[:3, 3] = _f32(t) * np.float32(scale)
    return np.ascontiguousarray(T)


def decompose_scw(L, S16):
    R, t, Ow = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    L.ref_decompose_scw(_p(S16), _p(R), _p(t), _p(Ow))
    return R, t, Ow


def keyframe_center(L, R, t):
    Ow = np.zeros(3, np.float32)
    R, t = _f32(R), _f32(t)
    L.ref_keyframe_center(_p(R), _p(t), _p(Ow))
    return Ow


def sim3_matrices(L, s12, R12, t12):
    sR12, sR21, t21 = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    R12, t12 = _f32(R12), _f32(t12)
    L.ref_sim3_matrices(float(s12), _p(R12), _p(t12), _p(sR12), _p(sR21), _p(t21))
    return sR12, sR21, t21


def scene(kA, dA, kB, dB, sf, W, H, seed):
    """the table and the states every function's case draws from"""
    rng = np.random.default_rng(seed)
    camA = SP.with_center(U.camera(W, H))
    cam = SP.with_center(U.moved_camera(W, H, 3, -2, 8.0, seed=seed + 1))
    nA, nB = len(kA), len(kB)
    pts = SP.triangulate_keypoints(kA, dA, sf, camA, seed + 2)
    dist = U._norm((pts['pos'] - cam['Ow']).astype(np.float32))
    r = rng.random(nA)
    far, near, away = r < 0.02, (r >= 0.02) & (r < 0.04), (r >= 0.04) & (r < 0.08)
    pts['max'][far] = (dist[far] * np.float32(0.7)).astype(np.float32)
    pts['min'][far] = (pts['max'][far] * np.float32(0.1)).astype(np.float32)
    pts['min'][near] = (dist[near] * np.float32(1.5)).astype(np.float32)
    pts['max'][near] = (dist[near] * np.float32(2.0)).astype(np.float32)
    pts['normal'][away] = -pts['normal'][away]
    take = lambda idx: {k: v[idx].copy() for k, v in pts.items()}
    twins = take(rng.choice(nA, nA // 25, replace=False))
    behind = take(rng.choice(nA, nA // 50, replace=False))
    half = len(behind['pos']) // 2                               # the first half behind the camera, the rest beside the image
    behind['pos'][:half, 2] = -behind['pos'][:half, 2]
    behind['pos'][half:, 0] = ((np.float32(1.2 * W) - cam['cx']) * behind['pos'][half:, 2] / cam['fx']).astype(np.float32)
    holders = take(rng.integers(0, nA, nB // 4))
    # the second keyframe's own points (SearchBySim3): triangulated from B's keypoints in B's camera frame, taken to the world
    ptsB = SP.triangulate_keypoints(kB, dB, sf, camA, seed + 3)
    R64, t64 = cam['Rcw'].astype(np.float64), cam['tcw'].astype(np.float64)
    ptsB['pos'] = ((ptsB['pos'].astype(np.float64) - t64) @ R64).astype(np.float32)        # R^T (Pc - t)
    tab = pts
    first = {}
    for name, part in (('twin', twins), ('behind', behind), ('holder', holders), ('B', ptsB)):
        first[name] = len(tab['pos'])
        tab = U.concat(tab, part)
    M = len(tab['pos'])
    st = dict(bad=(rng.random(M) < 0.03).astype(np.uint8), nObs=rng.integers(0, 6, M).astype(np.int32))
    return dict(tab=tab, M=M, nA=nA, nB=nB, first=first, st=st, camA=camA, cam=cam, bounds=(0.0, float(W), 0.0, float(H)),
                K=_f32([cam['fx'], cam['fy'], cam['cx'], cam['cy'], cam['lsf']]), seed=seed)


def _view(kps, desc, sc, sf, is2):
    cam = sc['cam']
    return OrcView(_p(kps), _p(desc), len(kps), (C.c_float * 4)(*sc['bounds']), cam['fx'], cam['fy'], cam['cx'], cam['cy'], _p(sf),
                   _p(is2), len(sf), cam['lsf'])


def _slots(sc, rng):
    """keyframe B's mvpMapPoints: a quarter of its keypoints hold a holder MapPoint"""
    nB, h0 = sc['nB'], sc['first']['holder']
    nh = nB // 4
    slot = np.full(nB, -1, np.int32)
    idx = np.full(sc['M'], -1, np.int32)
    kps = rng.choice(nB, nh, replace=False)
    slot[kps] = h0 + np.arange(nh)
    idx[h0 + np.arange(nh)] = kps
    return slot, idx


def make_case(L, fn, sc, th):
    """The inputs of one function call on scene sc: the oracle's arrays and, per direction, the GPU call's (projection, rows,
    flags, searched view, kp_skip, claim, chi2, max_dist)."""
    rng = np.random.default_rng(sc['seed'] * 7 + FUNCS.index(fn))
    cam, st, M, nA, nB, first = sc['cam'], sc['st'], sc['M'], sc['nA'], sc['nB'], sc['first']
    bad = st['bad'].copy()
    nObs = st['nObs'].copy()
    cand_pool = np.concatenate([np.arange(nA), first['twin'] + np.arange(first['behind'] - first['twin']),
                                first['behind'] + np.arange(first['holder'] - first['behind'])])
    case = dict(fn=fn, th=th, bad=bad, nObs=nObs)
    if fn == SIM3:
        mp1 = np.where(rng.random(nA) < 0.3, -1, np.arange(nA)).astype(np.int32)
        nb = first['holder'] - first['behind']
        swap = rng.choice(nA, nb, replace=False)                  # a few of keyframe 1's keypoints observe a point behind it
        mp1[swap] = first['behind'] + np.arange(nb)
        mp2 = np.where(rng.random(nB) < 0.3, -1, first['B'] + np.arange(nB)).astype(np.int32)
        idx = np.full(M, -1, np.int32)
        have2 = np.flatnonzero(mp2 >= 0)
        idx[mp2[have2]] = have2                                   # GetIndexInKeyFrame(pKF2)
        m12 = np.full(nA, -1, np.int32)
        pre = rng.choice(nA, nA // 20, replace=False)
        m12[pre] = mp2[rng.choice(have2, len(pre), replace=False)]
        # the true relative pose of the two cameras (keyframe 1 = identity), scaled: p1 = s12 * (R12 p2 + t12 / s12)
        R12 = np.ascontiguousarray(cam['Rcw'].T, np.float32)       # (row-major in memory: the oracle reads the buffer)
        t12 = (-(cam['Rcw'].astype(np.float64).T @ cam['tcw'].astype(np.float64)) * float(SIM3_SCALE)).astype(np.float32)
        sR12, sR21, t21 = sim3_matrices(L, SIM3_SCALE, R12, t12)
        already1 = m12 >= 0
        already2 = np.zeros(nB, bool)
        hit = idx[m12[already1]]
        already2[hit[hit >= 0]] = True
        I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        dirs = []
        for mp, already, R, t, sR, tt, to in ((mp1, already1, I3, z3, sR21, t21, 'B'), (mp2, already2, cam['Rcw'], cam['tcw'], sR12, t12, 'A')):
            fl = np.zeros(len(mp), np.uint8)
            fl[(mp < 0) | already] = MP_SKIP
            has = mp >= 0
            fl[has & (fl == 0)] |= np.where(bad[mp[has & (fl == 0)]] != 0, MP_BAD, 0).astype(np.uint8)
            dirs.append(dict(pr=projection(R, t, sc['K'], sR=sR, t2=tt, invz_double=True, angle=False, dist_point=True),
                             rows=np.where(has, mp, 1 << 30).astype(np.int32), flags=fl, to=to, kp_skip=None, claim=False, chi2=False,
                             max_dist=TH_HIGH))
        case.update(mp1=mp1, mp2=mp2, idx=idx, m12=m12, s12=SIM3_SCALE, R12=R12, t12=t12, T1=pose16(I3, z3), T2=pose16(cam['Rcw'], cam['tcw']),
                    dirs=dirs)
        return case
    slot, idx = _slots(sc, rng)
    nh = nB // 4
    nObs[first['holder'] + np.arange(nh)] = rng.integers(1, 6, nh)
    points = rng.permutation(cand_pool)[:int(0.9 * len(cand_pool))].astype(np.int32)
    some_holders = (first['holder'] + rng.choice(nh, nh // 10, replace=False)).astype(np.int32)
    points = np.concatenate([points, some_holders]).astype(np.int32)
    points = points[rng.permutation(len(points))]
    case.update(points=points, slot=slot, idx=idx)
    fl = np.zeros(len(points), np.uint8)
    if fn == FUSE:
        points[rng.random(len(points)) < 0.03] = -1              # NULL candidates
        Rcw, tcw = cam['Rcw'], cam['tcw']
        Ow = keyframe_center(L, Rcw, tcw)
        has = points >= 0
        fl[~has] = MP_SKIP
        fl[has] |= np.where(bad[points[has]] != 0, MP_BAD, 0).astype(np.uint8)
        fl[has] |= np.where((idx[points[has]] >= 0) & (bad[points[has]] == 0), MP_SKIP, 0).astype(np.uint8)
        case.update(T=pose16(Rcw, tcw))
        d = dict(pr=projection(Rcw, tcw, sc['K'], Ow=Ow), kp_skip=None, claim=False, chi2=True)
    else:
        S16 = pose16(cam['Rcw'], cam['tcw'], SCW_SCALE)
        Rcw, tcw, Ow = decompose_scw(L, S16)
        case.update(T=S16)
        fl[bad[points] != 0] = MP_BAD
        if fn == SBP_SCW:
            # vpMatched: the keyframe's slots plus nothing else; a point in it is in spAlreadyFound
            found = np.zeros(M, bool)
            found[slot[slot >= 0]] = True
            fl[(fl == 0) & found[points]] = MP_SKIP
            d = dict(pr=projection(Rcw, tcw, sc['K'], Ow=Ow), kp_skip=(slot >= 0).astype(np.uint8), claim=True, chi2=False)
        else:
            found = np.zeros(M, bool)
            ok = slot[slot >= 0]
            found[ok[bad[ok] == 0]] = True                        # pKF->GetMapPoints(): non-NULL, not bad
            fl[(fl == 0) & found[points]] = MP_SKIP
            d = dict(pr=projection(Rcw, tcw, sc['K'], Ow=Ow, invz_double=True), kp_skip=None, claim=False, chi2=False)
    d.update(rows=np.where(points >= 0, points, 1 << 30).astype(np.int32), flags=fl, to='B', max_dist=TH_LOW)
    case['dirs'] = [d]
    return case


def run_oracle(oracle, fn, case, sc, kA, dA, kB, dB, sf):
    """the whole function on the CPU: dict of the return value and every output array"""
    L = oracle.L
    tab = sc['tab']
    kA, kB = np.ascontiguousarray(kA, KP_DTYPE), np.ascontiguousarray(kB, KP_DTYPE)
    dA, dB = np.ascontiguousarray(dA, np.uint8), np.ascontiguousarray(dB, np.uint8)
    sf = _f32(sf)
    is2 = _f32(1.0 / (sf * sf))
    pos, nrm, mn, mx = (_f32(tab[k]) for k in ('pos', 'normal', 'min', 'max'))
    desc = np.ascontiguousarray(tab['desc'], np.uint8)
    bad, nObs, idx = case['bad'].copy(), case['nObs'].copy(), case['idx'].copy()
    P = OrcPoints(sc['M'], _p(pos), _p(nrm), _p(mn), _p(mx), _p(desc), _p(bad), _p(nObs), _p(idx))
    VB = _view(kB, dB, sc, sf, is2)
    out = dict(bad=bad, nObs=nObs, idx=idx)
    if fn == SIM3:
        VA = _view(kA, dA, sc, sf, is2)
        m12 = case['m12'].copy()
        out['ret'] = L.orc_search_by_sim3(C.byref(VA), _p(case['T1']), _p(case['mp1']), C.byref(VB), _p(case['T2']), _p(case['mp2']),
                                          C.byref(P), _p(m12), float(case['s12']), _p(case['R12']), _p(case['t12']), float(case['th']))
        out['m12'] = m12
        return out
    slot = case['slot'].copy()
    pts = np.ascontiguousarray(case['points'], np.int32)
    if fn == SBP_SCW:
        out['ret'] = L.orc_sbp_scw(C.byref(VB), _p(case['T']), _p(pts), len(pts), C.byref(P), _p(slot), int(case['th']))
    elif fn == FUSE:
        out['ret'] = L.orc_fuse(C.byref(VB), _p(case['T']), _p(pts), len(pts), C.byref(P), _p(slot), float(case['th']))
    else:
        rep = np.full(len(pts), -1, np.int32)
        out['ret'] = L.orc_fuse_scw(C.byref(VB), _p(case['T']), _p(pts), len(pts), C.byref(P), _p(slot), float(case['th']), _p(rep))
        out['replace'] = rep
    out['slot'] = slot
    return out


def replay(fn, case, best):
    """The bookkeeping that follows the search (orb_shim.hpp), on best = [best_idx per direction]: the same dict as
    run_oracle's.  MapPoint::Replace / AddObservation follow the oracle's simplified model (oracle/orb_oracle_pose.h)."""
    bad, nObs, idx = case['bad'].copy(), case['nObs'].copy(), case['idx'].copy()
    out = dict(bad=bad, nObs=nObs, idx=idx)
    if fn == SIM3:
        vn1, vn2 = best
        m12 = case['m12'].copy()
        n = 0
        for i1 in range(len(vn1)):
            i2 = vn1[i1]
            if i2 >= 0 and vn2[i2] == i1:
                m12[i1] = case['mp2'][i2]
                n += 1
        out.update(ret=n, m12=m12, disagree=int(((vn1 >= 0) & (vn2[np.maximum(vn1, 0)] != np.arange(len(vn1)))).sum()))
        return out
    slot = case['slot'].copy()
    points, b = case['points'], best[0]
    n = 0

    def add_observation(p, k):
        if idx[p] >= 0:
            return
        idx[p] = k
        nObs[p] += 1

    def replace(a, c):                                           # a->Replace(c)
        if a == c:
            return
        bad[a] = 1
        ia = idx[a]
        nObs[c] += nObs[a] - (1 if ia >= 0 else 0)
        nObs[a] = 0
        idx[a] = -1
        if ia >= 0:
            if idx[c] < 0:
                slot[ia] = c
                add_observation(c, ia)
            else:
                slot[ia] = -1
    if fn == SBP_SCW:
        for i in range(len(points)):
            if b[i] >= 0:
                slot[b[i]] = points[i]
                n += 1
    elif fn == FUSE:
        for i in range(len(points)):
            p = points[i]
            if p < 0 or bad[p] or idx[p] >= 0 or b[i] < 0:       # the live checks of :822-823
                continue
            q = slot[b[i]]
            if q >= 0:
                if not bad[q]:
                    if nObs[q] > nObs[p]:
                        replace(p, q)
                    else:
                        replace(q, p)
            else:
                add_observation(p, b[i])
                slot[b[i]] = p
            n += 1
    else:
        rep = np.full(len(points), -1, np.int32)
        for i in range(len(points)):
            if b[i] < 0:
                continue
            q = slot[b[i]]
            if q >= 0:
                if not bad[q]:
                    rep[i] = q
            else:
                add_observation(points[i], b[i])
                slot[b[i]] = points[i]
            n += 1
        out['replace'] = rep
    out.update(ret=n, slot=slot)
    return out


def same_outputs(got, want):
    assert got['ret'] == want['ret'], (got['ret'], want['ret'])
    for k in ('slot', 'replace', 'm12', 'bad', 'nObs', 'idx'):
        if k in want:
            assert (np.asarray(got[k]) == np.asarray(want[k])).all(), k


def view_of(d, kA, dA, kB, dB):
    return (kA, dA) if d['to'] == 'A' else (kB, dB)


def cpu_search(oracle, d, proj, sc, kps, desc, sf, chi2_gate=True, with_skip=True):
    """the restatement's sources through the oracle's array-form search (orc_search_projected)"""
    is2 = _f32(1.0 / (_f32(sf) * _f32(sf)))
    sdesc = sc['tab']['desc'][np.where(proj['valid'] == 1, d['rows'], 0)]
    return oracle.search_projected(kps, desc, sc['bounds'], proj['uv'], proj['radius'], proj['level'], proj['valid'], sdesc,
                                   kp_skip=d['kp_skip'] if with_skip else None, claim=d['claim'],
                                   inv_sigma2=is2 if (d['chi2'] and chi2_gate) else None, chi2=5.99, max_dist=d['max_dist'])


def checked_oracle_case(L, oracle, fn, sc, th, kA, dA, kB, dB, sf, W, info):
    """One case on the CPU: restatement -> orc_search_projected -> replay reproduces the whole-function oracle exactly; the
    conditions that keep the case from passing vacuously are asserted on the way.  info collects, per function, which
    rejection branches fired."""
    case = make_case(L, fn, sc, th)
    want = run_oracle(oracle, fn, case, sc, kA, dA, kB, dB, sf)
    best, projs = [], []
    for d in case['dirs']:
        kps, desc = view_of(d, kA, dA, kB, dB)
        proj = ref_project(L, sc['tab'], d['rows'], d['flags'], d['pr'], sc['bounds'], sf, th)
        v = proj['valid'] == 1
        assert ((proj['level'][v] >= 0) & (proj['level'][v] < len(sf))).all()        # pruned share 0
        for name, code in REASONS.items():
            info[name] = info.get(name, 0) + int((proj['reason'] == code).sum())
        nm, bi, bd = cpu_search(oracle, d, proj, sc, kps, desc, sf)
        if d['chi2']:
            info['chi2'] = info.get('chi2', 0) + int((cpu_search(oracle, d, proj, sc, kps, desc, sf, chi2_gate=False)[1] != bi).sum())
        if d['kp_skip'] is not None:
            info['kp_skip'] = info.get('kp_skip', 0) + int((cpu_search(oracle, d, proj, sc, kps, desc, sf, with_skip=False)[1] != bi).sum())
        best.append(bi)
        projs.append(proj)
    got = replay(fn, case, best)
    same_outputs(got, want)
    assert want['ret'] > (60 if W >= 1920 else 15), want['ret']
    if fn == SIM3:
        info['disagree'] = info.get('disagree', 0) + got['disagree']
    return dict(case=case, want=want, projs=projs, best=best)


def assert_branches(fn, info):
    """every rejection branch of the function fired in at least one of its cases"""
    need = ['valid', 'flagged', 'depth', 'image', 'near', 'far']
    need += ['disagree'] if fn == SIM3 else ['angle']
    need += ['chi2'] if fn == FUSE else []
    need += ['kp_skip'] if fn == SBP_SCW else []
    for k in need:
        assert info.get(k, 0) > 0, (fn, k, info)


def case_seed(fn, th, W):
    return 3000 + 100 * FUNCS.index(fn) + int(th * 2) + (1 if W >= 1920 else 0)


def ulp(x, k=1):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def edge_points(bounds, K, sf):
    """MapPoints on the edges of the projection for the identity pose (p = p3Dw, Ow = 0): z = +0, -0 and slightly negative;
    u exactly on maxX (rejected: IsInImage is half-open) and on minX (accepted), likewise v; dist3D exactly on both invariance
    bounds and one float beyond; dot == 0.5*dist and one float below.  Returns the table and a dict of named indices."""
    f32 = np.float32
    fx, fy, cx, cy = (f32(v) for v in K[:4])
    pos, nrm, mn, mx, names = [], [], [], [], {}

    def add(name, p, n=(0, 0, 1), lo=0.5, hi=60.0):
        names[name] = len(pos)
        pos.append(np.array(p, np.float32)); nrm.append(np.array(n, np.float32)); mn.append(f32(lo)); mx.append(f32(hi))
    add('z_plus0', (0.3, 0.2, 0.0))
    add('z_minus0', (0.3, 0.2, -0.0))
    add('z_plus0_origin', (0.0, 0.0, 0.0))
    add('z_minus0_origin', (0.0, 0.0, -0.0))
    add('z_negative', (0.0, 0.0, -1e-7))
    add('z_tiny', (0.0, 0.0, 1e-30))
    # z = 1: invz = 1 in both forms, x = X, u = fx*X + cx: search the X whose u lands exactly on each bound
    def on_bound(f, c, b):
        x = f32((f32(b) - c) / f)
        for k in range(-64, 65):
            X = ulp(x, k)
            if f32(f32(f * X) + c) == f32(b):
                return X
        raise AssertionError('no float projects onto the bound')
    add('u_maxX', (on_bound(fx, cx, bounds[1]), 0.0, 1.0), lo=0.1, hi=2.0)
    add('u_minX', (on_bound(fx, cx, bounds[0]), 0.0, 1.0), lo=0.1, hi=2.0)
    add('v_maxY', (0.0, on_bound(fy, cy, bounds[3]), 1.0), lo=0.1, hi=2.0)
    add('v_minY', (0.0, on_bound(fy, cy, bounds[2]), 1.0), lo=0.1, hi=2.0)
    Z = f32(10.0)                                               # dist3D = 10 exactly
    P = (0.0, 0.0, Z)

    def raw_for(factor, target, beyond):
        """a raw distance r with factor*r == target (float), or just beyond it on the side `beyond`"""
        r = f32(target / factor)
        for k in range(-8, 9):
            if f32(factor * ulp(r, k)) == target:
                r = ulp(r, k)
                break
        else:
            raise AssertionError('no raw distance lands on the bound')
        while beyond and f32(factor * r) == target:
            r = ulp(r, beyond)
        return r
    add('dist_on_max', P, lo=0.5, hi=raw_for(f32(1.2), Z, 0))
    add('dist_past_max', P, lo=0.5, hi=raw_for(f32(1.2), Z, -1))
    add('dist_on_min', P, lo=raw_for(f32(0.8), Z, 0), hi=100.0)
    add('dist_before_min', P, lo=raw_for(f32(0.8), Z, +1), hi=100.0)
    add('dot_on_half', P, n=(0.0, 0.0, 0.5), lo=8.0, hi=9.0)   # PO.dot(Pn) = 5 = 0.5*dist: not rejected
    add('dot_below_half', P, n=(0.0, 0.0, ulp(0.5, -1)), lo=8.0, hi=9.0)
    for lv in range(len(sf)):                                   # the ulp-sensitive PredictScale: max = dist * sf[level]
        add('level_%d' % lv, P, lo=0.01, hi=f32(Z * f32(sf[lv])))
    add('invz_probe', (0.37, -0.21, 3.0), lo=0.1, hi=100.0)   # both invz forms are run on every point (invz_forms_differ below)
    tab = dict(pos=np.array(pos, np.float32), normal=np.array(nrm, np.float32), min=np.array(mn, np.float32),
               max=np.array(mx, np.float32), desc=np.zeros((len(pos), 32), np.uint8))
    return tab, names


def assert_edges(L, tab, names, bounds, K, sf, th=4.0):
    """the restatement on the edge points, identity pose: each edge lands on the side the reference puts it"""
    n = len(tab['pos'])
    I3, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    rows, fl = np.arange(n, dtype=np.int32), np.zeros(n, np.uint8)
    out = {}
    for dbl in (False, True):
        out[dbl] = ref_project(L, tab, rows, fl, projection(I3, z3, K, Ow=z3, invz_double=dbl), bounds, sf, th)
    r = out[False]
    why = lambda k: int(r['reason'][names[k]])
    for k in ('z_plus0', 'z_minus0', 'z_plus0_origin', 'z_minus0_origin'):
        assert why(k) == REASONS['image'], k                    # a NaN or infinite projection fails IsInImage by itself
    assert why('z_tiny') == REASONS['near']                     # (on the optical axis a tiny z projects onto cx, cy: finite)
    assert why('z_negative') == REASONS['depth']
    assert why('u_maxX') == REASONS['image'] and why('v_maxY') == REASONS['image']     # half-open
    assert why('u_minX') == 0 and why('v_minY') == 0
    assert r['uv'][names['u_minX'], 0] == np.float32(bounds[0]) and r['uv'][names['v_minY'], 1] == np.float32(bounds[2])   # (on_bound put u_maxX on maxX likewise)
    assert why('dist_on_max') == 0 and why('dist_past_max') == REASONS['far']
    assert why('dist_on_min') == 0 and why('dist_before_min') == REASONS['near']
    assert why('dot_on_half') == 0 and why('dot_below_half') == REASONS['angle']
    for lv in range(len(sf)):
        assert r['valid'][names['level_%d' % lv]] == 1
    return out


def invz_forms_differ():
    """Number of floats z in [1, 2) -- every mantissa, so every normal float up to a power of two -- on which the float
    division 1/z (:326, :840) and the double division rounded to float (float)(1.0/(double)z) (:983, :1130, :1210) differ."""
    z = np.arange(0x3f800000, 0x40000000, dtype=np.uint32).view(np.float32)
    a = np.float32(1.0) / z
    b = (1.0 / z.astype(np.float64)).astype(np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())
