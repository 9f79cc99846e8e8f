"""Shared by tests/test_ransac_score.py and tests/test_gpu_ransac_score.py: the seeded scenes of the RANSAC-scoring tests, the
ctypes binding of the restatement tests/cpp/ransac_score_ref.cpp (built here with g++ -O2 -ffp-contract=off), a second,
independent restatement in numpy (np.float32 wherever the reference says float, np.float64 wherever it says double, every
widening and rounding an explicit astype), the crafted sets, the scripted round-robin scenes and the scene files
tests/cpp/ransac_score_test.cpp reads.

A Sim3 scene is one loop candidate: points seen by two keyframes whose camera frames differ by a similarity (s, R, t), projected
with pixel noise, about 30 % of the correspondences wrong.  A PnP scene is one relocalisation candidate: world points and their
noisy projections under a pose.  Hypotheses are perturbations of the true transform, from none to gross, so that inlier ratios
run from 1 to 0: they are INPUTS of the scoring and need not be what Horn's method or EPnP would give."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')
REF_SRC = os.path.join(CPP, 'ransac_score_ref.cpp')
SWEEP_N = (1, 63, 64, 65, 255, 256, 257, 1000)
SWEEP_K = (1, 5, 300)
MULTI_N = (65, 0, 257)
f32, f64 = np.float32, np.float64
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
TH2 = 5.991


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_ref(outdir, name='ransac_score_ref.so'):
    so = os.path.join(str(outdir), name)
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror',
                           '-I' + os.path.join(ROOT, 'oracle'), '-I' + CPP, REF_SRC, '-o', so])
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    L.rsr_check_sim3.argtypes = [vp, ci, vp, vp, vp, vp]
    L.rsr_check_pnp.argtypes = [vp, ci, vp, vp, vp]
    L.rsr_score_sim3.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.rsr_score_pnp.argtypes = [ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    return L


# ---------------------------------------------------------------------------------------------------------------------
# A call: model, corr [N][12 | 6], cams [n_seg][8 f32 | 4 f64], hyp [K][24 f32 = T12, T21 | 12 f64 = Rt], seg_off, hyp_seg
# ---------------------------------------------------------------------------------------------------------------------
class Call:
    def __init__(self, model, corr, cams, hyp, seg_off=None, hyp_seg=None):
        self.model = model
        row = 12 if model == 'sim3' else 6
        self.corr = np.ascontiguousarray(corr, f32).reshape(-1, row)
        if model == 'sim3':
            self.cams = np.ascontiguousarray(cams, f32).reshape(-1, 8)
            self.hyp = np.ascontiguousarray(hyp, f32).reshape(-1, 24)
        else:
            self.cams = np.ascontiguousarray(cams, f64).reshape(-1, 4)
            self.hyp = np.ascontiguousarray(hyp, f64).reshape(-1, 12)
        K = len(self.hyp)
        self.seg_off = np.ascontiguousarray([0, len(self.corr)] if seg_off is None else seg_off, np.int32)
        self.hyp_seg = np.ascontiguousarray(np.zeros(K, np.int32) if hyp_seg is None else hyp_seg, np.int32)

    @property
    def T12(self):
        return np.ascontiguousarray(self.hyp[:, :12])

    @property
    def T21(self):
        return np.ascontiguousarray(self.hyp[:, 12:])

    def n_of(self, k):
        s = self.hyp_seg[k]
        return int(self.seg_off[s + 1] - self.seg_off[s])

    def rows_of(self, k):
        s = self.hyp_seg[k]
        return self.corr[self.seg_off[s]:self.seg_off[s + 1]]


def words_of(n):
    return (int(n) + 63) // 64


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder='little')[:n].astype(bool)


def ref_score(L, call):
    """(counts, [bool mask per hypothesis]) by the C++ restatement, through its whole-call entry (packed words)."""
    K = len(call.hyp)
    ns = [call.n_of(k) for k in range(K)]
    counts = np.full(K, -1, np.int32)
    words = np.full(max(sum(words_of(n) for n in ns), 1), 0xdeadbeefdeadbeef, np.uint64)
    if call.model == 'sim3':
        T12, T21 = call.T12, call.T21
        rc = L.rsr_score_sim3(len(call.seg_off) - 1, _p(call.seg_off), _p(call.corr), _p(call.cams), K, _p(call.hyp_seg), _p(T12), _p(T21),
                              _p(counts), None, _p(words))
    else:
        rc = L.rsr_score_pnp(len(call.seg_off) - 1, _p(call.seg_off), _p(call.corr), _p(call.cams), K, _p(call.hyp_seg), _p(call.hyp), _p(counts),
                             None, _p(words))
    assert rc == 0
    masks, at = [], 0
    for n in ns:
        masks.append(unpack(words[at:at + words_of(n)], n))
        at += words_of(n)
    return counts, masks


# ---------------------------------------------------------------------------------------------------------------------
# The numpy restatement: one hypothesis, all correspondences of its segment at once; every operation is an array operation in
# the precision the reference's expression has, every change of precision an explicit astype (numpy fuses nothing).
# ---------------------------------------------------------------------------------------------------------------------
def _np_project(T, X, K):
    """Sim3Solver::Project (Sim3Solver.cc:385-406).  T: 12 float32 (top three rows of Tcw); X: [n][3] float32; K: fx fy cx cy."""
    T = [f32(v) for v in T]
    fx, fy, cx, cy = (f32(v) for v in K)
    x0, x1, x2 = X[:, 0], X[:, 1], X[:, 2]
    comp = []
    for r in range(3):
        t = T[4 * r] * x0 + T[4 * r + 1] * x1 + T[4 * r + 2] * x2             # float, left to right
        comp.append((t.astype(f64) + f64(T[4 * r + 3])).astype(f32))          # (float)((double)t + (double)tcw)
    invz = f32(1) / comp[2]
    x = comp[0] * invz
    y = comp[1] * invz
    return fx * x + cx, fy * y + cy


def _np_dot2(dx, dy):
    return (dx.astype(f64) * dx.astype(f64) + dy.astype(f64) * dy.astype(f64)).astype(f32)


def np_check_sim3(rows, cams, hyp):
    """Sim3Solver::CheckInliers (:343-367) -> bool mask"""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    with np.errstate(all='ignore'):
        u, v = _np_project(hyp[:12], rows[:, 3:6], cams[:4])        # vP2im1 = Project(mvX3Dc2, mT12i, mK1)
        err1 = _np_dot2(rows[:, 6] - u, rows[:, 7] - v)
        u, v = _np_project(hyp[12:], rows[:, 0:3], cams[4:])        # vP1im2 = Project(mvX3Dc1, mT21i, mK2)
        err2 = _np_dot2(u - rows[:, 8], v - rows[:, 9])
        return (err1 < rows[:, 10]) & (err2 < rows[:, 11])


def np_check_pnp(rows, cams, hyp, all_float=False):
    """PnPsolver::CheckInliers (PnPsolver.cc:313-344) -> bool mask.  all_float: the same test with every double replaced by float --
    NOT the reference; what an implementation that ignored the doubles would compute."""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 6)
    wide = f32 if all_float else f64
    R = [wide(v) for v in hyp]
    uc, vc, fu, fv = (wide(v) for v in cams)
    with np.errstate(all='ignore'):
        px, py, pz = (rows[:, i].astype(wide) for i in range(3))
        Xc = (R[0] * px + R[1] * py + R[2] * pz + R[9]).astype(f32)
        Yc = (R[3] * px + R[4] * py + R[5] * pz + R[10]).astype(f32)
        invZc = (wide(1.0) / (R[6] * px + R[7] * py + R[8] * pz + R[11])).astype(f32)
        ue = uc + fu * Xc.astype(wide) * invZc.astype(wide)
        ve = vc + fv * Yc.astype(wide) * invZc.astype(wide)
        distX = (rows[:, 3].astype(wide) - ue).astype(f32)
        distY = (rows[:, 4].astype(wide) - ve).astype(f32)
        error2 = distX * distX + distY * distY
        return error2 < rows[:, 5]


def np_score(call, all_float=False):
    K = len(call.hyp)
    masks = []
    for k in range(K):
        s = call.hyp_seg[k]
        if call.model == 'sim3':
            masks.append(np_check_sim3(call.rows_of(k), call.cams[s], call.hyp[k]))
        else:
            masks.append(np_check_pnp(call.rows_of(k), call.cams[s], call.hyp[k], all_float))
    return np.array([m.sum() for m in masks], np.int32), masks


def assert_same(got, want, what=''):
    gc, gm = got
    wc, wm = want
    assert np.array_equal(np.asarray(gc, np.int32), wc), '%s: counts differ at %s' % (what, np.nonzero(np.asarray(gc) != wc)[0][:8])
    assert len(gm) == len(wm)
    for k, (a, b) in enumerate(zip(gm, wm)):
        assert a.shape == b.shape and np.array_equal(a, b), '%s: mask of hypothesis %d differs at %s' % (what, k, np.nonzero(a != b)[0][:8])


# ---------------------------------------------------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------------------------------------------------
def sim3_max_error(sigma2):
    """(float)(size_t)(9.210*sigmaSquare): a double product, truncated (Sim3Solver.cc:87-88)"""
    return f32(int(9.210 * float(f32(sigma2))))


def pnp_max_error(sigma2, th2=TH2):
    """mvSigma2[i]*th2 in float (PnPsolver.cc:160)"""
    return f32(sigma2) * f32(th2)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _level_sigma2(rng, n):
    return (1.2 ** (2 * rng.integers(0, 8, n))).astype(f32)


def sim3_pack(s, R, t):
    """T12 = [sR | t], T21 = [(1/s)R' | -(1/s)R't] as 24 float32"""
    sR = s * R
    sRinv = (1.0 / s) * R.T
    return np.concatenate([np.concatenate([sR, t[:, None]], 1).reshape(12), np.concatenate([sRinv, (-sRinv @ t)[:, None]], 1).reshape(12)]).astype(f32)


def perturb_levels(K):
    """K perturbation sizes from 0 (the truth) to gross, so that inlier ratios run from 1 to 0"""
    return np.concatenate([[0.0], np.geomspace(1e-4, 0.5, K - 1)]) if K > 1 else np.array([0.0])


def make_sim3(seed, n, K, noise=0.5, wrong=0.3):
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(20, 730, n), rng.uniform(20, 460, n)], 1)
    depth = rng.uniform(2.0, 10.0, n)
    X1 = np.stack([(uv[:, 0] - CX) / FX * depth, (uv[:, 1] - CY) / FY * depth, depth], 1)
    s, R, t = 1.3, _rot(0.03, -0.06, 0.04), np.array([0.3, -0.05, 0.2])
    X2 = (X1 - t) @ R / s                                            # X1 = s R X2 + t
    K2 = (FX * 1.01, FY * 0.99, CX + 3, CY - 2)
    p1 = uv + rng.normal(0, noise, uv.shape)
    p2 = np.stack([K2[0] * X2[:, 0] / X2[:, 2] + K2[2], K2[1] * X2[:, 1] / X2[:, 2] + K2[3]], 1) + rng.normal(0, noise, uv.shape)
    bad = rng.random(n) < wrong
    p2[bad] = np.stack([rng.uniform(0, 752, bad.sum()), rng.uniform(0, 480, bad.sum())], 1)
    s1, s2 = _level_sigma2(rng, n), _level_sigma2(rng, n)
    corr = np.concatenate([X1, X2, p1, p2, np.array([sim3_max_error(v) for v in s1])[:, None], np.array([sim3_max_error(v) for v in s2])[:, None]], 1)
    hyp = np.zeros((K, 24), f32)
    for k, e in enumerate(perturb_levels(K)):
        d = rng.normal(0, 1, 7) * e
        hyp[k] = sim3_pack(s * (1 + d[0]), _rot(*(0.2 * d[1:4])) @ R, t + d[4:7])
    cams = np.array([FX, FY, CX, CY] + list(K2), f32)
    return np.ascontiguousarray(corr, f32), cams, hyp


def make_pnp(seed, n, K, noise=0.5, wrong=0.3):
    rng = np.random.default_rng(seed)
    R, t = _rot(0.4, -0.3, 0.2), np.array([30.0, -20.0, 60.0])       # a map whose origin is far away: R*X + t cancels, which an all-float evaluation feels
    uv = np.stack([rng.uniform(20, 730, n), rng.uniform(20, 460, n)], 1)
    depth = rng.uniform(2.0, 10.0, n)
    Xc = np.stack([(uv[:, 0] - CX) / FX * depth, (uv[:, 1] - CY) / FY * depth, depth], 1)
    Xw = (Xc - t) @ R                                                 # Xc = R Xw + t
    p = uv + rng.normal(0, noise, uv.shape)
    bad = rng.random(n) < wrong
    p[bad] = np.stack([rng.uniform(0, 752, bad.sum()), rng.uniform(0, 480, bad.sum())], 1)
    s2 = _level_sigma2(rng, n)
    corr = np.concatenate([Xw, p, np.array([pnp_max_error(v) for v in s2])[:, None]], 1)
    hyp = np.zeros((K, 12), f64)
    for k, e in enumerate(perturb_levels(K)):
        d = rng.normal(0, 1, 6) * e
        Rk = _rot(*(0.2 * d[:3]))                                    # the camera turned and moved a little: Xc' = Rk Xc + d
        hyp[k] = np.concatenate([(Rk @ R).reshape(9), Rk @ t + d[3:]])
    cams = np.array([CX, CY, FX, FY], f64)
    return np.ascontiguousarray(corr, f32), cams, hyp


_cache = {}


def sweep_call(model, n, K):
    """The call of the shape sweep for (model, N, K): one segment; built once per process and never changed."""
    key = (model, n, K)
    if key not in _cache:
        make = make_sim3 if model == 'sim3' else make_pnp
        corr, cams, hyp = make(1000 + 7 * n + K, n, K)
        _cache[key] = Call(model, corr, cams, hyp)
    return _cache[key]


def multi_call(model):
    """Three segments of N = 65, 0, 257 with interleaved hyp_seg, seg_off not starting at 0 (two unused rows in front)."""
    key = (model, 'multi')
    if key not in _cache:
        make = make_sim3 if model == 'sim3' else make_pnp
        parts = [make(77 + i, max(n, 1), 5) for i, n in enumerate(MULTI_N)]
        rows = [np.zeros((2, parts[0][0].shape[1]), f32)] + [p[0][:n] for p, n in zip(parts, MULTI_N)]
        seg_off = 2 + np.concatenate([[0], np.cumsum(MULTI_N)])
        hyp_seg = np.array([0, 2, 1, 2, 0, 1, 2, 0, 0, 2, 1], np.int32)
        taken = [0, 0, 0]
        hyp = []
        for s in hyp_seg:
            hyp.append(parts[s][2][taken[s] % 5])
            taken[s] += 1
        _cache[key] = Call(model, np.concatenate(rows), np.stack([p[1] for p in parts]), np.stack(hyp), seg_off, hyp_seg)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------------
# The crafted set.  Identity transform, z = 1, integer coordinates, fx = fy = 1, cx = cy = 0: every intermediate is exact, so the
# reference's verdict follows by hand.  With the image point offset by 3 in x the error is exactly 9.
# ---------------------------------------------------------------------------------------------------------------------
IDENT34 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], f64)
C_AT, C_BELOW, C_Z0, C_BEHIND, C_MAX0, C_PLAIN, C_SIGMA = range(7)
H_IDENT, H_NAN = 0, 1
BELOW3 = np.nextafter(f32(3), f32(0))        # the next float below 3; fl(BELOW3^2) is the next float below 9
SIGMA2_L1 = f32(1.44)                        # mvLevelSigma2[1] at scaleFactor 1.2


def crafted(model):
    """-> (Call, expected masks [2][7]).  Correspondences (C_*): an error exactly equal to the maximum 9 (outlier: the test is <);
    an offset of the next float below 3, whose error is the next float below 9 (inlier); z = 0 (1/0 = inf, an infinite error:
    outlier); z = -1 with the image point where the point behind the camera projects (inlier: nothing tests the sign of z); an
    exact hit with maxErr = 0 (0 < 0 is false: outlier); an ordinary exact hit; the maximum of sigmaSquare = 1.44 -- SIM3: 13,
    not 13.26, so an offset of 3.62 (error 13.1044) is an outlier; PNP: 1.44f * 5.991f = 8.627..., an offset of 2.9 (8.41) is an
    inlier.  Hypotheses: the identity; all NaN (counts 0)."""
    off = 3.62 if model == 'sim3' else 2.9
    X = np.array([[5, 2, 1], [0, 2, 1], [5, 2, 0], [5, 2, -1], [4, 1, 1], [7, 3, 1], [0, 0, 1]], f64)
    uv = np.array([[5 + 3, 2], [float(BELOW3), 2], [5, 2], [-5, -2], [4, 1], [7, 3], [off, 0]], f64)
    mx = np.array([9, 9, 9, 9, 0, 9, float(sim3_max_error(SIGMA2_L1) if model == 'sim3' else pnp_max_error(SIGMA2_L1))], f64)
    if model == 'sim3':
        corr = np.concatenate([X, X, uv, uv, mx[:, None], mx[:, None]], 1)
        cams = np.array([1, 1, 0, 0, 1, 1, 0, 0], f32)
        hyp = np.stack([np.concatenate([IDENT34, IDENT34]), np.full(24, np.nan)]).astype(f32)
    else:
        corr = np.concatenate([X, uv, mx[:, None]], 1)
        cams = np.array([0, 0, 1, 1], f64)
        hyp = np.stack([np.concatenate([IDENT34.reshape(3, 4)[:, :3].reshape(9), [0, 0, 0]]), np.full(12, np.nan)])
    want = np.array([[False, True, False, True, False, True, model != 'sim3'], [False] * 7])
    return Call(model, corr, cams, hyp), want


# ---------------------------------------------------------------------------------------------------------------------
# Scripted round-robin scenes for tests/cpp/ransac_score_test.cpp.  A scripted candidate has N correspondences X = (i, 0, 1) seen at
# (i, 0) with maxErr_i = i + 1, identity rotations, fx = 1, cx = 0.  A hypothesis that shifts every projection by sqrt(m + 1/2)
# has error ~ m + 1/2 everywhere, so exactly the correspondences i >= m are inliers: its count is N - m, whatever is asked for.
# ---------------------------------------------------------------------------------------------------------------------
def scripted_candidate(model, N, counts, refined_counts=(), n_full=None, seed=0):
    rng = np.random.default_rng(seed)
    n_full = N + 7 if n_full is None else n_full
    idx = np.sort(rng.choice(n_full, N, replace=False)).astype(np.int32)
    i = np.arange(N, dtype=f64)
    one, zero = np.ones(N), np.zeros(N)
    X = np.stack([i, zero, one], 1)
    shift = lambda c: float(f32(np.sqrt(N - c + 0.5)))
    if model == 'sim3':
        corr = np.concatenate([X, X, np.stack([i, zero], 1), np.stack([i, zero], 1), (i + 1)[:, None], (i + 1)[:, None]], 1)
        cams = np.array([1, 1, 0, 0, 1, 1, 0, 0], f32)
        hyp = np.zeros((len(counts), 24), f32)
        for k, c in enumerate(counts):
            a, b = IDENT34.copy(), IDENT34.copy()
            a[3], b[3] = shift(c), -shift(c)
            hyp[k] = np.concatenate([a, b])
        refined = np.zeros((0, 12), f64)
    else:
        corr = np.concatenate([X, np.stack([i, zero], 1), (i + 1)[:, None]], 1)
        cams = np.array([0, 0, 1, 1], f64)
        mk = lambda c: np.concatenate([np.eye(3).reshape(9), [shift(c), 0, 0]])
        hyp = np.stack([mk(c) for c in counts]) if len(counts) else np.zeros((0, 12), f64)
        refined = np.stack([mk(c) for c in refined_counts]) if len(refined_counts) else np.zeros((0, 12), f64)
    return dict(N=N, n_full=n_full, indices=idx, corr=np.ascontiguousarray(corr, f32), cams=cams, hyp=hyp, refined=refined)


def candidate_from(model, corr, cams, hyp, refined=None, seed=0):
    N = len(corr)
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(N + 11, N, replace=False)).astype(np.int32)
    return dict(N=N, n_full=N + 11, indices=idx, corr=np.ascontiguousarray(corr, f32), cams=cams, hyp=hyp,
                refined=np.zeros((0, 12), f64) if refined is None else np.ascontiguousarray(refined, f64))


def write_scene(path, model, cands, n_iter=5, min_inliers=20, max_its=300, probability=0.99, min_set=4, epsilon=0.5, calls=0):
    """The file tests/cpp/ransac_score_test.cpp reads.  calls > 0: exactly that many iterate() calls per candidate, whatever they return
    (a solver's state carried from call to call); 0: the round-robin's own rule, a candidate leaves when it gives a pose or gives up."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<6idfi', 0 if model == 'sim3' else 1, len(cands), n_iter, min_inliers, max_its, min_set, probability, epsilon, calls))
        for c in cands:
            f.write(struct.pack('<4i', c['N'], c['n_full'], len(c['hyp']), len(c['refined'])))
            f.write(np.ascontiguousarray(c['indices'], np.int32).tobytes())
            f.write(np.ascontiguousarray(c['corr'], f32).tobytes())
            if model == 'sim3':
                h = np.ascontiguousarray(c['hyp'], f32).reshape(-1, 24)
                f.write(np.ascontiguousarray(c['cams'], f32).tobytes())
                f.write(np.ascontiguousarray(h[:, :12]).tobytes())
                f.write(np.ascontiguousarray(h[:, 12:]).tobytes())
            else:
                f.write(np.ascontiguousarray(c['cams'], f64).tobytes())
                f.write(np.ascontiguousarray(c['hyp'], f64).tobytes())
                f.write(np.ascontiguousarray(c['refined'], f64).tobytes())
    return path


def compile_walk_test(out, host):
    """tests/cpp/ransac_score_test.cpp with the restatement; host: scoring by the restatement (no GPU), else through the library."""
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
           '-I' + os.path.join(ROOT, 'oracle'), '-I' + CPP, os.path.join(CPP, 'ransac_score_test.cpp'), REF_SRC, '-o', out]
    if host:
        cmd.append('-DRANSAC_SCORE_HOST')
    else:
        from os1_amd import api
        if not os.path.exists(api.lib_path()):
            api.build_library()
        cmd += [api.lib_path(), '-Wl,-rpath,' + os.path.dirname(api.lib_path()), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run_walk_test(exe, scene_files):
    """-> (all output lines, {scene path: [dict per iterate() line]})"""
    r = subprocess.run([exe] + list(scene_files), capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'PASS', r.stdout[-3000:] + r.stderr[-2000:]
    calls, cur = {}, None
    for ln in lines:
        if ln.startswith('  round '):
            w = ln.split()
            calls[cur].append({w[i]: int(w[i + 1]) for i in range(0, 16, 2)})
        elif ': model ' in ln:
            cur = ln.split(': model ')[0]
            calls[cur] = []
    return lines, calls


def sim3_round_robin_scene(path):
    """Three loop candidates in round-robin (LoopClosing.cc:286-346): one whose hypotheses improve from gross to exact and gives a
    pose after a few rounds, one with fewer correspondences than mRansacMinInliers (gone in round 0), one whose hypotheses never fit
    and which runs until its iterations are spent."""
    corr, cams, hyp = make_sim3(5, 100, 40)
    improving = candidate_from('sim3', corr, cams, hyp[::-1].copy(), seed=1)
    corr, cams, hyp = make_sim3(6, 15, 10)
    few = candidate_from('sim3', corr, cams, hyp, seed=2)
    corr, cams, hyp = make_sim3(7, 257, 40)
    hopeless = candidate_from('sim3', corr, cams, np.tile(hyp[-8:], (5, 1)), seed=3)
    return write_scene(path, 'sim3', [improving, few, hopeless], min_inliers=20)


def pnp_refine_scene(path):
    """Two relocalisation candidates (Tracking.cc:1015, :1040): one whose hypotheses improve until one is accepted, with a Refine
    that fails on a gross pose and then succeeds on the true one; one whose hypotheses never fit."""
    corr, cams, hyp = make_pnp(9, 100, 40)
    improving = candidate_from('pnp', corr, cams, hyp[::-1].copy(), refined=np.stack([hyp[-1], hyp[0]]), seed=4)
    corr, cams, hyp = make_pnp(10, 65, 40)
    hopeless = candidate_from('pnp', corr, cams, np.tile(hyp[-8:], (5, 1)), seed=5)
    return write_scene(path, 'pnp', [improving, hopeless], min_inliers=10, epsilon=0.5)
