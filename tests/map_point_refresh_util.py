"""Shared by tests/test_map_point_refresh.py and tests/test_gpu_map_point_refresh.py: the ctypes binding of the restatement
tests/cpp/map_point_refresh_ref.cpp (built here with g++ -O2 -ffp-contract=off), a second, independent restatement of the
normal / depth chain in numpy (np.float32 wherever the reference holds a float, Python floats = float64 for cv::norm and the
`1.0/...` scales), the seeded scene of the tests, and the build of tests/cpp/map_point_refresh_test.cpp.

The scene: keyframes of 64-300 random keypoints (random descriptors, octaves 0..7, a random camera centre each), a table of 64
rows, and a batch of MapPoints whose observation lists cover the shapes named in the GPU test."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')
REF_SRC = os.path.join(CPP, 'map_point_refresh_ref.cpp')
f32 = np.float32
NLEVELS = 8
SF = np.cumprod(np.concatenate([[1.0], np.full(NLEVELS - 1, 1.2)]).astype(f32), dtype=f32)   # mvScaleFactors as ORBextractor builds them
CAPACITY = 64
OBS_KF_BAD, DESCRIPTOR, NORMAL_DEPTH = 1, 1, 2


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_ref(outdir, name='map_point_refresh_ref.so'):
    so = os.path.join(str(outdir), name)
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC, '-o', so])
    L = C.CDLL(so)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.mpr_distinctive.argtypes = [vp, ci]
    L.mpr_normal_depth.argtypes = [vp, ci, vp, vp, cf, cf, vp]
    L.mpr_normal_depth.restype = None
    L.mpr_refresh_rows.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, ci] + [vp] * 11
    return L


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of UpdateNormalAndDepth (the chain of the issue, one operation per line)
# ---------------------------------------------------------------------------------------------------------------------
def np_normal_depth(pos, Ow, Ow_ref, sf_level, sf_last):
    """pos [3], Ow [n][3] in observation order -> (normal [3], min, max) as float32."""
    pos = np.asarray(pos, f32)
    Ow = np.asarray(Ow, f32).reshape(-1, 3)
    n = len(Ow)
    normal = np.zeros(3, f32)                                    # +0.0f
    for i in range(n):
        ni = pos - Ow[i]                                         # float32 subtraction
        nrm = float(np.sqrt(float(ni[0]) * float(ni[0]) + float(ni[1]) * float(ni[1]) + float(ni[2]) * float(ni[2])))
        beta = f32(1.0 / nrm)                                    # a double division, rounded to float
        normal = (ni * beta).astype(f32) + normal                # product rounded, then the sum
    normal = (normal * f32(1.0 / n)).astype(f32) + f32(0.0)      # convertTo: -0 becomes +0
    pc = pos - np.asarray(Ow_ref, f32)
    dist = f32(np.sqrt(float(pc[0]) * float(pc[0]) + float(pc[1]) * float(pc[1]) + float(pc[2]) * float(pc[2])))
    mx = f32(dist * f32(sf_level))
    mn = f32(mx / f32(sf_last))
    return normal.astype(f32), mn, mx


def ref_normal_depth(L, pos, Ow, Ow_ref, sf_level, sf_last):
    pos = np.ascontiguousarray(pos, f32)
    Ow = np.ascontiguousarray(Ow, f32).reshape(-1, 3)
    Ow_ref = np.ascontiguousarray(Ow_ref, f32)
    out = np.zeros(5, f32)
    L.mpr_normal_depth(_p(pos), len(Ow), _p(Ow), _p(Ow_ref), float(f32(sf_level)), float(f32(sf_last)), _p(out))
    return out[:3].copy(), out[3], out[4]


# ---------------------------------------------------------------------------------------------------------------------
# Scene
# ---------------------------------------------------------------------------------------------------------------------
class KF:
    def __init__(self, rng, n):
        from os1_amd.api import KP_DTYPE
        k = np.zeros(n, KP_DTYPE)
        k['x'], k['y'] = rng.uniform(1, 639, n).astype(f32), rng.uniform(1, 479, n).astype(f32)
        k['size'], k['angle'], k['class_id'] = 31, rng.uniform(0, 359, n).astype(f32), -1
        k['octave'] = rng.integers(0, NLEVELS, n)
        self.kps = k
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.oct = np.ascontiguousarray(k['octave'], np.int32)
        self.Ow = rng.uniform(-1.5, 1.5, 3).astype(f32)
        self.n = n


class Batch:
    """rows, offsets and the per-observation arrays of one refresh call, built from lists of (slot, keypoint, bad) tuples."""

    def __init__(self, rows, obs_lists, refs):
        self.rows = np.ascontiguousarray(rows, np.int32)
        self.offs = np.zeros(len(rows) + 1, np.int32)
        self.offs[1:] = np.cumsum([len(o) for o in obs_lists])
        flat = [t for o in obs_lists for t in o]
        self.kf = np.array([t[0] for t in flat] + [0], np.int32)[:len(flat)]
        self.kp = np.array([t[1] for t in flat] + [0], np.int32)[:len(flat)]
        self.fl = np.array([OBS_KF_BAD if t[2] else 0 for t in flat] + [0], np.uint8)[:len(flat)]
        self.ref_kf = np.ascontiguousarray([r[0] for r in refs], np.int32)
        self.ref_kp = np.ascontiguousarray([r[1] for r in refs], np.int32)
        self.obs_lists = obs_lists
        self.names = None

    def copy(self):
        b = Batch(self.rows.copy(), [list(o) for o in self.obs_lists], list(zip(self.ref_kf.tolist(), self.ref_kp.tolist())))
        b.names = self.names
        return b


N_SHAPES = (1, 2, 3, 63, 64, 65, 129)
NULL_SLOT = 0            # a keyframe slot whose frame is never handed over: only bad observations name it


def make_scene(seed=5):
    """(keyframes, table [64][64] uint8, batch).  The keyframes: slot NULL_SLOT is the one whose frame is withheld; enough slots
    that a MapPoint can have 129 observations in distinct keyframes, as std::map<KeyFrame*, size_t> implies."""
    rng = np.random.default_rng(seed)
    nkf = 132
    kfs = [KF(rng, int(n)) for n in rng.integers(64, 301, nkf)]
    table = np.zeros((CAPACITY, 64), np.uint8)
    tf = table.view(f32).reshape(CAPACITY, 16)
    tf[:, 0:3] = np.stack([rng.uniform(-4, 4, CAPACITY), rng.uniform(-3, 3, CAPACITY), rng.uniform(3, 9, CAPACITY)], 1).astype(f32)
    tf[:, 3:6] = rng.uniform(-1, 1, (CAPACITY, 3)).astype(f32)       # stale values the refresh must replace (or keep)
    tf[:, 6], tf[:, 7] = 0.5, 50.0
    table[:, 32:] = rng.integers(0, 256, (CAPACITY, 32), dtype=np.uint8)
    names, obs, refs = [], [], []

    def obs_in(slots, bad=()):
        return [(int(s), int(rng.integers(0, kfs[s].n)), s in bad) for s in slots]

    def add(name, o, ref=None):
        names.append(name)
        obs.append(o)
        if ref is None:
            good = [t for t in o if t[0] != NULL_SLOT]
            ref = (good[0][0], good[0][1]) if good else (1, 0)
        refs.append(ref)

    for n in N_SHAPES:
        add('n%d' % n, obs_in(1 + rng.choice(nkf - 1, n, replace=False)))
    o = obs_in(1 + rng.choice(nkf - 1, 9, replace=False))
    o[0] = (o[0][0], o[0][1], True)
    o[-1] = (o[-1][0], o[-1][1], True)
    add('bad_first_last', o, ref=(o[3][0], o[3][1]))
    add('all_bad', [(s, k, True) for s, k, _ in obs_in(1 + rng.choice(nkf - 1, 5, replace=False))])
    add('empty', [])
    # duplicate descriptors: keyframes 1..6 get the same row at keypoint 0 pairwise, so that two candidates tie on the median
    kfs[2].desc[0] = kfs[1].desc[0]
    kfs[4].desc[0] = kfs[3].desc[0]
    kfs[6].desc[0] = kfs[5].desc[0]
    add('duplicates', [(s, 0, False) for s in (1, 2, 3, 4, 5, 6)])
    add('all_equal', [(1, 0, False), (2, 0, False)])
    shared = obs_in([10, 11, 12, 13])
    add('shared_a', shared)
    add('shared_b', [(s, (k + 1) % kfs[s].n, False) for s, k, _ in shared])
    o = obs_in([20, 21, 22]) + [(NULL_SLOT, 5, True)]
    o.sort()                                                          # the NULL slot comes first in the list
    add('null_slot', o, ref=(20, o[1][1]))
    # a bad observation in a pass of its own past the 64 boundary, and 65 kept ones among 70
    o = obs_in(1 + rng.choice(nkf - 1, 70, replace=False))
    for i in (0, 13, 63, 64, 69):
        o[i] = (o[i][0], o[i][1], True)
    add('bad_across_passes', o, ref=(o[1][0], o[1][1]))
    # float corner cases (positions set below): |pos - Ow| = sqrt(3), whose reciprocal no float holds; and a component that
    # sums to the smallest negative denormal, halves to -0 and must come out as +0
    kfs[30].Ow = np.array([0, 1, 2], f32)
    kfs[31].Ow = np.array([np.float32(2.8e-45), 0, 0], f32)
    kfs[32].Ow = np.zeros(3, f32)
    add('sqrt3', obs_in([30]))
    add('neg_zero', obs_in([31, 32]))
    rows = rng.permutation(CAPACITY)[:len(obs)]
    tf[rows[names.index('sqrt3')], 0:3] = (1, 2, 3)
    tf[rows[names.index('neg_zero')], 0:3] = (0, 0, 2)
    b = Batch(rows, obs, refs)
    b.names = names
    return kfs, table, b


def ref_refresh(L, table, what, kfs, b, nlevels=NLEVELS, sf=SF):
    """The restatement on a copy of `table`: (new table, best, normal, min, max, return code)."""
    t = np.ascontiguousarray(table).copy()
    n = len(b.rows)
    dp = (C.c_void_p * len(kfs))(*[k.desc.ctypes.data for k in kfs])
    op = (C.c_void_p * len(kfs))(*[k.oct.ctypes.data for k in kfs])
    Ow = np.ascontiguousarray(np.stack([k.Ow for k in kfs]), f32)
    best = np.zeros(max(n, 1), np.int32)
    nrm = np.zeros((max(n, 1), 3), f32)
    mn, mx = np.zeros(max(n, 1), f32), np.zeros(max(n, 1), f32)
    sf = np.ascontiguousarray(sf, f32)
    rc = L.mpr_refresh_rows(_p(t), what, len(kfs), C.cast(dp, C.c_void_p), C.cast(op, C.c_void_p), _p(Ow), _p(sf), nlevels, n, _p(b.rows),
                            _p(b.offs), _p(b.kf), _p(b.kp), _p(b.fl), _p(b.ref_kf), _p(b.ref_kp), _p(best), _p(nrm), _p(mn), _p(mx))
    return t, best[:n], nrm[:n], mn[:n], mx[:n], rc


# ---------------------------------------------------------------------------------------------------------------------
# tests/cpp/map_point_refresh_test.cpp
# ---------------------------------------------------------------------------------------------------------------------
def _includes():
    return ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(CPP, 'mprefresh_stub')]


def syntax_check():
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only'] + _includes() +
                          [os.path.join(CPP, 'map_point_refresh_test.cpp')])


def compile_facade(out, host_backend):
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off'] + _includes() + \
          [os.path.join(CPP, 'map_point_refresh_test.cpp'), REF_SRC, '-o', out]
    if host_backend:
        cmd.insert(1, '-DMPR_HOST_BACKEND')
    else:
        from os1_amd import api
        if not os.path.exists(api.lib_path()):
            api.build_library()
        cmd += [api.lib_path(), '-Wl,-rpath,' + os.path.dirname(api.lib_path()), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run_facade(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'PASS', r.stdout[-3000:] + r.stderr[-2000:]
