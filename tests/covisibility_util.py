"""Shared by tests/test_covisibility.py and tests/test_gpu_covisibility.py: the ctypes binding of the restatement
tests/cpp/covisibility_ref.cpp (built here with g++), a second, independent count in numpy (np.add.at), the seeded cases of the
tests, and the builds of the stand-alone programs tests/cpp/covis_plan_test.cpp and tests/cpp/covisibility_test.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')
REF_SRC = os.path.join(CPP, 'covisibility_ref.cpp')
i32 = np.int32


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_ref(outdir, name='covisibility_ref.so'):
    so = os.path.join(str(outdir), name)
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC, '-o', so])
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    L.covis_ref_counts.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, C.POINTER(ci)]
    L.covis_ref_loop_ms.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp, vp, ci, C.POINTER(C.c_longlong)]
    L.covis_ref_loop_ms.restype = C.c_double
    return L


class Case:
    """The arrays of one orbfe_covisibility_counts call, from lists: observers[p] = slots observing MapPoint p, subjects[s] =
    (self, limit or None, [MapPoint index or -1, ...])."""

    def __init__(self, n_kf, observers, subjects, with_limit=None):
        self.n_kf = int(n_kf)
        self.obs_offsets = np.zeros(len(observers) + 1, i32)
        self.obs_offsets[1:] = np.cumsum([len(o) for o in observers])
        self.obs_kf = np.array([j for o in observers for j in o], i32)
        self.subj_self = np.array([s[0] for s in subjects], i32)
        self.subj_offsets = np.zeros(len(subjects) + 1, i32)
        self.subj_offsets[1:] = np.cumsum([len(s[2]) for s in subjects])
        self.subj_mp = np.array([p for s in subjects for p in s[2]], i32)
        if with_limit is None:
            with_limit = any(s[1] is not None for s in subjects)
        self.subj_limit = np.array([self.n_kf if s[1] is None else s[1] for s in subjects], i32) if with_limit else None

    @property
    def n_mp(self):
        return len(self.obs_offsets) - 1

    @property
    def n_subj(self):
        return len(self.subj_self)

    def with_limits(self, limits):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.subj_limit = None if limits is None else np.ascontiguousarray(limits, i32)
        return c

    def args(self):
        """positional arguments of os1_amd.api.covisibility_counts after the matcher"""
        return (self.n_kf, self.obs_offsets, self.obs_kf, self.subj_self, self.subj_offsets, self.subj_mp, self.subj_limit)


def ref_counts(L, c, cap=None):
    """(out_offsets, out_kf, out_count) of the restatement; with cap given: (rc, n_needed)."""
    room = max(1, c.n_subj * max(c.n_kf, 1)) if cap is None else max(cap, 1)
    offs = np.zeros(c.n_subj + 1, i32)
    kf, cnt = np.zeros(room, i32), np.zeros(room, i32)
    need = C.c_int(0)
    rc = L.covis_ref_counts(c.n_kf, c.n_mp, _p(c.obs_offsets), _p(c.obs_kf), c.n_subj, _p(c.subj_self), _p(c.subj_limit), _p(c.subj_offsets),
                            _p(c.subj_mp), _p(offs), _p(kf), _p(cnt), room if cap is None else cap, C.byref(need))
    if cap is not None:
        return rc, need.value
    assert rc == 0, rc
    return offs, kf[:need.value].copy(), cnt[:need.value].copy()


def np_counts(c):
    """The same three arrays from np.add.at over a dense counter per subject: a second, independent count."""
    offs, kfs, cnts = [0], [], []
    for s in range(c.n_subj):
        counter = np.zeros(max(c.n_kf, 1), np.int64)
        mp = c.subj_mp[c.subj_offsets[s]:c.subj_offsets[s + 1]]
        mp = mp[mp >= 0]
        if len(mp):
            j = np.concatenate([c.obs_kf[c.obs_offsets[p]:c.obs_offsets[p + 1]] for p in mp])
            limit = c.n_kf if c.subj_limit is None else c.subj_limit[s]
            j = j[(j != c.subj_self[s]) & (j < limit)]
            np.add.at(counter, j, 1)
        nz = np.flatnonzero(counter)
        kfs.append(nz.astype(i32))
        cnts.append(counter[nz].astype(i32))
        offs.append(offs[-1] + len(nz))
    return np.array(offs, i32), np.concatenate(kfs) if kfs else np.zeros(0, i32), np.concatenate(cnts) if cnts else np.zeros(0, i32)


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
def random_case(seed, n_kf, n_subj, n_mp=60, entries=(0, 90), max_obs=12, must=(), frames=0.25):
    """MapPoints observed by 0..max_obs distinct random slots (every slot of `must` that exists is observed by several of
    them); subjects of entries[0]..entries[1] entries, a tenth of them -1, some subjects Frames (self -1)."""
    rng = np.random.default_rng(seed)
    must = sorted({j for j in must if 0 <= j < n_kf})
    observers = []
    for p in range(n_mp):
        k = int(rng.integers(0, min(max_obs, n_kf) + 1))
        o = set(rng.choice(n_kf, k, replace=False).tolist())
        if must and p % 2 == 0:
            o.update(must[i] for i in range(len(must)) if (p >> 1) % (i + 2) != 1)
        observers.append(sorted(o))
    subjects = []
    for s in range(n_subj):
        n = int(rng.integers(entries[0], entries[1] + 1))
        mp = rng.integers(0, n_mp, n)
        mp[rng.random(n) < 0.1] = -1
        self_ = -1 if rng.random() < frames else (s % n_kf if s < 2 * n_kf else int(rng.integers(0, n_kf)))
        subjects.append((self_, None, mp.tolist()))
    return Case(n_kf, observers, subjects)


def special_case():
    """One call with the subjects the kernel can go wrong on; names[s] says which is which."""
    n_kf = 70
    observers = [[0, 3, 69], [], [5], [1, 2, 3, 4, 64, 65], list(range(70)), [7, 8]]      # MapPoint 1: no observation
    names = ['no_entries', 'all_skipped', 'zero_observations', 'only_itself', 'named_300_times', 'frame', 'plain', 'mixed']
    subjects = [(4, None, []),
                (4, None, [-1] * 37),
                (4, None, [1, 1, -1, 1]),
                (5, None, [2, 2, 2]),                       # observed by slot 5 only, and slot 5 is the subject: an empty segment
                (3, None, [3] * 300 + [0]),                 # counts of 300 (and 301 for nobody: slot 3 is the subject)
                (-1, None, [0, 3, 3, 5, -1, 4]),            # a Frame: nobody excluded
                (69, None, [0, 4, 5]),
                (64, None, [3, -1, 4, 4, 1, 2])]
    return Case(n_kf, observers, subjects), names


def small_map(seed=11, n_kf=40, entries=200):
    """A scene shaped like a small map: every keyframe has `entries` keypoint entries, most of them MapPoints observed by 2 to 12
    neighbouring keyframes.  Subjects are the keyframes, in slot order."""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(n_kf)]
    observers = []
    for _ in range(n_kf * entries):
        want, centre = int(rng.integers(2, 13)), int(rng.integers(0, n_kf))
        cand = [k for k in range(max(0, centre - 6), min(n_kf, centre + 7)) if len(lists[k]) < entries - 5]
        if len(cand) < 2:
            continue
        pick = sorted(rng.choice(cand, min(want, len(cand)), replace=False).tolist())
        for k in pick:
            lists[k].append(len(observers))
        observers.append(pick)
    subjects = []
    for k in range(n_kf):
        mp = lists[k] + [-1] * (entries - len(lists[k]))
        subjects.append((k, None, rng.permutation(mp).tolist()))
    return Case(n_kf, observers, subjects)


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone programs
# ---------------------------------------------------------------------------------------------------------------------
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def compile_plan_test(out, sanitize=True, src='covis_plan_test.cpp'):
    """os1_amd/csrc/covis_plan.h (or, with src given, another plan header's test) as a program of its own; the sanitizers, where
    asked for, linked into that program"""
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'os1_amd', 'csrc'), os.path.join(CPP, src), '-o', out]
    if sanitize:
        cmd[1:1] = SANITIZE
    subprocess.check_call(cmd)
    return out


def _includes():
    return ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(CPP, 'covis_stub')]


def syntax_check():
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only'] + _includes() + [os.path.join(CPP, 'covisibility_test.cpp')])


def compile_facade(out, host_backend, sanitize=False):
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + _includes() + [os.path.join(CPP, 'covisibility_test.cpp'), REF_SRC, '-o', out]
    if host_backend:
        cmd.insert(1, '-DCOVIS_HOST_BACKEND')
        if sanitize:
            cmd[1:1] = SANITIZE
    else:
        from os1_amd import api
        if not os.path.exists(api.lib_path()):
            api.build_library()
        cmd += [api.lib_path(), '-Wl,-rpath,' + os.path.dirname(api.lib_path()), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run(exe, timeout=120):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'PASS', r.stdout[-3000:] + r.stderr[-3000:]
