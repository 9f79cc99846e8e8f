"""Shared by tests/test_keyframe_culling.py, tests/test_gpu_keyframe_culling.py and tools/keyframe_culling_bench.py: the ctypes
binding of the restatement tests/cpp/keyframe_culling_ref.cpp (built here with g++), a second, independent count in numpy, the
cases of the tests, and the builds of the stand-alone programs under tests/cpp/."""
import ctypes as C
import os
import subprocess

import numpy as np

import covisibility_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')
REF_SRC = os.path.join(CPP, 'keyframe_culling_ref.cpp')
i32, u8 = np.int32, np.uint8
LONG = 64      # orbfe::kCullingLongList: a longer observation list goes to a whole wave


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_ref(outdir, name='keyframe_culling_ref.so'):
    so = os.path.join(str(outdir), name)
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC, '-o', so])
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    counts = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci]
    L.kfcull_ref_counts.argtypes = counts + [vp, vp]
    L.kfcull_ref_counts_structs.argtypes = counts + [vp, vp]
    L.kfcull_ref_loop_ms.argtypes = counts + [ci, C.POINTER(C.c_longlong)]
    L.kfcull_ref_loop_ms.restype = C.c_double
    L.kfcull_ref_writedown_ms.argtypes = counts[:-1] + [ci, C.POINTER(C.c_longlong)]
    L.kfcull_ref_writedown_ms.restype = C.c_double
    return L


class Case:
    """The arrays of one orbfe_redundant_observations call, from lists: observers[p] = [(slot, level), ...] of MapPoint p,
    subjects[s] = (self, [(MapPoint index or -1, level), ...]); nobs: None, or Observations() per MapPoint."""

    def __init__(self, n_kf, observers, subjects, nobs=None, th_obs=3):
        self.n_kf = int(n_kf)
        self.th_obs = int(th_obs)
        self.obs_offsets = np.zeros(len(observers) + 1, i32)
        self.obs_offsets[1:] = np.cumsum([len(o) for o in observers])
        self.obs_kf = np.array([j for o in observers for j, _ in o], i32)
        self.obs_level = np.array([v for o in observers for _, v in o], u8)
        self.subj_self = np.array([s[0] for s in subjects], i32)
        self.subj_offsets = np.zeros(len(subjects) + 1, i32)
        self.subj_offsets[1:] = np.cumsum([len(s[1]) for s in subjects])
        self.subj_mp = np.array([p for s in subjects for p, _ in s[1]], i32)
        self.subj_level = np.array([v for s in subjects for _, v in s[1]], u8)
        self.mp_nobs = None if nobs is None else np.array(nobs, i32)

    @property
    def n_mp(self):
        return len(self.obs_offsets) - 1

    @property
    def n_subj(self):
        return len(self.subj_self)

    def but(self, **change):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(change)
        return c

    def rebased(self, obs_pad=5, subj_pad=3):
        """the same call with both CSRs starting past junk the call must not read (slot and MapPoint numbers out of range)"""
        return self.but(obs_offsets=self.obs_offsets + obs_pad, obs_kf=np.concatenate([np.full(obs_pad, self.n_kf + 9, i32), self.obs_kf]),
                        obs_level=np.concatenate([np.zeros(obs_pad, u8), self.obs_level]), subj_offsets=self.subj_offsets + subj_pad,
                        subj_mp=np.concatenate([np.full(subj_pad, self.n_mp + 9, i32), self.subj_mp]),
                        subj_level=np.concatenate([np.zeros(subj_pad, u8), self.subj_level]))

    def args(self):
        """positional arguments of Matcher.redundant_observations"""
        return (self.n_kf, self.obs_offsets, self.obs_kf, self.obs_level, self.subj_self, self.subj_offsets, self.subj_mp, self.subj_level,
                self.th_obs, self.mp_nobs)


def _c_args(c):
    return (c.n_kf, c.n_mp, _p(c.obs_offsets), _p(c.obs_kf), _p(c.obs_level), _p(c.mp_nobs), c.n_subj, _p(c.subj_self), _p(c.subj_offsets),
            _p(c.subj_mp), _p(c.subj_level), c.th_obs)


def ref_counts(L, c, structs=False):
    """(n_mps, n_redundant) of the restatement, over the arrays or (structs) over std::map objects built from them."""
    a, b = np.zeros(max(c.n_subj, 1), i32), np.zeros(max(c.n_subj, 1), i32)
    rc = (L.kfcull_ref_counts_structs if structs else L.kfcull_ref_counts)(*_c_args(c), _p(a), _p(b))
    assert rc == 0, rc
    return a[:c.n_subj].copy(), b[:c.n_subj].copy()


def ref_loop_ms(L, c, reps):
    chk = C.c_longlong(0)
    ms = L.kfcull_ref_loop_ms(*_c_args(c), reps, C.byref(chk))
    assert ms >= 0
    return ms, chk.value


def ref_writedown_ms(L, c, reps):
    """(median ms, observations written) of the write-down of the call's arrays from std::map objects"""
    chk = C.c_longlong(0)
    ms = L.kfcull_ref_writedown_ms(*_c_args(c)[:-1], reps, C.byref(chk))
    assert ms >= 0
    return ms, chk.value


def np_counts(c):
    """The same two arrays without the early exit: per entry the full count of qualifying observers, compared with th_obs."""
    n_mps, n_red = np.zeros(c.n_subj, i32), np.zeros(c.n_subj, i32)
    for s in range(c.n_subj):
        for e in range(c.subj_offsets[s], c.subj_offsets[s + 1]):
            p = int(c.subj_mp[e])
            if p < 0:
                continue
            n_mps[s] += 1
            a, b = int(c.obs_offsets[p]), int(c.obs_offsets[p + 1])
            nobs = b - a if c.mp_nobs is None else int(c.mp_nobs[p])
            if nobs > c.th_obs:
                q = (c.obs_kf[a:b] != c.subj_self[s]) & (c.obs_level[a:b].astype(np.int64) <= int(c.subj_level[e]) + 1)
                n_red[s] += int(q.sum()) >= c.th_obs
    return n_mps, n_red


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
def crafted_case(th_obs=3):
    """One call with the MapPoints and subjects the kernel can go wrong on.  Returns (case, names, want): names[s] says what
    subject s is about, want[s] = (n_mps, n_redundant) worked out by hand, as a function of th_obs (1 or 3)."""
    t = th_obs
    n_kf = 400
    others = [j for j in range(1, n_kf)]           # slot 0 is the subject of most cases

    def run(n, level=0, first=None, last=None):
        """n observers at `level`, none of them slot 0, optionally with slot `first` in front / `last` at the end"""
        o = [(j, level) for j in others[:n]]
        if first is not None:
            o[0] = (first, level)
        if last is not None:
            o[-1] = (last, level)
        return o

    mp = {}
    observers = []

    def add(name, o):
        mp[name] = len(observers)
        observers.append(o)

    add('none', [])
    add('th', run(t))                              # Observations() == th_obs: never looked at
    add('th+1', run(t + 1))                        # looked at; th_obs + 1 others qualify
    add('th+1_self_first', run(t + 1, first=0))    # th_obs others: just enough
    add('th+1_self_last', run(t + 1, last=0))
    add('64', run(LONG))
    add('65', run(LONG + 1))
    add('300', run(300))
    add('64_self_last', run(LONG, last=0))
    add('65_self_first', run(LONG + 1, first=0))
    add('300_self_last', run(300, last=0))
    add('level+1', run(t + 1, level=6))            # seen from level 5: 6 <= 5 + 1 counts
    add('level+2', run(t + 1, level=7))            # seen from level 5: 7 > 6 does not
    add('level255', run(t + 1, level=255))
    add('level0', run(t + 1, level=0))
    add('exactly_th_with_self', [(0, 0)] + run(t - 1) + [(300 + k, 9) for k in range(3)])   # th_obs qualify, one is the subject
    add('exactly_th_others', [(0, 9)] + run(t) + [(300 + k, 9) for k in range(3)])
    add('65_two_qualify_late', [(j, 9) for j in others[:LONG - 1]] + [(399, 0), (398, 0)])   # long list, the qualifying ones in its last lanes
    add('300_th_qualify_spread', [(j, 0 if j in (1, 150, 299)[:t] else 9) for j in others[:300]])
    names, subjects, want = [], [], []

    def subj(name, self_, entries, n_mps, n_red):
        names.append(name)
        subjects.append((self_, entries))
        want.append((n_mps, n_red))

    E = lambda name, level=0: (mp[name], level)
    subj('no_entries', 0, [], 0, 0)
    subj('one_entry', 0, [E('th+1')], 1, 1)
    subj('all_skipped', 0, [(-1, 0)] * 37, 0, 0)
    subj('list_lengths', 0, [E('none'), E('th'), E('th+1'), E('64'), E('65'), E('300')], 6, 4)
    subj('self_first_last', 0, [E('th+1_self_first'), E('th+1_self_last'), E('64_self_last'), E('65_self_first'), E('300_self_last')], 5, 5)
    subj('self_absent', 399, [E('th+1_self_first'), E('th+1_self_last'), E('65_self_first')], 3, 3)
    subj('levels', 0, [E('level+1', 5), E('level+2', 5), E('level255', 254), E('level255', 253), E('level255', 255), E('level0', 0), E('level+2', 6)],
         7, 5)
    subj('exactly_th', 0, [E('exactly_th_with_self'), E('exactly_th_others')], 2, 1)
    subj('no_self', -1, [E('exactly_th_with_self'), E('th+1_self_first')], 2, 2)
    subj('named_twice', 0, [E('th+1'), E('th+1'), E('th'), E('th'), (-1, 0), E('300'), E('300')], 6, 4)
    subj('late_and_spread', 0, [E('65_two_qualify_late'), E('300_th_qualify_spread')], 2, (1 if t <= 2 else 0) + 1)
    # subject boundaries inside one wave: 10 + 7 + 64 entries
    subj('wave_a10', 0, [E('th+1')] * 5 + [E('th')] * 5, 10, 5)
    subj('wave_b7', 1, [E('65')] * 3 + [(-1, 0)] + [E('th+1')] * 3, 6, 6)     # slot 1 is among the observers: 64 / th_obs others are left
    subj('wave_c64', 0, [E('300'), E('none')] * 32, 64, 32)
    for n in (63, 64, 65, 130):
        subj('entries_%d' % n, 0, [E('th+1') if k % 3 else E('th') for k in range(n)], n, sum(1 for k in range(n) if k % 3))
    c = Case(n_kf, observers, subjects, th_obs=t)
    return c, names, want


def nobs_case():
    """mp_nobs that disagrees with the CSR: Observations() decides whether a MapPoint is looked at, the CSR what is counted.
    Returns (case, want)."""
    observers = [[(1, 0), (2, 0), (3, 0)],                    # three observers, Observations() says 4: looked at, and 3 qualify
                 [(1, 0), (2, 0), (3, 0), (4, 0)],            # four observers, Observations() says 3: not looked at
                 [],                                          # none, Observations() says 9: looked at, nothing to count
                 [(1, 0), (2, 0), (3, 0), (4, 0)]]            # agrees
    subjects = [(0, [(0, 0), (1, 0), (2, 0), (3, 0)])]
    return Case(5, observers, subjects, nobs=[4, 3, 9, 4]), [(4, 2)]


def random_map(seed=5, n_kf=40, entries=300, th_obs=3):
    """A scene shaped like a small map: every keyframe has `entries` keypoints, most of them MapPoints observed by 2 to 12
    neighbouring keyframes at levels 0..7 (a few MapPoints by up to 30).  Subjects are the keyframes, in slot order."""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(n_kf)]
    observers = []
    for _ in range(n_kf * entries):
        wide = rng.random() < 0.02
        want, centre = int(rng.integers(13, 31)) if wide else int(rng.integers(2, 13)), int(rng.integers(0, n_kf))
        reach = 20 if wide else 6
        cand = [k for k in range(max(0, centre - reach), min(n_kf, centre + reach + 1)) if len(lists[k]) < entries - 5]
        if len(cand) < 2:
            continue
        pick = sorted(rng.choice(cand, min(want, len(cand)), replace=False).tolist())
        base = int(rng.integers(0, 6))
        levels = np.clip(base + rng.integers(-2, 3, len(pick)), 0, 7).tolist()
        for k, v in zip(pick, levels):
            lists[k].append((len(observers), v))
        observers.append(list(zip(pick, levels)))
    subjects = []
    for k in range(n_kf):
        mp = lists[k] + [(-1, 0)] * (entries - len(lists[k]))
        subjects.append((k, [mp[i] for i in rng.permutation(len(mp))]))
    return Case(n_kf, observers, subjects, th_obs=th_obs)


def culling_job(seed=3, n_subj=100, entries=1000, obs=(2, 40)):
    """One KeyFrameCulling-sized job: n_subj local keyframes of `entries` MapPoint entries each, every MapPoint observed by
    obs[0]..obs[1] keyframes out of a neighbourhood of the map (the local keyframes and as many again around them)."""
    rng = np.random.default_rng(seed)
    n_kf = 2 * n_subj
    n_mp = n_subj * entries // 8                              # a MapPoint is seen from about 8 of the subjects on average
    counts = rng.integers(obs[0], obs[1] + 1, n_mp)
    observers, lists = [], [[] for _ in range(n_subj)]
    for p in range(n_mp):
        centre = int(rng.integers(0, n_kf))
        cand = np.arange(max(0, centre - 30), min(n_kf, centre + 31))
        pick = np.sort(rng.choice(cand, min(int(counts[p]), len(cand)), replace=False))
        base = int(rng.integers(0, 6))
        levels = np.clip(base + rng.integers(-2, 3, len(pick)), 0, 7)
        observers.append(list(zip(pick.tolist(), levels.tolist())))
        for k, v in zip(pick.tolist(), levels.tolist()):
            if k < n_subj and len(lists[k]) < entries:
                lists[k].append((p, v))
    subjects = [(k, lists[k] + [(-1, 0)] * (entries - len(lists[k]))) for k in range(n_subj)]
    return Case(n_kf, observers, subjects)


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone programs
# ---------------------------------------------------------------------------------------------------------------------
SANITIZE = covisibility_util.SANITIZE


def compile_plan_test(out, sanitize):
    """os1_amd/csrc/culling_plan.h as a program of its own; the sanitizers, where asked for, linked into that program"""
    return covisibility_util.compile_plan_test(out, sanitize, 'culling_plan_test.cpp')


def _includes():
    return ['-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(CPP, 'culling_stub')]


def syntax_check_call_site():
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-fsyntax-only'] + _includes() + [os.path.join(CPP, 'keyframe_culling_callsite.cpp')])


def compile_facade(out, gpu, sanitize=False):
    src = 'keyframe_culling_test.cpp' if gpu else 'keyframe_culling_facade_test.cpp'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror'] + _includes() + [os.path.join(CPP, src), REF_SRC, '-o', out]
    if gpu:
        from os1_amd import api
        if not os.path.exists(api.lib_path()):
            api.build_library()
        cmd += [api.lib_path(), '-Wl,-rpath,' + os.path.dirname(api.lib_path()), '-Wl,-rpath-link,/opt/rocm/lib']
    elif sanitize:
        cmd[1:1] = SANITIZE
    subprocess.check_call(cmd)
    return out


def run(exe, timeout=120):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'PASS', r.stdout[-3000:] + r.stderr[-3000:]
