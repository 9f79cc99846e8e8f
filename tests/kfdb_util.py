"""Shared by tests/test_kfdb.py and tests/test_gpu_kfdb.py: the seeded scenes of the keyframe database tests, the ctypes binding
of the reference restatement tests/cpp/kfdb_ref.cpp (built here with g++ -ffp-contract=off), a second, independent restatement
in pure Python (dict inverted file, Python floats = IEEE doubles, numpy float32 where the reference says float), and the
binary scene file tests/cpp/kfdb_test.cpp reads.

A scene is a list of model keyframes (mnId, BowVector, connected set, ordered covisibility list, bad flag) and a list of steps:
  ('add', kf) ('erase', kf) ('clear',) ('loop', kf, minScore or None = LoopClosing.cc:125-140's minimum) ('reloc', frame id, words, values)
plus the probe queries the C-ABI test sends after every mutation, and the pool capacities it creates the database with.
BowVector values are made the way TemplatedVocabulary::transform makes them: positive weights, L1-normalised by a division, so they
are no dyadic fractions and the order of a sum shows in its bits."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = os.path.join(ROOT, 'tests', 'cpp', 'kfdb_ref.cpp')
L1, L2, CHI, KL, BHATTA, DOT = range(6)
QUERY_LDS_WORDS = 4096          # the kernel's LDS budget for the query (os1_amd/csrc/orbfe_kfdb.hip kQueryLdsWords)
COUNTERS = ('candidates', 'duplicates', 'stale', 'connected_skips', 'best_other', 'unused', 'max_common', 'min_common')


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def build_ref(outdir):
    so = os.path.join(str(outdir), 'kfdb_ref.so')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-fPIC', '-shared', '-Wall', '-Werror', REF_SRC, '-o', so])
    L = C.CDLL(so)
    vp, ci, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.kref_create.argtypes = [ci, ci]
    L.kref_create.restype = vp
    L.kref_destroy.argtypes = [vp]
    L.kref_destroy.restype = None
    L.kref_new_kf.argtypes = [vp, u64, vp, vp, ci]
    L.kref_set_connected.argtypes = [vp, ci, vp, ci]
    L.kref_set_covisible.argtypes = [vp, ci, vp, ci]
    L.kref_set_bad.argtypes = [vp, ci, ci]
    for f in (L.kref_add, L.kref_erase):
        f.argtypes = [vp, ci]
        f.restype = None
    L.kref_clear.argtypes = [vp]
    L.kref_clear.restype = None
    L.kref_detect_loop.argtypes = [vp, ci, C.c_float, vp, ci]
    L.kref_detect_reloc.argtypes = [vp, u64, vp, vp, ci, vp, ci]
    L.kref_min_covisible_score.argtypes = [vp, ci]
    L.kref_min_covisible_score.restype = C.c_float
    L.kref_sharing.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci]
    L.kref_score.argtypes = [vp, vp, vp, ci, ci]
    L.kref_score.restype = C.c_double
    L.kref_members.argtypes = [vp, ci, vp, vp, vp]
    L.kref_members.restype = None
    L.kref_counters.argtypes = [vp, vp]
    L.kref_counters.restype = None
    return L


class Ref:
    """The C++ restatement loaded with a scene's keyframes."""

    def __init__(self, L, scene):
        self.L, self.scene = L, scene
        self.h = L.kref_create(scene['n_words'], scene['scoring'])
        for k in scene['kfs']:
            i = L.kref_new_kf(self.h, k['id'], _p(k['words']), _p(k['values']), len(k['words']))
            assert i == k['index']
        for k in scene['kfs']:
            conn = np.asarray(sorted(k['connected']), np.int32)
            cov = np.asarray(k['covisible'], np.int32)
            L.kref_set_connected(self.h, k['index'], _p(conn), len(conn))
            L.kref_set_covisible(self.h, k['index'], _p(cov), len(cov))
            L.kref_set_bad(self.h, k['index'], int(k['bad']))

    def close(self):
        if self.h:
            self.L.kref_destroy(self.h)
            self.h = None

    def step(self, st):
        """-> None for a mutation, the candidate list (keyframe indices) for a query"""
        L, cap = self.L, len(self.scene['kfs'])
        out = np.zeros(cap, np.int32)
        if st[0] == 'add':
            L.kref_add(self.h, st[1])
        elif st[0] == 'erase':
            L.kref_erase(self.h, st[1])
        elif st[0] == 'clear':
            L.kref_clear(self.h)
        elif st[0] == 'loop':
            ms = st[2] if st[2] is not None else self.min_covisible_score(st[1])
            n = L.kref_detect_loop(self.h, st[1], C.c_float(ms), _p(out), cap)
            return [int(v) for v in out[:n]]
        elif st[0] == 'reloc':
            n = L.kref_detect_reloc(self.h, st[1], _p(st[2]), _p(st[3]), len(st[2]), _p(out), cap)
            return [int(v) for v in out[:n]]
        return None

    def min_covisible_score(self, kf):
        return float(self.L.kref_min_covisible_score(self.h, kf))

    def sharing(self, words, values):
        cap = len(self.scene['kfs'])
        out, common, scores = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        n = self.L.kref_sharing(self.h, _p(words), _p(values), len(words), _p(out), _p(common), _p(scores), cap)
        return out[:n].copy(), common[:n].copy(), scores[:n].copy()

    def score(self, words, values, kf):
        return float(self.L.kref_score(self.h, _p(words), _p(values), len(words), kf))

    def members(self):
        """[(mnLoopQuery, mnLoopWords, mLoopScore bits, mnRelocQuery, mnRelocWords, mRelocScore bits)] of every keyframe"""
        res = []
        q, w, s = np.zeros(2, np.uint64), np.zeros(2, np.int32), np.zeros(2, np.float32)
        for k in self.scene['kfs']:
            self.L.kref_members(self.h, k['index'], _p(q), _p(w), _p(s))
            b = s.view(np.uint32)
            res.append((int(q[0]), int(w[0]), int(b[0]), int(q[1]), int(w[1]), int(b[1])))
        return res

    def counters(self):
        c = (C.c_long * 8)()
        self.L.kref_counters(self.h, c)
        return dict(zip(COUNTERS, [int(v) for v in c]))


# ---- the second restatement: pure Python ----------------------------------------------------------------------------------------
def py_score(scoring, v1, v2):
    """ScoringObject.cpp's scores on dict BowVectors: the common words in ascending order, one add at a time."""
    score = 0.0
    for w in sorted(set(v1) & set(v2)):
        vi, wi = v1[w], v2[w]
        if scoring == L1:
            score += abs(vi - wi) - abs(vi) - abs(wi)
        elif scoring == CHI:
            if vi + wi != 0.0:
                score += vi * wi / (vi + wi)
        else:
            score += vi * wi
    if scoring == L1:
        return -score / 2.0
    if scoring == L2:
        return 1.0 if score >= 1 else 1.0 - float(np.sqrt(np.float64(1.0 - score)))
    if scoring == CHI:
        return 2. * score
    return score


def py_score_pairwise(v1, v2):
    """The L1 score with its sum taken as a balanced tree (what a butterfly reduction computes): NOT the reference's order."""
    t = [abs(v1[w] - v2[w]) - abs(v1[w]) - abs(v2[w]) for w in sorted(set(v1) & set(v2))]
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return -(t[0] if t else 0.0) / 2.0


class PyKF:
    def __init__(self, k):
        self.index, self.mnId = k['index'], k['id']
        self.bow = dict(zip((int(w) for w in k['words']), (float(v) for v in k['values'])))
        self.words = [int(w) for w in k['words']]
        self.mnLoopQuery = self.mnLoopWords = self.mnRelocQuery = self.mnRelocWords = 0
        self.mLoopScore = self.mRelocScore = np.float32(0)
        self.bad = k['bad']


class PyRef:
    def __init__(self, scene):
        self.scene, self.scoring = scene, scene['scoring']
        self.kfs = [PyKF(k) for k in scene['kfs']]
        for k, m in zip(scene['kfs'], self.kfs):
            m.connected = {self.kfs[i] for i in k['connected']}
            m.covisible = [self.kfs[i] for i in k['covisible']]
        self.inv = {}

    def step(self, st):
        if st[0] == 'add':
            for w in self.kfs[st[1]].words:
                self.inv.setdefault(w, []).append(self.kfs[st[1]])
        elif st[0] == 'erase':
            for w in self.kfs[st[1]].words:
                lst = self.inv.get(w, [])
                if self.kfs[st[1]] in lst:
                    lst.remove(self.kfs[st[1]])      # the first one, the rest keep their order
        elif st[0] == 'clear':
            self.inv = {}
        elif st[0] == 'loop':
            ms = st[2] if st[2] is not None else self.min_covisible_score(st[1])
            return [k.index for k in self.detect_loop(self.kfs[st[1]], np.float32(ms))]
        elif st[0] == 'reloc':
            bow = dict(zip((int(w) for w in st[2]), (float(v) for v in st[3])))
            return [k.index for k in self.detect_reloc(st[1], bow)]
        return None

    def min_covisible_score(self, kf):
        cur, m = self.kfs[kf], np.float32(1)
        for k in cur.covisible:
            if k.bad:
                continue
            s = np.float32(py_score(self.scoring, cur.bow, k.bow))
            if s < m:
                m = s
        return float(m)

    def sharing(self, bow):
        order, words = [], {}
        for w in sorted(bow):
            for k in self.inv.get(w, []):
                if k not in words:
                    words[k] = 0
                    order.append(k)
                words[k] += 1
        return [k.index for k in order], [words[k] for k in order], [py_score(self.scoring, bow, k.bow) for k in order]

    def first_common_and_seq(self, bow, add_seq):
        """the sort-key claim: (first common word, add order) of every keyframe in any list of a query word"""
        keys = {}
        for w in sorted(bow):
            for k in self.inv.get(w, []):
                keys.setdefault(k.index, (w, add_seq[k.index]))
        return [i for i, _ in sorted(keys.items(), key=lambda e: e[1])]

    @staticmethod
    def _select(lScoreAndMatch, qid, query_attr, words_attr, score_attr, min_common, best0):
        lAcc, best_acc = [], np.float32(best0)
        for si, k in lScoreAndMatch:
            best_score, acc, best_kf = si, si, k
            for k2 in k.covisible[:10]:
                if getattr(k2, query_attr) != qid:
                    continue
                if min_common is not None and not getattr(k2, words_attr) > min_common:
                    continue
                acc = np.float32(acc + getattr(k2, score_attr))
                if getattr(k2, score_attr) > best_score:
                    best_kf, best_score = k2, getattr(k2, score_attr)
            lAcc.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = np.float32(np.float32(0.75) * best_acc)
        out = []
        for acc, k in lAcc:
            if acc > retain and k not in out:
                out.append(k)
        return out

    def detect_loop(self, q, min_score):
        lst = []
        for w in q.words:
            for k in self.inv.get(w, []):
                if k.mnLoopQuery != q.mnId:
                    k.mnLoopWords = 0
                    if k not in q.connected:
                        k.mnLoopQuery = q.mnId
                        lst.append(k)
                k.mnLoopWords += 1
        if not lst:
            return []
        max_common = max(k.mnLoopWords for k in lst)
        min_common = int(np.float32(max_common) * np.float32(0.8))
        sm = []
        for k in lst:
            if k.mnLoopWords > min_common:
                si = np.float32(py_score(self.scoring, q.bow, k.bow))
                k.mLoopScore = si
                if si >= min_score:
                    sm.append((si, k))
        if not sm:
            return []
        return self._select(sm, q.mnId, 'mnLoopQuery', 'mnLoopWords', 'mLoopScore', min_common, min_score)

    def detect_reloc(self, fid, bow):
        lst = []
        for w in sorted(bow):
            for k in self.inv.get(w, []):
                if k.mnRelocQuery != fid:
                    k.mnRelocWords = 0
                    k.mnRelocQuery = fid
                    lst.append(k)
                k.mnRelocWords += 1
        if not lst:
            return []
        max_common = max(k.mnRelocWords for k in lst)
        min_common = int(np.float32(max_common) * np.float32(0.8))
        sm = []
        for k in lst:
            if k.mnRelocWords > min_common:
                si = np.float32(py_score(self.scoring, bow, k.bow))
                k.mRelocScore = si
                sm.append((si, k))
        if not sm:
            return []
        return self._select(sm, fid, 'mnRelocQuery', 'mnRelocWords', 'mRelocScore', None, 0)

    def members(self):
        f = lambda x: int(np.float32(x).view(np.uint32))
        return [(k.mnLoopQuery, k.mnLoopWords, f(k.mLoopScore), k.mnRelocQuery, k.mnRelocWords, f(k.mRelocScore)) for k in self.kfs]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def values_for(rng, n):
    """positive, L1-normalised by a division: what transform + BowVector::normalize leave"""
    w = rng.uniform(0.2, 9.0, n) * rng.integers(1, 4, n)
    return w / np.sum(w)


def _vec(rng, words):
    words = np.asarray(sorted(set(int(w) for w in words)), np.uint32)
    return words, values_for(rng, len(words))


class _Builder:
    def __init__(self, n_words, scoring, seed):
        self.rng = np.random.default_rng(seed)
        self.scene = dict(n_words=n_words, scoring=scoring, kfs=[], steps=[], probes=[], seed=seed)

    def kf(self, words, values=None, mnId=None):
        if values is None:
            words = np.asarray(sorted(set(int(w) for w in words)), np.uint32)
            values = values_for(self.rng, len(words))
        else:                                   # given values follow their words; normalised again after any scaling
            order = np.argsort(np.asarray(words))
            words = np.asarray(words)[order].astype(np.uint32)
            values = np.asarray(values, np.float64)[order]
            values = values / np.sum(values)
            assert len(set(words.tolist())) == len(words)
        i = len(self.scene['kfs'])
        self.scene['kfs'].append(dict(index=i, id=100 + i if mnId is None else mnId, words=words, values=values, connected=set(),
                                      covisible=[], bad=False))
        return i

    def pick(self, pool, n):
        return self.rng.choice(np.asarray(pool), n, replace=False)

    def step(self, *st):
        self.scene['steps'].append(tuple(st))


def finish(scene, cap_slack_kf=0):
    """Pool capacities from a replay of the steps with the pool's own arithmetic (orbfe.h, keyframe database section): entries are
    appended behind the last keyframe; erased ones stay as tombstones until an add does not fit behind the tail, which compacts.
    capacity_entries is chosen so that compaction is needed where the scene wants it; the counters say what occurs."""
    kfs = scene['kfs']
    live, peak_k, peak_e = {}, 0, 0
    for st in scene['steps']:
        if st[0] == 'add':
            live[st[1]] = len(kfs[st[1]]['words'])
        elif st[0] == 'erase':
            live.pop(st[1], None)
        elif st[0] == 'clear':
            live = {}
        peak_k, peak_e = max(peak_k, len(live)), max(peak_e, sum(live.values()))
    scene['cap_k'], scene['cap_e'] = peak_k + cap_slack_kf, peak_e
    live, tail, compactions, readds, seen, clears_reused = {}, 0, 0, 0, set(), 0
    cleared = False
    for st in scene['steps']:
        if st[0] == 'add':
            n = len(kfs[st[1]]['words'])
            if tail + n > scene['cap_e']:
                compactions += 1
                tail = sum(live.values())
            assert tail + n <= scene['cap_e']
            tail += n
            live[st[1]] = n
            readds += st[1] in seen
            seen.add(st[1])
            clears_reused += cleared
            cleared = False
        elif st[0] == 'erase':
            live.pop(st[1], None)
        elif st[0] == 'clear':
            live, tail, cleared = {}, 0, True
    scene['expect'] = dict(compactions=compactions, readds=readds, clears_reused=clears_reused)
    return scene


def main_scene(seed=7, scoring=L1, n_random=40):
    """n_words 5 000, about 60 keyframes; every shape of the list in tests/test_kfdb.py's docstring but the maxCommonWords ones."""
    B = _Builder(5000, scoring, seed)
    rng = B.rng
    allw = np.arange(5000)
    qw = np.sort(B.pick(allw, 400))
    rest = np.setdiff1d(allw, qw)
    qv = values_for(rng, 400)
    Q = (qw.astype(np.uint32), qv)
    k_ident = B.kf(qw, qv)                                                     # identical to the query: score 1 up to rounding
    k_zero = B.kf(B.pick(rest, 120))                                           # no common word
    k_one = B.kf(np.concatenate([B.pick(rest, 90), qw[200:201]]))              # exactly one
    sized = [B.kf(np.concatenate([B.pick(rest, n - c), B.pick(qw[1:], c)])) for n, c in ((63, 20), (64, 64), (65, 30), (130, 100))]
    near = qv * rng.uniform(0.97, 1.03, 400)
    k_big = B.kf(np.concatenate([qw[:350], B.pick(rest, 60)]), np.concatenate([near[:350] * 0.9, values_for(rng, 60) * 0.1]))
    k_p1 = B.kf(np.concatenate([B.pick(qw[1:], 340), B.pick(rest, 80)]))
    k_p2 = B.kf(np.concatenate([B.pick(qw[1:], 330), B.pick(rest, 90)]))
    ties = [B.kf(np.concatenate([qw[:1], B.pick(qw[1:], 10 + 5 * i), B.pick(rest, 50)])) for i in range(3)]   # first common word: qw[0]
    own = B.pick(rest, 300)
    k_b = B.kf(own)                                                            # the second relocalisation query is about this one
    rnd = []
    for _ in range(n_random):
        c = int(rng.integers(0, 60))
        rnd.append(B.kf(np.concatenate([B.pick(qw, c), B.pick(rest, int(rng.integers(40, 200)))])))
    k_never = B.kf(np.concatenate([B.pick(qw, 50), B.pick(rest, 50)]))         # never added: a visitor of the covisible-score helper
    kfs = B.scene['kfs']
    # the loop query's keyframe: the query's words with other values; connected to the first keyframe of every list and one more
    k_loop = B.kf(qw, qv * rng.uniform(0.8, 1.25, 400), mnId=77)
    kfs[k_loop]['connected'] = {k_ident, ties[1], rnd[0]}
    kfs[k_loop]['covisible'] = [sized[3], rnd[1], k_never, rnd[2]]
    kfs[rnd[1]]['bad'] = True
    # covisibility that makes pBestKF another keyframe, twice the same one: duplicates
    kfs[k_p1]['covisible'] = [k_big, rnd[3]]
    kfs[k_p2]['covisible'] = [rnd[4], k_big, k_ident]
    kfs[k_big]['covisible'] = [k_p1]
    kfs[k_b]['covisible'] = [k_big, rnd[5]]
    # second relocalisation frame: k_b's words and three words that only k_big shares with it
    extra = np.setdiff1d(kfs[k_big]['words'], qw)[:3]
    Q2 = _vec(rng, np.concatenate([own, extra]))
    Q1w = (qw[7:8].astype(np.uint32), np.ones(1))                               # a query with one word
    B.scene['probes'] = [Q, Q1w, Q2]
    first = [k_ident, k_zero, k_one] + sized + [k_big, k_p1, k_p2] + ties + [k_b] + rnd[:10]
    for k in first:
        B.step('add', k)
    B.step('reloc', 1, Q[0], Q[1])
    B.step('reloc', 2, Q2[0], Q2[1])                                           # k_big: listed, not scored, its score of frame 1 is used
    B.step('loop', k_loop, None)
    B.step('erase', ties[0])
    B.step('add', ties[0])                                                     # back of every list: the tie order changes
    B.step('reloc', 3, Q[0], Q[1])
    for k in rnd[:10]:
        B.step('erase', k)                                                     # tombstones ...
    for k in rnd[10:]:
        B.step('add', k)                                                       # ... that the pool needs back: compaction
    B.step('loop', k_loop, np.float32(0.01))
    B.step('reloc', 3, Q[0], Q[1])                                             # the same frame id again: nobody is reset or listed
    B.step('erase', k_ident)
    B.step('erase', k_never)                                                   # not in the database
    B.step('reloc', 4, Q1w[0], Q1w[1])
    B.step('loop', k_loop, np.float32(0.0))
    B.step('clear')
    for k in [k_big, k_ident, ties[2], ties[0], k_p1]:
        B.step('add', k)                                                       # reuse after clear
    B.step('reloc', 5, Q[0], Q[1])
    B.scene['named'] = dict(ident=k_ident, zero=k_zero, one=k_one, sized=sized, big=k_big, ties=ties, loop=k_loop, never=k_never)
    return finish(B.scene)


def max_common_scene(maxc, seed=3):
    """maxCommonWords = maxc (5 or 10): maxc * 0.8f is an integer, and the keyframe with exactly that many common words is NOT scored."""
    B = _Builder(5000, L1, seed)
    rng = B.rng
    allw = np.arange(5000)
    qw = np.sort(B.pick(allw, 12))
    rest = np.setdiff1d(allw, qw)
    Q = (qw.astype(np.uint32), values_for(rng, 12))
    minc = int(np.float32(maxc) * np.float32(0.8))
    ks = [B.kf(np.concatenate([qw[:c], B.pick(rest, 30)])) for c in (maxc, minc, minc + 1, 1)]
    k_loop = B.kf(qw, values_for(rng, 12), mnId=9)
    B.scene['probes'] = [Q]
    for k in ks:
        B.step('add', k)
    B.step('reloc', 1, Q[0], Q[1])
    B.step('loop', k_loop, np.float32(0.0))
    B.scene['named'] = dict(at_min=ks[1], above_min=ks[2], maxc=maxc, minc=minc)
    return finish(B.scene)


def large_query_scene(seed=11):
    """n_words 50 000 and a query one word above the kernel's LDS budget (the route that reads the query from global memory), with a
    second query at the budget."""
    B = _Builder(50000, L1, seed)
    rng = B.rng
    allw = np.arange(50000)
    qw = np.sort(B.pick(allw, QUERY_LDS_WORDS + 1))
    rest = np.setdiff1d(allw, qw)
    Q = (qw.astype(np.uint32), values_for(rng, len(qw)))
    Qfit = (Q[0][:QUERY_LDS_WORDS].copy(), values_for(rng, QUERY_LDS_WORDS))
    ks = [B.kf(np.concatenate([B.pick(qw, int(rng.integers(0, 300))), B.pick(rest, int(rng.integers(50, 400)))])) for _ in range(38)]
    ks.append(B.kf(np.concatenate([qw[-1:], B.pick(rest, 70)])))               # shares only the query's last word
    ks.append(B.kf(qw[::2]))
    B.scene['probes'] = [Q, Qfit]
    for k in ks:
        B.step('add', k)
    B.step('erase', ks[3])
    B.step('reloc', 1, Q[0], Q[1])
    B.scene['named'] = {}
    return finish(B.scene)


def all_scenes():
    sc = {'main': main_scene(), 'max5': max_common_scene(5), 'max10': max_common_scene(10), 'large': large_query_scene()}
    for name, s in (('l2', L2), ('chi', CHI), ('dot', DOT)):
        sc[name] = main_scene(seed=21 + s, scoring=s, n_random=14)
    return sc


_SCENES = None


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = all_scenes()
    return _SCENES


def write_scene(scene, path):
    """The binary file tests/cpp/kfdb_test.cpp reads (little endian)."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<6i', scene['n_words'], scene['scoring'], len(scene['kfs']), len(scene['steps']), scene['cap_k'], scene['cap_e']))
        for k in scene['kfs']:
            conn, cov = sorted(k['connected']), k['covisible']
            f.write(struct.pack('<Q4i', k['id'], len(k['words']), len(conn), len(cov), int(k['bad'])))
            f.write(k['words'].astype('<u4').tobytes() + k['values'].astype('<f8').tobytes())
            f.write(np.asarray(conn, '<i4').tobytes() + np.asarray(cov, '<i4').tobytes())
        code = dict(add=0, erase=1, clear=2, loop=3, reloc=4)
        for st in scene['steps']:
            kf, fid, ms, has_ms, w, v = -1, 0, 0.0, 0, np.zeros(0, np.uint32), np.zeros(0)
            if st[0] in ('add', 'erase'):
                kf = st[1]
            elif st[0] == 'loop':
                kf, has_ms = st[1], int(st[2] is not None)
                ms = float(st[2]) if has_ms else 0.0
            elif st[0] == 'reloc':
                fid, w, v = st[1], st[2], st[3]
            f.write(struct.pack('<2iQfi i', code[st[0]], kf, fid, ms, has_ms, len(w)))
            f.write(np.asarray(w, '<u4').tobytes() + np.asarray(v, '<f8').tobytes())
