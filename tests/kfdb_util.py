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


# the comparisons PyRef can get wrong on purpose
FLIPS = frozenset(['minc_ge', 'minc_round', 'si_gt', 'retain_ge', 'retain_double', 'loop_best0', 'best_ge', 'neigh11', 'acc_reorder',
                   'loop_neigh_no_minc', 'reloc_neigh_minc', 'loop_neigh_no_query', 'ignore_query_id', 'connected_first', 'no_dedup',
                   'order_by_index'])


class PyKF:
    def __init__(self, k):
        self.index, self.mnId = k['index'], k['id']
        self.bow = dict(zip((int(w) for w in k['words']), (float(v) for v in k['values'])))
        self.words = [int(w) for w in k['words']]
        self.mnLoopQuery = self.mnLoopWords = self.mnRelocQuery = self.mnRelocWords = 0
        self.mLoopScore = self.mRelocScore = np.float32(0)
        self.bad = k['bad']


class PyRef:
    """flip: names of comparisons to get WRONG on purpose (FLIPS below).  The crafted scenes' witnesses: a scene built for a boundary
    must change its result when that boundary's comparison is flipped."""

    def __init__(self, scene, flip=()):
        self.scene, self.scoring = scene, scene['scoring']
        self.flip = frozenset(flip)
        assert self.flip <= FLIPS, self.flip - FLIPS
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

    def _min_common(self, max_common):
        x = np.float32(max_common) * np.float32(0.8)
        return int(np.rint(x)) if 'minc_round' in self.flip else int(x)

    def _above(self, words, min_common):
        return words >= min_common if 'minc_ge' in self.flip else words > min_common

    def _select(self, lScoreAndMatch, qid, query_attr, words_attr, score_attr, min_common, best0):
        flip = self.flip
        lAcc, best_acc = [], np.float32(best0)
        for si, k in lScoreAndMatch:
            best_score, acc, best_kf = si, si, k
            used = []
            for k2 in k.covisible[:11 if 'neigh11' in flip else 10]:
                if getattr(k2, query_attr) != qid and not (min_common is not None and 'loop_neigh_no_query' in flip):
                    continue
                if min_common is not None and 'loop_neigh_no_minc' not in flip and not getattr(k2, words_attr) > min_common:
                    continue
                if min_common is None and 'reloc_neigh_minc' in flip and not getattr(k2, words_attr) > self._reloc_min_common:
                    continue
                acc = np.float32(acc + getattr(k2, score_attr))
                used.append(getattr(k2, score_attr))
                if getattr(k2, score_attr) >= best_score if 'best_ge' in flip else getattr(k2, score_attr) > best_score:
                    best_kf, best_score = k2, getattr(k2, score_attr)
            if 'acc_reorder' in flip and used:      # the neighbours first, the keyframe's own score last
                acc = used[0]
                for s2 in used[1:]:
                    acc = np.float32(acc + s2)
                acc = np.float32(acc + si)
            lAcc.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = 0.75 * float(best_acc) if 'retain_double' in flip else np.float32(np.float32(0.75) * best_acc)
        out = []
        for acc, k in lAcc:
            if (acc >= retain if 'retain_ge' in flip else float(acc) > float(retain)) and (k not in out or 'no_dedup' in flip):
                out.append(k)
        if 'order_by_index' in flip:
            out.sort(key=lambda k: k.index)
        return out

    def detect_loop(self, q, min_score):
        lst = []
        for w in q.words:
            for k in self.inv.get(w, []):
                if 'connected_first' in self.flip and k in q.connected:
                    k.mnLoopWords = 1
                    continue
                if k.mnLoopQuery != q.mnId or ('ignore_query_id' in self.flip and k not in lst):
                    k.mnLoopWords = 0
                    if k not in q.connected:
                        k.mnLoopQuery = q.mnId
                        lst.append(k)
                k.mnLoopWords += 1
        if not lst:
            return []
        max_common = max(k.mnLoopWords for k in lst)
        min_common = self._min_common(max_common)
        sm = []
        for k in lst:
            if self._above(k.mnLoopWords, min_common):
                si = np.float32(py_score(self.scoring, q.bow, k.bow))
                k.mLoopScore = si
                if si > min_score if 'si_gt' in self.flip else si >= min_score:
                    sm.append((si, k))
        if not sm:
            return []
        return self._select(sm, q.mnId, 'mnLoopQuery', 'mnLoopWords', 'mLoopScore', min_common, 0 if 'loop_best0' in self.flip else min_score)

    def detect_reloc(self, fid, bow):
        lst = []
        for w in sorted(bow):
            for k in self.inv.get(w, []):
                if k.mnRelocQuery != fid or ('ignore_query_id' in self.flip and k not in lst):
                    k.mnRelocWords = 0
                    k.mnRelocQuery = fid
                    lst.append(k)
                k.mnRelocWords += 1
        if not lst:
            return []
        max_common = max(k.mnRelocWords for k in lst)
        min_common = self._reloc_min_common = self._min_common(max_common)
        sm = []
        for k in lst:
            if self._above(k.mnRelocWords, min_common):
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


# ---- crafted decision-boundary scenes -------------------------------------------------------------------------------------------
# One scene per comparison of KeyFrameDatabase.cc.  Scores are exact, hand-chosen floats: with L1 scoring and positive values the score
# of two vectors is the sum over their common words of the smaller value, so a query whose words all carry 1.0 scores a keyframe with
# the sum of the keyframe's values on the common words.  Those values are dyadic and NOT normalised (orbfe_kfdb_add takes values as
# given), every partial sum is exact in double and the total is a float.  Each scene carries
#   scene['literal']   the expected result of every query step, in step order, written from the reference text, and
#   scene['witness']   names of FLIPS: PyRef with that comparison flipped must NOT reproduce the scene (results or members).
EPS = 2.0 ** -20
F32 = np.float32
N_WORDS_CRAFTED = 1000


def ulps(x, n):
    """the float n ulps above (n < 0: below) the float x"""
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf if n > 0 else -np.inf), dtype=F32)
    return x


class _Crafted(_Builder):
    def __init__(self, nq, scoring=L1):
        super().__init__(N_WORDS_CRAFTED, scoring, 0)
        self.q = list(range(10, 10 + nq))                 # the query's words, 1.0 each
        self.fill = 500                                   # words no query has
        self.scene['literal'], self.scene['witness'] = [], []

    def raw(self, words, values, mnId=None):
        i = len(self.scene['kfs'])
        assert list(words) == sorted(set(words)) and len(words) == len(values) <= 64
        self.scene['kfs'].append(dict(index=i, id=100 + i if mnId is None else mnId, words=np.asarray(words, np.uint32),
                                      values=np.asarray(values, np.float64), connected=set(), covisible=[], bad=False))
        return i

    def fillers(self, n, value=0.5):
        w = list(range(self.fill, self.fill + n))
        self.fill += n
        return w, [value] * n

    def shares(self, score, common, nfill=3, fill_value=0.5):
        """a keyframe whose L1 score with the query is exactly the float `score`, sharing the query words q[i], i in `common`"""
        common = sorted(self.q[i] for i in common)
        c = len(common)
        assert F32(score) == score and score - (c - 1) * EPS > 0
        fw, fv = self.fillers(nfill, fill_value)
        return self.raw(common + fw, [float(score) - (c - 1) * EPS] + [EPS] * (c - 1) + fv)

    def query_kf(self, mnId, connected=()):
        k = self.raw(self.q, [1.0] * len(self.q), mnId)
        self.scene['kfs'][k]['connected'] = set(connected)
        return k

    def cov(self, k, others):
        self.scene['kfs'][k]['covisible'] = list(others)

    def adds(self, *ks):
        for k in ks:
            self.step('add', k)

    def reloc(self, fid, literal, words=None, values=None):
        w = np.asarray(self.q if words is None else words, np.uint32)
        v = np.ones(len(w)) if values is None else np.asarray(values, np.float64)
        self.step('reloc', fid, w, v)
        self.scene['literal'].append(list(literal))

    def loop(self, kf, min_score, literal):
        self.step('loop', kf, F32(min_score))
        self.scene['literal'].append(list(literal))

    def done(self, witness, **named):
        self.scene['witness'] = list(witness)
        self.scene['named'] = named
        self.scene['probes'] = [(np.asarray(self.q, np.uint32), np.ones(len(self.q)))]
        sc = finish(self.scene)
        assert len(sc['kfs']) <= 32 and all(len(k['words']) <= 64 for k in sc['kfs'])
        return sc


def crafted_min_common(maxc):
    """A. maxCommonWords = maxc: keyframes with exactly minc, minc + 1 and maxc common words (where those differ and are > 0), each
    common word worth 1/64.  `> minCommonWords` is strict: the one with minc is listed and never scored."""
    B = _Crafted(maxc + 2)
    minc = (4 * maxc) // 5                                # int(maxc * 0.8f), asserted in tests/test_os1_kfdb_ref.py
    counts = [c for c in (minc + 1, minc) if 0 < c < maxc] + [maxc]
    ks = {}
    for c in counts:                                      # added in this order: it is the order of every list they share
        fw, fv = B.fillers(2)
        ks[c] = B.raw(B.q[:c] + fw, [1.0 / 64] * c + fv)
    ql = B.query_kf(9)
    B.adds(*ks.values())
    lit = [ks[c] for c in counts if c > minc]             # (minc + 1) / 64 > 0.75f * maxc / 64 for every maxc
    B.reloc(1, lit)
    B.loop(ql, 0.0, lit)
    frac = (4 * maxc) % 5
    witness = (['minc_ge'] if minc > 0 else []) + (['minc_round'] if frac >= 3 else [])
    return B.done(witness, maxc=maxc, minc=minc, at_min=ks.get(minc), above_min=ks.get(minc + 1), at_max=ks[maxc])


def crafted_min_score():
    """B. si >= minScore: minScore equal to a keyframe's float score, one ulp above, one ulp below (three query keyframes with their own
    ids: a repeated id would find every member stale)."""
    B = _Crafted(4)
    s = F32(0.3)
    k = B.shares(s, (0, 1))
    low = B.shares(F32(0.125), (0, 2))
    q1, q2, q3 = B.query_kf(201), B.query_kf(202), B.query_kf(203)
    B.adds(k, low)
    B.loop(q1, s, [k])
    B.loop(q2, ulps(s, 1), [])
    B.loop(q3, ulps(s, -1), [k])
    return B.done(['si_gt'], k=k, s=s)


def crafted_retain():
    """C. accScore > 0.75f * bestAccScore: 0.75f * 0.5 = 0.375 exactly; keyframes at 0.375 and one ulp either side."""
    B = _Crafted(6)
    best, eq, up, dn = B.shares(0.5, (0,)), B.shares(0.375, (1,)), B.shares(ulps(0.375, 1), (2,)), B.shares(ulps(0.375, -1), (3,))
    ql = B.query_kf(9)
    B.adds(best, eq, up, dn)
    B.reloc(1, [best, up])
    B.loop(ql, 0.0, [best, up])
    return B.done(['retain_ge'], eq=eq)


def crafted_retain_rounds():
    """C. the float product rounds: best = 0.5 + 2^-24, 0.75 * best = 0.375 + 1.5 ulp, a tie that rounds to even: 0.375 + 2 ulp.  The
    keyframe AT 0.375 + 2 ulp is not above it (it would be above the unrounded product); the one at + 3 ulp is."""
    B = _Crafted(6)
    best, at, above = B.shares(ulps(0.5, 1), (0,)), B.shares(ulps(0.375, 2), (1,)), B.shares(ulps(0.375, 3), (2,))
    assert F32(0.75) * ulps(0.5, 1) == ulps(0.375, 2) and 0.75 * float(ulps(0.5, 1)) < float(ulps(0.375, 2))
    ql = B.query_kf(9)
    B.adds(best, at, above)
    B.reloc(1, [best, above])
    B.loop(ql, 0.0, [best, above])
    return B.done(['retain_double'], at=at)


def crafted_best_start():
    """C. bestAccScore starts at minScore in the loop search and at 0 in relocalisation.  Dot-product scoring with one negative value:
    k1 scores 0.5 and its neighbour k2 -0.25, so k1 accumulates 0.25, BELOW minScore = 0.5.  Loop: best stays 0.5, 0.25 is not above
    0.375, nothing returns.  Relocalisation on the same vectors: best is 0.25 and k1 returns."""
    B = _Crafted(2, scoring=DOT)
    fw, fv = B.fillers(2)
    k1 = B.raw(B.q[:1] + fw, [0.5] + fv)
    fw, fv = B.fillers(2)
    k2 = B.raw(B.q[1:2] + fw, [-0.25] + fv)
    B.cov(k1, [k2])
    ql = B.query_kf(9)
    B.adds(k1, k2)
    B.loop(ql, 0.5, [])
    B.reloc(1, [k1])
    return B.done(['loop_best0'], k1=k1, k2=k2)


def crafted_neighbour_best():
    """D. `mRelocScore > bestScore` is strict: a neighbour with an EQUAL score leaves pBestKF alone, one with a larger score moves it."""
    B = _Crafted(5)
    a, b, c, d = B.shares(0.5, (0,)), B.shares(0.5, (1,)), B.shares(0.5, (2,)), B.shares(0.75, (3,))
    B.cov(a, [b])
    B.cov(c, [d])
    ql = B.query_kf(9)
    B.adds(a, b, c, d)
    # accumulated: a 1.0 (elects a), b 0.5, c 1.25 (elects d), d 0.75; retained above 0.9375: a's and c's entries
    B.reloc(1, [a, d])
    B.loop(ql, 0.0, [a, d])
    return B.done(['best_ge'], a=a, d=d)


def crafted_eleventh_neighbour():
    """D. GetBestCovisibilityKeyFrames(10): ten covisibles that are not in the database, then an eleventh whose score would be
    accumulated and would take pBestKF."""
    B = _Crafted(3)
    a, big = B.shares(0.5, (0,)), B.shares(0.625, (1,))
    out = [B.shares(0.25, (2,)) for _ in range(10)]       # never added
    B.cov(a, out + [big])
    ql = B.query_kf(9)
    B.adds(a, big)
    B.reloc(1, [a, big])
    B.loop(ql, 0.0, [a, big])
    return B.done(['neigh11'], a=a, big=big)


def crafted_accumulation_order():
    """D. accScore is a float and the neighbours are added one at a time: 0.5 + 2^-25 + 2^-25 is 0.5 (each add is a tie that rounds to
    even); the neighbours first would give 0.5 + 2^-24, the threshold of crafted_retain_rounds, and b would drop out."""
    B = _Crafted(5)
    a, n1, n2, b = B.shares(0.5, (0,)), B.shares(2.0 ** -25, (1,)), B.shares(2.0 ** -25, (2,)), B.shares(ulps(0.375, 1), (3,))
    B.cov(a, [n1, n2])
    ql = B.query_kf(9)
    B.adds(a, n1, n2, b)
    B.reloc(1, [a, b])
    B.loop(ql, 0.0, [a, b])
    return B.done(['acc_reorder'], a=a, b=b)


def _own_words_query(B, n):
    """the words of keyframe n that no other vector has (its fillers), 1.0 each: a query about n alone"""
    k = B.scene['kfs'][n]
    w = [int(x) for x in k['words'] if int(x) >= 500]
    return w, [1.0] * len(w)


def crafted_loop_neighbour_min_common():
    """D, loop only.  A neighbour that is listed by this query with exactly minCommonWords words: not scored now, and its mLoopScore of
    an earlier query (0.25) is NOT accumulated, because the loop search repeats `mnLoopWords > minCommonWords` for neighbours."""
    B = _Crafted(6)
    a, b = B.shares(0.5, (0, 1, 2, 3, 4)), B.shares(ulps(0.375, 1), (0, 1, 2, 3, 5))
    n = B.shares(0.125, (0, 1, 2, 3), nfill=2, fill_value=0.125)
    B.cov(a, [n])
    w, v = _own_words_query(B, n)
    q0 = B.raw(w, v, mnId=300)
    q1 = B.query_kf(301)
    B.adds(a, b, n)
    B.loop(q0, 0.0, [n])                                  # n alone, 2 of 2 words, scored 0.25
    B.loop(q1, 0.0, [a, b])                               # a accumulates 0.5 only; with n's 0.25 the threshold would pass b
    return B.done(['loop_neigh_no_minc'], a=a, b=b, n=n)


def crafted_reloc_neighbour_stale_score():
    """D, relocalisation.  The same vectors: relocalisation has no such test, so the neighbour that is listed, not scored, and carries
    the mRelocScore of the earlier frame (0.25) IS accumulated: a reaches 0.75 and b is no longer above 0.75f of it."""
    B = _Crafted(6)
    a, b = B.shares(0.5, (0, 1, 2, 3, 4)), B.shares(ulps(0.375, 1), (0, 1, 2, 3, 5))
    n = B.shares(0.125, (0, 1, 2, 3), nfill=2, fill_value=0.125)
    B.cov(a, [n])
    w, v = _own_words_query(B, n)
    B.adds(a, b, n)
    B.reloc(1, [n], w, v)
    B.reloc(2, [a])
    return B.done(['reloc_neigh_minc'], a=a, b=b, n=n)


def crafted_loop_neighbour_connected():
    """D, loop.  A neighbour that is connected to the query keyframe is never given this query's id: its mnLoopQuery is that of the
    earlier query, so its mLoopScore (0.25) is not accumulated although its mnLoopWords (1, reset at every encounter) is above
    minCommonWords = 0."""
    B = _Crafted(4)
    a, n, b = B.shares(0.5, (0,)), B.shares(0.25, (1,)), B.shares(ulps(0.375, 1), (2,))
    B.cov(a, [n])
    q0, q1 = B.query_kf(400), B.query_kf(401, connected=[n])
    B.adds(a, n, b)
    B.loop(q0, 0.0, [a])                                  # a accumulates n: 0.75; b is not above 0.5625
    B.loop(q1, 0.0, [a, b])                               # n is connected: a stays at 0.5, b is above 0.375
    return B.done(['loop_neigh_no_query'], a=a, n=n, b=b)


def crafted_same_id_twice():
    """E. The same mnId / frame id twice in a row: the second query finds every member stale, resets and lists nobody and returns
    nothing; the word counts double."""
    B = _Crafted(3)
    a, b = B.shares(0.5, (0, 1)), B.shares(0.5, (1, 2))
    ql = B.query_kf(9)
    B.adds(a, b)
    B.reloc(5, [a, b])
    B.reloc(5, [])
    B.loop(ql, 0.0, [a, b])
    B.loop(ql, 0.0, [])
    B.reloc(6, [a, b])
    return B.done(['ignore_query_id'], a=a, b=b)


def crafted_connected_with_stale_id():
    """E. Two query keyframes with the same mnId.  The first is connected to nobody and leaves its id in k.  The second IS connected to
    k, but `mnLoopQuery != mnId` is tested before the connected set: k is not reset, and as n's neighbour it is accumulated with its
    score of the first query and elected: a keyframe connected to the query keyframe is returned."""
    B = _Crafted(3)
    k, n = B.shares(0.5, (0,)), B.shares(0.25, (1,))
    B.cov(n, [k])
    q1, q2 = B.query_kf(7), B.query_kf(7, connected=[k])
    B.adds(k)
    B.loop(q1, 0.0, [k])
    B.adds(n)
    B.loop(q2, 0.0, [k])
    return B.done(['connected_first'], k=k, n=n)


def crafted_clear_and_readd():
    """E. clear() empties the lists and leaves the keyframes' members alone: after a re-add the same frame id finds them stale."""
    B = _Crafted(3)
    a, b = B.shares(0.5, (0,)), B.shares(0.5, (1,))
    ql = B.query_kf(9)
    B.adds(a, b)
    B.reloc(9, [a, b])
    B.loop(ql, 0.0, [a, b])
    B.step('clear')
    B.reloc(9, [])                                        # nothing in the lists
    B.adds(b, a)
    B.reloc(9, [])                                        # stale
    B.loop(ql, 0.0, [])
    B.reloc(10, [a, b])                                   # a new id: a holds the query's first word, whatever the add order
    return B.done(['ignore_query_id'], a=a, b=b)


def crafted_duplicates():
    """F. Two entries elect the same pBestKF (and its own entry is not retained): it is returned once."""
    B = _Crafted(4)
    a, b, c = B.shares(0.5, (0,)), B.shares(0.5, (1,)), B.shares(0.75, (2,))
    B.cov(a, [c])
    B.cov(b, [c])
    ql = B.query_kf(9)
    B.adds(a, b, c)
    B.reloc(1, [c])
    B.loop(ql, 0.0, [c])
    return B.done(['no_dedup'], c=c)


def crafted_tie_order():
    """F. Two keyframes tied on their first common word come back in the order of that word's list: erase + re-add moves one behind."""
    B = _Crafted(3)
    a, b = B.shares(0.5, (0, 1)), B.shares(0.5, (0, 2))
    B.adds(b, a)
    B.reloc(1, [b, a])
    B.step('erase', b)
    B.adds(b)
    B.reloc(2, [a, b])
    return B.done(['order_by_index'], a=a, b=b)


MAXC_RANGE = range(1, 41)


def crafted_scenes():
    sc = {'A_maxc%02d' % m: crafted_min_common(m) for m in MAXC_RANGE}
    sc.update(B_min_score=crafted_min_score(), C_retain=crafted_retain(), C_retain_rounds=crafted_retain_rounds(),
              C_best_start=crafted_best_start(), D_neighbour_best=crafted_neighbour_best(), D_eleventh=crafted_eleventh_neighbour(),
              D_acc_order=crafted_accumulation_order(), D_loop_neigh_minc=crafted_loop_neighbour_min_common(),
              D_reloc_neigh_stale=crafted_reloc_neighbour_stale_score(), D_loop_neigh_connected=crafted_loop_neighbour_connected(),
              E_same_id=crafted_same_id_twice(), E_connected_stale_id=crafted_connected_with_stale_id(),
              E_clear_readd=crafted_clear_and_readd(), F_duplicates=crafted_duplicates(), F_tie_order=crafted_tie_order())
    return sc


_CRAFTED = None


def crafted():
    global _CRAFTED
    if _CRAFTED is None:
        _CRAFTED = crafted_scenes()
    return _CRAFTED


def every_scene():
    """the seeded scenes and the crafted ones, by name"""
    d = dict(scenes())
    d.update(crafted())
    return d


def trace(ref, scene):
    """(results, members): the result of every step (None for a mutation) and all six members of every keyframe after every step"""
    res, mem = [], []
    for st in scene['steps']:
        res.append(ref.step(st))
        mem.append(ref.members())
    return res, mem


# ---- the recorded outputs of the reference's own KeyFrameDatabase.cc (oracle/_ref/libos1_kfdb.so) ----------------------------------
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'os1_kfdb_outputs.npz')


def have_os1():
    from oracle import pyoracle
    return pyoracle.have_os1_kfdb()


def os1_ref(scene):
    from oracle import pyoracle
    return pyoracle.Os1KeyFrameDatabase(scene)


def encode_trace(res, mem):
    """-> {field: array}: results as a flat int32 list (per step: -1 for a mutation, else the count, then the keyframe indices);
    members as (steps, keyframes, 6) uint64"""
    flat = []
    for r in res:
        flat += [-1] if r is None else [len(r)] + list(r)
    return {'results': np.asarray(flat, np.int32), 'members': np.asarray(mem, np.uint64).reshape(len(mem), -1, 6)}


def decode_trace(rec):
    flat, res, i = rec['results'].tolist(), [], 0
    while i < len(flat):
        if flat[i] < 0:
            res.append(None)
            i += 1
        else:
            res.append(flat[i + 1:i + 1 + flat[i]])
            i += 1 + flat[i]
    return res, [[tuple(int(x) for x in k) for k in step] for step in rec['members']]


def golden_records():
    """{'<scene>|<field>': array} computed by the reference object now"""
    out = {}
    for name, scene in every_scene().items():
        ref = os1_ref(scene)
        for f, a in encode_trace(*trace(ref, scene)).items():
            out['%s|%s' % (name, f)] = a
        ref.close()
    return out


_GOLDEN = None


def golden():
    """{scene: (results, members)} of the recording, or None where the file is absent"""
    global _GOLDEN
    if _GOLDEN is None and os.path.exists(GOLDEN):
        z = np.load(GOLDEN)
        names = sorted({k.split('|')[0] for k in z.files})
        _GOLDEN = {n: decode_trace({f: z['%s|%s' % (n, f)] for f in ('results', 'members')}) for n in names}
    return _GOLDEN


def write_expected(scene, res, mem, path):
    """The file tests/cpp/kfdb_test.cpp reads beside a scene file: per step the recorded candidates and members of the reference."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<2i', len(res), len(scene['kfs'])))
        for r, m in zip(res, mem):
            f.write(struct.pack('<i', -1 if r is None else len(r)))
            if r:
                f.write(np.asarray(r, '<i4').tobytes())
            for k in m:
                f.write(struct.pack('<QiIQiI', k[0], k[1], k[2], k[3], k[4], k[5]))
