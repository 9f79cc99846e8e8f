"""Crafted feature sets that sit ON the decision boundaries of the three vocabulary-guided searches, with the expected result
written down by hand: SearchByBoW(KeyFrame, Frame) src/ORBmatcher.cc:154-283, SearchByBoW(KeyFrame, KeyFrame) :517-650,
SearchForTriangulation :652-804 with CheckDistEpipolarLine :135-152 and ComputeThreeMaxima :1554-1595.  The companion of
tests/search_boundary_util.py, whose helpers it reuses.

Every scene carries its inputs, the expected result as a literal stated from the reference text and a witness: a predicate in
numpy float32 / Python arithmetic that shows the scene really is on the boundary its name states.  Neither the oracle nor the
library computes an expectation.

Kinds: 'kf_frame' (valid2 = None, `bestDist1<=TH_LOW` :223), 'kf_kf' (valid2 given, `bestDist1<TH_LOW` :593), 'tri'
(SearchForTriangulation).  Expectations: (nmatches, {idx1: idx2}) for the two SearchByBoW kinds, (nmatches, [(idx1, idx2), ...])
in ascending idx1 for tri.

Descriptors are row(n) of search_boundary_util -- distance(row(a), row(b)) == |a - b| -- written as the integer n; n >= CPL is
the complement of row(n - CPL), at distance 256 - |a - (n - CPL)| from row(a).  FeatureVectors are hand-written (nodes, offsets,
features) triples: a scene lists its nodes as (node id, side-1 items, side-2 items); items get ascending feature indices in the
order written, so a feature's index is its position in the scene unless idx1 / idx2 say otherwise.  An item is n or
(n, on[, angle]) for the SearchByBoW kinds (on: valid1 / valid2) and (n, on, x, y[, octave[, angle]]) for tri (on: has NO
MapPoint).

The ratio test is `float(d1) < mfNNratio * float(d2)` (:225, :595).  The product is a float: for 0.6f * 5 and 0.6f * 40 the exact
product lies above 3 / 24 and rounds onto it, so the float test rejects (3 < 3 is false) where a double one accepts -- kind (i)
of ratio_float_pairs().  (0.6f * 50 does not: the exact product 30.0000012 lies past the midpoint to the next float and rounds up to
30.0000019, so (30, 50) is accepted in float as in double.)  Kind (ii), float accepts and double rejects, cannot exist for `<`: d1 is an integer, so a float, and
rounding is monotonic -- an exact product <= d1 never rounds above d1.  The pairs (9, 10) and (90, 100) at 0.9 of
search_boundary_util do NOT split this comparison: 0.9f lies below 0.9, the product rounds UP onto 9 / 90, and `9 < 9` is as
false as `9 < 8.9999998`; they split `bestDist > ratio * bestDist2` (:115) only.

Counts the searches below find (asserted in tests/test_bow_boundaries.py): ratio pairs of kind (i): 25 over the five ratios used (13 at 0.6, 12 at 0.8),
none of kind (ii); line-gate float / double splits with F12 = [t]x, t = (1, 0, 0): octaves 0, 5 and 7 of the 1.2 table and no other;
with a general F12 (den != 1): 4; single-rounding splits: 3 for a / b / c, 3 for num, 3 for den, 4 for the epipole sum."""
from fractions import Fraction

import numpy as np

from search_boundary_util import F32, HIST_COUNTS, ROT_PROBES, SF, hamming, make_kps, rot_bin32, row

# constants of os1_amd/csrc/orbfe_bow.hip the scenes of family G are sized to (the CPU test reads them out of the source)
CONSTANTS = {'TH_LOW': 50,              # :42
             'kMaxGroup': 65535,        # :44   features of one frame under one node
             'kBowTopK': 8,             # :180  keys per frame-1 feature of a large node
             'kTopkRegs': 32,           # :182  keys a lane keeps in registers: nodes of up to 64 * 32 = 2 048 frame-2 features
             'kTopkLdsFeatures': 4096,  # :183  frame-2 features of a node staged in LDS
             'kBowMatrix': 12288,       # :264  distance matrix entries / winners kept in LDS
             'kBowSide': 256}           # :265  features per side of a node handled from LDS
TH_LOW, K_GROUP = CONSTANTS['TH_LOW'], CONSTANTS['kMaxGroup']
K_SIDE, K_MATRIX, K_TOPK = CONSTANTS['kBowSide'], CONSTANTS['kBowMatrix'], CONSTANTS['kBowTopK']
K_REGS2, K_LDS2 = 64 * CONSTANTS['kTopkRegs'], CONSTANTS['kTopkLdsFeatures']      # frame-2 features: keys in registers / staged in LDS
CPL = 1000
S2 = (SF * SF).astype(np.float32)                                # mvLevelSigma2 (ORBextractor.cc:436)
_TABLE = np.stack([row(n) for n in range(257)])
_TABLE = np.concatenate([_TABLE, np.zeros((CPL - 257, 32), np.uint8), ~_TABLE])


def desc_rows(codes):
    return _TABLE[np.asarray(codes, np.int64)] if len(codes) else np.zeros((0, 32), np.uint8)


def dist(a, b):
    """Hamming distance of two descriptor codes, from the construction."""
    (ca, a), (cb, b) = divmod(a, CPL), divmod(b, CPL)
    return abs(a - b) if ca == cb else 256 - abs(a - b)


class Scene:
    def __init__(self, name, family, kind, inp, expect, witness, text=''):
        self.name, self.family, self.kind, self.inp, self.expect, self.witness, self.text = name, family, kind, inp, expect, witness, text

    def __repr__(self):
        return self.name


SCENES = []
T_OPEN = dict(F12=[[0, 0, 0], [0, 0, -1], [0, 1, 0]], ex=-1e4, ey=-1e4)      # a = 0, b = 1, c = -y1: dsqr = (y2 - y1)^2; epipole far away


def _item(it, kind, pos):
    it = it if isinstance(it, tuple) else (it,)
    if kind != 'tri':
        return (it[0], it[1] if len(it) > 1 else 1, 0.0, 0.0, 0, it[2] if len(it) > 2 else 0.0)
    return (it[0], it[1] if len(it) > 1 else 1, it[2] if len(it) > 2 else 10.0 + pos, it[3] if len(it) > 3 else 100.0,
            it[4] if len(it) > 4 else 0, it[5] if len(it) > 5 else 0.0)


def _side(nodes, which, kind, idx):
    ids, off, feat, items = [], [0], [], []
    for nd in nodes:
        its = nd[which]
        if its is None:
            continue
        ids.append(nd[0])
        for it in its:
            feat.append(len(items))
            items.append(_item(it, kind, len(items)))
        off.append(len(feat))
    n = len(items)
    idx = list(range(n)) if idx is None else list(idx)
    assert sorted(idx) == list(range(n))
    arr = [None] * n
    for pos, i in enumerate(idx):
        arr[i] = items[pos]
    fv = (np.array(ids, np.uint32), np.array(off, np.uint32), np.array([idx[p] for p in feat], np.uint32))
    for a, b in zip(off[:-1], off[1:]):
        assert list(fv[2][a:b]) == sorted(fv[2][a:b]), 'feature lists ascend inside a node'
    assert ids == sorted(set(ids))
    return arr, fv


def make_inp(kind, nodes, ratio=0.7, ori=False, idx1=None, idx2=None, geo=None):
    a1, fv1 = _side(nodes, 1, kind, idx1)
    a2, fv2 = _side(nodes, 2, kind, idx2)
    d1, d2 = desc_rows([a[0] for a in a1]), desc_rows([a[0] for a in a2])
    on1, on2 = np.array([a[1] for a in a1], np.uint8), np.array([a[1] for a in a2], np.uint8)
    if kind != 'tri':
        return dict(desc1=d1, angle1=np.array([a[5] for a in a1], np.float32), valid1=on1, fv1=fv1, desc2=d2,
                    angle2=np.array([a[5] for a in a2], np.float32), valid2=on2 if kind == 'kf_kf' else None, fv2=fv2, ratio=ratio, ori=ori)
    assert kind == 'tri'
    g = dict(T_OPEN, **(geo or {}))
    return dict(kps1=make_kps([(a[2], a[3], a[4], a[5]) for a in a1]), desc1=d1, has1=(1 - on1).astype(np.uint8), fv1=fv1,
                kps2=make_kps([(a[2], a[3], a[4], a[5]) for a in a2]), desc2=d2, has2=(1 - on2).astype(np.uint8), fv2=fv2,
                F12=np.asarray(g['F12'], np.float32).reshape(9), ex=float(g['ex']), ey=float(g['ey']), sf=g.get('sf', SF), s2=g.get('s2', S2), ori=ori)


def add(name, family, kind, nodes, expect, witness=None, text='', **kw):
    """expect: {idx1: idx2}; the match count is stated by its size unless given as (n, {...})."""
    assert name not in BY_NAME, name
    n, m = expect if isinstance(expect, tuple) else (len(expect), expect)
    inp = nodes if isinstance(nodes, dict) else make_inp(kind, nodes, **kw)
    s = Scene(name, family, kind, inp, (n, sorted(m.items())) if kind == 'tri' else (n, dict(m)), witness or (lambda: True), text)
    SCENES.append(s)
    BY_NAME[name] = s
    return s


BY_NAME = {}


def expected(scene):
    """The hand-stated result in the form run() returns."""
    n, m = scene.expect
    if scene.kind == 'tri':
        return (n, [tuple(p) for p in m])
    a = [-1] * len(scene.inp['desc1'])
    for k, v in m.items():
        a[k] = v
    return (n, a)


def run(scene, be, inp=None, desc1=None, desc2=None):
    """be: the oracle or a Matcher.  desc1 / desc2: device-resident rows in place of the host arrays."""
    i = inp or scene.inp
    if scene.kind == 'tri':
        n, p = be.search_for_triangulation(i['kps1'], i['desc1'], i['has1'], i['fv1'], i['kps2'], i['desc2'], i['has2'], i['fv2'], i['F12'], i['ex'],
                                           i['ey'], i['sf'], i['s2'], i['ori'])
        return (int(n), [(int(a), int(b)) for a, b in p])
    a = (i['desc1'] if desc1 is None else desc1, i['angle1'], i['valid1'], i['fv1'], i['desc2'] if desc2 is None else desc2, i['angle2'], i['valid2'],
         i['fv2'], i['ratio'], i['ori'])
    n, m = be.search_by_bow(*a, scene.kind == 'kf_kf') if hasattr(be, 'search_by_bow_batch') else be.search_by_bow(*a)
    return (int(n), [int(v) for v in m])


KF = ('kf_frame', 'kf_kf')
ALL = ('kf_frame', 'kf_kf', 'tri')
TAG = {'kf_frame': 'kff', 'kf_kf': 'kfk', 'tri': 'tri'}


# ==== A. TH_LOW ==============================================================================================================
def _family_a():
    # one node, one frame-1 feature row(0); the candidate at distance d; the worse second at 200 (0.7 * 200 = 140: the ratio is open)
    for kind, d, ok in [('kf_frame', 50, 1), ('kf_frame', 51, 0), ('kf_kf', 49, 1), ('kf_kf', 50, 0), ('tri', 50, 1), ('tri', 51, 0),
                        ('kf_frame', 0, 1), ('kf_kf', 0, 1), ('tri', 0, 1)]:
        w = lambda d=d: hamming(row(0), row(d)) == d and dist(0, d) == d
        tag = 'th_low_%d_%s_%s' % (d, 'in' if ok else 'out', TAG[kind])
        add(tag + '_lone', 'A', kind, [(5, [0], [d])], {0: 0} if ok else {}, w)
        add(tag + '_second_200', 'A', kind, [(5, [0], [200, d])], {0: 1} if ok else {}, w)
        add(tag + '_second_one_worse_ratio_1p5', 'A', kind, [(5, [0], [d, d + 1])], {0: 0} if ok else {}, w, ratio=1.5)
    # 255 and the complement (256): `dist<bestDist1` from 256 never takes a 256; nothing is accepted either way
    for kind in ALL:
        add('th_low_complement_256_out_%s' % TAG[kind], 'A', kind, [(5, [0], [CPL + 0, 255])], {}, lambda: dist(0, CPL) == 256 and hamming(row(0), ~row(0)) == 256)


# ==== B. ratio test ==========================================================================================================
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)


def ratio_float_pairs():
    """{'i': [(ratio, d1, d2)], 'ii': [...]}: (i) the float32 product rounds onto d1, so `float(d1) < ratio * float(d2)` rejects, while the same
    comparison widened to double accepts; (ii) the converse (none: see the module text)."""
    out = {'i': [], 'ii': []}
    for r in RATIOS:
        for d1 in range(0, 51):
            for d2 in range(d1, 256):
                f = bool(F32(d1) < F32(r) * F32(d2))
                d = bool(float(d1) < float(F32(r)) * float(d2))
                if f != d:
                    out['i' if d else 'ii'].append((r, d1, d2))
    assert len(out['i']) >= 2 and (0.6, 3, 5) in out['i'] and (0.6, 24, 40) in out['i'] and (0.6, 30, 50) not in out['i']
    return out


def _family_b():
    for kind in KF:
        t = TAG[kind]
        # second best absent: bestDist2 stays 256 (:198, :563) -- 40 < 0.6 * 256; a second candidate at 41 would reject (40 < 24.6 is false)
        add('ratio_second_absent_%s' % t, 'B', kind, [(2, [0], [40])], {0: 0}, lambda: F32(40) < F32(0.6) * F32(256), ratio=0.6)
        add('ratio_second_present_41_rejects_%s' % t, 'B', kind, [(2, [0], [40, 41])], {}, lambda: not F32(40) < F32(0.6) * F32(41), ratio=0.6)
        # ... and stays 256 when the only other candidate is already claimed (by feature 0, an exact copy of it: 0 < 0.6 * 1)
        add('ratio_second_absent_other_claimed_%s' % t, 'B', kind, [(2, [41, 0], [40, 41])], {0: 1, 1: 0}, lambda: not F32(40) < F32(0.6) * F32(41), ratio=0.6)
        # second best equal to the best: the first in list order stays best (`dist<bestDist1` :211), d2 == d1, rejected for every ratio <= 1
        for r in (0.6, 0.9, 1.0):
            add('ratio_tie_rejected_ratio_%s_%s' % (('%g' % r).replace('.', 'p'), t), 'B', kind, [(2, [0], [10, 10])], {},
                lambda r=r: not F32(10) < F32(r) * F32(10), ratio=r)
        # ... a ratio above 1 shows WHO is best: the first (index 1 here: index 0 is farther)
        add('ratio_tie_first_in_list_order_wins_ratio_1p5_%s' % t, 'B', kind, [(2, [0], [30, 10, 10, 10])], {0: 1}, lambda: F32(10) < F32(1.5) * F32(10), ratio=1.5)
        # the second best is the multiset's second smallest: the displaced earlier best (:213) and a later arrival (:217)
        w = lambda: (not F32(10) < F32(0.8) * F32(12)) and F32(10) < F32(0.8) * F32(13) and F32(10) < F32(0.8) * F32(30)
        add('ratio_second_is_displaced_best_12_rejects_%s' % t, 'B', kind, [(2, [0], [12, 10, 30])], {}, w, ratio=0.8)
        add('ratio_second_is_displaced_best_13_accepts_%s' % t, 'B', kind, [(2, [0], [13, 10, 30])], {0: 1}, w, ratio=0.8)
        add('ratio_second_is_later_arrival_12_rejects_%s' % t, 'B', kind, [(2, [0], [10, 30, 12])], {}, w, ratio=0.8)
        add('ratio_second_is_later_arrival_13_accepts_%s' % t, 'B', kind, [(2, [0], [10, 30, 13])], {0: 0}, w, ratio=0.8)
        add('ratio_second_twice_displaced_%s' % t, 'B', kind, [(2, [0], [30, 12, 10])], {}, w, ratio=0.8)
        # the float product
        pairs = ratio_float_pairs()['i']
        pick = [(0.6, 3, 5), (0.6, 24, 40)] + [p for p in pairs if p[0] != 0.6 and p[1] <= 49][:4]
        for r, d1, d2 in pick:
            def wf(r=r, d1=d1, d2=d2):
                return (not F32(d1) < F32(r) * F32(d2)) and float(d1) < float(F32(r)) * float(d2) and F32(r) * F32(d2) == F32(d1)
            add('ratio_float_product_%s_%d_%d_rejects_%s' % (('%g' % r).replace('.', 'p'), d1, d2, t), 'B', kind, [(2, [0], [d2, d1])], {}, wf, ratio=r)
            add('ratio_float_product_%s_%d_%d_accepts_%s' % (('%g' % r).replace('.', 'p'), d1, d2 + 1, t), 'B', kind, [(2, [0], [d2 + 1, d1])], {0: 1},
                lambda r=r, d1=d1, d2=d2: F32(d1) < F32(r) * F32(d2 + 1), ratio=r)
    # tri has no ratio test: a second candidate one bit worse does not stop the match; a tie goes to the LAST (family E)
    add('no_ratio_test_second_one_worse_tri', 'B', 'tri', [(2, [0], [10, 11])], {0: 0})
    add('no_ratio_test_second_one_worse_first_tri', 'B', 'tri', [(2, [0], [11, 10])], {0: 1})


# ==== C. order and claiming ==================================================================================================
def _family_c():
    for kind in KF:
        t = TAG[kind]
        # feature 0 = row(0) takes X = row(0) (0 < 0.7 * d2).  What X is to feature 1:
        # its best: 1 = row(20) sees X at 20, 45 at 25, 60 at 40 -- X gone, 25 < 0.7 * 40: takes the next free one
        add('claimed_was_best_next_free_taken_%s' % t, 'C', kind, [(3, [0, 20], [0, 45, 60])], {0: 0, 1: 1}, lambda: F32(25) < F32(0.7) * F32(40))
        # its second best: 1 = row(5) sees 9 at 4, X at 5, 40 at 35 -- with X free 4 < 3.5 fails; X gone, 4 < 24.5 passes
        add('claimed_was_second_ratio_now_passes_%s' % t, 'C', kind, [(3, [0, 5], [0, 9, 40])], {0: 0, 1: 1},
            lambda: (not F32(4) < F32(0.7) * F32(5)) and F32(4) < F32(0.7) * F32(35))
        # the one that made the ratio fail by a tie in front of the best: 1 = row(5) sees X at 5 (first), 10 at 5, 40 at 35
        add('claimed_was_tie_in_front_of_best_%s' % t, 'C', kind, [(3, [0, 5], [0, 10, 40])], {0: 0, 1: 1},
            lambda: (not F32(5) < F32(0.7) * F32(5)) and F32(5) < F32(0.7) * F32(35))
        # irrelevant: 1 = row(45) sees X at 45, 46 at 1, 40 at 5
        add('claimed_was_irrelevant_%s' % t, 'C', kind, [(3, [0, 45], [0, 46, 40])], {0: 0, 1: 1}, lambda: F32(1) < F32(0.7) * F32(5))
        # claimed leaves nothing: both want X, nothing else there
        add('claimed_was_the_only_candidate_%s' % t, 'C', kind, [(3, [0, 1], [0])], {0: 0})
        # a feature rejected by the ratio claims nothing: 0 = row(0) sees 10, 12 (10 < 8.4 fails); 1 = row(10) takes index 0 at 0 (second 2)
        add('rejected_by_ratio_claims_nothing_%s' % t, 'C', kind, [(3, [0, 10], [10, 12])], {1: 0},
            lambda: (not F32(10) < F32(0.7) * F32(12)) and F32(0) < F32(0.7) * F32(2))
        # ... by the threshold
        add('rejected_by_threshold_claims_nothing_%s' % t, 'C', kind, [(3, [0, 51], [51])], {1: 0})
        # valid1 == 0 (:188-192, :554-557): claims nothing
        add('invalid_frame1_feature_claims_nothing_%s' % t, 'C', kind, [(3, [(0, 0), 5], [0])], {1: 0})
        # three claims in a row in one node: 0 takes index 0 (0 < 0.7 * 4); 1 = row(1) sees 4 at 3 and 9 at 8 (3 < 5.6); 2 = row(2) is left index 2 at 7
        add('claims_chain_of_three_%s' % t, 'C', kind, [(3, [0, 1, 2], [0, 4, 9])], {0: 0, 1: 1, 2: 2},
            lambda: F32(0) < F32(0.7) * F32(4) and F32(3) < F32(0.7) * F32(8))
    # kf_kf: a candidate with valid2 == 0 is neither best nor second best (:571-575)
    add('invalid_candidate_not_best_kfk', 'C', 'kf_kf', [(3, [0], [(0, 0), 10])], {0: 1})
    add('invalid_candidate_not_second_kfk', 'C', 'kf_kf', [(3, [0], [10, (11, 0)])], {0: 0}, lambda: not F32(10) < F32(0.7) * F32(11))
    add('invalid_candidates_only_kfk', 'C', 'kf_kf', [(3, [0], [(0, 0), (1, 0)])], {})
    # tri: features with a MapPoint are skipped on either side (:698, :715)
    add('has_mp1_skipped_tri', 'C', 'tri', [(3, [(0, 0), 1], [0])], {1: 0})
    add('has_mp2_skipped_tri', 'C', 'tri', [(3, [0], [(0, 0), 7])], {0: 1})
    # vbMatched2 is never set (:672, :715): two frame-1 features take the SAME frame-2 feature, both pairs are reported
    add('same_candidate_taken_twice_tri', 'C', 'tri', [(3, [0, 2], [1, 40])], {0: 0, 1: 0})
    # pairs come out in ascending idx1 (:796-801) whatever the node order: node 3 holds frame-1 features 2, 3; node 8 holds 0, 1
    add('pairs_ascend_in_idx1_tri', 'C', 'tri', [(3, [0, 1], [0, 1]), (8, [20, 21], [20, 21])], {2: 0, 3: 1, 0: 2, 1: 3}, idx1=[2, 3, 0, 1])
    for kind in KF:
        add('matches_indexed_by_idx1_%s' % TAG[kind], 'C', kind, [(3, [0, 3], [0, 3]), (8, [20, 23], [20, 23])], {2: 0, 3: 1, 0: 2, 1: 3},
            lambda: F32(0) < F32(0.7) * F32(3), idx1=[2, 3, 0, 1])


# ==== D. node intersection ===================================================================================================
def _family_d():
    for kind in ALL:
        t = TAG[kind]
        # nodes on one side only before, between and after the common ones (:251-258 lower_bound on either side)
        nodes = [(1, [0], None), (2, None, [0]), (4, [10], [10]), (5, [0], None), (6, [0], None), (7, None, [0]), (9, [20], [20]), (11, None, [0]), (12, [0], None)]
        add('nodes_one_sided_before_between_after_%s' % t, 'D', kind, nodes, {1: 1, 4: 3})
        add('intersection_empty_%s' % t, 'D', kind, [(1, [0], None), (2, None, [0]), (3, [0], None), (4, None, [0])], {})
        # identical rows under different nodes do not match
        add('identical_rows_other_node_%s' % t, 'D', kind, [(1, [0, 1], None), (2, None, [0, 1]), (3, [30], [31])], {2: 2})
        add('side1_empty_%s' % t, 'D', kind, [(1, None, [0])], {})
        add('side2_empty_%s' % t, 'D', kind, [(1, [0], None)], {})
        add('both_sides_empty_%s' % t, 'D', kind, [], {})
        # node id 0 and the largest id a uint32 FeatureVector holds
        add('node_id_0_and_largest_%s' % t, 'D', kind, [(0, [0], [1]), (7, [2], None), (0xffffffff, [3], [4])], {0: 0, 2: 1})
        add('many_common_nodes_%s' % t, 'D', kind, [(10 * k, [k], [k]) for k in range(40)], {k: k for k in range(40)})


# ==== E. triangulation geometry ==============================================================================================
def r32(fr):
    """A Fraction rounded ONCE to float32, ties to even."""
    f = F32(float(fr))
    c = [np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))]
    return min(c, key=lambda v: (abs(Fraction(float(v)) - fr), int(v.view(np.uint32)) & 1))


def _q(v):
    return Fraction(float(v))


def _pa(p, q, r, s, fuse):
    """p*q + r*s rounded per operation (fuse None), or with one of the products fused into the addition (0: the first, 1: the second)."""
    if fuse is None:
        return r32(_q(r32(_q(p) * _q(q))) + _q(r32(_q(r) * _q(s))))
    return r32(_q(p) * _q(q) + _q(r32(_q(r) * _q(s)))) if fuse == 0 else r32(_q(r32(_q(p) * _q(q))) + _q(r) * _q(s))


def line_gate(F, x1, y1, x2, y2, o, fuse=None, where=('abc', 'num', 'den'), double=True):
    """CheckDistEpipolarLine (:138-151) in exact rational arithmetic rounded to float32 once per operation; fuse 0 / 1: the
    product-then-add of the expressions in `where` rounded once instead.  None for den == 0.  double=False: `dsqr < 3.84f * sigma2`."""
    F = [F32(v) for v in np.asarray(F, np.float32).reshape(9)]
    x1, y1, x2, y2 = F32(x1), F32(y1), F32(x2), F32(y2)
    fa = fuse if 'abc' in where else None
    a, b, c = [r32(_q(_pa(x1, F[k], y1, F[3 + k], fa)) + _q(F[6 + k])) for k in range(3)]
    num = r32(_q(_pa(a, x2, b, y2, fuse if 'num' in where else None)) + _q(c))
    den = _pa(a, a, b, b, fuse if 'den' in where else None)
    if den == 0:
        return None
    dsqr = r32(_q(r32(_q(num) * _q(num))) / _q(den))
    if double:
        return bool(_q(dsqr) < Fraction(3.84) * _q(S2[o]))
    return bool(dsqr < F32(F32(3.84) * S2[o]))


def epipole_gate(ex, ey, x2, y2, o, fuse=None):
    """True: skipped.  `distex*distex+distey*distey<100*mvScaleFactors[o]` (:727-729), all float."""
    dx, dy = r32(_q(F32(ex)) - _q(F32(x2))), r32(_q(F32(ey)) - _q(F32(y2)))
    return bool(_pa(dx, dx, dy, dy, fuse) < F32(100) * SF[o])


def _line_np(F, x1, y1, x2, y2):
    a, b, c = [x1 * F[k] + y1 * F[3 + k] + F[6 + k] for k in range(3)]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    return num * num / den, a, b, c, den


def line_t_cases():
    """[(y2 - y1, octave, double verdict)] with F12 = [[0,0,0],[0,0,-1],[0,1,0]] (dsqr = (y2 - y1)^2, one float product) where
    `dsqr < 3.84 * sigma2` in double and `dsqr < 3.84f * sigma2` in float disagree."""
    out = []
    for o in range(8):
        t64, t32 = 3.84 * float(S2[o]), F32(F32(3.84) * S2[o])
        d0 = F32(np.sqrt(t64))
        d = (d0 + np.arange(-2000, 2000, dtype=np.float32) * np.spacing(d0)).astype(np.float32)
        ds = d * d
        j = np.nonzero((ds.astype(np.float64) < t64) != (ds < t32))[0]
        if len(j):
            out.append((float(d[j[0]]), o, bool(float(ds[j[0]]) < t64)))
    assert [c[1] for c in out] == [0, 5, 7], out
    return out


def _random_geometry(rng):
    F = ((rng.integers(-8, 9, 9) / 8.0).astype(np.float32) * F32(0.01)).astype(np.float32)
    F[8] = F32(rng.integers(-100, 100) / 16.0)
    return F, F32(rng.integers(0, 2560) / 4), F32(rng.integers(0, 1920) / 4), F32(rng.integers(0, 2560) / 4), int(rng.integers(0, 8))


def line_general_cases(want=4):
    """[(F12, x1, y1, x2, y2, octave, double verdict)] with den != 1 where the double and the float comparison disagree."""
    rng = np.random.default_rng(5)
    out = []
    while len(out) < want:
        F, x1, y1, x2, o = _random_geometry(rng)
        t64, t32 = 3.84 * float(S2[o]), F32(F32(3.84) * S2[o])
        _, a, b, c, den = _line_np(F, x1, y1, x2, F32(0))
        if den == 0 or b == 0 or den == 1:
            continue
        y0 = F32((np.sqrt(t64 * float(den)) - float(c) - float(a) * float(x2)) / float(b))
        if not 0 < y0 < 480:
            continue
        y2 = (y0 + np.arange(-3000, 3000, dtype=np.float32) * np.spacing(y0)).astype(np.float32)
        ds = _line_np(F, x1, y1, x2, y2)[0]
        j = np.nonzero((ds.astype(np.float64) < t64) != (ds < t32))[0]
        if len(j) and line_gate(F, x1, y1, x2, y2[j[0]], o) != line_gate(F, x1, y1, x2, y2[j[0]], o, double=False):
            out.append((F, float(x1), float(y1), float(x2), float(y2[j[0]]), o, bool(float(ds[j[0]]) < t64)))
    return out


def line_fma_cases(where, want=3):
    """[(F12, x1, y1, x2, y2, octave, verdict)]: the verdict of the line gate with one rounding per operation; rounding the
    product-then-add of `where` once -- whichever product is fused, there alone or in all three expressions -- gives the opposite."""
    rng = np.random.default_rng({'abc': 11, 'num': 12, 'den': 13}[where])
    out = []
    while len(out) < want:
        F, x1, y1, x2, o = _random_geometry(rng)
        t64 = 3.84 * float(S2[o])
        _, a, b, c, den = _line_np(F, x1, y1, x2, F32(0))
        if den == 0 or b == 0:
            continue
        y0 = F32((np.sqrt(t64 * float(den)) - float(c) - float(a) * float(x2)) / float(b))
        if not 0 < y0 < 480:
            continue
        y2 = (y0 + np.arange(-24, 24, dtype=np.float32) * np.spacing(y0)).astype(np.float32)
        ds = _line_np(F, x1, y1, x2, y2)[0]
        near = np.nonzero(np.abs(ds.astype(np.float64) - t64) < 4 * float(np.spacing(F32(t64))))[0]
        for j in near:
            v = line_gate(F, x1, y1, x2, y2[j], o)
            if v is not None and all(line_gate(F, x1, y1, x2, y2[j], o, f, w) == (not v) for f in (0, 1) for w in ((where,), ('abc', 'num', 'den'))):
                out.append((F, float(x1), float(y1), float(x2), float(y2[j]), o, v))
                break
    return out


def epipole_edge(o, dy):
    """The least float distex >= 0 that is NOT skipped at octave o for this distey: its float sum reaches 100 * mvScaleFactors[o]."""
    t = F32(100) * SF[o]
    dx0 = F32(np.sqrt(float(t) - float(dy) ** 2))
    dx = (dx0 + np.arange(-64, 64, dtype=np.float32) * np.spacing(dx0)).astype(np.float32)
    j = np.nonzero(~(dx * dx + F32(dy) * F32(dy) < t))[0][0]
    return float(dx[j]), float(dx[j - 1])


def epipole_fma_cases(want=4):
    """[(distex, distey, octave, skipped)]: the epipole sum with two roundings gives `skipped`; with one, whichever product is fused, the opposite."""
    out = []
    for o in range(8):
        t = F32(100) * SF[o]
        for dy in np.arange(2.25, 9.0, 0.375, dtype=np.float32) * SF[o]:
            dy = F32(dy * F32(1.0009765625))
            dx0 = F32(np.sqrt(float(t) - float(dy) ** 2))
            for dx in (dx0 + np.arange(-6, 6, dtype=np.float32) * np.spacing(dx0)).astype(np.float32):
                v = epipole_gate(dx, dy, 0, 0, o)
                if F32(dx - F32(0)) == dx and all(epipole_gate(dx, dy, 0, 0, o, f) == (not v) for f in (0, 1)):
                    out.append((float(dx), float(dy), o, v))
                    break
            if len(out) >= want:
                return out
    return out


def _tri(name, cands1, cands2, expect, geo, witness, fam='E'):
    return add(name, fam, 'tri', [(4, cands1, cands2)], expect, witness, geo=geo)


def _family_e():
    # ties: every gate open, the LAST candidate of least distance in list order wins (`dist>bestDist` is the skip test, :722)
    add('tie_last_in_list_order_wins_tri', 'E', 'tri', [(4, [0], [12, 10, 10, 30, 10, 11])], {0: 4})
    add('tie_at_th_low_last_wins_tri', 'E', 'tri', [(4, [0], [50, 50])], {0: 1})
    # a later tie that fails the line gate (y2 = 110: dsqr = 100 >= 3.84) does not displace the holder
    add('later_tie_failing_gate_does_not_displace_tri', 'E', 'tri', [(4, [0], [10, (10, 1, 12.0, 110.0)])], {0: 0})
    # a closer candidate that fails the gate does not stop a farther one that passes, before or after it
    add('closer_failing_gate_does_not_stop_farther_tri', 'E', 'tri', [(4, [0], [(5, 1, 11.0, 110.0), 10])], {0: 1})
    add('closer_failing_gate_after_farther_tri', 'E', 'tri', [(4, [0], [10, (5, 1, 12.0, 110.0)])], {0: 0})
    add('farther_after_closer_is_skipped_tri', 'E', 'tri', [(4, [0], [10, 12])], {0: 0})
    # epipole gate, octave 0: (6, 8) gives 36 + 64 = 100, not < 100 * 1.0f: NOT skipped.  One ulp nearer in y is skipped.  One ulp nearer in x
    # is NOT: 36 - 5.7e-6 rounds to 36 - 7.6e-6, and 100 - 7.6e-6 is the midpoint of two floats, which rounds (to even) back onto 100 -- a sum
    # in double would skip it; two ulps nearer in x are skipped.  The epipole is (6, 8), the keypoints lie at the origin and a few ulps of
    # 6 / 8 beside it; y1 = 0 keeps dsqr = y2^2 tiny.
    x1u, x2u = F32(6) - np.nextafter(F32(6), F32(0)), F32(6) - np.nextafter(np.nextafter(F32(6), F32(0)), F32(0))
    y1u = F32(8) - np.nextafter(F32(8), F32(0))
    for tag, x2, y2, skipped in [('at_6_8_exactly_100_not_skipped', 0.0, 0.0, False), ('one_ulp_nearer_in_x_float_sum_still_100_not_skipped', float(x1u), 0.0, False),
                                 ('two_ulps_nearer_in_x_skipped', float(x2u), 0.0, True), ('one_ulp_nearer_in_y_skipped', 0.0, float(y1u), True)]:
        def w(x2=x2, y2=y2, skipped=skipped, tag=tag):
            dx, dy = F32(6) - F32(x2), F32(8) - F32(y2)
            s = dx * dx + dy * dy
            ulps = round((6.0 - float(dx)) / float(x1u)) + round((8.0 - float(dy)) / float(y1u))
            return bool(s < F32(100) * SF[0]) == skipped and (skipped or s == F32(100)) and ulps == (0 if 'exactly' in tag else 2 if 'two' in tag else 1) \
                and epipole_gate(6, 8, x2, y2, 0) == skipped and (ulps == 0 or float(dx) ** 2 + float(dy) ** 2 < 100.0)
        _tri('epipole_octave_0_%s_tri' % tag, [(0, 1, 3.0, 0.0)], [(0, 1, x2, y2, 0)], {} if skipped else {0: 0}, dict(ex=6.0, ey=8.0), w)
    for o in (1, 4):
        dy = float(F32(5.0))
        far, near = epipole_edge(o, dy)
        for tag, dx, skipped in [('at_edge_not_skipped', far, False), ('one_ulp_nearer_skipped', near, True)]:
            def w(o=o, dx=dx, dy=dy, skipped=skipped):
                s = F32(dx) * F32(dx) + F32(dy) * F32(dy)
                return bool(s < F32(100) * SF[o]) == skipped and F32(100) * SF[o] != F32(100 * 1.2 ** o) and F32(F32(dx) - F32(0)) == F32(dx)
            _tri('epipole_octave_%d_%s_tri' % (o, tag), [(0, 1, 3.0, 0.0)], [(0, 1, 0.0, 0.0, o)], {} if skipped else {0: 0}, dict(ex=dx, ey=dy), w)
    # line gate: dsqr is a float, the comparison with 3.84 * sigma2 is in double (:149-151)
    for d, o, v in line_t_cases():
        def w(d=d, o=o, v=v):
            ds = F32(d) * F32(d)
            return bool(float(ds) < 3.84 * float(S2[o])) == v and bool(ds < F32(3.84) * S2[o]) != v and line_gate(T_OPEN['F12'], 3, 0, 9, d, o) == v
        _tri('line_gate_double_%s_float_%s_octave_%d_tri' % ('accepts' if v else 'rejects', 'rejects' if v else 'accepts', o),
             [(0, 1, 3.0, 0.0)], [(0, 1, 9.0, d, o)], {0: 0} if v else {}, None, w)
    for j, (F, x1, y1, x2, y2, o, v) in enumerate(line_general_cases()):
        def w(F=F, x1=x1, y1=y1, x2=x2, y2=y2, o=o, v=v):
            return line_gate(F, x1, y1, x2, y2, o) == v and line_gate(F, x1, y1, x2, y2, o, double=False) == (not v) and _line_np(F, F32(x1), F32(y1), F32(x2), F32(y2))[4] != 1
        _tri('line_gate_general_f12_double_%s_float_%s_case_%d_tri' % ('accepts' if v else 'rejects', 'rejects' if v else 'accepts', j),
             [(0, 1, x1, y1)], [(0, 1, x2, y2, o)], {0: 0} if v else {}, dict(F12=F), w)
    # den == 0 (:146): a zero F12, and a non-zero F12 whose a and b vanish for this kp1 (a = x1 - 3, b = y1 - 7 at (3, 7)); with
    # kp1 = (4, 7) the same matrix gives a = 1, b = 0, c = 0: num = x2, dsqr = x2^2 -- x2 = 1 passes
    Fv = [[1, 0, 0], [0, 1, 0], [-3, -7, 0]]
    _tri('den_zero_zero_f12_tri', [(0, 1, 3.0, 7.0)], [(0, 1, 1.0, 1.0, 0)], {}, dict(F12=np.zeros(9)), lambda: line_gate(np.zeros(9), 3, 7, 1, 1, 0) is None)
    _tri('den_zero_a_and_b_vanish_for_this_kp1_tri', [(0, 1, 3.0, 7.0)], [(0, 1, 1.0, 1.0, 0)], {}, dict(F12=Fv), lambda: line_gate(Fv, 3, 7, 1, 1, 0) is None)
    _tri('den_nonzero_same_f12_other_kp1_tri', [(0, 1, 4.0, 7.0)], [(0, 1, 1.0, 1.0, 0)], {0: 0}, dict(F12=Fv), lambda: line_gate(Fv, 4, 7, 1, 1, 0) is True)
    _tri('den_zero_only_for_one_of_two_tri', [(0, 1, 3.0, 7.0), (0, 1, 4.0, 7.0)], [(0, 1, 1.0, 1.0, 0)], {1: 0}, dict(F12=Fv),
         lambda: line_gate(Fv, 3, 7, 1, 1, 0) is None and line_gate(Fv, 4, 7, 1, 1, 0) is True)
    # one rounding per operation (the build's -ffp-contract=off)
    for where in ('abc', 'num', 'den'):
        for j, (F, x1, y1, x2, y2, o, v) in enumerate(line_fma_cases(where)):
            def w(F=F, x1=x1, y1=y1, x2=x2, y2=y2, o=o, v=v, where=where):
                return line_gate(F, x1, y1, x2, y2, o) == v and all(line_gate(F, x1, y1, x2, y2, o, f, (where,)) == (not v) for f in (0, 1))
            _tri('line_gate_one_rounding_per_operation_%s_case_%d_%s_tri' % (where, j, 'accepts' if v else 'rejects'), [(0, 1, x1, y1)], [(0, 1, x2, y2, o)],
                 {0: 0} if v else {}, dict(F12=F), w)
    for j, (dx, dy, o, v) in enumerate(epipole_fma_cases()):
        def w(dx=dx, dy=dy, o=o, v=v):
            return epipole_gate(dx, dy, 0, 0, o) == v and all(epipole_gate(dx, dy, 0, 0, o, f) == (not v) for f in (0, 1))
        _tri('epipole_one_rounding_per_operation_case_%d_%s_tri' % (j, 'skipped' if v else 'not_skipped'), [(0, 1, 3.0, 0.0)], [(0, 1, 0.0, 0.0, o)],
             {} if v else {0: 0}, dict(ex=dx, ey=dy), w)


# ==== F. rotation histogram ==================================================================================================
def _hist(name, kind, matches, keep, ori, witness):
    """matches: (angle1, angle2) per isolated pair, one node each.  For kf_frame the reference's histogram holds FRAME indices
    (rotHist[bin].push_back(bestIdxF), :240) where the other two hold idx1 (:609, :754); only the bin counts decide."""
    if kind == 'tri':
        nodes = [(i, [(0, 1, 10.0 + i, 100.0, 0, m[0])], [(0, 1, 10.0 + i, 100.0, 0, m[1])]) for i, m in enumerate(matches)]
    else:
        nodes = [(i, [(0, 1, m[0])], [(0, 1, m[1])]) for i, m in enumerate(matches)]
    add(name, 'F', kind, nodes, {i: i for i in keep}, witness, 'histogram of frame indices for kf_frame: only bin counts decide', ori=ori)


def _family_f():
    for kind in ALL:
        t = TAG[kind]
        for tag, cnt, kept_bins in HIST_COUNTS:
            matches, keep = [], []
            for b, c in enumerate(cnt):
                for _ in range(c):
                    if b in kept_bins:
                        keep.append(len(matches))
                    matches.append((30.0 * b, 0.0))

            def wit(cnt=cnt, matches=matches):
                h = {}
                for a1, a2 in matches:
                    h[rot_bin32(a1, a2)] = h.get(rot_bin32(a1, a2), 0) + 1
                return h == {b: c for b, c in enumerate(cnt) if c}
            _hist('histogram_%s_%s' % (tag, t), kind, matches, keep, True, wit)
            _hist('histogram_%s_check_ori_off_%s' % (tag, t), kind, matches, list(range(len(matches))), False, wit)
        for tag, a1, a2, want_bin in ROT_PROBES:
            others = [b for b in (4, 8, 6) if b != want_bin][:2]
            matches = []
            for b in [want_bin] + others:
                matches += [(350.0 if b == 12 else 30.0 * b, 0.0)] * 3
            matches.append((a1, a2))
            _hist('rotation_bin_%s_%s' % (tag, t), kind, matches, list(range(10)), True,
                  lambda a1=a1, a2=a2, want_bin=want_bin: rot_bin32(a1, a2) == want_bin and rot_bin32(350.0, 0.0) == 12)
        matches = [(0.0, 0.0)] * 3 + [(120.0, 0.0)] * 3 + [(240.0, 0.0)] * 3 + [(15.0, 0.0)]
        _hist('rotation_bin_diff_15_is_not_bin_0_%s' % t, kind, matches, list(range(9)), True, lambda: rot_bin32(15.0, 0.0) == 1)


# ==== G. routes and sizes ====================================================================================================
# cores of families A-C and E: (tag, kinds, side-1 items, side-2 items, {item of side 1: item of side 2}, ratio, boundary).  `boundary` restates
# the core's witness on the HOSTED arrays: d(i, j) is the Hamming distance of the descriptor rows that item i of side 1 and item j of side 2 have in
# the inflated scene, y1(i) / y2(j) their keypoints' y.  None has "second best absent" as its point: the kf_frame filler is a live candidate at >= 196.
def _lt(d1, r, d2):
    return bool(F32(d1) < F32(r) * F32(d2))


CORES = [('th_low_50', ('kf_frame', 'tri'), [0], [50], {0: 0}, 0.7, lambda d, y1, y2: d(0, 0) == 50 == TH_LOW),
         ('th_low_51', ('kf_frame', 'tri'), [0], [51], {}, 0.7, lambda d, y1, y2: d(0, 0) == 51 == TH_LOW + 1),
         ('th_low_49', ('kf_kf',), [0], [49], {0: 0}, 0.7, lambda d, y1, y2: d(0, 0) == 49 == TH_LOW - 1),
         ('th_low_50', ('kf_kf',), [0], [50], {}, 0.7, lambda d, y1, y2: d(0, 0) == 50 == TH_LOW),
         # the best exactly at the threshold and a second best that fails the ratio (50 < 0.7 * 60 = 42 fails): the threshold test must not end the decision
         ('th_low_50_second_60_ratio_rejects', ('kf_frame',), [0], [60, 50], {}, 0.7, lambda d, y1, y2: (d(0, 1), d(0, 0)) == (50, 60) and not _lt(50, 0.7, 60)),
         ('th_low_49_second_60_ratio_rejects', ('kf_kf',), [0], [60, 49], {}, 0.7, lambda d, y1, y2: (d(0, 1), d(0, 0)) == (49, 60) and not _lt(49, 0.7, 60)),
         ('tie_rejected', KF, [0], [10, 10], {}, 1.0, lambda d, y1, y2: d(0, 0) == d(0, 1) == 10 and not _lt(10, 1.0, 10)),
         ('tie_last_wins', ('tri',), [0], [10, 10, 10], {0: 2}, 0.7, lambda d, y1, y2: d(0, 0) == d(0, 1) == d(0, 2) == 10 and y2(0) == y2(1) == y2(2) == y1(0)),
         ('claimed_was_best', KF, [0, 20], [0, 45, 60], {0: 0, 1: 1}, 0.7,
          lambda d, y1, y2: d(0, 0) == 0 and (d(1, 0), d(1, 1), d(1, 2)) == (20, 25, 40) and _lt(25, 0.7, 40)),
         ('claimed_was_second', KF, [0, 5], [0, 9, 40], {0: 0, 1: 1}, 0.7,
          lambda d, y1, y2: d(0, 0) == 0 and (d(1, 0), d(1, 1), d(1, 2)) == (5, 4, 35) and not _lt(4, 0.7, 5) and _lt(4, 0.7, 35)),
         ('claimed_was_tie_in_front', KF, [0, 5], [0, 10, 40], {0: 0, 1: 1}, 0.7,
          lambda d, y1, y2: d(0, 0) == 0 and (d(1, 0), d(1, 1), d(1, 2)) == (5, 5, 35) and not _lt(5, 0.7, 5) and _lt(5, 0.7, 35)),
         ('claimed_was_irrelevant', KF, [0, 45], [0, 46, 40], {0: 0, 1: 1}, 0.7,
          lambda d, y1, y2: d(0, 0) == 0 and (d(1, 0), d(1, 1), d(1, 2)) == (45, 1, 5) and _lt(1, 0.7, 5)),
         ('ratio_float_0p6_24_40_rejects', KF, [0], [40, 24], {}, 0.6,
          lambda d, y1, y2: (d(0, 1), d(0, 0)) == (24, 40) and F32(0.6) * F32(40) == F32(24) and float(F32(0.6)) * 40.0 > 24.0),
         ('ratio_float_0p6_24_41_accepts', KF, [0], [41, 24], {0: 1}, 0.6, lambda d, y1, y2: (d(0, 1), d(0, 0)) == (24, 41) and _lt(24, 0.6, 41)),
         ('gate_closer_fails', ('tri',), [0], [(5, 1, 11.0, 110.0), 10], {0: 1}, 0.7,
          lambda d, y1, y2: (d(0, 0), d(0, 1)) == (5, 10) and float((y2(0) - y1(0)) ** 2) >= 3.84 * float(S2[0]) and y2(1) == y1(0))]
N_LARGE = K_SIDE + 44               # 300: a node beyond kBowSide on both sides, within every other limit
TILE = K_MATRIX // K_SIDE           # 48 frame-1 rows per matrix tile when n2g == kBowSide
SIZES = [(K_SIDE, K_SIDE), (K_SIDE + 1, K_SIDE), (K_SIDE, K_SIDE + 1), (K_SIDE + 1, K_SIDE + 1), (N_LARGE, K_REGS2), (N_LARGE, K_REGS2 + 1),
         (N_LARGE, K_LDS2), (N_LARGE, K_LDS2 + 1), (K_MATRIX, K_SIDE + 1), (K_MATRIX + 1, K_SIDE + 1)]


def _spread(k, n, shift):
    """k ascending positions in a list of n: the first, the last and interior ones (one probe: which of the three rotates with `shift`)."""
    if k == 1:
        return [[0, n // 2, n - 1][shift % 3]]
    return [0] + [n // 2 + j for j in range(k - 2)] + [n - 1]


def hosted_node(kind, s1, s2, n1g, n2g, pos1, pos2, node=6):
    """One node of n1g x n2g features with the core's items at the positions given and filler elsewhere.  Side-1 filler: flagged
    off, or -- every other one -- a live row(128), which finds nothing within TH_LOW.  Side-2 filler: flagged off (kf_kf, tri) or, for
    kf_frame, which has no flag, the complement of row(k), k = 0 ... 60: a live candidate at distance >= 196 from every probe."""
    g = (5.0, 100.0) if kind == 'tri' else ()
    f1 = [((128, 1) if j % 2 else (0, 0)) + g for j in range(n1g)]
    f2 = [((CPL + j % 61, 1) if kind == 'kf_frame' else (j % 61, 0)) + g for j in range(n2g)]
    for it, p in zip(s1, pos1):
        f1[p] = it
    for it, p in zip(s2, pos2):
        f2[p] = it
    return (node, f1, f2)


def hosted_inp(kind, s1, s2, n1g, n2g, pos1, pos2, ratio):
    return make_inp(kind, [hosted_node(kind, s1, s2, n1g, n2g, pos1, pos2)], ratio)


def hosted_witness(inp, kind, pos1, pos2, n1g, n2g, b1=0, b2=0, boundary=None):
    """Sizes as stated; live filler of side 2 lies at >= 196 from every probe; live filler of side 1 finds nothing within TH_LOW; and the
    core's own boundary, restated on the hosted rows."""
    def w():
        if boundary is not None:
            k1, k2 = (inp['kps1'], inp['kps2']) if kind == 'tri' else (None, None)
            if not boundary(lambda i, j: hamming(inp['desc1'][b1 + pos1[i]], inp['desc2'][b2 + pos2[j]]), lambda i: k1['y'][b1 + pos1[i]],
                            lambda j: k2['y'][b2 + pos2[j]]):
                return False
        tri = kind == 'tri'
        d2 = inp['desc2'][b2:b2 + n2g]
        on2 = (inp['has2'] == 0) if tri else (inp['valid2'] if inp['valid2'] is not None else np.ones(len(inp['desc2']), np.uint8))
        on1 = ((inp['has1'] == 0) if tri else inp['valid1'])[b1:b1 + n1g]
        on2 = np.asarray(on2)[b2:b2 + n2g]
        fill2, fill1 = np.setdiff1d(np.arange(n2g), pos2), np.setdiff1d(np.arange(n1g), pos1)
        ok = True
        for p in pos1:
            x = np.unpackbits(d2[fill2] ^ inp['desc1'][b1 + p][None, :], axis=1).sum(1)
            ok = ok and bool(((x >= 196) | (on2[fill2] == 0)).all())
        live1 = fill1[on1[fill1] != 0]
        if len(live1):
            x = np.unpackbits(d2 ^ inp['desc1'][b1 + live1[0]][None, :], axis=1).sum(1)
            ok = ok and bool((x > TH_LOW).all()) and bool((inp['desc1'][b1 + live1] == inp['desc1'][b1 + live1[0]]).all())
        k1, k2 = list(inp['fv1'][1]), list(inp['fv2'][1])
        return ok and n1g in [int(b - a) for a, b in zip(k1[:-1], k1[1:])] and n2g in [int(b - a) for a, b in zip(k2[:-1], k2[1:])]
    return w


def _host(name, kind, s1, s2, exp, n1g, n2g, ratio, shift=0, pos1=None, pos2=None, boundary=None):
    pos1 = pos1 or _spread(len(s1), n1g, shift)
    pos2 = pos2 or _spread(len(s2), n2g, shift + 1)
    inp = hosted_inp(kind, s1, s2, n1g, n2g, pos1, pos2, ratio)
    e = {pos1[a]: pos2[b] for a, b in exp.items()}        # one node: a feature's index IS its position in the list
    return add(name, 'G', kind, inp, e, hosted_witness(inp, kind, pos1, pos2, n1g, n2g, boundary=boundary))


def _family_g():
    k = 0
    for n1g, n2g in SIZES:
        for tag, kinds, s1, s2, exp, ratio, bnd in CORES:
            for kind in kinds:
                k += 1
                _host('%s_in_%dx%d_%s' % (tag, n1g, n2g, TAG[kind]), kind, s1, s2, exp, n1g, n2g, ratio, k, boundary=bnd)
    # the second matrix tile: n2g = kBowSide gives kBowMatrix / kBowSide = 48 rows per tile; the claim is made in tile 0, seen in a later tile
    for tag, kinds, s1, s2, exp, ratio, bnd in [c for c in CORES if c[0].startswith('claimed')]:
        for kind in kinds:
            _host('%s_claim_in_tile_0_seen_in_tile_1_%s' % (tag, TAG[kind]), kind, s1, s2, exp, 100, K_SIDE, ratio, pos1=[3, TILE], pos2=[0, 128, K_SIDE - 1],
                  boundary=bnd)
            _host('%s_claim_in_tile_0_seen_in_last_tile_%s' % (tag, TAG[kind]), kind, s1, s2, exp, K_SIDE, K_SIDE, ratio, pos1=[TILE - 1, K_SIDE - 1],
                  pos2=[5, 6, 250], boundary=bnd)
    # small and large nodes in one call (the small ones then take the upload route too): node 6 is large (257 x 300), nodes 2 and 9 hold one
    # feature per side.  Features are numbered in node order: node 2 is index 0 on both sides, node 6 follows from index 1, node 9 is 258 / 301.
    for kind in ALL:
        tri = kind == 'tri'
        s1, s2, exp = ([0], [10, 10, 10], {0: 2}) if tri else ([0, 20], [0, 45, 60], {0: 0, 1: 1})
        pos1, pos2 = _spread(len(s1), K_SIDE + 1, 1), _spread(len(s2), N_LARGE, 1)
        small = [(2, [(3, 1, 7.0, 100.0) if tri else 3], [(3, 1, 8.0, 100.0) if tri else 3]), (9, [(8, 1, 7.0, 100.0) if tri else 8], [(9, 1, 8.0, 100.0) if tri else 9])]
        inp = make_inp(kind, [small[0], hosted_node(kind, s1, s2, K_SIDE + 1, N_LARGE, pos1, pos2), small[1]], 0.7)
        e = {1 + pos1[a]: 1 + pos2[b] for a, b in exp.items()}
        e.update({0: 0, K_SIDE + 2: N_LARGE + 1})
        add('small_and_large_nodes_in_one_call_%s' % TAG[kind], 'G', kind, inp, e, hosted_witness(inp, kind, pos1, pos2, K_SIDE + 1, N_LARGE, 1, 1,
                                                                                       [c for c in CORES if c[0] == ('tie_last_wins' if tri else 'claimed_was_best')][0][6]))
    _topk_scenes()
    _limit_scenes()


def _topk_scenes():
    """The top-eight list of the large route, in a node of 300 x 300 with flagged filler (kf_kf), so the only candidates are the ones written.
    Z = row(0), the last item of side 1, is the feature under test; every A before it is the row of one candidate and takes it at distance 0
    (its second best is 1 or 2 away: 0 < ratio * that).  The A's sit in group 0 of the walk (positions 0-7); Z in group 2 (position 16) or, where
    seven A's leave room, next to them in ONE group of eight (position 7)."""
    N, G = N_LARGE, K_TOPK                                      # the walk decides G = 8 features at a time and lists G keys per feature
    cp = [10 + 3 * j for j in range(G + 1)]                     # positions of the candidates on side 2
    seven = {j: j + 1 for j in range(G - 1)}                    # A_j takes candidate j + 1
    for zpos, g in [(2 * G, 'other_group'), (G - 1, 'same_group')]:
        p1 = list(range(G - 1)) + [zpos]
        # candidates row(1) ... row(9); rows 2 ... 8 taken; Z sees row(1) at 1 free and the list's eighth at 8: 1 < 0.7 * 8 decides whatever lies beyond
        _host('topk_seven_taken_ratio_decided_by_the_eighth_%s_kfk' % g, 'kf_kf', [2, 3, 4, 5, 6, 7, 8, 0], list(range(1, 10)), {**seven, 7: 0}, N, N, 0.7,
              pos1=p1, pos2=cp, boundary=lambda d, y1, y2: [d(7, j) for j in range(9)] == list(range(1, 10)) and _lt(1, 0.7, 8))
        # ratio 0.6; candidates 24 | 26 28 30 32 34 36 38 | ninth; Z sees 24 free and the eighth at 38: 24 < 0.6f * 38 = 22.8 fails, so the list does
        # not decide and the node is rescanned: a ninth at 41 accepts (24 < 24.6); a ninth at 40 rejects (0.6f * 40 rounds onto 24: the float pair)
        for nine, ok in [(41, True), (40, False)]:
            c = [24, 26, 28, 30, 32, 34, 36, 38, nine]
            _host('topk_seven_taken_not_decided_rescan_ninth_%d_%s_%s_kfk' % (nine, 'accepts' if ok else 'rejects', g), 'kf_kf', c[1:8] + [0], c,
                  ({**seven, 7: 0} if ok else seven), N, N, 0.6, pos1=p1, pos2=cp,
                  boundary=lambda d, y1, y2, c=c, ok=ok: [d(7, j) for j in range(9)] == c and not _lt(24, 0.6, 38) and _lt(24, 0.6, c[8]) == ok
                  and (ok or (F32(0.6) * F32(40) == F32(24) and float(F32(0.6)) * 40.0 > 24.0)))
    eight = {j: j for j in range(8)}
    # all eight of Z's list taken (rows 1 ... 8 by their copies): a ninth at 20 is found by the rescan (second best absent); without it nothing is
    # free.  'other_group': the A's fill group 0, Z is the first of group 1 and reads all eight bits from the bitmap.  'shared_group': the A's sit at
    # positions 3 ... 10, Z at 11 -- three of the eight claims are made inside Z's own group, ahead of its rescan
    for p9, g in [(list(range(G)) + [G], 'other_group'), (list(range(3, G + 3)) + [G + 3], 'shared_group')]:
        b8 = lambda d, y1, y2: [d(8, j) for j in range(8)] == list(range(1, 9)) and all(d(j, j) == 0 for j in range(8))
        _host('topk_all_eight_taken_ninth_free_%s_kfk' % g, 'kf_kf', list(range(1, 9)) + [0], list(range(1, 9)) + [20], {**eight, 8: 8}, N, N, 0.7, pos1=p9, pos2=cp,
              boundary=lambda d, y1, y2: b8(d, y1, y2) and d(8, 8) == 20)
        _host('topk_all_eight_taken_none_free_%s_kfk' % g, 'kf_kf', list(range(1, 9)) + [0], list(range(1, 9)), eight, N, N, 0.7, pos1=p9, pos2=cp[:8], boundary=b8)
        # kf_frame: the complement filler keeps every list full; beyond the eight, the best free one is at >= 196 > TH_LOW
        _host('topk_all_eight_taken_ninth_free_%s_kff' % g, 'kf_frame', list(range(1, 9)) + [0], list(range(1, 9)) + [20], {**eight, 8: 8}, N, N, 0.7, pos1=p9, pos2=cp,
              boundary=lambda d, y1, y2: b8(d, y1, y2) and d(8, 8) == 20)
        _host('topk_all_eight_taken_none_within_th_low_%s_kff' % g, 'kf_frame', list(range(1, 9)) + [0], list(range(1, 9)), eight, N, N, 0.7, pos1=p9, pos2=cp[:8],
              boundary=b8)
    # a list shorter than eight: three valid candidates in the node
    _host('topk_list_shorter_than_eight_kfk', 'kf_kf', [0, 2], [0, 3, 30], {0: 0, 1: 1}, N, N, 0.7, pos1=[8, 17], pos2=[0, 150, 299])
    _host('topk_list_of_one_kfk', 'kf_kf', [0, 2], [1], {0: 0}, N, N, 0.7, pos1=[8, 17], pos2=[299])
    # two features P, Q of ONE group of eight (positions 8, 9) -- and of two groups (positions 7, 8) -- want the same candidate X
    for (pp, pq), g in [((8, 9), 'one_group'), ((7, 8), 'two_groups')]:
        for kind in KF:
            t = TAG[kind]
            # P = row(0) accepts X = row(0); Q = row(1) finds X gone and takes Y = row(30) at 29
            _host('conflict_earlier_accepts_%s_%s' % (g, t), kind, [0, 1], [0, 30], {0: 0, 1: 1}, N, N, 0.7, pos1=[pp, pq], pos2=[4, 200])
            # P = row(0) rejects X = row(10) (the next at 11: 10 < 7.7 fails); Q = row(10) takes X at 0
            _host('conflict_earlier_rejects_%s_%s' % (g, t), kind, [0, 10], [10, 11], {1: 0}, N, N, 0.7, pos1=[pp, pq], pos2=[4, 200])
            # X is only Q's second best: Q = row(5) sees W = row(9) at 4, X = row(0) at 5 (4 < 3.5 fails while X is free), V = row(40) at 35
            _host('conflict_only_second_best_%s_%s' % (g, t), kind, [0, 5], [0, 9, 40], {0: 0, 1: 1}, N, N, 0.7, pos1=[pp, pq], pos2=[4, 100, 200])


    # a conflict sends the group to the one-by-one loop; there a third feature R has its best EXACTLY at the threshold and a free second best
    # that fails the ratio.  Side 2: X = row(0), A = row(4), B = row(10), D = row(8).  P = row(0) takes X (0 < 0.7 * 4); Q = row(1) would take X
    # too (1 < 0.7 * 3) and, X gone, takes A at 3 (3 < 0.7 * 7); R = row(60) / row(59) sees B at 50 / 49 and D at 52 / 51: 50 < 36.4 fails --
    # the threshold test must not end the decision with the second best still at 256
    for kind, r in (('kf_frame', 60), ('kf_kf', 59)):
        _host('conflict_group_third_feature_best_at_threshold_second_fails_ratio_%s' % TAG[kind], kind, [0, 1, r], [0, 4, 10, 8], {0: 0, 1: 1}, N, N, 0.7,
              pos1=[8, 9, 10], pos2=[4, 100, 200, 250],
              boundary=lambda d, y1, y2, kind=kind: d(2, 2) == (TH_LOW if kind == 'kf_frame' else TH_LOW - 1) and d(2, 3) == d(2, 2) + 2 and not _lt(d(2, 2), 0.7, d(2, 3))
              and d(0, 0) == 0 and d(1, 0) == 1 and d(1, 1) == 3 and _lt(1, 0.7, 3))


def _limit_scenes():
    # one node with n1g = 1 and n2g = 65 535 (the position field of the key is full); the only match is the last position
    for kind in KF:
        _host('node_of_65535_only_match_at_last_position_%s' % TAG[kind], kind, [0], [7], {0: 0}, 1, K_GROUP, 0.7, pos1=[0], pos2=[K_GROUP - 1])
    _host('node_of_65535_tie_of_first_and_last_position_ratio_1p5_kfk', 'kf_kf', [0], [7, 7], {0: 0}, 1, K_GROUP, 1.5, pos1=[0], pos2=[0, K_GROUP - 1])
    # tri in nodes of 257 (the global-memory form)
    _host('tie_last_wins_first_and_last_feature_of_257x257_tri', 'tri', [0, 0], [10, 10, 10], {0: 2, 1: 2}, 257, 257, 0.7, pos1=[0, 256], pos2=[0, 130, 256])
    _host('th_low_51_and_50_in_257x1_tri', 'tri', [0, 1], [51], {1: 0}, 257, 1, 0.7, pos1=[0, 256], pos2=[0])
    _host('gate_closer_fails_in_1x257_tri', 'tri', [0], [(5, 1, 11.0, 110.0), 10], {0: 1}, 1, 257, 0.7, pos1=[0], pos2=[100, 256])


def overflow_inp(kind):
    """65 536 features under one node on side 2: refused with ORBFE_ERR_OVERFLOW."""
    return hosted_inp(kind, [0], [7], 1, K_GROUP + 1, [0], [K_GROUP], 0.7)


# ==== batches ================================================================================================================
def companions(kind):
    """Two small scenes whose result depends on neither the ratio (>= 0.5) nor check_orientation: one match each at distance 0 with no second."""
    a = make_inp(kind, [(1, [3], [3])])
    b = make_inp(kind, [(1, [(9, 0)], [9]), (2, [20, (21, 0)], [20])])
    return (a, (1, [0])), (b, (1, [-1, 1, -1]))


def merge_batch(kind, members):
    """Side 2 of a batch: the members' side-2 features one after the other.  Node ids are renumbered so that the members' nodes are
    disjoint and both FeatureVectors stay ascending: member k's j-th smallest id (of either side) becomes 100000 k + j.
    Returns (sides1, desc2, angle2, valid2, fv2, [side-2 index offset per member])."""
    sides, d2, a2, v2, ids, off, feat, base = [], [], [], [], [], [0], [], []
    for k, i in enumerate(members):
        b = sum(len(x) for x in d2)
        base.append(b)
        rank = {n: 100000 * k + j for j, n in enumerate(sorted(set(int(x) for x in i['fv1'][0]) | set(int(x) for x in i['fv2'][0])))}
        sides.append((i['desc1'], i['angle1'], i['valid1'], (np.array([rank[int(n)] for n in i['fv1'][0]], np.uint32), i['fv1'][1], i['fv1'][2])))
        d2.append(i['desc2'])
        a2.append(i['angle2'])
        v2.append(i['valid2'] if i['valid2'] is not None else np.ones(len(i['desc2']), np.uint8))
        ids += [rank[int(n)] for n in i['fv2'][0]]
        off += [int(o) + len(feat) for o in i['fv2'][1][1:]]
        feat += list(i['fv2'][2].astype(np.int64) + b)
    fv2 = (np.array(ids, np.uint32), np.array(off, np.uint32), np.array(feat, np.uint32))
    return sides, np.concatenate(d2), np.concatenate(a2), np.concatenate(v2) if kind == 'kf_kf' else None, fv2, base


_family_a()
_family_b()
_family_c()
_family_d()
_family_e()
_family_f()
_family_g()
