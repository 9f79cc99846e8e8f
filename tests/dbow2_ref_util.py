"""Shared by tests/test_dbow2_ref.py, tests/test_gpu_dbow2_ref.py and tools/gen_dbow2_voc_golden.py: the cases that hold the vocabulary
descent and the BoW scores to the REFERENCE'S OWN DBoW2 code (oracle/_ref/libdbow2_voc.so: TemplatedVocabulary.h + ScoringObject.cpp
compiled from the reference's sources by oracle/Makefile), and the committed record of what that code returned for them
(tests/golden/dbow2_voc_outputs.npz), which stands in where the object is absent.

Transform cases: 5 vocabulary images x the 24 (scoring, weighting) headers x levelsup 0 .. L + 1 x 9 descriptor sets.  A result is
compared in its canonical form (canon()): BowVector ids and doubles, FeatureVector, per-feature word and node, byte for byte -- with
one carve-out that the reference's code forces.  Its batch transform declares `NodeId nid;` without a value and the single-feature
transform writes it only when the descent passes level L - levelsup; for a feature whose word lies ABOVE that level (possible only in
a tree with leaves at unequal depths) the batch transform files the feature under an indeterminate node (the object built here
happens to reuse the previous feature's).  Such features are found by the reference's own single-feature transform (its node id comes
back untouched, NID_UNWRITTEN); the oracle and the product file them under node 0.  canon() takes exactly these features out of the
FeatureVector on both sides and keeps everything else; that both sides agree on WHICH features they are is part of the comparison
(the per-feature node array carries NID_UNWRITTEN for them)."""
import hashlib
import os

import numpy as np

import kfdb_util as K
from bow_util import ragged_vocabulary, with_header
from os1_amd.synth import synth_vocabulary

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dbow2_voc_outputs.npz')
NID_UNWRITTEN = 0xffffffff
HEADERS = [(s, w) for s in range(6) for w in range(4)]
VOCS = ('synth3_10_4', 'ragged4', 'synth8_19_2', 'ragged31_4_3', 'dup12_7_2')
RAGGED = ('ragged4', 'ragged31_4_3')
SET_NAMES = ('n0', 'n1', 'n17', 'n63', 'n64', 'n65', 'n1500', 'exact', 'equi')
SCORINGS = (K.L1, K.L2, K.CHI, K.KL, K.BHATTA, K.DOT)
ACCEPTED = (K.L1, K.L2, K.CHI, K.DOT)          # the four the keyframe database accepts

_CACHE = {}


def voc_image(name):
    """the vocabulary image of a case, header (0, 0)"""
    if name not in _CACHE:
        from test_bow_oracle import _with_trailing_duplicate
        _CACHE[name] = {'synth3_10_4': lambda: synth_vocabulary(3, 10, 4), 'ragged4': lambda: ragged_vocabulary(4),
                        'synth8_19_2': lambda: synth_vocabulary(8, 19, 2), 'ragged31_4_3': lambda: ragged_vocabulary(31, k=4, L=3),
                        'dup12_7_2': lambda: _with_trailing_duplicate(synth_vocabulary(12, 7, 2))}[name]()
    return _CACHE[name]


def _records(image):
    rec = np.frombuffer(image, np.uint8, offset=4).reshape(-1, 45)
    return rec[:, 0:4].copy().view('<i4').ravel(), rec[:, 5:37]


def exact_descs(image, n=64):
    """descriptors equal to a node's own descriptor (distance 0), first and last record included"""
    _, desc = _records(image)
    return desc[np.unique(np.linspace(0, len(desc) - 1, n).astype(np.int64))].copy()


def equidistant_descs(image, n=64):
    """descriptors at the same distance from two sibling children, so that the first-child-wins rule decides: a sibling's descriptor
    with half of the bits flipped in which it differs from the next sibling.  Pairs that differ in an odd number of bits have no
    equidistant descriptor and are passed over."""
    parent, desc = _records(image)
    pairs = np.flatnonzero(parent[:-1] == parent[1:])
    pairs = pairs[np.unique(np.linspace(0, len(pairs) - 1, 2 * n).astype(np.int64))]
    out = []
    for i in pairs:
        a, b = np.unpackbits(desc[i]), np.unpackbits(desc[i + 1])
        diff = np.flatnonzero(a != b)
        if len(diff) == 0 or len(diff) % 2:
            continue
        d = a.copy()
        d[diff[:len(diff) // 2]] ^= 1
        assert int((d != a).sum()) == int((d != b).sum())
        out.append(np.packbits(d))
    return np.asarray(out[:n], np.uint8).reshape(-1, 32)


def desc_sets(name):
    key = ('sets', name)
    if key not in _CACHE:
        from test_bow_oracle import _descs
        image = voc_image(name)
        s = {'n0': np.zeros((0, 32), np.uint8), 'exact': exact_descs(image), 'equi': equidistant_descs(image)}
        for n in (1, 17, 63, 64, 65, 1500):
            s['n%d' % n] = _descs(n, image, n)
        assert tuple(s) != () and set(s) == set(SET_NAMES) and len(s['equi']) > 0
        _CACHE[key] = s
    return _CACHE[key]


def inputs_digest(name):
    h = hashlib.sha256(bytes(voc_image(name)))
    for sn in SET_NAMES:
        h.update(np.ascontiguousarray(desc_sets(name)[sn]).tobytes())
    return h.hexdigest()


def transform_cases(name):
    """(scoring, weighting, levelsup, set name) of every case of a vocabulary, in the order the golden file records them"""
    L = voc_image(name)[1]
    return [(s, w, lu, sn) for s, w in HEADERS for lu in range(L + 2) for sn in SET_NAMES]


def canon(res, L, levelsup):
    """The comparable form of a transform result (see the module docstring): [ids, values, fv nodes, fv offsets, fv features,
    word of feature, node of feature], the features without a written node id marked NID_UNWRITTEN and taken out of the FeatureVector."""
    ids, vals, (fvn, fvo, fvf), wof, nof = res
    nof = np.array(nof, np.uint32)
    if L - levelsup > 0:
        nof[nof == 0] = NID_UNWRITTEN        # node 0 is never WRITTEN below the root level: the oracle's and the product's "none"
    unwritten = nof == NID_UNWRITTEN
    fvf = np.asarray(fvf, np.uint32)
    node_of_entry = np.repeat(np.asarray(fvn, np.uint32), np.diff(np.asarray(fvo, np.int64)))
    keep = ~unwritten[fvf] if len(fvf) else np.zeros(0, bool)
    nodes, counts = np.unique(node_of_entry[keep], return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return [np.asarray(ids, np.uint32), np.asarray(vals, np.float64), nodes.astype(np.uint32), off, fvf[keep],
            np.asarray(wof, np.uint32), nof]


CANON_NAMES = ('bow ids', 'bow values', 'fv nodes', 'fv offsets', 'fv features', 'word of feature', 'node of feature')


def digest(c):
    h = hashlib.sha256()
    for a in c:
        h.update(np.int64(a.size).tobytes() + np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint8)


def assert_same(got, want, what):
    for name, a, b in zip(CANON_NAMES, got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, name)


class Reference:
    """What the reference's code returns for the cases: computed by oracle/_ref/libdbow2_voc.so where it is present (and then also
    checked against the committed record), else read from the record."""

    def __init__(self, live=None):
        from oracle import pyoracle
        self.live = pyoracle.have_dbow2_voc() if live is None else live
        self.rec = np.load(GOLDEN) if os.path.exists(GOLDEN) else None
        assert self.live or self.rec is not None, 'neither oracle/_ref/libdbow2_voc.so nor tests/golden/dbow2_voc_outputs.npz'

    def transforms(self, name):
        """yields ((scoring, weighting, levelsup, set name), image, descriptors, check) of every case; check(result, what) holds a
        transform result (api / oracle layout) to the reference's"""
        from oracle import pyoracle
        base, sets, cases = voc_image(name), desc_sets(name), transform_cases(name)
        L = base[1]
        rec = None
        if self.rec is not None:
            assert str(self.rec[name + '_in']) == inputs_digest(name), 'the golden file was recorded for other inputs: ' + name
            rec = self.rec[name + '_digests']
            assert rec.shape == (len(cases), 8)
        voc, header = None, None
        for i, (s, w, lu, sn) in enumerate(cases):
            if header != (s, w):
                header, image = (s, w), with_header(base, s, w)
                if self.live:
                    voc = pyoracle.Dbow2Vocabulary(image)
            want = canon(voc.transform(sets[sn], lu), L, lu) if self.live else None
            if self.live and rec is not None:
                assert digest(want).tobytes() == rec[i].tobytes(), ('the reference object and the golden file disagree', name, s, w, lu, sn)

            def check(result, what, want=want, i=i, lu=lu):
                got = canon(result, L, lu)
                if name not in RAGGED:
                    assert not (got[6] == NID_UNWRITTEN).any(), what
                if want is not None:
                    assert_same(got, want, what)
                else:
                    assert digest(got).tobytes() == rec[i].tobytes(), what
            yield (s, w, lu, sn), image, sets[sn], check


# ---- scores -----------------------------------------------------------------------------------------------------------------------
SCORE_WORDS = 60000


def score_pairs():
    """[(name, (words1, values1), (words2, values2))]: the shapes ScoringObject.cpp's merge walk and k_kfdb_query can get wrong, then every
    (probe, keyframe) pair of kfdb_util.scenes()."""
    if 'pairs' in _CACHE:
        return _CACHE['pairs']
    rng = np.random.default_rng(2024)

    def vec(words):
        words = np.asarray(sorted(set(int(w) for w in words)), np.uint32)
        return words, K.values_for(rng, len(words))

    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float64))
    a, b = vec(range(0, 400, 2)), vec(range(1, 400, 2))
    pairs = [('disjoint', a, b), ('identical', a, (a[0].copy(), a[1].copy())), ('empty_second', a, empty), ('empty_first', empty, a),
             ('both_empty', empty, empty)]
    pairs.append(('common_first_only', vec([3] + list(range(10, 200, 2))), vec([3] + list(range(11, 200, 2)))))
    pairs.append(('common_last_only', vec(list(range(10, 200, 2)) + [900]), vec(list(range(11, 200, 2)) + [900])))
    pairs.append(('common_first_of_one_last_of_other', vec([500] + list(range(600, 700))), vec(list(range(100, 200)) + [500])))
    pairs.append(('single_words', vec([7]), vec([7])))
    common = rng.choice(5000, 100, replace=False)
    pairs.append(('above_64', vec(list(common) + list(rng.choice(np.arange(5000, 9000), 100, replace=False))),
                  vec(list(common) + list(rng.choice(np.arange(9000, 13000), 130, replace=False)))))
    common = rng.choice(30000, 3000, replace=False)
    pairs.append(('above_4096', vec(list(common) + list(rng.choice(np.arange(30000, 45000), 2000, replace=False))),
                  vec(list(common) + list(rng.choice(np.arange(45000, SCORE_WORDS), 1100, replace=False)))))
    assert len(pairs[-1][1][0]) > 4096 and len(pairs[-1][2][0]) > 4096
    # chi-square's `vi + wi != 0` guard: opposite values and both zero at common words (values as given, not normalised)
    w = np.arange(20, 140, dtype=np.uint32)
    v1, v2 = K.values_for(rng, len(w)), K.values_for(rng, len(w))
    v2[::3] = -v1[::3]
    v1[1::3] = 0.0
    v2[1::3] = 0.0
    pairs.append(('chi_zero_sums', (w, v1), (w.copy(), v2)))
    for sname, scene in K.scenes().items():
        for j, (qw, qv) in enumerate(scene['probes']):
            for k in scene['kfs']:
                pairs.append(('scene/%s/p%d/k%d' % (sname, j, k['index']), (qw, qv), (k['words'], k['values'])))
    _CACHE['pairs'] = pairs
    return pairs


def pairs_digest():
    h = hashlib.sha256()
    for _, (w1, v1), (w2, v2) in score_pairs():
        for a, t in ((w1, np.uint32), (v1, np.float64), (w2, np.uint32), (v2, np.float64)):
            h.update(np.int64(len(a)).tobytes() + np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def tiny_vocabulary(scoring):
    """a two-word vocabulary whose header makes the reference's loader create the scoring object asked for"""
    return with_header(synth_vocabulary(1, 2, 1), scoring, 0)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def reference_scores(ref):
    """(pairs, 6) score bits of every pair under every scoring type, column = DBoW2 ScoringType: live where the object is present
    (then also held to the record for the four accepted scorings), else the record."""
    from oracle import pyoracle
    pairs = score_pairs()
    rec = None
    if ref.rec is not None:
        assert str(ref.rec['scores_in']) == pairs_digest(), 'the golden file was recorded for other score pairs'
        rec = ref.rec['scores']
        assert rec.shape == (len(pairs), 6)
    if not ref.live:
        return rec
    out = np.zeros((len(pairs), 6), np.uint64)
    for s in SCORINGS:
        voc = pyoracle.Dbow2Vocabulary(tiny_vocabulary(s))
        assert voc.info()['scoring'] == s
        out[:, s] = bits([voc.score(w1, v1, w2, v2) for _, (w1, v1), (w2, v2) in pairs])
        voc.close()
    if rec is not None:
        assert out[:, list(ACCEPTED)].tobytes() == rec[:, list(ACCEPTED)].tobytes(), 'the reference object and the golden file disagree'
    return out


# ---- the keyframe database against the reference's score ------------------------------------------------------------------------
KFDB_SIZES = (0, 1, 63, 64, 65, 300)


def kfdb_case():
    """About 70 keyframes of 0, 1, 63, 64, 65 and 300 words (the last block of k_kfdb_query has idle waves) and two queries, one at the
    kernel's LDS budget and one a word above it; keyframe `tomb` is erased for good, `readd` erased and added again, which the pool
    (capacity = the entries of all keyframes) can only take after a compaction."""
    if 'kfdb' not in _CACHE:
        rng = np.random.default_rng(77)
        qw = np.sort(rng.choice(SCORE_WORDS, K.QUERY_LDS_WORDS + 1, replace=False)).astype(np.uint32)
        rest = np.setdiff1d(np.arange(SCORE_WORDS), qw)
        queries = [(qw[:K.QUERY_LDS_WORDS].copy(), K.values_for(rng, K.QUERY_LDS_WORDS)), (qw, K.values_for(rng, len(qw)))]
        kfs = []
        for i in range(70):
            n = KFDB_SIZES[i % len(KFDB_SIZES)]
            c = int(rng.integers(0, n + 1)) if i % 5 else n // 2
            words = np.sort(np.concatenate([rng.choice(qw, c, replace=False), rng.choice(rest, n - c, replace=False)])).astype(np.uint32)
            kfs.append((words, K.values_for(rng, n)))
        kfs[5] = (qw[-1:].copy(), np.ones(1))            # shares only the longer query's last word
        kfs[11] = (qw[:300].copy(), queries[1][1][:300] / np.sum(queries[1][1][:300]))
        _CACHE['kfdb'] = dict(queries=queries, kfs=kfs, tomb=17, readd=23, cap_e=sum(len(w) for w, _ in kfs))
    return _CACHE['kfdb']


def kfdb_reference_scores(ref):
    """(6, queries, keyframes) bits of the reference's score(query, keyframe), first index = DBoW2 ScoringType"""
    from oracle import pyoracle
    case = kfdb_case()
    rec = ref.rec['kfdb_scores'] if ref.rec is not None else None
    if not ref.live:
        return rec
    out = np.zeros((6, len(case['queries']), len(case['kfs'])), np.uint64)
    for s in SCORINGS:
        voc = pyoracle.Dbow2Vocabulary(tiny_vocabulary(s))
        for j, (qw, qv) in enumerate(case['queries']):
            out[s, j] = bits([voc.score(qw, qv, w, v) for w, v in case['kfs']])
    if rec is not None:
        assert out[list(ACCEPTED)].tobytes() == rec[list(ACCEPTED)].tobytes(), 'the reference object and the golden file disagree'
    return out


# ---- descriptors of extracted frames: the fused routes and the chain ---------------------------------------------------------------
def frame_case(name):
    """vocabulary image, levelsup, nfeatures and frames of a fused-route / chain case (the shapes of tests/test_gpu_bow.py's fused tests)"""
    from os1_amd.synth import shifted, synth
    if ('frame', name) not in _CACHE:
        if name == 'extractor':
            c = dict(image=synth_vocabulary(4, 10, 5), levelsup=3, nfeatures=900, size=(800, 600), frames=[synth(31, 800, 600)])
        elif name == 'stream':
            base = synth(61, 800, 600)
            c = dict(image=synth_vocabulary(9, 10, 4), levelsup=2, nfeatures=700, size=(800, 600),
                     batch=3,
                     frames=[base] + [shifted(base, 3 * i, -2 * i, 900 + i) for i in range(1, 6)])
        else:
            c = dict(image=voc_image('synth3_10_4'), levelsup=4, nfeatures=1000, size=(640, 480), frames=[synth(1, 640, 480)])
        _CACHE[('frame', name)] = c
    return _CACHE[('frame', name)]


FRAME_CASES = ('extractor', 'stream', 'chain')
CHAIN_KEYFRAMES = 12


def chain_subsets(n):
    """rows of the frame's n descriptors that make up the chain's keyframes, and last the query frame's"""
    rng = np.random.default_rng(9)
    return [rng.choice(n, int(rng.integers(40, 200)), replace=False) for _ in range(CHAIN_KEYFRAMES + 1)]


def _desc_digest(desc):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(desc, np.uint8).tobytes()).digest()[:8], np.uint8)


def frame_check(ref, name, i, desc):
    """-> check(result, what) for the transform of frame i's descriptors (as the GPU extracted them) of a frame case"""
    from oracle import pyoracle
    c = frame_case(name)
    L, lu = c['image'][1], c['levelsup']
    if ref.live:
        if 'voc' not in c:
            c['voc'] = pyoracle.Dbow2Vocabulary(c['image'])
        want = canon(c['voc'].transform(desc, lu), L, lu)
        return lambda result, what: assert_same(canon(result, L, lu), want, what)
    assert _desc_digest(desc).tobytes() == ref.rec['frame_%s_in' % name][i].tobytes(), 'the golden file was recorded for other descriptors'
    want = ref.rec['frame_%s_digests' % name][i]

    def check(result, what):
        assert digest(canon(result, L, lu)).tobytes() == want.tobytes(), what
    return check


def chain_reference(ref, desc):
    """the reference's side of the chain on the frame's descriptors: -> ([check(result, what) per subset], score bits of (query, keyframe i))"""
    from oracle import pyoracle
    c = frame_case('chain')
    L, lu = c['image'][1], c['levelsup']
    subsets = chain_subsets(len(desc))
    if ref.live:
        if 'voc' not in c:
            c['voc'] = pyoracle.Dbow2Vocabulary(c['image'])
        res = [c['voc'].transform(desc[rows], lu) for rows in subsets]
        checks = [lambda result, what, w=canon(r, L, lu): assert_same(canon(result, L, lu), w, what) for r in res]
        q = res[-1]
        return checks, bits([c['voc'].score(q[0], q[1], r[0], r[1]) for r in res[:-1]])
    assert _desc_digest(desc).tobytes() == ref.rec['frame_chain_in'][0].tobytes(), 'the golden file was recorded for other descriptors'

    def mk(want):
        def check(result, what):
            assert digest(canon(result, L, lu)).tobytes() == want.tobytes(), what
        return check
    return [mk(w) for w in ref.rec['chain_digests']], ref.rec['chain_scores']
