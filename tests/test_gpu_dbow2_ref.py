"""-m gpu: the vocabulary descent (k_bow_descend: orbfe_bow_transform and the routes fused behind the descriptor kernel and into the
stream runner) and the keyframe database's scores (k_kfdb_query: orbfe_kfdb_query / orbfe_kfdb_score) against the REFERENCE'S OWN
DBoW2 code, with no oracle in between: oracle/_ref/libdbow2_voc.so (TemplatedVocabulary.h's loader and transform, ScoringObject.cpp's
scores) where it is present, else what it returned for the same inputs (tests/golden/dbow2_voc_outputs.npz).  BowVector doubles and
scores byte for byte.  Cases and the one carve-out (features whose node id the reference never writes): tests/dbow2_ref_util.py."""
import numpy as np
import pytest

import dbow2_ref_util as U
import kfdb_util as K

pytestmark = pytest.mark.gpu
KEY0 = 5000


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def ref():
    return U.Reference()


@pytest.mark.parametrize('name', U.VOCS)
def test_bow_transform_equals_reference_transform(api, ref, name):
    """every vocabulary image x header x levelsup 0 .. L + 1 x descriptor set (n = 0, 1, 17, 63, 64, 65, 1500, exact node descriptors,
    descriptors equidistant from two siblings)"""
    v, header, n = None, None, 0
    for (s, w, lu, sn), image, d, check in ref.transforms(name):
        if header != (s, w):
            if v is not None:
                v.close()
            header, v = (s, w), api.Vocabulary(image)
            assert v.info()['n_nodes'] == (len(image) - 4) // 45 + 1
        check(v.transform(d, lu), (name, s, w, lu, sn))
        n += 1
    v.close()
    assert n == len(U.transform_cases(name))


def test_extractor_fused_descent_equals_reference_transform(api, ref):
    c = U.frame_case('extractor')
    v = api.Vocabulary(c['image'])
    ex = api.Extractor(c['nfeatures'], 1.2, 8, 20, 7)
    ex.set_vocabulary(v, c['levelsup'])
    k, d = ex(c['frames'][0])
    assert len(k) > 500
    U.frame_check(ref, 'extractor', 0, d)(ex.bow(0, len(k)), 'extractor')
    v.close()


def test_stream_fused_descent_equals_reference_transform(api, ref):
    c = U.frame_case('stream')
    W, H = c['size']
    B = c['batch']
    v = api.Vocabulary(c['image'])
    dev = api.DeviceFrames(c['frames'], 0)
    st = api.Stream(c['nfeatures'], 1.2, 8, 20, 7, 0, B, 2)
    st.set_matching((0.0, float(W), 0.0, float(H)), 100, 0.9, True)
    st.set_vocabulary(v, c['levelsup'])
    for b in range(2):
        st.push_ptrs(dev.ptrs[b * B:(b + 1) * B], H, W, dev.stride, True)
    for b in range(2):
        kps, desc, n, m12, nm = st.pop(copy=True)
        for i in range(B):
            leaf, node = st.bow_raw(i)
            assert len(leaf) == n[i] and n[i] > 300
            U.frame_check(ref, 'stream', b * B + i, desc[i, :n[i]])(v.assemble(leaf, node), ('stream', b, i))
    st.close()
    v.close()


def _expected(queries_kfs, live_order, scores):
    """the reference's lKFsSharingWords for a query: keyframes with a common word, by (first common word, add order); common-word
    counts are a set intersection of the two BowVectors"""
    qw, kfs = queries_kfs
    q = set(qw.tolist())
    rows = []
    for seq, i in enumerate(live_order):
        common = q & set(kfs[i][0].tolist())
        if common:
            rows.append((min(common), seq, i, len(common), int(scores[i])))
    rows.sort()
    return [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows]


@pytest.mark.parametrize('scoring', U.ACCEPTED)
def test_kfdb_query_and_score_equal_reference_score(api, ref, scoring):
    case = U.kfdb_case()
    want = U.kfdb_reference_scores(ref)[scoring]
    kfs = case['kfs']
    db = api.KeyFrameDatabase(U.SCORE_WORDS, scoring, len(kfs), case['cap_e'])
    for i, (w, v) in enumerate(kfs):
        db.add(KEY0 + i, w, v)
    order = list(range(len(kfs)))
    db.erase(KEY0 + case['tomb'])
    db.erase(KEY0 + case['readd'])
    order.remove(case['tomb'])
    order.remove(case['readd'])
    db.add(KEY0 + case['readd'], *kfs[case['readd']])        # the tail stands at the capacity: fits only after a compaction
    order.append(case['readd'])
    assert db.size() == (len(order), sum(len(kfs[i][0]) for i in order))
    for j, (qw, qv) in enumerate(case['queries']):
        assert len(qw) == K.QUERY_LDS_WORDS + j
        ek, ec, es = _expected((qw, kfs), order, want[j])
        keys, common, scores = db.query(qw, qv)
        assert len(ek) > 40
        assert (keys.astype(np.int64) - KEY0).tolist() == ek and common.tolist() == ec
        assert U.bits(scores).tolist() == es
        got = db.score(qw, qv, [KEY0 + i for i in order])      # every live keyframe, also those without a common word
        assert U.bits(got).tolist() == [int(want[j][i]) for i in order]
    db.close()


def test_chain_descriptors_to_scores_equals_reference_chain(api, ref):
    """descriptors of one extracted 640 x 480 frame -> orbfe_bow_transform -> add -> query; the reference from the same descriptors with
    its own loader, descent and score"""
    c = U.frame_case('chain')
    ex = api.Extractor(c['nfeatures'], 1.2, 8, 20, 7)
    k, d = ex(c['frames'][0])
    assert len(k) > 500
    checks, want = U.chain_reference(ref, d)
    v = api.Vocabulary(c['image'])
    bows = []
    for i, rows in enumerate(U.chain_subsets(len(d))):
        res = v.transform(d[rows], c['levelsup'])
        checks[i](res, ('chain', i))
        bows.append((res[0].copy(), res[1].copy()))
    n_kf = U.CHAIN_KEYFRAMES
    db = api.KeyFrameDatabase(v.info()['n_words'], K.L1, n_kf, sum(len(w) for w, _ in bows[:n_kf]))
    for i, (w, val) in enumerate(bows[:n_kf]):
        db.add(KEY0 + i, w, val)
    qw, qv = bows[n_kf]
    ek, ec, es = _expected((qw, bows), list(range(n_kf)), want)
    keys, common, scores = db.query(qw, qv)
    assert len(ek) > 0
    assert (keys.astype(np.int64) - KEY0).tolist() == ek and common.tolist() == ec and U.bits(scores).tolist() == es
    db.close()
    v.close()
