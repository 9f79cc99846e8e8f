"""CPU: the restatements of DBoW2 held to the REFERENCE'S OWN code -- oracle.vocabulary(image).transform (orc_bow_transform) to
TemplatedVocabulary::transform, and the score of tests/cpp/kfdb_ref.cpp and of tests/kfdb_util.py's Python restatement to the six
ScoringObject.cpp scores -- through oracle/_ref/libdbow2_voc.so (oracle/dbow2_voc_wrap.cpp; built by oracle/Makefile where the
reference's sources are present).  The `live` tests skip where that object is absent; the `recorded` tests run everywhere, against
what the object returned for the same inputs (tests/golden/dbow2_voc_outputs.npz <- tools/gen_dbow2_voc_golden.py).  The cases and the
one carve-out the reference's code forces (features whose node id it never writes) are described in tests/dbow2_ref_util.py.

What the reference's loader does with the images, found here and asserted below: it accepts every one of the 6 x 4 header combinations
and holds them as given; it appends one copy of the last record (its `while(!eof)` loop), so size() is the number of leaf records + 1
and the tree has one node more than records + root."""
import ctypes as C

import numpy as np
import pytest

import dbow2_ref_util as U
import kfdb_util as K
from oracle import pyoracle

needs_object = pytest.mark.skipif(not pyoracle.have_dbow2_voc(), reason='oracle/_ref/libdbow2_voc.so is not built (no reference sources here)')


def _descent(oracle, ref, name):
    ov, header, n, unwritten = None, None, 0, 0
    for (s, w, lu, sn), image, d, check in ref.transforms(name):
        if header != (s, w):
            header, ov = (s, w), oracle.vocabulary(image)
        res = ov.transform(d, lu)
        check(res, (name, s, w, lu, sn))
        n += 1
        unwritten += int((U.canon(res, image[1], lu)[6] == U.NID_UNWRITTEN).sum())
    assert n == len(U.transform_cases(name))
    # the carve-out exists only where leaves lie at unequal depths, and ragged_vocabulary(4) meets it
    assert unwritten == 0 or name in U.RAGGED
    assert unwritten > 0 or name != 'ragged4'


@needs_object
@pytest.mark.parametrize('name', U.VOCS)
def test_descent_equals_reference_transform_live(oracle, name):
    oracle.use_dbow2_ref(False)
    _descent(oracle, U.Reference(live=True), name)


@pytest.mark.parametrize('name', U.VOCS)
def test_descent_equals_recorded_reference_transform(oracle, name):
    oracle.use_dbow2_ref(False)
    _descent(oracle, U.Reference(live=False), name)


@needs_object
@pytest.mark.parametrize('name', U.VOCS)
def test_reference_loader_holds_the_header_and_appends_one_copy_of_the_last_record(name):
    base = U.voc_image(name)
    rec = np.frombuffer(base, np.uint8, offset=4).reshape(-1, 45)
    leaves = int((rec[:, 4] > 0).sum())
    for s, w in U.HEADERS:
        info = pyoracle.Dbow2Vocabulary(U.with_header(base, s, w)).info()
        assert (info['k'], info['L'], info['scoring'], info['weighting']) == (base[0], base[1], s, w)
        assert info['n_nodes'] == len(rec) + 2 and info['size'] == leaves + 1
    g = np.load(U.GOLDEN)
    info = pyoracle.Dbow2Vocabulary(base).info()
    assert g[name + '_info'].tolist() == [info[k] for k in ('size', 'k', 'L', 'scoring', 'weighting', 'n_nodes')]


@needs_object
def test_reference_loader_refuses_headers_out_of_range():
    base = U.voc_image('ragged31_4_3')
    for bad in (bytes([21, 3, 0, 0]), bytes([4, 0, 0, 0]), bytes([4, 11, 0, 0]), bytes([4, 3, 6, 0]), bytes([4, 3, 0, 4])):
        with pytest.raises(ValueError):
            pyoracle.Dbow2Vocabulary(bad + base[4:])


def test_recorded_sample_cases_in_full(oracle):
    """one case per vocabulary is recorded array by array, so that a disagreement can be read and not only detected"""
    g = np.load(U.GOLDEN)
    oracle.use_dbow2_ref(False)
    for name in U.VOCS:
        base = U.voc_image(name)
        got = U.canon(oracle.vocabulary(base).transform(U.desc_sets(name)['n17'], 1), base[1], 1)
        want = [g['%s_sample_%s' % (name, k)] for k in ('ids', 'vals', 'fvn', 'fvo', 'fvf', 'wof', 'nof')]
        U.assert_same(got, want, name)


@pytest.fixture(scope='module')
def kref(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kfdbref_dbow2'))


def _restated_scores(kref, scoring):
    """tests/cpp/kfdb_ref.cpp's score and tests/kfdb_util.py's, as bits, for every pair"""
    pairs = U.score_pairs()
    h = kref.kref_create(U.SCORE_WORDS, scoring)
    cpp, py = [], []
    for i, (_, (w1, v1), (w2, v2)) in enumerate(pairs):
        w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
        v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
        assert kref.kref_new_kf(h, i, w2.ctypes.data_as(C.c_void_p), v2.ctypes.data_as(C.c_void_p), len(w2)) == i
        cpp.append(kref.kref_score(h, w1.ctypes.data_as(C.c_void_p), v1.ctypes.data_as(C.c_void_p), len(w1), i))
        py.append(K.py_score(scoring, dict(zip(w1.tolist(), v1.tolist())), dict(zip(w2.tolist(), v2.tolist()))))
    kref.kref_destroy(h)
    return U.bits(cpp), U.bits(py)


def _scores(kref, ref, scoring):
    want = U.reference_scores(ref)[:, scoring]
    cpp, py = _restated_scores(kref, scoring)
    names = [p[0] for p in U.score_pairs()]
    bad = [n for n, a, b in zip(names, cpp, want) if a != b]
    assert not bad, ('tests/cpp/kfdb_ref.cpp', scoring, bad[:10])
    bad = [n for n, a, b in zip(names, py, want) if a != b]
    assert not bad, ('kfdb_util.py_score', scoring, bad[:10])


@needs_object
@pytest.mark.parametrize('scoring', U.ACCEPTED)
def test_restated_scores_equal_reference_score_live(kref, scoring):
    _scores(kref, U.Reference(live=True), scoring)


@pytest.mark.parametrize('scoring', U.ACCEPTED)
def test_restated_scores_equal_recorded_reference_score(kref, scoring):
    _scores(kref, U.Reference(live=False), scoring)


def test_score_pairs_have_the_shapes_they_are_built_for():
    p = {n: (a, b) for n, a, b in U.score_pairs()}
    common = lambda n: sorted(set(p[n][0][0].tolist()) & set(p[n][1][0].tolist()))
    assert common('disjoint') == [] and len(p['empty_second'][1][0]) == 0 and len(p['empty_first'][0][0]) == 0
    assert common('common_first_only') == [int(p['common_first_only'][0][0][0])] == [int(p['common_first_only'][1][0][0])]
    assert common('common_last_only') == [int(p['common_last_only'][0][0][-1])] == [int(p['common_last_only'][1][0][-1])]
    assert len(common('above_64')) > 64 and len(common('above_4096')) < 4096 < min(len(p['above_4096'][0][0]), len(p['above_4096'][1][0]))
    (w, v1), (_, v2) = p['chi_zero_sums']
    assert ((v1 + v2) == 0).sum() >= 2 * (len(w) // 3) and (v1[::3] != 0).all() and ((v1 + v2) != 0).any()
    assert sum(n.startswith('scene/') for n in p) == sum(len(s['probes']) * len(s['kfs']) for s in K.scenes().values())
    # the record keeps what the reference returns for the two scorings the database refuses, too
    g = np.load(U.GOLDEN)
    assert g['scores'].shape == (len(p), 6) and g['scores'].dtype == np.uint64
