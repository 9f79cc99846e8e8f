"""The keyframe database (orbfe_kfdb_*, include/orbfe/KeyFrameDatabase.h) without a GPU: the reference restatement
tests/cpp/kfdb_ref.cpp (src/KeyFrameDatabase.cc:38-334, ScoringObject.cpp, LoopClosing.cc:125-140) is pinned to a second,
independent restatement in pure Python on every scene -- every returned vector and all six members of every keyframe after
every step -- and the conditions tests/test_gpu_kfdb.py relies on are shown to hold on the reference alone:
  * the scenes contain every shape they are built for: a keyframe with 0 and with exactly 1 common word; keyframes of 63, 64, 65
    and 130 entries; >= 150 common words; a keyframe identical to the query; a one-word query; keyframes tied on the first common
    word; erase and re-add of a key; erases that force a pool compaction, then more adds; clear and reuse; maxCommonWords 5 and 10
    (`* 0.8f` lands on an integer, the strict > bites); a stale mRelocScore taking part; a loop query whose connected set holds
    the first keyframe of a list; pBestKF != pKFi and duplicates;
  * where >= 150 words are common, a pairwise sum of the score's terms differs from the sequential one in at least one bit (so a
    reordered reduction on the GPU cannot pass);
  * ordering by (first common word, add order) IS the restatement's list order, after erases and re-adds.
The facade test compiles and links, the library exports the seven calls."""
import os
import re

import numpy as np
import pytest

import kfdb_util as K


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kfdbref'))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def _replay(lib, scene):
    """both restatements through the scene; -> what occurred"""
    ref, py = K.Ref(lib, scene), K.PyRef(scene)
    seen = dict(zero=0, one=0, ge150=0, pairwise_differs=0, ties_decided=0, queries=0, nonempty=0)
    add_seq, seq = {}, 0
    for st in scene['steps']:
        a, b = ref.step(st), py.step(st)
        assert a == b, (st[0], a, b)
        assert ref.members() == py.members(), st[0]
        if st[0] == 'add':
            add_seq[st[1]] = seq
            seq += 1
        if a is not None:
            seen['queries'] += 1
            seen['nonempty'] += bool(a)
        if st[0] in ('add', 'erase', 'clear'):
            live = {k for w in py.inv.values() for k in w}
            for qw, qv in scene['probes']:
                kfs, common, scores = ref.sharing(qw, qv)
                bow = dict(zip((int(w) for w in qw), (float(v) for v in qv)))
                pk, pc, ps = py.sharing(bow)
                assert kfs.tolist() == pk and common.tolist() == pc and _bits(scores) == _bits(ps)
                # the sort-key claim of orbfe_kfdb_query
                assert py.first_common_and_seq(bow, add_seq) == pk
                firsts = [min(set(bow) & set(py.kfs[i].bow)) for i in pk]
                seen['ties_decided'] += len(firsts) - len(set(firsts))
                seen['zero'] += len(live) - len(pk)
                seen['one'] += pc.count(1)
                for i, c in zip(pk, pc):
                    if c >= 150 and scene['scoring'] == K.L1:
                        seen['ge150'] += 1
                        seq_score = K.py_score(K.L1, bow, py.kfs[i].bow)
                        seen['pairwise_differs'] += seq_score != K.py_score_pairwise(bow, py.kfs[i].bow)
    counters = ref.counters()
    ref.close()
    return seen, counters


@pytest.mark.parametrize('name', ['main', 'max5', 'max10', 'large', 'l2', 'chi', 'dot'])
def test_restatement_equals_the_python_restatement_on_every_scene(lib, name):
    scene = K.scenes()[name]
    seen, counters = _replay(lib, scene)
    assert seen['queries'] > 0
    if name == 'main':
        assert seen['nonempty'] >= 5 and seen['zero'] and seen['one'] and seen['ge150'] and seen['ties_decided']
        # the condition that lets the GPU test catch a reordered sum
        assert seen['pairwise_differs'] > 0
        for key in ('candidates', 'duplicates', 'stale', 'connected_skips', 'best_other'):
            assert counters[key] > 0, (key, counters)
        assert scene['expect']['compactions'] >= 1 and scene['expect']['readds'] >= 1 and scene['expect']['clears_reused'] == 1
    if name in ('max5', 'max10'):
        assert counters['max_common'] == scene['named']['maxc'] and counters['min_common'] == scene['named']['minc']
        assert scene['named']['minc'] * 5 == scene['named']['maxc'] * 4


def test_main_scene_shapes():
    scene = K.scenes()['main']
    kfs, nm = scene['kfs'], scene['named']
    qw, qv = scene['probes'][0]
    q = set(qw.tolist())
    assert [len(kfs[i]['words']) for i in nm['sized']] == [63, 64, 65, 130]
    assert len(q & set(kfs[nm['zero']]['words'].tolist())) == 0
    assert len(q & set(kfs[nm['one']]['words'].tolist())) == 1
    assert len(q & set(kfs[nm['big']]['words'].tolist())) >= 150
    assert kfs[nm['ident']]['words'].tolist() == qw.tolist() and kfs[nm['ident']]['values'].tolist() == qv.tolist()
    assert all(min(q & set(kfs[i]['words'].tolist())) == int(qw[0]) for i in nm['ties'])
    assert len(scene['probes'][1][0]) == 1
    # the loop keyframe is connected to the keyframe added first, which is first in every list of the query's words
    assert scene['steps'][0] == ('add', nm['ident']) and nm['ident'] in kfs[nm['loop']]['connected']
    assert not any(st[0] == 'add' and st[1] == nm['never'] for st in scene['steps'])
    for k in kfs:   # values as transform leaves them: positive, summing to 1 up to rounding, not dyadic
        assert (k['values'] > 0).all() and abs(float(np.sum(k['values'])) - 1) < 1e-12
    large = K.scenes()['large']
    assert len(large['probes'][0][0]) == K.QUERY_LDS_WORDS + 1 and len(large['probes'][1][0]) == K.QUERY_LDS_WORDS
    assert large['n_words'] == 50000 and 40 <= len(large['kfs']) <= 200 and 40 <= len(kfs) <= 200


def test_identical_keyframe_scores_one_and_strict_threshold_bites(lib):
    scene = K.scenes()['main']
    ref = K.Ref(lib, scene)
    qw, qv = scene['probes'][0]
    assert abs(ref.score(qw, qv, scene['named']['ident']) - 1.0) < 1e-12
    assert ref.score(qw, qv, scene['named']['zero']) == 0.0
    ref.close()
    for name in ('max5', 'max10'):
        sc = K.scenes()[name]
        ref = K.Ref(lib, sc)
        for st in sc['steps'][:-1]:
            ref.step(st)
        m = ref.members()
        at, above = m[sc['named']['at_min']], m[sc['named']['above_min']]
        assert at[4] == sc['named']['minc'] and at[5] == 0            # listed with exactly minCommonWords: mRelocScore never written
        assert above[4] == sc['named']['minc'] + 1 and above[5] != 0
        ref.close()


def test_facade_test_compiles_and_links(tmp_path):
    import kfdb_facade as F
    exe = F.compile_test(str(tmp_path / 'kfdb_test'))
    assert os.path.exists(exe)


def test_keyframe_database_header_compiles_against_the_reference_names(tmp_path):
    import kfdb_facade as F
    F.syntax_check(str(tmp_path / 'kfdb_header.o'))


def test_library_exports_the_seven_calls():
    from os1_amd import api
    L = api.load_library()
    names = dict(orbfe_kfdb_create=6, orbfe_kfdb_add=5, orbfe_kfdb_erase=2, orbfe_kfdb_clear=1, orbfe_kfdb_size=3, orbfe_kfdb_query=9,
                 orbfe_kfdb_score=7)
    hdr = open(os.path.join(K.ROOT, 'include', 'orbfe.h')).read()
    for name, n in names.items():
        assert len(getattr(L, name).argtypes) == n
        m = re.search(r'\bint %s\(([^;]*)\);' % name, hdr)
        assert m and len(m.group(1).split(',')) == n, name
    assert L.orbfe_kfdb_destroy is not None
    assert api.KeyFrameDatabase.query and api.KeyFrameDatabase.score


def test_header_stays_c89():
    import test_header_c as T
    T.test_header_compiles_as_c_and_cpp()
