"""The keyframe database on the GPU (orbfe_kfdb_*, k_kfdb_query) against the reference restatement tests/cpp/kfdb_ref.cpp, bit
for bit: keys, common-word counts and scores (compared as uint64) of orbfe_kfdb_query in the restatement's lKFsSharingWords order
after EVERY mutation of every scene; orbfe_kfdb_score for given keys; the route that reads a query above the LDS budget from
global memory; capacity errors around a pool compaction; the scorings that are refused at create; the C++ facade
(tests/cpp/kfdb_test.cpp) on all scenes; and one chain descriptors -> orbfe_bow_transform -> add -> query.  What makes these
comparisons sharp (a pairwise sum differs from the sequential one on the scenes with >= 150 common words, ties on the first
common word, ...) is asserted on the restatement alone in tests/test_kfdb.py."""
import numpy as np
import pytest

import kfdb_util as K

pytestmark = pytest.mark.gpu
KEY0 = 1000     # key of keyframe i: KEY0 + i


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return K.build_ref(tmp_path_factory.mktemp('kfdbref'))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def _same_query(db, ref, qw, qv, what):
    keys, common, scores = db.query(qw, qv)
    rk, rc, rs = ref.sharing(qw, qv)
    assert (keys.astype(np.int64) - KEY0).tolist() == rk.tolist(), what
    assert common.tolist() == rc.tolist(), what
    assert _bits(scores) == _bits(rs), what


def _mutate(db, ref, scene, st):
    ref.step(st)
    if st[0] == 'add':
        k = scene['kfs'][st[1]]
        db.add(KEY0 + st[1], k['words'], k['values'])
    elif st[0] == 'erase':
        db.erase(KEY0 + st[1])
    else:
        db.clear()


@pytest.mark.parametrize('name', ['main', 'max5', 'max10', 'large', 'l2', 'chi', 'dot'])
def test_query_equals_the_restatement_after_every_mutation(lib, name):
    from os1_amd import api
    scene = K.scenes()[name]
    db = api.KeyFrameDatabase(scene['n_words'], scene['scoring'], scene['cap_k'], scene['cap_e'])
    ref = K.Ref(lib, scene)
    live, nmut = {}, 0
    for i, st in enumerate(scene['steps']):
        if st[0] not in ('add', 'erase', 'clear'):
            continue
        _mutate(db, ref, scene, st)
        nmut += 1
        if st[0] == 'add':
            live[st[1]] = len(scene['kfs'][st[1]]['words'])
        elif st[0] == 'erase':
            live.pop(st[1], None)
        else:
            live = {}
        assert db.size() == (len(live), sum(live.values()))
        for j, (qw, qv) in enumerate(scene['probes']):
            _same_query(db, ref, qw, qv, (name, i, st[0], j))
    assert nmut >= 4
    ref.close()
    db.close()


def test_score_for_given_keys_and_unknown_keys(lib):
    from os1_amd import api
    scene = K.scenes()['main']
    nm = scene['named']
    db = api.KeyFrameDatabase(scene['n_words'], scene['scoring'], scene['cap_k'], scene['cap_e'])
    ref = K.Ref(lib, scene)
    adds = [st for st in scene['steps'] if st[0] == 'add'][:20]
    for st in adds:
        _mutate(db, ref, scene, st)
    erased = adds[15][1]          # one of the random keyframes: none of the keys scored below
    assert erased not in [nm['zero'], nm['ident'], nm['big'], nm['one'], nm['never']] + nm['sized']
    _mutate(db, ref, scene, ('erase', erased))
    for qw, qv in scene['probes']:
        kfs = [nm['zero'], nm['ident'], nm['big'], nm['one'], nm['ident']] + nm['sized']      # a key may repeat
        got = db.score(qw, qv, [KEY0 + k for k in kfs])
        assert _bits(got) == _bits([ref.score(qw, qv, k) for k in kfs])
        for bad in (erased, nm['never']):
            out = np.full(3, -7.0)
            with pytest.raises(api.OrbfeError) as e:
                db.score(qw, qv, [KEY0 + nm['big'], KEY0 + bad, KEY0 + nm['one']], out=out)
            assert e.value.code == -1 and (out == -7.0).all()
    ref.close()
    db.close()


def test_query_above_the_lds_budget_takes_the_global_route(lib):
    """The split is by size alone: the query one word above the budget against the restatement, the one at the budget beside it
    (test_query_equals_the_restatement_after_every_mutation[large] sends both after every mutation; here: after an erase and a re-add,
    with orbfe_kfdb_score on the same two queries)."""
    from os1_amd import api
    scene = K.scenes()['large']
    db = api.KeyFrameDatabase(scene['n_words'], scene['scoring'], scene['cap_k'], scene['cap_e'] + 1000)
    ref = K.Ref(lib, scene)
    for st in [s for s in scene['steps'] if s[0] in ('add', 'erase')] + [('add', 3)]:
        _mutate(db, ref, scene, st)
    (qw, qv), (fw, fv) = scene['probes']
    assert len(qw) == K.QUERY_LDS_WORDS + 1 and len(fw) == K.QUERY_LDS_WORDS
    for w, v in ((qw, qv), (fw, fv)):
        _same_query(db, ref, w, v, len(w))
        kfs = list(range(0, len(scene['kfs']), 3))
        assert _bits(db.score(w, v, [KEY0 + k for k in kfs])) == _bits([ref.score(w, v, k) for k in kfs])
    ref.close()
    db.close()


def test_capacity_errors_and_compaction():
    from os1_amd import api
    rng = np.random.default_rng(5)

    def vec(n):
        w = np.sort(rng.choice(500, n, replace=False)).astype(np.uint32)
        return w, K.values_for(rng, n)

    db = api.KeyFrameDatabase(500, K.L1, 2, 1000)
    db.add(1, *vec(10))
    db.add(2, *vec(10))
    with pytest.raises(api.OrbfeError) as e:      # one keyframe too many
        db.add(3, *vec(10))
    assert e.value.code == -5 and db.size() == (2, 20)
    with pytest.raises(api.OrbfeError) as e:      # a key twice
        db.add(2, *vec(10))
    assert e.value.code == -1
    db.close()

    db = api.KeyFrameDatabase(500, K.L1, 8, 100)
    a, b, c = vec(60), vec(40), vec(60)
    db.add(1, *a)
    db.add(2, *b)
    db.erase(1)
    with pytest.raises(api.OrbfeError) as e:      # 40 live + 61 > 100: no compaction can help
        db.add(3, *vec(61))
    assert e.value.code == -5 and db.size() == (1, 40)
    db.add(3, *c)                                 # fits only after the pool is compacted (the tail stood at 100)
    with pytest.raises(api.OrbfeError) as e:      # one entry too many after compaction
        db.add(4, *vec(1))
    assert e.value.code == -5 and db.size() == (2, 100)
    q = vec(200)
    keys, common, scores = db.query(*q)
    qb = dict(zip(q[0].tolist(), q[1].tolist()))
    want = []
    for key, (w, v) in ((2, b), (3, c)):
        kb = dict(zip(w.tolist(), v.tolist()))
        if set(qb) & set(kb):
            want.append((min(set(qb) & set(kb)), key, len(set(qb) & set(kb)), K.py_score(K.L1, qb, kb)))
    want.sort()
    assert len(want) == 2
    assert keys.tolist() == [k for _, k, _, _ in want] and common.tolist() == [n for _, _, n, _ in want]
    assert _bits(scores) == _bits([s for _, _, _, s in want])
    db.close()


@pytest.mark.parametrize('scoring', [K.KL, K.BHATTA])
def test_unsupported_scoring_is_refused_at_create(scoring):
    from os1_amd import api
    with pytest.raises(api.OrbfeError) as e:
        api.KeyFrameDatabase(5000, scoring, 16, 1000)
    assert e.value.code == -1 and 'not supported' in str(e.value)


def test_facade_on_every_scene(tmp_path):
    import kfdb_facade as F
    exe = F.compile_test(str(tmp_path / 'kfdb_test'))
    files = []
    for name, scene in K.scenes().items():
        files.append(str(tmp_path / (name + '.scene')))
        K.write_scene(scene, files[-1])
    stats = F.run(exe, files)
    assert stats['scenes'] == len(files)
    for key in ('candidates', 'duplicates', 'stale', 'connected_skips', 'best_other', 'queries', 'checks'):
        assert stats[key] > 0, (key, stats)


def test_chain_descriptors_to_candidates(lib):
    """descriptors -> orbfe_bow_transform (k = 4, L = 3 vocabulary) -> add -> query, against the restatement fed the same BowVectors."""
    from os1_amd import api
    from bow_util import ragged_vocabulary
    voc = api.Vocabulary(ragged_vocabulary(31, k=4, L=3))
    n_words = voc.info()['n_words']
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    bows = []
    for i in range(31):     # 30 keyframes and the query frame: overlapping draws from one set of descriptors
        rows = rng.choice(300, int(rng.integers(20, 120)), replace=False)
        ids, vals = voc.transform(base[rows])[:2]
        bows.append((ids.copy(), vals.copy()))
    scene = dict(n_words=n_words, scoring=K.L1, kfs=[dict(index=i, id=i, words=w, values=v, connected=set(), covisible=[], bad=False)
                                                      for i, (w, v) in enumerate(bows[:30])])
    ref = K.Ref(lib, scene)
    db = api.KeyFrameDatabase(n_words, K.L1, 30, sum(len(w) for w, _ in bows[:30]))
    for i, (w, v) in enumerate(bows[:30]):
        db.add(KEY0 + i, w, v)
        ref.step(('add', i))
    assert len(bows[30][0]) > 0
    _same_query(db, ref, bows[30][0], bows[30][1], 'chain')
    assert len(db.query(*bows[30])[0]) > 0
    ref.close()
    db.close()
    voc.close()
