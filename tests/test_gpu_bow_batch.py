"""-m gpu: the map-load bulk calls.  orbfe_bow_transform_batch (k_bow_descend_batch: one grid over every (set, feature) pair, a wave
finds its set by a search over a table of wave offsets) must give, for every set, the bytes orbfe_bow_transform gives for that set
alone -- and, where the reference's own DBoW2 object (oracle/_ref/libdbow2_voc.so) or its record (tests/golden/dbow2_voc_outputs.npz)
covers the set, the reference's bytes, with the carve-out of tests/dbow2_ref_util.py.  orbfe_kfdb_add_batch must leave the database
answering queries exactly as single adds do.  One batch mixes sets of 0, 1, 63, 64, 65 and 200 features -- an empty set, a wave that
is partly filled, a set that ends on a wave boundary and one that ends one feature past it -- in 7 sets, so that the table's size is
no power of two.  Vocabularies: a balanced tree and two ragged ones; levelsup 0, 4 and L + 1."""
import os

import numpy as np
import pytest

import bow_batch_util as B
import dbow2_ref_util as U
import kfdb_util as K

pytestmark = pytest.mark.gpu
VOCS = ('synth3_10_4', 'ragged4', 'ragged31_4_3')
SETS = ('n63', 'n0', 'n200', 'n1', 'n65', 'n64', 'n0b')      # 7 sets; the first and the last empty set are different objects
CANARY = 0xA5


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def ref():
    return U.Reference()


def _sets(name):
    """the batch's descriptor sets: the recorded cases' own sets where they exist, 200 features drawn like them"""
    from test_bow_oracle import _descs
    s = U.desc_sets(name)
    image = U.voc_image(name)
    return {'n63': s['n63'], 'n0': s['n0'], 'n200': _descs(200, image, 200), 'n1': s['n1'], 'n65': s['n65'], 'n64': s['n64'],
            'n0b': np.zeros((0, 32), np.uint8)}


def _levels(name):
    L = U.voc_image(name)[1]
    return sorted({0, 4, L + 1})


def _flat(res):
    ids, vals, (fvn, fvo, fvf), wof, nof = res
    return [np.asarray(a).tobytes() for a in (ids, vals, fvn, fvo, fvf, wof, nof)]


def _reference_check(ref, name, lu, sn, live_voc):
    """-> check(result, what) against the reference's DBoW2 for set `sn` at header (0, 0), or None where neither the object nor the
    record covers it (the 200-feature set without the object)"""
    L = U.voc_image(name)[1]
    if ref.live:
        want = U.canon(live_voc.transform(_sets(name)[sn], lu), L, lu)
        return lambda res, what: U.assert_same(U.canon(res, L, lu), want, what)
    rec_name = {'n0b': 'n0'}.get(sn, sn)
    if rec_name not in U.SET_NAMES:
        return None
    i = U.transform_cases(name).index((0, 0, lu, rec_name))
    want = ref.rec[name + '_digests'][i]

    def check(res, what):
        assert U.digest(U.canon(res, L, lu)).tobytes() == want.tobytes(), what
    return check


@pytest.mark.parametrize('name', VOCS)
def test_batch_equals_the_single_call_and_the_reference_in_every_memory_placement(api, ref, name):
    image = U.voc_image(name)
    sets = _sets(name)
    assert [len(sets[s]) for s in SETS] == [63, 0, 200, 1, 65, 64, 0]
    if ref.rec is not None:
        assert str(ref.rec[name + '_in']) == U.inputs_digest(name)
    voc = api.Vocabulary(image)
    live_voc = None
    if ref.live:
        from oracle import pyoracle
        live_voc = pyoracle.Dbow2Vocabulary(image)
    m = api.Matcher()
    # the same rows in ordinary memory, page-locked memory and as the device rows of resident frames
    plain = [np.ascontiguousarray(sets[s]) for s in SETS]
    pinned = []
    for d in plain:
        p = api.PinnedArray((max(len(d), 1), 32), np.uint8)
        p.a[:len(d)] = d
        pinned.append(p)
    frames = []
    for d in plain:
        kps = np.zeros(len(d), api.KP_DTYPE)
        kps['x'] = np.arange(len(d)) % 600 + 10
        kps['y'] = np.arange(len(d)) % 400 + 10
        frames.append(api.Frame.from_host(m, kps, d, (0, 640, 0, 480)) if len(d) else None)
    pin_rows = [p.a[:len(d)] for p, d in zip(pinned, plain)]
    dev_rows = [f.descriptors_device() if f is not None else api.DeviceRows(0, 0) for f in frames]
    placements = dict(host=plain, pinned=pin_rows, device=dev_rows,
                      mixed=[(plain, pin_rows, dev_rows)[i % 3][i] for i in range(len(SETS))])
    compared = 0
    for lu in _levels(name):
        single = [_flat(voc.transform(d, lu)) for d in plain]
        for where, rows in placements.items():
            got = voc.transform_batch(rows, lu)
            assert len(got) == len(SETS)
            for k, sn in enumerate(SETS):
                assert _flat(got[k]) == single[k], (name, lu, where, sn)          # expectation 1: every array, byte for byte
                if where == 'host':
                    check = _reference_check(ref, name, lu, sn, live_voc)          # expectation 2: the reference's DBoW2
                    if check is not None:
                        check(got[k], (name, lu, sn))
                        compared += 1
        assert len(got[2][0]) > 0 and len(got[1][0]) == 0 and got[1][2][1].tolist() == [0]
    assert compared >= 6 * len(_levels(name))
    for f in frames:
        if f is not None:
            f.close()
    for p in pinned:
        p.free()
    m.close()
    voc.close()


def test_capacity_one_short_on_set_3_refuses_the_call_and_writes_nothing(api):
    name = 'ragged4'
    voc = api.Vocabulary(U.voc_image(name))
    sets = _sets(name)
    # (set 3 must have room to be short of: the 65-feature set takes its place in this order)
    order = ('n63', 'n0', 'n200', 'n65', 'n1', 'n64', 'n0b')
    rows = [np.ascontiguousarray(sets[s]) for s in order]
    cap = np.array([len(r) for r in rows], np.int32)
    cap[3] -= 1
    out = api.BowBatchOutputs(cap, fill=CANARY)
    with pytest.raises(api.OrbfeError) as e:
        voc.transform_batch(rows, 4, capacity=cap, out=out)
    assert e.value.code == -5 and 'set 3' in str(e.value)
    for t in out:
        for a in t:
            assert (a.view(np.uint8) == CANARY).all()
    assert (out.nw.view(np.uint8) == CANARY).all() and (out.nn.view(np.uint8) == CANARY).all()
    cap[3] += 1            # the same outputs with the full capacity: accepted, and equal to the single call
    got = voc.transform_batch(rows, 4, capacity=cap, out=api.BowBatchOutputs(cap, fill=CANARY))
    assert _flat(got[3]) == _flat(voc.transform(rows[3], 4))
    voc.close()


# ---- orbfe_kfdb_add_batch ---------------------------------------------------------------------------------------------------------
KEY0 = 7000


def _kfdb_case():
    """12 keyframes: 0..2 are there before the batch (1 and 2 are erased: tombstones), 3..11 are the batch of 9; keyframe 6 is empty.
    The pool holds exactly the entries that are live after the batch, so the batch fits only behind a compaction."""
    rng = np.random.default_rng(31)
    sizes = [40, 70, 50, 63, 64, 65, 0, 1, 130, 30, 17, 90]
    kfs = []
    for n in sizes:
        w = np.sort(rng.choice(3000, n, replace=False)).astype(np.uint32)
        kfs.append((w, K.values_for(rng, n) if n else np.zeros(0)))
    queries = []
    for src in (8, 0, 11):          # each shares words with several keyframes: drawn from three of them plus fresh words
        w = np.unique(np.concatenate([kfs[src][0][::2], kfs[3][0][::5], kfs[5][0][::7], rng.choice(3000, 40, replace=False)])).astype(np.uint32)
        queries.append((w, K.values_for(rng, len(w))))
    cap_e = sizes[0] + sum(sizes[3:])
    return kfs, queries, cap_e


def _prepared(api, kfs, cap_e, cap_k=10):
    db = api.KeyFrameDatabase(3000, K.L1, cap_k, cap_e)
    for i in range(3):
        db.add(KEY0 + i, *kfs[i])
    db.erase(KEY0 + 1)
    db.erase(KEY0 + 2)
    return db


def _answers(db, queries):
    out = []
    for qw, qv in queries:
        keys, common, scores = db.query(qw, qv)
        out.append((keys.tobytes(), common.tobytes(), scores.tobytes()))
    return out


def test_kfdb_add_batch_equals_single_adds_across_tombstones_and_a_compaction(api):
    kfs, queries, cap_e = _kfdb_case()
    a, b = _prepared(api, kfs, cap_e), _prepared(api, kfs, cap_e)
    batch = list(range(3, 12))
    assert len(batch) == 9 and len(kfs[6][0]) == 0
    # the tail stands behind the tombstones: 160 + the batch's 460 entries exceed the pool of 500, the live 40 + 460 fit exactly
    assert sum(len(kfs[i][0]) for i in range(3)) + sum(len(kfs[i][0]) for i in batch) > cap_e
    a.add_batch([KEY0 + i for i in batch], [kfs[i][0] for i in batch], [kfs[i][1] for i in batch])
    for i in batch:
        b.add(KEY0 + i, *kfs[i])
    assert a.size() == b.size() == (10, cap_e)
    got, want = _answers(a, queries), _answers(b, queries)
    assert got == want
    assert all(len(np.frombuffer(k, np.uint64)) >= 3 for k, _, _ in want)
    # both go on alike: an erase, a re-add through either call, the same answers
    for db in (a, b):
        db.erase(KEY0 + 8)
    a.add_batch([KEY0 + 8], [kfs[8][0]], [kfs[8][1]])
    b.add(KEY0 + 8, *kfs[8])
    assert _answers(a, queries) == _answers(b, queries)
    a.add_batch([], [], [])
    assert a.size() == b.size()
    a.close()
    b.close()


def test_kfdb_add_batch_is_all_or_nothing(api):
    kfs, queries, cap_e = _kfdb_case()
    db = _prepared(api, kfs, cap_e)
    before, size = _answers(db, queries), db.size()
    batch = list(range(3, 12))
    words, values = [kfs[i][0] for i in batch], [kfs[i][1] for i in batch]
    keys = [KEY0 + i for i in batch]
    dup = list(keys)
    dup[5] = KEY0                                   # position 5 names a keyframe that is in the database
    with pytest.raises(api.OrbfeError) as e:
        db.add_batch(dup, words, values)
    assert e.value.code == -1 and 'entry 5' in str(e.value)
    assert db.size() == size and _answers(db, queries) == before
    twice = list(keys)
    twice[5] = keys[2]                              # ... or one named earlier in the same batch
    with pytest.raises(api.OrbfeError) as e:
        db.add_batch(twice, words, values)
    assert e.value.code == -1 and 'entry 5' in str(e.value) and db.size() == size
    big = list(words)
    bigv = list(values)
    big[8] = np.arange(len(words[8]) + 1, dtype=np.uint32)        # one entry more than the pool can take, at position 8
    bigv[8] = np.full(len(big[8]), 1.0 / len(big[8]))
    with pytest.raises(api.OrbfeError) as e:
        db.add_batch(keys, big, bigv)
    assert e.value.code == -5 and 'entry 8' in str(e.value)
    assert db.size() == size and _answers(db, queries) == before
    small = _prepared(api, kfs, cap_e, cap_k=9)                     # the ninth keyframe of the batch is one keyframe too many
    with pytest.raises(api.OrbfeError) as e:
        small.add_batch(keys, words, values)
    assert e.value.code == -5 and 'entry 8' in str(e.value) and small.size() == size
    small.close()
    db.add_batch(keys, words, values)                               # and the database is still usable
    assert db.size() == (10, cap_e)
    db.close()


def test_shim_compute_bow_and_add_of_a_vector(api, tmp_path):
    """orbfe::ComputeBoW on 4 stub keyframes, one computed already and one resident on the device, against the one-keyframe overload;
    KeyFrameDatabaseT::add(vector) against single adds through DetectRelocalizationCandidates"""
    voc = str(tmp_path / 'voc.bin')
    open(voc, 'wb').write(bytes(U.voc_image('ragged31_4_3')))
    B.run(B.compile_shim_test(str(tmp_path / 'shim_gpu'), host_backend=False), [voc], timeout=60)
