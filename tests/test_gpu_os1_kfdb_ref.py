"""The keyframe database on the GPU against the reference's own compiled src/KeyFrameDatabase.cc (oracle/_ref/libos1_kfdb.so where
it is built, else its recorded outputs tests/golden/os1_kfdb_outputs.npz), with exact equality.
Python level: every scene is replayed on orbfe_kfdb_*; at every relocalisation step orbfe_kfdb_query's keys and common counts are
compared with the mnRelocWords the reference object left in the keyframes it met, and (float)score with the mRelocScore bits of
every keyframe it scored; the same at loop steps with mnLoopWords / mLoopScore over the keyframes that are not connected.  The
'large' scene sends a query above the kernel's LDS budget.
Facade: tests/cpp/kfdb_test.cpp runs orbfe::KeyFrameDatabaseT on every scene, the crafted families included, and compares the
candidates and all six members after every step with the recorded reference outputs."""
import numpy as np
import pytest

import kfdb_util as K

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY0 = 1000
ALL = list(K.every_scene())


def _reference(name):
    scene = K.every_scene()[name]
    if K.have_os1():
        ref = K.os1_ref(scene)
        out = K.trace(ref, scene)
        ref.close()
        assert out == K.golden()[name], 'the golden is stale: run tools/gen_os1_kfdb_golden.py'
        return out
    return K.golden()[name]


def _check_query(db, scene, st, before, after, what):
    """one query step: the GPU's answer for the step's vector against the members the reference object held before and after it"""
    loop = st[0] == 'loop'
    qi, wi, si = (0, 1, 2) if loop else (3, 4, 5)
    if loop:
        q = scene['kfs'][st[1]]
        qid, words, values, connected = q['id'], q['words'], q['values'], q['connected']
    else:
        qid, words, values, connected = st[1], st[2], st[3], set()
    keys, common, scores = db.query(words, values)
    got = {int(k) - KEY0: (int(c), F32(s)) for k, c, s in zip(keys, common, scores)}
    assert len(got) == len(keys)
    met, listed = {}, []
    for i in range(len(scene['kfs'])):
        if i in connected:
            continue
        stale = before[i][qi] == qid
        delta = after[i][wi] - (before[i][wi] if stale else 0)
        if after[i][qi] == qid and delta > 0:
            met[i] = delta
            if not stale:
                listed.append(i)
    assert {i: c for i, (c, _) in got.items() if i not in connected} == met, what
    scored = 0
    if listed:
        minc = int(F32(max(after[i][wi] for i in listed)) * F32(0.8))
        for i in listed:
            if after[i][wi] > minc:
                assert int(got[i][1].view(np.uint32)) == after[i][si], (what, i)
                scored += 1
    return len(met), scored


@pytest.mark.parametrize('name', ALL)
def test_query_equals_the_reference_members_at_every_query_step(name):
    from os1_amd import api
    scene = K.every_scene()[name]
    res, mem = _reference(name)
    db = api.KeyFrameDatabase(scene['n_words'], scene['scoring'], scene['cap_k'], scene['cap_e'])
    zero = [(0, 0, 0, 0, 0, 0)] * len(scene['kfs'])
    met = scored = 0
    try:
        for i, st in enumerate(scene['steps']):
            if st[0] == 'add':
                k = scene['kfs'][st[1]]
                db.add(KEY0 + st[1], k['words'], k['values'])
            elif st[0] == 'erase':
                if any(s[0] == 'add' and s[1] == st[1] for s in scene['steps'][:i]):
                    db.erase(KEY0 + st[1])
            elif st[0] == 'clear':
                db.clear()
            else:
                a, b = _check_query(db, scene, st, mem[i - 1] if i else zero, mem[i], (name, i, st[0]))
                met, scored = met + a, scored + b
    finally:
        db.close()
    assert met > 0 and scored > 0
    if name == 'large':
        assert any(st[0] == 'reloc' and len(st[2]) > K.QUERY_LDS_WORDS for st in scene['steps'])


def test_facade_on_every_scene_against_the_recorded_reference(tmp_path):
    import kfdb_facade as F
    exe = F.compile_test(str(tmp_path / 'kfdb_test'))
    files = []
    for name, scene in K.every_scene().items():
        files.append(str(tmp_path / (name + '.scene')))
        K.write_scene(scene, files[-1])
        res, mem = _reference(name)
        K.write_expected(scene, res, mem, files[-1] + '.expect')
    stats = F.run(exe, files)
    assert stats['scenes'] == len(files) == len(ALL)
    assert stats['ref_checks'] == sum(len(s['steps']) * len(s['kfs']) for s in K.every_scene().values())
    assert stats['ref_queries'] == sum(st[0] in ('loop', 'reloc') for s in K.every_scene().values() for st in s['steps'])
