"""tests/golden/dbow2_voc_outputs.npz: what the reference's own DBoW2 vocabulary code (oracle/_ref/libdbow2_voc.so: TemplatedVocabulary.h's
loader and transform, ScoringObject.cpp's scores, built by oracle/Makefile where the reference's sources are present) returns for the
cases of tests/dbow2_ref_util.py.  The fixture is DATA the reference's code wrote while running:
  <voc>_in        digest of the vocabulary image and its descriptor sets (the inputs are regenerated from seeds, not stored)
  <voc>_info      size(), k, L, scoring, weighting, node count of the loaded object (header 0, 0)
  <voc>_digests   (cases, 8) uint8: the first 8 bytes of the SHA-256 of every case's canonical transform result, in the order of
                  dbow2_ref_util.transform_cases
  <voc>_sample_*  one case in full (header (0, 0), levelsup 1, 17 descriptors): ids, values, FeatureVector, word and node per feature
  kfdb_scores     (6, queries, keyframes) uint64: score(query, keyframe) of dbow2_ref_util.kfdb_case under each scoring type
  frame_<case>_in, frame_<case>_digests   per frame of a fused-route / chain case: digest of its descriptors (extracted by the CPU
                  oracle) and of their canonical transform result; chain_digests, chain_scores: the chain's BowVectors and L1 scores
  scores_in, scores   digest of the score pairs; (pairs, 6) uint64 = the bits of score(v1, v2) under each of the six scoring types
                  (KL and Bhattacharyya are recorded only: the keyframe database refuses them)
The tests hold the oracle, tests/cpp/kfdb_ref.cpp, tests/kfdb_util.py and the GPU kernels to it where that object is absent.
Usage: python tools/gen_dbow2_voc_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    from oracle import pyoracle
    import dbow2_ref_util as U
    pyoracle.build()
    if not pyoracle.have_dbow2_voc():
        raise SystemExit('oracle/_ref/libdbow2_voc.so is not built: nothing written')
    out = {}
    for name in U.VOCS:
        base, sets = U.voc_image(name), U.desc_sets(name)
        L = base[1]
        info = pyoracle.Dbow2Vocabulary(base).info()
        out[name + '_in'] = np.array(U.inputs_digest(name))
        out[name + '_info'] = np.array([info[k] for k in ('size', 'k', 'L', 'scoring', 'weighting', 'n_nodes')], np.int32)
        digests, voc, header = [], None, None
        for s, w, lu, sn in U.transform_cases(name):
            if header != (s, w):
                header, voc = (s, w), pyoracle.Dbow2Vocabulary(U.with_header(base, s, w))
            c = U.canon(voc.transform(sets[sn], lu), L, lu)
            digests.append(U.digest(c))
            if (s, w, lu, sn) == (0, 0, 1, 'n17'):
                for key, a in zip(('ids', 'vals', 'fvn', 'fvo', 'fvf', 'wof', 'nof'), c):
                    out['%s_sample_%s' % (name, key)] = a
        out[name + '_digests'] = np.asarray(digests, np.uint8)
    scores = np.zeros((len(U.score_pairs()), 6), np.uint64)
    for s in U.SCORINGS:
        voc = pyoracle.Dbow2Vocabulary(U.tiny_vocabulary(s))
        scores[:, s] = U.bits([voc.score(w1, v1, w2, v2) for _, (w1, v1), (w2, v2) in U.score_pairs()])
    out['scores_in'] = np.array(U.pairs_digest())
    out['scores'] = scores
    ref = U.Reference(live=True)
    ref.rec = None
    out['kfdb_scores'] = U.kfdb_reference_scores(ref)
    # descriptors of extracted frames (the fused routes, the chain): extracted by the CPU oracle here, bit-equal to the GPU's
    o = pyoracle.Oracle()
    for name in U.FRAME_CASES:
        c = U.frame_case(name)
        L, lu = c['image'][1], c['levelsup']
        voc = pyoracle.Dbow2Vocabulary(c['image'])
        ox = pyoracle.OracleExtractor(c['nfeatures'], 1.2, 8, 20, 7, o)
        descs = [ox.extract(f)[1] for f in c['frames']]
        out['frame_%s_in' % name] = np.asarray([U._desc_digest(d) for d in descs], np.uint8)
        out['frame_%s_digests' % name] = np.asarray([U.digest(U.canon(voc.transform(d, lu), L, lu)) for d in descs], np.uint8)
        if name == 'chain':
            res = [voc.transform(descs[0][rows], lu) for rows in U.chain_subsets(len(descs[0]))]
            out['chain_digests'] = np.asarray([U.digest(U.canon(r, L, lu)) for r in res], np.uint8)
            out['chain_scores'] = U.bits([voc.score(res[-1][0], res[-1][1], r[0], r[1]) for r in res[:-1]])
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes,', sum(len(out[n + '_digests']) for n in U.VOCS), 'transform cases,',
          len(scores), 'score pairs')


if __name__ == '__main__':
    main()
