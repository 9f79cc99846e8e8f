"""tests/golden/dbow2_ref_outputs.npz: what the reference's own DBoW2 BowVector / FeatureVector accumulation (oracle/_ref/libdbow2_vec.so,
built by oracle/Makefile where the reference's sources are present) returns for the inputs of
tests/test_bow_oracle.py::test_restated_accumulation_equals_reference_dbow2.  The fixture is DATA (ids, values, FeatureVector, and a
digest of the inputs per case): the test holds the oracle's restatement to it where that object is absent.
Usage: python tools/gen_dbow2_ref_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    from oracle.pyoracle import Oracle, build
    import test_bow_oracle as t
    build()
    o = Oracle()
    out = {}
    try:
        for name, image, d, lu in t.accumulation_cases():
            v = o.vocabulary(image)
            if not o.use_dbow2_ref(True):
                raise SystemExit('oracle/_ref/libdbow2_vec.so is not built: nothing written')
            ids, vals, (fvn, fvo, fvf), _, _ = v.transform(d, lu)
            out.update({name + '_in': np.array(t.case_digest(image, d, lu)), name + '_ids': ids, name + '_vals': vals,
                        name + '_fvn': fvn, name + '_fvo': fvo, name + '_fvf': fvf})
    finally:
        o.use_dbow2_ref(False)
    np.savez_compressed(t.DBOW2_REF_OUTPUTS, **out)
    print('wrote', t.DBOW2_REF_OUTPUTS, os.path.getsize(t.DBOW2_REF_OUTPUTS), 'bytes,', len(out) // 6, 'cases')


if __name__ == '__main__':
    main()
