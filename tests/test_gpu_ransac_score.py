"""orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses on the GPU against the restatement tests/cpp/ransac_score_ref.cpp, bit
for bit and without any tolerance: counts and masks over the shape sweep and a multi-segment call, the crafted set with verdicts
that follow by hand, packed against explicit mask_off, NULL outputs, argument errors, the C++ walks through the C ABI, and a
chain from two resident keyframes through an existing search.  One test runs on the CPU: it shows that the PNP sweep tells an
all-float evaluation from the reference's mixed one.

The cases are functions that the two GPU tests at the end of the file call in a loop, with the case named in every assertion
message: the whole file takes under three seconds on the device, and the suite's list of test ids stays short."""
import ctypes as C

import numpy as np
import pytest

import ransac_score_util as U

gpu = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL = 0xa5a5a5a5a5a5a5a5


@pytest.fixture(scope='module')
def ref(tmp_path_factory):
    return U.build_ref(tmp_path_factory.mktemp('ransac_score_ref'))


@pytest.fixture(scope='module')
def matcher():
    from os1_amd import api
    m = api.Matcher(0)
    yield m
    m.close()


def gpu_score(matcher, call):
    if call.model == 'sim3':
        return matcher.score_sim3_hypotheses(call.corr, call.cams, call.T12, call.T21, call.seg_off, call.hyp_seg)
    return matcher.score_pnp_hypotheses(call.corr, call.cams, call.hyp, call.seg_off, call.hyp_seg)


def raw_call(matcher, call, want_counts=True, want_masks=True, mask_off=None, n_words=None, handle='own', **over):
    """The C call itself -> (rc, counts, words); both outputs are filled with sentinels first.  over: arguments to replace."""
    p = U._p
    K = len(call.hyp)
    packed = sum(U.words_of(call.n_of(k)) for k in range(K)) if K else 0
    counts = np.full(max(K, 1) + 1, -77, np.int32)
    words = np.full((packed if n_words is None else n_words) + 1, SENTINEL, np.uint64)
    a = dict(n_seg=len(call.seg_off) - 1, seg_off=p(call.seg_off), corr=p(call.corr), cams=p(call.cams), n_hyp=K, hyp_seg=p(call.hyp_seg))
    a.update(over)
    h = matcher.h if handle == 'own' else handle
    tail = [p(counts) if want_counts else None, None if mask_off is None else p(mask_off), p(words) if want_masks else None]
    if call.model == 'sim3':
        T12, T21 = call.T12, call.T21
        rc = matcher.L.orbfe_score_sim3_hypotheses(h, a['n_seg'], a['seg_off'], a['corr'], a['cams'], a['n_hyp'], a['hyp_seg'], a.get('hyp', p(T12)),
                                                   p(T21), *tail)
    else:
        rc = matcher.L.orbfe_score_pnp_hypotheses(h, a['n_seg'], a['seg_off'], a['corr'], a['cams'], a['n_hyp'], a['hyp_seg'], a.get('hyp', p(call.hyp)),
                                                  *tail)
    return rc, counts, words


def check_words(call, counts, words, want):
    """counts[k] == popcount(mask k), the words are the restatement's, the bits at and above N are 0, nothing is written past the end"""
    wc, wm = want
    at = 0
    for k in range(len(call.hyp)):
        n = call.n_of(k)
        w = words[at:at + U.words_of(n)]
        bits = np.unpackbits(w.view(np.uint8), bitorder='little')
        assert np.array_equal(bits[:n].astype(bool), wm[k]), 'mask of hypothesis %d' % k
        assert not bits[n:].any(), 'tail bits of hypothesis %d' % k
        assert counts[k] == int(bits.sum()) == wc[k]
        at += U.words_of(n)
    assert words[at] == SENTINEL and at == len(words) - 1 and counts[len(call.hyp)] == -77


def shape_sweep(ref, matcher, model, n):
    for K in U.SWEEP_K:
        call = U.sweep_call(model, n, K)
        want = U.ref_score(ref, call)
        if n <= 65 or K <= 5:                       # the numpy restatement agrees before either is used (all cases: tests/test_ransac_score.py)
            U.assert_same(U.np_score(call), want, 'numpy %s n=%d K=%d' % (model, n, K))
        U.assert_same(gpu_score(matcher, call), want, '%s n=%d K=%d' % (model, n, K))
        rc, counts, words = raw_call(matcher, call)
        assert rc == 0
        check_words(call, counts, words, want)
        if K == 300 and n >= 63:
            r = want[0] / n
            assert r.max() > 0.5 and r.min() == 0    # inlier ratios from most of the scene to nothing


def multi_segment_call(ref, matcher, model):
    call = U.multi_call(model)
    assert list(np.diff(call.seg_off)) == list(U.MULTI_N) and call.seg_off[0] == 2 and len(set(call.hyp_seg[:3])) == 3
    want = U.ref_score(ref, call)
    U.assert_same(U.np_score(call), want, 'numpy')
    got = gpu_score(matcher, call)
    U.assert_same(got, want, model)
    assert [len(m) for m in got[1]] == [U.MULTI_N[s] for s in call.hyp_seg]
    assert all(c == 0 for c, s in zip(got[0], call.hyp_seg) if s == 1)          # the N = 0 segment: no words, count 0
    rc, counts, words = raw_call(matcher, call)
    assert rc == 0
    check_words(call, counts, words, want)
    assert matcher.L.orbfe_ransac_mask_words(3, U._p(call.seg_off), len(call.hyp), U._p(call.hyp_seg)) == len(words) - 1


def crafted_set(ref, matcher, model):
    call, verdict = U.crafted(model)
    want = U.ref_score(ref, call)
    U.assert_same(U.np_score(call), want, 'numpy')
    counts, masks = gpu_score(matcher, call)
    U.assert_same((counts, masks), want, model)
    m = np.stack(masks)
    assert np.array_equal(m, verdict)
    ident = m[U.H_IDENT]
    assert not ident[U.C_AT] and ident[U.C_BELOW] and not ident[U.C_Z0] and ident[U.C_BEHIND] and not ident[U.C_MAX0] and ident[U.C_PLAIN]
    assert ident[U.C_SIGMA] == (model == 'pnp')                                  # SIM3: the maximum is 13, the error 13.1044
    assert counts[U.H_NAN] == 0 and not m[U.H_NAN].any()
    assert call.corr[U.C_SIGMA, 10 if model == 'sim3' else 5] == (13 if model == 'sim3' else f32(1.44) * f32(5.991))


def test_pnp_sweep_tells_float_from_double(ref):
    """Discriminating power, no GPU: over the PNP sweep an evaluation that does everything in float gives another verdict than the
    restatement for at least one (hypothesis, correspondence), so the GPU tests above would see a kernel that ignored the doubles."""
    differ = 0
    for n in U.SWEEP_N:
        for K in U.SWEEP_K:
            call = U.sweep_call('pnp', n, K)
            _, want = U.ref_score(ref, call)
            _, flt = U.np_score(call, all_float=True)
            differ += sum(int((a != b).sum()) for a, b in zip(want, flt))
    print('verdicts that differ between the all-float and the reference evaluation: %d' % differ)
    assert differ >= 1


def packed_and_explicit_mask_off_agree_and_null_outputs(ref, matcher, model):
    call = U.multi_call(model)
    want = U.ref_score(ref, call)
    rc, counts, packed = raw_call(matcher, call)
    assert rc == 0
    K = len(call.hyp)
    # explicit offsets: the hypotheses' words in reverse order, four unused words between two neighbours
    nw = [U.words_of(call.n_of(k)) for k in range(K)]
    off = np.zeros(K, np.int64)
    at = 3
    for k in reversed(range(K)):
        off[k] = at
        at += nw[k] + 4
    rc, counts2, spread = raw_call(matcher, call, mask_off=off, n_words=at)
    assert rc == 0 and np.array_equal(counts, counts2)
    used = np.zeros(len(spread), bool)
    src = 0
    for k in range(K):
        assert np.array_equal(spread[off[k]:off[k] + nw[k]], packed[src:src + nw[k]])
        used[off[k]:off[k] + nw[k]] = True
        src += nw[k]
    assert (spread[~used] == SENTINEL).all()
    # counts alone, masks alone, neither
    rc, c3, w3 = raw_call(matcher, call, want_masks=False)
    assert rc == 0 and np.array_equal(c3, counts) and (w3 == SENTINEL).all()
    rc, c4, w4 = raw_call(matcher, call, want_counts=False)
    assert rc == 0 and (c4 == -77).all() and np.array_equal(w4, packed)
    rc, c5, w5 = raw_call(matcher, call, want_counts=False, want_masks=False)
    assert rc == 0 and (c5 == -77).all() and (w5 == SENTINEL).all()
    check_words(call, counts, packed, want)


def argument_errors_leave_outputs_untouched(ref, matcher, model):
    call = U.multi_call(model)
    p = U._p
    K = len(call.hyp)

    def refused(**kw):
        rc, counts, words = raw_call(matcher, call, **kw)
        assert rc == -1, kw
        assert b'invalid' in matcher.L.orbfe_last_error()
        assert (counts == -77).all() and (words == SENTINEL).all(), kw

    refused(handle=None)                                                        # a NULL matcher
    refused(n_seg=0)
    refused(n_hyp=0)
    refused(n_hyp=-1)
    bad = call.seg_off.copy(); bad[2] = bad[1] - 1
    refused(seg_off=p(bad))                                                     # non-monotone
    neg = call.seg_off.copy(); neg[0] = -1
    refused(seg_off=p(neg))
    for v in (3, -1, 1 << 30):
        hs = call.hyp_seg.copy(); hs[K // 2] = v
        refused(hyp_seg=p(hs))
    refused(seg_off=None)
    refused(corr=None)
    refused(cams=None)
    refused(hyp=None)
    off = np.arange(K, dtype=np.int64) * 8; off[1] = -8
    refused(mask_off=off, n_words=8 * K)
    # totals beyond int32 indexing, refused from seg_off and hyp_seg alone
    huge = np.array([0, (1 << 31) // 12 + 1], np.int32)
    refused(n_seg=1, seg_off=p(huge), hyp_seg=p(np.zeros(K, np.int32)))
    most = np.array([0, ((1 << 31) - 1) // 12], np.int32)
    many = np.zeros(768, np.int32)
    refused(n_seg=1, seg_off=p(most), n_hyp=768, hyp_seg=p(many), want_masks=False)
    assert matcher.L.orbfe_ransac_mask_words(1, p(most), 768, p(many)) == 0 and b'invalid' in matcher.L.orbfe_last_error()
    # and the handle still works
    U.assert_same(gpu_score(matcher, call), U.ref_score(ref, call), 'after the refusals')


def cpp_walks_through_the_c_abi(tmp_path):
    """tests/cpp/ransac_score_test.cpp: a Sim3 round-robin of three candidates, one scoring call per round; a PnP scene with a failing
    and a succeeding Refine (n_hyp = 1 calls); every iterate() equals the restated one."""
    exe = U.compile_walk_test(str(tmp_path / 'ransac_score_test'), host=False)
    files = [U.sim3_round_robin_scene(str(tmp_path / 'sim3.bin')), U.pnp_refine_scene(str(tmp_path / 'pnp.bin'))]
    lines, calls = U.run_walk_test(exe, files)
    assert lines[-2] == 'scenes 2 mismatches 0' and lines[0].endswith(' ok')
    s, p = calls[files[0]], calls[files[1]]
    assert {x['cand'] for x in s} == {0, 1, 2} and max(x['round'] for x in s) >= 2 and any(x['ret'] >= 0 for x in s)
    assert any(x['ret'] == -2 for x in p)


def sim3_choice(counts, min_inliers):
    """Sim3Solver::iterate's rule over a list of counts: the first hypothesis that is at least the best so far and above
    mRansacMinInliers (Sim3Solver.cc:186-202); -1 if none."""
    best = 0
    for k, c in enumerate(counts):
        if c >= best:
            best = c
            if c > min_inliers:
                return k
    return -1


def chain_from_resident_keyframes(ref, matcher):
    """Two resident synthetic keyframes of the same points, matched by the projected search (what SearchBySim3 runs); the
    correspondences are packed from its output; the hypotheses are noisy copies of the true relative pose, gross first."""
    from os1_amd.api import KP_DTYPE
    rng = np.random.default_rng(21)
    n = 400
    uv = np.stack([rng.uniform(60, 690, n), rng.uniform(60, 420, n)], 1)
    depth = rng.uniform(3.0, 9.0, n)
    X1 = np.stack([(uv[:, 0] - U.CX) / U.FX * depth, (uv[:, 1] - U.CY) / U.FY * depth, depth], 1)
    R, t = U._rot(0.01, -0.02, 0.015), np.array([0.05, -0.02, 0.03])
    X2 = X1 @ R.T + t                                                        # T21: camera 1 -> camera 2
    uv2 = np.stack([U.FX * X2[:, 0] / X2[:, 2] + U.CX, U.FY * X2[:, 1] / X2[:, 2] + U.CY], 1)
    bounds = (0.0, 752.0, 0.0, 480.0)
    k1, k2 = np.zeros(n, KP_DTYPE), np.zeros(n, KP_DTYPE)
    perm = rng.permutation(n)                                                 # keyframe 2 holds the points in another order
    k1['x'], k1['y'] = uv[:, 0], uv[:, 1]
    k2['x'], k2['y'] = (uv2 + rng.normal(0, 0.4, uv2.shape))[perm].T
    for k in (k1, k2):
        k['size'], k['octave'], k['class_id'] = 31, 0, -1
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = d1[perm].copy()
    d2[np.arange(n), rng.integers(0, 32, n)] ^= 1                             # one bit of noise per descriptor
    f1, f2 = matcher.frame(k1, d1, bounds), matcher.frame(k2, d2, bounds)
    try:
        nm, best, _ = matcher.search_projected(f2, None, None, uv2.astype(f32), np.full(n, 10.0, f32), np.zeros(n, np.int32), np.ones(n, np.uint8),
                                               f1.descriptors_device(), max_dist=100)
        assert nm > n // 2
        dk1, dk2 = f1.download()[0], f2.download()[0]
        i1 = np.nonzero(best >= 0)[0]
        i2 = best[i1]
        assert (perm[i2] == i1).mean() > 0.95                                 # the search found the same points
        X2k = X2[perm]                                                        # keyframe 2's points in its keypoint order
        nine = np.full((len(i1), 1), U.sim3_max_error(1.0), f32)
        corr = np.concatenate([X1[i1], X2k[i2], np.stack([dk1['x'][i1], dk1['y'][i1]], 1), np.stack([dk2['x'][i2], dk2['y'][i2]], 1), nine, nine], 1)
        hyp = np.stack([U.sim3_pack(1.0 + e * rng.normal(), U._rot(*(0.2 * e * rng.normal(0, 1, 3))) @ R.T, -R.T @ t + e * rng.normal(0, 1, 3))
                        for e in U.perturb_levels(50)[::-1]])
        call = U.Call('sim3', corr, np.array([U.FX, U.FY, U.CX, U.CY] * 2, f32), hyp)
        want = U.ref_score(ref, call)
        got = gpu_score(matcher, call)
        U.assert_same(got, want, 'chain')
        choice = sim3_choice(got[0], 20)
        assert choice == sim3_choice(want[0], 20) and 0 < choice < 49 and got[0][-1] > 0.9 * len(i1)
    finally:
        f1.close()
        f2.close()


MODELS = ('sim3', 'pnp')


def case(fn, *args):
    """Run one case; a failure names it."""
    try:
        fn(*args)
    except AssertionError as e:
        raise AssertionError('%s(%s): %s' % (fn.__name__, ', '.join(str(a) for a in args if isinstance(a, (str, int))), e)) from e


@gpu
def test_counts_and_masks_equal_the_restatement(ref, matcher):
    """The scoring calls themselves: the shape sweep N x K, the multi-segment call, the crafted set, packed against explicit
    mask_off with NULL outputs, and the argument errors, for both models."""
    for model in MODELS:
        for n in U.SWEEP_N:
            case(shape_sweep, ref, matcher, model, n)
        case(multi_segment_call, ref, matcher, model)
        case(crafted_set, ref, matcher, model)
        case(packed_and_explicit_mask_off_agree_and_null_outputs, ref, matcher, model)
        case(argument_errors_leave_outputs_untouched, ref, matcher, model)


@gpu
def test_walks_through_the_c_abi_and_chain_from_resident_keyframes(ref, matcher, tmp_path):
    """What is built on the calls: the C++ walks (tests/cpp/ransac_score_test.cpp) and the chain from an existing search."""
    case(cpp_walks_through_the_c_abi, tmp_path)
    case(chain_from_resident_keyframes, ref, matcher)
