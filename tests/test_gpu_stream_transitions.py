"""-m gpu: the stream runners across setting changes, against the oracle bit for bit.

Every frame's predecessor follows the contract above orbfe_stream_create (include/orbfe.h): frame 0 of a batch is matched against the
last frame pushed before it, whatever its size, route or matching setting, except for the runner's first batch, batches pushed while
isolated batches are on, and the first batch after they are switched off.  A batch pushed with matching off reports no matches.
Held results (orbfe_stream_pop_hold) stay valid until released, and what would move them is refused meanwhile."""
import numpy as np
import pytest

from oracle.pyoracle import OracleExtractor
from os1_amd.synth import shifted, synth

pytestmark = pytest.mark.gpu

N, NL = 200, 3
SMALL = (600, 800)     # rows, cols: GPU quadtree route
WIDE = (100, 1600)     # 23-29 quadtree roots per level: host-quadtree route, and 4 x roots > a level's quota, so the row stride grows
B_SMALL = (0.0, 800.0, 0.0, 600.0)
B_TIGHT = (40.0, 760.0, 30.0, 570.0)
B_BOTH = (0.0, 1600.0, 0.0, 600.0)
ON = (100, 0.9, True, B_SMALL)
TIGHT = (25, 0.7, False, B_TIGHT)
BOTH = (100, 0.9, True, B_BOTH)

_IMAGES = {}
_WANT = {}     # frame key -> the oracle's (keypoints, descriptors), shared by every parametrisation


def _image(key):
    if key not in _IMAGES:
        kind, i = key
        if kind == 'blank':
            img = np.full(SMALL, 90, np.uint8)
        else:
            (h, w), seed = (SMALL, 81) if kind == 'small' else (WIDE, 82)
            if (kind, 0) not in _IMAGES:
                _IMAGES[(kind, 0)] = synth(seed, w, h)
            img = _IMAGES[(kind, 0)] if i == 0 else shifted(_IMAGES[(kind, 0)], 3 * (i % 7), -2 * (i % 5), 900 + i)
        _IMAGES[key] = img
    return _IMAGES[key]


def _want(oracle, key):
    if key not in _WANT:
        _WANT[key] = OracleExtractor(N, 1.2, NL, 20, 7, oracle).extract(_image(key))
    return _WANT[key]


def _script(B, isolated_phase):
    """[('match', params or None) | ('isolated', bool) | ('push', geometry, [frame keys]) | ('pop',)], phases in order."""
    count = {'small': 0, 'wide': 0}

    def batch(kind, keys=None):
        if keys is None:
            keys = []
            for _ in range(B):
                keys.append((kind, count[kind]))
                count[kind] += 1
        return ('push', WIDE if kind == 'wide' else SMALL, keys)
    s = [('match', ON), batch('small'), batch('small'), ('pop',)]                              # 1. two matched batches
    s += [('match', None), batch('small'), ('pop',), ('match', ON), batch('small'), ('pop',)]  # 2. matching off for one batch, on again
    if isolated_phase:                                                                          # 3. isolated on for two, off for two
        s += [('isolated', True), batch('small'), batch('small'), ('pop',),
              ('isolated', False), batch('small'), batch('small'), ('pop',)]
    s += [('match', TIGHT), batch('small'), ('pop',)]                                           # 4. other matching parameters
    n_small = sum(1 for x in s if x[0] == 'push')
    assert n_small % 2 == 1   # so the first wide batch lands on a multi runner's sub[1] (or sub[2])
    # 5. the host route, which grows the row stride, and back with batches in flight.  (The first wide batch is popped on its own: a
    #    runner that reads it with an older stride then fails by assertion, inside the batch's buffers.)
    s += [('match', BOTH), batch('wide'), ('pop',), batch('wide'), batch('small'), batch('small'), ('pop',)]
    blank = ('blank', 0)
    last = batch('small')[2][:B - 1] + [blank]
    first = [blank] + batch('small')[2][:B - 1]
    s += [('match', ON), ('push', SMALL, last), ('push', SMALL, first), ('pop',)]               # 6. a frame without keypoints on a boundary
    return s


def _check(oracle, got, keys, pred0, match, where):
    kps, desc, n, m12, nm = got
    for i, key in enumerate(keys):
        wk, wd = _want(oracle, key)
        at = (where, i, key)
        assert n[i] == len(wk), at
        assert kps[i, :n[i]].tobytes() == wk.tobytes() and desc[i, :n[i]].tobytes() == wd.tobytes(), at
        pred = pred0 if i == 0 else keys[i - 1]
        if match is None or pred is None:
            assert nm[i] == 0 and (m12[i] == -1).all(), at
            continue
        window, ratio, ori, bounds = match
        pk, pd = _want(oracle, pred)
        on, om12, _ = oracle.search_for_initialization(pk, pd, wk, wd, bounds, np.stack([pk['x'], pk['y']], 1).reshape(-1, 2),
                                                       window, ratio, ori)
        assert nm[i] == on, at + (pred, nm[i], on)
        assert (m12[i, :len(pk)] == om12).all() and (m12[i, len(pk):] == -1).all(), at + (pred,)


def _run(api, oracle, st, script):
    keys = sorted({k for x in script if x[0] == 'push' for k in x[2]})
    dev, ptr = [], {}
    for geom in (SMALL, WIDE):
        ks = [k for k in keys if _image(k).shape == geom]
        d = api.DeviceFrames([_image(k) for k in ks], 0)
        dev.append(d)
        ptr.update({k: (p, d.stride) for k, p in zip(ks, d.ptrs)})
    for k in keys:
        _want(oracle, k)
    match, isolated, fresh, last = ON, False, True, None
    pending, total, grew = [], 0, False
    try:
        for b, step in enumerate(script):
            if step[0] == 'match':
                match = step[1]
                if match is None:
                    st.set_matching(B_SMALL, 0)
                else:
                    st.set_matching(match[3], match[0], match[1], match[2])
            elif step[0] == 'isolated':
                st.set_isolated_batches(step[1])
                if isolated and not step[1]:
                    fresh = True            # (c) the first batch after isolated batches are switched off
                isolated = step[1]
            elif step[0] == 'push':
                (h, w), ks = step[1], step[2]
                cap = st.cap
                st.push_ptrs([ptr[k][0] for k in ks], h, w, ptr[ks[0]][1], True)
                grew |= st.cap > cap
                pred0 = None if fresh or isolated else last   # (a) the first batch, (b) isolated batches
                fresh, last = False, ks[-1]
                pending.append((ks, pred0, match, b))
            else:
                for ks, pred0, m, at in pending:
                    got = st.pop(copy=True)
                    _check(oracle, got, ks, pred0, m, at)
                    total += int(got[4].sum())
                pending = []
    finally:
        st.close()
    assert grew, 'the wide frames were meant to grow the row stride'
    assert total > 100


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.mark.parametrize('bd', [(1, 4), (3, 2)], ids=['gpu-chain-batch1-depth4', 'gpu-chain-batch3-depth2'])
def test_stream_transitions_follow_the_predecessor_contract(api, oracle, bd):
    """orbfe_stream_*: matching off and on, isolated batches on and off, other matching parameters, the host-quadtree route (with a
    larger row stride) and back while batches are in flight, and a keypoint-less frame on a batch boundary -- on the GPU-resident
    matching chain."""
    B, depth = bd
    st = api.Stream(N, 1.2, NL, 20, 7, 0, B, depth)
    _run(api, oracle, st, _script(B, True))


@pytest.mark.parametrize('devices', [[0, 0], [0, 0, 0]])
def test_multi_runner_transitions_follow_the_predecessor_contract(api, oracle, devices):
    """orbfe_stream_multi_*: the same script without isolated batches (the sub-runners' batches always are).  An odd number of
    800 x 600 batches goes first, so that the first wide batch, which grows the row stride, lands on a sub-runner other than sub[0]."""
    st = api.MultiStream(N, 1.2, NL, 20, 7, devices, 2, 2)
    _run(api, oracle, st, _script(2, False))


def test_held_results_survive_and_misuse_is_refused(api, oracle):
    """orbfe_stream_pop_hold / _release: held results stay where they are while the runner goes on; a push that would grow the row
    stride, set_* and set_queue_slots are refused while a ticket is out, and so are a second release, a release of a ticket never
    handed out and orbfe_stream_pop."""
    B = 2
    small = [('small', 100 + i) for i in range(6 * B)]
    wide = [('wide', 100 + i) for i in range(B)]
    ds = api.DeviceFrames([_image(k) for k in small], 0)
    dw = api.DeviceFrames([_image(k) for k in wide], 0)
    for k in small + wide:
        _want(oracle, k)
    st = api.Stream(N, 1.2, NL, 20, 7, 0, B, 2)
    try:
        st.set_matching(B_BOTH, *BOTH[:3])
        keys = [small[b * B:(b + 1) * B] for b in range(6)]
        pred0 = [None] + [keys[b - 1][-1] for b in range(1, 6)]
        for b in range(3):
            st.push_ptrs(ds.ptrs[b * B:(b + 1) * B], SMALL[0], SMALL[1], ds.stride, True)
        held = [st.pop_hold() for _ in range(3)]
        st.push_ptrs(ds.ptrs[3 * B:4 * B], SMALL[0], SMALL[1], ds.stride, True)
        t3, v3 = st.pop_hold()
        cap = st.cap
        # nothing that would move a held result while one is out (the held views are read only after these)
        with pytest.raises(RuntimeError):
            st.push_ptrs(dw.ptrs, WIDE[0], WIDE[1], dw.stride, True)
        with pytest.raises(RuntimeError):
            st.set_matching(B_BOTH, *BOTH[:3])
        with pytest.raises(RuntimeError):
            st.set_queue_slots(st.queue_slots() + 4)
        assert st.cap == cap
        for b, (_, v) in enumerate(held + [(t3, v3)]):
            _check(oracle, v, keys[b], pred0[b], BOTH, b)
        st.release(t3)
        with pytest.raises(RuntimeError):
            st.release(t3)
        tickets = {t for t, _ in held}
        with pytest.raises(RuntimeError):
            st.release(min(set(range(st.queue_slots())) - tickets))
        with pytest.raises(RuntimeError):
            st.release(10 ** 6)
        st.push_ptrs(ds.ptrs[4 * B:5 * B], SMALL[0], SMALL[1], ds.stride, True)
        with pytest.raises(RuntimeError):
            st.pop()
        t4, v4 = st.pop_hold(copy=True)
        st.release(t4)
        _check(oracle, v4, keys[4], pred0[4], BOTH, 4)
        st.push_ptrs(ds.ptrs[5 * B:6 * B], SMALL[0], SMALL[1], ds.stride, True)   # goes on while three results are held
        t5, v5 = st.pop_hold()
        _check(oracle, v5, keys[5], pred0[5], BOTH, 5)
        st.release(t5)
        for b, (t, v) in enumerate(held):
            _check(oracle, v, keys[b], pred0[b], BOTH, b)
            st.release(t)
        st.push_ptrs(dw.ptrs, WIDE[0], WIDE[1], dw.stride, True)
        assert st.cap > cap
        _check(oracle, st.pop(copy=True), wide, keys[5][-1], BOTH, 'wide')
    finally:
        st.close()
