"""orbfe_local_map_refresh_rows on the GPU against the CPU restatement tests/cpp/map_point_refresh_ref.cpp: the table's rows byte
for byte, the host outputs, equivalence with the route it replaces (orbfe_distinctive_descriptors + host restatement +
set_rows), the projection that consumes the rows, every refusal, and the C++ facade on the stub map.

Shapes (tests/map_point_refresh_util.py make_scene): N in {1, 2, 3, 63, 64, 65, 129} observations; first and last bad; all bad;
empty; duplicate descriptors; two MapPoints sharing keyframes; a NULL frame slot named by a bad observation only; bad
observations on both sides of the 64-observation pass boundary; |pos - Ow| = sqrt(3); a sum that ends in -0."""
import numpy as np
import pytest

import map_point_refresh_util as U

pytestmark = pytest.mark.gpu
f32 = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)
BOTH = U.DESCRIPTOR | U.NORMAL_DEPTH
ALL_ROWS = np.arange(U.CAPACITY, dtype=np.int32)


class World:
    pass


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from os1_amd import api
    w = World()
    w.api = api
    w.ref = U.build_ref(tmp_path_factory.mktemp('mpr_ref'))
    w.kfs, w.table, w.batch = U.make_scene()
    w.m = api.Matcher(0)
    w.frames = [None if s == U.NULL_SLOT else api.Frame.from_host(w.m, k.kps, k.desc, BOUNDS) for s, k in enumerate(w.kfs)]
    w.Ow = np.stack([k.Ow for k in w.kfs]).astype(f32)
    w.want = {what: U.ref_refresh(w.ref, w.table, what, w.kfs, w.batch) for what in (U.DESCRIPTOR, U.NORMAL_DEPTH, BOTH)}
    yield w
    for f in w.frames:
        if f is not None:
            f.close()
    w.m.close()


def fresh_map(w):
    lm = w.api.LocalMap(w.m, U.CAPACITY)
    tf = w.table.view(f32).reshape(-1, 16)
    lm.set_rows(ALL_ROWS, tf[:, 0:3], tf[:, 3:6], tf[:, 6], tf[:, 7], w.table[:, 32:])
    return lm


def refresh(w, lm, what, b=None, frames=None, nlevels=U.NLEVELS, sf=U.SF, outputs=True):
    b = b or w.batch
    return lm.refresh_rows(what, w.frames if frames is None else frames, w.Ow, b.rows, b.offs, b.kf, b.kp, b.fl, b.ref_kf, b.ref_kp,
                           scale_factors=sf, nlevels=nlevels, outputs=outputs)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize('what', (U.DESCRIPTOR, U.NORMAL_DEPTH, BOTH))
def test_rows_and_host_outputs_equal_the_restatement(world, what):
    w = world
    lm = fresh_map(w)
    best, nrm, mn, mx = refresh(w, lm, what)
    t, wbest, wnrm, wmn, wmx, rc = w.want[what]
    assert rc == 0
    got = lm.download_rows(ALL_ROWS)
    for p, name in enumerate(w.batch.names):
        assert got[w.batch.rows[p]].tobytes() == t[w.batch.rows[p]].tobytes(), name
    assert got.tobytes() == t.tobytes()                              # rows outside the batch, pos, unselected fields
    assert got[:, :12].tobytes() == w.table[:, :12].tobytes()
    if not (what & U.DESCRIPTOR):
        assert got[:, 32:].tobytes() == w.table[:, 32:].tobytes() and (best == -1).all()
    if not (what & U.NORMAL_DEPTH):
        assert got[:, 12:32].tobytes() == w.table[:, 12:32].tobytes()
    assert best.tolist() == wbest.tolist()
    assert bits(nrm).tolist() == bits(wnrm).tolist()
    assert bits(mn).tolist() == bits(wmn).tolist() and bits(mx).tolist() == bits(wmx).tolist()
    i = w.batch.names.index('neg_zero')
    if what & U.NORMAL_DEPTH:
        assert bits(nrm[i])[0] == 0                                  # +0, not -0
    lm.close()


def test_enqueue_only_call_is_ordered_before_the_download(world):
    w = world
    lm = fresh_map(w)
    assert refresh(w, lm, BOTH, outputs=False) is None
    assert lm.download_rows(ALL_ROWS).tobytes() == w.want[BOTH][0].tobytes()
    lm.close()


def old_route(w, lm):
    """orbfe_distinctive_descriptors on host-gathered lists + the host restatement of UpdateNormalAndDepth + set_rows."""
    b = w.batch
    lists, kept_at = [], []
    for o in b.obs_lists:
        kept = [i for i, t in enumerate(o) if not t[2]]
        kept_at.append(kept)
        lists.append(np.stack([w.kfs[o[i][0]].desc[o[i][1]] for i in kept]) if kept else np.zeros((0, 32), np.uint8))
    best = w.m.distinctive_descriptors(lists)
    rows_d = [p for p in range(len(lists)) if best[p] >= 0]
    lm.set_rows(b.rows[rows_d], desc=np.stack([lists[p][best[p]] for p in rows_d]))
    tf = w.table.view(f32).reshape(-1, 16)
    rows_g, nrm, mn, mx = [], [], [], []
    for p, o in enumerate(b.obs_lists):
        if not o:
            continue
        k = w.kfs[b.ref_kf[p]]
        n3, a, c = U.ref_normal_depth(w.ref, tf[b.rows[p], 0:3], np.stack([w.kfs[s].Ow for s, _, _ in o]), k.Ow, U.SF[k.oct[b.ref_kp[p]]], U.SF[-1])
        rows_g.append(p); nrm.append(n3); mn.append(a); mx.append(c)
    lm.set_rows(b.rows[rows_g], normal=np.stack(nrm), min_raw=np.array(mn, f32), max_raw=np.array(mx, f32))
    return [kept_at[p][best[p]] if best[p] >= 0 else -1 for p in range(len(lists))]


def test_same_rows_as_the_route_it_replaces_and_same_projection(world):
    w = world
    new, old = fresh_map(w), fresh_map(w)
    best, _, _, _ = refresh(w, new, BOTH)
    assert best.tolist() == old_route(w, old)
    a, b = new.download_rows(ALL_ROWS), old.download_rows(ALL_ROWS)
    assert a.tobytes() == b.tobytes()
    # the consumer: Frame::isInFrustum over both tables, a camera at the origin looking down +z
    cam = w.api.Camera.make(np.eye(3), np.zeros(3), np.zeros(3), 500.0, 500.0, 320.0, 240.0, np.log(1.2))
    f = w.frames[1]
    flags = np.zeros(len(w.batch.rows), np.uint8)
    pa = w.m.project_local_map(f, new, cam, w.batch.rows, flags)
    pb = w.m.project_local_map(f, old, cam, w.batch.rows, flags)
    assert pa['n_in_view'] == pb['n_in_view'] and pa['n_in_view'] > 0
    for k in ('in_view', 'level', 'view_cos'):
        assert pa[k].tobytes() == pb[k].tobytes(), k
    new.close()
    old.close()


def test_refusals_leave_the_table_unchanged(world):
    w = world
    api = w.api
    lm = fresh_map(w)
    before = lm.download_rows(ALL_ROWS)
    i3 = w.batch.names.index('n3')

    def refused(mutate, **kw):
        b = w.batch.copy()
        mutate(b)
        with pytest.raises(api.OrbfeError) as e:
            refresh(w, lm, BOTH, b=b, **kw)
        assert e.value.code == -1, e.value
        assert lm.download_rows(ALL_ROWS).tobytes() == before.tobytes()

    def set_(arr, i, v):
        def f(b):
            getattr(b, arr)[i] = v
        return f
    o3 = int(w.batch.offs[i3])
    refused(set_('rows', 2, U.CAPACITY))                             # a row outside [0, capacity)
    refused(set_('rows', 2, -1))
    refused(set_('rows', 2, int(w.batch.rows[5])))                   # a row named twice
    refused(set_('offs', i3 + 1, o3 - 1))                            # non-monotone offsets
    refused(set_('kf', o3, len(w.kfs)))                              # a slot outside [0, n_kf)
    refused(set_('kf', o3, -1))
    refused(set_('kp', o3, w.kfs[w.batch.kf[o3]].n))                 # a keypoint index outside its frame
    refused(set_('kp', o3, -1))
    refused(set_('ref_kp', i3, w.kfs[w.batch.ref_kf[i3]].n))
    refused(set_('ref_kf', i3, len(w.kfs)))
    refused(set_('kf', o3, U.NULL_SLOT))                             # a NULL frame behind an observation that is not bad
    refused(lambda b: None, nlevels=0)                               # nlevels outside 1..32
    refused(lambda b: None, nlevels=33, sf=np.ones(33, f32))
    if api.device_count() > 1:                                       # a frame on another device
        m1 = api.Matcher(1)
        other = api.Frame.from_host(m1, w.kfs[1].kps, w.kfs[1].desc, BOUNDS)
        refused(lambda b: None, frames=[w.frames[0], other] + w.frames[2:])
        other.close()
        m1.close()
    # n_mp == 0 is fine and does nothing
    empty = U.Batch([], [], [])
    assert refresh(w, lm, BOTH, b=empty)[0].size == 0
    assert lm.download_rows(ALL_ROWS).tobytes() == before.tobytes()
    # and the handles still work
    refresh(w, lm, BOTH)
    assert lm.download_rows(ALL_ROWS).tobytes() == w.want[BOTH][0].tobytes()
    lm.close()


def test_out_of_range_level_fails_and_leaves_everything_usable(world):
    w = world
    lm = fresh_map(w)
    t, _, _, _, _, rc = U.ref_refresh(w.ref, w.table, BOTH, w.kfs, w.batch, nlevels=4, sf=U.SF[:4])
    assert rc < 0
    with pytest.raises(w.api.OrbfeError) as e:
        refresh(w, lm, BOTH, nlevels=4, sf=U.SF[:4])
    assert e.value.code == -1 and 'MapPoint %d' % (-1 - rc) in str(e.value)
    got = lm.download_rows(ALL_ROWS)
    levels = [w.kfs[w.batch.ref_kf[p]].oct[w.batch.ref_kp[p]] if o else 0 for p, o in enumerate(w.batch.obs_lists)]
    for p, l in enumerate(levels):
        if l >= 4:
            assert got[w.batch.rows[p]].tobytes() == w.table[w.batch.rows[p]].tobytes()   # left unwritten
    assert got.tobytes() == t.tobytes()
    best, nrm, mn, mx = refresh(w, lm, BOTH)                          # matcher, frames and table are usable
    assert lm.download_rows(ALL_ROWS).tobytes() == w.want[BOTH][0].tobytes()
    assert best.tolist() == w.want[BOTH][1].tolist()
    lm.close()


def test_facade_on_the_stub_map(tmp_path):
    U.run_facade(U.compile_facade(str(tmp_path / 'mpr_gpu'), host_backend=False))
