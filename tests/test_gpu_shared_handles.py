"""-m gpu: resident frames and maps used the way the reference uses them -- built through one matcher and consumed through another,
destroyed behind work that is still queued, and read by three host threads at once.  Every call's result is compared with the value
tests/shared_handles_util.py computes on the CPU from the oracle or from the restatement that call is pinned to (tests/
test_shared_handles.py shows those values are not empty); where two matchers make the same call, the two results are compared byte
for byte as well.  No reference of its own: the question is only whether the pinned answer survives sharing.

WHERE EVERY orbfe_frame*-TAKING ENTRY POINT WAITS FOR THE FRAME'S `ready` EVENT (checked in the code; `st` = the caller's stream):
  orbfe_search_by_projection_frame, _frame_rows, _uv_frame, orbfe_search_projected_frame
                                              run_search (orbfe_frame.hip): hipStreamWaitEvent(st, f->ready) in front of k_window_match
  orbfe_search_local_points_frame             the projection kernel reads only the frame's bounds (host fields); the search behind it
                                              goes through sbp_frame_device_queries -> run_search
  orbfe_search_by_projection_sources_frame    src_frame: frame_wait_ready in front of k_project_sources (orbfe_localmap.hip);
                                              cur_frame: sbp_uv_frame_device_queries -> run_search
  orbfe_search_projected_keyframe_frame       search_projected_frame_device_queries -> run_search (the projection: bounds only)
  orbfe_project_local_map, orbfe_project_keyframe   no device memory of the frame is read (bounds only): nothing to wait for
  orbfe_project_sources                       src_frame: frame_wait_ready in front of k_project_sources; cur_frame: bounds only
  orbfe_search_for_triangulation_frames_batch, _frames   frame_wait_ready for frame1 and every frame2 on the call's stream, behind
                                              the upload and in front of k_bow_triangulate_batch (orbfe_bow.hip)
  orbfe_local_map_refresh_rows                frame_wait_ready per non-NULL slot in front of the upload (orbfe_mprefresh.hip)
  orbfe_score_init_hypotheses_frames          frame_wait_ready(f1), (f2) in front of the gather (orbfe_initscore.hip)
  orbfe_frame_descriptors_device, orbfe_frame_download   a HOST wait (hipEventSynchronize(ready)): the rows are complete on return
  orbfe_frame_destroy                         hipEventSynchronize(ready), then hipFree / hipHostFree
  orbfe_frame_size, orbfe_frame_device        host fields, set before orbfe_frame_create returns
No entry point lacks its wait, so section 1 found nothing to fix.

WHICH CALLS CAN RETURN BEFORE THEIR KERNELS COMPLETE: orbfe_frame_create / _create_from_extract (always), orbfe_local_map_set_rows,
orbfe_matcher_upload_async, and orbfe_local_map_refresh_rows when no host output is asked for and no keyframe holds an octave >=
nlevels.  Every search, both triangulation forms (one upload, one launch, one download, one wait), the Initializer scoring, the
covisibility and culling counts, the database queries and the BoW transforms return after their kernels.  So only the refresh can
leave a reader of a frame behind; destroying the frame then is safe because ~orbfe_frame frees with hipFree, which waits for every
stream of the device (hip_buffers.h DevBuf::release: plain hipMalloc / hipFree, no pool) -- test_destroy_behind_an_enqueue_only_refresh
keeps that pinned should the buffers ever become pooled.

THE WINDOW.  A search cannot be queued without waiting for it (it returns on its kernel's completion word), so the work in front of
the frame builds is what the API can queue: orbfe_matcher_upload_async of a 32 MB page-locked block, several times, on matcher A's
stream -- milliseconds of DMA, behind which the builds wait while B's call is submitted.  On correct code the tests pass whether or
not the builds are still pending; a missing wait is caught only while they are, i.e. with high probability, not with certainty.

Reverting one wait, dry: take frame_wait_ready(kf_frames[s], m->stream) of orbfe_local_map_refresh_rows away.  In
the 'refresh' entry of test_built_on_a_consumed_through_b B's stream then holds nothing that orders k_refresh_map_points behind A's stream; A's
stream is still copying the block, the keyframes' D.desc and D.oct are fresh hipMalloc memory no kernel has written, and the
kernel gathers whatever lies there: the rows and best_obs differ from the restatement's, both with and without host outputs.  The
single-matcher tests cannot see this -- their consumer is stream-ordered behind the build.  The same argument holds for each wait
listed above, with the entry of ENTRY_POINTS that goes through it.

Measured on an MI355X (RUN_TIMES below): the whole module 3 s, 1.9 s of it the CPU expectations; the three-roles test 0.16 s at ROUNDS =
40 (its threads' loops 0.1 s), so the count stays at 40; section 1, nine entry points in one test, 0.5 s, its slowest entry (refresh: 131 keyframes, a 43 ms hold) 0.10 s.  The
call through B lasted 5.0 - 5.8 ms (43 ms for the refresh) against 0.11 - 0.18 ms (0.8 ms) for the same call through A afterwards: it
did wait for builds that were still pending."""
import threading
import time

import numpy as np
import pytest

import init_score_util as IS
import keyframe_projection_util as KP
import local_map_util as LM
import map_point_refresh_util as MR
import shared_handles_util as SH
import source_projection_util as SP
import triangulation_batch_util as TB

pytestmark = pytest.mark.gpu

# whole-test wall times measured on an MI355X (s): the three-roles test at ROUNDS = 40, the slowest section-1 case
RUN_TIMES = dict(three_roles=0.16, slowest_entry_point=0.10)
ROUNDS = 40
JOIN_S = 120.0
BLOCK_ROWS = 1 << 20                       # 32 MB of page-locked memory and as much device memory
ALL_ROWS = np.arange(MR.CAPACITY, dtype=np.int32)


class Env:
    pass


@pytest.fixture(scope='module')
def env(tmp_path_factory):
    from os1_amd import api
    assert api.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    e = Env()
    e.api = api
    e.w = SH.world(tmp_path_factory.mktemp('shared_handles'))
    e.block = api.DescTable(BLOCK_ROWS)
    yield e
    api.device_synchronize(0)
    e.block.free()


def hold(env, m, n=8):
    """n copies of the block queued on m's stream: what m submits next waits behind milliseconds of DMA"""
    for _ in range(n):
        env.block.upload(m, 0, BLOCK_ROWS)


def table_of(api, m, tab):
    n = len(tab['pos'])
    lm = api.LocalMap(m, n)
    lm.set_rows(np.arange(n), tab['pos'], tab['normal'], tab['min'], tab['max'], tab['desc'])
    return lm


def refresh_table(api, m, table):
    lm = api.LocalMap(m, MR.CAPACITY)
    tf = table.view(np.float32).reshape(-1, 16)
    lm.set_rows(ALL_ROWS, tf[:, 0:3], tf[:, 3:6], tf[:, 6], tf[:, 7], table[:, 32:])
    return lm


def blob(x):
    """a call's result as bytes, for the comparison of two matchers' results"""
    if isinstance(x, dict):
        return [(k, blob(x[k])) for k in sorted(x)]
    if isinstance(x, (tuple, list)):
        return [blob(v) for v in x]
    if isinstance(x, IS.Result) or type(x).__name__ == 'InitScores':
        return [blob(getattr(x, k)) for k in ('scores_h', 'scores_f', 'best_h', 'best_f', 'score_h', 'score_f', 'inliers_h', 'inliers_f', 'n_matches')]
    if x is None:
        return None
    return np.asarray(x).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# The calls: build(api, m, w) -> frames, tables(api, m, w) -> local maps of matcher m, call(api, m, w, frames, maps) -> result,
# check(w, result) -> asserts the result is the CPU's.  One entry per consuming entry point.
# ---------------------------------------------------------------------------------------------------------------------------------
def _fr(api, m, w, k, d):
    return api.Frame.from_host(m, k, d, w.bounds)


def _no_tables(api, m, w):
    return []


def _build_b(api, m, w):
    return [_fr(api, m, w, w.kB, w.dB)]


def _call_sbp(api, m, w, fr, maps):
    s = w.sbp
    return m.search_by_projection(fr[0], None, None, w.sf, s['occ'], s['xy'], s['level'], s['viewcos'], s['flags'], s['desc'], s['th'], s['nnratio'])


def _check_sbp(w, got):
    assert got[0] == w.sbp['nmatches'] and (got[1] == w.sbp['kp_assigned']).all()


def _call_projected(api, m, w, fr, maps):
    p = w.projected
    return m.search_projected(fr[0], None, None, p['uv'], p['radius'], p['level'], p['valid'], p['sdesc'], p['kp_skip'], p['claim'], p['inv_sigma2'],
                              5.99, p['max_dist'])


def _check_projected(w, got):
    p = w.projected
    assert got[0] == p['nmatches'] and got[1].tobytes() == p['best_idx'].tobytes() and got[2].tobytes() == p['best_dist'].tobytes()


def _build_ba(api, m, w):
    return [_fr(api, m, w, w.kB, w.dB), _fr(api, m, w, w.kA, w.dA)]


def _tables_sources(api, m, w):
    return [table_of(api, m, w.sources['sc']['tab'])]


def _call_sources(api, m, w, fr, maps):
    s = w.sources
    sc = s['sc']
    return m.search_by_projection_sources(fr[0], fr[1], maps[0], LM.api_camera(api, sc['cam']), s['mode'], sc['rows'], s['want']['flags'],
                                          sc['st']['occ'], w.sf, s['th'], s['max_dist'], True)


def _check_sources(w, got):
    want, sc = w.sources['want'], w.sources['sc']
    SP.check_projection(got, want['proj'])
    assert got['nmatches'] == want['nmatches']
    assert (SP.cur_mp_from_assigned(want['before'], got['kp_assigned'], sc['rows']) == want['cur_mp']).all()


def _tables_kfproj(api, m, w):
    return [table_of(api, m, w.kfproj['sc']['tab'])]


def _call_kfproj(api, m, w, fr, maps):
    k = w.kfproj
    d = k['d']
    return m.search_projected_keyframe(fr[0], maps[0], KP.api_projection(api, d['pr']), d['rows'], d['flags'], w.sf, float(k['th']),
                                       kp_skip=d['kp_skip'], claim=d['claim'], inv_sigma2=SH.inv_sigma2(w.sf) if d['chi2'] else None, chi2=5.99,
                                       max_dist=d['max_dist'])


def _check_kfproj(w, got):
    k = w.kfproj
    KP.check_projection(got, k['proj'])
    assert (got['best_idx'] == k['best']).all() and got['nmatches'] == int((k['best'] >= 0).sum())


def _tables_local(api, m, w):
    return [table_of(api, m, w.local['mp'])]


def _call_local(api, m, w, fr, maps):
    c = w.local
    return m.search_local_points(fr[0], maps[0], LM.api_camera(api, c['cam']), c['rows'], c['flags'], c['occ'], w.sf, c['th'])


def _check_local(w, got):
    c = w.local
    for k in ('in_view', 'proj_xy', 'level', 'view_cos'):
        assert got[k].tobytes() == np.ascontiguousarray(c['proj'][k]).tobytes(), k
    assert got['n_in_view'] == c['proj']['n_in_view'] and got['nmatches'] == c['nmatches'] and (got['kp_assigned'] == c['kp_assigned']).all()


def _build_tri(api, m, w):
    job = w.tri['job']
    return [_fr(api, m, w, kf['kps'], kf['desc']) for kf in [job['kf1']] + job['nb']]


def _call_tri(api, m, w, fr, maps):
    job = w.tri['job']
    return m.search_for_triangulation_frames_batch(fr[0], job['kf1']['has'], job['kf1']['fv'], [TB.neighbour_arg(f, nb) for f, nb in zip(fr[1:], job['nb'])])


def _check_tri(w, got):
    assert got.dtype == np.int32 and got.tobytes() == w.tri['raw'].tobytes()


def _build_refresh(api, m, w, flip=False):
    return [None if s == MR.NULL_SLOT else _fr(api, m, w, k.kps, ~k.desc if flip else k.desc) for s, k in enumerate(w.refresh['kfs'])]


def _tables_refresh(api, m, w):
    return [refresh_table(api, m, w.refresh['table']), refresh_table(api, m, w.refresh['table'])]


def _refresh(w, lm, frames, outputs):
    r = w.refresh
    b = r['batch']
    return lm.refresh_rows(SH.BOTH, frames, r['Ow'], b.rows, b.offs, b.kf, b.kp, b.fl, b.ref_kf, b.ref_kp, scale_factors=MR.SF, nlevels=MR.NLEVELS,
                           outputs=outputs)


def _call_refresh(api, m, w, fr, maps):
    """once with the host outputs, once without (enqueue-only) on a second table, each followed by the rows' download"""
    out = _refresh(w, maps[0], fr, True)
    rows = maps[0].download_rows(ALL_ROWS)
    assert _refresh(w, maps[1], fr, False) is None
    return dict(out=out, rows=rows, rows_enqueue_only=maps[1].download_rows(ALL_ROWS))


def _check_refresh(w, got):
    r = w.refresh
    assert got['rows'].tobytes() == r['rows_after'].tobytes() and got['rows_enqueue_only'].tobytes() == r['rows_after'].tobytes()
    best, nrm, mn, mx = got['out']
    assert best.tolist() == r['best'].tolist()
    for g, want in ((nrm, r['normal']), (mn, r['min']), (mx, r['max'])):
        assert np.ascontiguousarray(g, np.float32).tobytes() == np.ascontiguousarray(want, np.float32).tobytes()


def _build_init(api, m, w):
    i = w.init
    rng = np.random.default_rng(1)
    return [_fr(api, m, w, k, rng.integers(0, 256, (len(k), 32), dtype=np.uint8)) for k in (i['k1'], i['k2'])]


def _call_init(api, m, w, fr, maps):
    i = w.init
    return m.score_init_hypotheses_frames(fr[0], fr[1], i['m12'], IS.SIGMA, i['H21'], i['H12'], i['F21'])


def _check_init(w, got):
    IS.assert_same(got, w.init['want'], 'frames')
    assert got.n_matches == w.init['n']


def _build_ab(api, m, w):
    return [_fr(api, m, w, w.kA, w.dA), _fr(api, m, w, w.kB, w.dB)]


def _call_device_rows(api, m, w, fr, maps):
    """frame A's resident descriptor rows are the query rows of a search on frame B"""
    u = w.uv
    rows = fr[0].descriptors_device()
    assert len(rows) == len(w.kA) and rows.ptr % 16 == 0
    return m.search_by_projection_uv(fr[1], None, None, w.sf, u['occ'], u['uv'], u['level'], u['angle'], u['flags'], u['valid'], rows, u['th'],
                                     u['max_dist'], 0, True)


def _check_device_rows(w, got):
    assert got[0] == w.uv['nmatches'] and (got[1] == w.uv['kp_assigned']).all()


ENTRY_POINTS = {
    'search_by_projection': (_build_b, _no_tables, _call_sbp, _check_sbp),
    'search_projected': (_build_b, _no_tables, _call_projected, _check_projected),
    'search_by_projection_sources': (_build_ba, _tables_sources, _call_sources, _check_sources),
    'search_projected_keyframe': (_build_b, _tables_kfproj, _call_kfproj, _check_kfproj),
    'search_local_points_frame': (_build_b, _tables_local, _call_local, _check_local),
    'triangulation_batch': (_build_tri, _no_tables, _call_tri, _check_tri),
    'refresh': (_build_refresh, _tables_refresh, _call_refresh, _check_refresh),
    'init_score_frames': (_build_init, _no_tables, _call_init, _check_init),
    'descriptors_device': (_build_ab, _no_tables, _call_device_rows, _check_device_rows),
}


def _close(*things):
    for t in things:
        for h in (t if isinstance(t, (list, tuple)) else [t]):
            if h is not None:
                h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. built on matcher A, consumed at once through matcher B
# ---------------------------------------------------------------------------------------------------------------------------------
def _built_on_a_consumed_through_b(env, name):
    api, w = env.api, env.w
    build, tables, call, check = ENTRY_POINTS[name]
    A, B = api.Matcher(0), api.Matcher(0)
    frames, maps_a, maps_b = [], [], []
    try:
        maps_a, maps_b = tables(api, A, w), tables(api, B, w)      # a local map belongs to the matcher that searches through it
        A.synchronize()                                             # (A's own uploads are done: only the hold and the builds will be pending)
        n_frames = {'triangulation_batch': 4, 'refresh': len(w.refresh['kfs'])}.get(name, 2)
        hold(env, A, 8 + n_frames // 2)                             # (131 builds take the host longer: a longer hold)
        frames += build(api, A, w)
        t0 = time.perf_counter()
        got_b = call(api, B, w, frames, maps_b)                     # no host synchronisation since the builds were queued
        t1 = time.perf_counter()
        for f in frames:
            if f is not None:
                f.download()                                        # forces completion
        t2 = time.perf_counter()
        got_a = call(api, A, w, frames, maps_a)
        # (a figure, not an assertion: B's call lasting milliseconds longer than A's says it waited for builds that were still pending)
        print('%s: through B %.2f ms, through A afterwards %.2f ms' % (name, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t2)))
        check(w, got_b)
        check(w, got_a)
        assert blob(got_b) == blob(got_a), 'the two matchers\' results differ'
    finally:
        _close(frames, maps_a, maps_b, A, B)                        # maps and frames before the matchers, whatever happened


def test_built_on_a_consumed_through_b(env):
    """Every entry of ENTRY_POINTS, one after the other in one test (0.3 s in all); an entry that fails does not hide the others: the
    failures are collected per entry point and asserted at the end, with the handles of the failed entry closed in order."""
    import traceback
    failed = {}
    for name in ENTRY_POINTS:
        try:
            _built_on_a_consumed_through_b(env, name)
        except AssertionError:
            failed[name] = traceback.format_exc(limit=-3)
    assert not failed, '\n'.join('%s:\n%s' % kv for kv in failed.items())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. destroying frames behind an enqueue-only call
# ---------------------------------------------------------------------------------------------------------------------------------
def test_destroy_behind_an_enqueue_only_refresh(env):
    """Cannot go wrong today: ~orbfe_frame releases with hipFree, which synchronises the device, so the queued kernel has read the rows
    before they are freed.  (No triangulation form returns before completion: nothing of the kind to test there.)"""
    api, w = env.api, env.w
    A, B = api.Matcher(0), api.Matcher(0)
    lm = refresh_table(api, B, w.refresh['table'])
    frames = _build_refresh(api, A, w)
    hold(env, B, 8)                                                 # the refresh kernel stays queued behind this
    assert _refresh(w, lm, frames, False) is None
    _close(frames)                                                  # LocalMapping's next step: the culled keyframes go
    again = _build_refresh(api, A, w, flip=True)                    # the same sizes, other bytes: a freed allocation would be reused
    rows = lm.download_rows(ALL_ROWS)
    assert rows.tobytes() == w.refresh['rows_after'].tobytes()
    _close(again, lm, A, B)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3 + 4. three roles at once on shared keyframes, and a fourth thread whose calls are refused
# ---------------------------------------------------------------------------------------------------------------------------------
class Role(threading.Thread):
    """A host thread that owns its handles and loops a fixed number of rounds over named calls, counting mismatches per call."""

    def __init__(self, name, stop, setup, calls, rounds=ROUNDS):
        super().__init__(name=name, daemon=True)
        self.stop_flag, self.setup, self.calls, self.rounds = stop, setup, calls, rounds
        self.bad = {n: 0 for n, _ in calls}
        self.done = {n: 0 for n, _ in calls}
        self.error = None
        self.last_error = None

    def run(self):
        from os1_amd import api
        own = None
        try:
            own = self.setup()
            for _ in range(self.rounds):
                for n, fn in self.calls:
                    if self.stop_flag.is_set():
                        return
                    try:
                        fn(own)
                    except AssertionError:
                        self.bad[n] += 1
                    self.done[n] += 1
            self.last_error = api.load_library().orbfe_last_error()     # this thread's own message
        except BaseException as e:                                     # noqa: B036 -- carried to the main thread, re-raised after the join
            self.error = e
            self.stop_flag.set()
        finally:
            if own is not None:
                _close(*reversed(list(own.values())))                      # maps and frames before the matcher they were made through


def _same(got, want):
    assert len(got) == len(want)
    for g, r in zip(got, want):
        assert np.array_equal(g, r)


def test_three_roles_on_shared_keyframes_and_a_thread_of_refused_calls(env):
    """Tracking, LocalMapping and LoopClosing, each a host thread with handles of its own, ROUNDS rounds each, on keyframes built
    once through a fourth matcher and never synchronised by the host.  Shared, read-only (include/orbfe.h says so per call): the
    triangulation job's four keyframes (LocalMapping's batch reads them while LoopClosing transforms their device rows), the 131
    keyframes of the refresh, and frame A as Tracking's source keyframe and descriptor rows.  Each searching thread owns the frame it
    searches.  Beside them a fourth thread makes calls that are refused -- one from the culling, the refresh and the triangulation
    refusal lists -- and must see its own code and message every time; the looping threads must see no error at all."""
    api, w = env.api, env.w
    L = api.load_library()
    t0 = time.perf_counter()
    M0 = api.Matcher(0)
    tri = _build_tri(api, M0, w)
    kfs = _build_refresh(api, M0, w)
    frame_a = _fr(api, M0, w, w.kA, w.dA)
    db = api.KeyFrameDatabase(w.kfdb['scene']['n_words'], w.kfdb['scene']['scoring'], w.kfdb['scene']['cap_k'], w.kfdb['scene']['cap_e'])
    for k in w.kfdb['adds']:
        kf = w.kfdb['scene']['kfs'][k]
        db.add(SH.KEY0 + k, kf['words'], kf['values'])
    stop = threading.Event()

    # ---- Tracking --------------------------------------------------------------------------------------------------------------
    def tracking_setup():
        m = api.Matcher(0)
        return dict(m=m, fr=[_fr(api, m, w, w.kB, w.dB)], local=_tables_local(api, m, w), sources=_tables_sources(api, m, w))

    tracking = [
        ('search_by_projection', lambda o: _check_sbp(w, _call_sbp(api, o['m'], w, o['fr'], None))),
        ('search_local_points_frame', lambda o: _check_local(w, _call_local(api, o['m'], w, o['fr'], o['local']))),
        ('search_by_projection_sources', lambda o: _check_sources(w, _call_sources(api, o['m'], w, [o['fr'][0], frame_a], o['sources']))),
        ('descriptors_device', lambda o: _check_device_rows(w, _call_device_rows(api, o['m'], w, [frame_a, o['fr'][0]], None))),
    ]

    # ---- LocalMapping ----------------------------------------------------------------------------------------------------------
    def mapping_setup():
        m = api.Matcher(0)
        return dict(m=m, maps=_tables_refresh(api, m, w))

    def refresh_call(o):
        got = dict(out=_refresh(w, o['maps'][0], kfs, True), rows=o['maps'][0].download_rows(ALL_ROWS))
        got['rows_enqueue_only'] = got['rows']
        _check_refresh(w, got)

    c, v = w.culling, w.covis
    mapping = [
        ('triangulation_batch', lambda o: _check_tri(w, _call_tri(api, o['m'], w, tri, None))),
        ('refresh', refresh_call),
        ('covisibility_special', lambda o: _same(api.covisibility_counts(o['m'], *v['special'].args()), v['special_want'])),
        ('covisibility_small', lambda o: _same(api.covisibility_counts(o['m'], *v['small'].args()), v['small_want'])),
        ('redundant_crafted', lambda o: _same(o['m'].redundant_observations(*c['crafted'].args()), c['crafted_want'])),
        ('redundant_cut_map', lambda o: _same(o['m'].redundant_observations(*c['cut'].args()), c['cut_want'])),
    ]

    # ---- LoopClosing -----------------------------------------------------------------------------------------------------------
    def closing_setup():
        return dict(voc=api.Vocabulary(w.bow['image']))

    def query_call(name, qw, qv):
        def f(o):
            keys, common, scores = db.query(qw, qv)
            rk, rc, rs = w.kfdb['want'][name]
            assert (keys.astype(np.int64) - SH.KEY0).tolist() == rk.tolist() and common.tolist() == rc.tolist()
            assert np.asarray(scores, np.float64).tobytes() == np.asarray(rs, np.float64).tobytes()
        return f

    def bow_sets(o):
        got = o['voc'].transform_batch(w.bow['sets'], SH.BOW_LEVELSUP)
        assert [SH.flat_bow(g) for g in got] == w.bow['want']

    def bow_keyframes(o):
        got = o['voc'].transform_batch([f.descriptors_device() for f in tri], SH.BOW_LEVELSUP)
        assert [SH.flat_bow(g) for g in got] == w.bow['kf_want']

    closing = [('query_' + n, query_call(n, qw, qv)) for n, qw, qv in SH.kfdb_queries(w.kfdb['scene'])] + \
              [('bow_batch_sets', bow_sets), ('bow_batch_shared_keyframes', bow_keyframes)]

    # ---- the refused calls -----------------------------------------------------------------------------------------------------
    def refused_setup():
        m = api.Matcher(0)
        return dict(m=m, maps=[refresh_table(api, m, w.refresh['table'])])

    def refused(word, fn):
        def f(o):
            with pytest.raises(api.OrbfeError) as e:
                fn(o)
            assert e.value.code == -1 and word in str(e.value), e.value
            assert word.encode() in L.orbfe_last_error()
        return f

    bad_cull = c['crafted'].but(obs_kf=np.concatenate([c['crafted'].obs_kf[:2], [400], c['crafted'].obs_kf[3:]]).astype(np.int32))
    bad_batch = w.refresh['batch'].copy()
    bad_batch.rows[2] = MR.CAPACITY
    job = w.tri['job']
    bad_fv = [a.copy() for a in job['kf1']['fv']]
    bad_fv[2][0] = len(job['kf1']['kps'])

    def refresh_refused(o):
        r, b = w.refresh, bad_batch
        o['maps'][0].refresh_rows(SH.BOTH, kfs, r['Ow'], b.rows, b.offs, b.kf, b.kp, b.fl, b.ref_kf, b.ref_kp, scale_factors=MR.SF, nlevels=MR.NLEVELS)

    refusals = [
        ('culling', refused('obs_kf[2] = 400', lambda o: o['m'].redundant_observations(*bad_cull.args()))),
        ('refresh', refused('outside the local map', refresh_refused)),
        ('triangulation', refused('feature index', lambda o: o['m'].search_for_triangulation_frames_batch(
            tri[0], job['kf1']['has'], bad_fv, [TB.neighbour_arg(f, nb) for f, nb in zip(tri[1:], job['nb'])]))),
    ]

    roles = [Role('Tracking', stop, tracking_setup, tracking), Role('LocalMapping', stop, mapping_setup, mapping),
             Role('LoopClosing', stop, closing_setup, closing), Role('Refused', stop, refused_setup, refusals)]
    for r in roles:
        r.start()
    for r in roles:
        r.join(JOIN_S)
    hung = [r.name for r in roles if r.is_alive()]
    stop.set()
    assert not hung, hung
    for r in roles:
        if r.error is not None:
            raise r.error
    print('three roles: %.2f s' % (time.perf_counter() - t0))
    for r in roles:
        assert r.done == {n: ROUNDS for n in r.done}, (r.name, r.done)
        assert r.bad == {n: 0 for n in r.bad}, (r.name, r.bad)
    for r in roles[:3]:
        assert r.last_error == b'', (r.name, r.last_error)           # no looping thread ever saw an error, its own or another's
    assert b'feature index' in roles[3].last_error                    # the refused thread's last message is its own last refusal
    db.close()
    _close(tri, kfs, frame_a, M0)


def test_resident_epoch_is_monotonic_under_concurrent_invalidation(env):
    L = env.api.load_library()
    N, READS = 2000, 5000
    start = L.orbfe_resident_epoch()
    seen = [[], []]

    def read(i):
        seen[i] = [L.orbfe_resident_epoch() for _ in range(READS)]

    def invalidate():
        for _ in range(N):
            L.orbfe_resident_invalidate()
    ths = [threading.Thread(target=read, args=(0,)), threading.Thread(target=read, args=(1,)), threading.Thread(target=invalidate)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in ths)
    for s in seen:
        a = np.array(s, np.uint64)
        assert len(a) == READS and (np.diff(a.astype(np.int64)) >= 0).all() and a[0] >= start and a[-1] <= start + N
    assert L.orbfe_resident_epoch() == start + N
