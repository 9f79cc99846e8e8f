"""Shared by tests/test_shared_handles.py (CPU) and tests/test_gpu_shared_handles.py (-m gpu): the scenes the shared-handle tests run
and, for every call they make, the value it must return -- computed here, on the CPU, from the oracle or from the restatement the
call's own test file already pins it to.  Nothing here generates a scene of its own: every input comes from the builders of
triangulation_batch_util, local_map_util, map_point_refresh_util, keyframe_culling_util, covisibility_util, kfdb_util,
init_score_util, source_projection_util and keyframe_projection_util (the util of orbfe_search_projected_keyframe_frame, built on
source_projection_util), each at the smallest scene it offers.

world(tmpdir) -> World, built once per process:
  kA dA kB dB sf bounds   the 640 x 480 / 500-feature pair of source_projection_util.frames, on the oracle extractor's keypoints
  sbp        SearchByProjection(F, MapPoints): local_map_util's MapPoints projected by its restatement, searched by the oracle
  local      the same through the fused call (orbfe_search_local_points_frame): projection + search
  sources    source_projection_util's KEYFRAME case (th 10, ORBdist 100): restatement + orc_sbp_keyframe
  kfproj     keyframe_projection_util's Fuse case (th 3): restatement + orc_search_projected (replayed against orc_fuse there)
  projected  the array-form search of that case (orbfe_search_projected_frame) on the restatement's projection
  uv         SearchByProjection(CurrentFrame, LastFrame) with the sources' descriptors = frame A's rows (the device-rows consumer)
  tri        the recorded 'edge256' triangulation job and its raw rows (the oracle reproduces them: the CPU test says so)
  refresh    map_point_refresh_util.make_scene with both bits: table, best_obs, normal, min, max of its restatement
  init       init_score_util's general scene, 300 matches in keypoint form, the 'k3' set: its restatement's result
  culling    keyframe_culling_util.crafted_case(3) and random_map cut to 8 keyframes of 130 entries: restatement (+ hand figures)
  covis      covisibility_util.special_case and random_case(63 keyframes, 2 subjects): np_counts
  kfdb       kfdb_util.main_scene after its first block of adds: the restatement's lKFsSharingWords for the two relocalisation
             frames and for the loop keyframe's own vector
  bow        three descriptor sets (63, 0, 65 features), and the triangulation job's four keyframes' descriptors, through the oracle's
             vocabulary descent at levelsup 4"""
import numpy as np

import covisibility_util as CV
import init_score_util as IS
import keyframe_culling_util as KC
import keyframe_projection_util as KP
import kfdb_util as KD
import local_map_util as LM
import map_point_refresh_util as MR
import source_projection_util as SP
import triangulation_batch_util as TB

W_IMG, H_IMG, NFEAT = 640, 480, 500
BOTH = MR.DESCRIPTOR | MR.NORMAL_DEPTH
KEY0 = 1000                      # key of keyframe i of the database scene
BOW_LEVELSUP = 4
CULL_KF, CULL_ENTRIES = 8, 130   # the random culling map, cut down
WAVE = 64


class World:
    pass


_WORLD = None


def inv_sigma2(sf):
    sf = np.asarray(sf, np.float32)
    return (1.0 / (sf * sf)).astype(np.float32)


def flat_bow(res):
    ids, vals, (fvn, fvo, fvf), wof, nof = res
    return [np.asarray(a).tobytes() for a in (ids, vals, fvn, fvo, fvf, wof, nof)]


def kfdb_first_adds(scene):
    """the add steps in front of the scene's first query"""
    out = []
    for st in scene['steps']:
        if st[0] != 'add':
            break
        out.append(st[1])
    return out


def kfdb_queries(scene):
    """(name, words, values): both relocalisation frames' vectors and the loop keyframe's own"""
    (qw, qv), _, (q2w, q2v) = scene['probes']
    loop = scene['kfs'][scene['named']['loop']]
    return [('reloc', qw, qv), ('reloc2', q2w, q2v), ('loop', loop['words'], loop['values'])]


def world(tmpdir):
    global _WORLD
    if _WORLD is not None:
        return _WORLD
    from oracle.pyoracle import Oracle
    from os1_amd.synth import synth_vocabulary
    from test_bow_oracle import _descs
    w = World()
    o = Oracle()
    SP.bind_oracle(o)
    KP.bind_oracle(o)
    w.oracle = o
    kA, dA, kB, dB, sf = SP.frames(W_IMG, H_IMG, NFEAT)
    w.kA, w.dA, w.kB, w.dB, w.sf = kA, dA, kB, dB, sf
    w.bounds = (0.0, float(W_IMG), 0.0, float(H_IMG))

    # ---- SearchByProjection(F, MapPoints) on frame B and its fused form -------------------------------------------------------
    lm_ref = LM.build_ref(tmpdir)
    camA = LM.camera(W_IMG, H_IMG)
    n_mp = 600
    mp = LM.triangulate(kA, dA, sf, n_mp, camA, seed=31)
    cam = LM.moved_camera(W_IMG, H_IMG, 3, -2, 8.0, seed=32)
    rng = np.random.default_rng(33)
    rows = np.concatenate([rng.permutation(n_mp), rng.integers(0, n_mp, n_mp // 20)]).astype(np.int32)
    flags = LM.flags_for(len(rows), seed=34)
    occ = (rng.random(len(kB)) < 0.1).astype(np.uint8)
    proj = LM.ref_project(lm_ref, mp, rows, flags, cam, w.bounds)
    th = 5.0
    mflags = LM.oracle_flags(proj, flags)
    n, a = o.search_by_projection(kB, dB, w.bounds, sf, occ, proj['proj_xy'], proj['level'], proj['view_cos'], mflags, mp['desc'][rows], th, 0.8)
    w.local = dict(mp=mp, cam=cam, rows=rows, flags=flags, occ=occ, th=th, proj=proj, nmatches=int(n), kp_assigned=a.copy())
    w.sbp = dict(occ=occ, xy=proj['proj_xy'], level=proj['level'], viewcos=proj['view_cos'], flags=mflags, desc=np.ascontiguousarray(mp['desc'][rows]),
                 th=th, nnratio=0.8, nmatches=int(n), kp_assigned=a.copy())

    # ---- SearchByProjection(CurrentFrame, pKF, ...) fused ----------------------------------------------------------------------
    sp_ref = SP.build_ref(tmpdir)
    mode = SP.KEYFRAME
    sth, smax = SP.CASES[mode][0]
    sc = SP.scene(kA, dA, kB, sf, W_IMG, H_IMG, seed=SP.case_seed(mode, sth, W_IMG))
    want = SP.checked_oracle_case(sp_ref, o, sc, mode, kA, kB, dB, sf, sth, smax, True, W_IMG, dict(pruned=0))
    w.sources = dict(sc=sc, mode=mode, th=sth, max_dist=smax, want=want)

    # ---- Fuse(pKF, vpMapPoints, th): fused, and the array form on the restatement's projection ----------------------------------
    kp_ref = KP.build_ref(tmpdir)
    fn = KP.FUSE
    kth = KP.CASES[fn][0]
    ksc = KP.scene(kA, dA, kB, dB, sf, W_IMG, H_IMG, seed=KP.case_seed(fn, kth, W_IMG))
    c = KP.checked_oracle_case(kp_ref, o, fn, ksc, kth, kA, dA, kB, dB, sf, W_IMG, {})
    d, kproj, kbest = c['case']['dirs'][0], c['projs'][0], c['best'][0]
    assert d['to'] == 'B'
    w.kfproj = dict(sc=ksc, th=kth, d=d, proj=kproj, best=kbest)
    nm, bi, bd = KP.cpu_search(o, d, kproj, ksc, kB, dB, sf)
    assert (bi == kbest).all()
    w.projected = dict(uv=kproj['uv'], radius=kproj['radius'], level=kproj['level'], valid=kproj['valid'],
                       sdesc=np.ascontiguousarray(ksc['tab']['desc'][np.where(kproj['valid'] == 1, d['rows'], 0)]), kp_skip=d['kp_skip'],
                       claim=d['claim'], inv_sigma2=inv_sigma2(sf) if d['chi2'] else None, max_dist=d['max_dist'], nmatches=int(nm),
                       best_idx=bi.copy(), best_dist=bd.copy())

    # ---- frame A's descriptor rows as the query rows of a search on frame B ------------------------------------------------------
    uv = np.stack([kA['x'] + np.float32(3), kA['y'] - np.float32(2)], 1).astype(np.float32)      # B = A shifted by (3, -2)
    sflags = np.full(len(kA), 8, np.uint8)
    valid = np.ones(len(kA), np.uint8)
    occ0 = np.zeros(len(kB), np.uint8)
    n, a = o.search_by_projection_uv(kB, dB, w.bounds, sf, occ0, uv, kA['octave'], kA['angle'], sflags, valid, dA, 7.0, 100, 0, True)
    w.uv = dict(occ=occ0, uv=uv, level=np.ascontiguousarray(kA['octave'], np.int32), angle=np.ascontiguousarray(kA['angle'], np.float32), flags=sflags,
                valid=valid, th=7.0, max_dist=100, nmatches=int(n), kp_assigned=a.copy())

    # ---- SearchForTriangulation, all neighbours in one call ----------------------------------------------------------------------
    job, raw, _ = TB.golden()['edge256']
    w.tri = dict(job=job, raw=np.ascontiguousarray(raw, np.int32))

    # ---- MapPoint refresh ---------------------------------------------------------------------------------------------------------
    mr_ref = MR.build_ref(tmpdir)
    kfs, table, batch = MR.make_scene()
    t, best, nrm, mn, mx, rc = MR.ref_refresh(mr_ref, table, BOTH, kfs, batch)
    assert rc == 0
    w.refresh = dict(kfs=kfs, table=table, batch=batch, Ow=np.stack([k.Ow for k in kfs]).astype(np.float32), rows_after=t, best=best, normal=nrm,
                     min=mn, max=mx)

    # ---- Initializer scoring on two resident frames ------------------------------------------------------------------------------
    is_ref = IS.build_ref(tmpdir)
    s, sets = IS.scenes(is_ref)[1]
    pts = s['pts'][:300]
    k1, k2, m12 = IS.keypoint_form(pts, 3)
    H21, H12, F21 = sets['k3']
    w.init = dict(k1=k1, k2=k2, m12=m12, H21=H21, H12=H12, F21=F21, n=len(pts), want=IS.ref_find(is_ref, pts, IS.SIGMA, H21, H12, F21))

    # ---- KeyFrameCulling and UpdateConnections --------------------------------------------------------------------------------------
    kc_ref = KC.build_ref(tmpdir)
    crafted, names, hand = KC.crafted_case(3)
    cut = KC.random_map(n_kf=CULL_KF, entries=CULL_ENTRIES, th_obs=3)
    w.culling = dict(crafted=crafted, crafted_names=names, crafted_hand=hand, crafted_want=KC.ref_counts(kc_ref, crafted), cut=cut,
                     cut_want=KC.ref_counts(kc_ref, cut))
    special, snames = CV.special_case()
    small = CV.random_case(165, 63, 2, must=(0, 62))
    w.covis = dict(special=special, special_want=CV.np_counts(special), small=small, small_want=CV.np_counts(small))

    # ---- the keyframe database ------------------------------------------------------------------------------------------------------
    kd_ref = KD.build_ref(tmpdir)
    scene = KD.scenes()['main']
    ref = KD.Ref(kd_ref, scene)
    adds = kfdb_first_adds(scene)
    for k in adds:
        ref.step(('add', k))
    w.kfdb = dict(scene=scene, adds=adds, want={name: ref.sharing(qw, qv) for name, qw, qv in kfdb_queries(scene)})
    ref.close()

    # ---- batched ComputeBoW ---------------------------------------------------------------------------------------------------------
    image = synth_vocabulary(3, 10, 4)
    ov = o.vocabulary(image)
    sets = [_descs(63, image, 63), np.zeros((0, 32), np.uint8), _descs(65, image, 65)]
    w.bow = dict(image=image, sets=sets, want=[flat_bow(ov.transform(dset, BOW_LEVELSUP)) for dset in sets],
                 # the triangulation job's four keyframes: their resident rows are the sets of the shared-keyframe batch
                 kf_want=[flat_bow(ov.transform(kf['desc'], BOW_LEVELSUP)) for kf in [job['kf1']] + job['nb']])
    _WORLD = w
    return w
