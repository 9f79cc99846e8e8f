"""Shared by tests/test_triangulation_finish.py, tests/test_gpu_triangulation_batch.py, tools/gen_triangulation_batch_golden.py
and tools/triangulation_search_bench.py: seeded CreateNewMapPoints-shaped jobs -- one current keyframe against several
neighbours -- for ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:652-804), the crafted scene on which the order "mask,
then orientation histogram" decides the result, the reference backend and the reader of the recorded results.

A job is a dict: 'kf1' and 'nb' (a list) of keyframes {kps, desc, has, fv}, each neighbour also carrying F12, ex, ey, sf, s2.
Two jobs of three neighbours are recorded in tests/golden/triangulation_batch_outputs.npz (inputs and the reference's results,
arrays only) for checkouts without oracle/_ref:
  'large'    side 1 has a node of 257 features and neighbour 1 a node of 257 (both beyond kBowSide = 256: the global-memory route);
             neighbour 0 shares no node with side 1;
  'edge256'  a node of exactly 256 features on side 1 and on neighbour 0 (the last size of the LDS route); neighbour 1 shares none.
Every neighbour has its own F12 (a translation along its own direction), its own epipole and its own scale table (1.2, 1.25,
1.15), so a table row read for the wrong neighbour changes the result; about half of every keyframe's keypoints are flagged.
A side-2 feature of a common node is derived from a live side-1 feature of that node: its descriptor a few bits away (0 ... 60,
the values around TH_LOW = 50 among them), its position along the neighbour's epipolar line plus a perpendicular offset on
either side of the 3.84 sigma2 gate; every fourth repeats its predecessor's descriptor (a tie: the LAST one wins); a few sit
next to the epipole."""
import os

import numpy as np

from oracle.pyoracle import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'triangulation_batch_outputs.npz')
F32 = np.float32
K_SIDE = 256          # kBowSide of os1_amd/csrc/orbfe_bow.hip
BOUNDS = (0.0, 640.0, 0.0, 480.0)
NB_FIELDS = ('kps', 'desc', 'has', 'nodes', 'offsets', 'features', 'F12', 'e', 'sf', 's2')

JOBS = {'large': dict(seed=11, kf1=[(10, 257), (20, 12), (30, 40), (40, 50), (77, 41)],
                      nb=[[(5, 100), (15, 100), (25, 100)], [(10, 30), (20, 257), (30, 40), (50, 63)], [(10, 100), (30, 60), (40, 80), (77, 80)]]),
        'edge256': dict(seed=12, kf1=[(10, 256), (30, 64), (40, 80)],
                        nb=[[(10, 256), (30, 94)], [(11, 150), (31, 150)], [(10, 200), (40, 130)]])}
SCALES = (1.2, 1.25, 1.15)
BITS = (0, 10, 30, 45, 49, 50, 51, 60)
PERP = (0.0, 1.0, 1.9, 2.1, 3.0, 5.0, 8.0)
ROTS = (10.0, 100.0, 200.0)


def reference_backend(oracle):
    """the reference's compiled ORBmatcher.cc where oracle/_ref holds it, the oracle otherwise"""
    import os1_matcher_ref_util as R
    return R.RefBackend(oracle) if R.have_lib() else oracle


def _fv(node_of):
    ids = np.unique(node_of[node_of >= 0])
    feats = [np.nonzero(node_of == i)[0] for i in ids]
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats])])
    return ids.astype(np.uint32), off.astype(np.uint32), (np.concatenate(feats) if feats else np.zeros(0)).astype(np.uint32)


def _nodes(rng, nodes):
    n = sum(c for _, c in nodes)
    node_of = np.repeat([i for i, _ in nodes], [c for _, c in nodes]).astype(np.int64)
    return n, node_of[rng.permutation(n)]


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _keyframe(rng, nodes):
    n, node_of = _nodes(rng, nodes)
    k = np.zeros(n, KP_DTYPE)
    k['x'], k['y'] = rng.uniform(20, 620, n).astype(F32), rng.uniform(20, 460, n).astype(F32)
    k['octave'], k['angle'], k['size'] = rng.integers(0, 8, n), rng.uniform(0, 360, n).astype(F32), 31.0
    return dict(kps=k, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), has=(rng.random(n) < 0.5).astype(np.uint8), fv=_fv(node_of)), node_of


def make_job(spec):
    rng = np.random.default_rng(spec['seed'])
    kf1, node1 = _keyframe(rng, spec['kf1'])
    nbs = []
    for j, nodes in enumerate(spec['nb']):
        nb, node2 = _keyframe(rng, nodes)
        th = 0.3 + 0.9 * j
        c, s = np.cos(th), np.sin(th)
        sf = np.cumprod(np.array([1.0] + [SCALES[j % 3]] * 7, F32)).astype(F32)
        near = []
        prev = None
        for i2 in range(len(node2)):
            src = np.nonzero((node1 == node2[i2]) & (kf1['has'] == 0))[0]
            if not len(src):
                continue
            if prev is not None and i2 % 4 == 3 and node1[prev[0]] == node2[i2]:
                i1, d = prev      # a tie with the feature derived before
            else:
                i1 = int(rng.choice(src))
                d = _flip(rng, kf1['desc'][i1], int(rng.choice(BITS)))
            prev = (i1, d)
            nb['desc'][i2] = d
            along, perp = rng.uniform(-30, 30), float(rng.choice(PERP)) * (1 if rng.random() < 0.5 else -1)
            nb['kps']['x'][i2] = F32(kf1['kps']['x'][i1] + along * c - perp * s)
            nb['kps']['y'][i2] = F32(kf1['kps']['y'][i1] + along * s + perp * c)
            rot = float(rng.choice(ROTS)) if rng.random() < 0.85 else float(rng.uniform(0, 360))
            nb['kps']['angle'][i2] = F32((float(kf1['kps']['angle'][i1]) - rot) % 360.0)
            if nb['has'][i2] == 0 and abs(perp) < 1.5:
                near.append(i2)
        e = nb['kps'][near[0]] if near else nb['kps'][0]
        nb.update(F12=np.array([0, 0, s, 0, 0, -c, -s, c, 0], F32), ex=float(F32(e['x'] + 3.0)), ey=float(F32(e['y'] + 4.0)), sf=sf, s2=(sf * sf).astype(F32))
        for i2 in near[1:6]:       # a few more live candidates inside / at the edge of the epipole's radius
            nb['kps']['x'][i2], nb['kps']['y'][i2] = F32(nb['ex'] + rng.uniform(-12, 12)), F32(nb['ey'] + rng.uniform(-12, 12))
        nbs.append(nb)
    return dict(kf1=kf1, nb=nbs)


def bench_job(n_nb=20, n=2000, n_nodes=100, seed=5):
    """One CreateNewMapPoints-sized job: node sizes as a real vocabulary at levelsup 4 leaves them (uneven, about n / n_nodes)."""
    rng = np.random.default_rng(seed)

    def spec():
        w = rng.dirichlet(np.full(n_nodes, 2.0))
        c = np.floor(w * n).astype(int)
        c[0] += n - c.sum()
        return [(int(i), int(k)) for i, k in enumerate(c) if k]
    return make_job(dict(seed=seed, kf1=spec(), nb=[spec() for _ in range(n_nb)]))


# ---- running a job ----------------------------------------------------------------------------------------------------------
def ref_search(be, kf1, nb, has1, ori):
    """(nmatches, [(idx1, idx2)]) of the reference / oracle for one neighbour with side 1's flags given"""
    n, p = be.search_for_triangulation(kf1['kps'], kf1['desc'], has1, kf1['fv'], nb['kps'], nb['desc'], nb['has'], nb['fv'], nb['F12'], nb['ex'],
                                       nb['ey'], nb['sf'], nb['s2'], ori)
    return int(n), [(int(a), int(b)) for a, b in p]


def raw_from_pairs(pairs, n1):
    raw = np.full(n1, -1, np.int32)
    for a, b in pairs:
        raw[a] = b
    return raw


def ref_raw_rows(be, job):
    return np.stack([raw_from_pairs(ref_search(be, job['kf1'], nb, job['kf1']['has'], False)[1], len(job['kf1']['kps'])) for nb in job['nb']])


def neighbour_arg(frame2, nb):
    return (frame2, nb['has'], nb['fv'], nb['F12'], nb['ex'], nb['ey'], nb['sf'], nb['s2'])


def triangulated(rng, pairs):
    """the idx1 of a seeded subset of the pairs: the ones CreateNewMapPoints would have given a MapPoint"""
    return [a for a, _ in pairs if rng.random() < 0.6]


def ref_sequence(be, job, ori, seed=3):
    """The loop of LocalMapping.cc:207-232 on the reference: [(nmatches, pairs)] per neighbour with the current keyframe's flags evolving."""
    rng = np.random.default_rng(seed)
    has1 = job['kf1']['has'].copy()
    out = []
    for nb in job['nb']:
        n, p = ref_search(be, job['kf1'], nb, has1, ori)
        out.append((n, p))
        has1[triangulated(rng, p)] = 1
    return out


# ---- the recorded results ---------------------------------------------------------------------------------------------------
def pack(name, job, raw, seq):
    out = {}
    for tag, kf in [('kf1', job['kf1'])] + [('nb%d' % j, nb) for j, nb in enumerate(job['nb'])]:
        v = dict(kps=kf['kps'].view(np.uint8).reshape(len(kf['kps']), -1), desc=kf['desc'], has=kf['has'], nodes=kf['fv'][0], offsets=kf['fv'][1], features=kf['fv'][2])
        if tag != 'kf1':
            v.update(F12=kf['F12'], e=np.array([kf['ex'], kf['ey']], F32), sf=kf['sf'], s2=kf['s2'])
        for k, a in v.items():
            out['%s/%s/%s' % (name, tag, k)] = a
    out['%s/raw' % name] = raw
    for ori in (0, 1):
        for j, (n, p) in enumerate(seq[ori]):
            out['%s/seq%d/%d' % (name, ori, j)] = np.array(p, np.int32).reshape(-1, 2)
    return out


_G = {}


def golden():
    """{name: (job, raw rows, {ori: [(nmatches, pairs)]})} as recorded from the reference"""
    if not _G:
        z = np.load(GOLDEN)
        for name, spec in JOBS.items():
            def kf(tag):
                g = lambda k: z['%s/%s/%s' % (name, tag, k)]
                d = dict(kps=np.ascontiguousarray(g('kps')).view(KP_DTYPE).reshape(-1), desc=g('desc'), has=g('has'), fv=(g('nodes'), g('offsets'), g('features')))
                if tag != 'kf1':
                    d.update(F12=g('F12'), ex=float(g('e')[0]), ey=float(g('e')[1]), sf=g('sf'), s2=g('s2'))
                return d
            job = dict(kf1=kf('kf1'), nb=[kf('nb%d' % j) for j in range(len(spec['nb']))])
            seq = {ori: [(len(z['%s/seq%d/%d' % (name, ori, j)]), [(int(a), int(b)) for a, b in z['%s/seq%d/%d' % (name, ori, j)]])
                         for j in range(len(spec['nb']))] for ori in (0, 1)}
            _G[name] = (job, z['%s/raw' % name], seq)
    return _G


# ---- the scene on which the order of the finish decides ----------------------------------------------------------------------
def order_scene():
    """Isolated pairs, one vocabulary node each, every gate open; rotation bins 1, 4, 7, 10 hold 10, 8, 6 and 5 of them.  Flagging
    three of bin 7's keypoints leaves it 3: the three maxima move from {1, 4, 7} to {1, 4, 10}.  Masking first keeps bins 1, 4 and
    10 (23 pairs); pruning first and masking afterwards keeps bins 1, 4 and what is left of 7 (21 pairs).
    Returns (inp of bow_boundary_util.make_inp, has_mp1_now)."""
    import bow_boundary_util as BB
    rots = [30.0] * 10 + [120.0] * 8 + [210.0] * 6 + [300.0] * 5
    nodes = [(i, [(0, 1, 10.0 + i, 100.0, 0, r)], [(0, 1, 10.0 + i, 100.0, 0, 0.0)]) for i, r in enumerate(rots)]
    inp = BB.make_inp('tri', nodes, ori=True)
    now = inp['has1'].copy()
    now[[18, 19, 20]] = 1
    return inp, now


# ---- the C++ facade (include/orbfe/TriangulationSearch.h) ---------------------------------------------------------------------
def facade_syntax_check():
    """tests/cpp/triangulation_search_syntax.cpp against the declaration-level stand-ins of OpenCV and of the reference's classes"""
    import subprocess
    cpp = os.path.join(ROOT, 'tests', 'cpp')
    r = subprocess.run(['g++', '-std=c++17', '-fsyntax-only', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(cpp, 'opencv_stub'),
                        '-I' + os.path.join(cpp, 'os1_stub'), os.path.join(cpp, 'triangulation_search_syntax.cpp')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def facade_compile(out):
    import subprocess
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'cpp', 'triangulation_search_test.cpp'), '-o', out, '-L' + os.path.join(ROOT, 'os1_amd'), '-lorbfe',
                           '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib'])
    return out


def facade_write_job(d, job):
    """the files tests/cpp/triangulation_search_test.cpp reads"""
    with open(os.path.join(d, 'meta.txt'), 'w') as f:
        f.write('%d\n' % len(job['nb']))
    for j, kf in enumerate([job['kf1']] + job['nb']):
        b = os.path.join(d, 'kf%d' % j)
        np.ascontiguousarray(kf['kps']).tofile(b + '.kps')
        np.ascontiguousarray(kf['desc'], np.uint8).tofile(b + '.desc')
        np.ascontiguousarray(kf['has'], np.uint8).tofile(b + '.has')
        nodes, off, feats = kf['fv']
        fv = []
        for i, a, e in zip(nodes, off[:-1], off[1:]):
            fv += [int(i), int(e - a)] + [int(v) for v in feats[a:e]]
        np.array(fv, np.uint32).tofile(b + '.fv')
        if j:
            assert len(kf['sf']) == 8
            np.concatenate([kf['F12'], [kf['ex'], kf['ey']], kf['sf'], kf['s2']]).astype(F32).tofile(b + '.geo')


def facade_ref_sequence(be, job, ori):
    """the loop of the test program on the reference: after neighbour i the pairs with (7 idx1 + 3 idx2 + i) % 5 < 3 get a MapPoint"""
    has1 = job['kf1']['has'].copy()
    out = []
    for i, nb in enumerate(job['nb']):
        n, p = ref_search(be, job['kf1'], nb, has1, ori)
        out.append(p)
        has1[[a for a, b in p if (7 * a + 3 * b + i) % 5 < 3]] = 1
    return out
