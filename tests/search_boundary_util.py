"""Crafted frames that sit ON the decision boundaries of the windowed searches, with the expected result written down by hand.

Every scene carries its inputs, the expected result as a literal stated from the reference text (Frame::GetFeaturesInArea /
PosInGrid src/Frame.cc:209-274, ORBmatcher::SearchByProjection src/ORBmatcher.cc:45-132, the projected loops :357-392 /
:872-936 / :1014-1050, SearchByProjection(Frame, Frame / KeyFrame) :1292-1552, ComputeThreeMaxima :1554-1595) and a witness: a
predicate, evaluated in float32 with numpy, that shows the scene really is on the boundary its name states.  Neither the oracle
nor the library computes an expectation.

Keypoints are KP_DTYPE rows written by hand.  Descriptors have exact Hamming distances: row(n) is one seeded base row with the
first n bits of one seeded permutation flipped, so distance(row(a), row(b)) == |a - b|; row(256) is the complement.

Kinds (what run() calls):  'win'  candidate lists (GetFeaturesInArea + distances), 'mp' SearchByProjection(F, MapPoints, th),
'uv' SearchByProjection(F, LastFrame / KeyFrame) from the projection on, 'proj' the projected best-match loops, 'init'
SearchForInitialization on host arrays.  Expectations: win [[(idx, dist), ...] per query]; mp / uv (n, {keypoint: query});
proj (n, [best_idx], [best_dist]); init (n, {keypoint1: keypoint2})."""
import numpy as np

from oracle.pyoracle import KP_DTYPE

F32 = np.float32
B0 = (0.0, 640.0, 0.0, 480.0)          # invW = invH = float32(0.1): a cell is 10 x 10 pixels, column = roundf(x * 0.1f)
BC = (-320.0, 320.0, -240.0, 240.0)    # the same cells around the origin: a keypoint's x IS its dx for a query at (0, 0)

_rng = np.random.default_rng(20240607)
_BASE = _rng.integers(0, 256, 32, dtype=np.uint8)
_PERM = _rng.permutation(256)


def row(n):
    d = _BASE.copy()
    for bit in _PERM[:n]:
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def rows(ns):
    return np.stack([row(int(n)) for n in ns]) if len(ns) else np.zeros((0, 32), np.uint8)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def make_kps(pts):
    """pts: (x, y, octave[, angle])"""
    k = np.zeros(len(pts), KP_DTYPE)
    for i, p in enumerate(pts):
        k['x'][i], k['y'][i], k['octave'][i] = p[0], p[1], p[2]
        k['angle'][i] = p[3] if len(p) > 3 else 0.0
        k['size'][i] = 31.0
    return k


def cell_coord(v, lo, hi, ncell):
    """(v - lo) * inv in float32, as PosInGrid forms it before rounding (Frame.cc:98-99, 266-267)."""
    inv = F32(ncell) / F32(F32(hi) - F32(lo))
    return F32(F32(F32(v) - F32(lo)) * inv)


class Scene:
    def __init__(self, name, family, kind, inp, expect, witness, route=None):
        self.name, self.family, self.kind, self.inp, self.expect, self.witness, self.route = name, family, kind, inp, expect, witness, route

    def __repr__(self):
        return self.name


SCENES = []


def _add(*a, **k):
    s = Scene(*a, **k)
    assert s.name not in [t.name for t in SCENES], s.name
    SCENES.append(s)
    return s


# ---- running a scene --------------------------------------------------------------------------------------------------------
def _dense(n, sparse):
    a = [-1] * n
    for k, v in sparse.items():
        a[k] = v
    return a


def expected(scene):
    """The hand-stated result in the form run() returns."""
    e, i = scene.expect, scene.inp
    if scene.kind in ('mp', 'uv'):
        return (e[0], _dense(len(i['kps']), e[1]))
    if scene.kind == 'init':
        return (e[0], _dense(len(i['kps1']), e[1]))
    if scene.kind == 'proj':
        return (e[0], list(e[1]), list(e[2]))
    return [list(l) for l in e]


def run(scene, be, first=None, pinned=None):
    """be: the oracle or a Matcher.  first: a resident Frame in place of the keypoint array.  pinned: a function that
    returns a page-locked copy of a query array."""
    i = scene.inp
    pin = pinned or (lambda a: a)
    kps = i.get('kps') if first is None else first
    if scene.kind == 'mp':
        n, a = be.search_by_projection(kps, i['desc'], i['bounds'], i['sf'], pin(i['occ']), pin(i['xy']), pin(i['level']), pin(i['viewcos']),
                                       pin(i['flags']), pin(i['qdesc']), i['th'], i['ratio'])
        return (int(n), [int(v) for v in a])
    if scene.kind == 'uv':
        n, a = be.search_by_projection_uv(kps, i['desc'], i['bounds'], i['sf'], pin(i['occ']), pin(i['xy']), pin(i['level']), pin(i['angle']),
                                          pin(i['flags']), pin(i['valid']), pin(i['qdesc']), i['th'], i['maxd'], i['skip_any'], i['ori'])
        return (int(n), [int(v) for v in a])
    if scene.kind == 'proj':
        n, bi, bd = be.search_projected(kps, i['desc'], i['bounds'], pin(i['xy']), pin(i['radius']), pin(i['level']), pin(i['valid']),
                                        pin(i['qdesc']), i['skip'], i['claim'], i['is2'], i['chi2'], i['maxd'])
        return (int(n), [int(v) for v in bi], [int(v) for v in bd])
    if scene.kind == 'init':
        n, m12, prev = be.search_for_initialization(i['kps1'], i['desc1'], i['kps2'], i['desc2'], i['bounds'], i['prev'], i['window'],
                                                    i['ratio'], i['ori'])
        return (int(n), [int(v) for v in m12])
    assert scene.kind == 'win'
    if hasattr(be, 'window_candidates'):
        got = be.window_candidates(i['kps'], i['desc'], i['bounds'], i['qx'], i['qy'], i['qr'], i['qmin'], i['qmax'], i['qdesc'])
        return [[(int(a), int(b)) for a, b in zip(*l)] for l in got]
    out = []
    for q in range(len(i['qx'])):
        idx = be.get_features_in_area(i['kps'], i['bounds'], float(i['qx'][q]), float(i['qy'][q]), float(i['qr'][q]), int(i['qmin'][q]),
                                      int(i['qmax'][q]))
        out.append([(int(j), int(be.hamming(i['qdesc'][q], i['desc'][j]))) for j in idx])
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------------
def win_inp(pts, nflip, bounds, queries, qflip=None):
    """queries: (x, y, r, minL, maxL)"""
    q = np.array([[a[0], a[1], a[2]] for a in queries], np.float32).reshape(-1, 3)
    return dict(kps=make_kps(pts), desc=rows(nflip), bounds=bounds, qx=q[:, 0].copy(), qy=q[:, 1].copy(), qr=q[:, 2].copy(),
                qmin=np.array([a[3] for a in queries], np.int32), qmax=np.array([a[4] for a in queries], np.int32),
                qdesc=rows(qflip if qflip is not None else [0] * len(queries)))


def mp_inp(pts, nflip, bounds, queries, th=1.0, ratio=0.8, sf=None, occ=None, qflip=None):
    """queries: (x, y, level, viewcos, flags)"""
    n = len(queries)
    return dict(kps=make_kps(pts), desc=rows(nflip), bounds=bounds, sf=np.asarray(sf if sf is not None else [1.0] * 8, np.float32),
                occ=np.asarray(occ if occ is not None else [0] * len(pts), np.uint8),
                xy=np.array([[a[0], a[1]] for a in queries], np.float32).reshape(-1, 2), level=np.array([a[2] for a in queries], np.int32),
                viewcos=np.array([a[3] for a in queries], np.float32), flags=np.array([a[4] for a in queries], np.uint8),
                qdesc=rows(qflip if qflip is not None else [0] * n), th=th, ratio=ratio)


def uv_inp(pts, nflip, bounds, queries, th=1.0, maxd=100, skip_any=0, ori=False, sf=None, occ=None, qflip=None):
    """queries: (x, y, level, angle, flags, valid)"""
    n = len(queries)
    return dict(kps=make_kps(pts), desc=rows(nflip), bounds=bounds, sf=np.asarray(sf if sf is not None else [1.0] * 8, np.float32),
                occ=np.asarray(occ if occ is not None else [0] * len(pts), np.uint8),
                xy=np.array([[a[0], a[1]] for a in queries], np.float32).reshape(-1, 2), level=np.array([a[2] for a in queries], np.int32),
                angle=np.array([a[3] for a in queries], np.float32), flags=np.array([a[4] for a in queries], np.uint8),
                valid=np.array([a[5] for a in queries], np.uint8), qdesc=rows(qflip if qflip is not None else [0] * n), th=th, maxd=maxd,
                skip_any=skip_any, ori=ori)


def proj_inp(pts, nflip, bounds, queries, maxd=100, claim=False, skip=None, is2=None, chi2=5.99, qflip=None):
    """queries: (x, y, radius, level, valid)"""
    n = len(queries)
    return dict(kps=make_kps(pts), desc=rows(nflip), bounds=bounds, xy=np.array([[a[0], a[1]] for a in queries], np.float32).reshape(-1, 2),
                radius=np.array([a[2] for a in queries], np.float32), level=np.array([a[3] for a in queries], np.int32),
                valid=np.array([a[4] for a in queries], np.uint8), qdesc=rows(qflip if qflip is not None else [0] * n),
                skip=None if skip is None else np.asarray(skip, np.uint8), claim=claim,
                is2=None if is2 is None else np.asarray(is2, np.float32), chi2=chi2, maxd=maxd)


QX, QY = 320.0, 240.0   # column 32.0, row 24.0 of B0


def one_query(name, family, kind, cands, want, level=0, r=4.0, witness=None, ratio=0.8, maxd=100, viewcos=0.5, flags=9, b=0):
    """One query at (QX, QY) with window radius r; cands: (dx, dy, octave, nflip).  want: None or (index, distance)."""
    pts = [(QX + c[0], QY + c[1], c[2]) for c in cands]
    nf = [c[3] for c in cands]
    w = witness or (lambda: True)
    if kind == 'mp':       # plCandidato off, viewCos <= 0.998: 4.0 * mvScaleFactors[level] (ORBmatcher.cc:63-71, 126-132)
        inp = mp_inp(pts, nf, B0, [(QX, QY, level, viewcos, flags)], 1.0, ratio, sf=[r / 4.0] * 8, qflip=[b])
        exp = (1, {want[0]: 0}) if want else (0, {})
    elif kind == 'uv':     # th * mvScaleFactors[level] (:1347)
        inp = uv_inp(pts, nf, B0, [(QX, QY, level, 0.0, 8, 1)], 1.0, maxd, sf=[r] * 8, qflip=[b])
        exp = (1, {want[0]: 0}) if want else (0, {})
    else:
        inp = proj_inp(pts, nf, B0, [(QX, QY, r, level, 1)], maxd, qflip=[b])
        exp = (1, [want[0]], [want[1]]) if want else (0, [-1], [-1])
    return _add(name, family, kind, inp, exp, w)


KINDS = ('mp', 'uv', 'proj')


# ==== A. window geometry =====================================================================================================
def _family_a():
    R = F32(10.0)
    nr = np.nextafter(R, F32(0))
    # 0..7: (-R,0) (-nr,0) (R,0) (nr,0) (0,-R) (0,-nr) (0,R) (0,nr); the keypoints AT r carry the smallest distances
    pts = [(-R, 0, 0), (-nr, 0, 0), (R, 0, 0), (nr, 0, 0), (0, -R, 0), (0, -nr, 0), (0, R, 0), (0, nr, 0)]
    nf = [1, 10, 2, 41, 3, 40, 4, 42]
    k = make_kps(pts)

    def wit_edge():
        d = np.maximum(np.abs(k['x'] - F32(0)), np.abs(k['y'] - F32(0)))
        return bool((d[0::2] == R).all() and (d[1::2] == nr).all() and nr < R)
    # Frame.cc:253 `if(fabs(distx)<r && fabs(disty)<r)`: strict.  Order: columns 31 (x = -nr), 32 (rows 23: y = -nr, 25: y = nr), 33
    _add('edge_abs_dx_eq_r_is_out_win', 'A', 'win', win_inp(pts, nf, BC, [(0, 0, R, -1, -1)]), [[(1, 10), (5, 40), (7, 42), (3, 41)]], wit_edge)
    _add('edge_abs_dx_eq_r_is_out_mp', 'A', 'mp', mp_inp(pts, nf, BC, [(0, 0, 0, 0.5, 9)], 2.5, 0.8), (1, {1: 0}), wit_edge)   # 4.0 * 2.5 * 1.0
    _add('edge_abs_dx_eq_r_is_out_uv', 'A', 'uv', uv_inp(pts, nf, BC, [(0, 0, 0, 0.0, 8, 1)], 10.0), (1, {1: 0}), wit_edge)
    _add('edge_abs_dx_eq_r_is_out_proj', 'A', 'proj', proj_inp(pts, nf, BC, [(0, 0, R, 0, 1)]), (1, [1], [10]), wit_edge)
    # r == 0 and r < 0: nothing satisfies |d| < r, not even the keypoint under the query
    p0 = [(QX, QY, 0)]
    _add('radius_zero_and_negative_win', 'A', 'win', win_inp(p0, [0], B0, [(QX, QY, 0.0, -1, -1), (QX, QY, -1.0, -1, -1), (QX, QY, 0.5, -1, -1)]),
         [[], [], [(0, 0)]], lambda: True)
    _add('radius_zero_and_negative_proj', 'A', 'proj', proj_inp(p0, [0], B0, [(QX, QY, 0.0, 0, 1), (QX, QY, -1.0, 0, 1), (QX, QY, 0.5, 0, 1)]),
         (1, [-1, -1, 0], [-1, -1, 0]), lambda: True)
    _add('radius_zero_mp', 'A', 'mp', mp_inp(p0, [0], B0, [(QX, QY, 0, 0.5, 9), (QX, QY, 1, 0.5, 9)], sf=[0.0, 0.25] + [1.0] * 6),
         (1, {0: 1}), lambda: True)
    _add('radius_zero_uv', 'A', 'uv', uv_inp(p0, [0], B0, [(QX, QY, 0, 0.0, 8, 1), (QX, QY, 1, 0.0, 8, 1)], sf=[0.0, 1.0] + [1.0] * 6),
         (1, {0: 1}), lambda: True)
    # windows wholly / partly outside each side (Frame.cc:216-230: nMinCellX >= 64, nMaxCellX < 0, ... return nothing)
    pc = [(2.0, 2.0, 0), (633.0, 474.0, 0), (320.0, 2.0, 0), (2.0, 240.0, 0)]
    qs = [(-5, -5, 10), (-20, 100, 10), (-10, 5, 10), (650, 470, 20), (665, 470, 20), (630, 500, 15), (630, 490, 20), (320, -12, 10),
          (320, -5, 10), (-4, 240, 10), (700, 600, 300)]
    ex = [[0], [], [], [1], [], [], [1], [], [2], [3], [1]]

    def wit_sides():
        inv = F32(0.1)
        return bool(np.floor(F32(F32(665 - 20) * inv)) == 64 and np.ceil(F32(F32(-20 + 10) * inv)) == -1 and np.floor(F32(F32(500 - 15) * inv)) == 48
                    and np.ceil(F32(F32(-12 + 10) * inv)) == 0 and np.ceil(F32(F32(-10 + 10) * inv)) == 0)
    _add('window_outside_each_side_win', 'A', 'win', win_inp(pc, [0, 1, 2, 3], B0, [(q[0], q[1], q[2], -1, -1) for q in qs]),
         [[(j, j) for j in l] for l in ex], wit_sides)
    _add('window_outside_each_side_proj', 'A', 'proj', proj_inp(pc, [0, 1, 2, 3], B0, [(q[0], q[1], q[2], 0, 1) for q in qs]),
         (6, [l[0] if l else -1 for l in ex], [l[0] if l else -1 for l in ex]), wit_sides)
    # one call per window for mp / uv (the radius is th * sf there): partly outside left / top, right / bottom, wholly outside right
    for tag, (qx_, qy_, r_), want in [('partly_left_top', (-5.0, -5.0, 10.0), 0), ('partly_right_bottom', (650.0, 490.0, 20.0), 1),
                                      ('wholly_right', (665.0, 470.0, 20.0), None), ('wholly_above', (320.0, -20.0, 10.0), None),
                                      ('wholly_below', (630.0, 500.0, 15.0), None), ('wholly_left', (-20.0, 100.0, 10.0), None)]:
        _add('window_outside_%s_mp' % tag, 'A', 'mp', mp_inp(pc, [0, 30, 60, 90], B0, [(qx_, qy_, 0, 0.5, 9)], sf=[r_ / 4.0] * 8),
             (1, {want: 0}) if want is not None else (0, {}), wit_sides)
        _add('window_outside_%s_uv' % tag, 'A', 'uv', uv_inp(pc, [0, 30, 60, 90], B0, [(qx_, qy_, 0, 0.0, 8, 1)], th=r_),
             (1, {want: 0}) if want is not None else (0, {}), wit_sides)
    # bounds that start neither at zero nor on an integer (cell width 26.7): columns of x = 50 / 150 are 10 / 14
    bn = (-211.5, 1500.25, -80.0, 799.0)
    pn = [(150.0, 50.0, 0), (50.0, 60.0, 0), (165.0, 50.0, 0), (100.0, 115.0, 0)]

    def wit_bn():
        c = [float(cell_coord(p[0], bn[0], bn[1], 64)) for p in pn]
        return round(c[1]) == 10 and round(c[0]) == 14 and round(c[3]) == 12
    _add('bounds_off_zero_off_integer_win', 'A', 'win', win_inp(pn, [5, 6, 7, 8], bn, [(100.3, 50.7, 60.0, -1, -1)]), [[(1, 6), (0, 5)]], wit_bn)
    _add('bounds_off_zero_off_integer_proj', 'A', 'proj', proj_inp(pn, [5, 6, 7, 8], bn, [(100.3, 50.7, 60.0, 0, 1)]), (1, [0], [5]), wit_bn)
    _add('bounds_off_zero_off_integer_mp', 'A', 'mp', mp_inp(pn, [5, 60, 2, 1], bn, [(100.3, 50.7, 0, 0.5, 9)], sf=[15.0] * 8), (1, {0: 0}), wit_bn)
    _add('bounds_off_zero_off_integer_uv', 'A', 'uv', uv_inp(pn, [5, 6, 2, 1], bn, [(100.3, 50.7, 0, 0.0, 8, 1)], th=60.0), (1, {0: 0}), wit_bn)
    # (x - minX) * invW == k + 0.5 in float32: roundf goes away from zero (Frame.cc:266-267), so x = 5 lies in column 1 and
    # x = 25 in column 3 -- behind keypoints of columns 0 / 2 whatever their rows and indices.  Half-to-even would put them first.
    ph = [(5.0, 100.0, 0), (4.0, 300.0, 0), (25.0, 100.0, 0), (24.0, 300.0, 0), (100.0, 5.0, 0), (100.0, 4.0, 0)]

    def wit_half():
        return bool(cell_coord(5.0, 0, 640, 64) == F32(0.5) and cell_coord(25.0, 0, 640, 64) == F32(2.5) and cell_coord(5.0, 0, 480, 48) == F32(0.5))
    # column 0: [1]; column 1: [0]; column 2: [3]; column 3: [2]; column 10: row 0: [5], row 1: [4]
    _add('cell_half_rounds_away_from_zero_win', 'A', 'win', win_inp(ph, [0, 1, 2, 3, 4, 5], B0, [(50.0, 200.0, 400.0, -1, -1)]),
         [[(1, 1), (0, 0), (3, 3), (2, 2), (5, 5), (4, 4)]], wit_half)
    # through the searches: equal distances, so the first candidate in grid order wins -- x = 4 (column 0) before x = 5 (column 1,
    # although its row and its index are lower), x = 24 before x = 25, y = 4 (row 0) before y = 5 (row 1)
    pq = [(5.0, 100.0, 0), (4.0, 300.0, 0)], [(25.0, 100.0, 0), (24.0, 300.0, 0)], [(100.0, 5.0, 0), (100.0, 4.0, 0)]
    for tag, pts_ in zip(('x_0p5', 'x_2p5', 'y_0p5'), pq):
        _add('cell_half_rounds_away_from_zero_%s_proj' % tag, 'A', 'proj', proj_inp(pts_, [20, 20], B0, [(50.0, 200.0, 400.0, 0, 1)]), (1, [1], [20]), wit_half)
        _add('cell_half_rounds_away_from_zero_%s_uv' % tag, 'A', 'uv', uv_inp(pts_, [20, 20], B0, [(50.0, 200.0, 0, 0.0, 8, 1)], th=400.0), (1, {1: 0}), wit_half)
        # mode 0: the two lie on different levels, so the tie is accepted (ORBmatcher.cc:115) and goes to the first in grid order
        pm = [(pts_[0][0], pts_[0][1], 1), (pts_[1][0], pts_[1][1], 0)]
        _add('cell_half_rounds_away_from_zero_%s_mp' % tag, 'A', 'mp', mp_inp(pm, [20, 20], B0, [(50.0, 200.0, 1, 0.5, 9)], sf=[100.0] * 8), (1, {1: 0}), wit_half)
    # keypoints that round to px == 64, py == 48 or below 0 are in no cell (Frame.cc:270-271)
    pd = [(635.0, 470.0, 0), (634.0, 470.0, 0), (630.0, 475.0, 0), (630.0, 474.0, 0), (-5.0, 10.0, 0), (-4.0, 10.0, 0), (10.0, -5.0, 0),
          (10.0, -4.9, 0)]

    def wit_drop():
        return bool(cell_coord(635.0, 0, 640, 64) == F32(63.5) and cell_coord(634.0, 0, 640, 64) < F32(63.5)
                    and cell_coord(475.0, 0, 480, 48) == F32(47.5) and cell_coord(-5.0, 0, 640, 64) == F32(-0.5)
                    and cell_coord(-5.0, 0, 480, 48) == F32(-0.5))
    _add('keypoints_outside_the_grid_are_dropped_win', 'A', 'win',
         win_inp(pd, [10, 11, 12, 13, 14, 15, 16, 17], B0, [(630.0, 470.0, 20.0, -1, -1), (0.0, 0.0, 30.0, -1, -1)]),
         [[(1, 11), (3, 13)], [(5, 15), (7, 17)]], wit_drop)
    _add('keypoints_outside_the_grid_are_dropped_proj', 'A', 'proj',
         proj_inp(pd, [12, 11, 10, 13, 14, 15, 16, 17], B0, [(630.0, 470.0, 20.0, 0, 1), (0.0, 0.0, 30.0, 0, 1)]), (2, [1, 5], [11, 15]), wit_drop)
    _add('keypoints_outside_the_grid_are_dropped_uv', 'A', 'uv',
         uv_inp(pd, [12, 11, 10, 13, 14, 15, 16, 17], B0, [(630.0, 470.0, 0, 0.0, 8, 1), (0.0, 0.0, 0, 0.0, 8, 1)], th=20.0), (2, {1: 0, 5: 1}), wit_drop)
    # level pairs (Frame.cc:232, 245-250): bCheckLevels = minLevel > 0 || maxLevel >= 0
    pl = [(QX + i, QY, o) for i, o in enumerate([0, 1, 2, 7, 8, 9])]
    lv = [(-1, -1), (0, -1), (0, 0), (1, -1), (7, 8)]
    exl = [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0], [1, 2, 3, 4, 5], [3, 4]]
    _add('level_pairs_win', 'A', 'win', win_inp(pl, [0, 1, 2, 3, 4, 5], B0, [(QX, QY, 20.0, a, b) for a, b in lv]),
         [[(j, j) for j in l] for l in exl], lambda: True)
    # query level 0 in every raw kind: [-1, 0] (mp, proj), [-1, 1] (uv); level -1 in the projected kind: no window
    plv = [(QX, QY, 2), (QX + 1, QY, 1), (QX + 2, QY, 0)]
    _add('query_level_0_mp', 'A', 'mp', mp_inp(plv, [0, 5, 9], B0, [(QX, QY, 0, 0.5, 9)], sf=[2.0] * 8), (1, {2: 0}), lambda: True)
    _add('query_level_0_uv', 'A', 'uv', uv_inp(plv, [0, 5, 9], B0, [(QX, QY, 0, 0.0, 8, 1)], th=8.0), (1, {1: 0}), lambda: True)
    _add('query_level_0_and_minus_1_proj', 'A', 'proj', proj_inp(plv, [0, 5, 9], B0, [(QX, QY, 8.0, 0, 1), (QX, QY, 8.0, -1, 1), (QX, QY, 8.0, 0, 0)]),
         (1, [2, -1, -1], [9, -1, -1]), lambda: True)


# ==== B. column runs and lane groups =========================================================================================
def _run_pts(N, holes=False):
    """N keypoints in ONE cell (column 32, row 24), so position in the column's run == index.  Window r = 4 around (320, 240)."""
    pts = []
    for i in range(N):
        x, y, o = 318.0 + (i % 8) * 0.5, 238.0 + (i // 8) * 0.25, 0
        if holes and i in (62, 65):
            x = 324.5            # same cell, |dx| = 4.5 >= r
        if holes and i in (63, 66):
            o = 3                # off level
        pts.append((x, y, o))
    return pts


def _family_b():
    for N in (63, 64, 65, 130):
        pts = _run_pts(N)
        nf = list(range(N))                       # distance to a query row(b) is |i - b|
        k = make_kps(pts)

        def wit(k=k, N=N):
            inw = (np.abs(k['x'] - F32(QX)) < 4) & (np.abs(k['y'] - F32(QY)) < 4)
            cx, cy = np.round(cell_coord(k['x'], 0, 640, 64)), np.round(cell_coord(k['y'], 0, 480, 48))
            return bool(inw.sum() == N and (cx == 32).all() and (cy == 24).all())
        bq = [N - 1, 0, 62]
        _add('column_run_%d_win' % N, 'B', 'win', win_inp(pts, nf, B0, [(QX, QY, 4.0, 0, 0)] * 3, qflip=bq),
             [[(i, abs(i - b)) for i in range(N)] for b in bq], wit)
        _add('column_run_%d_mp' % N, 'B', 'mp', mp_inp(pts, nf, B0, [(QX, QY, 0, 0.5, 1)] * 3, qflip=bq), (3, {N - 1: 0, 0: 1, 62: 2}), wit)
        _add('column_run_%d_uv' % N, 'B', 'uv', uv_inp(pts, nf, B0, [(QX, QY, 0, 0.0, 0, 1)] * 3, th=4.0, qflip=bq), (3, {N - 1: 0, 0: 1, 62: 2}), wit)
        _add('column_run_%d_proj' % N, 'B', 'proj', proj_inp(pts, nf, B0, [(QX, QY, 4.0, 0, 1)] * 3, qflip=bq), (3, [N - 1, 0, 62], [0, 0, 0]), wit)
    # positions 62, 65 out of the window and 63, 66 off level: of 62..66 only 64 is a candidate (the mask ends at 63)
    pts, nf = _run_pts(130, True), list(range(130))
    k = make_kps(pts)

    def wit_h():
        inw = (np.abs(k['x'] - F32(QX)) < 4) & (np.abs(k['y'] - F32(QY)) < 4) & (k['octave'] == 0)
        return [i for i in range(60, 69) if inw[i]] == [60, 61, 64, 67, 68] and int(inw.sum()) == 126
    keep = [i for i in range(130) if i not in (62, 63, 65, 66)]
    bq = [63, 65, 129]
    _add('column_run_130_holes_62_to_66_win', 'B', 'win', win_inp(pts, nf, B0, [(QX, QY, 4.0, 0, 0)] * 3, qflip=bq),
         [[(i, abs(i - b)) for i in keep] for b in bq], wit_h)
    # b = 63: 64 at 1, 61 at 2 (0.8 * 2 = 1.6 >= 1: accepted).  b = 65: 64 at 1, 67 at 2.
    _add('column_run_130_holes_62_to_66_mp', 'B', 'mp', mp_inp(pts, nf, B0, [(QX, QY, 0, 0.5, 1)] * 3, qflip=bq), (3, {64: 1, 129: 2}), wit_h)
    _add('column_run_130_holes_62_to_66_proj', 'B', 'proj', proj_inp(pts, nf, B0, [(QX, QY, 4.0, 0, 1)] * 3, qflip=bq), (3, [64, 64, 129], [1, 1, 0]), wit_h)
    # lane groups: one keypoint per grid column (x = 10 c + 1), index scrambled against the column; the widest window of the call
    # decides LPQ = 8 / 16 / 32 / 64 lanes per query for ALL its queries, the narrow ones included
    col_of = [(37 * i) % 64 for i in range(64)]          # keypoint i lies in column col_of[i]
    idx_of = {c: i for i, c in enumerate(col_of)}
    pts = [(10.0 * c + 1.0, 240.0 + (c % 3), 2 if c % 2 else 0) for c in col_of]
    nf = [2 * c for c in col_of]
    # (x, r) -> columns floor((x - r) * .1) .. ceil((x + r) * .1) = span, first and last column with |dx| < r
    wide = {1: (320.0, 0.0, None), 2: (325.0, 4.0, None), 3: (320.0, 4.0, (32, 32)), 4: (325.0, 6.0, (32, 32)), 5: (320.0, 14.0, (31, 33)),
            8: (325.0, 26.0, (30, 34)), 9: (320.0, 34.0, (29, 35)), 16: (325.0, 66.0, (26, 38)), 17: (320.0, 74.0, (25, 39)),
            33: (320.0, 154.0, (17, 47)), 64: (320.0, 400.0, (0, 63))}
    lanes = {1: 8, 2: 8, 3: 8, 4: 8, 5: 8, 8: 16, 9: 16, 16: 32, 17: 32, 33: 64, 64: 64}
    for span, (x, r, rng_) in wide.items():
        def wit(x=x, r=r, span=span):
            lo, hi = np.floor(F32(F32(x - r) * F32(0.1))), np.ceil(F32(F32(x + r) * F32(0.1)))
            cols = int(min(hi, 63) - max(lo, 0) + 1)
            need = int(np.ceil(F32(2.0) * F32(r) * F32(0.1) + F32(3.0)))
            lpq = 8
            while lpq < 64 and lpq < need:
                lpq <<= 1
            return cols == span and lpq == lanes[span]
        cols = list(range(rng_[0], rng_[1] + 1)) if rng_ else []
        # narrow queries in the same call: columns 5 (x = 51) and 60 (x = 601), r = 4, and r = 0
        qs = [(x, 241.0, r, -1, -1), (52.0, 241.0, 4.0, -1, -1), (600.0, 241.0, 4.0, -1, -1), (51.0, 242.0, 0.0, -1, -1)]
        bq = [2 * 32, 0, 0, 0]
        ex = [[(idx_of[c], abs(2 * c - 64)) for c in cols], [(idx_of[5], 10)], [(idx_of[60], 120)], []]
        _add('lane_groups_widest_window_%d_columns_win' % span, 'B', 'win', win_inp(pts, nf, B0, qs, qflip=bq), ex, wit)
        # projected kind, level 0: even columns only (octave 0); column 32 is at distance 0 when it is inside
        best = idx_of[32] if 32 in cols else -1
        _add('lane_groups_widest_window_%d_columns_proj' % span, 'B', 'proj',
             proj_inp(pts, nf, B0, [(x, 241.0, r, 0, 1), (52.0, 241.0, 4.0, 2, 1), (600.0, 241.0, 4.0, 0, 1), (51.0, 242.0, 0.0, 0, 1)], maxd=256, qflip=bq),
             (2 + (best >= 0), [best, idx_of[5], idx_of[60], -1], [0 if best >= 0 else -1, 10, 120, -1]), wit)


# ==== C. list length and availability ========================================================================================
def _family_c():
    """Cluster k (k = 0..8) holds k keypoints at distances 10, 20, ... from row(0), in grid order; k + 1 identical queries
    arrive there one after the other, each taking the best keypoint still free: query j ends on candidate j, the last on none.
    Lists of 0-3 candidates live in the record, 4-6 in the wide record, 7-8 in the pool."""
    pts, nf, cl = [], [], []
    for k in range(9):
        cx, cy = 40.0 + 60.0 * (k % 5), 100.0 + 200.0 * (k // 5)
        first = len(pts)
        for j in range(k):
            pts.append((cx - 12.0 + 3.0 * j, cy + (j % 2), 0))
            nf.append(10 * (j + 1))
        cl.append((cx, cy, first, k))
    nkp = len(pts)
    assert nkp == 36

    def wit():
        k_ = make_kps(pts)
        cnt = [int(((np.abs(k_['x'] - F32(c[0])) < 14) & (np.abs(k_['y'] - F32(c[1])) < 14)).sum()) for c in cl]
        return cnt == list(range(9))
    # claim / skip_any / OBSERVED: every accepted keypoint is taken from the later queries
    q_xy, bi, bd, asg = [], [], [], {}
    for cx, cy, first, k in cl:
        for j in range(k + 1):
            if j < k:
                asg[first + j] = len(q_xy)
            bi.append(first + j if j < k else -1)
            bd.append(10 * (j + 1) if j < k else -1)
            q_xy.append((cx, cy))
    nq = len(q_xy)
    assert nq == 45
    _add('list_length_0_to_8_chain_by_claim_proj', 'C', 'proj', proj_inp(pts, nf, B0, [(x, y, 14.0, 0, 1) for x, y in q_xy], claim=True), (36, bi, bd), wit)
    _add('list_length_0_to_8_chain_by_occupancy_uv', 'C', 'uv', uv_inp(pts, nf, B0, [(x, y, 0, 0.0, 0, 1) for x, y in q_xy], th=14.0, skip_any=1),
         (36, asg), wit)
    _add('list_length_0_to_8_chain_by_observations_uv', 'C', 'uv', uv_inp(pts, nf, B0, [(x, y, 0, 0.0, 8, 1) for x, y in q_xy], th=14.0, skip_any=0),
         (36, asg), wit)
    # mode 0, nnratio 1.0 (best > 1.0 * second never holds): MapPoints with observations occupy what they take (ORBmatcher.cc:89-91)
    _add('list_length_0_to_8_chain_by_observations_mp', 'C', 'mp', mp_inp(pts, nf, B0, [(x, y, 0, 0.5, 9) for x, y in q_xy], ratio=1.0, sf=[3.5] * 8),
         (36, asg), wit)
    # MapPoints WITHOUT observations leave the keypoint free: every query of a cluster takes its first keypoint, the last one stays
    last = {first: sum(c[3] + 1 for c in cl[:i]) + k for i, (cx, cy, first, k) in enumerate(cl) if k}
    _add('list_length_0_to_8_no_observations_last_writer_mp', 'C', 'mp',
         mp_inp(pts, nf, B0, [(x, y, 0, 0.5, 1) for x, y in q_xy], ratio=1.0, sf=[3.5] * 8), (44, last), wit)
    # kp_skip takes the first keypoint of every cluster away before the search: query 0 ends on its second candidate, ...
    skip = [0] * nkp
    bi2, bd2 = [], []
    for cx, cy, first, k in cl:
        if k:
            skip[first] = 1
        for j in range(k + 1):
            ok = j + 1 < k
            bi2.append(first + j + 1 if ok else -1)
            bd2.append(10 * (j + 2) if ok else -1)
    _add('list_length_0_to_8_chain_by_kp_skip_and_claim_proj', 'C', 'proj',
         proj_inp(pts, nf, B0, [(x, y, 14.0, 0, 1) for x, y in q_xy], claim=True, skip=skip), (28, bi2, bd2), wit)
    # kp_skip without claim: every query of a cluster ends on the second candidate
    bi3 = [c[2] + 1 if c[3] >= 2 else -1 for c in cl for j in range(c[3] + 1)]
    _add('list_length_0_to_8_kp_skip_no_claim_proj', 'C', 'proj',
         proj_inp(pts, nf, B0, [(x, y, 14.0, 0, 1) for x, y in q_xy], claim=False, skip=skip), (sum(c[3] + 1 for c in cl if c[3] >= 2), bi3, [20 if v >= 0 else -1 for v in bi3]), wit)
    # initial occupancy (a MapPoint with observations already there): mode 0 skips keypoints 0 and 1 of every cluster
    occ = [0] * nkp
    asg2 = {}
    q = 0
    for cx, cy, first, k in cl:
        for j in range(min(k, 2)):
            occ[first + j] = 1
        for j in range(k + 1):
            if j + 2 < k:
                asg2[first + j + 2] = q
            q += 1
    _add('list_length_0_to_8_initial_occupancy_mp', 'C', 'mp', mp_inp(pts, nf, B0, [(x, y, 0, 0.5, 9) for x, y in q_xy], ratio=1.0, sf=[3.5] * 8, occ=occ),
         (len(asg2), asg2), wit)


# ==== D. distance thresholds =================================================================================================
def _family_d():
    for kind in KINDS:
        # one candidate: no second best, no ratio test.  Mode 0: bestDist <= TH_HIGH (ORBmatcher.cc:113)
        if kind == 'mp':
            for d, ok in [(0, 1), (100, 1), (101, 0), (255, 0), (256, 0)]:
                one_query('th_high_best_%d_%s_mp' % (d, 'in' if ok else 'out'), 'D', 'mp', [(1, 1, 0, d)], (0, d) if ok else None,
                          witness=lambda d=d: hamming(row(0), row(d)) == d)
            continue
        for maxd in (50, 64, 100):
            for d, ok in [(maxd, 1), (maxd + 1, 0)]:
                one_query('maxdist_%d_best_%d_%s_%s' % (maxd, d, 'in' if ok else 'out', kind), 'D', kind, [(1, 1, 0, d)], (0, d) if ok else None,
                          maxd=maxd, witness=lambda d=d: hamming(row(0), row(d)) == d)
        # maxd = 256.  uv: bestDist starts at 256 and `dist < bestDist` (:1356, 1371): 256 never matches.  The projected loop starts
        # from INT_MAX (:1024, 1163, 1243): the complement row matches at 256.
        one_query('maxdist_256_best_255_in_%s' % kind, 'D', kind, [(1, 1, 0, 255)], (0, 255), maxd=256)
        one_query('maxdist_256_best_256_%s_%s' % ('out' if kind == 'uv' else 'in', kind), 'D', kind, [(1, 1, 0, 256)], None if kind == 'uv' else (0, 256),
                  maxd=256, witness=lambda: hamming(row(0), row(256)) == 256)
        # ties go to the first candidate in reference order (strict `dist < bestDist`): column ascending -- the LAST index here
        one_query('tie_two_first_in_grid_order_%s' % kind, 'D', kind, [(20, 0, 0, 20), (-20, 0, 0, 20)], (1, 20), r=30.0)
        one_query('tie_three_first_in_grid_order_%s' % kind, 'D', kind, [(20, 0, 0, 20), (0, 0, 0, 20), (-20, 0, 0, 20)], (2, 20), r=30.0)
        one_query('tie_rows_then_insertion_%s' % kind, 'D', kind, [(1, 12, 0, 20), (2, -12, 0, 20), (1, -12.5, 0, 20)], (1, 20), r=30.0)
    # mode 0: a tie of best and second on one level fails the ratio test (20 > 0.8 * 20); on different levels it is not applied
    one_query('tie_best_second_same_level_rejected_mp', 'D', 'mp', [(20, 0, 1, 20), (-20, 0, 1, 20)], None, level=1, r=30.0)
    one_query('tie_best_second_other_level_accepted_mp', 'D', 'mp', [(20, 0, 1, 20), (-20, 0, 0, 20)], (1, 20), level=1, r=30.0)
    one_query('tie_three_same_level_rejected_mp', 'D', 'mp', [(20, 0, 0, 20), (0, 0, 0, 20), (-20, 0, 0, 20)], None, r=30.0)


# ==== E. ratio test ==========================================================================================================
RATIO_CASES = [(0.8, 40, 50, 1), (0.8, 41, 50, 0), (0.8, 100, 124, 0), (0.8, 100, 125, 1), (0.6, 3, 5, 1), (0.6, 4, 5, 0), (0.6, 54, 90, 1),
               (0.6, 55, 90, 0), (0.9, 9, 10, 1), (0.9, 90, 100, 1), (0.9, 91, 100, 0), (1.0, 100, 100, 1), (1.0, 100, 101, 1)]


def _family_e():
    for ratio, d1, d2, ok in RATIO_CASES:
        tag = ('%g' % ratio).replace('.', 'p')

        def wit(ratio=ratio, d1=d1, d2=d2, ok=ok):     # ORBmatcher.cc:115 `bestDist > mfNNratio * bestDist2`, a float product
            return bool(F32(d1) > F32(ratio) * F32(d2)) == (not ok)
        # the second best comes first in grid order (so of two equal distances it is the one that stays best: index 1)
        bi = 1 if d1 == d2 else 0
        one_query('ratio_%s_%d_%d_same_level' % (tag, d1, d2), 'E', 'mp', [(20, 0, 1, d1), (-20, 0, 1, d2)], (bi, d1) if ok else None, level=1, r=30.0,
                  ratio=ratio, witness=wit)
        one_query('ratio_%s_%d_%d_other_level' % (tag, d1, d2), 'E', 'mp', [(20, 0, 1, d1), (-20, 0, 0, d2)], (bi, d1), level=1, r=30.0, ratio=ratio,
                  witness=wit)


def ratio_differs_in_double(ratio, d1, d2):
    """The float test of ORBmatcher.cc:115 against the same comparison with the operands widened to double first."""
    return bool(F32(d1) > F32(ratio) * F32(d2)) != bool(float(d1) > float(F32(ratio)) * float(d2))


def ratio_product_is_exact_tie(ratio, d1, d2):
    """The exact product lies above d1 and rounds (to even) onto it in float32: accepted only because it is a float product."""
    return bool(F32(ratio) * F32(d2) == F32(d1)) and float(F32(ratio)) * d2 > d1


# ==== F. radius and gate =====================================================================================================
def chi2_cases():
    """The float SUM of the gate.  (dx, dy, octave, float verdict 'rejected') where Fuse's gate (ORBmatcher.cc:896-903),
    evaluated as the reference does -- ex, ey, e2 and e2 * mvInvLevelSigma2[octave] in float, the comparison with 5.99 in
    double -- and the same expression evaluated in double from the same float offsets fall on different sides of 5.99, two
    each way.  These splits come from summing ex*ex + ey*ey in float or in double; the product itself is pinned by
    chi2_product_cases()."""
    is2 = IS2
    out = {True: [], False: []}
    for o in range(8):
        t = 5.99 / float(is2[o])
        for dx in np.arange(0.25, 2.0, 0.25, dtype=np.float32) * F32(SF[o]):
            if float(dx) ** 2 >= t:
                continue
            dy0 = F32(np.sqrt(t - float(dx) ** 2))
            dy = dy0 + np.arange(-3000, 3000, dtype=np.float32) * np.spacing(dy0)
            dy = dy.astype(np.float32)
            e2 = dx * dx + dy * dy                                   # float32
            rej32 = (e2 * is2[o]).astype(np.float64) > 5.99
            e64 = float(dx) ** 2 + dy.astype(np.float64) ** 2
            rej64 = e64 * float(is2[o]) > 5.99
            for j in np.nonzero(rej32 != rej64)[0]:
                if len(out[bool(rej32[j])]) < 2:
                    out[bool(rej32[j])].append((float(dx), float(dy[j]), o, bool(rej32[j])))
        if len(out[True]) >= 2 and len(out[False]) >= 2:
            break
    assert len(out[True]) >= 2 and len(out[False]) >= 2, 'no float / double split of the chi-square gate found'
    return out[True] + out[False]


def level_tables(scale, nlevels):
    """mvScaleFactors and mvInvLevelSigma2 as ORBextractor builds them in float (ORBextractor.cc:430-445)."""
    sf = np.cumprod(np.array([1.0] + [scale] * (nlevels - 1), np.float32)).astype(np.float32)
    return sf, (F32(1.0) / (sf * sf)).astype(np.float32)


def chi2_product_cases():
    """The float PRODUCT of the gate.  (dx, dy, octave, is2 table) where, with e2 the SAME float, float32(e2 * is2) <= 5.99 <
    double(e2) * double(is2): the reference's float product accepts, a product widened to double would reject.  Only this
    direction exists: float32(5.99) lies below 5.99, which lies below the midpoint to the next float, so a product that rounds
    down to float32(5.99) from the band (5.99, midpoint) is the only one rounding can carry across 5.99 -- 'two each way' is
    not possible for the product.  The band is about 1e-8 wide and needs is2 != 1 (octave >= 1); the table of scale factor 1.2
    has no float e2 whose product falls into it at any octave, so the search runs over the tables of other scale factors."""
    out = []
    for scale in np.arange(84, 161, dtype=np.float32) * F32(0.0125):
        sf, is2 = level_tables(scale, 9)
        for o in range(1, 9):
            e0 = F32(5.99 / float(is2[o]))
            if e0 > F32(150.0 * 150.0):          # the keypoint must stay inside the 200-pixel window
                continue
            cand = (e0 + np.arange(-4, 5, dtype=np.float32) * np.spacing(e0)).astype(np.float32)
            hit = ((cand * is2[o]).astype(np.float64) <= 5.99) & (cand.astype(np.float64) * float(is2[o]) > 5.99)
            if not hit.any():
                continue
            want = cand[np.nonzero(hit)[0][0]]
            for dx in np.arange(1, 64, dtype=np.float32) * F32(0.03125) * sf[o]:     # offsets whose float sum of squares IS that e2
                dy0 = F32(np.sqrt(max(float(want) - float(dx) ** 2, 0.0)))
                dy = (dy0 + np.arange(-16, 17, dtype=np.float32) * np.spacing(dy0)).astype(np.float32)
                j = np.nonzero(dx * dx + dy * dy == want)[0]
                if len(j):
                    out.append((float(dx), float(dy[j[0]]), o, is2))
                    break
            if len(out) >= 3:
                break
        if len(out) >= 3:
            break
    assert len(out) >= 2, 'no float-accepts / double-rejects product of the chi-square gate found'
    return out


SF = np.cumprod(np.array([1.0] + [1.2] * 7, np.float32)).astype(np.float32)       # mvScaleFactors, scale 1.2
IS2 = (F32(1.0) / (SF * SF)).astype(np.float32)                                    # mvInvLevelSigma2


def _family_f():
    c0 = F32(0.998)
    for name, vc, r25 in [('at_float_0p998', c0, True), ('one_ulp_below', np.nextafter(c0, F32(0)), False), ('one_ulp_above', np.nextafter(c0, F32(2)), True)]:
        def wit(vc=vc, r25=r25):     # ORBmatcher.cc:128 `viewCos>0.998`: float against a double constant
            return bool(float(vc) > 0.998) == r25
        # the keypoint lies 3 pixels away: inside 4.0 * sf, outside 2.5 * sf (sf = 1)
        _add('viewcos_%s_radius_%s' % (name, '2p5' if r25 else '4p0'), 'F', 'mp', mp_inp([(QX + 3.0, QY, 0)], [7], B0, [(QX, QY, 0, vc, 9)]),
             (0, {}) if r25 else (1, {0: 0}), wit)
    _add('candidato_flag_radius_4p0', 'F', 'mp', mp_inp([(QX + 3.0, QY, 0)], [7], B0, [(QX, QY, 0, 1.0, 9 | 4)]), (1, {0: 0}), lambda: True)
    _add('viewcos_1_radius_2p5', 'F', 'mp', mp_inp([(QX + 3.0, QY, 0)], [7], B0, [(QX, QY, 0, 1.0, 9)]), (0, {}), lambda: True)
    _add('th_2_doubles_the_radius', 'F', 'mp', mp_inp([(QX + 3.0, QY, 0)], [7], B0, [(QX, QY, 0, 1.0, 9)], th=2.0), (1, {0: 0}), lambda: True)
    # th == 1.0 is not applied as a factor at all (:49, 67-68); th = nextafter(1) is: 2.5 * th * 1.2 reaches past the keypoint
    th1 = float(np.nextafter(F32(1.0), F32(2.0)))
    d3 = float(F32(2.5) * F32(1.2))                                  # 3.0 exactly in float32: the keypoint at 3.0 is out for th == 1.0
    _add('th_1_is_no_factor', 'F', 'mp', mp_inp([(QX + d3, QY, 0)], [7], B0, [(QX, QY, 0, 1.0, 9)], th=1.0, sf=[1.2] * 8), (0, {}),
         lambda: F32(2.5) * F32(1.2) == F32(3.0))
    _add('th_next_after_1_is_a_factor', 'F', 'mp', mp_inp([(QX + d3, QY, 0)], [7], B0, [(QX, QY, 0, 1.0, 9)], th=th1, sf=[1.2] * 8), (1, {0: 0}),
         lambda: F32(F32(2.5) * F32(th1)) * F32(1.2) > F32(3.0))
    # chi-square gate: one scene per case; the query at the origin, the keypoint at (-dx, -dy): u - kp.x == dx exactly
    for j, (dx, dy, o, rej) in enumerate(chi2_cases()):
        def wit_chi(dx=dx, dy=dy, o=o, rej=rej):
            k = make_kps([(-dx, -dy, o)])
            ex, ey = F32(0) - k['x'][0], F32(0) - k['y'][0]
            e2 = ex * ex + ey * ey
            return bool(float(F32(e2 * IS2[o])) > 5.99) == rej and bool((float(ex) ** 2 + float(ey) ** 2) * float(IS2[o]) > 5.99) != rej
        _add('chi2_gate_float_%s_double_%s_case_%d' % ((('rejects', 'accepts') if rej else ('accepts', 'rejects')) + (j,)), 'F', 'proj',
             proj_inp([(-dx, -dy, o)], [3], BC, [(0.0, 0.0, 40.0, o, 1)], is2=IS2, chi2=5.99), (0, [-1], [-1]) if rej else (1, [0], [3]), wit_chi)
        _add('chi2_gate_off_case_%d' % j, 'F', 'proj', proj_inp([(-dx, -dy, o)], [3], BC, [(0.0, 0.0, 40.0, o, 1)]), (1, [0], [3]), wit_chi)
    # ... and the product: a float, compared in double (:902 `e2*pKF->mvInvLevelSigma2[kpLevel]>5.99`)
    for j, (dx, dy, o, is2) in enumerate(chi2_product_cases()):
        def wit_prod(dx=dx, dy=dy, o=o, is2=is2):
            k = make_kps([(-dx, -dy, o)])
            ex, ey = F32(0) - k['x'][0], F32(0) - k['y'][0]
            e2 = F32(ex * ex + ey * ey)
            return bool(float(F32(e2 * is2[o])) <= 5.99 < float(e2) * float(is2[o])) and is2[o] != F32(1.0)
        _add('chi2_gate_float_product_accepts_double_product_rejects_case_%d' % j, 'F', 'proj',
             proj_inp([(-dx, -dy, o)], [3], BC, [(0.0, 0.0, 200.0, o, 1)], is2=is2, chi2=5.99), (1, [0], [3]), wit_prod)


# ==== G. rotation histogram ==================================================================================================
def _hist_scene(name, matches, keep, ori=True, init=False, witness=None, qflip=0):
    """matches: (query angle, keypoint angle) per isolated match; keep: indices that survive the rotation check."""
    n = len(matches)
    if not init:
        pts = [(20.0 + 40.0 * (i % 15), 20.0 + 40.0 * (i // 15), 0, m[1]) for i, m in enumerate(matches)]
        qs = [(p[0], p[1], 0, m[0], 8, 1) for p, m in zip(pts, matches)]
        asg = {i: (i if i in keep else -2) for i in range(n)} if qflip == 0 else {}         # pruned slots are reported as -2 (set to NULL, :1415)
        return _add(name, 'G', 'uv', uv_inp(pts, [0] * n, B0, qs, th=3.0, ori=ori, qflip=[qflip] * n), (len(keep), asg), witness or (lambda: True))
    bounds = (0.0, 6400.0, 0.0, 4800.0)
    pts2 = [(150.0 + 250.0 * (i % 25), 150.0 + 250.0 * (i // 25), 0, m[1]) for i, m in enumerate(matches)]
    pts1 = [(p[0], p[1], 0, m[0]) for p, m in zip(pts2, matches)]
    inp = dict(kps1=make_kps(pts1), desc1=rows([qflip] * n), kps2=make_kps(pts2), desc2=rows([0] * n), bounds=bounds,
               prev=np.array([[p[0], p[1]] for p in pts1], np.float32).reshape(-1, 2), window=100, ratio=0.9, ori=ori)
    return _add(name, 'G', 'init', inp, (len(keep), {i: i for i in keep}), witness or (lambda: True))


def rot_bin32(a1, a2):
    """ORBmatcher.cc:1386-1391 in float32: factor = 1.0f / HISTO_LENGTH, rot < 0 -> += 360, round half away from zero."""
    rot = F32(a1) - F32(a2)
    if rot < 0:
        rot = F32(rot + F32(360.0))
    v = F32(rot * (F32(1.0) / F32(30)))
    b = int(np.floor(v + F32(0.5)))
    return 0 if b == 30 else b


# counts per bin: bin b is produced by a query angle of 30 b against a keypoint angle of 0
HIST_COUNTS = [('only_30', [30], [0]), ('10_1_keeps_small', [10, 1], [0, 1]), ('11_1_drops_small', [11, 1], [0]), ('30_3_keeps_small', [30, 3], [0, 1]),
          ('31_3_drops_small', [31, 3], [0]), ('10_5_1_keeps_third', [10, 5, 1], [0, 1, 2]), ('11_5_1_drops_third', [11, 5, 1], [0, 1]),
          ('two_equal_top_bins', [7, 7], [0, 1]), ('four_equal_bins_highest_index_loses', [4, 4, 4, 4], [0, 1, 2]),
          ('5_5_5_4_drops_fourth', [5, 5, 5, 4], [0, 1, 2]), ('10_1_small_bin_first', [0, 1, 10], [1, 2]),
          ('four_equal_bins_descending_later', [0, 3, 4, 4, 4, 4], [2, 3, 4])]
# bin edges: three bins of three matches each; the probe (last match) survives only if it falls into the bin stated
ROT_PROBES = [('diff_0_bin_0', 0.0, 0.0, 0), ('diff_15_bin_1', 15.0, 0.0, 1), ('diff_45_bin_2', 45.0, 0.0, 2), ('diff_345_bin_12', 345.0, 0.0, 12),
          ('diff_359p99_bin_12', 359.99, 0.0, 12), ('negative_wraps_to_bin_11', 10.0, 40.0, 11), ('negative_small_wraps_to_bin_12', 0.0, 0.01, 12),
          ('minus_zero_bin_0', -0.0, 0.0, 0), ('diff_14p99_bin_0', 14.99, 0.0, 0)]


def _family_g():
    for tag, cnt, kept_bins in HIST_COUNTS:
        matches, keep = [], []
        for b, c in enumerate(cnt):
            for _ in range(c):
                if b in kept_bins:
                    keep.append(len(matches))
                matches.append((30.0 * b, 0.0))

        def wit(cnt=cnt, matches=matches, tag=tag):
            h = {}
            for a1, a2 in matches:
                h[rot_bin32(a1, a2)] = h.get(rot_bin32(a1, a2), 0) + 1
            lim = F32(0.1) * F32(max(cnt))
            return h == {b: c for b, c in enumerate(cnt) if c} and (tag != '30_3_keeps_small' or (lim == F32(3.0) and float(F32(0.1)) * 30 > 3.0))
        for init in (False, True):
            _hist_scene('histogram_%s_%s' % (tag, 'init' if init else 'uv'), matches, keep, True, init, wit)
        _hist_scene('histogram_%s_check_ori_off_uv' % tag, matches, list(range(len(matches))), False, False, wit)
        _hist_scene('histogram_%s_check_ori_off_init' % tag, matches, list(range(len(matches))), False, True, wit)
    five = [(0.0, 0.0), (30.0, 0.0), (60.0, 0.0), (90.0, 0.0), (120.0, 0.0)]     # complement rows: distance 256, nothing is accepted
    _hist_scene('histogram_no_match_at_all_uv', five, [], True, False, lambda: hamming(row(0), row(256)) == 256, 256)
    _hist_scene('histogram_no_match_at_all_init', five, [], True, True, lambda: hamming(row(0), row(256)) == 256, 256)
    for tag, a1, a2, want_bin in ROT_PROBES:
        others = [b for b in (4, 8, 6) if b != want_bin][:2]
        matches = []
        for b in [want_bin] + others:
            a = 350.0 if b == 12 else 30.0 * b
            matches += [(a, 0.0)] * 3
        matches.append((a1, a2))

        def wit(a1=a1, a2=a2, want_bin=want_bin):
            return rot_bin32(a1, a2) == want_bin and rot_bin32(350.0, 0.0) == 12
        for init in (False, True):
            _hist_scene('rotation_bin_%s_%s' % (tag, 'init' if init else 'uv'), matches, list(range(10)), True, init, wit)
    # ... and a probe that falls into a fourth bin is pruned: 15 degrees is bin 1, not bin 0
    matches = [(0.0, 0.0)] * 3 + [(120.0, 0.0)] * 3 + [(240.0, 0.0)] * 3 + [(15.0, 0.0)]
    for init in (False, True):
        _hist_scene('rotation_bin_diff_15_is_not_bin_0_%s' % ('init' if init else 'uv'), matches, list(range(9)), True, init, lambda: rot_bin32(15.0, 0.0) == 1)


_family_a()
_family_b()
_family_c()
_family_d()
_family_e()
_family_f()
_family_g()

BY_NAME = {s.name: s for s in SCENES}
