"""os1_amd/csrc/equidistant_tan.h on the host (tests/cpp/equidistant_tan_test.cpp) against mpmath at 60 digits: the enclosure of tan,
its width, the candidate set, and the verdict of the equidistant undistortion against the oracle."""
import mpmath as mp
import numpy as np

import equidistant_util as E
import undistort_stream_util as U


def _thetas():
    r = np.random.RandomState(11)
    nx = lambda v, d: float(np.nextafter(v, d))     # noqa: E731
    edge = [nx(E.THETA_MIN, 1), nx(nx(E.THETA_MIN, 1), 1), E.THETA_MAX, nx(E.THETA_MAX, 0), 1.0, 0.5, nx(1.0, 0), nx(1.0, 2)]
    # (the header has no argument reduction, hence no internal breakpoint: 1e-8 and THETA_MAX are the only edges)
    return np.concatenate([r.uniform(E.THETA_MIN, E.THETA_MAX, 20000), np.logspace(-7.99, -1, 600), edge])


def test_enclosure_width_and_candidates_against_mpmath():
    th = _thetas()
    th = th[(th > E.THETA_MIN) & (th <= E.THETA_MAX)]
    got = E.enclosures(th)
    assert (got[:, 0] == 1).all()
    for t, (_, hi, lo_l, hi_l, nc, c0, c1, c2) in zip(th, got):
        true = mp.tan(mp.mpf(float(t)))
        lo, up = mp.mpf(hi) + mp.mpf(lo_l), mp.mpf(hi) + mp.mpf(hi_l)
        assert lo < true < up, t                                           # contains the real value
        assert (up - lo) / 2 <= true * mp.mpf(2) ** -62, t                 # relative half-width
        want = E.candidates_of(lo, up)
        assert [c0, c1, c2][:int(nc)] == want, t                           # the candidate set of that enclosure
        assert E.floor_double(true) in want and E.ceil_double(true) in want
        assert len(want) == 2 or lo <= mp.mpf(hi) <= up                    # three only when the enclosure contains a double


def test_out_of_domain_arguments():
    nx = lambda v, d: float(np.nextafter(v, d))     # noqa: E731
    bad = [E.THETA_MIN, nx(E.THETA_MIN, 0), 0.0, -0.0, -0.5, -1e-9, nx(E.THETA_MAX, 2), 1.6, 1e300, np.inf, -np.inf, np.nan]
    assert (E.enclosures(bad)[:, 0] == 0).all()
    assert (E.enclosures([nx(E.THETA_MIN, 1), E.THETA_MAX])[:, 0] == 1).all()


def test_host_program_under_the_sanitizers():
    got = E.enclosures(_thetas()[:500], sanitize=True)
    assert got.shape == (500, 8)
    xy, und = E.verdict(np.concatenate([U.seeded_points()[:200], U.crafted_points('k4')]), E.SONY, sanitize=True)
    assert und.any() and not und[:200].any()


def test_decided_floats_equal_the_oracle(oracle):
    pts = U.seeded_points()
    xy, und = E.verdict(pts, E.SONY)
    assert not und.any()          # the condition of this test: a seed that ever hits an undecided point is changed, not excused
    assert xy.tobytes() == oracle.undistort_equidistant(pts, *E.SONY).tobytes()
    # both sides of 1e-8: the principal point itself and its float neighbours take the `: 1.0` branch or the series
    near = np.asarray([(E.SONY[2], E.SONY[3]), (np.nextafter(np.float32(E.SONY[2]), np.float32(1e9)), E.SONY[3]),
                       (E.SONY[2], np.nextafter(np.float32(E.SONY[3]), np.float32(0)))], np.float32)
    xy, und = E.verdict(near, E.SONY)
    assert not und.any() and xy.tobytes() == oracle.undistort_equidistant(near, *E.SONY).tobytes()


def test_crafted_points_out_of_domain_are_undecided_and_returned_unchanged():
    pts = U.crafted_points('k4')
    xy, und = E.verdict(pts, E.SONY)
    th = np.asarray([E.theta_of(E.SONY, u, v) for u, v in pts])
    assert (und == (th > E.THETA_MAX)).all() and und.sum() >= 2       # (1e6, -1e6) among them
    assert xy[und].tobytes() == pts[und].tobytes()


def test_golden_undecided_points(oracle):
    g = np.load(E.GOLDEN)
    cam = tuple(float(v) for v in g['camera'])
    assert cam == E.SONY
    for ax in 'xy':
        for kind in ('upper', 'lower'):
            pts = g['%s_%s' % (ax, kind)]
            assert len(pts) >= 8 and pts.dtype == np.float32
            xy, und = E.verdict(pts, cam)
            assert und.all()                                              # flagged
            final = oracle.undistort_equidistant(pts, *cam)
            enc = E.enclosures([E.theta_of(cam, u, v) for u, v in pts])
            k = 'xy'.index(ax)
            for i, (u, v) in enumerate(pts):
                undecided, kinds, _ = E.classify(cam, u, v)               # confirmed by mpmath
                assert undecided and kinds[k] == kind, (ax, kind, i)
                low = E.project(cam, u, v, enc[i, 5])                      # the lowest candidate's floats
                assert (xy[i, 0], xy[i, 1]) == low, (ax, kind, i)
                # whatever the host libm returns (any double within 1 ULP), the oracle's value is one candidate's
                nc = int(enc[i, 4])
                assert any(tuple(final[i]) == E.project(cam, u, v, c) for c in enc[i, 5:5 + nc]), (ax, kind, i)
    px = g['pixel']
    for cx, cy in g['centres']:
        c = (cam[0], cam[1], float(cx), float(cy))
        undecided, kinds, _ = E.classify(c, px[0], px[1])
        assert undecided and 'upper' in kinds
        assert E.verdict(px[None], c)[1][0]
