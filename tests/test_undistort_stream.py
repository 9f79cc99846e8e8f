"""CPU: the scenes of test_gpu_undistort_stream.py satisfy the conditions without which the GPU tests would show nothing, and the
host undistortion, the oracle and a plain-double restatement agree on every point list the GPU sweep uses."""
import numpy as np
import pytest

import undistort_stream_util as U
from os1_amd import api


@pytest.fixture(scope='module')
def lib():
    api.build_library()
    return api.load_library()


@pytest.mark.parametrize('cam', list(U.CAMERAS))
def test_host_oracle_and_model_agree(oracle, lib, cam):
    fx, fy, cx, cy, dist = U.CAMERAS[cam]
    for pts in (U.crafted_points(cam), U.seeded_points(), np.zeros((0, 2), np.float32)):
        want = oracle.undistort_pinhole(pts, fx, fy, cx, cy, dist) if len(pts) else pts
        got = api.undistort_pinhole(pts, fx, fy, cx, cy, dist) if len(pts) else pts
        assert got.tobytes() == want.tobytes()
        assert U.model(pts, fx, fy, cx, cy, dist)[0].tobytes() == want.tobytes()


def test_crafted_list_reaches_the_fall_back_branch():
    pts = U.crafted_points('barrel')
    _, fell = U.model(pts, *U.CAMERAS['barrel'][:4], U.CAMERAS['barrel'][4])
    assert fell.any() and not fell.all()
    fx, fy, cx, cy, _ = U.CAMERAS['barrel']
    assert (pts == np.float32([cx, cy])).all(1).any()                      # the principal point
    assert ((pts[:, 0] > 4 * U.W) | (pts[:, 1] < -4 * U.H)).any()          # far outside the image


def test_identity_camera_has_other_coefficients():
    d = U.CAMERAS['identity'][4]
    assert d[0] == 0.0 and d[1] != 0.0 and d[2] != 0.0 and U.is_identity('identity')
    assert [len(U.CAMERAS[c][4]) for c in ('k4', 'k5', 'k8')] == [4, 5, 8]


def test_frames_yield_keypoints_on_every_level(oracle):
    for k, d in U.extracted(oracle):
        assert len(k) > 500 and set(np.unique(k['octave'])) == set(range(U.NLEVELS))


@pytest.mark.parametrize('cam', ['k5', 'barrel'])
def test_matches_differ_from_raw_keypoints(oracle, cam):
    un, raw = U.expected(oracle, cam), U.expected(oracle, None)
    assert any(a[0] != b[0] or (a[1] != b[1]).any() for a, b in zip(un['pairs'], raw['pairs']))
    assert all(n > 50 for n, _ in un['pairs'])      # and there is something to match


def test_barrel_moves_a_level0_keypoint_out_of_the_bounds(oracle):
    e = U.expected(oracle, 'barrel')
    outside = 0
    for (k, _), xy in zip(U.extracted(oracle), e['xy_un']):
        l0 = k['octave'] == 0
        _, _, inside = U.cell_of(xy[l0], e['bounds'])
        outside += int((~inside).sum())
    assert outside > 0


@pytest.mark.parametrize('cam', U.DISTORTING)
def test_a_keypoint_changes_grid_cell(oracle, cam):
    e, raw = U.expected(oracle, cam), U.expected(oracle, None)
    changed = 0
    for (k, _), xy, rxy in zip(U.extracted(oracle), e['xy_un'], raw['xy_un']):
        l0 = k['octave'] == 0
        px, py, _ = U.cell_of(xy[l0], e['bounds'])
        qx, qy, _ = U.cell_of(rxy[l0], raw['bounds'])
        changed += int(((px != qx) | (py != qy)).sum())
    assert changed > 0


def test_strip_takes_more_than_four_roots(oracle):
    assert U.STRIP_W / U.STRIP_H > 4.5
    e = U.expected(oracle, 'k5', 'strip')
    assert e['pairs'][0][0] > 20
