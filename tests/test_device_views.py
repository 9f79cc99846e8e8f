"""CPU side of tests/test_gpu_device_views.py: the utility imports without a GPU, its colour -> gray restatement is the oracle's
conversion, the crafted frame holds the pixels on which the rounding term decides, the alignment grid holds the family the GPU suite did
not reach, and the guard band refuses a view near an end of the allocation or near another view."""
import numpy as np
import pytest

import device_view_util as U


def test_gray_restatement_is_the_oracles_conversion(oracle):
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (37, 53, 4), dtype=np.uint8), U.colour_frame(7, 97, 66), U.rounding_frame(8, 163, 131)]
    extremes = np.array([[[0, 0, 0, 9], [255, 255, 255, 0], [255, 0, 0, 1], [0, 255, 0, 2], [0, 0, 255, 3]]], np.uint8)
    frames.append(extremes)
    for full in frames:
        for fmt, ch, rgb in U.FORMATS:
            img = np.ascontiguousarray(full[..., :ch])
            for variant in (0, 1):
                assert (U.gray_restatement(img, rgb, variant) == oracle.cvt_gray(img, rgb, variant)).all(), (fmt, variant, full.shape)
    # variant 0 is the 15-bit set, variant 1 the 14-bit one; the channel order swaps the outer coefficients
    assert U.gray_coefficients(True, 0) == ((9798, 19235, 3735), 15) and U.gray_coefficients(False, 1) == ((1868, 9617, 4899), 14)
    assert (U.gray_restatement(extremes, True, 0) == [[0, 255, 76, 150, 29]]).all()


def test_rounding_frame_holds_both_sides_of_the_step():
    for W in (161, 162, 163, 164):
        img = U.rounding_frame(50 + W, W, 131)
        plain = U.colour_frame(50 + W, W, 131)
        assert (img[..., 3] == plain[..., 3]).all()                     # alpha stays random
        assert len(np.unique(img[..., 3])) == 256
        for variant in (0, 1):
            for rgb in (True, False):
                below, on = U.rounding_residues(img, rgb, variant)
                assert below >= 8 and on >= 8, (W, variant, rgb, below, on)
    # the step itself: the last residue below it rounds down, on it the rounding term carries
    for variant in (0, 1):
        s, shift = U.gray_sums(img, True, variant)
        res = s & ((1 << shift) - 1)
        below, on = U.rounding_targets(variant)
        g = U.gray_restatement(img, True, variant)
        assert (g[res == below] == (s >> shift)[res == below]).all() and (g[res == on] == (s >> shift)[res == on] + 1).all()


def test_which_residues_eight_bit_pixels_reach():
    """sum & mask == half - 1 and == half for each coefficient set: the 14-bit set reaches both.  No eight-bit triple brings the
    15-bit set to half - 1 -- all 2^24 are enumerated here -- so its crafted pixels sit on half - 4, the last residue below the step
    that exists, and on half."""
    res = U.all_residues(1)
    assert (res == (1 << 13) - 1).any() and (res == 1 << 13).any() and U.rounding_targets(1) == ((1 << 13) - 1, 1 << 13)
    res = U.all_residues(0)
    half = 1 << 14
    assert res.shape == (256, 256, 256) and (res == half).any()
    assert not ((res >= half - 3) & (res < half)).any() and (res == half - 4).any()
    assert U.rounding_targets(0) == (half - 4, half)
    for variant in (0, 1):                                  # the B-first order is the mirror image: same residues
        t = U.rounding_triples(variant)
        a, _ = U.gray_sums(t, True, variant)
        b, _ = U.gray_sums(t[:, ::-1], False, variant)
        assert (a == b).all()


def test_grid_holds_the_family_nothing_else_reaches():
    g = U.grid()
    assert len(g) == len(set(g)) == 2 * 6 + 2 * 2
    assert {c for c in g if U.uncovered_before(*c)} == {(s, dx) for s in (256, 260) for dx in (1, 2, 3, 13)}
    assert {s % 16 == 0 for s, _ in g} == {True, False} and {s % 4 for s, _ in g} == {0, 2, 3}
    for dx in U.DXS:
        assert U.partner(dx) in U.DXS and U.partner(dx) % 4 != dx % 4


def test_guard_band():
    s = 256
    ok = [(9, 0, 131, 161)]
    U.check_guard(9 + 131 + 10, s, ok)
    with pytest.raises(ValueError):
        U.check_guard(9 + 131 + 10, s, [(0, 0, 131, 161)])              # flush with the start
    with pytest.raises(ValueError):
        U.check_guard(9 + 131 + 10, s, [(8, 63, 131, 161)])             # eight rows but not 64 bytes more
    U.check_guard(9 + 131 + 10, s, [(8, 64, 131, 161)])
    with pytest.raises(ValueError):
        U.check_guard(9 + 131 + 7, s, ok)                               # too close to the end
    with pytest.raises(ValueError):
        U.check_guard(400, s, [(9, 100, 131, 161)])                     # wraps around a canvas row
    with pytest.raises(ValueError):
        U.check_guard(400, s, ok + [(9 + 131 + 7, 0, 131, 161)])        # two views closer than the band
    U.check_guard(400, s, ok + [(9 + 131 + 10, 3, 131, 161)])
    # every layout the GPU tests use: the stacked views of the grid, grey and colour
    for name, W, H, N, nl in U.SHAPES:
        for stride, dx in U.grid():
            for dxs in ([dx], [dx, U.partner(dx)], [dx, dx + 1, dx + 2, dx + 3]):
                dys, rows_c = U.stacked(dxs, H)
                U.check_guard(rows_c, stride, [(dy, x, H, W) for dy, x in zip(dys, dxs)])
    img = np.arange(20 * 30, dtype=np.uint8).reshape(20, 30)
    dys, rows_c = U.stacked([1, 3], 20)
    buf = U.canvas_bytes(rows_c, 100, 0xff, list(zip(dys, [1, 3], [img, img[::-1]])))
    assert (buf[dys[0]:dys[0] + 20, 1:31] == img).all() and (buf[dys[1]:dys[1] + 20, 3:33] == img[::-1]).all()
    assert (buf == 0xff).sum() >= buf.size - 2 * img.size
