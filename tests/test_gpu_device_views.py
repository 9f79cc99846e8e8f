"""-m gpu: level 0 read IN PLACE from device views at every byte alignment -- a ROI of a larger device image, which is what a GPU decode
pipeline hands over -- against the CPU oracle on the contiguous host copy of each view.  Bit for bit, no tolerance anywhere.

Every front-end kernel derives a byte alignment from the address of the caller's frame; before this file a dword-multiple stride under
a view that does not start on a dword never reached the GPU (api.DeviceFrames only makes base + i * rows * stride; the random sweep gets
odd addresses only with odd strides, i.e. the byte routes; the odd-address case of the registered-buffer test is a host frame that is
copied to an aligned buffer first).  The grid (device_view_util.grid()): canvas stride 256 / 260 (dword multiples: all of dx = 0, 1, 2,
3, 13, 16) and 258 / 259 (dx = 0, 1), dy = 9, on three shapes; the views lie inside a guard band (device_view_util, module docstring),
so none of the aligned-down or piece-rounded loads can leave the allocation whatever a kernel does.

Which case would notice a lost alignment term (all on strides 256 / 260 with dx % 4 != 0, where the term is not zero):
  k_fast_tasks `a`     LEAN prologue: every route below (its gate is stride % 4 only); generic prologue: strides 258 / 259 (byte loop,
                       `a` shifts the tile) -- candidates are compared where a case asks for them, keypoints everywhere
  k_pyramid_cone padA  one- and two-frame calls (one_frame_views, two_frame_views): level 1 and up, pixel-exact
  k_resize_fixed `a`   LDS-DMA: four-frame batch and ORBFE_CONE_MAX_FRAMES=0 (landscape, portrait: level 1 <- level 0, tilesX >= 2);
                       dword loads through registers: the ORBFE_LDS_DMA=0 child; byte loop: strides 258 / 259
  k_resize `a`         shape 'narrow' (level 1 is one tile wide, so the generic kernel reads the view itself) in the four-frame batch,
                       with ORBFE_CONE_MAX_FRAMES=0, and in the child
  k_describe `pa`      LDS-DMA patches: every route; register patches: the child, and patches that hold the view's last row everywhere
                       (the level-0 last-row guard: keypoints with y + 21 == rows - 1)
  mixed alignments     two-frame calls (inline level-0 pointers) and four-frame batches / submit / stream push (pointer table) whose
                       frames differ in dx % 4: a term taken from frame 0 for all frames shifts the others
  k_to_gray            `aligned` is one flag per call: offsets 0 / 4 / 16 on a dword (16-byte) multiple stride with widths 161 - 163
                       take the aligned path WITH a row tail, 164 without; offset 1, stride + 1 and the mixed two-frame calls take the
                       byte path for every frame of the call
Every case runs on a canvas filled with 0x00 and on one filled with 0xff: a byte from outside a view that reaches a result fails even
where the arithmetic is right.

The cases are functions that the two tests at the end of the file call in turn, with the case named in every assertion message: the
suite's list of GPU test ids is long, and the whole file takes about four seconds on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import device_view_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def api():
    from os1_amd import api as a
    assert a.device_count() >= 1, 'no GPU visible: the product has no CPU fallback'
    return a


@pytest.fixture(scope='module')
def refs(oracle):
    R = U.references(oracle)
    lw = [r.shape[1] for r in R['landscape'][4][0].levels]
    assert min(lw) > 64, lw                                    # k_resize_fixed with tilesX >= 2 on every level
    lh, lw = R['portrait'][4][0].levels[-1].shape
    assert lw <= 64 < lh, (lw, lh)                             # one tile column, several tile rows: the generic k_resize
    lh, lw = R['narrow'][4][0].levels[1].shape
    assert lw <= 64 < lh, (lw, lh)                             # ... already on level 1, which reads the view
    for name in R:
        assert all(len(r.kd[0]) > 0 for r in R[name][4]) and len(R[name][4][0].kd[0]) > 20, name
    for name in ('landscape', 'portrait'):
        # frame 0 has level-0 keypoints whose 43-row patch holds the view's last row: k_describe's last-row guard is on the way
        k = R[name][4][0].kd[0]
        assert ((k['octave'] == 0) & (k['y'] + 21 == R[name][1] - 1)).any(), name
    return R


def one_frame_views(api, refs):
    """extract_batch_ptrs([p], ...): k_pyramid_cone, level-0 pointer in the kernel arguments."""
    U.one_frame_sweep(api, refs, 'one-frame')


def two_frame_views(api, refs):
    """Two frames whose dx % 4 differ: both inline level-0 pointers, each frame its own alignment."""
    for name, W, H, N, nl in U.SHAPES:
        ex = api.Extractor(N, 1.2, nl, 20, 7)
        for stride, dx in U.grid():
            dxs = [dx, U.partner(dx)]
            assert dxs[0] % 4 != dxs[1] % 4
            U.run_views(ex, refs[name], stride, dxs, 'two-frame %s stride %d dx %r' % (name, stride, dxs), (stride, dx) == (256, 13))
        ex.close()


def batch_views(api, refs):
    """Four frames, more than the cone kernel takes: the per-level resize launches and the pointer table, four different dx % 4."""
    U.batch_sweep(api, refs, 'batch')


def per_level_kernels_on_one_frame_views(api, refs, monkeypatch):
    """ORBFE_CONE_MAX_FRAMES=0 (read when a handle is created): the one-frame call through the per-level kernels."""
    with monkeypatch.context() as m:
        m.setenv('ORBFE_CONE_MAX_FRAMES', '0')
        U.one_frame_sweep(api, refs, 'per-level one-frame')


def register_route_on_views():
    """ORBFE_LDS_DMA=0 is read once per process: a child runs device_view_util.register_route_main()."""
    tests = os.path.dirname(os.path.abspath(__file__))
    script = 'import sys; sys.path[:0] = [%r, %r]; import device_view_util as U; U.register_route_main()' % (os.path.dirname(tests), tests)
    e = dict(os.environ)
    e['ORBFE_LDS_DMA'] = '0'
    r = subprocess.run([sys.executable, '-c', script], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith('OK'), (r.stdout[-500:], r.stderr[-1500:])


def submit_collect_and_stream_push_on_views(api, refs):
    """submit_ptrs / collect once (three views, three alignments), push_ptrs once: one stream runner, two batches of two views with
    dx % 4 = 1 and 3."""
    name, W, H, N, nl = U.SHAPES[0]

    def submit_collect(ex, ptrs, H, W, stride):
        ex.submit_ptrs(ptrs, H, W, stride, True)
        ex.wait()
        return ex.collect()
    ex = api.Extractor(N, 1.2, nl, 20, 7)
    U.run_views(ex, refs[name], 260, [1, 2, 3], 'submit/collect stride 260 dx 1, 2, 3', True, submit_collect)
    ex.close()
    R = refs[name][4]
    st = api.Stream(N, 1.2, nl, 20, 7, 0, 2, 2)
    st.set_matching((0.0, float(W), 0.0, float(H)), 100, 0.9, True)
    raw = []
    for fill in (0x00, 0xff):
        cv = U.DeviceCanvas.stack(256, fill, [1, 3, 13, 3], [r.img for r in R])
        for b in range(2):
            st.push_ptrs(cv.ptrs[2 * b:2 * b + 2], H, W, cv.stride, True)
        for b in range(2):
            kps, desc, n, _, _ = st.pop(copy=True)
            for i in range(2):
                U.cmp_extract((kps[i, :n[i]], desc[i, :n[i]]), R[2 * b + i].kd, 'stream push fill 0x%02x batch %d frame %d' % (fill, b, i))
                raw.append((fill, kps[i, :n[i]].tobytes(), desc[i, :n[i]].tobytes()))
        cv.free()
    assert [r[1:] for r in raw if r[0] == 0x00] == [r[1:] for r in raw if r[0] == 0xff]
    st.close()


def _colour_views(api, oracle, ch):
    """k_to_gray<ch> on device views: level 0 == the numpy restatement (== oracle.cvt_gray, checked first), keypoints and descriptors ==
    the oracle's on that gray image.  Frame 0 is the crafted frame on which the rounding term decides; a two-frame call adds a plain one."""
    from oracle.pyoracle import OracleExtractor
    H, N, nl = 131, 300, 3
    ex = api.Extractor(N, 1.2, nl, 20, 7)
    ox = OracleExtractor(N, 1.2, nl, 20, 7, oracle)
    unit = 4 if ch == 3 else 16
    for W in (161, 162, 163, 164):
        full = [U.rounding_frame(50 + W, W, H), U.colour_frame(40 + W, W, H)]
        for variant in (0, 1):
            # pixels with sum & mask == half (the rounding term carries) and on the last residue below it that eight-bit pixels reach:
            # half - 1 with the 14-bit set; half - 4 with the 15-bit set, which cannot reach half - 1 (tests/test_device_views.py)
            assert U.rounding_targets(variant) == (((1 << 14) - 4, 1 << 14), ((1 << 13) - 1, 1 << 13))[variant]
            for rgb in (True, False):
                below, on = U.rounding_residues(full[0], rgb, variant)
                assert below >= 1 and on >= 1, (W, variant, rgb, below, on)
        for fmt, fch, rgb in U.FORMATS:
            if fch != ch:
                continue
            imgs = [np.ascontiguousarray(f[..., :ch]) for f in full]
            for variant in (0, 1):
                grays = [U.gray_restatement(im, rgb, variant) for im in imgs]
                for im, g in zip(imgs, grays):
                    assert (oracle.cvt_gray(im, rgb, variant) == g).all(), (fmt, variant, W)
                want = [ox.extract(g) for g in grays]
                ex.set_input_format(fmt, variant)
                rows = [im.reshape(H, W * ch) for im in imgs]
                tail = (W * ch + 16 + unit - 1) // unit * unit + unit          # a dword (16-byte) multiple that holds offset 16 + a row, and more
                for stride in (tail, tail + 1):
                    assert stride > W * ch and (stride % unit == 0) == (stride == tail)
                    for offs in ([0], [4], [16], [1], [0, 16], [4, 16], [16, 1]):
                        what = '%s variant %d width %d stride %d offsets %r' % (fmt, variant, W, stride, offs)
                        raw = []
                        for fill in (0x00, 0xff):
                            cv = U.DeviceCanvas.stack(stride, fill, offs, rows[:len(offs)])
                            kps, desc, n = ex.extract_batch_ptrs(cv.ptrs, H, W, stride, True)
                            for i in range(len(offs)):
                                assert (ex.level(0, frame=i) == grays[i]).all(), (what, fill, 'gray of frame %d' % i)
                                U.cmp_extract((kps[i, :n[i]], desc[i, :n[i]]), want[i], '%s fill 0x%02x frame %d' % (what, fill, i))
                            raw.append((n.tobytes(), kps[:, :n.max()].tobytes(), desc[:, :n.max()].tobytes()))
                            cv.free()
                        assert raw[0] == raw[1], (what, 'the result depends on bytes outside the views')
    ex.close()


def test_grey_views_on_every_route(api, refs, monkeypatch):
    one_frame_views(api, refs)
    two_frame_views(api, refs)
    batch_views(api, refs)
    per_level_kernels_on_one_frame_views(api, refs, monkeypatch)
    submit_collect_and_stream_push_on_views(api, refs)
    register_route_on_views()


def test_colour_views(api, oracle):
    _colour_views(api, oracle, 3)
    _colour_views(api, oracle, 4)
