"""Device frames as views into a larger device image (a ROI of a decoder's output): the canvas the views live in, the guard band that
keeps every aligned-down or piece-rounded load of the front-end kernels inside the allocation, the shapes and the alignment grid of
tests/test_gpu_device_views.py, a numpy restatement of the 8-bit colour -> gray conversion and the crafted frame on which its rounding
term decides the result, and the per-frame comparison against the oracle.  Nothing here touches the GPU until a DeviceCanvas is created.

Guard band.  A load leaves an allocation along the address axis, so the band is measured there: the first byte of a view lies at least
GUARD_ROWS full canvas rows plus GUARD_BYTES after the allocation's first byte, its last byte as far in front of the allocation's last
byte, and between the last byte of one view and the first byte of the next (in address order) lies the same distance.  A view never
wraps around a canvas row.  check_guard() refuses every layout that breaks one of these; DeviceCanvas calls it before it allocates."""
import ctypes as C
import functools

import numpy as np

GUARD_ROWS = 8
GUARD_BYTES = 64

# (name, W, H, nfeatures, nlevels), scale 1.2 everywhere
#   landscape: every level wider than 64 px -> k_resize_fixed with tilesX >= 2 on every level
#   portrait : test_batch_with_a_level_one_tile_wide's 110 x 150; its top level is one tile wide -> the generic k_resize (from the slab)
#   narrow   : level 1 is already one tile wide -> the generic k_resize reads the caller's level 0 in place
SHAPES = [('landscape', 161, 131, 300, 3), ('portrait', 110, 150, 120, 4), ('narrow', 76, 104, 120, 2)]
DY = 9
DXS = (0, 1, 2, 3, 13, 16)
STRIDES = (256, 260, 258, 259)                    # a multiple of 16, of 4 only, even, odd


def grid():
    """(stride, dx) of the alignment grid: every dx on the dword-multiple strides, dx in {0, 1} on the others."""
    return [(s, dx) for s in STRIDES for dx in (DXS if s % 4 == 0 else (0, 1))]


def uncovered_before(stride, dx):
    """The family no other test reaches: a dword-multiple stride under a view that does not start on a dword."""
    return stride % 4 == 0 and dx % 4 != 0


# ---- canvas ----------------------------------------------------------------------------------------------------------------------

def check_guard(rows_c, stride_c, views):
    """views: [(dy, dx, rows, row_bytes)].  Raises ValueError unless every view keeps the guard band (module docstring)."""
    need = GUARD_ROWS * stride_c + GUARD_BYTES
    spans = []
    for dy, dx, rows, row_bytes in views:
        if dy < 0 or dx < 0 or rows < 1 or row_bytes < 1 or dx + row_bytes > stride_c or dy + rows > rows_c:
            raise ValueError('view %r does not fit a %d x %d canvas' % ((dy, dx, rows, row_bytes), rows_c, stride_c))
        spans.append((dy * stride_c + dx, (dy + rows - 1) * stride_c + dx + row_bytes - 1))
    spans.sort()
    total = rows_c * stride_c
    for first, last in spans:
        if first < need or total - 1 - last < need:
            raise ValueError('a view lies closer than %d rows + %d bytes to an end of the allocation' % (GUARD_ROWS, GUARD_BYTES))
    for (_, last), (first, _) in zip(spans, spans[1:]):
        if first - last - 1 < need:
            raise ValueError('two views lie closer than %d rows + %d bytes to each other' % (GUARD_ROWS, GUARD_BYTES))


def stacked(dxs, rows):
    """dy of k equally high views stacked under each other with the guard band between them, and the canvas height that holds them."""
    step = rows + GUARD_ROWS + 2          # two rows more than the band: GUARD_BYTES and the views' different dx fit in
    dys = [DY + i * step for i in range(len(dxs))]
    return dys, dys[-1] + rows + GUARD_ROWS + 2


def canvas_bytes(rows_c, stride_c, fill, placed):
    """placed: [(dy, dx, image[rows, row_bytes] uint8)] -> the canvas as a host array, `fill` everywhere outside the views."""
    check_guard(rows_c, stride_c, [(dy, dx) + im.shape for dy, dx, im in placed])
    buf = np.full((rows_c, stride_c), fill, np.uint8)
    for dy, dx, im in placed:
        buf[dy:dy + im.shape[0], dx:dx + im.shape[1]] = im
    return buf


class DeviceCanvas:
    """One device buffer of rows_c x stride_c bytes, filled with `fill`, with k equally sized images written into it as views at
    (dy, dx); .ptrs are their device pointers, all with the row stride .stride."""

    def __init__(self, rows_c, stride_c, fill, placed, device=0):
        from os1_amd import api
        assert len({im.shape for _, _, im in placed}) == 1 and all(im.dtype == np.uint8 and im.ndim == 2 for _, _, im in placed)
        buf = canvas_bytes(rows_c, stride_c, fill, placed)
        self.L = api.load_library()
        self.device = device
        self.stride = stride_c
        p = C.c_void_p()
        api._check(self.L.orbfe_device_malloc(device, buf.size, C.byref(p)))
        self.base = p.value
        api._check(self.L.orbfe_device_upload(device, C.c_void_p(self.base), buf.ctypes.data_as(C.c_void_p), buf.size))
        self.ptrs = [self.base + dy * stride_c + dx for dy, dx, _ in placed]

    @classmethod
    def stack(cls, stride_c, fill, dxs, images, device=0):
        dys, rows_c = stacked(dxs, images[0].shape[0])
        return cls(rows_c, stride_c, fill, list(zip(dys, dxs, images)), device)

    def free(self):
        if getattr(self, 'base', None):
            self.L.orbfe_device_free(self.device, C.c_void_p(self.base))
            self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- colour -> gray ----------------------------------------------------------------------------------------------------------------

FORMATS = [('rgb', 3, True), ('bgr', 3, False), ('rgba', 4, True), ('bgra', 4, False)]      # (name, channels, R first)
GRAY = {0: ((9798, 19235, 3735), 15), 1: ((4899, 9617, 1868), 14)}                          # variant -> ((R, G, B), shift)


def gray_coefficients(rgb_order, variant):
    (r, g, b), shift = GRAY[variant]
    return ((r, g, b) if rgb_order else (b, g, r)), shift


def gray_sums(img, rgb_order, variant):
    (s0, s1, s2), shift = gray_coefficients(rgb_order, variant)
    c = img.astype(np.int64)
    return c[..., 0] * s0 + c[..., 1] * s1 + c[..., 2] * s2, shift


def gray_restatement(img, rgb_order, variant):
    """(H, W, 3|4) uint8 -> (H, W) uint8: (c0*s0 + c1*s1 + c2*s2 + (1 << (shift-1))) >> shift in int64, alpha ignored."""
    s, shift = gray_sums(img, rgb_order, variant)
    out = (s + (1 << (shift - 1))) >> shift
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def all_residues(variant):
    """sum mod 2^shift of ALL 2^24 eight-bit triples, R-first order, as [c0][c1][c2] (the B-first order is its transpose)."""
    (s0, s1, s2), shift = gray_coefficients(True, variant)
    v = np.arange(256, dtype=np.int64)
    return ((v[:, None, None] * s0 + v[None, :, None] * s1 + v[None, None, :] * s2) & ((1 << shift) - 1)).astype(np.int32)


@functools.lru_cache(None)
def rounding_targets(variant):
    """(below, on): the step `on` = half, where the rounding term carries into the result, and the largest residue `below` it that
    eight-bit pixels reach.  below == half - 1 for the 14-bit set.  The 15-bit set cannot reach half - 1 (nor half - 2): with
    R + G + B coefficients = 2^15 the residue is 9798 (R - G) + 3735 (B - G) mod 2^15, and none of the (R - G, B - G) that give
    half - 1 fits three bytes (tests/test_device_views.py enumerates all 2^24 triples)."""
    res = all_residues(variant)
    half = 1 << (GRAY[variant][1] - 1)
    return int(res[res < half].max()), half


def rounding_residues(img, rgb_order, variant):
    """How many pixels of img sit on the last reachable residue below the rounding step / exactly on the step."""
    s, shift = gray_sums(img, rgb_order, variant)
    res = s & ((1 << shift) - 1)
    below, on = rounding_targets(variant)
    return int((res == below).sum()), int((res == on).sum())


def colour_frame(seed, W, H):
    """A textured (H, W, 4) frame: os1_amd.synth gray with per-channel jitter, random alpha."""
    from os1_amd.synth import synth
    rng = np.random.default_rng(seed)
    g = synth(seed, W, H).astype(np.int32)
    return np.stack([np.clip(g + rng.integers(-30, 31, g.shape), 0, 255), np.clip(g + rng.integers(-10, 11, g.shape), 0, 255),
                     np.clip(g + rng.integers(-40, 41, g.shape), 0, 255), rng.integers(0, 256, g.shape)], axis=-1).astype(np.uint8)


@functools.lru_cache(None)
def rounding_triples(variant):
    """Up to 40 triples (R-first order) on each of rounding_targets(variant), spread over the whole colour cube."""
    res = all_residues(variant)
    out = []
    for want in rounding_targets(variant):
        hit = np.argwhere(res == want)
        assert len(hit) >= 8
        out.append(hit[np.linspace(0, len(hit) - 1, min(40, len(hit))).astype(np.int64)])
    return np.concatenate(out).astype(np.uint8)


def rounding_frame(seed, W, H):
    """colour_frame with pixels of rows 24 .. H - 24, every other column, overwritten by triples whose weighted sum lies on the last
    reachable residue below the rounding step or exactly on it -- for both coefficient sets and both channel orders (a triple and its
    mirror image).  The alpha bytes stay random.  The textured pixels in between keep FAST corners in the frame."""
    img = colour_frame(seed, W, H)
    rng = np.random.default_rng(seed + 1)
    picks = np.concatenate([t for variant in (0, 1) for t in (rounding_triples(variant), rounding_triples(variant)[:, ::-1])])
    ys, xs = np.mgrid[24:H - 24, 0:W:2]
    at = rng.permutation(ys.size)[:len(picks)]
    assert len(at) == len(picks)
    img[ys.ravel()[at], xs.ravel()[at], :3] = picks
    return img


# ---- comparison ----------------------------------------------------------------------------------------------------------------------

def cmp_extract(got, want, what):
    """Keypoints and descriptors bit for bit (test_gpu_parity._cmp_extract with the case in the message)."""
    (gk, gd), (wk, wd) = got, want
    assert len(gk) == len(wk), (what, len(gk), len(wk))
    for f in gk.dtype.names:
        assert (gk[f] == wk[f]).all(), (what, f)
    assert gk.tobytes() == wk.tobytes(), what
    assert gd.tobytes() == wd.tobytes(), what


class Reference:
    """What the oracle computes on the contiguous host copy of a frame: keypoints, descriptors, every pyramid level, every level's
    candidate list.  Computed once per frame and shared."""

    def __init__(self, ox, img, nlevels):
        self.img = img
        self.kd = ox.extract(img)
        self.levels = [ox.level(l) for l in range(nlevels)]
        self.cands = [ox.candidates(l) for l in range(nlevels)]
        for a in self.levels:
            a.setflags(write=False)


def check_frame(ex, i, got, ref, what, candidates=False):
    """Frame i of the call `ex` has just finished against its Reference: keypoints, descriptors, every level pixel-exact, and the
    candidate lists where asked for."""
    cmp_extract(got, ref.kd, what)
    for l, want in enumerate(ref.levels):
        assert (ex.level(l, frame=i) == want).all(), (what, 'frame %d pyramid level %d' % (i, l))
    if candidates:
        for l, oc in enumerate(ref.cands):
            c = ex.candidates(l, frame=i)
            assert len(c) == len(oc), (what, 'frame %d level %d candidate count' % (i, l))
            assert (c[:, 0] == oc['x']).all() and (c[:, 1] == oc['y']).all() and (c[:, 2] == oc['response']).all(), \
                (what, 'frame %d level %d candidates' % (i, l))


def references(oracle, frames_per_shape=4):
    """{shape name: (W, H, N, nlevels, [Reference] * frames_per_shape)} on os1_amd.synth texture."""
    from oracle.pyoracle import OracleExtractor
    from os1_amd.synth import synth
    out = {}
    for k, (name, W, H, N, nl) in enumerate(SHAPES):
        ox = OracleExtractor(N, 1.2, nl, 20, 7, oracle)
        out[name] = (W, H, N, nl, [Reference(ox, synth(300 + 10 * k + i, W, H), nl) for i in range(frames_per_shape)])
    return out


def run_views(ex, refs, stride, dxs, what, candidates=False, call=None):
    """len(dxs) views of the shape's first frames, stacked in one canvas, through one extract call -- on a canvas filled with 0x00 and
    on one filled with 0xff, views at the same places.  Both against the references, and against each other byte for byte.
    call(ex, ptrs, H, W, stride) -> (kps, desc, n); default: extract_batch_ptrs."""
    W, H, N, nl, R = refs
    raw = []
    for fill in (0x00, 0xff):
        cv = DeviceCanvas.stack(stride, fill, list(dxs), [R[i].img for i in range(len(dxs))])
        if call is None:
            kps, desc, n = ex.extract_batch_ptrs(cv.ptrs, H, W, stride, True)
        else:
            kps, desc, n = call(ex, cv.ptrs, H, W, stride)
        for i in range(len(dxs)):
            check_frame(ex, i, (kps[i, :n[i]], desc[i, :n[i]]), R[i], '%s fill 0x%02x frame %d' % (what, fill, i), candidates)
        raw.append((n.tobytes(), [kps[i, :n[i]].tobytes() for i in range(len(dxs))], [desc[i, :n[i]].tobytes() for i in range(len(dxs))]))
        cv.free()
    assert raw[0] == raw[1], (what, 'the result depends on bytes outside the views')


def partner(dx):
    """A second dx of the grid whose dx % 4 differs from the first one's (two-frame calls)."""
    return {0: 1, 1: 2, 2: 3, 3: 0, 13: 16, 16: 13}[dx]


def one_frame_sweep(api, refs_by_shape, tag, candidates_at=(260, 3), shapes=None):
    """The one-frame call over the whole grid, every shape, with a fresh handle per shape (it reads the environment's switches)."""
    for name, W, H, N, nl in SHAPES:
        if shapes is not None and name not in shapes:
            continue
        ex = api.Extractor(N, 1.2, nl, 20, 7)
        for stride, dx in grid():
            run_views(ex, refs_by_shape[name], stride, [dx], '%s %s stride %d dx %d' % (tag, name, stride, dx), (stride, dx) == candidates_at)
        ex.close()


def batch_sweep(api, refs_by_shape, tag, candidates_at=(256, 1)):
    """Four frames -- more than the cone kernel takes -- with four different dx % 4, over the whole grid."""
    for name, W, H, N, nl in SHAPES:
        ex = api.Extractor(N, 1.2, nl, 20, 7)
        for stride, dx in grid():
            run_views(ex, refs_by_shape[name], stride, [dx, dx + 1, dx + 2, dx + 3], '%s %s stride %d dx %d..%d' % (tag, name, stride, dx, dx + 3),
                      (stride, dx) == candidates_at)
        ex.close()


def register_route_main():
    """Body of the child process that test_gpu_device_views starts with ORBFE_LDS_DMA=0 (read once per process): the footprints of the
    pyramid and the descriptor patches come in through registers.  One-frame calls through the cone kernel, then with
    ORBFE_CONE_MAX_FRAMES=0 through the per-level kernels, then the four-frame batch."""
    import os
    from os1_amd import api
    from oracle.pyoracle import Oracle
    assert os.environ.get('ORBFE_LDS_DMA') == '0'
    R = references(Oracle())
    one_frame_sweep(api, R, 'no-dma one-frame')
    os.environ['ORBFE_CONE_MAX_FRAMES'] = '0'
    one_frame_sweep(api, R, 'no-dma per-level one-frame')
    del os.environ['ORBFE_CONE_MAX_FRAMES']
    batch_sweep(api, R, 'no-dma batch')
    print('OK')
