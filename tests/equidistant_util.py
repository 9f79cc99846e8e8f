"""The host build of os1_amd/csrc/equidistant_tan.h (tests/cpp/equidistant_tan_test.cpp) and its mpmath counterpart, shared by
test_equidistant_tan.py, test_gpu_equidistant.py and tools/find_equidistant_undecided.py."""
import atexit
import os
import shutil
import subprocess
import tempfile

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'equidistant_tan_test.cpp')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'equidistant_undecided.npz')
THETA_MAX, THETA_MIN = 1.5, 1e-8
# Sony AS-20 720p fisheye calibration, unscaled, on the 640 x 480 frames of undistort_stream_util
SONY = (732.0, 732.0, 613.0, 385.0)

mp.mp.dps = 60
_EXE = {}


def program(fast=False, sanitize=False):
    """Path of the compiled host program (fast: -O2 -mfma for the scans of the tool; fma is exact either way)."""
    key = (fast, sanitize)
    if key not in _EXE:
        d = tempfile.mkdtemp(prefix='equidistant_')
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, 'equidistant_tan_test')
        flags = ['-O2', '-mfma'] if fast else ['-O1']
        if sanitize:
            flags += ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
        subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-ffp-contract=off', '-pthread'] + flags +
                              ['-I' + os.path.join(ROOT, 'os1_amd', 'csrc'), '-o', exe, SRC])
        _EXE[key] = exe
    return _EXE[key]


def _run(args, data, dtype, sanitize=False):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, 'in'), os.path.join(d, 'out')
        np.ascontiguousarray(data).tofile(a)
        subprocess.check_call([program(sanitize=sanitize)] + args + [a, b])
        return np.fromfile(b, dtype)


def enclosures(thetas, sanitize=False):
    """-> (n, 8) float64: ok, hi, lo_l, hi_l, ncand, cand0, cand1, cand2."""
    return _run(['enc'], np.asarray(thetas, np.float64), np.float64, sanitize).reshape(-1, 8)


def verdict(xy, cam, sanitize=False):
    """-> ((n, 2) float32, undecided flags)."""
    out = _run(['verdict'] + [repr(float(np.float32(v))) for v in cam], np.asarray(xy, np.float32), np.float32, sanitize).reshape(-1, 3)
    return np.ascontiguousarray(out[:, :2]), out[:, 2] != 0


def floor_double(v):
    """Largest double <= the mpf v (v > 0)."""
    d = float(v)     # round to nearest
    return d if mp.mpf(d) <= v else float(np.nextafter(d, -np.inf))


def ceil_double(v):
    d = float(v)
    return d if mp.mpf(d) >= v else float(np.nextafter(d, np.inf))


def candidates_of(lo, hi):
    """Every double within (strictly) 1 ULP of some non-double value of the mpf interval [lo, hi], or adjacent to a double in it."""
    a, b = floor_double(lo), ceil_double(hi)
    if mp.mpf(a) == lo:                      # the interval starts ON a double: the libm may land below it
        a = float(np.nextafter(a, -np.inf))
    if mp.mpf(b) == hi:
        b = float(np.nextafter(b, np.inf))
    out = [a]
    while out[-1] < b:
        out.append(float(np.nextafter(out[-1], np.inf)))
    return out


def project(cam, u, v, T):
    """Frame.cc:366-383 from tan(theta_d) = T on, in Python doubles (IEEE, no contraction) -> two float32."""
    fx, fy, cx, cy = (float(np.float32(c)) for c in cam)
    pw0, pw1 = (float(np.float32(u)) - cx) / fx, (float(np.float32(v)) - cy) / fy
    th = float(np.sqrt(np.float64(pw0 * pw0 + pw1 * pw1)))
    scale = T / th
    pu0, pu1 = pw0 * scale, pw1 * scale
    pr0 = fx * pu0 + 0.0 * pu1 + cx * 1.0
    pr1 = 0.0 * pu0 + fy * pu1 + cy * 1.0
    pr2 = 0.0 * pu0 + 0.0 * pu1 + 1.0 * 1.0
    return np.float32(pr0 / pr2), np.float32(pr1 / pr2)


def theta_of(cam, u, v):
    fx, fy, cx, cy = (float(np.float32(c)) for c in cam)
    pw0, pw1 = (float(np.float32(u)) - cx) / fx, (float(np.float32(v)) - cy) / fy
    return float(np.sqrt(np.float64(pw0 * pw0 + pw1 * pw1)))


def classify(cam, u, v):
    """mpmath's view of one point with theta in the domain -> (undecided, [x: 'upper' / 'lower' / None, y: ...], lowest floats).
    undecided: the two doubles around the real tan give different floats.  'upper': the correctly rounded tan gives another float than
    the lower double does, on that axis."""
    th = theta_of(cam, u, v)
    t = mp.tan(mp.mpf(th))
    a, b = floor_double(t), ceil_double(t)
    rn = a if t - mp.mpf(a) < mp.mpf(b) - t else b
    fa, fb, fr = project(cam, u, v, a), project(cam, u, v, b), project(cam, u, v, rn)
    kinds = [None if fa[k] == fb[k] else ('upper' if fr[k] != fa[k] else 'lower') for k in range(2)]
    return kinds != [None, None], kinds, fa
