"""Build and check tests/cpp/equidistant_facade_test.cpp (orb_shim.hpp's Extractor::SetEquidistantCamera over a Tracking-shaped
sequence): shared by tests/test_equidistant_facade.py (it compiles and links) and tests/test_gpu_equidistant_facade.py (it runs, sends no
coordinates, agrees with the host UndistortKeyPoints and matches the oracle composition)."""
import os
import subprocess

import numpy as np

import equidistant_util as E
import undistort_stream_util as U
from oracle.pyoracle import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_test(out):
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    cmd = ['g++', '-std=c++17', '-O2', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(ROOT, 'tests', 'cpp', 'equidistant_facade_test.cpp'), '-o', out, '-L' + os.path.join(ROOT, 'os1_amd'),
           '-lorbfe', '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run_and_check(exe, tmp_path, oracle):
    d = str(tmp_path)
    cam = E.SONY
    frames = U.frames()
    open(os.path.join(d, 'meta.txt'), 'w').write('%d %d %d %d %r %r %r %r\n' % ((U.W, U.H, len(frames), U.NFEAT) + cam))
    for k, f in enumerate(frames):
        f.tofile(os.path.join(d, 'f%d.gray' % k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'uploads 0 ' in r.stdout and 'coordinate_bytes 0' in r.stdout, r.stdout
    ex = U.extracted(oracle)
    bounds = oracle.image_bounds(U.W, U.H, 1, *cam)
    un, xy = [], []
    for kps, _ in ex:
        p = oracle.undistort_equidistant(np.stack([kps['x'], kps['y']], 1).astype(np.float32), *cam)
        u = kps.copy()
        u['x'], u['y'] = p[:, 0], p[:, 1]
        un.append(u)
        xy.append(p)
    for k in range(len(frames)):
        wk, wd = ex[k]
        pre = os.path.join(d, 'f%d' % k)
        assert np.fromfile(pre + '.kp', KP_DTYPE).tobytes() == wk.tobytes()
        assert np.fromfile(pre + '.desc', np.uint8).tobytes() == wd.tobytes()
        assert np.fromfile(pre + '.un', np.float32).tobytes() == xy[k].tobytes()
        if k:
            wn, wm, _ = oracle.search_for_initialization(un[k - 1], ex[k - 1][1], un[k], wd, bounds, xy[k - 1], 100, 0.9, True)
            assert int(np.fromfile(os.path.join(d, 'p%d.nm' % k), np.int32)[0]) == wn
            assert (np.fromfile(os.path.join(d, 'p%d.m12' % k), np.int32) == wm).all()
