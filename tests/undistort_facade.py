"""Build and check tests/cpp/undistort_facade_test.cpp (orb_shim.hpp's Extractor::SetCamera over a Tracking-shaped sequence): shared by
tests/test_undistort_facade.py (it compiles and links) and tests/test_gpu_undistort_facade.py (it runs, sends no coordinates and matches
the oracle composition)."""
import os
import subprocess

import numpy as np

import undistort_stream_util as U
from oracle.pyoracle import KP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = 'k5'


def compile_test(out):
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    cmd = ['g++', '-std=c++17', '-O2', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(ROOT, 'tests', 'cpp', 'undistort_facade_test.cpp'), '-o', out, '-L' + os.path.join(ROOT, 'os1_amd'),
           '-lorbfe', '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run_and_check(exe, tmp_path, oracle):
    d = str(tmp_path)
    fx, fy, cx, cy, dist = U.CAMERAS[CAM]
    frames = U.frames()
    open(os.path.join(d, 'meta.txt'), 'w').write('%d %d %d %d %r %r %r %r %d %s\n' % (
        U.W, U.H, len(frames), U.NFEAT, fx, fy, cx, cy, len(dist), ' '.join(repr(v) for v in dist)))
    for k, f in enumerate(frames):
        f.tofile(os.path.join(d, 'f%d.gray' % k))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'uploads 0 ' in r.stdout and 'coordinate_bytes 0' in r.stdout, r.stdout
    want = U.expected(oracle, CAM)
    for k in range(len(frames)):
        wk, wd = U.extracted(oracle)[k]
        pre = os.path.join(d, 'f%d' % k)
        assert np.fromfile(pre + '.kp', KP_DTYPE).tobytes() == wk.tobytes()
        assert np.fromfile(pre + '.desc', np.uint8).tobytes() == wd.tobytes()
        assert np.fromfile(pre + '.un', np.float32).tobytes() == want['xy_un'][k].tobytes()
        if k:
            wn, wm = want['pairs'][k - 1]
            assert int(np.fromfile(os.path.join(d, 'p%d.nm' % k), np.int32)[0]) == wn
            assert (np.fromfile(os.path.join(d, 'p%d.m12' % k), np.int32) == wm).all()
