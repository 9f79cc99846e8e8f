"""Build and run tests/cpp/keyframe_projection_test.cpp (orb_shim.hpp's SearchByProjectionScw / FuseKeyFrame / FuseScw /
SearchBySim3Device on facade_pose_test's mock model): shared by tests/test_keyframe_projection.py (it compiles and links) and
tests/test_gpu_keyframe_projection.py (it runs and matches the CPU oracle)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_test(out):
    from os1_amd import api
    from oracle import pyoracle
    if not os.path.exists(api.lib_path()):
        api.build_library()
    pyoracle.build()
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
           '-I' + os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests', 'cpp', 'keyframe_projection_test.cpp'), '-o', out,
           os.path.join(ROOT, 'os1_amd', 'liborbfe.so'), os.path.join(ROOT, 'oracle', 'liborb_oracle.so'),
           '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath,' + os.path.join(ROOT, 'oracle'),
           '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith('PASS'), r.stdout[-3000:] + r.stderr[-2000:]
    stats = lines[-2].split()
    return dict(zip(stats[0::2], (int(v) for v in stats[1::2])))
