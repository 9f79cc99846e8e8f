"""Build and run tests/cpp/source_projection_test.cpp (orb_shim.hpp's SearchByProjectionLastFrame / SearchByProjectionKeyFrame
over a short tracking-shaped sequence): shared by tests/test_source_projection.py (it compiles and links) and
tests/test_gpu_source_projection.py (it runs and matches the CPU oracle)."""
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
           '-I' + os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests', 'cpp', 'source_projection_test.cpp'), '-o', out,
           os.path.join(ROOT, 'os1_amd', 'liborbfe.so'), os.path.join(ROOT, 'oracle', 'liborb_oracle.so'),
           '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath,' + os.path.join(ROOT, 'oracle'),
           '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run(exe, tmp_path, W=640, H=480, NF=5, N=1000, dx=-3, dy=1):
    from os1_amd.synth import shifted, synth
    base = synth(71, W, H)
    for k in range(NF):
        shifted(base, k * dx, k * dy, 700 + k).tofile(os.path.join(str(tmp_path), 'f%03d.gray' % k))
    open(os.path.join(str(tmp_path), 'meta.txt'), 'w').write('%d %d %d %d %d %d\n' % (W, H, NF, N, dx, dy))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith('PASS'), r.stdout[-3000:] + r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-3].split()
    return dict(zip(line[0::2], (int(v) for v in line[1::2])))
