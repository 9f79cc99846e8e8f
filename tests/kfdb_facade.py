"""Build and run tests/cpp/kfdb_test.cpp (orb_shim.hpp's KeyFrameDatabaseT on mock KeyFrame / Frame types against
tests/cpp/kfdb_ref.cpp): shared by tests/test_kfdb.py (it compiles and links; the header compiles against the reference's names)
and tests/test_gpu_kfdb.py (it runs the scenes and matches the restatement)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')


def compile_test(out):
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(CPP, 'kfdb_test.cpp'), os.path.join(CPP, 'kfdb_ref.cpp'), '-o', out, os.path.join(ROOT, 'os1_amd', 'liborbfe.so'),
           '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def syntax_check(out):
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), '-I' + os.path.join(ROOT, 'include', 'orbfe'),
                           '-I' + os.path.join(CPP, 'kfdb_stub'), '-c', os.path.join(CPP, 'kfdb_header_check.cpp'), '-o', out])


def run(exe, scene_files):
    r = subprocess.run([exe] + list(scene_files), capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith('PASS'), r.stdout[-3000:] + r.stderr[-2000:]
    stats = lines[-2].split()
    return dict(zip(stats[0::2], (int(v) for v in stats[1::2])))
