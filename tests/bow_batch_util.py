"""Shared by tests/test_bow_batch.py and tests/test_gpu_bow_batch.py: builds the two stand-alone programs of the map-load bulk calls
(tests/cpp/bow_batch_plan_test.cpp, tests/cpp/bow_batch_shim_test.cpp) and runs them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, 'tests', 'cpp')


def compile_plan_test(out, sanitize=True):
    """the host-side bookkeeping (os1_amd/csrc/bow_batch_plan.h) as a program of its own; with the address and undefined-behaviour
    sanitizers linked into that program"""
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'os1_amd', 'csrc'),
           os.path.join(CPP, 'bow_batch_plan_test.cpp'), '-o', out]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    subprocess.check_call(cmd)
    return out


def compile_shim_test(out, host_backend):
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(CPP, 'bow_batch_shim_test.cpp'), '-o', out]
    if host_backend:
        cmd.insert(1, '-DBOWB_HOST_BACKEND')
    else:
        from os1_amd import api
        if not os.path.exists(api.lib_path()):
            api.build_library()
        cmd += [os.path.join(ROOT, 'os1_amd', 'liborbfe.so'), '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run(exe, args=(), timeout=120):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == 'PASS', r.stdout[-3000:] + r.stderr[-3000:]
