"""Build and check tests/cpp/local_map_test.cpp (orb_shim.hpp's SearchLocalPoints over a short tracking-shaped sequence):
shared by tests/test_local_map.py (it compiles and links) and tests/test_gpu_local_map.py (it runs and matches the reference
restatement and the CPU oracle)."""
import os
import subprocess

import numpy as np

import local_map_util as U
from os1_amd.synth import shifted, synth

ROOT = U.ROOT


def compile_test(out):
    from os1_amd import api
    if not os.path.exists(api.lib_path()):
        api.build_library()
    cmd = ['g++', '-std=c++17', '-O2', '-Wall', '-Werror', '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'),
           os.path.join(ROOT, 'tests', 'cpp', 'local_map_test.cpp'), '-o', out, '-L' + os.path.join(ROOT, 'os1_amd'),
           '-lorbfe', '-Wl,-rpath,' + os.path.join(ROOT, 'os1_amd'), '-Wl,-rpath-link,/opt/rocm/lib']
    subprocess.check_call(cmd)
    return out


def run_and_check(api, exe, tmp_path, ref, oracle, W=1920, H=1080, NMP=3000, NF=5):
    A = synth(61, W, H)
    B = shifted(A, 3, -2, 62)
    ex = api.Extractor(2000, 1.2, 8, 20, 7)
    kA, dA = ex(A)
    kB, dB = ex(B)
    sf = ex.tables()['sf']
    ex.close()
    camA = U.camera(W, H)
    mp = U.triangulate(kA, dA, sf, NMP, camA, seed=63, max_octave=5)   # (the sequence widens some depth ranges)
    rec = np.zeros((NMP, 16), np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7] = mp['pos'], mp['normal'], mp['min'], mp['max']
    rec.view(np.uint8).reshape(NMP, 64)[:, 32:] = mp['desc']
    cams = [U.moved_camera(W, H, 3, -2, 8.0, seed=70 + k) for k in range(NF)]
    d = str(tmp_path)
    open(os.path.join(d, 'meta.txt'), 'w').write('%d %d %d %d %d\n' % (W, H, len(kB), NMP, NF))
    np.ascontiguousarray(kB).tofile(os.path.join(d, 'kps.bin'))
    np.ascontiguousarray(dB).tofile(os.path.join(d, 'desc.bin'))
    sf.astype(np.float32).tofile(os.path.join(d, 'sf.bin'))
    rec.tofile(os.path.join(d, 'mp.bin'))
    np.stack([U.cam_array(c) for c in cams]).astype(np.float32).tofile(os.path.join(d, 'cam.bin'))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    bounds = (0.0, float(W), 0.0, float(H))
    total = 0
    for fi in range(NF):
        pre = os.path.join(d, 'f%d' % fi)
        nm, th, n = np.fromfile(pre + '.nm', np.float32)
        n = int(n)
        rc = np.fromfile(pre + '.rec', np.float32).reshape(n, 16)
        snap = dict(pos=np.ascontiguousarray(rc[:, 0:3]), normal=np.ascontiguousarray(rc[:, 3:6]), min=np.ascontiguousarray(rc[:, 6]),
                    max=np.ascontiguousarray(rc[:, 7]), desc=np.ascontiguousarray(rc.view(np.uint8).reshape(n, 64)[:, 32:]))
        flags = np.fromfile(pre + '.flags', np.uint8)
        occ = np.fromfile(pre + '.occ', np.uint8)
        out = np.fromfile(pre + '.out', np.float32).reshape(n, 6)
        want = U.ref_project(ref, snap, np.arange(n, dtype=np.int32), flags, cams[fi], bounds)
        projected = (flags & (2 | 16)) == 0
        inv = want['in_view'] == 1
        assert (out[:, 0] == want['in_view']).all()
        assert (out[:, 5] == want['in_view']).all()                    # IncreaseVisible once per MapPoint in view
        assert out[inv, 1].tobytes() == want['proj_xy'][inv, 0].tobytes()
        assert out[inv, 2].tobytes() == want['proj_xy'][inv, 1].tobytes()
        assert (out[inv, 3] == want['level'][inv]).all()
        assert out[inv, 4].tobytes() == want['view_cos'][inv].tobytes()
        assert (out[~inv, 1] == -1).all() and (out[~inv, 3] == -99).all()   # isInFrustum leaves them alone
        assert projected.sum() > n // 2 and inv.sum() > n // 3
        on, oa = oracle.search_by_projection(kB, dB, bounds, sf, occ, want['proj_xy'], want['level'], want['view_cos'],
                                             U.oracle_flags(want, flags), snap['desc'], float(th), 0.8)
        assigned = np.fromfile(pre + '.assigned', np.int32)
        assert int(nm) == on
        assert (assigned == oa).all()
        total += on
    assert total > 100
