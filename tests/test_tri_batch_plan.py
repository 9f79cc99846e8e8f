"""os1_amd/csrc/tri_batch_plan.h -- the host plan of orbfe_search_for_triangulation_frames_batch -- as a stand-alone program
(tests/cpp/tri_batch_plan_test.cpp) under the address and undefined-behaviour sanitizers: records against a brute-force
intersection, image layout, output bound, every refusal with nothing left in the plan, the finish's mask step."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_header_under_the_sanitizers(tmp_path):
    out = str(tmp_path / 'tri_batch_plan')
    subprocess.check_call(['g++', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-std=c++17', '-O1', '-g', '-Wall', '-Werror',
                           '-I' + os.path.join(ROOT, 'os1_amd', 'csrc'), os.path.join(ROOT, 'tests', 'cpp', 'tri_batch_plan_test.cpp'), '-o', out])
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'tri_batch_plan_test ok' in r.stdout, r.stdout
