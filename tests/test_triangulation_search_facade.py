"""CPU: include/orbfe/TriangulationSearch.h type-checks with cv::Mat and ORB_SLAM2::KeyFrame of the declaration-level stand-ins
(tests/cpp/triangulation_search_syntax.cpp), and its GPU test program compiles and links against the C ABI.  The program runs in
tests/test_gpu_triangulation_batch.py."""
import os

import triangulation_batch_util as T


def test_facade_type_checks_against_the_stub_headers():
    T.facade_syntax_check()


def test_facade_test_program_compiles_and_links(tmp_path):
    assert os.path.exists(T.facade_compile(str(tmp_path / 'triangulation_search_test')))
