"""CPU: tests/cpp/undistort_facade_test.cpp (Extractor::SetCamera, extractUndistorted, MatcherContext::residentCoordBytes) compiles
against include/orbfe/orb_shim.hpp with -Wall -Werror and links against the library."""
import undistort_facade as F


def test_undistort_facade_compiles_and_links(tmp_path):
    F.compile_test(str(tmp_path / 'undistort_facade_test'))
