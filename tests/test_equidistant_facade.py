"""CPU: tests/cpp/equidistant_facade_test.cpp (Extractor::SetEquidistantCamera, extractUndistorted, MatcherContext::resident) compiles
against include/orbfe/orb_shim.hpp with -Wall -Werror and links against the library."""
import equidistant_facade as F


def test_equidistant_facade_compiles_and_links(tmp_path):
    F.compile_test(str(tmp_path / 'equidistant_facade_test'))
