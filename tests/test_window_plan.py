"""os1_amd/csrc/window_plan.h -- lanes per query and blocks of the window kernel's one launch (orbfe_window.hip), from the widest
window of a call -- as a stand-alone program (tests/cpp/window_plan_test.cpp), built plainly and under the address and
undefined-behaviour sanitizers: the four lane classes at their edges, widths that are negative, infinite or not a number, query
counts around a block, and the two spellings of the rule it replaces swept against it."""
import covisibility_util as U


def test_plan_header(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'window_plan'), sanitize=False, src='window_plan_test.cpp'))


def test_plan_header_under_the_sanitizers(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'window_plan_san'), sanitize=True, src='window_plan_test.cpp'))
