"""os1_amd/csrc/extract_plan.h -- the slot layout of the extractor's result arena and the choice between the GPU and the host
quadtree -- as a stand-alone program (tests/cpp/extract_plan_test.cpp), built plainly and under the address and
undefined-behaviour sanitizers: the layout against the create-time formula it replaces, the hand-over at 4 / 5 roots and at
2 044 / 2 045 features on a level, the slots of wide strips, the layout against the keypoint bounds of the C ABI."""
import covisibility_util as U


def test_plan_header(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'extract_plan'), sanitize=False, src='extract_plan_test.cpp'))


def test_plan_header_under_the_sanitizers(tmp_path):
    U.run(U.compile_plan_test(str(tmp_path / 'extract_plan_san'), sanitize=True, src='extract_plan_test.cpp'))
