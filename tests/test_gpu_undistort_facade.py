"""-m gpu: the Tracking-shaped sequence of tests/cpp/undistort_facade_test.cpp with a distorting camera: residentUploads() == 0, zero
bytes of coordinates sent, mvKeysUn and the matches equal to the oracle composition."""
import pytest

import undistort_facade as F

pytestmark = pytest.mark.gpu


def test_tracking_shaped_sequence_sends_no_coordinates(tmp_path, oracle):
    exe = F.compile_test(str(tmp_path / 'undistort_facade_test'))
    F.run_and_check(exe, tmp_path, oracle)
