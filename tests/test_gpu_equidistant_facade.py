"""-m gpu: the Tracking-shaped sequence of tests/cpp/equidistant_facade_test.cpp with a camaraModo == 1 camera: extractUndistorted equals
the host orbfe::UndistortKeyPoints, residentUploads() == 0, zero bytes of coordinates sent, mvKeysUn and the matches equal to the oracle
composition."""
import pytest

import equidistant_facade as F

pytestmark = pytest.mark.gpu


def test_tracking_shaped_sequence_of_a_fisheye_camera(tmp_path, oracle):
    exe = F.compile_test(str(tmp_path / 'equidistant_facade_test'))
    F.run_and_check(exe, tmp_path, oracle)
