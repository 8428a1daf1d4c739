"""The BAM tools on the device write the bytes recorded for the host backend (tests/golden/bam_stage_digests.json): sort_bam, markdup_bam and
index_bam over their fixtures with backend="device" and the device's own compressor, complete files by SHA-256, and the counts."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_stage_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return bc.write_inputs(tmp_path_factory.mktemp("bam_stage_gpu"))


@pytest.mark.parametrize("name", bc.NAMES)
def test_the_device_backend_writes_the_recorded_bytes(inputs, name, tmp_path):
    got = bc.run(name, inputs, str(tmp_path / "out"), backend="device", deflate="device")
    assert got == bc.golden()[name]
    assert os.listdir(str(tmp_path)) == ["out"]
