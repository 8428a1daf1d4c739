"""The BAM tools write what they wrote before their shared code became one (clair_amd/bam_stage.py, hostsrc/bam_job.h): every complete
output file of sort_bam, markdup_bam and index_bam over their fixtures, on the host backend with the project's own compressor, against the
SHA-256 recorded in tests/golden/bam_stage_digests.json, and every count of the result dicts with it."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_stage_cases as bc  # noqa: E402


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return bc.write_inputs(tmp_path_factory.mktemp("bam_stage"))


def test_the_golden_file_lists_the_entries():
    golden = bc.golden()
    assert sorted(golden) == sorted(bc.NAMES) and len(bc.NAMES) == 16
    assert all(len(e["sha256"]) == 64 and e["counts"] for e in golden.values())
    groups = [golden[n]["counts"]["groups"] for n in bc.NAMES if n.startswith("sort-") and n.endswith("-groups")]
    assert len(groups) == 3 and min(groups) >= 3
    assert all(golden[n]["counts"]["groups"] == 1 for n in bc.NAMES if n.startswith("sort-") and n.endswith("-default"))


@pytest.mark.parametrize("max_blocks", [2, 64])
@pytest.mark.parametrize("name", bc.NAMES)
def test_the_host_backend_writes_the_recorded_bytes(inputs, name, max_blocks, tmp_path):
    got = bc.run(name, inputs, str(tmp_path / "out"), backend="host", deflate="host", max_blocks=max_blocks)
    assert got == bc.golden()[name]
    assert os.listdir(str(tmp_path)) == ["out"]
