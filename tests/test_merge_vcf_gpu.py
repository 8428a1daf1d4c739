"""merge_vcf on the MI355X: the device compressor and the device overlap filter write the files the host backends write, and
callVarBamParallel --run --merged_fn leaves one BGZF VCF that holds the per-chunk VCFs' rows."""
import gzip
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_e2e_gpu import FAKE_SAMTOOLS, _bam_case, _model, _run  # noqa: E402
from test_merge_vcf import expected_text, write_case  # noqa: E402
from test_tabix import parse_tbi  # noqa: E402

from clair_amd import overlap_variant  # noqa: E402


def test_device_backends_write_the_files_of_the_host_backends(tmp_path):
    fa, prefix, _ = write_case(str(tmp_path))
    files = {}
    for backend in ("host", "device"):
        out = str(tmp_path / ("%s.vcf.gz" % backend))
        r = _run(["clair_amd.merge_vcf", "--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", out, "--bgzf_deflate", backend, "--overlap_filter", backend])
        assert "1 dropped" in r.stderr
        files[backend] = (open(out, "rb").read(), open(out + ".tbi", "rb").read())
    assert files["device"] == files["host"]
    assert gzip.decompress(files["device"][0]).decode() == overlap_variant.filter_vcf_text(expected_text())


def test_callVarBamParallel_run_merges_its_chunks(tmp_path):
    """Modelled on test_e2e_gpu.test_callVarBamParallel_run_writes_the_vcfs_of_the_printed_commands: same fixture, same region size."""
    tmp = str(tmp_path)
    case, fa, sam = _bam_case(tmp, seed=55)
    ck = _model(tmp)
    common = ["--chkpnt_fn", ck, "--bam_fn", sam, "--ref_fn", fa, "--samtools", FAKE_SAMTOOLS, "--includingAllContigs", "--refChunkSize", "700",
              "--threshold", "0.15", "--minCoverage", "5", "--batch_size", "64", "--python", sys.executable]
    merged = os.path.join(tmp, "all", "snp_and_indel.vcf.gz")
    r = _run(["clair_amd.callVarBamParallel", "--run", "--readers", "2", "--output_prefix", os.path.join(tmp, "all", "var"), "--merged_fn", merged, "--merge_bgzf_deflate", "device"] + common)
    assert "merge_vcf:" in r.stderr
    names = sorted((n for n in os.listdir(os.path.join(tmp, "all")) if n.endswith(".vcf") and case["ctg"] in n),
                   key=lambda n: int(n[:-4].rsplit("_", 2)[1]))
    assert len(names) == 5
    texts = [open(os.path.join(tmp, "all", n)).read() for n in names]
    header = "".join(ln + "\n" for ln in texts[0].splitlines() if ln.startswith("#"))
    rows = [ln + "\n" for t in texts for ln in t.splitlines() if not ln.startswith("#")]
    assert len(rows) > 30
    got = gzip.decompress(open(merged, "rb").read()).decode()
    others = [ln + "\n" for n in os.listdir(os.path.join(tmp, "all")) if n.endswith(".vcf") and case["ctg"] not in n
              for ln in open(os.path.join(tmp, "all", n)).read().splitlines() if not ln.startswith("#")]
    assert got == header + "".join(rows) + "".join(others)                  # the case's contig comes first in the .fai
    index = parse_tbi(open(merged + ".tbi", "rb").read())
    assert index["names"][0] == case["ctg"] and index["header"][0] == 2
