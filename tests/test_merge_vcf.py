"""python -m clair_amd.merge_vcf: the per-chunk VCFs as one sorted file, the overlap filter across chunk borders, BGZF and .tbi output, and
callVarBamParallel's --merged_fn guard.  The chunk files are synthesised here."""
import gzip
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_tabix import BgzfFile, fetch, parse_tbi  # noqa: E402

from clair_amd import overlap_variant  # noqa: E402

HEADER = "##fileformat=VCFv4.1\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
CONTIGS = ["chr1", "chr2", "chr10", "chrUn_KI270302v1", "HLA-A.01_02"]       # .fai order: not lexicographic; names with '_' and '.'


def row(ctg, pos, ref="A", alt="G", qual=50):
    return "%s\t%d\t.\t%s\t%s\t%d\t.\t.\tGT:GQ:DP:AF\t0/1:%d:30:0.5000\n" % (ctg, pos, ref, alt, qual, qual)


def chunks():
    """{(contig, start, end): rows}: chr2's first chunk ends in a deletion that covers the SNP the second begins with."""
    return {
        ("chr1", 0, 1000): [row("chr1", 10), row("chr1", 500, "AT", "A", 70)],
        ("chr2", 0, 1000): [row("chr2", 20), row("chr2", 998, "ACGTA", "A", 80)],
        ("chr2", 1000, 2000): [row("chr2", 1001, "C", "T", 30), row("chr2", 1500)],
        ("chr2", 2000, 3000): [],                                                # a header and no records
        ("chr10", 0, 1000): [row("chr10", 7), row("chr10", 9)],
        ("chrUn_KI270302v1", 0, 1000): [row("chrUn_KI270302v1", 3)],
        ("HLA-A.01_02", 0, 1000): [row("HLA-A.01_02", 5, "G", "GTT", 12)],
    }


def write_case(tmp, which=None):
    os.makedirs(os.path.join(tmp, "out"), exist_ok=True)
    fa = os.path.join(tmp, "ref.fa")
    with open(fa + ".fai", "w") as f:
        for k, name in enumerate(CONTIGS):
            f.write("%s\t5000\t%d\t60\t61\n" % (name, 10 + 6000 * k))
    paths = {}
    for (ctg, start, end), rows in chunks().items():
        if which is not None and (ctg, start, end) not in which:
            continue
        paths[(ctg, start, end)] = os.path.join(tmp, "out", "var.%s_%d_%d.vcf" % (ctg, start, end))
        with open(paths[(ctg, start, end)], "w") as f:
            f.write(HEADER + "".join(rows))
    return fa, os.path.join(tmp, "out", "var"), paths


def expected_text():
    c = chunks()
    order = sorted(c, key=lambda k: (CONTIGS.index(k[0]), k[1]))
    return HEADER + "".join("".join(c[k]) for k in order)


def run(argv):
    return subprocess.run([sys.executable, "-m", "clair_amd.merge_vcf"] + argv, capture_output=True, text=True, cwd=ROOT)


def test_merged_text_is_the_concatenation_in_fai_order(tmp_path):
    fa, prefix, _ = write_case(str(tmp_path))
    out = str(tmp_path / "merged.vcf")
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", out])
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    assert text == expected_text()
    assert text.index("chr2\t") < text.index("chr10\t") < text.index("chrUn_KI270302v1\t") < text.index("HLA-A.01_02\t")
    assert not os.path.exists(out + ".tbi")                                  # plain text gets no index
    assert "7 file(s), 10 row(s) in, 0 dropped" in r.stderr


@pytest.mark.parametrize("backend", ["host", "python"])
def test_overlap_filter_sees_the_pair_across_the_chunk_border(tmp_path, backend):
    fa, prefix, _ = write_case(str(tmp_path))
    off, on = str(tmp_path / "off.vcf"), str(tmp_path / "on.vcf")
    assert run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", off]).returncode == 0
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", on, "--overlap_filter", backend])
    assert r.returncode == 0, r.stderr
    kept, filtered = open(off).read(), open(on).read()
    assert "chr2\t998\t" in kept and "chr2\t1001\t" in kept                  # off: both rows stay
    assert "chr2\t998\t" in filtered and "chr2\t1001\t" not in filtered     # the deletion (QUAL 80) covers the SNP (QUAL 30) of the next chunk
    assert filtered == overlap_variant.filter_vcf_text(expected_text())
    assert "1 dropped" in r.stderr


def test_incomplete_file_is_named(tmp_path):
    fa, prefix, paths = write_case(str(tmp_path))
    broken = [paths[("chr1", 0, 1000)], paths[("chr10", 0, 1000)]]
    for p in broken:
        with open(p, "r+") as f:
            text = f.read()
            f.seek(0)
            f.truncate()
            f.write(text[:-1])
    out = str(tmp_path / "merged.vcf")
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", out])
    assert r.returncode != 0 and "incomplete" in r.stderr and all(p in r.stderr for p in broken)
    assert not os.path.exists(out)


def test_differing_header_is_an_error(tmp_path):
    fa, prefix, paths = write_case(str(tmp_path))
    p = paths[("chr2", 1000, 2000)]
    text = open(p).read()
    open(p, "w").write(text.replace("VCFv4.1", "VCFv4.2"))
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", str(tmp_path / "merged.vcf")])
    assert r.returncode != 0 and p in r.stderr and "header" in r.stderr


def test_contig_outside_the_fai_is_an_error(tmp_path):
    fa, prefix, _ = write_case(str(tmp_path))
    with open(prefix + ".chrZ_0_1000.vcf", "w") as f:
        f.write(HEADER + row("chrZ", 4))
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", str(tmp_path / "merged.vcf")])
    assert r.returncode != 0 and "chrZ" in r.stderr


def test_explicit_files_out_of_order_come_out_sorted(tmp_path):
    fa, prefix, paths = write_case(str(tmp_path))
    given = [paths[k] for k in sorted(paths, key=lambda k: (k[0], -k[1]))]       # lexicographic contigs, starts descending
    out = str(tmp_path / "merged.vcf")
    r = run(["--ref_fn", fa, "--merged_fn", out] + given)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == expected_text()


def test_unsorted_rows_are_sorted_stably(tmp_path):
    tmp = str(tmp_path)
    fa, prefix, paths = write_case(tmp, which=[("chr1", 0, 1000)])
    with open(paths[("chr1", 0, 1000)], "w") as f:
        f.write(HEADER + row("chr1", 500, "A", "C") + row("chr1", 10) + row("chr1", 500, "A", "T"))
    out = str(tmp_path / "merged.vcf")
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", out])
    assert r.returncode == 0 and "(sorted)" in r.stderr
    assert open(out).read() == HEADER + row("chr1", 10) + row("chr1", 500, "A", "C") + row("chr1", 500, "A", "T")


@pytest.mark.parametrize("deflate", ["host", "zlib"])
def test_gz_output_is_bgzf_with_an_index(tmp_path, deflate):
    fa, prefix, _ = write_case(str(tmp_path))
    out = str(tmp_path / "snp_and_indel.vcf.gz")
    r = run(["--output_prefix", prefix, "--ref_fn", fa, "--merged_fn", out, "--bgzf_deflate", deflate])
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    assert gzip.decompress(data).decode() == expected_text()
    index = parse_tbi(open(out + ".tbi", "rb").read())
    assert index["header"] == (2, 1, 2, 0, ord("#"), 0) and index["names"] == CONTIGS
    assert [r_.rstrip("\n") for r_ in chunks()[("chr2", 0, 1000)][1:] + chunks()[("chr2", 1000, 2000)][:1]] == fetch(index, BgzfFile(data), "chr2", 999, 1001)
    assert fetch(index, BgzfFile(data), "chr10", 0, 100) == [r_.rstrip("\n") for r_ in chunks()[("chr10", 0, 1000)]]
    assert fetch(index, BgzfFile(data), "HLA-A.01_02", 4, 5) == [chunks()[("HLA-A.01_02", 0, 1000)][0].rstrip("\n")]


def test_dispatcher_help_and_parallel_guard(tmp_path):
    r = subprocess.run([sys.executable, "-m", "clair_amd", "merge_vcf", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "--merged_fn" in r.stdout and "--bgzf_deflate" in r.stdout
    r = subprocess.run([sys.executable, "-m", "clair_amd.callVarBamParallel", "--chkpnt_fn", "x", "--output_prefix", "out/var", "--merged_fn", "m.vcf.gz"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "--merged_fn needs --run" in r.stderr and "python -m clair_amd.merge_vcf" in r.stderr
