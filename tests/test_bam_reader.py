"""--bam_reader native on the host (CPU only): BGZF, header, .bai, the record walker and the SAM renderer of include/clair_host.h
(clair_host_bam_*, hostsrc/host_bam.cpp) against BAMs written by tests/bam_fixture.py and the canonical text `samtools view` prints for
them; the FASTA slice against tests/fake_samtools.py faidx; the host stages of callVarBam on the BAM against the same stages on the text."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_fixture as bf  # noqa: E402
import frontend_cases as fc  # noqa: E402
import pileup_synth  # noqa: E402

from clair_amd import _hostapi  # noqa: E402

FAKE = os.path.join(HERE, "fake_samtools.py")
FAKE_SAMTOOLS = "%s %s" % (sys.executable, FAKE)


def read_all(path, ctg, lo=None, hi=None, chunk=1 << 20, threads=3, use_index=True):
    r = _hostapi.BamReader(path, threads=threads)
    r.query(ctg, lo, hi, use_index=use_index)
    buf, off, out = np.empty(chunk, np.uint8), _hostapi.bam_offsets_for(chunk), []
    while True:
        n, k = r.readinto(buf, off)
        if not k:
            break
        out.append(r.render(buf, off, k))
    info = r.info()
    r.close()
    return b"".join(out).decode(), info


def fake_view(sam_path, region):
    r = subprocess.run([sys.executable, FAKE, "view", "-F", "2316", sam_path, region], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def view_filter(text, ctg):
    """what `samtools view -F 2316 <bam> ctg` keeps of canonical lines"""
    return "".join(l + "\n" for l in text.splitlines() if not int(l.split("\t")[1]) & 2316 and l.split("\t")[2] == ctg)


def mixed_sam():
    """two contigs, an empty third; unmapped, secondary, supplementary, `*` CIGAR, `*` SEQ, `*` QUAL, odd l_seq, lower case and
    non-IUPAC bases, mate columns, tags, one read of 70 000 CIGAR operations"""
    case = pileup_synth.synth_case(seed=11, n_reads=400, ref_len=40000, read_len=(40, 301))
    lines = [l for l in case["sam"].splitlines() if l and not l.startswith("@")]
    rng = np.random.default_rng(5)
    extra = []
    for k in range(120):
        pos = int(rng.integers(1, 38000))
        n = int(rng.integers(1, 60)) | 1                                  # odd
        seq = "".join(rng.choice(list("ACGTacgtNnRYx.")) for _ in range(n))
        extra.append("b%d\t%d\tchrB\t%d\t%d\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:%d\tRG:Z:g1" % (k, int(rng.choice([0, 16, 1, 256, 2048, 4, 8])), pos, k % 61, n,
                                                                                    pos + 100, 150 - k, seq, "".join(chr(33 + (i % 40)) for i in range(n)), k))
    extra += ["u1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII", "s1\t0\tchrB\t500\t60\t*\t*\t0\t0\tACGT\tIIII", "s2\t0\tchrB\t600\t60\t4M\t*\t0\t0\t*\t*",
              "s3\t0\tchrB\t700\t60\t5M\tchrS\t10\t0\tACGTA\t*", "s4\t16\tchrS\t16380\t60\t20M\t*\t0\t0\t%s\t%s" % ("A" * 20, "I" * 20)]
    ops = "".join("1M1I" for _ in range(35000))                            # 70 000 operations: stored as kSmN, real CIGAR in CG:B:I
    extra.append("long1\t0\tchrS\t2000\t60\t%s\t*\t0\t0\t%s\t*" % (ops, "ACGT" * 17500))
    refs = [("chrS", 40000), ("chrB", 40000), ("chrE", 5000), ("chrOther", 120)]
    return "\n".join(lines + extra) + "\n", refs


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    sam, refs = mixed_sam()
    bam = bf.Bam(sam, refs)
    d = tmp_path_factory.mktemp("bam")
    canon = os.path.join(str(d), "canon.sam")
    open(canon, "w").write(bam.canonical())
    return bam, d, canon


@pytest.mark.parametrize("layout", [dict(per_record=True), dict(block=977), dict(block=65280)], ids=["record_per_block", "straddling", "full_blocks"])
def test_records_render_to_the_canonical_text(mixed, layout):
    bam, d, _ = mixed
    path = os.path.join(str(d), "m.bam")
    bam.write(path, **layout)
    canon = bam.canonical()
    assert "long1\t" in canon and len(canon.split("long1\t")[1].split("\t")[4]) > 65535 * 2
    for ctg in ("chrS", "chrB", "chrE"):
        for threads in (1, 4):
            got, info = read_all(path, ctg, threads=threads, chunk=1 << 20)
            assert got == view_filter(canon, ctg), (ctg, threads)
            assert info["used_index"] == 1 and info["eof_block"] == 1
    # a scan without the index, and records one per chunk
    got, info = read_all(path, "chrB", use_index=False, chunk=1 << 20)
    assert got == view_filter(canon, "chrB") and info["used_index"] == 0
    got, _ = read_all(path, "chrB", chunk=700)
    assert got == view_filter(canon, "chrB")


@pytest.mark.parametrize("region", ["chrS:1-1", "chrS:1-150", "chrS:16300-16400", "chrS:16384-16385", "chrS:32000-32769", "chrS:39900-40000",
                                    "chrS:39999-60000", "chrB:500-700", "chrB:1-40000", "chrE:1-5000", "chrS:2000-2000"])
def test_index_queries_equal_a_scan_and_the_text_view(mixed, region):
    bam, d, canon_path = mixed
    path = os.path.join(str(d), "q.bam")
    bam.write(path, block=1500)
    ctg, lo, hi = region.split(":")[0], int(region.split(":")[1].split("-")[0]), int(region.split("-")[1])
    want = fake_view(canon_path, region)
    indexed, info = read_all(path, ctg, lo, hi)
    scanned, _ = read_all(path, ctg, lo, hi, use_index=False)
    assert indexed == scanned == want and info["used_index"] == 1
    if region.startswith("chrE"):
        assert want == "" and info["records"] == 0


def test_the_aux_walk_to_the_real_cigar_branch_by_branch(tmp_path):
    """ten records that store the placeholder CIGAR: the renderer's CIGAR column against the walk over the aux fields written out in
    tests/aux_walk_cases.py, one record per branch of it"""
    import aux_walk_cases as aw
    bam, want = aw.bam()
    assert len(want) == 10 and want.count(aw.PLACEHOLDER) == 7 and want[:3] == ["4M1I5M"] * 3
    path = str(tmp_path / "aux.bam")
    bam.write(path)
    got, info = read_all(path, aw.CTG)
    rows = [l.split("\t") for l in got.splitlines()]
    assert [r[0] for r in rows] == [r.qname for r in bam.records] and info["records"] == 10
    for row, cigar, (name, _) in zip(rows, want, aw.CASES):
        assert row[5] == cigar, name
    # every other column is the canonical one
    assert ["\t".join(r[:5] + r[6:]) for r in rows] == ["\t".join(l.split("\t")[:5] + l.split("\t")[6:]) for l in bam.canonical().splitlines()]


def test_the_walk_stops_at_the_first_record_past_the_region(mixed):
    bam, d, _ = mixed
    path = os.path.join(str(d), "s.bam")
    bam.write(path, block=1500)
    _, near = read_all(path, "chrS", 1, 200)
    _, whole = read_all(path, "chrS")
    assert 0 < near["records"] < whole["records"] / 4


def _fresh(tmp_path, **write):
    case = fc.synth(3, n_reads=60, ref_len=2000)
    bam = bf.Bam(case["sam"].decode(), [(case["ctg"], 2000)])
    path = str(tmp_path / "x.bam")
    bam.write(path, **write)
    return path, case


def test_corrupt_and_truncated_blocks_name_their_offset(tmp_path):
    path, case = _fresh(tmp_path, block=2000)
    raw = bytearray(open(path, "rb").read())
    second = struct.unpack("<H", raw[16:18])[0] + 1                        # compressed offset of the second block
    bad = bytearray(raw)
    bad[second + 18 + (struct.unpack("<H", raw[second + 16:second + 18])[0] + 1 - 26) // 2] ^= 0x55
    crc = bytearray(raw)
    end2 = second + struct.unpack("<H", raw[second + 16:second + 18])[0] + 1
    crc[end2 - 8] ^= 1
    for name, data, what in (("bad.bam", bad, "offset %d" % second), ("crc.bam", crc, "offset %d" % second), ("cut.bam", raw[:end2 + 40], "truncated")):
        p = str(tmp_path / name)
        open(p, "wb").write(bytes(data))
        with pytest.raises(_hostapi.BamError) as ei:
            read_all(p, case["ctg"], use_index=False)
        assert what in str(ei.value) or "CRC32" in str(ei.value) or "corrupt" in str(ei.value), str(ei.value)
    with pytest.raises(_hostapi.BamError, match="CRC32"):
        read_all(str(tmp_path / "crc.bam"), case["ctg"], use_index=False)


def test_a_missing_eof_block_is_a_warning_only(tmp_path):
    path, case = _fresh(tmp_path, eof=False)
    got, info = read_all(path, case["ctg"])
    assert info["eof_block"] == 0 and got == view_filter(bf.Bam(case["sam"].decode(), [(case["ctg"], 2000)]).canonical(), case["ctg"])


def _args(tmp_path, bam_fn, ref_fn, ctg, *extra):
    from clair_amd import callVarBam
    return callVarBam.build_parser().parse_args(["--bam_fn", bam_fn, "--ref_fn", ref_fn, "--ctgName", ctg, "--samtools", FAKE_SAMTOOLS,
                                                 "--bam_reader", "native"] + list(extra))


def _case_files(tmp_path, seed=301, index=True, block=3000):
    case = pileup_synth.synth_case(seed=seed, n_reads=500, ref_len=3000)
    fa = str(tmp_path / "ref.fa")
    text, fai = bf.fasta_of({case["ctg"]: "".join(l for l in case["fasta"].split(">chrOther")[0].splitlines()[1:]), "chrOther": "ACGT" * 30})
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    bam = bf.Bam(case["sam"], [(case["ctg"], 3000), ("chrOther", 120)])
    bam_fn = str(tmp_path / "reads.bam")
    bam.write(bam_fn, block=block, index=index)
    canon = str(tmp_path / "canon.sam")
    open(canon, "w").write(bam.canonical())
    return case, fa, bam_fn, canon


def test_clean_exits(tmp_path):
    from clair_amd import callVarBam
    case, fa, bam_fn, canon = _case_files(tmp_path)
    with pytest.raises(SystemExit, match="not in the header"):
        callVarBam.native_reader(_args(tmp_path, bam_fn, fa, "chrNope"), "chrNope")
    for path, text in (("t.sam", open(canon).read()), ("t.cram", "CRAM\3\0"), ("t.gz", None)):
        p = str(tmp_path / path)
        if text is None:
            import gzip
            with gzip.open(p, "wt") as f:
                f.write(open(canon).read())
        else:
            open(p, "w").write(text)
        with pytest.raises(SystemExit, match="--bam_reader samtools"):
            callVarBam.native_reader(_args(tmp_path, p, fa, case["ctg"]), case["ctg"])
    csi = str(tmp_path / "c.bam")
    open(csi, "wb").write(open(bam_fn, "rb").read())
    open(csi + ".csi", "wb").write(b"CSI\1")
    with pytest.raises(SystemExit, match=r"\.csi.*--bam_reader samtools"):
        callVarBam.native_reader(_args(tmp_path, csi, fa, case["ctg"]), case["ctg"])
    base = ["--chkpnt_fn", "x", "--bam_fn", bam_fn, "--ref_fn", fa, "--ctgName", case["ctg"], "--call_fn", str(tmp_path / "o.vcf"), "--bam_reader", "native"]
    for extra, name in ((["--samtools_view_args=-x"], "--samtools_view_args"), (["--samtools_threads", "2"], "--samtools_threads"),
                        (["--view_readers", "2"], "--view_readers"), (["--bam_threads", "17"], "--bam_threads")):
        with pytest.raises(SystemExit, match=name):
            callVarBam.main(base + extra)


@pytest.mark.parametrize("region", [(None, None), (1, 1), (100, 250), (2950, 9000), (1, 3000)])
def test_native_fasta_slice_equals_faidx(tmp_path, region):
    seq = "".join("acgtACGTNn"[i % 10] for i in range(3007))
    text, fai = bf.fasta_of({"chrL": seq, "chrM": "ACGT" * 50}, width=61)
    fa = str(tmp_path / "l.fa")
    open(fa, "w").write(text)
    open(fa + ".fai", "w").write(fai)
    reg = "chrL" if region[0] is None else "chrL:%d-%d" % region
    r = subprocess.run([sys.executable, FAKE, "faidx", fa, reg], capture_output=True, text=True)
    want = "".join(r.stdout.splitlines()[1:])
    assert _hostapi.faidx(fa, "chrL", *region) == want and any(c.islower() for c in want)
    assert _hostapi.faidx(fa, "chrNope") is None
    from clair_amd import create_tensor as ct, extract_variant_candidates as evc
    if region[0] is not None:
        assert ct.reference_sequence_from(FAKE_SAMTOOLS, fa, "chrL", region[0] + 5, region[1], native=True) == \
            ct.reference_sequence_from(FAKE_SAMTOOLS, fa, "chrL", region[0] + 5, region[1])
    assert evc.load_reference(FAKE_SAMTOOLS, fa, reg, native=True) == evc.load_reference(FAKE_SAMTOOLS, fa, reg)


@pytest.mark.parametrize("index", [True, False], ids=["bai", "scan"])
@pytest.mark.parametrize("region", [[], ["--ctgStart", "300", "--ctgEnd", "2500"]], ids=["contig", "region"])
def test_host_stages_on_the_bam_equal_the_host_stages_on_the_text(tmp_path, region, index):
    """candidate_positions / tensor_batches (--front_end host) with --bam_reader native on the BAM = the same with samtools on the canonical text"""
    from clair_amd import callVarBam
    case, fa, bam_fn, canon = _case_files(tmp_path, index=index)
    native = _args(tmp_path, bam_fn, fa, case["ctg"], "--threshold", "0.15", "--minCoverage", "5", *region)
    text = callVarBam.build_parser().parse_args(["--bam_fn", canon, "--ref_fn", fa, "--ctgName", case["ctg"], "--samtools", FAKE_SAMTOOLS,
                                                 "--threshold", "0.15", "--minCoverage", "5"] + region)
    for a in (native, text):
        callVarBam.normalise(a)
    pos_n, pos_t = callVarBam.candidate_positions(native), callVarBam.candidate_positions(text)
    assert len(pos_t) > 20 and np.array_equal(pos_n, pos_t)
    got = list(callVarBam.tensor_batches(native, pos_n, 64, progress=False))
    want = list(callVarBam.tensor_batches(text, pos_t, 64, progress=False))
    assert len(got) == len(want) > 1
    for (xg, ig, cg), (xw, iw, cw) in zip(got, want):
        assert np.array_equal(xg, xw) and np.array_equal(cg, cw) and np.array_equal(ig.pos, iw.pos)


def test_parallel_commands_pass_the_reader_on(tmp_path):
    from clair_amd import callVarBamParallel as par
    for fn, text in (("ref.fa", ">x\n"), ("ref.fa.fai", "chr1\t25000000\t6\t60\t61\n"), ("a.bam", ""), ("model.meta", "")):
        open(str(tmp_path / fn), "w").write(text)
    argv = ["--chkpnt_fn", str(tmp_path / "model"), "--ref_fn", str(tmp_path / "ref.fa"), "--bam_fn", str(tmp_path / "a.bam"),
            "--output_prefix", str(tmp_path / "var"), "--python", "PY"]
    plain = par.commands(par.build_parser().parse_args(argv))
    native = par.commands(par.build_parser().parse_args(argv + ["--bam_reader", "native", "--bam_threads", "8"]))
    assert len(plain) == len(native) == 3
    assert all("--bam_reader" not in l for l in plain)
    assert all(' --bam_reader "native" --bam_threads "8" ' in l + " " for l in native)
    args = callVarBam_args_of(native[0])
    assert args.bam_reader == "native" and args.bam_threads == 8


def callVarBam_args_of(line):
    import shlex
    from clair_amd import callVarBam
    argv = shlex.split(line)
    return callVarBam.build_parser().parse_args(argv[argv.index("clair_amd.callVarBam") + 1:])
