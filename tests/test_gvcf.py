"""gVCF on the CPU (docs/gvcf.md): the host twin's tallies and block records against the restatement of tests/gvcf_cases.py, the interval
arithmetic, the text of the file and the command lines.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import frontend_cases as fc  # noqa: E402
import gvcf_cases as gc  # noqa: E402

from clair_amd import gvcf  # noqa: E402

FAKE_SAMTOOLS = "%s %s" % (sys.executable, os.path.join(HERE, "fake_samtools.py"))
BAND_VARIANTS = {"gatk": gc.GATK_BANDS, "one": [], "each": list(range(1, 100))}


def _stacks():
    return {
        "flat": gc.stack_case(300, [(20, 280, 5)]),
        "steps": gc.stack_case(400, [(10, 390, 2), (50, 120, 4), (100, 300, 9), (290, 291, 40)]),
        "alt_and_n": gc.stack_case(260, [(5, 250, 8), (40, 200, 3)], alt={60: None, 61: "N", 130: "N", 131: "R", 200: None},
                                   ref_edit={20: "N", 90: "R", 91: "Y", 150: "n", 151: "K"}),
        "empty": gc.stack_case(150, []),
    }


_CACHE = {}


def _case(name):
    """(case, restated tallies, rows taken out of the allowed set), made once per name"""
    if name not in _CACHE:
        if name.startswith("stack:"):
            case = _stacks()[name[6:]]
        elif name.startswith("golden:"):
            case = gc.golden_case(os.path.join(HERE, "golden", name[7:]))
        else:
            case = gc.synth_case(int(name[6:]), n_reads=120, ref_len=1500, ins_rate=0.04, del_rate=0.04)
        pile = case.get("ctg_range")
        tallies = gc.restate_tallies(case["sam"], case["ctg"], case["lo"], case["hi"], pile_region=pile)
        n = len(case["ref"])
        rows = [(n // 7, 1), (n // 3, 4), (n // 3 + 2, 1), (n - 40, 2)]      # a SNP, a deletion with a row inside its span, one more
        _CACHE[name] = (case, tallies, rows)
    return _CACHE[name]


CASES = (["stack:" + k for k in ("flat", "steps", "alt_and_n", "empty")] + ["golden:" + os.path.basename(p) for p in fc.EVC_GOLDEN]
         + ["synth:%d" % s for s in (3, 17, 40)])


def _allowed(case, rows):
    span = (case["ctg_range"][0] - 1, case["ctg_range"][1]) if case.get("ctg_range") else (case["ref0"], case["ref0"] + len(case["ref"]))
    return span, gc.restate_allowed(span, (case["lo"], case["hi"]), case.get("bed"), rows)


def _product_allowed(case, span, rows):
    from clair_amd._hostapi import merged_bed
    bs, be, n_bed = merged_bed(case.get("bed"))
    pos = np.array([r[0] for r in rows], dtype=np.int64)
    length = np.array([r[1] for r in rows], dtype=np.int64)
    return gvcf.allowed_intervals(span, (case["lo"], case["hi"]), None if n_bed < 0 else (bs, be), pos, pos + length)


@pytest.mark.parametrize("name", CASES)
def test_twin_tallies_equal_the_restatement(name):
    case, want, _ = _case(name)
    got = gc.host_tallies(case, pile_region=case.get("ctg_range"))
    assert got.anomalies == 0
    assert got.tallies.tolist() == want
    if name != "stack:empty":
        assert got.tallies.sum() > 0


@pytest.mark.parametrize("bands", sorted(BAND_VARIANTS))
@pytest.mark.parametrize("name", CASES)
def test_twin_records_equal_the_restatement_and_tile_the_allowed_set(name, bands):
    case, tallies, rows = _case(name)
    span, allowed = _allowed(case, rows)
    st, en = _product_allowed(case, span, rows)
    assert list(zip(st.tolist(), en.tolist())) == allowed
    bounds = gvcf.parse_bands(BAND_VARIANTS[bands])
    table = gvcf.band_table(bounds)
    assert [int(table[g]) for g in range(100)] == [sum(1 for b in bounds if b <= g) - 1 for g in range(100)]
    for e in (0.001, 0.1, 0.3):
        costs = gvcf.costs_from(e)
        assert costs == gc.restate_costs(e) and costs[2] == 3083
        want = gc.restate_blocks(tallies, case["lo"], case["ref"], case["ref0"], costs, BAND_VARIANTS[bands], allowed)
        got = gvcf.host_blocks(np.array(tallies, dtype=np.uint32).reshape(-1, 7), case["lo"], case["ref"], case["ref0"], costs, table, st, en, guard=3)
        assert (got[-3:].view(np.uint8) == 0xA5).all()          # nothing behind the records was touched
        assert gc.records_as_tuples(got[:-3]) == want
        gc.check_tiling(want, allowed)
    if bands == "one":
        assert len(want) == len(allowed)
    if bands == "gatk" and name in ("stack:steps", "golden:pileup_evc_default.json.gz"):
        assert len(want) > len(allowed) + 3


def test_costs_and_bands_are_checked():
    assert gvcf.costs_from(0.1) == (469, 10240, 3083)
    assert gvcf.costs_from(0.001) == (4, 30720, 3083)
    # 0 < e < 1; below about 1.1e-4 c_match rounds to 0, near 1 c_err does, and 1e-14 would also need 140 phred: all outside 1 .. 2^17 - 1
    for e in (0.0, 1.0, -0.5, float("nan"), 1e-5, 1e-14, 0.9999999):
        with pytest.raises(ValueError):
            gvcf.costs_from(e)
    assert gvcf.parse_bands(None) == [0] + gc.GATK_BANDS
    assert gvcf.parse_bands("20, 40") == [0, 20, 40] and gvcf.parse_bands("") == [0]
    for bad in ("5,5", "9,3", "100", "-1", "a"):
        with pytest.raises(ValueError):
            gvcf.parse_bands(bad)


def test_twin_verdicts_on_bad_intervals():
    case, tallies, _ = _case("stack:flat")
    t = np.array(tallies, dtype=np.uint32).reshape(-1, 7)
    table = gvcf.band_table([0])
    for st, en, word in (([50, 10], [60, 20], "sorted and disjoint"), ([10, 15], [20, 30], "sorted and disjoint"), ([10], [10], "is empty"),
                         ([-5], [10], "outside the tables"), ([10], [301], "outside the tables")):
        with pytest.raises(gvcf.GvcfArgumentError, match=word):
            gvcf.host_blocks(t, 0, case["ref"], 0, (469, 10240, 3083), table, st, en)
    with pytest.raises(gvcf.GvcfArgumentError, match="cost c_err"):
        gvcf.host_blocks(t, 0, case["ref"], 0, (469, 1 << 17, 3083), table, [0], [10])
    assert len(gvcf.host_blocks(t, 0, case["ref"], 0, (469, 10240, 3083), table, [0, 10], [10, 300])) == 2      # adjacent intervals stay two


# ---- the file ------------------------------------------------------------------------------------------------------------------------------
HEADER = ["##fileformat=VCFv4.1\n", "##FILTER=<ID=PASS,Description=\"All filters passed\">\n", "##contig=<ID=chrG,length=400>\n",
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"]


def _row(ctg, pos1, ref, alt):
    return "%s\t%d\t.\t%s\t%s\t33\tPASS\t.\tGT:GQ:DP:AF\t0/1:33:9:0.5\n" % (ctg, pos1, ref, alt)


def _parse_block_row(line):
    col = line.rstrip("\n").split("\t")
    assert col[2] == "." and col[4] == "<NON_REF>" and col[5] == "." and col[6] == "." and col[8] == "GT:GQ:DP:MIN_DP:PL"
    gt, gq, dp, min_dp, pl = col[9].split(":")
    assert gt == "0/0" and col[7].startswith("END=")
    return col[0], col[3], (int(col[1]) - 1, int(col[7][4:]), int(min_dp), int(dp), int(gq)) + tuple(int(x) for x in pl.split(","))


def _write_case(tmp, case, rows_text):
    fa, sam, vcf = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.sam"), os.path.join(tmp, "calls.vcf")
    ref = case["ref"]
    open(fa, "w").write(">%s\n%s\n" % (case["ctg"], "\n".join(ref[i:i + 60] for i in range(0, len(ref), 60))))
    open(fa + ".fai", "w").write("%s\t%d\t%d\t60\t61\n" % (case["ctg"], len(ref), len(case["ctg"]) + 2))
    open(sam, "wb").write(case["sam"])
    open(vcf, "w").write(rows_text)
    return ["--bam_fn", sam, "--ref_fn", fa, "--ctgName", case["ctg"], "--vcf_fn", vcf, "--samtools", FAKE_SAMTOOLS]


def _expected_file(case, header, rows, span, bed, costs, band_list, tallies=None):
    """the whole gVCF from the restatement: header, rows with <NON_REF>, block rows, interleaved by position"""
    spans = [(int(r.split("\t")[1]) - 1, len(r.split("\t")[3])) for r in rows]
    allowed = gc.restate_allowed(span, (case["lo"], case["hi"]), bed, spans)
    if tallies is None:
        tallies = gc.restate_tallies(case["sam"], case["ctg"], case["lo"], case["hi"])
    blocks = gc.restate_blocks(tallies, case["lo"], case["ref"], case["ref0"], costs, band_list, allowed)
    bounds = sorted(set([0] + band_list))
    extra = [l + "\n" for l in gvcf.EXTRA_HEADER.splitlines()]
    extra += ["##GVCFBlock%d-%d=minGQ=%d(inclusive),maxGQ=%d(exclusive)\n" % (a, b, a, b) for a, b in zip(bounds, bounds[1:] + [100])]
    body = [(b[0], 1, gc.restate_row(case["ctg"], case["ref"], case["ref0"], b)) for b in blocks]
    for k, r in enumerate(rows):
        col = r.split("\t")
        col[4] = "<NON_REF>" if col[4] == "." else col[4] + ",<NON_REF>"
        body.append((int(col[1]) - 1, 0, "\t".join(col)))
    body.sort(key=lambda x: (x[0], x[1]))                   # stable: rows of one position keep their order; no block shares a position with a row
    return "".join(header[:-1] + extra + header[-1:] + [x[2] for x in body]), blocks, allowed


def test_file_text_header_rows_and_blocks(tmp_path):
    """Header lines, verbatim rows plus <NON_REF>, block rows that parse back to the records; overlapping rows, a row at the first and one at the
    last position of the region, a --showRef row."""
    case = _stacks()["steps"]
    case["lo"], case["hi"] = -64, 400 + 64                  # the tables callVarBam makes for a whole contig
    ref = case["ref"]
    rows = [_row("chrG", 1, ref[0], "T" if ref[0] != "T" else "A"), _row("chrG", 101, ref[100:105], ref[100]), _row("chrG", 103, ref[102], "."),
            _row("chrG", 104, ref[103:110], ref[103]), _row("chrG", 400, ref[399], "G,<*>")]
    argv = _write_case(str(tmp_path), case, "".join(HEADER + rows))
    out = os.path.join(str(tmp_path), "o.g.vcf")
    gvcf.main(argv + ["--gvcf_fn", out, "--backend", "host"])
    want, blocks, allowed = _expected_file(case, HEADER, rows, (0, 400), None, gc.restate_costs(0.1), gc.GATK_BANDS)
    got = open(out).read()
    assert got == want
    assert allowed[0][0] == 1 and allowed[-1][1] == 399 and (110, 399) in allowed
    lines = got.splitlines(True)
    assert lines[:3] == HEADER[:3] and lines[3].startswith("##ALT=<ID=NON_REF,") and lines[4].startswith("##INFO=<ID=END,")
    assert lines[5].startswith("##FORMAT=<ID=MIN_DP,") and lines[6].startswith("##FORMAT=<ID=PL,Number=G,")
    assert lines[7] == "##GVCFBlock0-1=minGQ=0(inclusive),maxGQ=1(exclusive)\n" and "##GVCFBlock99-100=minGQ=99(inclusive),maxGQ=100(exclusive)\n" in lines
    assert sum(l.startswith("##GVCFBlock") for l in lines) == 65 and lines[7 + 65] == HEADER[3]
    body = lines[7 + 66:]
    parsed = [_parse_block_row(l) for l in body if "<NON_REF>\t.\t.\tEND=" in l]
    assert [p[2] for p in parsed] == blocks and all(p[0] == "chrG" and p[1] == ref[p[2][0]] for p in parsed)
    kept = [l for l in body if "END=" not in l]
    assert [l.replace(",<NON_REF>", "").replace("<NON_REF>", ".") for l in kept] == rows and kept[2].split("\t")[4] == "<NON_REF>"
    assert kept[4].split("\t")[4] == "G,<*>,<NON_REF>"
    positions = [int(l.split("\t")[1]) for l in body]
    assert positions == sorted(positions)


def test_file_with_an_empty_call_vcf_a_region_a_bed_and_no_reads(tmp_path):
    """An empty call VCF (a header alone, and no byte at all); a region without reads gives one GQ 0, MIN_DP 0 block per allowed interval."""
    tmp = str(tmp_path)
    case = _stacks()["empty"]
    case["lo"], case["hi"] = 20 - 1 - 64, 120 + 64          # callVarBam's tables for --ctgStart 20 --ctgEnd 120
    bed = os.path.join(tmp, "r.bed")
    open(bed, "w").write("chrG\t10\t40\nchrG\t60\t61\nchrG\t100\t140\nchrOther\t1\t5\n")
    for text, header in (("".join(HEADER), HEADER), ("", ["##fileformat=VCFv4.1\n", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"])):
        argv = _write_case(tmp, case, text)
        out = os.path.join(tmp, "o.g.vcf")
        gvcf.main(argv + ["--gvcf_fn", out, "--backend", "host", "--ctgStart", "20", "--ctgEnd", "120", "--bed_fn", bed, "--gvcf_gq_bands", "20,40"])
        want, blocks, allowed = _expected_file(case, header, [], (19, 120), [(10, 40), (60, 61), (100, 140)], gc.restate_costs(0.1), [20, 40])
        assert open(out).read() == want
        assert allowed == [(19, 40), (60, 61), (100, 120)]
        assert blocks == [(a, b, 0, 0, 0, 0, 0, 0) for a, b in allowed]
        assert open(out).read().count("##GVCFBlock") == 3


def test_a_region_that_ends_beyond_the_contig_is_cut_at_its_end(tmp_path):
    tmp = str(tmp_path)
    case = _stacks()["flat"]
    case["lo"], case["hi"] = 250 - 1 - 64, 1000 + 64
    argv = _write_case(tmp, case, "".join(HEADER))
    out = os.path.join(tmp, "o.g.vcf")
    gvcf.main(argv + ["--gvcf_fn", out, "--backend", "host", "--ctgStart", "250", "--ctgEnd", "1000"])
    case["hi"] = 300
    want, blocks, allowed = _expected_file(case, HEADER, [], (249, 1000), None, gc.restate_costs(0.1), gc.GATK_BANDS)
    assert open(out).read() == want and allowed == [(249, 300)] and [(b[0], b[1]) for b in blocks] == [(249, 280), (280, 300)]


def test_stand_alone_host_backend_on_a_golden_fixture(tmp_path):
    """The stand-alone command end to end over a reference-minted fixture's SAM and FASTA, with an error rate of its own."""
    tmp = str(tmp_path)
    case, tallies, spans = _case("golden:pileup_evc_default.json.gz")
    ref = case["ref"]
    rows = [_row(case["ctg"], p + 1, ref[p:p + n], "A" if ref[p] != "A" else "C") for p, n in spans]
    header = HEADER[:2] + ["##contig=<ID=%s,length=%d>\n" % (case["ctg"], len(ref))] + HEADER[3:]
    argv = _write_case(tmp, case, "".join(header + rows))
    out = os.path.join(tmp, "o.g.vcf")
    gvcf.main(argv + ["--gvcf_fn", out, "--backend", "host", "--gvcf_error_rate", "0.3"])
    want, blocks, _ = _expected_file(case, header, rows, (0, len(ref)), None, gc.restate_costs(0.3), gc.GATK_BANDS, tallies=tallies)
    assert open(out).read() == want and len(blocks) > 100


# ---- command lines -------------------------------------------------------------------------------------------------------------------------
def _cli(argv):
    return subprocess.run([sys.executable, "-m"] + argv, cwd=ROOT, capture_output=True, text=True)


def test_help_texts():
    r = _cli(["clair_amd", "gvcf", "--help"])
    assert r.returncode == 0 and "--gvcf_fn" in r.stdout and "--backend" in r.stdout and "--gvcf_gq_bands" in r.stdout
    r = _cli(["clair_amd", "callVarBam", "--help"])
    assert r.returncode == 0 and "--gvcf_fn" in r.stdout and "--gvcf_error_rate" in r.stdout
    assert "gvcf" in _cli(["clair_amd", "--help"]).stdout
    r = _cli(["clair_amd", "callVarBamParallel", "--help"])
    assert r.returncode == 0 and "--gvcf " in r.stdout.replace("\n", " ")


def test_callVarBam_refuses_what_is_out_of_scope(tmp_path):
    from clair_amd import callVarBam
    tmp = str(tmp_path)
    for name in ("a.bam", "ref.fa", "b.bam"):
        open(os.path.join(tmp, name), "w").write("x")
    base = ["--bam_fn", os.path.join(tmp, "a.bam"), "--ref_fn", os.path.join(tmp, "ref.fa"), "--ctgName", "c", "--call_fn", os.path.join(tmp, "o.vcf"),
            "--gvcf_fn", os.path.join(tmp, "o.g.vcf"), "--chkpnt_fn", "none"]
    parser = callVarBam.build_parser()
    for extra, word in ((["--vcf_fn", "sites.vcf"], "--vcf_fn"), (["--ensemble_bam_fn", os.path.join(tmp, "b.bam")], "--ensemble_bam_fn"),
                        (["--bam_reader", "native", "--ensemble_subsample", "0.5"], "--ensemble_subsample"), (["--output_for_ensemble"], "--output_for_ensemble"),
                        (["--gvcf_error_rate", "1.5"], "--gvcf_error_rate"), (["--gvcf_error_rate", "1e-14"], "outside 1 .."),
                        (["--gvcf_gq_bands", "30,10"], "--gvcf_gq_bands")):
        with pytest.raises(SystemExit) as ei:
            callVarBam.normalise(parser.parse_args(base + extra))
        assert word in str(ei.value) and "[ERROR]" in str(ei.value), extra
    callVarBam.normalise(parser.parse_args(base))            # the flag alone is fine
    r = _cli(["clair_amd.gvcf", "--bam_fn", os.path.join(tmp, "a.bam"), "--ref_fn", os.path.join(tmp, "ref.fa"), "--ctgName", "c", "--vcf_fn",
              os.path.join(tmp, "a.bam"), "--gvcf_fn", os.path.join(tmp, "x.g.vcf"), "--gvcf_error_rate", "0"])
    assert r.returncode != 0 and "--gvcf_error_rate" in r.stderr and not os.path.exists(os.path.join(tmp, "x.g.vcf"))


def test_callVarBamParallel_names_the_chunks_gvcfs(tmp_path):
    from clair_amd import callVarBamParallel as par
    tmp = str(tmp_path)
    for name, text in (("a.bam", "x"), ("ref.fa", "x"), ("ref.fa.fai", "chr20\t2500\t6\t60\t61\n"), ("m.npz", "x")):
        open(os.path.join(tmp, name), "w").write(text)
    common = ["--chkpnt_fn", os.path.join(tmp, "m"), "--bam_fn", os.path.join(tmp, "a.bam"), "--ref_fn", os.path.join(tmp, "ref.fa"), "--refChunkSize", "1000",
              "--output_prefix", os.path.join(tmp, "var")]
    plain = par.commands(par.build_parser().parse_args(common))
    assert len(plain) == 3 and not any("gvcf" in l for l in plain)
    lines = par.commands(par.build_parser().parse_args(common + ["--gvcf", "--gvcf_error_rate", "0.05"]))
    for l, (a, b) in zip(lines, ((0, 1000), (1000, 2000), (2000, 2500))):
        name = '--gvcf_fn "%s.chr20_%d_%d.gvcf"' % (os.path.join(tmp, "var"), a, b)
        assert name in l and '--gvcf_error_rate "0.05"' in l and not name.rstrip('"').endswith(".vcf")
        assert l.replace(" " + name, "").replace(' --gvcf_error_rate "0.05"', "") == plain[lines.index(l)]
