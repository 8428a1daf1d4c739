"""GetTruth: truth VCF -> rows `ctg pos ref alt g1 g2` (dataPrepScripts/GetTruth.py), the `--var_fn` of `evaluate`.

What the reference does, kept as it is written there:
  * records of --ctgName inside --ctgStart..--ctgEnd (both given, 1-based inclusive), in file order            GetTruth.py:100-110
  * genotype from the first field of the LAST column: `/` -> `|`, `.` -> 0, the two digits in ascending order   :114-123
  * a `*` among the alternates splits the record into one 0/1 row per alternate; the `*` row moves one base to
    the left, its REF = that base + the first base of REF, its ALT = that base (one `samtools faidx` per row).
    When `*` is the SECOND alternate it goes first and the other slot takes the first CHARACTER of the ALT
    column -- `alternate[0]`, not `alternate_list[0]` -- as the reference has it                                 :29-55
  * consecutive rows of one position merge into a 1/2 row                                                        :57-71, :127-134
callVarBam --vcf_fn reads the position column of the same rows (callVarBam.py: positions_from_vcf); both walk `expanded_records`.
"""
import shlex
import sys
from argparse import ArgumentParser
from collections import namedtuple
from subprocess import PIPE

VariantInfo = namedtuple('VariantInfo', ['chromosome', 'position', 'reference', 'alternate', 'genotype_1', 'genotype_2'])


def _popen(args, stdin=None, stdout=PIPE):
    from clair_amd.create_tensor import subprocess_popen
    return subprocess_popen(args, stdin=stdin, stdout=stdout)


def base_reader(ref_fn, samtools="samtools"):
    """-> get_base(ctg, position_str): the reference base there (GetTruth.py:18-24), read with `samtools faidx` when samtools is
    on the PATH and through the .fai by the native reader (clair_host_faidx) otherwise."""
    import shutil

    def get_base(ctg, position):
        if ref_fn is None:
            sys.exit("Please provide a reference file correspond to the vcf.")
        if shutil.which(samtools) is None:
            from clair_amd import _hostapi
            seq = _hostapi.faidx(ref_fn, ctg, int(position), int(position))
            return None if seq is None else seq.strip()
        p = _popen(shlex.split("%s faidx %s %s:%s-%s" % (samtools, ref_fn, ctg, position, position)))
        base = None
        for line in p.stdout:
            if line[0] != ">":
                base = line.strip()
                break
        p.stdout.close()
        p.wait()
        return base
    return get_base


def expanded_records(vcf_fn, ctg_name, ctg_start, ctg_end, get_base=None, with_genotype=True):
    """The rows of GetTruth.py:100-127 BEFORE same-position merging, as VariantInfo.  get_base=None leaves the base of a `*` row
    unread (reference and alternate None) and with_genotype=False leaves the last column alone: the position column alone is
    what callVarBam --vcf_fn needs, from a VCF that need not carry genotypes."""
    have_range = ctg_start is not None and ctg_end is not None
    p = _popen(shlex.split("gzip -fdc %s" % vcf_fn))
    for row in p.stdout:
        col = row.strip().split()
        if not col or col[0][0] == "#" or col[0] != ctg_name:
            continue
        position = col[1]
        if have_range and not ctg_start <= int(position) <= ctg_end:
            continue
        reference, alternate = col[3], col[4]
        g1 = g2 = None
        if with_genotype:
            g1, g2 = col[-1].split(":")[0].replace("/", "|").replace(".", "0").split("|")
            if int(g1) > int(g2):
                g1, g2 = g2, g1
        if "*" not in alternate:
            yield VariantInfo(ctg_name, position, reference, alternate, g1, g2)
            continue
        alts = alternate.split(",")
        if len(alts) < 2:
            sys.exit("[ERROR] %s: a lone '*' alternate at %s:%d (the reference's GetTruth cannot read it either)" % (vcf_fn, ctg_name, int(position)))
        if alts[1] == "*":
            alts[0], alts[1] = "*", alternate[0]
        for alt in alts:
            if alt == "*":
                new_pos = str(int(position) - 1)
                new_alt = get_base(ctg_name, new_pos) if get_base is not None else None
                new_ref = None if new_alt is None else new_alt + reference[0]
                yield VariantInfo(ctg_name, new_pos, new_ref, new_alt, "0", "1")
            else:
                yield VariantInfo(ctg_name, position, reference, alt, "0", "1")
    p.stdout.close()
    p.wait()


def merge_infos(info_1, info_2):
    """GetTruth.py:57-71: two rows of one position become one 1/2 row (a row that already has two alleles stays)."""
    if "," in info_1.reference or "," in info_1.alternate:
        return info_1
    if info_1.reference == info_2.reference:
        if info_1.alternate == info_2.alternate:
            return info_1
        return VariantInfo(info_1.chromosome, info_1.position, info_1.reference, "%s,%s" % (info_1.alternate, info_2.alternate), "1", "2")
    if len(info_1.alternate) > len(info_2.alternate):
        info_1, info_2 = info_2, info_1
    new_alternate = "%s,%s" % (info_1.alternate + info_2.reference[len(info_1.reference) - len(info_2.reference):], info_2.alternate)
    return VariantInfo(info_1.chromosome, info_1.position, info_2.reference, new_alternate, "1", "2")


def truth_rows(vcf_fn, ctg_name, ctg_start=None, ctg_end=None, ref_fn=None, samtools="samtools"):
    """The rows GetTruth writes (:127-136), as VariantInfo, in its order."""
    held = None
    for info in expanded_records(vcf_fn, ctg_name, ctg_start, ctg_end, get_base=base_reader(ref_fn, samtools)):
        if held is not None and int(info.position) == int(held.position):
            held = merge_infos(held, info)
        else:
            if held is not None:
                yield held
            held = info
    if held is not None:
        yield held


def output_variant(args):
    if args.var_fn != "PIPE":
        var_fpo = open(args.var_fn, "wb")
        gz = _popen(shlex.split("gzip -c"), stdin=PIPE, stdout=var_fpo)
        out = gz.stdin
    else:
        out = sys.stdout
    for info in truth_rows(args.vcf_fn, args.ctgName, args.ctgStart, args.ctgEnd, args.ref_fn, args.samtools):
        out.write(" ".join(info) + "\n")
    if args.var_fn != "PIPE":
        out.close()
        gz.wait()
        var_fpo.close()
    else:
        out.flush()


def build_parser():
    """Same flags and defaults as GetTruth.py:147-166, plus --samtools."""
    parser = ArgumentParser(description="Extract variant type and allele from a Truth dataset")
    parser.add_argument('--vcf_fn', type=str, default="input.vcf", help="Truth vcf file input, default: %(default)s")
    parser.add_argument('--var_fn', type=str, default="PIPE", help="Truth variants output, use PIPE for standard output, default: %(default)s")
    parser.add_argument('--ref_fn', type=str, default=None, help="Reference file input, must be provided if the vcf contains '*' in ALT field.")
    parser.add_argument('--ctgName', type=str, default="chr17", help="The name of sequence to be processed, default: %(default)s")
    parser.add_argument('--ctgStart', type=int, default=None, help="The 1-based starting position of the sequence to be processed")
    parser.add_argument('--ctgEnd', type=int, default=None, help="The 1-based inclusive ending position of the sequence to be processed")
    # addition of this implementation
    parser.add_argument('--samtools', type=str, default="samtools",
                        help="Path to the 'samtools' that reads the base before a '*' alternate; without it the .fai is read natively, default: %(default)s")
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    output_variant(args)


if __name__ == "__main__":
    main()
