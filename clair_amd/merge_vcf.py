"""merge_vcf: the per-chunk VCFs of callVarBamParallel as ONE sorted VCF, bgzipped and tabix-indexed.

The last line of the reference's whole-genome recipe (README.md:299-303, docs/POST_PROCESSING.md step 5) without vcflib, bcftools and htslib:

    python -m clair_amd.merge_vcf --output_prefix out/var --ref_fn ref.fa --merged_fn snp_and_indel.vcf.gz
          [--overlap_filter off|python|host|device] [--bgzf_deflate zlib|host|device] [--device N] [--threads N] [FILE ...]

  * inputs: the FILEs, or every <prefix>.<contig>_<start>_<end>.vcf that exists (the name is read from the right: contigs contain '_' and '.');
  * order: contig rank in <ref>.fai, then start (chr2 before chr10); a contig the .fai does not have is an error;
  * a non-empty file that does not end in a line end is the reference's "incomplete VCF" (`tail -c 1`): every such file is named, exit 1;
  * the header rows are the first file's; every other file's must equal them;
  * rows by (contig rank, POS), stable: a concatenation for disjoint chunks in order, a stable sort otherwise;
  * --overlap_filter: one walk of clair_amd.overlap_variant over the merged rows, which also sees the pairs that straddle two chunks;
  * --merged_fn *.gz is written as BGZF (clair_amd.bgzf) with <merged_fn>.tbi (clair_amd.tabix); any other name as plain text.
docs/merge_vcf.md has the rules and the measurements."""
import logging
import os
import sys
from argparse import ArgumentParser
from time import time

from clair_amd import bgzf, overlap_variant

FILTERS = ("off",) + overlap_variant.BACKENDS


def contig_ranks(ref_fn):
    fai = ref_fn + ".fai"
    if not os.path.isfile(fai):
        sys.exit("[ERROR] file %s not found" % fai)
    ranks = {}
    with open(fai) as f:
        for row in f:
            name = row.rstrip("\n").split("\t")[0]
            if name:
                ranks.setdefault(name, len(ranks))
    return ranks


def chunk_of(stem, ranks):
    """`<anything>.<contig>_<start>_<end>` or `<contig>_<start>_<end>` -> (contig, start, end), None when it is no such name."""
    parts = stem.rsplit("_", 2)
    if len(parts) != 3 or not parts[1].isdigit() or not parts[2].isdigit():
        return None
    best = None
    for name in ranks:
        if (parts[0] == name or parts[0].endswith("." + name)) and (best is None or len(name) > len(best)):
            best = name
    return None if best is None else (best, int(parts[1]), int(parts[2]))


def find_inputs(output_prefix, ranks):
    """Every <prefix>.<contig>_<start>_<end>.vcf that exists -> [(rank, start, path)]; a chunk name with a contig outside the .fai is an error."""
    folder, base = os.path.split(os.path.abspath(output_prefix))
    found = []
    for name in sorted(os.listdir(folder)) if os.path.isdir(folder) else []:
        if not (name.startswith(base + ".") and name.endswith(".vcf")):
            continue
        middle = name[len(base) + 1:-4]
        parts = middle.rsplit("_", 2)
        if len(parts) != 3 or not parts[1].isdigit() or not parts[2].isdigit():
            continue
        if parts[0] not in ranks:
            sys.exit("[ERROR] %s: contig %s is not in the .fai" % (os.path.join(folder, name), parts[0]))
        found.append((ranks[parts[0]], int(parts[1]), os.path.join(folder, name)))
    return found


def order_inputs(files, ranks):
    keyed = []
    for path in files:
        if not os.path.isfile(path):
            sys.exit("[ERROR] file %s not found" % path)
        name = os.path.basename(path)
        chunk = chunk_of(name[:-4] if name.endswith(".vcf") else name, ranks)
        if chunk is None:
            sys.exit("[ERROR] %s: not a chunk name <prefix>.<contig>_<start>_<end>.vcf with a contig of the .fai" % path)
        keyed.append((ranks[chunk[0]], chunk[1], path))
    return keyed


def merge_texts(paths, ranks):
    """-> (header text, rows [str without line end], keys [(rank, pos)], bytes in).  Exits on an incomplete file or a differing header."""
    texts, incomplete = [], []
    for path in paths:
        with open(path, "rb") as f:
            data = f.read()
        if data and not data.endswith(b"\n"):
            incomplete.append(path)
        texts.append(data)
    if incomplete:
        sys.exit("[ERROR] incomplete VCF (no line end at the end of the file): %s" % " ".join(incomplete))
    header, rows, keys, first = None, [], [], None
    for path, data in zip(paths, texts):
        if not data:
            continue
        lines = data.decode("latin-1").split("\n")
        lines.pop()
        k = 0
        while k < len(lines) and lines[k].startswith("#"):
            k += 1
        mine = "".join(line + "\n" for line in lines[:k])
        if header is None:
            header, first = mine, path
        elif mine != header:
            sys.exit("[ERROR] %s: its header rows differ from those of %s" % (path, first))
        for n, row in enumerate(lines[k:]):
            col = row.split("\t", 2)
            if len(col) < 3 or not col[1].isdigit():
                sys.exit("[ERROR] %s: row %d is not a VCF row" % (path, k + n + 1))
            if col[0] not in ranks:
                sys.exit("[ERROR] %s: contig %s is not in the .fai" % (path, col[0]))
            rows.append(row)
            keys.append((ranks[col[0]], int(col[1])))
    return header or "", rows, keys, sum(len(t) for t in texts)


def sort_rows(rows, keys):
    """Rows by (contig rank, POS), stable; untouched when they already are."""
    import numpy as np
    if len(rows) < 2:
        return rows, keys, False
    k = np.array(keys, dtype=np.int64)
    flat = k[:, 0] << 40 | k[:, 1]
    if bool(np.all(flat[1:] >= flat[:-1])):
        return rows, keys, False
    order = np.argsort(flat, kind="stable")
    return [rows[i] for i in order], [keys[i] for i in order], True


def write_merged(args, header, rows):
    """-> bytes written (index included)."""
    text_rows = [row + "\n" for row in rows]
    if not args.merged_fn.endswith(".gz"):
        with open(args.merged_fn, "w", newline="") as f:
            f.write(header)
            f.writelines(text_rows)
        return len(header) + sum(map(len, text_rows))
    from clair_amd import tabix
    writer = bgzf.BgzfWriter(args.merged_fn, deflate=args.bgzf_deflate, device=args.device, threads=args.threads)
    writer.write(header.encode("latin-1"))
    writer.write("".join(text_rows).encode("latin-1"))
    writer.close()
    present, records, at = {}, [], len(header)
    for row in text_rows:
        col = row.split("\t", 4)
        tid = present.setdefault(col[0], len(present))
        records.append((tid, int(col[1]), len(col[3]), at, at + len(row)))
        at += len(row)
    # the index is a few KiB: the host twin writes the bytes the device would (same compressor), without a second device handle
    tabix.write_tbi(args.merged_fn + ".tbi", list(present), records, writer.virtual_offset,
                    deflate="host" if args.bgzf_deflate == "device" else args.bgzf_deflate, threads=args.threads)
    return writer.compressed_bytes + os.path.getsize(args.merged_fn + ".tbi")


def build_parser():
    parser = ArgumentParser(description="Merge the per-chunk VCFs of callVarBamParallel into one sorted VCF; *.gz is written as BGZF with a tabix index")
    add = parser.add_argument
    add('--output_prefix', type=str, default=None, help="the --output_prefix the chunks were called with: <prefix>.<contig>_<start>_<end>.vcf are the inputs")
    add('--ref_fn', type=str, default="ref.fa", help="reference FASTA: its .fai gives the order of the contigs")
    add('--merged_fn', type=str, default=None, help="output; a name ending in .gz is BGZF-compressed and gets <name>.tbi")
    add('--overlap_filter', type=str, default="off", choices=FILTERS,
        help="the merged rows through the overlap filter (who walks them: this module, the host library or the GPU), default: %(default)s")
    add('--bgzf_deflate', type=str, default="host", choices=bgzf.BACKENDS,
        help="who compresses the BGZF blocks: zlib, the host twin of the device compressor, or the GPU, default: %(default)s")
    add('--device', type=int, default=0, help="HIP device ordinal of the device backends, default: %(default)s")
    add('--threads', type=int, default=4, help="blocks --bgzf_deflate host compresses side by side, default: %(default)s")
    add('files', nargs='*', metavar="FILE", help="the chunk VCFs, in any order (default: every chunk of --output_prefix that exists)")
    return parser


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        sys.exit(1)
    args = parser.parse_args(argv)
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    if args.merged_fn is None:
        sys.exit("[ERROR] --merged_fn is required")
    if not args.files and args.output_prefix is None:
        sys.exit("[ERROR] --output_prefix or FILEs are required")
    t0 = time()
    ranks = contig_ranks(args.ref_fn)
    keyed = order_inputs(args.files, ranks) if args.files else find_inputs(args.output_prefix, ranks)
    if not keyed:
        sys.exit("[ERROR] no chunk VCF found for %s" % (args.output_prefix if not args.files else "the given names"))
    keyed.sort(key=lambda k: (k[0], k[1]))       # stable: equal chunks keep the order they were given in
    paths = [k[2] for k in keyed]
    header, rows, keys, bytes_in = merge_texts(paths, ranks)
    rows, keys, was_sorted = sort_rows(rows, keys)
    rows_in = len(rows)
    try:
        if args.overlap_filter != "off":
            text = overlap_variant.filter_vcf_text(header + "".join(row + "\n" for row in rows), args.overlap_filter, args.device)
            lines = text.split("\n")
            lines.pop()
            header = "".join(line + "\n" for line in lines if line.startswith("#"))
            rows = [line for line in lines if not line.startswith("#")]
        bytes_out = write_merged(args, header, rows)
    except (RuntimeError, ValueError) as exc:    # the device library's errors (no GPU, no library), a POS beyond .tbi: a message and a non-zero exit
        sys.exit("[ERROR] %s" % exc)
    logging.info("[INFO] merge_vcf: %d file(s), %d row(s) in%s, %d dropped by the overlap filter, %d bytes in, %d bytes out, %.2f s -> %s" % (
        len(paths), rows_in, " (sorted)" if was_sorted else "", rows_in - len(rows), bytes_in, bytes_out, time() - t0, args.merged_fn))
    return 0


if __name__ == "__main__":
    main()
