"""PairWithNonVariants: thin the non-variant tensors against the variant ones (dataPrepScripts/PairWithNonVariants.py), a text filter.

    python -m clair_amd PairWithNonVariants --tensor_can_fn can.gz --tensor_var_fn var.gz --bed_fn confident.bed --output_fn paired.gz --amp 2

Same flags, same log lines, same output order (every variant row, then the kept non-variant rows in file order) as the reference
(PairWithNonVariants.py:17-90).  A non-variant row is usable when its position, as it stands in the file, lies in the 0-based bed
intervals (the reference's off-by-one, see clair_amd.evaluate) and no variant row has its `ctg-pos`; r = min(1, v amp / c).  What differs: a
usable row is kept when the counter-based draw of (--seed, contig, position) is below r (csrc/train_set_core.h, through the host twin
clair_host_train_set_*) instead of `random() < r`, and with no usable row r is 1 where the reference divides by zero.
clair_amd.make_train_set does the same pairing over windows that never become text.
"""
import gzip
import logging
import shlex
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import param


def positions_by_contig(path):
    """-> ({ctg: [pos, ...]} in file order, number of rows)"""
    from clair_amd.create_tensor import subprocess_popen
    p = subprocess_popen(shlex.split("gzip -fdc %s" % path))
    out, n = {}, 0
    for row in p.stdout:
        col = row.split(None, 2)
        if len(col) < 2:
            continue
        out.setdefault(col[0], []).append(int(col[1]))
        n += 1
    p.stdout.close()
    p.wait()
    return out, n


def Run(args):
    from clair_amd import _hostapi
    from clair_amd.create_tensor import subprocess_popen
    from clair_amd.extract_variant_candidates import bed_regions_from
    bed = bed_regions_from(args.bed_fn)

    logging.info("Counting the number of Truth Variants in %s ..." % args.tensor_var_fn)
    variants, v = positions_by_contig(args.tensor_var_fn)
    logging.info("%d Truth Variants" % v)
    logging.info("%d non-variants to be picked" % (v * args.amp))

    logging.info("Counting the number of usable non-variants in %s ..." % args.tensor_can_fn)
    candidates, _ = positions_by_contig(args.tensor_can_fn)
    truth = {ctg: np.unique(np.array(variants.get(ctg, []), dtype=np.int64)) for ctg in candidates}
    # (a contig the bed file does not name has no usable row: is_region_in is False there)
    bed_of = {ctg: None if bed is None else bed.get(ctg, []) for ctg in candidates}
    c = sum(_hostapi.train_set_pair_count(pos, truth[ctg], bed_of[ctg])[1] for ctg, pos in candidates.items())
    logging.info("%d usable non-variant" % c)
    r = _hostapi.train_set_ratio(v, args.amp, c)
    logging.info("%.2f of all non-variants are selected" % r)

    keep = {}
    for ctg, pos in candidates.items():
        kept, n_var = _hostapi.train_set_pair_keep(pos, truth[ctg], bed_of[ctg], r, _hostapi.train_set_key(ctg, args.seed, _hostapi.TS_STAGE_PAIR))
        flags = np.zeros(len(pos), dtype=bool)
        flags[kept[n_var:]] = True          # (rows at a variant's position are the variant file's to write)
        keep[ctg] = iter(flags.tolist())

    o1 = o2 = 0
    with open(args.output_fn, "wb") as fo, gzip.GzipFile(filename="", mode="wb", fileobj=fo, mtime=0) as out:
        p = subprocess_popen(shlex.split("gzip -fdc %s" % args.tensor_var_fn))
        for row in p.stdout:
            out.write((row.strip() + "\n").encode("latin-1"))
            o1 += 1
        p.stdout.close()
        p.wait()
        p = subprocess_popen(shlex.split("gzip -fdc %s" % args.tensor_can_fn))
        for row in p.stdout:
            col = row.split(None, 2)
            if len(col) < 2:
                continue
            if next(keep[col[0]]):
                out.write((row.strip() + "\n").encode("latin-1"))
                o2 += 1
        p.stdout.close()
        p.wait()
    logging.info("%.2f/%.2f Truth Variants/Non-variants outputed" % (o1, o2))


def build_parser():
    """Same flags and defaults as PairWithNonVariants.py:94-110, plus --seed."""
    parser = ArgumentParser(description="Pair the truth-variant tensors with a share of the non-variant tensors")
    parser.add_argument('--tensor_can_fn', type=str, default=None, help="tensors at the sampled sites (make_train_set / CreateTensor)")
    parser.add_argument('--tensor_var_fn', type=str, default=None, help="tensors at the truth sites (GetTruth + CreateTensor)")
    parser.add_argument('--bed_fn', type=str, default=None, help="usable genome regions in the BED format")
    parser.add_argument('--output_fn', type=str, default=None, help="tensors output, gzip")
    parser.add_argument('--amp', type=float, default=2, help="keep (truth variants * amp) non-variants, default: %(default)s")
    # addition of this implementation
    parser.add_argument('--seed', type=int, default=param.RANDOM_SEED if param.RANDOM_SEED is not None else 0, help="seed of the draws, default: %(default)s")
    return parser


def main():
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    if args.tensor_can_fn is None or args.tensor_var_fn is None or args.output_fn is None:
        sys.exit("[ERROR] --tensor_can_fn, --tensor_var_fn and --output_fn are required")
    Run(args)


if __name__ == "__main__":
    main()
