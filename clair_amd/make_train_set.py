"""make_train_set: BAM + truth rows -> a labelled training set, in one process (docs/train_set.md).

    python -m clair_amd.make_train_set --bam_fn a.bam --ref_fn ref.fa --ctgName chr20 --var_fn truth.var --bed_fn confident.bed --set_fn chr20.npz
    python -m clair_amd.train --set_fn chr20.npz --ochk_prefix out/model

Stands behind steps 3-9 of the reference's docs/TRAIN.md: ExtractVariantCandidates --gen4Training, CreateTensor at the truth sites and at
the sampled sites, PairWithNonVariants, and the label join of get_training_array (clair/utils.py:133-220) that Tensor2Bin runs.  With
--front_end device (auto) the tallies, the sampling, the windows, the pairing, the labels and the gather of the kept windows run on the GPU
(clair_frontend_sample_candidates / _build_windows / _pair / _train_set_*); --front_end host runs the sequential host stages and the twin
of the rules (clair_host_train_set_*).  Both write the same bytes.

What differs from the reference: the draws are counter based -- a function of (--seed, contig, position) -- instead of Python's random
stream, so a run is reproducible and runs over differently down-sampled BAMs with one seed sample the same sites wherever the depth
allows; one BAM per run; the candidate rows (--can_fn) are not written.
"""
import gzip
import io
import json
import logging
import shlex
import sys
import zipfile
from argparse import ArgumentParser

import numpy as np

from clair_amd import param, task
from clair_amd.extract_variant_candidates import RATIO_OF_NON_VARIANT_TO_VARIANT

# ExtractVariantCandidates.py:209-214
PLAIN_PROB = 7000000.0 * RATIO_OF_NON_VARIANT_TO_VARIANT / 3000000000
NEAR_PROB = 3500000.0 * 1.0 * RATIO_OF_NON_VARIANT_TO_VARIANT / 14000000
OUTSIDE_PROB = 3500000.0 * RATIO_OF_NON_VARIANT_TO_VARIANT / (3000000000 - 14000000)
ROWS_PER_TAKE = 4096


def probabilities(args):
    """-> (p_near, p_outside) of --sampling, with the overrides"""
    if args.sampling == "plain":
        p_near = p_outside = args.outputProb
    else:
        p_near, p_outside = NEAR_PROB, OUTSIDE_PROB
    return (p_near if args.near_prob is None else args.near_prob), (p_outside if args.outside_prob is None else args.outside_prob)


def truth_rows_of(args):
    """The truth rows of the contig as column lists `ctg pos ref alt g1 g2`, in file order: --var_fn as GetTruth wrote it, or --vcf_fn through
    GetTruth's own code."""
    if args.var_fn is not None:
        from clair_amd.create_tensor import subprocess_popen
        p = subprocess_popen(shlex.split("gzip -fdc %s" % args.var_fn))
        rows = [r.split() for r in p.stdout]
        p.stdout.close()
        p.wait()
        return [c for c in rows if c and c[0] == args.ctgName]
    from clair_amd.get_truth import truth_rows
    return [list(info) for info in truth_rows(args.vcf_fn, args.ctgName, args.ctgStart, args.ctgEnd, args.ref_fn, args.samtools)]


def truth_table(rows):
    """-> (positions int64 ascending, labels uint8 [n,4]): stable by position, so that the last row of a position is the last of its run"""
    positions = np.array([int(c[1]) for c in rows], dtype=np.int64)
    labels = np.array([task.labels_from_vcf_columns(c) for c in rows], dtype=np.uint8).reshape(len(rows), 4)
    order = np.argsort(positions, kind="stable")
    return positions[order], labels[order]


def in_range(positions, args):
    if args.ctgStart is None or args.ctgEnd is None:
        return positions
    return positions[(positions >= args.ctgStart) & (positions <= args.ctgEnd)]


# ---- the two front ends: -> (centres int64 [k], refseq uint8 [k,34], counts int16 [k,33,8,4], labels uint8 [k,4], in_set uint8 [k], stats) ----
def run_host(args, truth, truth_labels, p_near, p_outside, keys):
    """The sequential host stages (clair_host_evc_* with threshold 0, clair_host_pileup_*) and the twin of the rules."""
    from time import time
    from clair_amd import _hostapi, callVarBam as cvb, create_tensor as ct, extract_variant_candidates as evc
    t_start = time()
    seq, ref0, bed = cvb.reference_and_bed(args, True, "[ERROR] Failed to load reference seqeunce from file (%s)." % args.ref_fn)
    have_range = args.ctgStart is not None and args.ctgEnd is not None
    finder = _hostapi.CandidateFinder(args.ctgName, seq, ref0, ctg_start=args.ctgStart if have_range else None, ctg_end=args.ctgEnd if have_range else None,
                                      bed=bed, min_coverage=args.minCoverage, threshold=0.0, min_mq=0)
    view = cvb.alignment_text(args, evc.reference_region(args.ctgName, args.ctgStart if have_range else None, args.ctgEnd if have_range else None)[0])
    chunks = [finder.take_positions() for _ in _hostapi.feed_stream(finder, view.read, 1 << 22)]
    if view.finish() != 0:
        sys.exit("[ERROR] `samtools view` failed on %s" % args.bam_fn)
    eligible = np.concatenate(chunks)
    t_search = time()
    _cls, _draws, sampled, n_near, n_outside = _hostapi.train_set_sample(eligible, truth, p_near, p_outside, keys[0])
    sites = np.union1d(in_range(truth, args), eligible[sampled != 0]).astype(np.int64)
    builder = _hostapi.PileupBuilder(args.ctgName, seq, ref0, sites, consider_left_edge=not args.stop_consider_left_edge, dcov=args.dcov,
                                     min_coverage=int(args.minCoverage), set_order=ct.set_order_of(getattr(args, "pypy", None)))
    view = cvb.alignment_text(args, "%s:%d-%d" % (args.ctgName, args.ctgStart, args.ctgEnd) if have_range else args.ctgName)
    parts = [[], [], []]
    for _ in _hostapi.feed_stream(builder, view.read, 1 << 22):
        while builder.pending():
            for col, piece in zip(parts, builder.take_columns(ROWS_PER_TAKE)):
                col.append(piece)
    if view.finish() != 0:
        sys.exit("[ERROR] `samtools view` failed on %s" % args.bam_fn)
    centres = np.concatenate(parts[0]) if parts[0] else np.zeros(0, np.int64)
    seqs = np.concatenate(parts[1]) if parts[1] else np.zeros((0, 34), np.uint8)
    counts = np.concatenate(parts[2]) if parts[2] else np.zeros((0, 33, 8, 4), np.int32)
    if counts.size and (int(counts.max()) > 32767 or int(counts.min()) < -32768):
        sys.exit("[ERROR] a count beyond int16: the set holds int16 counts")
    t_pileup = time()
    kept, stats = _hostapi.train_set_pair(centres, truth, bed, args.amp, keys[1])
    logging.info("host front end: %d eligible sites, %d windows in %.2f s (candidate search %.2f s, pileup %.2f s)"
                 % (len(eligible), len(centres), t_pileup - t_start, t_search - t_start, t_pileup - t_search))
    centres, seqs, counts = centres[kept], seqs[kept], counts[kept].astype(np.int16)
    labels, in_set = _hostapi.train_set_labels(centres, seqs[:, 16], truth, truth_labels, bed)
    stats.update(in_set=int(in_set.sum()), n_near=n_near, n_outside=n_outside)
    return centres, seqs, counts, labels, in_set, stats


def run_device(args, truth, truth_labels, p_near, p_outside, keys):
    """callVarBam's device front end with the sampling in place of its candidate search -> the same tuple, or None after a logged hand-back."""
    from clair_amd import callVarBam as cvb
    have_range = args.ctgStart is not None and args.ctgEnd is not None
    counted = {}

    def sample(f, bed):
        counted["bed"] = bed
        n, counted["n_near"], counted["n_outside"] = f.sample_candidates(truth, p_near, p_outside, keys[0], min_coverage=args.minCoverage,
                                                                       ctg_start=args.ctgStart if have_range else None,
                                                                       ctg_end=args.ctgEnd if have_range else None, bed=bed, add_truth=True)
        return n

    fe = cvb.DeviceFrontEnd(args, args.device, candidate_step=sample, window_kw=dict(min_coverage=int(args.minCoverage), drop_non_iupac_centre=False))
    try:
        if fe.run() is None:
            return None
        f = fe.frontend
        from time import time
        t0 = time()
        stats = f.pair(truth, truth_labels, args.amp, keys[1], bed=counted["bed"])
        k = stats["kept_var"] + stats["kept_non"]
        parts = [[], [], [], [], []]
        for first in range(0, k, ROWS_PER_TAKE):
            n = min(ROWS_PER_TAKE, k - first)
            for col, piece in zip(parts, f.train_set_info(first, n) + (f.train_set_counts(first, n),)):
                col.append(piece)
        logging.info("device pairing, labels and gather of %d rows: %.2f s" % (k, time() - t0))
    finally:
        fe.close()
    empty = (np.zeros(0, np.int64), np.zeros((0, 34), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(0, np.uint8), np.zeros((0, 33, 8, 4), np.int16))
    centres, seqs, labels, in_set, counts = (np.concatenate(c) if c else e for c, e in zip(parts, empty))
    from clair_amd import _hostapi
    stats.update(r=_hostapi.train_set_ratio(stats["v"], args.amp, stats["c"]), n_near=counted["n_near"], n_outside=counted["n_outside"])
    return centres, seqs, counts, labels, in_set, stats


# ---- the two outputs ------------------------------------------------------------------------------------------------------------------
def write_tensors(path, ctg, centres, seqs, counts):
    """The paired rows as CreateTensor / PairWithNonVariants write them (CreateTensor.py:60-65), gzip without a time stamp."""
    from clair_amd.create_tensor import format_record
    raw = np.ascontiguousarray(seqs).tobytes()
    with open(path, "wb") as fo, gzip.GzipFile(filename="", mode="wb", fileobj=fo, mtime=0) as gz:
        for i, c in enumerate(centres.tolist()):
            gz.write((format_record(ctg, int(c), raw[i * 34:i * 34 + 34].split(b"\0", 1)[0].decode("latin-1"), counts[i]) + "\n").encode("latin-1"))


def save_set(path, arrays):
    """What np.savez_compressed writes -- a zip of deflated .npy members, read back with np.load -- with the members' time stamps fixed, so
    that the same set is the same file."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, allowZip64=True) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def write_set(path, args, centres, seqs, counts, labels, in_set, stats, p_near, p_outside):
    rows = in_set != 0
    meta = dict(seed=args.seed, sampling=args.sampling, p_near=p_near, p_outside=p_outside, amp=args.amp, v=stats["v"], c=stats["c"], r=stats["r"],
                n_near=stats["n_near"], n_outside=stats["n_outside"])
    if args.subsample is not None:              # only then: a set of all the reads is the same file as before the flag existed
        meta.update(subsample=args.subsample, subsample_seed=args.subsample_seed)
    save_set(path, dict(counts=counts[rows], labels=labels[rows], positions=centres[rows],
                        refseq=np.ascontiguousarray(seqs[rows][:, :33]).view("S33").ravel(), ctg=np.array(args.ctgName), meta=np.array(json.dumps(meta, sort_keys=True))))


def load_sets(paths):
    """--set_fn of train / evaluate: the rows of the files, concatenated -> (X float32 [n,33,8,4] (channels 1..3 minus channel 0), keys
    [`ctg:pos`, ...], labels uint8 [n,4]); the first row of a `ctg:pos` wins, as in the text data set -- among the sets of one depth: a set
    made with --subsample FRAC (its meta says so) is keyed by `FRAC:SEED` as well, so that a site stays once per depth it was made at."""
    from clair_amd import _hostapi
    xs, ys, keys, seen = [], [], [], set()
    for path in paths:
        with np.load(path, allow_pickle=False) as z:
            ctg, positions, counts, labels = str(z["ctg"]), z["positions"], z["counts"], z["labels"]
            meta = json.loads(str(z["meta"])) if "meta" in z.files else {}
        tag = "%r:%d" % (float(meta["subsample"]), int(meta.get("subsample_seed", 0))) if "subsample" in meta else ""
        new = np.array([(ctg, int(p), tag) not in seen for p in positions], dtype=bool)
        seen.update((ctg, int(p), tag) for p in positions)
        xs.append(_hostapi.counts_to_input(np.ascontiguousarray(counts[new], dtype=np.int16)).reshape(-1, 33, 8, 4))
        ys.append(labels[new].astype(np.uint8).reshape(-1, 4))
        keys += ["%s:%d" % (ctg, p) for p in positions[new]]
    if not xs:
        return np.zeros((0, 33, 8, 4), np.float32), [], np.zeros((0, 4), np.uint8)
    return np.concatenate(xs, axis=0), keys, np.concatenate(ys, axis=0)


def set_batches(paths, batch_size):
    """load_sets as evaluate.labelled_batches yields it"""
    X, keys, labels = load_sets(paths)
    for at in range(0, len(X), batch_size):
        yield X[at:at + batch_size], keys[at:at + batch_size], labels[at:at + batch_size]


def build_parser():
    parser = ArgumentParser(description="Sample, pair and label the training sites of one contig: BAM + truth -> training set")
    add = parser.add_argument
    add('--bam_fn', type=str, default="input.bam", help="sorted alignments, default: %(default)s")
    add('--ref_fn', type=str, default="ref.fa", help="reference FASTA with its .fai, default: %(default)s")
    add('--ctgName', type=str, default=None, help="contig to process (required)")
    add('--ctgStart', type=int, default=None, help="1-based first position of the region")
    add('--ctgEnd', type=int, default=None, help="1-based last position of the region (inclusive)")
    add('--var_fn', type=str, default=None, help="truth rows `ctg pos ref alt g1 g2` as GetTruth writes them")
    add('--vcf_fn', type=str, default=None, help="truth VCF, read as GetTruth reads it (in place of --var_fn)")
    add('--bed_fn', type=str, default=None, help="BED file of the regions whose sites are sampled and make the data set")
    add('--minCoverage', type=float, default=4, help="minimum depth of a sampled site and of a window's centre, default: %(default)s")
    add('--dcov', type=int, default=250, help="at most this many reads per start position, default: %(default)s")
    add('--stop_consider_left_edge', action='store_true', help="open a window only for reads that cover its left edge")
    add('--sampling', type=str, default="plain", choices=("plain", "near_variant"),
        help="plain: every eligible site with --outputProb; near_variant: sites 15 or 16 from their nearest truth site with %g, every other one "
             "with %g, default: %%(default)s" % (NEAR_PROB, OUTSIDE_PROB))
    add('--outputProb', type=float, default=PLAIN_PROB, help="probability of a site with --sampling plain, default: %(default)s")
    add('--near_prob', type=float, default=None, help="probability of a site near a truth site, in place of the mode's")
    add('--outside_prob', type=float, default=None, help="probability of every other site, in place of the mode's")
    add('--amp', type=float, default=2, help="keep (truth windows * amp) non-variant windows, default: %(default)s")
    add('--seed', type=int, default=param.RANDOM_SEED if param.RANDOM_SEED is not None else 0, help="seed of the draws, default: %(default)s")
    add('--tensor_fn', type=str, default=None, help="output: the paired rows as CreateTensor writes them, gzip")
    add('--set_fn', type=str, default=None, help="output: the rows of the data set with their labels, .npz (train / evaluate --set_fn)")
    add('--front_end', type=str, default="auto", choices=("auto", "device", "host"),
        help="where the tallies, the sampling, the windows, the pairing and the labels are made: on the GPU (auto = device, handing back to the "
             "host stages, with a message, where the device formulation does not reproduce them exactly) or on the host")
    add('--bam_reader', type=str, default="samtools", choices=("samtools", "native"), help="how the alignments and the reference slice are read")
    add('--bam_threads', type=int, default=4, help="with --bam_reader native: threads that inflate BGZF blocks (1 .. 16), default: %(default)s")
    add('--subsample', type=float, default=None, metavar="FRAC",
        help="make the set from this fraction of the BAM's reads (0 < FRAC <= 1), chosen by read name as `samtools view -s` chooses them, in the "
             "native reader's view: one run per depth, no down-sampled copy on disk (needs --bam_reader native; docs/subsample.md)")
    add('--subsample_seed', type=int, default=0, metavar="INT", help="the 32-bit word the read name's hash is XORed with, default: %(default)s")
    add('--samtools', type=str, default="samtools", help="samtools executable")
    add('--device', type=int, default=0, help="HIP device ordinal, default: %(default)s")
    # what callVarBam's front end reads from its options and this module does not offer
    parser.set_defaults(threshold=0.0, view_readers=1, samtools_threads=0, samtools_view_args=None, bam_inflate="host", indel_lookup="pysam", pypy=None)
    return parser


def Run(args):
    if args.ctgName is None:
        sys.exit("--ctgName must be specified.")
    if args.tensor_fn is None and args.set_fn is None:
        sys.exit("[ERROR] nothing to write: give --tensor_fn, --set_fn or both")
    if (args.var_fn is None) == (args.vcf_fn is None):
        sys.exit("[ERROR] the truth comes from --var_fn (GetTruth's rows) or from --vcf_fn: give one of the two")
    if (args.ctgStart is None) != (args.ctgEnd is None) or (args.ctgStart is not None and args.ctgStart > args.ctgEnd):
        args.ctgStart = args.ctgEnd = None
    if args.subsample is not None or args.subsample_seed:
        from clair_amd import callVarBam as cvb
        if args.subsample is not None:
            cvb.check_subsample_fraction("--subsample", args.subsample, args.subsample_seed)
        cvb.check_subsample_fraction("--subsample_seed", 1.0, args.subsample_seed)
        if not cvb.native_input(args):
            sys.exit("[ERROR] --subsample and --subsample_seed select reads in the native reader's view: add --bam_reader native")
    from clair_amd import _hostapi
    truth, truth_labels = truth_table(truth_rows_of(args))
    args.vcf_fn = None          # from here on the options are the front end's, where --vcf_fn means "windows at these sites only"
    p_near, p_outside = probabilities(args)
    keys = (_hostapi.train_set_key(args.ctgName, args.seed, _hostapi.TS_STAGE_SAMPLE), _hostapi.train_set_key(args.ctgName, args.seed, _hostapi.TS_STAGE_PAIR))
    out = None
    if args.front_end != "host":
        out = run_device(args, truth, truth_labels, p_near, p_outside, keys)
    if out is None:
        out = run_host(args, truth, truth_labels, p_near, p_outside, keys)
    centres, seqs, counts, labels, in_set, stats = out
    if args.sampling == "near_variant":
        logging.info("# of candidates near variant: %d" % stats["n_near"])
        logging.info("# of candidates outside variant: %d" % stats["n_outside"])
    logging.info("%d Truth Variants" % stats["v"])
    logging.info("%d non-variants to be picked" % (stats["v"] * args.amp))
    logging.info("%d usable non-variant" % stats["c"])
    logging.info("%.2f of all non-variants are selected" % stats["r"])
    logging.info("%.2f/%.2f Truth Variants/Non-variants outputed" % (stats["kept_var"], stats["kept_non"]))
    logging.info("%d rows make the data set" % stats["in_set"])
    if args.tensor_fn is not None:
        write_tensors(args.tensor_fn, args.ctgName, centres, seqs, counts)
    if args.set_fn is not None:
        write_set(args.set_fn, args, centres, seqs, counts, labels, in_set, stats, p_near, p_outside)


def main(argv=None):
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 0:
        parser.print_help()
        sys.exit(1)
    Run(parser.parse_args(argv))


if __name__ == "__main__":
    main()
