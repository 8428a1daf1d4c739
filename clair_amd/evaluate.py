"""evaluate: score a checkpoint against truth labels (clair/evaluate.py), the scoring on the device.

    python -m clair_amd GetTruth --vcf_fn truth.vcf.gz --ref_fn ref.fa --ctgName chr20 --var_fn truth.var
    python -m clair_amd evaluate --chkpnt_fn model --tensor_fn tensors.gz --var_fn truth.var [--bed_fn confident.bed]
    python -m clair_amd evaluate --chkpnt_fn model --set_fn chr20.npz [--set_fn chr21.npz]      (sets of clair_amd.make_train_set)

The data set is the one clair/utils.py:133-220 (get_training_array) builds from text, streamed instead of held:
  * bed filter as written there -- is_region_in(tree, chrom, int(coord)): membership of the position number AS IT STANDS IN THE
    FILE (1-based) in the 0-based half-open bed intervals, for truth rows (:122) and tensors (:145) alike.  The reference's
    off-by-one is kept: the 1-based site p is looked up as if it were 0-based, so the base BEFORE an interval counts as inside
    it and its last base as outside;
  * sequence upper-cased, centre base in ACGTU (:147-149); the first tensor of a `ctg:pos` wins (:156);
  * channels 1..3 minus channel 0 (:152-154);
  * label from --var_fn (the last row of a key wins, :125-126), else the homozygous-reference label of the centre base (:168-170).
Shuffling does not change counts and is not done.  The text goes through the native tensor reader (clair_amd.utils), which keeps
records whose centre is an upper-case IUPAC letter: a record with a LOWER-case centre base, which get_training_array would upper-case
and keep, is dropped here (CreateTensor of either project writes upper-case sequences).

Scoring (evaluate.py:87-129) runs behind the forward pass on the device (--score_on device: clair_submit_eval, only the 2 631
counters come back) or in NumPy on downloaded probabilities (--score_on host: evaluate_counts_host, the twin of the kernel).
Counter layout and tie rule: include/clair_amd.h (clair_eval_*), docs/evaluate.md.  The report is the reference's stdout
(:136-163).  The blosc/pickle binaries (--bin_fn, --train_bin_fn, --validation_bin_fn) need the `blosc` module and are not read.
"""
import os
import shlex
import sys
from argparse import ArgumentParser

import numpy as np

from clair_amd import param, task
from clair_amd._capi import EVAL_COUNTS

# counter block: name -> (offset, rows); matrices are row-major [true][predicted]
LAYOUT = (("gt21", 3, 21), ("genotype", 3 + 441, 3), ("len1", 3 + 441 + 9, 33), ("len2", 3 + 441 + 9 + 1089, 33))
assert LAYOUT[-1][1] + 33 * 33 == EVAL_COUNTS


def split_counts(counts):
    """int64 [EVAL_COUNTS] -> dict(all, top1, top2, gt21 [21,21], genotype [3,3], len1 [33,33], len2 [33,33])."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.shape != (EVAL_COUNTS,):
        raise ValueError("counter block must have %d elements, got shape %r" % (EVAL_COUNTS, counts.shape))
    out = {"all": int(counts[0]), "top1": int(counts[1]), "top2": int(counts[2])}
    for name, offset, size in LAYOUT:
        out[name] = counts[offset:offset + size * size].reshape(size, size)
    return out


def evaluate_counts_host(probabilities, labels):
    """The NumPy twin of eval_kernel (clair_amd/csrc/evaluate.hip.h): evaluate.py:87-129 on probabilities [n,90] (or the list
    [gt21, genotype, len1, len2]) and true indices uint8 [n,4] -> int64 [EVAL_COUNTS].  arg-max = lowest index among equals; the
    true class is first / second in DESCENDING probability, then DESCENDING index."""
    if isinstance(probabilities, (list, tuple)):
        probabilities = np.concatenate([np.asarray(a, dtype=np.float32) for a in probabilities], axis=1)
    P = np.asarray(probabilities, dtype=np.float32)
    lab = np.asarray(labels)
    n = P.shape[0]
    if P.shape != (n, 90) or lab.shape != (n, 4):
        raise ValueError("probabilities [n,90] and labels [n,4] expected, got %r and %r" % (P.shape, lab.shape))
    lab = lab.astype(np.int64)
    if n and ((lab < 0).any() or (lab >= np.array([21, 3, 33, 33])).any()):
        raise ValueError("label out of range: gt21 < 21, genotype < 3, lengths < 33")
    counts = np.zeros(EVAL_COUNTS, dtype=np.int64)
    if n == 0:
        return counts
    rows = np.arange(n)
    gt21 = P[:, 0:21]
    true = lab[:, 0]
    p_true = gt21[rows, true][:, None]
    ahead = ((gt21 > p_true) | ((gt21 == p_true) & (np.arange(21)[None, :] > true[:, None]))).sum(axis=1)
    counts[0] = n
    counts[1] = int((ahead == 0).sum())
    counts[2] = int((ahead <= 1).sum())
    np.add.at(counts, 3 + true * 21 + np.argmax(gt21, axis=1), 1)
    np.add.at(counts, LAYOUT[1][1] + lab[:, 1] * 3 + np.argmax(P[:, 21:24], axis=1), 1)
    p1, p2 = np.argmax(P[:, 24:57], axis=1), np.argmax(P[:, 57:90], axis=1)
    np.add.at(counts, LAYOUT[2][1] + np.minimum(lab[:, 2], lab[:, 3]) * 33 + np.minimum(p1, p2), 1)
    np.add.at(counts, LAYOUT[3][1] + np.maximum(lab[:, 2], lab[:, 3]) * 33 + np.maximum(p1, p2), 1)
    return counts


def f1_score(confusion_matrix):
    """evaluate.py:18-31 in float64."""
    m = np.asarray(confusion_matrix)
    column_sum, row_sum = m.sum(axis=0), m.sum(axis=1)
    epsilon = 1e-15
    out = np.array([])
    for i in range(m.shape[0]):
        tp = m[i][i] + 0.0
        precision = tp / (column_sum[i] + epsilon)
        recall = tp / (row_sum[i] + epsilon)
        out = np.append(out, (2.0 * precision * recall) / (precision + recall + epsilon))
    return out


def report_lines(counts):
    """The reference's stdout (evaluate.py:136-163), one string per print()."""
    c = split_counts(counts)
    if c["all"] == 0:
        raise ValueError("no candidate was scored")
    lines = ["[INFO] Evaluation on gt21:",
             "[INFO] all/top1/top2/top1p/top2p: %d/%d/%d/%.2f/%.2f" % (c["all"], c["top1"], c["top2"], float(c["top1"]) / c["all"] * 100,
                                                                     float(c["top2"]) / c["all"] * 100)]
    for name, title in (("gt21", None), ("genotype", "\n[INFO] Evaluation on Genotype:"), ("len1", "\n[INFO] evaluation on indel length 1:"),
                        ("len2", "\n[INFO] evaluation on indel length 2:")):
        if title:
            lines.append(title)
        for row in c[name]:
            lines.append("\t".join(str(v) for v in row))
        lines.append("[INFO] f-measure:  %s" % (f1_score(c[name]),))      # print("[INFO] f-measure: ", array): two arguments, one space between
    return lines


# ---- the data set ---------------------------------------------------------------------------------------------------------------
def bed_tree_from(bed_fn):
    """shared/interval_tree.py:7-39 -> {ctg: BedRegions}; empty without a bed file (then nothing is filtered, utils.py:135)."""
    from clair_amd.extract_variant_candidates import BedRegions, bed_regions_from
    return {ctg: BedRegions(iv) for ctg, iv in (bed_regions_from(bed_fn) or {}).items()}


def is_region_in(tree, ctg, position):
    return ctg in tree and position in tree[ctg]


def variant_map_from(var_fn, tree):
    """clair/utils.py:112-130: `ctg:pos` -> true indices of the truth rows inside the bed regions."""
    from clair_amd.create_tensor import subprocess_popen
    labels = {}
    if var_fn is None:
        return labels
    p = subprocess_popen(shlex.split("gzip -fdc %s" % var_fn))
    for row in p.stdout:
        columns = row.split()
        if not columns:
            continue
        if tree and not is_region_in(tree, columns[0], int(columns[1])):
            continue
        labels[columns[0] + ":" + columns[1]] = task.labels_from_vcf_columns(columns)
    p.stdout.close()
    p.wait()
    return labels


def labelled_batches(tensor_fn, var_fn, bed_fn, batch_size):
    """get_training_array (clair/utils.py:133-220) as a stream: yields (X float32 [m,33,8,4], keys [`ctg:pos`, ...], labels uint8
    [m,4]) for the tensors that make the data set, m <= batch_size, in file order."""
    import contextlib
    from clair_amd import utils
    tree = bed_tree_from(bed_fn)
    truth = variant_map_from(var_fn, tree)
    seen = set()
    devnull = open(os.devnull, "w")
    generator = utils.tensor_generator_from(tensor_fn, batch_size)
    while True:
        with contextlib.redirect_stderr(devnull):      # the reader's per-batch progress lines belong to call_var
            item = next(generator, None)
        if item is None:
            break
        X, infos = item
        keep, keys, labels = [], [], []
        for i, (ctg, pos, seq) in enumerate(infos):
            if tree and not is_region_in(tree, ctg, int(pos)):
                continue
            centre = seq.upper()[param.flankingBaseNum]
            if centre not in task.BASIC_BASES:
                continue
            key = ctg + ":" + pos
            if key in seen:
                continue
            seen.add(key)
            keep.append(i)
            keys.append(key)
            labels.append(truth[key] if key in truth else task.labels_from_reference(task.IUPAC_TO_ACGT[centre]))
        if keep:
            yield (X if len(keep) == len(X) else X[keep]), keys, np.array(labels, dtype=np.uint8).reshape(len(keep), 4)
    devnull.close()


def evaluate_counts(m, batches, score_on="device"):
    """Run the batches through the engine, pipelined over its slots as call_var does, -> (counter block int64 [EVAL_COUNTS], n)."""
    engine, n_slots = m.engine, m.n_slots
    device = score_on == "device"
    counts = np.zeros(EVAL_COUNTS, dtype=np.int64)
    if device:
        engine.eval_reset()
    inflight, total = [], 0

    def finish(slot, labels):
        prediction = m.wait(slot)
        if not device:
            counts[:] += evaluate_counts_host(prediction, labels)

    for k, (X, _keys, labels) in enumerate(batches):
        slot = k % n_slots
        if len(inflight) == n_slots:
            finish(*inflight.pop(0))
        if device:
            engine.submit_eval(slot, X, labels)
        else:
            m.submit(slot, X)
        inflight.append((slot, labels))
        total += len(labels)
    while inflight:
        finish(*inflight.pop(0))
    return (engine.eval_read() if device else counts), total


def build_parser():
    """Same flags and defaults as evaluate.py:166-186, plus --batch_size / --device / --score_on."""
    parser = ArgumentParser(description="Evaluate trained model")
    parser.add_argument('--bin_fn', type=str, default=None,
                        help="Binary tensor input generated by tensor2Bin.py, tensor_fn, var_fn and bed_fn will be ignored")
    parser.add_argument('--train_bin_fn', type=str, default=None,
                        help="Train Binary, used together with --validation_bin_fn (would ignore: bin_fn, tensor_fn, var_fn, bed_fn)")
    parser.add_argument('--validation_bin_fn', type=str, default=None,
                        help="Validation Binary, used together with --train_bin_fn (would ignore: bin_fn, tensor_fn, var_fn, bed_fn)")
    parser.add_argument('--tensor_fn', type=str, default="vartensors", help="Tensor input")
    parser.add_argument('--var_fn', type=str, default="truthvars", help="Truth variants list input")
    parser.add_argument('--bed_fn', type=str, default=None, help="High confident genome regions input in the BED format")
    parser.add_argument('--chkpnt_fn', type=str, default=None, help="Input a checkpoint for testing, REQUIRED")
    # additions of this implementation
    parser.add_argument('--batch_size', type=int, default=None, help="Candidates per forward pass, default: %d" % param.engineBatchSize)
    parser.add_argument('--device', type=int, default=0, help="HIP device ordinal, default: %(default)s")
    parser.add_argument('--set_fn', type=str, action='append', default=None, metavar="NPZ",
                        help="Training set written by make_train_set --set_fn, repeatable (the rows are concatenated); tensor_fn, var_fn and bed_fn "
                             "will be ignored")
    parser.add_argument('--score_on', type=str, default="device", choices=("device", "host"),
                        help="Where the confusion counters are accumulated: behind the forward pass on the device, or in NumPy on "
                             "downloaded probabilities, default: %(default)s")
    return parser


BINARY_MESSAGE = ("[ERROR] --bin_fn / --train_bin_fn / --validation_bin_fn: the blosc/pickle binaries need the `blosc` module, which this build "
                  "does not read; evaluate from text with --tensor_fn and --var_fn.")


def main():
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    if args.bin_fn is not None or args.train_bin_fn is not None or args.validation_bin_fn is not None:
        sys.exit(BINARY_MESSAGE)
    if args.chkpnt_fn is None:
        sys.exit("[ERROR] --chkpnt_fn is required")
    print("[INFO] Loading model ...", file=sys.stderr)
    from clair_amd.model import Clair
    batch = args.batch_size or param.engineBatchSize
    try:
        m = Clair(device=args.device, max_batch=batch, n_slots=param.pipeline_slots())
        m.init()
        m.restore_parameters(os.path.abspath(args.chkpnt_fn))
    except Exception as exc:   # C-ABI errors surface as messages + non-zero exit
        sys.exit("[ERROR] %s" % exc)
    try:
        print("[INFO] Loading dataset...", file=sys.stderr)
        print("[INFO] Testing on the training and validation dataset ...", file=sys.stderr)
        if args.set_fn:
            from clair_amd.make_train_set import set_batches
            batches = set_batches(args.set_fn, batch)
        else:
            batches = labelled_batches(args.tensor_fn, args.var_fn, args.bed_fn, batch)
        counts, total = evaluate_counts(m, batches, args.score_on)
        print("[INFO] The size of dataset: %d" % total, file=sys.stderr)
    finally:
        m.close()
    if total == 0:
        sys.exit("[ERROR] no tensor of %s is part of the data set" % (", ".join(args.set_fn) if args.set_fn else args.tensor_fn))
    sys.stdout.write("\n".join(report_lines(counts)) + "\n")


if __name__ == "__main__":
    main()
