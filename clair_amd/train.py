"""train: clair/train.py on the device -- `python -m clair_amd.train --tensor_fn tensors --var_fn truth.var --ochk_prefix model`.

The behaviour of the flags, the per-epoch log lines, the checkpoint names (prefix-%06d, the epoch number continued from
--chkpnt_fn[-6:]), the learning-rate schedule and the block shuffle are the reference's (clair/train.py:18-76, 191-259), restated.  What differs:
  * the data set is the text one of clair_amd.evaluate.labelled_batches (get_training_array, clair/utils.py:133-220), held in host
    memory, shuffled once as get_training_array does by default -- or the same rows from the sets of clair_amd.make_train_set
    (--set_fn, repeatable); the blosc binaries (--bin_fn, --train_bin_fn, --validation_bin_fn)
    are not read;
  * the first int(N * 0.9) rows train in batches of --batch_size, the rest validate in batches of param.predictBatchSize; between epochs
    the first int(n_train / 500) blocks of 500 rows are permuted (permute_leading_blocks);
  * --max_epochs bounds the loop (the reference's ends only after three learning-rate switches);
  * --olog_dir is accepted and ignored (the reference's summary writer is a dead path too);
  * everything is float32 on the device (docs/train.md).
At the end the best epoch is restored and evaluate's report is printed.
"""
import logging
import os
import random
import sys
from argparse import ArgumentParser
from time import time

import numpy as np

from clair_amd import param
from clair_amd.evaluate import BINARY_MESSAGE


# ---- the learning-rate schedule: three questions about the per-epoch validation totals (truth tables of clair/train.py:18-62) ----------
def minimum_is_recent(totals):
    """True while the smallest validation total so far is one of the last five epochs' (always, for five epochs or fewer)."""
    totals = np.asarray(totals, dtype=float)
    return len(totals) <= 5 or bool(totals[-5:].min() == totals.min())


def zigzags(totals):
    """True when the last six totals strictly alternate: down-up-down-up-down or up-down-up-down-up.  Needs more than six epochs."""
    totals = np.asarray(totals, dtype=float)
    if len(totals) <= 6:
        return False
    direction = np.sign(np.diff(totals[-6:]))
    return bool((direction != 0).all() and (direction[1:] == -direction[:-1]).all())


def stays_above_minimum(totals):
    """True when each of the last five totals is above the smallest so far.  Needs more than six epochs."""
    totals = np.asarray(totals, dtype=float)
    return len(totals) > 6 and bool((totals[-5:] > totals.min()).all())


def learning_rate_is_due(epochs_at_this_rate, totals):
    """The reference's switch rule (clair/train.py:217-227): after six epochs at a rate, a zigzag whose minimum is not recent; after eight,
    five epochs in a row above the minimum."""
    return ((epochs_at_this_rate >= 6 and not minimum_is_recent(totals) and zigzags(totals))
            or (epochs_at_this_rate >= 8 and stays_above_minimum(totals)))


def permute_leading_blocks(blocks, n):
    """What the reference's shuffle_first_n_items does to the block list between epochs: the first n entries in a new random order (NumPy's
    global generator), the rest where they are; all of them when the list has n entries or fewer."""
    blocks = np.asarray(blocks)
    n = len(blocks) if len(blocks) <= n else n
    return np.concatenate([blocks[:n][np.random.permutation(n)], blocks[n:]])


def split_sizes(dataset_size):
    """-> (training rows, validation rows, training blocks of bloscBlockSize rows that the epoch shuffle permutes)"""
    n_train = int(dataset_size * param.trainingDatasetPercentage)
    return n_train, dataset_size - n_train, int(n_train / param.bloscBlockSize)


def row_order(block_index_list, dataset_size):
    """The rows of the data set in the order of its blocks of bloscBlockSize rows."""
    size = param.bloscBlockSize
    return np.concatenate([np.arange(b * size, min((b + 1) * size, dataset_size)) for b in block_index_list]) if dataset_size else np.zeros(0, dtype=int)


def load_dataset(tensor_fn, var_fn, bed_fn, set_fn=None):
    """get_training_array (clair/utils.py:133-220): -> (X float32 [N,33,8,4], labels uint8 [N,4]), shuffled once.  set_fn: the sets
    make_train_set wrote for the same sites, in place of the text (the same rows, the same bits)."""
    if set_fn:
        from clair_amd.make_train_set import load_sets
        X, _keys, Y = load_sets(set_fn)
    else:
        from clair_amd.evaluate import labelled_batches
        xs, ys = [], []
        for X, _keys, labels in labelled_batches(tensor_fn, var_fn, bed_fn, param.engineBatchSize):
            xs.append(np.array(X, dtype=np.float32))
            ys.append(labels)
        if not xs:
            return np.zeros((0, 33, 8, 4), dtype=np.float32), np.zeros((0, 4), dtype=np.uint8)
        X, Y = np.concatenate(xs, axis=0), np.concatenate(ys, axis=0)
    order = np.random.permutation(len(X))
    return X[order], Y[order]


def checkpoint_name(prefix, epoch):
    return "%s-%0*d" % (prefix, param.parameterOutputPlaceHolder, epoch)


def run_epoch(m, X, Y, rows, n_train, batch_size, before_batch=None, train_batch=None):
    """One pass: optimizer steps over the first n_train rows of `rows`, then validation over the rest.
    -> (training total, [validation total, gt21, genotype, indel 1, indel 2])
    The two hooks are train_clr's and learning_rate_finder's: before_batch() runs before every batch, training or validation, and
    train_batch(x, y) takes a training batch in place of m.train."""
    train_batch = train_batch or m.train
    trained = 0.0
    for at in range(0, n_train, batch_size):
        pick = rows[at:min(at + batch_size, n_train)]
        if before_batch is not None:
            before_batch()
        train_batch(X[pick], Y[pick])
        trained += m.training_loss_on_one_batch
    validated = np.zeros(5)
    for at in range(n_train, len(rows), param.predictBatchSize):
        pick = rows[at:at + param.predictBatchSize]
        if before_batch is not None:
            before_batch()
        m.validate(X[pick], Y[pick])
        validated += (m.validation_loss_on_one_batch, m.gt21_loss, m.genotype_loss, m.indel_length_loss_1, m.indel_length_loss_2)
    return trained, validated


def train_model(m, X, Y, learning_rate, lambd, prefix, start_from, batch_size, max_epochs, last_epoch=None, before_batch=None, train_batch=None,
                after_epoch=None):
    """The epoch loop -> [(validation total, epoch), ...].  Log lines, checkpoint names and the schedule are the reference's
    (clair/train.py:94-96, 191-235); the loop also ends after max_epochs.
    train_clr and learning_rate_finder run the same loop with a rate of their own: last_epoch (an absolute epoch number) bounds it in
    place of max_epochs and takes the learning-rate switches and the early stop out, before_batch / train_batch are run_epoch's hooks,
    and after_epoch(epoch) runs once the epoch's checkpoint is written."""
    first_epoch = 1
    if start_from is not None:
        m.restore_parameters(os.path.abspath(start_from))
        first_epoch = int(start_from[-param.parameterOutputPlaceHolder:]) + 1
    logging.info("[INFO] Start training...")
    logging.info("[INFO] Learning rate: %.2e" % m.set_learning_rate(learning_rate))
    logging.info("[INFO] L2 regularization lambda: %.2e" % m.set_l2_regularization_lambda(lambd))

    started = time()
    n_train, n_validation, n_train_blocks = split_sizes(len(X))
    blocks = np.arange(-(-len(X) // param.bloscBlockSize))
    history, totals = [], []
    switches_left, epochs_at_this_rate = param.maxLearningRateSwitch, 0
    for epoch in range(first_epoch, first_epoch + max_epochs if last_epoch is None else last_epoch + 1):
        if epoch > first_epoch:
            blocks = permute_leading_blocks(blocks, n_train_blocks)
            logging.info("[INFO] Shuffled: " + " ".join(str(b) for b in np.append(blocks[:5], blocks[-5:])))
        epoch_started = time()
        trained, validated = run_epoch(m, X, Y, row_order(blocks, len(X)), n_train, batch_size, before_batch, train_batch)
        logging.info("%d Training loss: %s" % (epoch, trained / n_train))
        logging.info("%d Validation loss (Total/Base/Genotype/Indel_1_2):\t%s" % (epoch, "\t".join(str(v / n_validation) for v in validated)))
        logging.info("[INFO] Epoch time elapsed: %.2f s" % (time() - epoch_started))
        history.append((validated[0], epoch))
        totals.append(validated[0])
        m.save_parameters(os.path.abspath(checkpoint_name(prefix, epoch)))
        if after_epoch is not None:
            after_epoch(epoch)
        epochs_at_this_rate += 1
        if last_epoch is None and learning_rate_is_due(epochs_at_this_rate, totals):
            switches_left -= 1
            if switches_left == 0:
                break
            logging.info("[INFO] New learning rate: %.2e" % m.decay_learning_rate())
            logging.info("[INFO] New L2 regularization lambda: %.2e" % m.decay_l2_regularization_lambda())
            epochs_at_this_rate = 0
    logging.info("[INFO] Training time elapsed: %.2f s" % (time() - started))
    return history


# (flag, keyword arguments of add_argument): the reference's flags and defaults (clair/train.py:270-319), then this implementation's own
SWITCHES = (("--SGDM", "optimizer: momentum SGD (%g, no Nesterov)" % param.momentum), ("--Adam", "optimizer: Adam"),
            ("--cross_entropy", "loss: cross entropy with per-class weights"), ("--focal_loss", "loss: focal loss, gamma 2"))
OPTIONS = (
    ("--bin_fn", str, None, "blosc binary of the whole data set (not read by this build)"),
    ("--train_bin_fn", str, None, "blosc binary of the training part (not read by this build)"),
    ("--validation_bin_fn", str, None, "blosc binary of the validation part (not read by this build)"),
    ("--tensor_fn", str, "vartensors", "tensors as CreateTensor writes them, default: %(default)s"),
    ("--var_fn", str, "truthvars", "truth rows `ctg pos ref alt g1 g2` as GetTruth writes them, default: %(default)s"),
    ("--bed_fn", str, None, "BED file of the regions whose sites make the data set"),
    ("--chkpnt_fn", str, None, "checkpoint to go on from; its last six characters are the epoch number to continue after"),
    ("--learning_rate", float, param.initialLearningRate, "learning rate of the first epochs, default: %(default)s"),
    ("--lambd", float, param.l2RegularizationLambda, "weight of the L2 term, default: %(default)s"),
    ("--ochk_prefix", str, None, "where the checkpoint of each epoch goes: PREFIX-000001, ...; required"),
    ("--olog_dir", str, None, "accepted for the reference's command lines and ignored"),
    ("--batch_size", int, param.trainBatchSize, "rows of one optimizer step, default: %(default)s"),
    ("--micro_batch", int, param.trainMicroBatchSize, "rows of one forward + backward pass on the device; a batch's micro-batches add their "
                                                      "gradients up, default: %(default)s"),
    ("--device", int, 0, "HIP device ordinal, default: %(default)s"),
    ("--seed", int, None, "seed of the initial weights, the shuffles and the dropout masks, default: a random one"),
    ("--max_epochs", int, param.maxEpoch, "stop after this many epochs at the latest, default: %(default)s"),
)


def build_parser(description="Train a model on the GPU from text tensors and truth rows", leave_out=()):
    """leave_out: flags of OPTIONS a sibling command does not take (learning_rate_finder)."""
    parser = ArgumentParser(description=description)
    for flag, text in SWITCHES:
        parser.add_argument(flag, action="store_true", help=text)
    for flag, kind, default, text in OPTIONS:
        if flag not in leave_out:
            parser.add_argument(flag, type=kind, default=default, help=text)
    parser.add_argument("--set_fn", type=str, action="append", default=None, metavar="NPZ",
                        help="training set written by make_train_set --set_fn, repeatable (the rows are concatenated); --tensor_fn, --var_fn and "
                             "--bed_fn are ignored then")
    return parser


def check_arguments(args):
    """The exits of main() before anything is loaded."""
    if args.bin_fn is not None or args.train_bin_fn is not None or args.validation_bin_fn is not None:
        sys.exit(BINARY_MESSAGE)
    if args.ochk_prefix is None:
        sys.exit("[ERROR] --ochk_prefix is required")
    if args.batch_size < 1 or args.micro_batch < 1 or args.max_epochs < 1:
        sys.exit("[ERROR] --batch_size, --micro_batch and --max_epochs are at least 1")


def run_command(args, loop):
    """What main() does once the arguments are read and checked, shared with train_clr and learning_rate_finder: seed, model, data set,
    loop(m, X, Y) -> [(validation total, epoch), ...], then the best epoch restored and evaluate's report printed."""
    seed = args.seed if args.seed is not None else param.RANDOM_SEED
    random.seed(seed)
    np.random.seed(seed)

    # a flag that is given wins over the default; SGDM over Adam and focal loss over cross entropy when both are given, as in the reference
    optimizer = "SGDM" if args.SGDM else "Adam" if args.Adam else param.default_optimizer
    loss_function = "FocalLoss" if args.focal_loss else "CrossEntropy" if args.cross_entropy else param.default_loss_function
    logging.info("[INFO] Initializing")
    logging.info("[INFO] Optimizer: %s" % optimizer)
    logging.info("[INFO] Loss Function: %s" % loss_function)

    from clair_amd import evaluate
    from clair_amd.model import Clair
    try:
        m = Clair(optimizer_name=optimizer, loss_function=loss_function, device=args.device, micro_batch=args.micro_batch,
                  max_batch=param.engineBatchSize, n_slots=param.pipeline_slots(),
                  seed=seed if seed is not None else random.SystemRandom().randrange(1 << 31))
        m.init()
    except Exception as exc:   # C-ABI errors surface as messages + non-zero exit
        sys.exit("[ERROR] %s" % exc)
    try:
        logging.info("[INFO] Loading dataset...")
        X, Y = load_dataset(args.tensor_fn, args.var_fn, args.bed_fn, args.set_fn)
        logging.info("[INFO] The size of dataset: %d" % len(X))
        n_train, n_validation, _ = split_sizes(len(X))
        if n_train == 0 or n_validation == 0:
            sys.exit("[ERROR] %d tensors of %s make the data set: too few to split %d%% / %d%%"
                     % (len(X), ", ".join(args.set_fn) if args.set_fn else args.tensor_fn, round(param.trainingDatasetPercentage * 100), round((1 - param.trainingDatasetPercentage) * 100)))
        history = loop(m, X, Y)
        best_epoch = min(history)[1]        # the smallest validation total; the earlier epoch of equal ones
        logging.info("[INFO] Best validation loss at epoch: %d" % best_epoch)
        m.restore_parameters(os.path.abspath(checkpoint_name(args.ochk_prefix, best_epoch)))
        step = param.engineBatchSize
        counts, _total = evaluate.evaluate_counts(m, ((X[i:i + step], None, Y[i:i + step]) for i in range(0, len(X), step)))
    finally:
        m.close()
    sys.stdout.write("\n".join(evaluate.report_lines(counts)) + "\n")


def main():
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    check_arguments(args)
    run_command(args, lambda m, X, Y: train_model(m, X, Y, args.learning_rate, args.lambd, args.ochk_prefix, args.chkpnt_fn, args.batch_size, args.max_epochs))


if __name__ == "__main__":
    main()
