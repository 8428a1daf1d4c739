"""learning_rate_finder: clair/learning_rate_finder.py on the device --
`python -m clair_amd.learning_rate_finder --tensor_fn tensors --var_fn truth.var --ochk_prefix model [--olr_fn lr_finder.txt]`.

What a user runs before train_clr to pick the two ends of the cycle: param.lr_finder_max_epoch epochs with the rate swept up and down
(Clair.clr, mode tri, up to param.max_lr), every training batch through Clair.lr_train, one row (rate the batch trained with, accuracy of
the batch, loss of the batch) per training batch; after each epoch `[INFO] min_lr: %g, max_lr: %g` is logged and the table written.
The loop is train's (train.train_model by way of train_clr.train_model); the accuracy of a batch is counted on the device
(clair_train_accuracy, docs/train_clr.md).  What is the reference's (clair/learning_rate_finder.py:100-267):
  * step_size = stepsizeConstant * ceil(n_train / batch_size + 1): the training batches alone, although clr is advanced before every batch,
    validation ones included;
  * param.min_lr is only logged (and --learning_rate not even that): the sweep starts from param.clr_min_lr, the floor of Clair.clr;
  * accuracy comes from the training-mode forward pass, dropout on (the reference reads m.prediction, which only lr_train sets);
  * the epoch loop runs while epoch <= param.lr_finder_max_epoch, an absolute epoch number as in train_clr.
What differs: --olr_fn names the table (the reference's fixed name is the default); --ochk_prefix is required; the optimizer and loss
switches and train's own flags are taken; a tie for the largest or the smallest diff is settled (lr_finder) where the reference raises;
fewer than two training batches is an [ERROR] before training (no diff could be taken).
"""
import logging
import sys

from clair_amd import param, train, train_clr

TABLE_HEADER = "lr,accuracy,loss,diff"


def lr_finder(rows):
    """clair/learning_rate_finder.py:76-84 without pandas: rows [(lr, accuracy, loss), ...] in batch order
    -> (min_lr, max_lr, table [(lr, accuracy, loss, diff), ...]).
    diff is a row's accuracy minus the previous row's and the first row is dropped; min_lr is the rate of the row with the largest diff,
    max_lr that of the row with the smallest, and the two are swapped when out of order.  Ties: the reference raises (.item() on more than
    one row); here the first row of the reference's own sort is taken -- the largest rate among the rows tied for min_lr, the smallest among
    those tied for max_lr."""
    rows = [(float(lr), float(accuracy), float(loss)) for lr, accuracy, loss in rows]
    if len(rows) < 2:
        raise ValueError("lr_finder needs at least two rows, got %d" % len(rows))
    table = [(lr, accuracy, loss, accuracy - before[1]) for before, (lr, accuracy, loss) in zip(rows, rows[1:])]
    largest, smallest = max(r[3] for r in table), min(r[3] for r in table)
    minimum_lr = max(r[0] for r in table if r[3] == largest)
    maximum_lr = min(r[0] for r in table if r[3] == smallest)
    if minimum_lr > maximum_lr:
        minimum_lr, maximum_lr = maximum_lr, minimum_lr
    return minimum_lr, maximum_lr, table


def table_text(table):
    """The reference's `to_csv(sep=',', index=False)` of the table: float64 columns are written as repr(float)."""
    return "".join(line + "\n" for line in [TABLE_HEADER] + [",".join(repr(float(v)) for v in row) for row in table])


def find_rates(m, X, Y, lambd, prefix, start_from, batch_size, olr_fn):
    """The finder's epochs -> [(validation total, epoch), ...]; the table goes to olr_fn after each epoch."""
    n_train, n_validation, _ = train.split_sizes(len(X))
    if -(-n_train // batch_size) < 2:
        sys.exit("[ERROR] %d training rows in batches of %d make fewer than two training batches: no accuracy difference to take" % (n_train, batch_size))
    cycle = train_clr.Cycle(m, train_clr.step_size_of(n_train, n_validation, batch_size, with_validation=False), param.max_lr, "tri")
    rows = []

    def train_batch(x, y):
        rate = m.learning_rate_value
        m.lr_train(x, y)
        rows.append((rate, m.training_accuracy, m.training_loss_on_one_batch))

    def after_epoch(_epoch):
        minimum_lr, maximum_lr, table = lr_finder(rows)
        logging.info("[INFO] min_lr: %g, max_lr: %g" % (minimum_lr, maximum_lr))
        with open(olr_fn, "w") as f:
            f.write(table_text(table))

    return train_clr.train_model(m, X, Y, param.min_lr, lambd, prefix, start_from, batch_size, param.lr_finder_max_epoch, cycle,
                                 train_batch=train_batch, after_epoch=after_epoch)


def build_parser():
    """The reference's flags (clair/learning_rate_finder.py:275-308: no --train_bin_fn / --validation_bin_fn, no --max_epochs), the
    optimizer and loss switches, train's own flags and --olr_fn."""
    parser = train.build_parser("Learning rate finder: sweep the rate over one epoch and propose train_clr's min_lr / max_lr",
                                leave_out=("--train_bin_fn", "--validation_bin_fn", "--max_epochs"))
    parser.add_argument("--olr_fn", type=str, default="lr_finder.txt", help="where the table lr,accuracy,loss,diff goes, default: %(default)s")
    parser.set_defaults(train_bin_fn=None, validation_bin_fn=None, max_epochs=param.lr_finder_max_epoch)      # what train.check_arguments reads
    for action in parser._actions:
        if action.dest == "learning_rate":
            action.help = "accepted for the reference's command lines and ignored: the sweep runs from param.clr_min_lr to param.max_lr, default: %(default)s"
    return parser


def main():
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    train.check_arguments(args)
    train.run_command(args, lambda m, X, Y: find_rates(m, X, Y, args.lambd, args.ochk_prefix, args.chkpnt_fn, args.batch_size, args.olr_fn))


if __name__ == "__main__":
    main()
