"""train_clr: clair/train_clr.py on the device -- `python -m clair_amd.train_clr --tensor_fn tensors --var_fn truth.var --ochk_prefix model`.

clair_amd.train with a cyclical learning rate (Clair.clr, clair/model.py:1086-1103) in place of the per-epoch schedule: the data set, the
split, the block shuffle, the epoch loop, the log lines, the checkpoint names and the final report are train's own (train.train_model with
its per-batch hook).  What is the reference's (clair/train_clr.py:28-195):
  * clr is advanced exactly once before every batch, training or validation, in the order they run; global_step and the decayed max_lr
    carry over from epoch to epoch;
  * step_size = stepsizeConstant * (ceil(n_train / batch_size + 1) + ceil(n_validation / predictBatchSize + 1)), with true division;
  * the rate cycles between param.clr_min_lr and param.clr_max_lr whatever --learning_rate says: that flag only shows in the first log line;
  * there is no learning-rate switch and no early stop;
  * the loop runs while epoch <= --max_epochs (default param.maxEpoch): an ABSOLUTE epoch number, where train's --max_epochs counts epochs.
    After --chkpnt_fn model-000004, `--max_epochs 6` runs epochs 5 and 6.
What differs: the --*bin_fn flags exit with evaluate's message, --ochk_prefix is required, --clr_mode takes tri, tri2 or exp only
(the reference treats any other word as tri), and train's own flags (--set_fn, --batch_size, --micro_batch, --device, --seed) are taken.
docs/train_clr.md.
"""
import logging
import sys

import numpy as np

from clair_amd import param, train

CLR_MODES = ("tri", "tri2", "exp")


def step_size_of(n_train, n_validation, batch_size, with_validation=True):
    """Half a cycle in clr calls (clair/train_clr.py:63-65; clair/learning_rate_finder.py:135-136 without the validation batches)."""
    iterations = np.ceil(n_train / batch_size + 1)
    if with_validation:
        iterations = iterations + np.ceil(n_validation / param.predictBatchSize + 1)
    return param.stepsizeConstant * iterations


class Cycle(object):
    """The state clr hands back and wants again: one advance() per batch."""

    def __init__(self, m, step_size, max_lr, mode):
        self.m, self.step_size, self.max_lr, self.mode, self.global_step = m, step_size, max_lr, mode, 0

    def advance(self):
        _rate, self.global_step, self.max_lr = self.m.clr(self.global_step, self.step_size, self.max_lr, self.mode)


def train_model(m, X, Y, learning_rate, lambd, prefix, start_from, batch_size, last_epoch, cycle, train_batch=None, after_epoch=None):
    """train.train_model bounded by the absolute epoch number last_epoch, `cycle` advanced before every batch
    -> [(validation total, epoch), ...]"""
    if start_from is not None and int(start_from[-param.parameterOutputPlaceHolder:]) + 1 > last_epoch:
        sys.exit("[ERROR] %s is epoch %d: nothing is left to run up to epoch %d (an absolute epoch number)"
                 % (start_from, int(start_from[-param.parameterOutputPlaceHolder:]), last_epoch))
    return train.train_model(m, X, Y, learning_rate, lambd, prefix, start_from, batch_size, None, last_epoch=last_epoch, before_batch=cycle.advance,
                             train_batch=train_batch, after_epoch=after_epoch)


def build_parser():
    parser = train.build_parser("Train a model on the GPU with a cyclical learning rate")
    parser.add_argument("--clr_mode", type=str, default="exp", choices=CLR_MODES, help="how max_lr changes from cycle to cycle: tri keeps it, tri2 halves it, "
                        "exp multiplies it by %g, default: %%(default)s" % param.clrGamma)
    parser.set_defaults(learning_rate=param.clr_min_lr)
    for action in parser._actions:
        if action.dest == "learning_rate":
            action.help = "only logged: the rate cycles between param.clr_min_lr and param.clr_max_lr, default: %(default)s"
        elif action.dest == "max_epochs":
            action.help = "the last epoch NUMBER to run (the count goes on from --chkpnt_fn), default: %(default)s"
    return parser


def main():
    logging.basicConfig(format='%(message)s', level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv) == 1:
        parser.print_help()
        sys.exit(1)
    train.check_arguments(args)

    def loop(m, X, Y):
        n_train, n_validation, _ = train.split_sizes(len(X))
        cycle = Cycle(m, step_size_of(n_train, n_validation, args.batch_size), param.clr_max_lr, args.clr_mode)
        return train_model(m, X, Y, args.learning_rate, args.lambd, args.ochk_prefix, args.chkpnt_fn, args.batch_size, args.max_epochs, cycle)

    train.run_command(args, loop)


if __name__ == "__main__":
    main()
