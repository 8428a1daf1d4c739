#!/usr/bin/env python3
"""One full training step, measured (a measurement for the record, not a gate; docs/train.md).

A step is Clair.train on one batch: --batch rows (default 10000) cut into micro-batches of --micro_batch (default 1024), forward + loss +
backward on each with dropout on, then the optimizer step (Adam, focal loss).  Median of --steps (default 10) after --warmup (default 3),
one JSON line with every step's time.  The input upload from pageable host memory is part of the step, as it is in clair_amd.train.

    python tools/gpu/train_step_bench.py [--batch 10000] [--micro_batch 1024] [--steps 10] [--warmup 3] [--lr_train]

--lr_train times Clair.lr_train instead: the same step plus, per micro-batch, the accuracy count on the device and the download of the
probabilities (docs/train_clr.md).

The per-kernel split comes from a separate, shorter run under the profiler, summed by kernel and grid (a tgemm shape is told by its grid):

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gpu/train_step_bench.py --steps 2 --warmup 1
    python tools/gpu/train_step_bench.py --trace OUT/.../*_kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def trace_summary(path, top=24):
    """kernel-trace CSV -> rows (total ms, launches, kernel, grid in workgroups), largest first"""
    total = defaultdict(lambda: [0.0, 0])
    with open(path) as f:
        for row in csv.DictReader(f):
            wg = [int(row["Grid_Size_%s" % a]) // max(int(row["Workgroup_Size_%s" % a]), 1) for a in "XYZ"]
            key = (row["Kernel_Name"].split("(")[0], tuple(wg))
            total[key][0] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
            total[key][1] += 1
    rows = sorted(((ms, n, k, g) for (k, g), (ms, n) in total.items()), reverse=True)
    everything = sum(r[0] for r in rows)
    print("%10.3f ms in %d launches" % (everything, sum(r[1] for r in rows)))
    for ms, n, k, g in rows[:top]:
        print("%10.3f ms %5.1f%% %7d x %-44s grid %s" % (ms, 100 * ms / everything, n, k[-44:], "x".join(str(v) for v in g)))


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batch", type=int, default=10000)
    p.add_argument("--micro_batch", type=int, default=1024)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--optimizer", default="Adam", choices=("Adam", "SGDM"))
    p.add_argument("--loss", default="FocalLoss", choices=("FocalLoss", "CrossEntropy"))
    p.add_argument("--lr_train", action="store_true", help="time Clair.lr_train (the learning-rate finder's step) instead of Clair.train")
    p.add_argument("--trace", default=None, help="summarise a rocprofv3 kernel-trace CSV instead of running")
    a = p.parse_args()
    if a.trace:
        return trace_summary(a.trace)
    from clair_amd import synth
    from clair_amd.model import Clair
    x, _ = synth.synthetic_input(a.batch, seed=1)
    rng = np.random.default_rng(2)
    labels = np.stack([rng.integers(0, k, a.batch) for k in (21, 3, 33, 33)], axis=1).astype(np.uint8)
    m = Clair(max_batch=16, n_slots=1, micro_batch=a.micro_batch, optimizer_name=a.optimizer, loss_function=a.loss, seed=1)
    try:
        m.init()
        times, step = [], m.lr_train if a.lr_train else m.train
        for k in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            step(x, labels)
            times.append(time.perf_counter() - t0)
        measured = times[a.warmup:]
        print(json.dumps(dict(member="lr_train" if a.lr_train else "train", batch=a.batch, micro_batch=a.micro_batch, optimizer=a.optimizer, loss=a.loss, warmup=a.warmup,
                              step_seconds=[round(t, 5) for t in measured], median_step_seconds=round(float(np.median(measured)), 5),
                              rows_per_second=round(a.batch / float(np.median(measured)), 1), last_loss_per_row=m.training_loss_on_one_batch / a.batch,
                              gradient_norm=m.gradient_norm_on_one_batch)))
    finally:
        m.close()


if __name__ == "__main__":
    main()
