#!/usr/bin/env python3
"""Mint tests/golden/train_clr_cases.json from the REAL reference functions (runs only where a reference checkout exists, like the other
tools/make_*_golden.py): clair.model.Clair.clr and clair.learning_rate_finder.accuracy / lr_finder are IMPORTED and CALLED on inputs built
here; nothing of them is copied.  The fixture holds inputs and recorded outputs only.

    python tools/mint_train_clr_golden.py --reference DIR        (or $CLAIR_REFERENCE: a checkout of the reference project)

TensorFlow and blosc are not needed by the three functions but are imported by their modules; an import hook of this tool answers those
imports (and intervaltree / pysam, where they are missing) with empty stand-in modules.  pandas is needed: lr_finder is the reference's.
clr is called unbound on a bare object: it reads nothing of a Clair but writes learning_rate_value.

The fixture:
  param      the seven constants of shared/param.py the three programs read
  clr        per case mode, step_size, max_lr and, per call, [learning rate, global_step, max_lr] as returned (and the rate as stored)
  accuracy   per case probabilities [n][90], labels [n][4], the reference's accuracy, and for the hand-made cases the counts they were
             made to give (checked here: the reference's accuracy is their mean rate)
  lr_finder  per case the rows and either min_lr, max_lr, the table and the bytes of to_csv, or the name of what the reference raises
"""
import argparse
import importlib.abc
import importlib.machinery
import importlib.util
import io
import json
import os
import sys
import types
from unittest import mock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "train_clr_cases.json")
HEADS = ((0, 21), (21, 24), (24, 57), (57, 90))


class StandIn(types.ModuleType):
    """A module that has every attribute and every submodule asked of it."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return mock.MagicMock(name="%s.%s" % (self.__name__, name))


class StandInFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def __init__(self, roots):
        self.roots = tuple(roots)

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in self.roots:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        return StandIn(spec.name)

    def exec_module(self, module):
        pass


def install_stand_ins(reference):
    roots = ["tensorflow", "blosc"] + [name for name in ("intervaltree", "pysam") if importlib.util.find_spec(name) is None]
    sys.meta_path.insert(0, StandInFinder(roots))
    sys.path.insert(0, reference)
    if not hasattr(np, "int"):
        np.int = int                # the reference predates NumPy 1.24


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
CLR_CASES = [(mode, step_size, max_lr, calls)
             for step_size, max_lr, calls in ((4, 3e-2, 3 * 9 + 2), (7.0, 1e-1, 3 * 15 + 4), (11.0, 3e-2, 30), (9.0, 1e-1, 12))
             for mode in ("tri", "tri2", "exp")]


def rows_from(top, labels, rng=None, ties=()):
    """probabilities [n][90] whose arg-max per head is `top` [n][4] (softmax-like when rng is given, one-hot otherwise); `ties`: (row, head,
    [indices]) -- those indices share the row's largest value, so the lowest of them is the arg-max"""
    n = len(top)
    p = np.zeros((n, 90), dtype=np.float32)
    for i in range(n):
        for k, (a, b) in enumerate(HEADS):
            v = rng.random(b - a).astype(np.float32) if rng is not None else np.zeros(b - a, dtype=np.float32)
            v[top[i][k]] = v.max() + np.float32(0.5)
            p[i, a:b] = v / v.sum()
    for i, k, where in ties:
        a, _ = HEADS[k]
        p[i, [a + j for j in where]] = p[i].max() + np.float32(1.0)
    return p, np.asarray(labels, dtype=np.uint8)


def accuracy_cases():
    cases = []
    # the issue's four rows: a swapped indel pair (still right), a wrong gt21, a wrong larger indel -> 14 of 16
    top = [[3, 1, 2, 5], [4, 0, 0, 0], [7, 2, 16, 16], [20, 1, 30, 4]]
    lab = [[3, 1, 5, 2], [5, 0, 0, 0], [7, 2, 16, 16], [20, 1, 4, 31]]
    cases.append(("four rows: swapped pair, wrong gt21, wrong larger indel", rows_from(top, lab), [3, 4, 4, 3]))
    # swapped on the prediction side, on the label side, on both; equal pair elements against an unequal pair
    top = [[0, 0, 9, 1], [0, 0, 1, 9], [0, 0, 9, 1], [1, 1, 6, 6], [1, 1, 6, 7], [2, 2, 0, 32], [2, 2, 32, 0]]
    lab = [[0, 0, 1, 9], [0, 0, 9, 1], [0, 0, 9, 1], [1, 1, 6, 7], [1, 1, 6, 6], [2, 2, 32, 0], [2, 2, 31, 1]]
    cases.append(("pairs swapped on either side, equal elements", rows_from(top, lab), [7, 7, 6, 4]))
    # ties: the lowest index wins (np.argmax)
    lab = [[2, 0, 4, 8], [9, 2, 8, 12]]               # the second row would be all right if the HIGHEST index won
    ties = [(0, 0, [2, 9]), (0, 1, [0, 2]), (0, 2, [4, 8]), (0, 3, [8, 12]), (1, 0, [2, 9]), (1, 1, [0, 2]), (1, 2, [4, 8]), (1, 3, [8, 12])]
    cases.append(("arg-max ties: the lowest index wins", rows_from([[2, 0, 4, 8], [2, 0, 4, 8]], lab, ties=ties), [1, 1, 1, 1]))
    cases.append(("one row, all right", rows_from([[5, 2, 3, 1]], [[5, 2, 1, 3]]), [1, 1, 1, 1]))
    cases.append(("one row, all wrong", rows_from([[5, 2, 3, 1]], [[6, 1, 4, 2]]), [0, 0, 0, 0]))
    cases.append(("uniform rows: every arg-max is index 0", (np.full((3, 90), 1.0 / 90, dtype=np.float32),
                                                              np.array([[0, 0, 0, 0], [1, 1, 1, 1], [0, 1, 1, 0]], dtype=np.uint8)), [2, 1, 2, 1]))
    rng = np.random.default_rng(20)
    for n in (7, 50):                  # softmax-like rows, half of every head's labels right; counts left to the reference's accuracy alone
        top = np.stack([rng.integers(0, b - a, n) for a, b in HEADS], axis=1)
        lab = np.where(rng.random((n, 4)) < 0.5, top, np.stack([rng.integers(0, b - a, n) for a, b in HEADS], axis=1))
        cases.append(("%d random rows" % n, rows_from(top, lab, rng=rng), None))
    return cases


LR_FINDER_CASES = [
    ("six rows", [(1e-4, 0.25, 2.5), (0.02, 0.375, 2.25), (0.04, 0.625, 2.0), (0.06, 0.5625, 2.125), (0.08, 0.3125, 3.0), (0.1, 0.3125, 3.5)]),
    ("out of order: the steepest fall comes at a lower rate than the steepest rise", [(1e-4, 0.5, 1.0), (1e-3, 0.25, 1.5), (1e-2, 0.75, 0.5), (1e-1, 0.7, 0.6)]),
    ("two rows", [(1e-5, 0.1, 9.0), (3e-05, 0.30000000000000004, 8.0)]),
    ("tied for the largest diff", [(0.01, 0.25, 1.0), (0.02, 0.5, 1.0), (0.03, 0.375, 1.0), (0.04, 0.625, 1.0), (0.05, 0.0, 1.0)]),
    ("tied for the smallest diff", [(0.01, 0.5, 1.0), (0.02, 0.25, 1.0), (0.03, 0.75, 1.0), (0.04, 0.5, 1.0)]),
]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("CLAIR_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=OUT, help="where the fixture is written, default: %(default)s")
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "clair", "learning_rate_finder.py")):
        ap.error("--reference DIR (or CLAIR_REFERENCE) is needed: this tool calls the reference's own functions")
    install_stand_ins(args.reference)
    import shared.param as rparam
    from clair.model import Clair
    from clair import learning_rate_finder as rfinder

    out = {"param": {k: getattr(rparam, k) for k in ("clr_max_lr", "clr_min_lr", "stepsizeConstant", "clrGamma", "min_lr", "max_lr", "lr_finder_max_epoch")}}

    out["clr"] = []
    for mode, step_size, max_lr, calls in CLR_CASES:
        bare, global_step, top, rows = types.SimpleNamespace(), 0, max_lr, []
        for _ in range(calls):
            rate, global_step, top = Clair.clr(bare, global_step, step_size, top, mode)
            assert float(rate) == float(bare.learning_rate_value)
            rows.append([float(rate), int(global_step), float(top)])
        out["clr"].append({"mode": mode, "step_size": step_size, "max_lr": max_lr, "calls": rows})
        print("clr %-4s step_size %-4s %2d calls, last max_lr %r" % (mode, step_size, calls, rows[-1][2]))

    out["accuracy"] = []
    for name, (p, lab), counts in accuracy_cases():
        one_hot = np.zeros((len(p), 90), dtype=np.float32)
        for k, (a, _) in enumerate(HEADS):
            one_hot[np.arange(len(p)), a + lab[:, k].astype(int)] = 1.0
        got = float(rfinder.accuracy([p[:, a:b] for a, b in HEADS], one_hot))
        if counts is not None:
            assert got == sum(c / float(len(p)) for c in counts) / 4, (name, got, counts)
        out["accuracy"].append({"name": name, "probabilities": [[float(v) for v in row] for row in p], "labels": lab.tolist(), "counts": counts,
                                "accuracy": got})
        print("accuracy %-60s n=%2d -> %r" % (name, len(p), got))

    out["lr_finder"] = []
    for name, rows in LR_FINDER_CASES:
        case = {"name": name, "rows": [list(r) for r in rows]}
        try:
            minimum_lr, maximum_lr, df = rfinder.lr_finder(rows)
        except Exception as exc:            # the tied cases: .item() on more than one row
            case["raises"] = type(exc).__name__
        else:
            text = io.StringIO()
            df.to_csv(text, sep=",", index=False)
            case.update(min_lr=float(minimum_lr), max_lr=float(maximum_lr), table=[[float(v) for v in row] for row in df.values.tolist()], csv=text.getvalue())
        out["lr_finder"].append(case)
        print("lr_finder %-80s -> %s" % (name, case.get("raises") or (case["min_lr"], case["max_lr"])))
    assert [("raises" in c) for c in out["lr_finder"]] == [False, False, False, True, True]

    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
