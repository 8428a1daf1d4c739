#!/usr/bin/env python3
"""The cost of scoring on the device, measured (a measurement for the record, not a gate).

ONT-shaped candidates resident in HBM, batch 1024, four slots, each leg sustained for at least --seconds:
  forward        clair_run_resident on the float32 tensor: the forward pass alone (what bench.py sustains);
  forward_eval   clair_submit_eval on the int16 counts of the same candidates at a device address, labels
                 from the host, no probabilities returned: counts -> float32, the forward pass, eval_kernel, the slot's completion
                 event.  Besides the scoring this leg carries the conversion kernel, 4 KB of labels over the link and one
                 submit / wait pair per pass on the host, so the gap between the legs is an UPPER bound on the scoring.
The legs alternate, --repeats times each; one JSON line with every repeat and the medians.  eval_kernel's own duration comes from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/gpu/evaluate_bench.py --seconds 0.5 --repeats 1`.

    python tools/gpu/evaluate_bench.py [--seconds 2] [--repeats 3] [--lib PATH_OF_ANOTHER_BUILD]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
BATCH, SLOTS, N_BATCHES = 1024, 4, 8


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--seconds", type=float, default=2.0, help="each leg runs at least this long, default: %(default)s")
    p.add_argument("--repeats", type=int, default=3, help="alternating repeats of each leg, default: %(default)s")
    p.add_argument("--lib", type=str, default=None, help="another build of libclair_amd.so (e.g. the parent commit's): its forward leg only")
    a = p.parse_args()
    from clair_amd import _capi, build, synth, weights
    e = _capi.Engine(device=0, max_batch=BATCH, n_slots=SLOTS, lib_path=a.lib)
    e.load_weights(weights.synthetic_weights(seed=20250928, head_gain=4.0))
    raw, _ = synth.synthetic_candidates(BATCH * N_BATCHES, "ont", seed=1)
    xd, od = e.dataset_alloc(len(raw))
    e.dataset_upload(xd, 0, synth.to_model_input(raw))
    can_eval = a.lib is None
    if can_eval:
        # the int16 counts in HBM: a resident buffer of the engine, filled with the raw bytes (two candidates per float32 row)
        cd, cod = e.dataset_alloc(len(raw) // 2)
        e.dataset_upload(cd, 0, np.ascontiguousarray(raw.astype(np.int16)).view(np.float32).reshape(-1, 33, 8, 4))
        counts_address = cd.value
        rng = np.random.default_rng(2)
        labels = [np.stack([rng.integers(0, k, BATCH) for k in (21, 3, 33, 33)], axis=1).astype(np.uint8) for _ in range(N_BATCHES)]
        row_bytes = 1056 * 2

    def forward():
        passes, t0 = 0, time.perf_counter()
        while True:
            for k in range(64):
                e.run_resident(k % SLOTS, xd, od, (k % N_BATCHES) * BATCH, BATCH)
            e.sync()
            passes += 64
            dt = time.perf_counter() - t0
            if dt >= a.seconds:
                return passes * BATCH / dt

    def forward_eval():
        e.eval_reset()
        passes, inflight, t0 = 0, [], time.perf_counter()
        while True:
            for k in range(64):
                slot = k % SLOTS
                if len(inflight) == SLOTS:
                    e.wait(inflight.pop(0))
                b = k % N_BATCHES
                e.submit_eval(slot, (counts_address + b * BATCH * row_bytes, BATCH), labels[b])
                inflight.append(slot)
            passes += 64
            dt = time.perf_counter() - t0
            if dt >= a.seconds:
                while inflight:
                    e.wait(inflight.pop(0))
                dt = time.perf_counter() - t0
                assert int(e.eval_read()[0]) == passes * BATCH
                return passes * BATCH / dt

    forward()                                                     # warm-up
    if can_eval:
        forward_eval()
    out = dict(batch=BATCH, slots=SLOTS, seconds=a.seconds, csrc=build.csrc_digest(), lib=a.lib or "this build", forward=[], forward_eval=[])
    for _ in range(a.repeats):
        out["forward"].append(round(forward()))
        if can_eval:
            out["forward_eval"].append(round(forward_eval()))
    out["forward_median"] = float(np.median(out["forward"]))
    if can_eval:
        out["forward_eval_median"] = float(np.median(out["forward_eval"]))
        out["forward_eval_over_forward"] = round(out["forward_eval_median"] / out["forward_median"], 4)
    e.dataset_free(xd, od)
    if can_eval:
        e.dataset_free(cd, cod)
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
