#!/usr/bin/env python3
"""The cost of ensemble calling on the device, measured (a measurement for the record, not a gate; docs/ensemble.md quotes it).

ONT-shaped candidates resident in HBM as int16 counts, batch 1024, four slots, call records back (no probabilities): the lean path of
callVarBam.  Each leg is sustained for at least --seconds on a host clock that starts on an idle device and stops after the last
clair_wait (the engine's lanes are streams of its own: events recorded outside the library would not bracket them):
  plain         clair_submit_ex with one checkpoint;
  ensemble_k1   clair_submit_ensemble with that checkpoint alone: the plain pass plus one averaging launch;
  ensemble_k3   clair_submit_ensemble with three checkpoints: three forward passes and three averaging launches per submit.
Rates are candidates per second (a candidate counts once, whatever K).  The legs alternate, --repeats times each; one JSON line with every
repeat and the medians.  --lib names another build of libclair_amd.so (the parent commit's): its plain leg only, for the comparison
"plain before / plain after".  The averaging kernel's own duration comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/gpu/ensemble_bench.py --seconds 0.5 --repeats 1`.

    python tools/gpu/ensemble_bench.py [--seconds 2] [--repeats 3] [--lib PATH_OF_ANOTHER_BUILD]
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
SEEDS = (20250928, 515, 9001)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--seconds", type=float, default=2.0, help="each leg runs at least this long, default: %(default)s")
    p.add_argument("--repeats", type=int, default=3, help="alternating repeats of each leg, default: %(default)s")
    p.add_argument("--lib", type=str, default=None, help="another build of libclair_amd.so (e.g. the parent commit's): its plain leg only")
    a = p.parse_args()
    from clair_amd import _capi, _hostapi, build, synth, weights

    class Resident(_capi.DeviceWindows):
        """n windows of int16 counts at a device address (what the device front end leaves in HBM)."""

        def __init__(self, address, n):
            self.address, self.n = int(address), int(n)

    ws = [weights.synthetic_weights(seed=s, head_gain=4.0) for s in SEEDS]
    e = _capi.Engine(device=0, max_batch=BATCH, n_slots=SLOTS, lib_path=a.lib)
    e.load_weights(ws[0])
    raw, infos = synth.synthetic_candidates(BATCH * N_BATCHES, "ont", seed=1)
    centre = _hostapi.centre_bytes(infos)
    # the int16 counts in HBM: a resident buffer of the engine, filled with the raw bytes (two candidates per float32 row)
    cd, cod = e.dataset_alloc(len(raw) // 2)
    e.dataset_upload(cd, 0, np.ascontiguousarray(raw.astype(np.int16)).view(np.float32).reshape(-1, 33, 8, 4))
    row_bytes = 1056 * 2
    windows = [Resident(cd.value + b * BATCH * row_bytes, BATCH) for b in range(N_BATCHES)]
    centres = [centre[b * BATCH:(b + 1) * BATCH] for b in range(N_BATCHES)]

    def leg(submit):
        e.sync()
        passes, inflight, t0 = 0, [], time.perf_counter()
        while True:
            for k in range(64):
                slot = k % SLOTS
                if len(inflight) == SLOTS:
                    e.wait(inflight.pop(0))
                submit(slot, windows[k % N_BATCHES], centres[k % N_BATCHES])
                inflight.append(slot)
            passes += 64
            if time.perf_counter() - t0 >= a.seconds:
                while inflight:
                    e.wait(inflight.pop(0))
                return passes * BATCH / (time.perf_counter() - t0)

    legs = [("plain", 1, lambda: leg(e.submit_calls))]
    if a.lib is None:
        legs += [("ensemble_k1", 1, lambda: leg(e.submit_ensemble)), ("ensemble_k3", 3, lambda: leg(e.submit_ensemble))]
    out = dict(batch=BATCH, slots=SLOTS, seconds=a.seconds, csrc=build.csrc_digest(), lib=a.lib or "this build")
    loaded = 1
    for name, _, _ in legs:
        out[name] = []
    for r in range(a.repeats + 1):                                # the first round is the warm-up of every leg
        for name, models, run in legs:
            if a.lib is None and models != loaded:
                e.load_ensemble(ws[:models])
                loaded = models
            rate = run()
            if r:
                out[name].append(round(rate))
    for name, _, _ in legs:
        out[name + "_median"] = float(np.median(out[name]))
    if a.lib is None:
        out["k1_over_plain"] = round(out["ensemble_k1_median"] / out["plain_median"], 4)
        out["k3_over_plain"] = round(out["ensemble_k3_median"] / out["plain_median"], 4)
    e.dataset_free(cd, cod)
    e.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
