#!/usr/bin/env python3
"""Times of the adjoint model on one GPU by events on the engine's stream: a plain step, a step with a tangent, a step that records
the adjoint's tape, one backward step (Model.adjoint_back(1)), and one backward step of an adjoint set of M = 1, 4 and 8 variables
(Model.set_adjoints; the rows are left out on a library that predates the set, as FFTBARO_LIB may name).  Per configuration `reps`
timings of `steps` steps each, warmed, interleaved; prints median [min, max] in ms per step and one JSON line.  DESIGN.md, "Adjoint
model" and "Adjoint subspace", holds the 4096^2 figures.

    python tools/adjoint_time.py [--n 4096] [--steps 8] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


SET_COUNTS = (1, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    n, steps = a.n, a.steps
    v0 = X.make_field("elliptic", n)
    rng = np.random.default_rng(1)
    d0 = (1e-3 * np.abs(v0).max() * rng.standard_normal((n, n))).astype(np.float32)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    plain, tangent, rec = X.Model(n, n), X.Model(n, n), X.Model(n, n)
    for m in (plain, tangent, rec):
        m.set_vort(v0)
    tangent.set_tangent(d0)
    rec.record_adjoint(steps)
    rec.set_adjoint(d0)

    def rec_forward():
        rec.record_adjoint(steps)                               # an empty tape, the allocation reused by the allocator or not: outside the timing
        return timed(lambda: rec.step(steps))

    def set_backward(count):
        def run():
            rec.record_adjoint(steps)                           # refill the tape and set the variables: outside the timing
            rec.step(steps)
            rec.set_adjoints(lams[:count])
            return timed(lambda: rec.adjoint_back(steps))
        return run

    def backward():
        rec.set_adjoint(d0)                                     # the one variable, whatever set the rows below left
        return timed(lambda: rec.adjoint_back(steps))

    runs = {"plain": lambda: timed(lambda: plain.step(steps)), "tangent": lambda: timed(lambda: tangent.step(steps)), "recording": rec_forward,
            "backward": backward}
    if hasattr(X.lib(), "fb_model_set_adjoints"):
        lams = torch.from_numpy(np.stack([np.roll(d0, 97 * k, axis=0) for k in range(max(SET_COUNTS))])).cuda()
        for count in SET_COUNTS:
            runs["backward_set_%d" % count] = set_backward(count)
    for f in runs.values():                                     # warm-up, in the order that leaves a full tape for "backward"
        f()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            ms[k].append(f())
    out = {"n": n, "steps": steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
        print("%-14s %.3f [%.3f, %.3f] ms per step" % (k, out[k]["median_ms"], v[0], v[-1]))
    print("recording overhead per forward step: %.3f ms" % (out["recording"]["median_ms"] - out["plain"]["median_ms"]))
    print(json.dumps(out))
    for m in (plain, tangent, rec):
        m.close()


if __name__ == "__main__":
    main()
