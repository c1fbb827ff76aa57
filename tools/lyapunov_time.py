#!/usr/bin/env python3
"""Times of the tangent subspace on one GPU by events on the engine's stream: a plain step, a step with M = 1, 4 and 8 perturbations,
one orthonormalisation (fb_model_tangent_qr) at M = 4 and 8 and one norm (fb_model_tangent_norm).  Per configuration `reps` timings (of
`steps` steps each, or of one call), warmed, interleaved, in one process; prints median [min, max] in ms, the deviation of a step with
M perturbations from plain + M (tangent - plain), the QR's share of renorm_every = 10 steps, and one JSON line.  DESIGN.md, "Tangent
subspace and Lyapunov spectrum", holds the 4096^2 figures.

    python tools/lyapunov_time.py [--n 4096] [--steps 8] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1, 4, 8)
QR_COUNTS = (4, 8)
RENORM_EVERY = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    n, steps = a.n, a.steps
    v0 = X.make_field("elliptic", n)
    rng = np.random.default_rng(1)
    scale = 1e-3 * np.abs(v0).max()

    def timed(fn, per):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / per

    models = {0: X.Model(n, n)}
    models[0].set_vort(v0)
    for M in COUNTS:
        m = models[M] = X.Model(n, n)
        m.set_vort(v0)
        m.set_tangents(torch.from_numpy((scale * rng.standard_normal((M, n, n))).astype(np.float32)).cuda())
    r = torch.zeros(max(QR_COUNTS) ** 2, dtype=torch.float64, device="cuda")

    runs = {"plain": lambda: timed(lambda: models[0].step(steps), steps)}
    for M in COUNTS:
        runs["step_M%d" % M] = lambda M=M: timed(lambda: models[M].step(steps), steps)
    for M in QR_COUNTS:                                         # the engine's call alone: R stays on the device
        runs["qr_M%d" % M] = lambda M=M: timed(lambda: models[M]._call("tangent_qr", 0, B._ptr(r)), 1)
    runs["norm"] = lambda: timed(lambda: models[1]._call("tangent_norm", 0, B._ptr(r)), 1)     # of the one perturbation, as the QR's call
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            ms[k].append(f())
    out = {"n": n, "steps": steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
        print("%-10s %.3f [%.3f, %.3f] ms per %s" % (k, out[k]["median_ms"], v[0], v[-1], "step" if "step" in k or k == "plain" else "call"))
    plain, one = out["plain"]["median_ms"], out["step_M1"]["median_ms"]
    for M in COUNTS[1:]:
        got, want = out["step_M%d" % M]["median_ms"], plain + M * (one - plain)
        spread = out["step_M%d" % M]["max_ms"] - out["step_M%d" % M]["min_ms"]
        out["deviation_M%d" % M] = got - want
        print("step with %d perturbations: %.3f ms, plain + %d (tangent - plain) = %.3f ms, deviation %+.3f ms (%+.2f %%; spread of the run %.3f ms)"
              % (M, got, M, want, got - want, 100 * (got / want - 1), spread))
    for M in QR_COUNTS:
        qr, step = out["qr_M%d" % M]["median_ms"], out["step_M%d" % M]["median_ms"]
        out["qr_share_M%d" % M] = qr / (RENORM_EVERY * step)
        print("QR at M = %d: %.3f ms per call, %.2f %% of the %d steps it follows" % (M, qr, 100 * out["qr_share_M%d" % M], RENORM_EVERY))
    print(json.dumps(out))
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
