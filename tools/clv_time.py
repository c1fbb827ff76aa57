#!/usr/bin/env python3
"""Times of the covariant Lyapunov vectors' two field-moving calls on one GPU by events on the engine's stream: one push of the bases
into the tape (fb_model_tangent_tape_push) and one combination V = Q C (fb_model_tangent_combine), in place and from a tape slot, at
M = 4 and 8 perturbations.  Per configuration `reps` timings of one call, warmed, interleaved, in one process; prints median [min, max]
in ms, the bytes moved (push: M half spectra read and M written; combination: the same, 2 M half spectra whatever C holds) and the
TB/s, beside the 6.29 TB/s of a device-to-device copy and the 5.1-5.6 TB/s of the QR's kernels, and one JSON line.  DESIGN.md,
"Covariant Lyapunov vectors", holds the 4096^2 figures.

    python tools/clv_time.py [--n 4096] [--reps 10] [--counts 4,8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS, QR_TBS = 6.29, (5.1, 5.6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--counts", default="4,8")
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    n = a.n
    counts = tuple(int(c) for c in a.counts.split(","))
    v0 = X.make_field("elliptic", n)
    rng = np.random.default_rng(1)
    scale = 1e-3 * np.abs(v0).max()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    models, coef, base_bytes = {}, {}, {}
    for M in counts:
        m = models[M] = X.Model(n, n)
        m.set_vort(v0)
        m.set_tangents(torch.from_numpy((scale * rng.standard_normal((M, n, n))).astype(np.float32)).cuda())
        m.orthonormalize_tangents()
        h0 = m.info()["hbm_bytes"]
        m.tangent_tape(1)
        base_bytes[M] = (m.info()["hbm_bytes"] - h0) // M       # one half spectrum in the engine's padded layout
        m.push_tangents()
        c = np.triu(rng.standard_normal((M, M))) + 2 * np.eye(M)
        coef[M] = torch.from_numpy(c / np.linalg.norm(c, axis=0)).cuda()      # (unit columns: repeated in-place combinations stay finite for a while)
    torch.cuda.synchronize()

    def push(M):
        models[M].tangent_tape(1)                               # (an empty tape again; its allocation is outside the events)
        models[M]._wait()
        return timed(lambda: models[M]._call("tangent_tape_push"))

    runs = {}
    for M in counts:
        runs["push_M%d" % M] = lambda M=M: push(M)
        runs["combine_slot_M%d" % M] = lambda M=M: timed(lambda: models[M]._call("tangent_combine", 0, B._ptr(coef[M])))
        runs["combine_inplace_M%d" % M] = lambda M=M: timed(lambda: models[M]._call("tangent_combine", -1, B._ptr(coef[M])))
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            ms[k].append(f())
    out = {"n": n, "reps": a.reps, "device": torch.cuda.get_device_name(0), "base_bytes": {str(k): v for k, v in base_bytes.items()}}
    for k, v in ms.items():
        v = sorted(v)
        M = int(k.rsplit("M", 1)[1])
        moved = 2 * M * base_bytes[M]
        med = float(np.median(v))
        out[k] = {"median_ms": med, "min_ms": v[0], "max_ms": v[-1], "bytes": moved, "tb_per_s": moved / (med * 1e-3) / 1e12}
        print("%-20s %.3f [%.3f, %.3f] ms per call, %.1f MB moved, %.2f TB/s (a copy: %.2f TB/s; the QR's kernels: %.1f-%.1f TB/s)"
              % (k, med, v[0], v[-1], moved / 1e6, out[k]["tb_per_s"], COPY_TBS, QR_TBS[0], QR_TBS[1]))
    print(json.dumps(out))
    for m in models.values():
        m.close()


if __name__ == "__main__":
    main()
