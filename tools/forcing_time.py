#!/usr/bin/env python3
"""Times of the split stage (Model.set_forcing: stochastic ring forcing, linear drag, hyperviscosity) on one GPU by events on the
engine's stream.  Per grid n^2 (1024 and 4096): ms per step of a model with forcing, drag and nabla^8 hyperviscosity all on, beside the
plain step of the same build and beside a model with drag alone (no ring, no trigonometry), all in one process.  Per configuration
`reps` timings of `steps` steps, warmed, interleaved; prints median [min, max] in ms and one JSON line.  DESIGN.md, "Stochastic forcing,
drag and hyperviscosity", holds the figures.

    python tools/forcing_time.py [--grids 1024,4096] [--steps 20] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K1 = 2.0 * np.pi / 600000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="1024,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    out = {"steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0), "grids": {}}
    for n in (int(k) for k in a.grids.split(",")):
        dt = 3.0 * min(1.0, 1024.0 / n)
        v0 = X.make_field("elliptic", n)
        kmax2 = 2.0 * np.ceil(n / 3.0) ** 2 * K1 * K1
        hyper = dict(hyper_nu=0.3 / (dt * kmax2 ** 4), hyper_order=4)
        models = {"plain": {}, "drag": dict(drag=1e-3), "forced": dict(rate=1e-3, k=33.0 * K1, width=2.0 * K1, seed=1, drag=1e-3, **hyper)}
        ms = {}
        for name, kw in models.items():
            m = X.Model(n, n, dt=dt)
            m.set_vort(v0)
            if kw:
                m.set_forcing(**kw)
            m.step(a.steps)                                     # warm-up, in the order of the table
            models[name], ms[name] = m, []
        for _ in range(a.reps):
            for name, m in models.items():
                ms[name].append(m.time_steps(a.steps) / a.steps)
        res = {}
        for name, v in ms.items():
            v = sorted(v)
            res[name] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
            print("%5d^2 %-7s %.4f [%.4f, %.4f] ms per step" % (n, name, res[name]["median_ms"], v[0], v[-1]))
        res["hbm_bytes"] = {name: m.info()["hbm_bytes"] for name, m in models.items()}
        base = res["plain"]["median_ms"]
        print("%5d^2: the split stage costs %.4f ms per step with everything on (%.1f %% of the plain step), %.4f ms with drag alone; memory + %d bytes"
              % (n, res["forced"]["median_ms"] - base, 100.0 * (res["forced"]["median_ms"] / base - 1), res["drag"]["median_ms"] - base,
                 res["hbm_bytes"]["forced"] - res["hbm_bytes"]["plain"]))
        out["grids"][str(n)] = res
        for m in models.values():
            m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
