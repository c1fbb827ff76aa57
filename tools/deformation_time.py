#!/usr/bin/env python3
"""Times of the particles' deformation gradient on one GPU: ms per step (fb_model_time_steps, graph replay) of a plain step, a step
with particles and a step with particles that carry F, for 2^20 particles seeded on a 1024^2 lattice in grid order and randomly
permuted, and one call of fb_model_particle_stretching on the model's own F.  Per configuration `reps` timings of `steps` steps each,
warmed, interleaved, in one process; prints median [min, max] and one JSON line.  The per-kernel times of k_particle_stage_def<0..3>
against k_particle_stage<0..3> come from a kernel trace of a run of this tool with one order and few repeats:

    python tools/deformation_time.py [--n 4096] [--lattice 1024] [--steps 20] [--reps 5] [--order both|grid|permuted]
    rocprofv3 --kernel-trace --stats -d OUT -o t --output-format csv -- python tools/deformation_time.py --order grid --reps 2

DESIGN.md, "Particle deformation and FTLE", holds the 4096^2 figures.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--lattice", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--order", choices=("both", "grid", "permuted"), default="both")
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    n, q = a.n, a.lattice
    L = float(np.float32(600000.0))
    v0 = X.make_field("kuo2004", n)
    g = (np.arange(q) + 0.5) * (L / q)
    lattice = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    orders = {"grid": lattice, "permuted": lattice[np.random.default_rng(1).permutation(lattice.shape[0])]}
    if a.order != "both":
        orders = {a.order: orders[a.order]}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        def model(xy, deformation):
            m = X.Model(n, n, dt=3.0 * min(1.0, 1024.0 / n))
            m.use_graph(True)
            m.set_vort(v0)
            if xy is not None:
                m.set_particles(xy)
            if deformation:
                m.set_particle_deformation()
            m.step(3)                                           # the eager step, the capture, one replay
            return m
        models = {"plain": model(None, False)}
        for name, xy in orders.items():
            models["particles_" + name] = model(xy, False)
            models["deformation_" + name] = model(xy, True)
        ms = {k: [] for k in models}
        for _ in range(a.reps):
            for k, m in models.items():
                ms[k].append(m.time_steps(a.steps) / a.steps)
        out = {"n": n, "particles": int(lattice.shape[0]), "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        for k, v in ms.items():
            v = sorted(v)
            out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
            print("%-22s %.3f [%.3f, %.3f] ms per step" % (k, out[k]["median_ms"], v[0], v[-1]))
        for name in orders:
            d = out["deformation_" + name]["median_ms"] - out["particles_" + name]["median_ms"]
            out["added_ms_" + name] = d
            print("F along the particles, %s order: %+.3f ms per step (%+.1f %% of the step with particles)" % (name, d, 100 * d / out["particles_" + name]["median_ms"]))
        m = models["deformation_" + next(iter(orders))]
        table = torch.empty((lattice.shape[0], 4), dtype=torch.float64, device="cuda")
        sv = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            m.fop.synchronize()
            e0.record()
            m._call("particle_stretching", None, 0, B._ptr(table))
            e1.record()
            e1.synchronize()
            sv.append(e0.elapsed_time(e1))
        out["stretching_ms"] = float(np.median(sv[1:]))
        print("particle_stretching of %d matrices: %.3f ms per call" % (lattice.shape[0], out["stretching_ms"]))
        print(json.dumps(out))
        for m in models.values():
            m.close()


if __name__ == "__main__":
    main()
