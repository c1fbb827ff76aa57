#!/usr/bin/env python3
"""Times of the Lagrangian observations on one GPU: a forward step with and without the particle tape (Model.time_steps, events on the
engine's stream), and Model.adjoint_back(1) with and without a particle adjoint (host clock around the call, the engine waited for
before and after), with the drifters in grid order and permuted (the gather of an unsorted set misses the caches: DESIGN.md,
"Lagrangian particles"); and, per step of a call of four, the captured step (use_graph) against the eager steps that the particle
tape makes of it.  Per configuration `reps` timings, warmed, interleaved; prints median [min, max] in ms and one JSON line
per grid.  DESIGN.md, "Lagrangian observations", holds the tables.

    python tools/lagrangian_time.py [--n 1024 4096] [--lg 16 20] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--lg", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    torch.cuda.set_stream(torch.cuda.Stream())                  # a captured step needs a stream of its own
    depth = 4 * (a.reps + WARM)
    for n in a.n:
        v0 = X.make_field("elliptic", n)
        lam = torch.from_numpy(v0).cuda()
        out = {"n": n, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        for lg in a.lg:
            k = 1 << lg
            side = 1 << (lg // 2)
            ij = np.stack(np.meshgrid(np.arange(side), np.arange(k // side), indexing="ij"), axis=-1).reshape(-1, 2)
            grid = (ij + 0.37) * np.array([600000.0 / side, 600000.0 / (k // side)])          # row-major: the order of the field in memory
            perm = np.random.default_rng(1).permutation(k)
            models, runs = [], {}

            def model(xy, tape, adjoint, particle_adjoint, graph=False):
                m = X.Model(n, n)
                if graph:                                       # (replayed only while neither tape is on)
                    m.fop.use_current_stream()
                    m.use_graph(True)
                m.set_vort(v0)
                if xy is not None:
                    m.set_particles(xy)
                if adjoint:
                    m.record_adjoint(a.reps + WARM)
                if tape:
                    m.record_particles(depth)
                if adjoint:
                    m.step(a.reps + WARM)
                    m.set_adjoint(lam)
                    if particle_adjoint:
                        m.set_particle_adjoint(np.random.default_rng(2).standard_normal((k, 2)))
                models.append(m)
                return m

            def back(m):
                m._wait()
                t0 = time.perf_counter()
                m.adjoint_back(1)
                m._wait()
                return (time.perf_counter() - t0) * 1e3

            for order, xy in (("grid order", grid), ("permuted", grid[perm])):
                plain, taped = model(xy, False, False, False), model(xy, True, False, False)
                runs["step, particles, %s" % order] = lambda m=plain: m.time_steps(1)
                runs["step, particles and tape, %s" % order] = lambda m=taped: m.time_steps(1)
                if order == "grid order":
                    captured, taped4 = model(xy, False, False, False, graph=True), model(xy, True, False, False, graph=True)
                    runs["4 steps, particles, use_graph, per step"] = lambda m=captured: m.time_steps(4) / 4
                    runs["4 steps, particles and tape (eager), per step"] = lambda m=taped4: m.time_steps(4) / 4
                with_pa = model(xy, True, True, True)
                runs["adjoint_back(1), particle adjoint, %s" % order] = lambda m=with_pa: back(m)
            none = model(None, False, True, False)
            runs["adjoint_back(1), no particles"] = lambda m=none: back(m)
            no_pa = model(grid, True, True, False)
            runs["adjoint_back(1), particles, no particle adjoint"] = lambda m=no_pa: back(m)
            for _ in range(WARM):
                for f in runs.values():
                    f()
            ms = {key: [] for key in runs}
            for _ in range(a.reps):
                for key, f in runs.items():
                    ms[key].append(f())
            print("%d^2, n = 2^%d drifters:" % (n, lg))
            for key, v in ms.items():
                v = sorted(v)
                out["2^%d, %s" % (lg, key)] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
                print("  %-55s %.3f [%.3f, %.3f] ms" % (key, float(np.median(v)), v[0], v[-1]))
            for m in models:
                m.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
