#!/usr/bin/env python3
"""Times of the point observations on one GPU by events on the engine's stream: Model.scatter and Model.observe at n = 2^20 and 2^24
random points, and one Model.fourdvar over `steps` steps with `times` observation times of u and v at 2^16 points each.  Per
configuration `reps` timings, warmed, interleaved; prints median [min, max] in ms, the scatter's atomic bytes per second (each
point adds to 16 cells, two 8-byte limbs each), and one JSON line.  DESIGN.md, "Point observations and the 4D-Var gradient", holds
the 1024^2 figures.  The times of scatter and observe include the host's hand-over (a wait for torch's stream before, for the
engine's after).

    python tools/fourdvar_time.py [--n 1024] [--steps 20] [--times 4] [--reps 10]
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
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--times", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    n = a.n
    v0 = X.make_field("elliptic", n)
    m = X.Model(n, n)
    m.set_vort(v0)
    g = torch.Generator(device="cuda").manual_seed(1)

    def points(k):
        return torch.rand((k, 2), dtype=torch.float64, device="cuda", generator=g) * 600000.0, torch.randn(k, dtype=torch.float64, device="cuda", generator=g)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    runs = {}
    for lg in (20, 24):
        xy, w = points(1 << lg)
        runs["scatter 2^%d" % lg] = lambda xy=xy, w=w: timed(lambda: m.scatter(w, xy))
        runs["observe 2^%d" % lg] = lambda xy=xy: timed(lambda: m.observe("u", xy))
    xy, w = points(1 << 16)
    when = [a.steps * (k + 1) // a.times for k in range(a.times)]
    obs = [X.Observations(s, kind, xy, w) for s in when for kind in ("u", "v")]
    runs["fourdvar"] = lambda: timed(lambda: m.fourdvar(v0, obs))
    runs["forward only"] = lambda: timed(lambda: (m.set_vort(v0), m.step(a.steps)))
    for f in runs.values():
        f()
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            ms[k].append(f())
    out = {"n": n, "steps": a.steps, "times": a.times, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
        rate = ""
        if k.startswith("scatter"):
            lg = int(k.split("^")[1])
            out[k]["atomic_GB_per_s"] = (1 << lg) * 16 * 2 * 8 / (out[k]["median_ms"] * 1e-3) / 1e9
            rate = "  %.0f GB/s of atomic adds" % out[k]["atomic_GB_per_s"]
        print("%-14s %.3f [%.3f, %.3f] ms%s" % (k, out[k]["median_ms"], v[0], v[-1], rate))
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
