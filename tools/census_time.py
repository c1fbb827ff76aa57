#!/usr/bin/env python3
"""Times of the vortex census on one GPU: the median of `reps` calls of fb_model_census under HIP events, per grid, on two fields -- the
Kuo2004 vorticity with a threshold of a tenth of its maximum, and Bernoulli noise at p = 0.59, the percolation worst case -- beside one
field record (fb_model_get_vort) and the azimuthal record (fb_model_get_azimuthal, default bins) of the same grid.  Prints one line
per grid and field and one JSON line.  The per-kernel times come from a kernel trace of a run of its own:

    python tools/census_time.py [--sizes 1024,4096,16384] [--reps 20]
    rocprofv3 --kernel-trace --stats -d OUT -o t --output-format csv -- python tools/census_time.py --sizes 4096 --reps 5

(7 calls at 16384^2 whatever --reps says.)  DESIGN.md, "Vortex census", holds the figures.
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
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "grids": {}}
    with torch.cuda.stream(torch.cuda.Stream()):
        run(a, torch, X, B, out)
    print(json.dumps(out))


def run(a, torch, X, B, out):
    """everything on one stream: the engine is put on torch's current stream, so the events bracket the engine's own work in stream
    order and no host synchronisation lies inside a timed interval"""
    for n in [int(s) for s in a.sizes.split(",")]:
        reps = min(a.reps, 7) if n >= 16384 else a.reps
        m = X.Model(n, n)
        m.fop.use_current_stream()
        v0 = X.make_field("kuo2004", n)
        m.set_vort(v0)
        zeta = m.vort()
        noise = (torch.rand((n, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) < 0.59).float()
        table = torch.empty((1024, 12), dtype=torch.float64, device="cuda")
        count = torch.empty(2, dtype=torch.int32, device="cuda")
        mode, xc, yc, nbins, dr = B.azimuthal_args(n, n, m.Lx, m.Ly, "psi-min", None, None)
        atab = torch.empty((nbins, 20), dtype=torch.float64, device="cuda")
        acen = torch.empty(4, dtype=torch.float64, device="cuda")
        field = torch.empty((n, n), dtype=torch.float32, device="cuda")
        thr = 0.1 * float(v0.max())
        calls = {
            "census_kuo2004": lambda: m._call("census", B._ptr(zeta), None, 0, thr, 1, 1024, B._ptr(table), B._ptr(count), None),
            "census_bernoulli": lambda: m._call("census", B._ptr(noise), B._ptr(zeta), 0, 0.5, 1, 1024, B._ptr(table), B._ptr(count), None),
            "get_vort": lambda: m._call("get_vort", B._ptr(field)),
            "get_azimuthal": lambda: m._call("get_azimuthal", mode, xc, yc, nbins, dr, 4, B._ptr(atab), B._ptr(acen)),
        }
        torch.cuda.synchronize()
        res = {}
        for name, call in calls.items():
            ms = []
            for _ in range(reps + 1):                           # the first call allocates and warms: dropped
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            ms = sorted(ms[1:])
            res[name] = {"median_ms": float(np.median(ms)), "min_ms": ms[0], "max_ms": ms[-1]}
            if name.startswith("census"):
                res[name]["found"], res[name]["structures"] = (int(x) for x in count.cpu())
        for name in ("census_kuo2004", "census_bernoulli"):
            r = res[name]
            print("%5d^2 %-17s %8.3f [%.3f, %.3f] ms, %d structures; %.1f field records, %.2f azimuthal records" % (
                n, name, r["median_ms"], r["min_ms"], r["max_ms"], r["structures"], r["median_ms"] / res["get_vort"]["median_ms"],
                r["median_ms"] / res["get_azimuthal"]["median_ms"]))
        print("%5d^2 get_vort %.3f ms, get_azimuthal %.3f ms" % (n, res["get_vort"]["median_ms"], res["get_azimuthal"]["median_ms"]))
        out["grids"][str(n)] = res
        m.close()
        del zeta, noise, field
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
