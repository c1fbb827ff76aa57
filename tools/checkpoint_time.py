#!/usr/bin/env python3
"""Times of adjoint checkpointing on one GPU by events on the engine's stream, against the full tape in the same process: a plain
step, a forward step that records the full tape, a forward step in checkpoint mode (K = 8), each of the plain and the checkpointed
one without and with use_graph; a backward step from the full tape, and a backward step in checkpoint mode at K = 8 and at
K = checkpoint_every(steps), which takes every step of the window again once.  Per configuration `reps` timings of `steps` steps
each, warmed, interleaved; whatever sets a configuration up (the mode on, the forward run before a sweep) is outside its timing.
Prints median [min, max] in ms per step, the two ratios and one JSON line.  DESIGN.md, "Adjoint checkpointing", holds the 4096^2
figures.  `steps` must be a window whose full tape fits (271 MB per step at 4096^2).

    python tools/checkpoint_time.py [--n 4096] [--steps 32] [--reps 10]
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
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X
    n, steps = a.n, a.steps
    k_sqrt = X.checkpoint_every(steps)
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

    with torch.cuda.stream(torch.cuda.Stream()):                # a stream of its own: use_graph needs one, and the events share it
        names = ("plain", "plain_graph", "tape", "ck", "ck_graph")
        m = {k: X.Model(n, n) for k in names}
        for k, mod in m.items():
            mod.fop.use_current_stream()
            mod.use_graph(k.endswith("_graph"))
            mod.set_vort(v0)
        for k in ("tape", "ck"):
            m[k].set_adjoint(d0)

        def forward_tape():
            m["tape"].record_adjoint(steps)                     # an empty tape
            return timed(lambda: m["tape"].step(steps))

        def forward_ck(name):
            def run():
                m[name].checkpoint_adjoint(8, steps)            # an empty window
                return timed(lambda: m[name].step(steps))
            return run

        def backward_tape():
            m["tape"].record_adjoint(steps)
            m["tape"].step(steps)
            m["tape"].set_adjoint(d0)
            return timed(lambda: m["tape"].adjoint_back(steps))

        def backward_ck(every):
            def run():
                m["ck"].checkpoint_adjoint(every, steps)
                m["ck"].step(steps)
                m["ck"].set_adjoint(d0)
                t = timed(lambda: m["ck"].adjoint_back(steps))
                assert m["ck"].adjoint_checkpoints()[3] == steps
                return t
            return run

        runs = {"plain": lambda: timed(lambda: m["plain"].step(steps)), "plain_graph": lambda: timed(lambda: m["plain_graph"].step(steps)),
                "forward_tape": forward_tape, "forward_ck8": forward_ck("ck"), "forward_ck8_graph": forward_ck("ck_graph"),
                "backward_tape": backward_tape, "backward_ck8": backward_ck(8), "backward_ck%d" % k_sqrt: backward_ck(k_sqrt)}
        for f in runs.values():                                 # warm-up
            f()
        ms = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, f in runs.items():
                ms[k].append(f())
        out = {"n": n, "steps": steps, "reps": a.reps, "checkpoint_every": k_sqrt, "device": torch.cuda.get_device_name(0)}
        for k, v in ms.items():
            v = sorted(v)
            out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
            print("%-18s %.3f [%.3f, %.3f] ms per step" % (k, out[k]["median_ms"], v[0], v[-1]))
        med = {k: out[k]["median_ms"] for k in ms}
        out["forward_ratio"] = med["forward_ck8"] / med["plain"]
        out["forward_graph_ratio"] = med["forward_ck8_graph"] / med["plain_graph"]
        out["forward_tape_ratio"] = med["forward_tape"] / med["plain"]
        out["backward_ratio_8"] = med["backward_ck8"] / med["backward_tape"]
        out["backward_ratio_sqrt"] = med["backward_ck%d" % k_sqrt] / med["backward_tape"]
        print("forward step, checkpoint mode over plain: %.3f (use_graph: %.3f); full tape over plain: %.3f"
              % (out["forward_ratio"], out["forward_graph_ratio"], out["forward_tape_ratio"]))
        print("backward step, checkpoint mode over full tape: K = 8 %.3f, K = %d %.3f" % (out["backward_ratio_8"], k_sqrt, out["backward_ratio_sqrt"]))
        print(json.dumps(out))
        for mod in m.values():
            mod.close()


if __name__ == "__main__":
    main()
