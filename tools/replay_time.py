#!/usr/bin/env python3
"""Times of the tangent replay on one GPU by events on the engine's stream.  At n1^2 (4096): ms per step of Model.tangent_replay for a
set of M = 1, 4 and 8 perturbations, beside the live tangent step of the same M (the step of the vorticity with the set riding along,
and that step less a plain one: the set's own share) and beside one Model.adjoint_back step of one variable, all in one process.  At
n2^2 (1024): one Model.gauss_newton_hvp beside one Model.fourdvar of the same window, the window of tools/fourdvar_time.py (`steps`
steps, `times` observation times of u and v at 2^16 points each).  Per configuration `reps` timings, warmed, interleaved; prints
median [min, max] in ms and one JSON line.  DESIGN.md, "Tangent replay and Gauss-Newton 4D-Var", holds the figures.

    python tools/replay_time.py [--n1 4096] [--tape 8] [--n2 1024] [--steps 20] [--times 4] [--reps 10]
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
    ap.add_argument("--n1", type=int, default=4096)
    ap.add_argument("--tape", type=int, default=8)
    ap.add_argument("--n2", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--times", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import xlab_fftbarotropic_amd as X

    def timed(fn, per=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / per

    def measure(runs):
        for f in runs.values():                                 # warm-up, in the order of the table
            f()
        ms = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, f in runs.items():
                ms[k].append(f())
        out = {}
        for k, v in ms.items():
            v = sorted(v)
            out[k] = {"median_ms": float(np.median(v)), "min_ms": v[0], "max_ms": v[-1]}
        return out

    out = {"n1": a.n1, "tape": a.tape, "n2": a.n2, "steps": a.steps, "times": a.times, "reps": a.reps, "device": torch.cuda.get_device_name(0)}

    # ---- the replayed step beside the live one and the backward one ----
    n, steps = a.n1, a.tape
    v0 = X.make_field("elliptic", n)
    rng = np.random.default_rng(1)
    d0 = (1e-3 * np.abs(v0).max() * rng.standard_normal((n, n))).astype(np.float32)
    sets = torch.from_numpy(np.stack([np.roll(d0, 97 * k, axis=0) for k in range(max(SET_COUNTS))])).cuda()
    plain, live, rec = X.Model(n, n), X.Model(n, n), X.Model(n, n)
    for m in (plain, live, rec):
        m.set_vort(v0)
    rec.record_adjoint(steps)
    rec.step(steps)                                             # the one forward run: every row below reads this tape

    def replayed(count):
        def run():
            rec.set_tangents(sets[:count])                      # outside the timing
            return timed(lambda: rec.tangent_replay(0, steps), steps)
        return run

    def stepped(count):
        def run():
            live.set_tangents(sets[:count])
            live.step(1)                                        # the eager step after a set call: outside the timing
            return timed(lambda: live.step(steps), steps)
        return run

    def backward():
        rec.adjoint_rewind(-1)
        rec.set_adjoint(d0)
        return timed(lambda: rec.adjoint_back(steps), steps)

    runs = {"plain": lambda: timed(lambda: plain.step(steps), steps)}
    for count in SET_COUNTS:
        runs["replay_%d" % count] = replayed(count)
        runs["live_%d" % count] = stepped(count)
    runs["backward"] = backward
    step_ms = measure(runs)
    out["step"] = step_ms
    for k, v in step_ms.items():
        print("%-12s %.3f [%.3f, %.3f] ms per step" % (k, v["median_ms"], v["min_ms"], v["max_ms"]))
    base = step_ms["plain"]["median_ms"]
    for count in SET_COUNTS:
        r, lv = step_ms["replay_%d" % count]["median_ms"], step_ms["live_%d" % count]["median_ms"] - base
        print("M = %d: replay %.3f ms, the live set's share of its step %.3f ms, ratio %.3f (the field count: %.3f)"
              % (count, r, lv, r / lv, (4 + 5 * count) / (10.0 * count)))
    for m in (plain, live, rec):
        m.close()

    # ---- one Hessian-vector product beside one cost gradient ----
    n = a.n2
    v0 = X.make_field("elliptic", n)
    d0 = (1e-3 * np.abs(v0).max() * np.random.default_rng(2).standard_normal((n, n))).astype(np.float32)
    m = X.Model(n, n)
    g = torch.Generator(device="cuda").manual_seed(1)
    xy = torch.rand((1 << 16, 2), dtype=torch.float64, device="cuda", generator=g) * 600000.0
    w = torch.randn(1 << 16, dtype=torch.float64, device="cuda", generator=g)
    when = [a.steps * (k + 1) // a.times for k in range(a.times)]
    obs = [X.Observations(s, kind, xy, w) for s in when for kind in ("u", "v")]
    dv = torch.from_numpy(d0).cuda()
    runs = {"fourdvar": lambda: timed(lambda: m.fourdvar(v0, obs, keep_tape=True)),
            "gauss_newton_hvp": lambda: timed(lambda: m.gauss_newton_hvp(dv, obs))}
    hvp_ms = measure(runs)
    m.record_adjoint(0)
    out["window"] = hvp_ms
    for k, v in hvp_ms.items():
        print("%-17s %.3f [%.3f, %.3f] ms" % (k, v["median_ms"], v["min_ms"], v["max_ms"]))
    print(json.dumps(out))
    m.close()


if __name__ == "__main__":
    main()
