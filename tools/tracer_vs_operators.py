#!/usr/bin/env python3
"""The fused tracer step against the only alternative: the coupled RK4 step of vorticity and tracer composed from the operator ABI
(fb_gradx, fb_grady, fb_invert_laplacian, fb_laplacian, fb_c2r, fb_jacobian, fb_r2c, fb_spec_axpy, fb_spec_evolve, fb_spec_rk4_combine,
fb_dealiase), which is all a library without fb_model_set_tracer offers.

    tools/tracer_vs_operators.py [N] [--steps K] [--operators-lib libfftbaro.so of another build]

The composition runs in a process of its own on the library named by --operators-lib (default: this build's; the operator entry points
are the same), and Model.set_tracer + step of this build in a second one after it; each runs under the time limit of --timeout seconds
and leaves its tracer after K steps in a file.  This process touches no GPU: it starts the two, one after the other, the second only
if the first ended well, and prints one JSON line: ms per step of both (HIP events, median of 20 after warm-up), their ratio, and the
relative L2 difference of the two tracers after K steps (bar: 1e-5)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NU, KAPPA, DT = 6.5, 20.0, 3.0


def fields(n):
    import xlab_fftbarotropic_amd as X
    v0 = X.make_field("kuo2004", n)
    g = X.make_field("gaussian", n)
    return v0, np.ascontiguousarray(np.roll(np.roll(g, n // 4, axis=0), n // 8, axis=1))


def child(n, steps, out):
    import torch
    import xlab_fftbarotropic_amd as X
    fop = X.FftwfOperation(n, n, 600000.0, 600000.0)
    v0, c0 = fields(n)
    S, R = fop.empty_spec, fop.empty_real
    vc, cc = fop.r2c(torch.from_numpy(v0).cuda()), fop.r2c(torch.from_numpy(c0).cuda())
    tmp, psi, lap = S(), S(), S()
    u, v, ax, ay, jr = R(), R(), R(), R(), R()
    kv, kc = [S() for _ in range(4)], [S() for _ in range(4)]
    sv, sc = S(), S()

    def tend(z, a, coef, out_k):
        """out_k = dealiase(r2c(-u a_x - v a_y) + coef laplacian(a)), u, v from psi = invertLaplacian(z) (already in u, v)"""
        fop.gradx(a, tmp); fop.c2r(tmp, ax, normalize=True)
        fop.grady(a, tmp); fop.c2r(tmp, ay, normalize=True)
        fop.jacobian(u, v, ax, ay, None, jr)
        fop.r2c(jr, out_k)
        fop.laplacian(a, lap)
        fop.spec_axpy(out_k, lap, coef)
        fop.dealiase(out_k, out_k)

    def stage(z, a, k):
        fop.invertLaplacian(z, psi)
        fop.grady(psi, tmp); fop.c2r(tmp, u, normalize=True); fop.negate(u)
        fop.gradx(psi, tmp); fop.c2r(tmp, v, normalize=True)
        tend(z, z, NU, kv[k])
        tend(z, a, KAPPA, kc[k])

    def step():
        nonlocal vc, cc
        stage(vc, cc, 0)
        for k, h in ((1, DT / 2), (2, DT / 2), (3, DT)):
            fop.spec_evolve(vc, kv[k - 1], h, sv); fop.spec_evolve(cc, kc[k - 1], h, sc)
            stage(sv, sc, k)
        fop.spec_rk4_combine(vc, kv[0], kv[1], kv[2], kv[3], DT, vc)
        fop.spec_rk4_combine(cc, kc[0], kc[1], kc[2], kc[3], DT, cc)

    for _ in range(steps):
        step()
    np.save(out, fop.c2r(cc.clone(), normalize=True).cpu().numpy())
    for _ in range(5):
        step()
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); step(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"operators_ms_per_step": sorted(ms)[10]}))


def fused_child(n, steps, out):
    import xlab_fftbarotropic_amd as X
    v0, c0 = fields(n)
    m = X.Model(n, n, nu=NU, dt=DT)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=KAPPA)
    m.step(steps)
    np.save(out, m.tracer().cpu().numpy())
    m.step(20)
    k = max(1, 200 * 1024 * 1024 // (n * n) // 10)
    fused = sorted(m.time_steps(k) / k for _ in range(20))[10]
    m.set_tracer(None)
    m.step(5)
    plain = sorted(m.time_steps(k) / k for _ in range(20))[10]
    print(json.dumps({"fused_ms_per_step": fused, "plain_ms_per_step": plain}))


def run_child(a, leg, out, env):
    """one leg in a fresh process under the time limit; its last stdout line is its JSON"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.n), "--steps", str(a.steps), "--child", out, "--leg", leg],
                       env=env, stdout=subprocess.PIPE, timeout=a.timeout, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--operators-lib", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--leg", choices=("operators", "fused"), default="operators")
    ap.add_argument("--timeout", type=int, default=240, help="seconds, for each of the two GPU processes")
    a = ap.parse_args()
    if a.child:
        return (child if a.leg == "operators" else fused_child)(a.n, a.steps, a.child)
    with tempfile.TemporaryDirectory() as d:
        ref_f, got_f = os.path.join(d, "operators.npy"), os.path.join(d, "fused.npy")
        env = dict(os.environ)
        if a.operators_lib:
            env["FFTBARO_LIB"] = os.path.abspath(a.operators_lib)
        res = run_child(a, "operators", ref_f, env)
        res.update(run_child(a, "fused", got_f, dict(os.environ)))     # only if the first leg ended well
        ref, got = np.load(ref_f), np.load(got_f)
    err = float(np.linalg.norm((got - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))
    fused, plain = res["fused_ms_per_step"], res["plain_ms_per_step"]
    res.update({"n": a.n, "steps": a.steps, "tracer_over_plain": fused / plain,
                "operators_over_fused": res["operators_ms_per_step"] / fused, "rel_l2_tracer": err, "agree_1e-5": err <= 1e-5})
    print(json.dumps(res))
    return 0 if (err <= 1e-5 and fused < res["operators_ms_per_step"]) else 1


if __name__ == "__main__":
    sys.exit(main())
