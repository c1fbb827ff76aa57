#!/usr/bin/env python3
"""Float64 fixtures of the tangent-linear model's path matrix (tests/test_gpu_tangent.py) for the cases whose reference is too slow to
run inside a test.  The project's own numpy code (tests/tangent_numpy.py) on the CPU; the GPU box never regenerates them:

    python tests/golden/make_tangent_fixtures.py 4096x4096       # ~1 min in three processes (reference and the two probes)
    python tests/golden/make_tangent_fixtures.py 16384x64        # ~3 min
    python tests/golden/make_tangent_fixtures.py 128x16384       # ~2 min

The grid, the noise amplitude and the step count are the case's row of tangent_numpy.PATH_CASES.  Each run writes
tests/golden/tangent_<nx>x<ny>_step<steps>.npz, in the format of the tracer's fixtures (make_tracer_fixtures.py):

  tangent_sub, vort_sub  TangentModel64 on tangent_numpy.tangent_inputs (never-dealiased noise on both fields, a vorticity source) after
                         `steps` steps, every sub[0]-th point in x and sub[1]-th in y, stored as float32 (3e-8 relative, against a bar
                         of 1e-5)
  tangent_l2, vort_l2    the full-field L2 norms sqrt(sum(f^2)) in float64
  seed, vort_noise, steps, dt, nu, sub     the recipe's parameters; the test rebuilds the inputs from them
  shift_vort, shift_tangent   the sensitivity probe: rel L2 of the perturbation of ProbeTangent64(blind_vort=True) / (blind_tangent=True)
                         against the unmodified run, over the full field.  Both must be >= 1e-4, ten times the parity bar.
  f32_tangent, f32_vort  the float32 torch restatement (tangent_numpy.float32_errors) against the same run; the first must be <= 2.5e-6
"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def fixture_path(nx, ny, steps):
    return os.path.join(HERE, "tangent_%dx%d_step%d.npz" % (nx, ny, steps))


def _run(job):
    import tangent_numpy as G
    nx, ny, noise, steps, blind = job
    v, d, s = G.tangent_inputs(nx, ny, noise)
    kw = {"cls": G.ProbeTangent64, blind: True} if blind else {}
    m = G.recipe_model(nx, ny, v, d, s, **kw)
    t0 = time.time()
    for k in range(steps):
        m.step(1)
        print("%s: step %d  %.0f s" % (blind or "reference", k + 1, time.time() - t0), flush=True)
    if blind:
        return m.tangent(), None, None
    return m.tangent(), m.vort(), G.float32_errors(nx, ny, v, d, s, steps, m)


def make(nx, ny):
    import tangent_numpy as G
    from ref_numpy import rel_l2
    import tracer_numpy as T
    case = [k for k in G.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]
    jobs = [(nx, ny, case.vort_noise, case.steps, b) for b in (None, "blind_vort", "blind_tangent")]
    with Pool(3) as pool:
        (tg, vo, f32), (tv, _, _), (tt, _, _) = pool.map(_run, jobs)
    sx, sy = max(1, nx // 256), max(1, ny // 256)
    out = {"note": np.array("tests/tangent_numpy.py TangentModel64 (float64, numpy rfft2/irfft2) on tangent_inputs(%d, %d, %g), %d steps; "
                            "made by tests/golden/make_tangent_fixtures.py" % (nx, ny, case.vort_noise, case.steps)),
           "tangent_sub": tg[::sx, ::sy].astype(np.float32), "vort_sub": vo[::sx, ::sy].astype(np.float32),
           "tangent_l2": np.float64(np.sqrt((tg * tg).sum())), "vort_l2": np.float64(np.sqrt((vo * vo).sum())),
           "seed": np.int64(G.SEED), "vort_noise": np.float64(case.vort_noise), "steps": np.int64(case.steps),
           "dt": np.float64(T.recipe_dt(nx, ny)), "nu": np.float64(G.NU), "sub": np.array([sx, sy], dtype=np.int64),
           "shift_vort": np.float64(rel_l2(tv, tg)), "shift_tangent": np.float64(rel_l2(tt, tg)),
           "f32_tangent": np.float64(f32[0]), "f32_vort": np.float64(f32[1])}
    np.savez_compressed(fixture_path(nx, ny, case.steps), **out)
    print("%dx%d, %d steps: probe shifts %.3g (vorticity's stage state), %.3g (perturbation's); float32 on the CPU %.3g / %.3g"
          % (nx, ny, case.steps, out["shift_vort"], out["shift_tangent"], f32[0], f32[1]))


if __name__ == "__main__":
    make(*(int(k) for k in sys.argv[1].split("x")))
