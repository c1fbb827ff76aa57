#!/usr/bin/env python3
"""Float64 fixtures of the tracer's path matrix (tests/test_gpu_tracer_paths.py) for the cases whose reference is too slow to run inside
a test.  The project's own numpy code (tests/tracer_numpy.py) on the CPU; the GPU box never regenerates them:

    python tests/golden/make_tracer_fixtures.py 4096x4096        # ~1 min in three processes (reference and the two probes)
    python tests/golden/make_tracer_fixtures.py 8192x8192        # ~4 min, a few GiB per process
    python tests/golden/make_tracer_fixtures.py 16384x64         # ~2 min
    python tests/golden/make_tracer_fixtures.py 128x16384        # ~2 min

The grid, the noise amplitude and the step count are the case's row of tracer_numpy.PATH_CASES.  Each run writes
tests/golden/tracer_<nx>x<ny>_step<steps>.npz (the square 4096 grid: tracer_4096_step3.npz):

  tracer_sub, vort_sub   TracerModel64 on tracer_numpy.noisy_inputs (never-dealiased noise on both fields, a vorticity source) after
                         `steps` steps, every sub[0]-th point in x and sub[1]-th in y, stored as float32 (3e-8 relative, against a bar
                         of 1e-5)
  tracer_l2, vort_l2     the full-field L2 norms sqrt(sum(f^2)) in float64
  seed, vort_noise, steps, dt, kappa, nu, sub     the recipe's parameters; the test rebuilds the inputs from them
  shift_vort, shift_tracer   the sensitivity probe: rel L2 of the tracer of ProbeModel64(blind_vort=True) / (blind_tracer=True) against
                         the unmodified run, over the full field.  Both must be >= 1e-4, ten times the parity bar.
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
    return os.path.join(HERE, "tracer_4096_step%d.npz" % steps if nx == ny == 4096 else "tracer_%dx%d_step%d.npz" % (nx, ny, steps))


def _run(job):
    import tracer_numpy as T
    nx, ny, noise, steps, blind = job
    v, c, s = T.noisy_inputs(nx, ny, noise)
    kw = {"cls": T.ProbeModel64, blind: True} if blind else {}
    m = T.recipe_model(nx, ny, v, c, s, **kw)
    t0 = time.time()
    for k in range(steps):
        m.step(1)
        print("%s: step %d  %.0f s" % (blind or "reference", k + 1, time.time() - t0), flush=True)
    return m.tracer(), (m.vort() if not blind else None)


def make(nx, ny):
    import tracer_numpy as T
    from ref_numpy import rel_l2
    case = [k for k in T.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]
    jobs = [(nx, ny, case.vort_noise, case.steps, b) for b in (None, "blind_vort", "blind_tracer")]
    with Pool(3) as pool:
        (tr, vo), (tv, _), (tt, _) = pool.map(_run, jobs)
    sx, sy = max(1, nx // 256), max(1, ny // 256)
    out = {"note": np.array("tests/tracer_numpy.py TracerModel64 (float64, numpy rfft2/irfft2) on noisy_inputs(%d, %d, %g), %d steps; "
                            "made by tests/golden/make_tracer_fixtures.py" % (nx, ny, case.vort_noise, case.steps)),
           "tracer_sub": tr[::sx, ::sy].astype(np.float32), "vort_sub": vo[::sx, ::sy].astype(np.float32),
           "tracer_l2": np.float64(np.sqrt((tr * tr).sum())), "vort_l2": np.float64(np.sqrt((vo * vo).sum())),
           "seed": np.int64(T.RECIPE_SEED), "vort_noise": np.float64(case.vort_noise), "steps": np.int64(case.steps),
           "dt": np.float64(T.recipe_dt(nx, ny)), "kappa": np.float64(T.RECIPE_KAPPA), "nu": np.float64(T.RECIPE_NU),
           "sub": np.array([sx, sy], dtype=np.int64),
           "shift_vort": np.float64(rel_l2(tv, tr)), "shift_tracer": np.float64(rel_l2(tt, tr))}
    np.savez_compressed(fixture_path(nx, ny, case.steps), **out)
    print("%dx%d, %d steps: probe shifts %.3g (vorticity's stage state), %.3g (tracer's)" % (nx, ny, case.steps, out["shift_vort"], out["shift_tracer"]))


if __name__ == "__main__":
    make(*(int(k) for k in sys.argv[1].split("x")))
