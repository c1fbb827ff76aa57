#!/usr/bin/env python3
"""Float64 fixtures of the particles' path matrix (tests/test_gpu_particle_paths.py) for the cases whose reference is too slow to run
inside a test.  The project's own numpy code (tests/particles_numpy.py) on the CPU; the GPU box never regenerates them:

    python tests/golden/make_particle_fixtures.py 16384x64       # ~3 min
    python tests/golden/make_particle_fixtures.py 128x16384      # ~3 min
    python tests/golden/make_particle_fixtures.py 4096x4096      # ~4 min, 4 GiB
    python tests/golden/make_particle_fixtures.py 8192x8192      # ~10 min, 15 GiB

The grid, the noise amplitude and the step count are the case's row of particles_numpy.PATH_CASES.  A case without a fixture is only
measured (its figures are printed, for its row of the table).  Each run writes tests/golden/particles_<nx>x<ny>_step<steps>.npz:

  xy                     float64 [1000, 2]: ParticleModel64's positions after `steps` steps on particles_numpy.particle_inputs
  seed, vort_noise, steps, dt, nu     the case's parameters; the test rebuilds the inputs from them
  f32                    max |X_f32 - X_64| of the float32 restatement (particles_numpy.float32_positions), metres; the bar is 10 f32
  shift_masked, shift_base   the two sensitivity probes (ProbedParticleModel64): max shift of the positions, metres
  moved                  the largest displacement of a particle, metres
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]


def make(nx, ny):
    import particles_numpy as P
    from tracer_numpy import RECIPE_NU, recipe_dt
    case = P.path_case(nx, ny)
    t0 = time.time()
    r = P.path_figures(nx, ny, case.vort_noise, case.steps, progress=lambda k: print("step %d  %.0f s" % (k, time.time() - t0), flush=True))
    print("%dx%d, noise %g, %d steps (%.0f s): float32 %.3g m, probes %.3g (masked) / %.3g (base) m, moved %.3g m, finite %s"
          % (nx, ny, case.vort_noise, case.steps, time.time() - t0, r["f32"], r["masked"], r["base"], r["moved"], r["finite"]))
    if not case.fixture:
        return
    assert r["finite"]
    out = {"note": np.array("tests/particles_numpy.py ProbedParticleModel64 (float64, numpy rfft2/irfft2) on particle_inputs(%d, %d, %g), "
                            "%d steps; made by tests/golden/make_particle_fixtures.py" % (nx, ny, case.vort_noise, case.steps)),
           "xy": r["xy"], "seed": np.int64(P.PARTICLE_SEED), "vort_noise": np.float64(case.vort_noise), "steps": np.int64(case.steps),
           "dt": np.float64(recipe_dt(nx, ny)), "nu": np.float64(RECIPE_NU), "f32": np.float64(r["f32"]),
           "shift_masked": np.float64(r["masked"]), "shift_base": np.float64(r["base"]), "moved": np.float64(r["moved"])}
    np.savez_compressed(os.path.join(HERE, P.fixture_name(case)), **out)


if __name__ == "__main__":
    make(*(int(k) for k in sys.argv[1].split("x")))
