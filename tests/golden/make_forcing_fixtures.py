#!/usr/bin/env python3
"""Float64 fixture of the split stage's path matrix (tests/test_gpu_forcing.py) for the grid whose reference is too slow to run inside
a test: 4096^2, the grid of k_col_full's state layout.  The project's own numpy code (tests/forcing_numpy.py) on the CPU; the GPU box
never regenerates it:

    python tests/golden/make_forcing_fixtures.py        # a few minutes in three processes (reference and the two probes)

It writes tests/golden/forcing_4096x4096_step3.npz, in the format of the tracer's fixtures (make_tracer_fixtures.py):

  vort_sub            ForcedModel64 on tracer_numpy.noisy_vort (never-dealiased noise, no source) with the forcing, drag and nabla^8
                      hyperviscosity of forcing_numpy.case_forcing after `steps` steps, every sub[0]-th point in x and sub[1]-th in y,
                      stored as float32 (3e-8 relative, against a bar of 1e-5)
  vort_l2             the full-field L2 norm sqrt(sum(f^2)) in float64
  dE_forc, dE_diss, dZ_forc, dZ_diss, n_ring      the float64 budget of the run
  seed, vort_noise, steps, dt, nu, sub, rate, k, width, forcing_seed, drag, hyper_nu, hyper_order     the recipe; the test rebuilds the inputs from them
  shift_conj, shift_clock   the sensitivity probes: rel L2 of the vorticity of a run whose forcing omits the conjugate rule on j = 0 and
                      j = ny/2, and of a run whose forcing clock stays at 0, against the unmodified run, over the full field.  Both must
                      be >= 1e-4, ten times the parity bar.
"""
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

NX = NY = 4096
STEPS = 3
NOISE = 3e-2


def _case():
    import forcing_numpy as F
    return F.ForcingCase(NX, NY, STEPS, F.RATE, F.RING_K, F.RING_WIDTH, 0.0, 0.0)


def _run(probe):
    import forcing_numpy as F
    import tracer_numpy as T
    v = T.noisy_vort(NX, NY, NOISE)
    m = F.recipe_model(_case(), v, None, None, **({probe: probe == "frozen_clock"} if probe else {}))
    t0 = time.time()
    for k in range(STEPS):
        m.step(1)
        print("%s: step %d  %.0f s" % (probe or "reference", k + 1, time.time() - t0), flush=True)
    return m.vort(), m.budget()


def make():
    import forcing_numpy as F
    import tangent_numpy as G
    import tracer_numpy as T
    from ref_numpy import rel_l2
    case = _case()
    with Pool(3) as pool:
        (vo, b), (vc, _), (vk, _) = pool.map(_run, (None, "conj_rule", "frozen_clock"))
    sx, sy = NX // 256, NY // 256
    kw = F.case_forcing(case)
    out = {"note": np.array("tests/forcing_numpy.py ForcedModel64 (float64, numpy rfft2/irfft2) on noisy_vort(%d, %d, %g), %d steps; "
                            "made by tests/golden/make_forcing_fixtures.py" % (NX, NY, NOISE, STEPS)),
           "vort_sub": vo[::sx, ::sy].astype(np.float32), "vort_l2": np.float64(np.sqrt((vo * vo).sum())),
           "seed": np.int64(T.RECIPE_SEED), "vort_noise": np.float64(NOISE), "steps": np.int64(STEPS),
           "dt": np.float64(T.recipe_dt(NX, NY)), "nu": np.float64(G.NU), "sub": np.array([sx, sy], dtype=np.int64),
           "rate": np.float64(case.rate), "k": np.float64(case.k), "width": np.float64(case.width), "forcing_seed": np.int64(F.SEED),
           "drag": np.float64(kw["drag"]), "hyper_nu": np.float64(kw["hyper_nu"]), "hyper_order": np.int64(kw["hyper_order"]),
           "n_ring": np.int64(b["n_ring"]),
           "shift_conj": np.float64(rel_l2(vc, vo)), "shift_clock": np.float64(rel_l2(vk, vo))}
    for k in ("dE_forc", "dE_diss", "dZ_forc", "dZ_diss"):
        out[k] = np.float64(b[k])
    np.savez_compressed(os.path.join(HERE, "forcing_%dx%d_step%d.npz" % (NX, NY, STEPS)), **out)
    print("%dx%d, %d steps: N_ring %d, probe shifts %.3g (no conjugate rule), %.3g (frozen clock); budget %s"
          % (NX, NY, STEPS, b["n_ring"], out["shift_conj"], out["shift_clock"], b))


if __name__ == "__main__":
    make()
