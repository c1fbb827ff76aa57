"""CPU checks of the passive tracer: the float64 reference of the coupled system (tests/tracer_numpy.py) pinned by a twin run and an
analytic decay, the condition on the inputs of the GPU path matrix (tests/test_gpu_tracer_paths.py), and the entry points declared, exported, bound, with the argument checks that run before any HIP call.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ref_numpy import rel_l2                                   # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from tracer_numpy import TracerModel64, cellular_flow, rk4_factor   # noqa: E402

NAMES = ("fb_model_set_tracer", "fb_model_get_tracer", "fb_model_get_tracer_eddy_diffusivity",
         "fb_slab_set_tracer_local", "fb_slab_get_tracer_local", "fb_slab_get_tracer_eddy_diffusivity")
FB_EINVAL = 1


def test_twin_tracer_follows_the_vorticity_in_float64():
    """c = zeta and kappa = nu: the float64 tracer equals the float64 vorticity after 100 steps at 128^2, to 1e-12 relative"""
    import oracle_py as O
    n = 128
    v0 = O.make_field("kuo2004", n)
    m = TracerModel64(n, n, kappa=6.5)
    m.set_vort(v0)
    m.set_tracer(v0)
    m.step(100)
    err = rel_l2(m.tracer(), m.vort())
    print("twin, float64, 128^2, 100 steps: rel L2 = %.3g" % err)
    assert err <= 1e-12
    assert rel_l2(m.vort(), v0) > 1e-3                         # (the state has moved: the comparison is not of two copies of the input)


def test_analytic_decay_in_a_steady_cellular_flow():
    """psi = A cos cos, zeta = laplacian(psi), c = psi, nu = 0: J(psi, c) = 0, the flow is steady and c = c0 R(-kappa k^2 dt)^n"""
    for nx, ny in ((128, 128), (256, 128), (128, 256)):
        psi, zeta, k2 = cellular_flow(nx, ny, amp=1.0e6)
        kappa, dt, steps = 50.0, 3.0, 200
        m = TracerModel64(nx, ny, nu=0.0, dt=dt, kappa=kappa)
        m.set_vort(zeta)
        m.set_tracer(psi)
        m.step(steps)
        want = psi * rk4_factor(-kappa * k2 * dt) ** steps
        err = rel_l2(m.tracer(), want)
        print("decay, float64, %dx%d, %d steps: rel L2 = %.3g, factor %.6f" % (nx, ny, steps, err, rk4_factor(-kappa * k2 * dt) ** steps))
        assert err <= 1e-10
        assert rel_l2(m.vort(), zeta) <= 1e-10                 # the flow is steady


LIVE_CASES = [k for k in T.PATH_CASES if not k.fixture]


@pytest.mark.parametrize("case", LIVE_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in LIVE_CASES])
def test_path_matrix_inputs_make_the_parity_bar_decisive(case):
    """The condition on the inputs of the GPU path matrix, for every case whose float64 run takes under about 20 s (the others: the
    fixture stores the shifts, tests/golden/make_tracer_fixtures.py): a reference whose tracer tendency at the stages 1 to 3 is blind
    to the masked modes of the vorticity's stage state, or of the tracer's, shifts the float64 tracer by >= 1e-4 relative L2, ten
    times the parity bar of 1e-5; the vorticity is untouched by the probe; the shifts are those recorded in the table to 10 %; the
    source changes the tracer, through the velocity only."""
    nx, ny = case.nx, case.ny
    v, c, s = T.noisy_inputs(nx, ny, case.vort_noise)
    ref = T.recipe_model(nx, ny, v, c, s)
    share = T.masked_share(ref)
    ref.step(case.steps)
    shifts = {}
    for which in ("blind_vort", "blind_tracer"):
        p = T.recipe_model(nx, ny, v, c, s, cls=T.ProbeModel64, **{which: True})
        p.step(case.steps)
        assert rel_l2(p.vort(), ref.vort()) == 0.0
        shifts[which] = rel_l2(p.tracer(), ref.tracer())
    print("%dx%d, noise %g, %d steps: probe shifts %.3g (vorticity's stage state) / %.3g (tracer's); %.0f %% of the tracer's norm in masked modes"
          % (nx, ny, case.vort_noise, case.steps, shifts["blind_vort"], shifts["blind_tracer"], 100 * share))
    assert shifts["blind_vort"] >= T.SHIFT_BAR and shifts["blind_tracer"] >= T.SHIFT_BAR
    assert abs(shifts["blind_vort"] / case.shift_vort - 1) <= 0.1 and abs(shifts["blind_tracer"] / case.shift_tracer - 1) <= 0.1
    assert share >= 0.15


@pytest.mark.parametrize("nx,ny", [(256, 256), (192, 192), (1024, 64), (64, 4096)])
def test_float32_stays_well_inside_the_bar(nx, ny):
    """the ordinary float32 evaluation of the recipe (torch FFTs on the CPU) is within 1e-6 of the float64 run, a tenth of the parity
    bar, so the bar of 1e-5 has room for a correct float32 engine and none for the probes' 1e-4; and the vorticity source (white noise
    of 1e-9 s^-2) is not lost in rounding: without it the float64 vorticity differs by more than the float32 error"""
    case = [k for k in T.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]
    v, c, s = T.noisy_inputs(nx, ny, case.vort_noise)
    ref = T.recipe_model(nx, ny, v, c, s)
    ref.step(case.steps)
    et, ev = T.float32_errors(nx, ny, v, c, s, case.steps, ref)
    bare = T.recipe_model(nx, ny, v, c, None)
    bare.step(case.steps)
    ds = rel_l2(bare.vort(), ref.vort())
    print("%dx%d float32 on the CPU: tracer %.3g, vorticity %.3g; the source moves the vorticity by %.3g" % (nx, ny, et, ev, ds))
    assert et <= 1e-6 and ev <= 1e-6
    assert ds > 0


def test_tracer_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None, n
    from importlib import import_module
    S = import_module("xlab-fftbarotropic_amd.slab")
    for cls, names in ((X.Model, ("set_tracer", "tracer", "tracer_eddy_diffusivity")),
                       (S.EngineSlab, ("set_tracer_local", "tracer_local", "tracer_eddy_diffusivity"))):
        for n in names:
            assert callable(getattr(cls, n, None)), (cls, n)


def test_tracer_argument_errors_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    buf = (ctypes.c_float * 4)()
    w = ctypes.cast(buf, ctypes.c_void_p)
    tab = ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p)
    assert L.fb_model_set_tracer(None, w, 1.0) == FB_EINVAL
    assert b"fb_model_set_tracer" in L.fb_last_error()
    assert L.fb_model_set_tracer(None, None, 0.0) == FB_EINVAL
    assert L.fb_model_get_tracer(None, w) == FB_EINVAL
    assert b"fb_model_get_tracer" in L.fb_last_error()
    assert L.fb_model_get_tracer_eddy_diffusivity(None, 16, tab, None, None) == FB_EINVAL
    assert b"fb_model_get_tracer_eddy_diffusivity" in L.fb_last_error()
    assert L.fb_slab_set_tracer_local(None, w, 1.0) == FB_EINVAL
    assert L.fb_slab_get_tracer_local(None, w) == FB_EINVAL
    assert L.fb_slab_get_tracer_eddy_diffusivity(None, 16, tab, None, None) == FB_EINVAL
