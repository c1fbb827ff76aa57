"""CPU checks of the passive tracer: the float64 reference of the coupled system (tests/tracer_numpy.py) pinned by a twin run and an
analytic decay, and the entry points declared, exported, bound, with the argument checks that run before any HIP call.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ref_numpy import rel_l2                                   # noqa: E402
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
