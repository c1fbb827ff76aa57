"""CPU checks of the tangent-linear model: the float64 reference of the coupled system (tests/tangent_numpy.py) shown to be the tangent
of the discrete step (Taylor test), linear, and right in two analytic cases; the condition on the inputs of the GPU path matrix
(tests/test_gpu_tangent.py); and the entry points declared, exported, bound, with the argument checks that run before any HIP call.
No GPU needed."""
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

from ref_numpy import Model64, rel_l2                           # noqa: E402
import tangent_numpy as G                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402

NAMES = ("fb_model_set_tangent", "fb_model_get_tangent", "fb_model_tangent_norm", "fb_model_tangent_scale",
         "fb_slab_set_tangent", "fb_slab_get_tangent", "fb_slab_tangent_norm", "fb_slab_tangent_scale")
FB_EINVAL = 1


def _small(n=64, noise=3e-2):
    v, d, _ = G.tangent_inputs(n, n, noise)
    return v.astype(np.float64), d.astype(np.float64)


def test_taylor_the_model_is_the_tangent_of_the_discrete_step():
    """64^2, 5 steps, float64: r(eps) = |[M(zeta + eps d) - M(zeta)] / eps - T(d)| / |T(d)| for eps = 1e-2, 1e-3, 1e-4 of |zeta| / |d|
    falls by a factor in [5, 20] per decade (first order: 10)"""
    n, steps = 64, 5
    v, d = _small(n)
    m = G.TangentModel64(n, n)
    m.set_vort(v)
    m.set_tangent(d)
    m.step(steps)
    base, td = m.vort(), m.tangent()
    scale = np.linalg.norm(v) / np.linalg.norm(d)
    r = []
    for rel in (1e-2, 1e-3, 1e-4):
        eps = rel * scale
        p = Model64(n, n)
        p.set_vort(v + eps * d)
        p.step(steps)
        r.append(rel_l2((p.vort() - base) / eps, td))
    print("Taylor test, 64^2, %d steps: r = %.3g, %.3g, %.3g; ratios %.3g, %.3g" % (steps, r[0], r[1], r[2], r[0] / r[1], r[1] / r[2]))
    assert 5 <= r[0] / r[1] <= 20 and 5 <= r[1] / r[2] <= 20
    assert r[2] < 1e-3


def test_linearity():
    """T(a d1 + b d2) = a T(d1) + b T(d2) to 1e-12 relative L2"""
    n, steps, a, b = 64, 5, 0.7, -2.3
    v, d1 = _small(n)
    d2 = np.roll(d1, 17, axis=0)[:, ::-1].copy()
    out = []
    for d in (d1, d2, a * d1 + b * d2):
        m = G.TangentModel64(n, n)
        m.set_vort(v)
        m.set_tangent(d)
        m.step(steps)
        out.append(m.tangent())
    err = rel_l2(out[2], a * out[0] + b * out[1])
    print("linearity, 64^2, %d steps: rel L2 = %.3g" % (steps, err))
    assert err <= 1e-12


def test_zero_flow_every_mode_decays_by_the_rk4_factor():
    """zeta = 0: the two advective terms vanish and a mode inside the dealiasing circle decays by rk4_factor(-nu k^2 dt)^n; a mode
    outside keeps its value"""
    n, steps, nu, dt = 64, 7, 6.5, 3.0
    _, d = _small(n)
    m = G.TangentModel64(n, n, nu=nu, dt=dt)
    m.set_vort(np.zeros((n, n)))
    m.set_tangent(d)
    d0 = m.dc.copy()
    m.step(steps)
    want = d0 * np.where(m.mask != 0, T.rk4_factor(m.nu * m.lap * m.dt) ** steps, 1.0)
    err = np.abs(m.dc - want).max() / np.abs(d0).max()
    print("zero flow, 64^2, %d steps: max mode error %.3g of the largest mode" % (steps, err))
    assert err <= 1e-13
    assert np.abs(m.vc).max() == 0.0


def test_translation_mode():
    """the noise-free elliptic vortex at 256^2, no source: dz_0 = gradx(zeta_0) stays gradx(zeta_n) up to the aliasing that the circular
    mask leaves; the residual measured here is tangent_numpy.TRANSLATION_RESIDUAL (the GPU test's bar is 10 times it)"""
    import oracle_py as O
    n = 256
    m = G.TangentModel64(n, n)
    m.set_vort(O.make_field("elliptic", n).astype(np.float64))
    m.dc = m.ikx * m.vc
    d0 = m.tangent()
    m.step(G.TRANSLATION_STEPS)
    want = m._c2r(m.ikx * m.vc)
    res = rel_l2(m.tangent(), want)
    print("translation mode, float64, 256^2, %d steps: residual %.4g (recorded %.4g); gradx(zeta) moved by %.3g" % (G.TRANSLATION_STEPS, res, G.TRANSLATION_RESIDUAL, rel_l2(want, d0)))
    assert abs(res / G.TRANSLATION_RESIDUAL - 1) <= 0.05
    assert rel_l2(want, d0) > 10 * res                          # the flow has moved: the identity is not that of two copies of the input


LIVE_CASES = [k for k in G.PATH_CASES if not k.fixture]


@pytest.mark.parametrize("case", LIVE_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in LIVE_CASES])
def test_path_matrix_inputs_make_the_parity_bar_decisive(case):
    """The condition on the inputs of the GPU path matrix, for every case whose float64 run takes under about 20 s (the others: the
    fixture stores both figures, tests/golden/make_tangent_fixtures.py): a reference whose tangent tendency at the stages 1 to 3 is
    blind to the masked modes of the vorticity's stage state, or of the perturbation's, shifts the float64 perturbation by >= 1e-4
    relative L2, ten times the parity bar of 1e-5, and the float32 restatement stays at or below 2.5e-6; the shifts are those recorded
    in the table to 10 %."""
    nx, ny = case.nx, case.ny
    v, d, s = G.tangent_inputs(nx, ny, case.vort_noise)
    ref = G.recipe_model(nx, ny, v, d, s)
    ref.step(case.steps)
    sv, st = G.probe_shifts(nx, ny, v, d, s, case.steps, ref)
    ft, fv = G.float32_errors(nx, ny, v, d, s, case.steps, ref)
    print("%dx%d, noise %g, %d steps: probe shifts %.3g (vorticity's stage state) / %.3g (perturbation's); float32 on the CPU: perturbation %.3g, vorticity %.3g"
          % (nx, ny, case.vort_noise, case.steps, sv, st, ft, fv))
    assert sv >= G.SHIFT_BAR and st >= G.SHIFT_BAR
    assert ft <= G.F32_BAR
    assert abs(sv / case.shift_vort - 1) <= 0.1 and abs(st / case.shift_tangent - 1) <= 0.1


def test_fixture_cases_meet_the_same_condition():
    """the stored figures of the cases that read a fixture, and the table's copy of them"""
    for case in G.PATH_CASES:
        if not case.fixture:
            continue
        with np.load(os.path.join(HERE, "golden", "tangent_%dx%d_step%d.npz" % (case.nx, case.ny, case.steps))) as z:
            sv, st, ft = float(z["shift_vort"]), float(z["shift_tangent"]), float(z["f32_tangent"])
            assert (int(z["seed"]), float(z["vort_noise"]), int(z["steps"])) == (G.SEED, case.vort_noise, case.steps)
        print("%dx%d, %d steps (fixture): probe shifts %.3g / %.3g, float32 on the CPU %.3g" % (case.nx, case.ny, case.steps, sv, st, ft))
        assert sv >= G.SHIFT_BAR and st >= G.SHIFT_BAR and ft <= G.F32_BAR
        assert abs(sv / case.shift_vort - 1) <= 0.1 and abs(st / case.shift_tangent - 1) <= 0.1


def test_norms_of_a_single_mode():
    """dz = A cos(kx x) cos(ky y): <dz^2> / 2 = A^2 / 8 and <|grad dpsi|^2> / 2 = A^2 / (8 k^2)"""
    n, amp = 64, 3.0e-6
    psi, _, k2 = T.cellular_flow(n, n, amp=amp)
    m = G.TangentModel64(n, n)
    m.set_tangent(psi)
    assert abs(m.tangent_norm("enstrophy") / (amp * amp / 8) - 1) <= 1e-12
    assert abs(m.tangent_norm("energy") / (amp * amp / 8 / k2) - 1) <= 1e-6     # (the float32 wavenumber tables)


def test_tangent_entry_points_declared_exported_and_bound():
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
    for cls in (X.Model, S.EngineSlab):
        for n in ("set_tangent", "tangent", "tangent_norm", "rescale_tangent", "lyapunov"):
            assert callable(getattr(cls, n, None)), (cls, n)


def test_tangent_argument_errors_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    w = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    out = ctypes.cast((ctypes.c_double * 1)(), ctypes.c_void_p)
    for fn in (L.fb_model_set_tangent, L.fb_model_get_tangent, L.fb_slab_set_tangent, L.fb_slab_get_tangent):
        assert fn(None, w) == FB_EINVAL
    assert b"fb_slab_get_tangent" in L.fb_last_error()
    for fn, name in ((L.fb_model_tangent_norm, b"fb_model_tangent_norm"), (L.fb_slab_tangent_norm, b"fb_slab_tangent_norm")):
        assert fn(None, 0, out) == FB_EINVAL
        assert name in L.fb_last_error()
    assert L.fb_model_tangent_norm(None, 2, out) == FB_EINVAL
    assert b"kind" in L.fb_last_error()
    assert L.fb_model_tangent_norm(None, -1, out) == FB_EINVAL
    assert L.fb_model_tangent_norm(None, 1, None) == FB_EINVAL
    for a in (0.0, float("nan"), float("inf")):
        assert L.fb_model_tangent_scale(None, a) == FB_EINVAL
        assert b"finite" in L.fb_last_error()
    assert L.fb_model_tangent_scale(None, 2.0) == FB_EINVAL
    assert b"NULL model" in L.fb_last_error()
    with pytest.raises(ValueError):
        X.tangent_kind("vorticity")
