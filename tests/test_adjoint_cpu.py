"""CPU checks of the adjoint model: the float64 reference (tests/adjoint_numpy.py) shown to be the transpose of the tangent-linear
reference (the dot-product identity), linear, and right in the analytic case of a fluid at rest; the conditions on the inputs of the
GPU path matrix (tests/test_gpu_adjoint.py): the probe shift, the float32 restatement's error and its dot-product residual, from which
the GPU's dot-product bar is taken; the float32 restatement of the power iteration; and the entry points declared, exported, bound,
with the argument checks that run before any HIP call.  No GPU needed."""
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

from ref_numpy import rel_l2                                    # noqa: E402
import adjoint_numpy as A                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402

NAMES = tuple("fb_%s_%s" % (k, n) for k in ("model", "slab") for n in ("adjoint_record", "adjoint_recorded", "set_adjoint", "get_adjoint", "adjoint_back"))
METHODS = ("record_adjoint", "adjoint_recorded", "set_adjoint", "adjoint", "adjoint_back", "singular_values")
FB_EINVAL = 1


@pytest.mark.parametrize("n,steps", [(64, 5), (192, 2)])
def test_dot_product_identity_of_the_float64_reference(n, steps):
    """|<T d, lam> - <d, T^T lam>| / (|T d| |lam|) <= 1e-12 on tangent_inputs (never-dealiased noise on zeta and dz, a source) and lam as
    white noise, never dealiased"""
    v, d, s, lam = A.adjoint_inputs(n, n, 3e-2)
    m = A.run_case(n, n, v, d, s, lam, steps)
    res = A.dot_residual(m.tangent(), lam, d, m.adjoint())
    print("dot-product identity, float64, %d^2, %d steps: %.3g" % (n, steps, res))
    assert res <= 1e-12
    assert m.adjoint_recorded() == 0
    assert rel_l2(m.adjoint(), lam) > 1e-3 and rel_l2(m.tangent(), d) > 1e-3      # neither operator is the identity


def test_linearity_of_the_transpose():
    """T^T(a l1 + b l2) = a T^T(l1) + b T^T(l2) to 1e-12 relative L2"""
    n, steps, a, b = 64, 5, 0.7, -2.3
    v, d, s, l1 = A.adjoint_inputs(n, n, 3e-2)
    l1 = l1.astype(np.float64)
    l2 = np.roll(l1, 17, axis=0)[:, ::-1].copy()
    out = [A.run_case(n, n, v, d, s, lam, steps).adjoint() for lam in (l1, l2, a * l1 + b * l2)]
    err = rel_l2(out[2], a * out[0] + b * out[1])
    print("linearity of T^T, 64^2, %d steps: rel L2 = %.3g" % (steps, err))
    assert err <= 1e-12


def test_zero_flow_every_mode_is_scaled_by_the_rk4_factor():
    """zeta = 0: the advective terms vanish; a mode of lam inside the dealiasing circle is scaled by rk4_factor(-nu k^2 dt)^n, a mode
    outside keeps its value"""
    n, steps, nu, dt = 64, 7, 6.5, 3.0
    lam = A.adjoint_inputs(n, n, 3e-2)[3]
    m = A.AdjointModel64(n, n, nu=nu, dt=dt)
    m.set_vort(np.zeros((n, n)))
    m.record_adjoint(steps)
    m.step(steps)
    m.set_adjoint(lam)
    l0 = m.lc.copy()
    m.adjoint_back(steps)
    want = l0 * np.where(m.mask != 0, T.rk4_factor(m.nu * m.lap * m.dt) ** steps, 1.0)
    err = np.abs(m.lc - want).max() / np.abs(l0).max()
    print("zero flow, 64^2, %d steps: max mode error %.3g of the largest mode" % (steps, err))
    assert err <= 1e-13


def test_tape_discipline_of_the_reference():
    n = 64
    v, d, s, lam = A.adjoint_inputs(n, n, 3e-2)
    m = A.recipe_model(n, n, v, d, s)
    m.record_adjoint(3)
    m.step(2)
    with pytest.raises(ValueError):
        m.step(2)
    assert m.adjoint_recorded() == 2
    m.set_adjoint(lam)
    with pytest.raises(ValueError):
        m.adjoint_back(3)
    m.set_vort(v)
    assert m.adjoint_recorded() == 0


@pytest.mark.parametrize("case", A.PATH_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in A.PATH_CASES])
def test_path_matrix_inputs_make_the_parity_bar_decisive(case):
    """For every case of the GPU path matrix: a reference that linearises all four stages of a step about the step's base state shifts
    the float64 lam_0 by >= 1e-4 relative L2 (SHIFT_BAR, ten times the parity bar), as recorded in the table to 10 %; the float32
    restatement stays at or below 2.5e-6 (F32_BAR) of float64; its dot-product residual is at most the table's figure, from which
    the GPU test's bar is taken (allowing 1.5 for another FFT library's summation order on the CPU)."""
    nx, ny = case.nx, case.ny
    v, d, s, lam = A.adjoint_inputs(nx, ny, case.vort_noise)
    ref = A.run_case(nx, ny, v, d, s, lam, case.steps)
    probe = A.run_case(nx, ny, v, d, s, lam, case.steps, cls=A.ProbeAdjoint64)
    assert rel_l2(probe.vort(), ref.vort()) == 0.0
    shift = rel_l2(probe.adjoint(), ref.adjoint())
    f32, fdot = A.float32_figures(nx, ny, v, d, s, lam, case.steps, ref)
    print("%dx%d, noise %g, %d steps: probe shift %.3g; float32 on the CPU: lam_0 %.3g, dot-product residual %.3g (float64: %.3g)"
          % (nx, ny, case.vort_noise, case.steps, shift, f32, fdot, A.dot_residual(ref.tangent(), lam, d, ref.adjoint())))
    assert shift >= A.SHIFT_BAR
    assert abs(shift / case.shift - 1) <= 0.1
    assert f32 <= A.F32_BAR
    assert fdot <= 1.5 * case.f32_dot
    assert A.DOT_BAR == 4 * max(k.f32_dot for k in A.PATH_CASES)


def test_float32_restatement_of_the_power_iteration():
    """singular_values at 256^2, 3 steps, 4 iterations from the tangent inputs' dz: the float32 restatement's singular values agree with
    float64 to SV_F32 (recorded, an upper bound to 1.5), far below the GPU test's 1e-4"""
    n = A.SV_N
    v, d, s, _ = A.adjoint_inputs(n, n, 3e-2)
    ref = A.recipe_model(n, n, v, d, s)
    s64, v64 = A.singular_values(ref, ref.spectrum(), A.SV_STEPS, A.SV_ITERS, d)
    f = A.Float32Model(ref, s)
    f.set_vort(v)
    s32, v32 = A.singular_values(f, f.spectrum(), A.SV_STEPS, A.SV_ITERS, d)
    err = max(abs(a / b - 1) for a, b in zip(s32, s64))
    print("power iteration, 256^2, %d steps: sigma (float64) = %s; float32 off by %.3g, the vector by %.3g" % (A.SV_STEPS, s64, err, rel_l2(v32, v64)))
    assert err <= 1.5 * A.SV_F32 and A.SV_F32 <= A.SV_BAR / 4
    assert s64[-1] > s64[0]                                     # the iteration moves towards the leading vector


def test_adjoint_entry_points_declared_exported_and_bound():
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
        for n in METHODS:
            assert callable(getattr(cls, n, None)), (cls, n)
    assert callable(X.singular_values)


def test_adjoint_argument_errors_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    w = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    cnt = ctypes.c_int(7)
    for kind in ("model", "slab"):
        f = {n: getattr(L, "fb_%s_%s" % (kind, n)) for n in ("adjoint_record", "adjoint_recorded", "set_adjoint", "get_adjoint", "adjoint_back")}
        for n, args in (("adjoint_record", (None, 2)), ("adjoint_recorded", (None, ctypes.byref(cnt))), ("set_adjoint", (None, w)), ("get_adjoint", (None, w)),
                        ("adjoint_back", (None, 1))):
            assert f[n](*args) == FB_EINVAL, (kind, n)
            assert ("fb_%s_%s" % (kind, n)).encode() in L.fb_last_error(), (kind, n)
    assert L.fb_model_adjoint_record(None, -1) == FB_EINVAL
    assert b"depth" in L.fb_last_error()
    assert L.fb_model_adjoint_back(None, -1) == FB_EINVAL
    assert b"nsteps" in L.fb_last_error()
    assert L.fb_model_get_adjoint(None, None) == FB_EINVAL

