"""CPU checks of the tangent subspace (fb_model_set_tangents, tangent_qr; csrc/fb_tangent.h): the float64 reference and its
float32-storage restatement (tests/lyapunov_numpy.py), the inputs the GPU bars rest on, the analytic spectrum of a fluid at rest,
kaplan_yorke, and the argument refusals of the new entry points (refused before any HIP call: no GPU needed)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lyapunov_numpy as Y                                      # noqa: E402
import tracer_numpy as T                                        # noqa: E402

FB_EINVAL = 1


@functools.lru_cache(maxsize=None)
def _case(nx, ny):
    """(model, the spectra of subspace_inputs' three perturbations), computed once per grid"""
    m = Y.SubspaceModel64(nx, ny)
    return m, Y.spectra(Y.subspace_inputs(nx, ny)[1])


@pytest.mark.parametrize("kind", Y.KINDS)
def test_mgs_in_float64(kind):
    m, V = _case(64, 64)
    Q, R = Y.mgs(m, V, kind)
    d = Y.defect(m, Q, kind)
    scale = max(np.abs(v).max() for v in V)
    back = max(np.abs(sum(R[i, j] * Q[i] for i in range(j + 1)) - V[j]).max() for j in range(3)) / scale
    print("mgs, 64^2, %s: max |Q^T W Q - I| = %.3g, max |Q R - V| / max |V| = %.3g" % (kind, d, back))
    assert d <= 1e-12 and back <= 1e-12
    assert np.array_equal(R, np.triu(R)) and (np.diagonal(R) > 0).all()
    assert abs(R[0, 1]) > 0.1 * R[1, 1]                          # (the off-diagonal coefficients matter)


@pytest.mark.parametrize("nx,ny", Y.QR_GRIDS, ids=["%dx%d" % g for g in Y.QR_GRIDS])
def test_inputs_are_conditioned_for_the_gpu_bars_and_float32_storage_stays_clean(nx, ny):
    """10 <= cond <= 100: the coefficients r_ij matter and float32 storage does not lose the subspace.  mgs_f32's defect is the
    figure the GPU's orthonormality bar is four times of (lyapunov_numpy.MGS_F32_DEFECT holds the largest)."""
    m, V = _case(nx, ny)
    for kind in Y.KINDS:
        cond = Y.condition(m, V, kind)
        Q, R = Y.mgs_f32(m, V, kind)
        _, R64 = Y.mgs(m, V, kind)
        d, dr = Y.defect(m, Q, kind), float(np.abs(R - R64).max() / np.abs(R64).max())
        scale = max(np.abs(v).max() for v in V)
        back = max(np.abs(sum(R[i, j] * Q[i].astype(np.complex128) for i in range(j + 1)) - V[j]).max() for j in range(3)) / scale
        print("subspace_inputs %dx%d, %s: cond = %.4g; mgs_f32: max |Q^T W Q - I| = %.3g, max |R - R64| / max |R64| = %.3g, max |Q R - V| / max |V| = %.3g"
              % (nx, ny, kind, cond, d, dr, back))
        assert 10.0 <= cond <= 100.0
        assert d <= 1e-6
        assert d <= Y.MGS_F32_DEFECT
        assert dr <= 1e-6


def test_fluid_at_rest_has_the_analytic_spectrum():
    """zeta = 0: every mode decays by rk4_factor(nu lap dt) per step on its own.  A, A + B, A + B + C of three single modes are nested
    invariant subspaces, so r_ii of every interval is the i-th mode's factor to the power of the interval, from the first one on."""
    n, nu, dt, every, intervals = 64, 1.0e4, 3.0, 5, 3
    m = Y.SubspaceModel64(n, n, nu=nu, dt=dt)
    m.set_vort(np.zeros((n, n)))
    modes = ((3, 5), (7, 2), (10, 11))
    A, B, Cm = (T.cellular_flow(n, n, amp=1.0e-6, mx=mx, my=my)[0] for mx, my in modes)
    assert all(m.mask[mx, my] == 1.0 for mx, my in modes)
    m.set_tangents([A, A + B, A + B + Cm])
    want = np.array([T.rk4_factor(nu * m.lap[mx, my] * dt) ** every for mx, my in modes])
    assert np.ptp(want) > 1e-3
    for kind in Y.KINDS:
        m.dcs, _ = Y.mgs(m, m.dcs, kind)
        for k in range(intervals):
            m.step(every)
            m.dcs, R = Y.mgs(m, m.dcs, kind)
            err = np.abs(np.diagonal(R) / want - 1)
            print("fluid at rest, %s, interval %d: r_ii = %s, off by %s" % (kind, k, np.diagonal(R), err))
            assert (err <= 1e-12).all()


def test_kaplan_yorke():
    import xlab_fftbarotropic_amd as X
    assert X.kaplan_yorke([1.0, 0.0, -2.0]) == 2.5
    assert X.kaplan_yorke([-1.0, -2.0]) == 0.0
    assert X.kaplan_yorke([1.0, -0.5]) == 2.0
    assert X.kaplan_yorke([-2.0, 1.0, 0.0]) == X.kaplan_yorke([1.0, 0.0, -2.0])
    assert X.kaplan_yorke(np.array([0.5, -2.0, 0.25, -0.5])) == 3.0 + 0.25 / 2.0


def test_lyapunov_spectrum_checks_its_arguments_as_lyapunov_does():
    import xlab_fftbarotropic_amd as X
    for steps, every in ((0, 1), (1, 0)):
        with pytest.raises(ValueError):
            X.lyapunov_spectrum(None, steps, every)


def _both(stem):
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    return L, [(name, getattr(L, name)) for name in ("fb_model_" + stem, "fb_slab_" + stem)]


@pytest.mark.parametrize("count", [0, 33])
def test_set_tangents_names_the_count_before_the_null_handle(count):
    L, fns = _both("set_tangents")
    buf = (C.c_double * 64)()
    for name, fn in fns:
        assert fn(None, C.cast(buf, C.c_void_p), count) == FB_EINVAL, name
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and "count" in msg and "NULL" not in msg, (name, msg)


@pytest.mark.parametrize("stem", ["tangent_gram", "tangent_qr"])
def test_gram_and_qr_name_the_kind_before_the_null_handle(stem):
    L, fns = _both(stem)
    buf = (C.c_double * 64)()
    for name, fn in fns:
        assert fn(None, 2, C.cast(buf, C.c_void_p)) == FB_EINVAL, name
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and "kind" in msg and "NULL" not in msg, (name, msg)
