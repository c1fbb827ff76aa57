"""CPU checks of the Lagrangian (drifter) observations: the float64 reference (tests/lagrangian_numpy.py) shown to give the gradient of
J = 1/2 sum |X(T) - y|^2 / sigma^2 with respect to the initial vorticity and to the drifters' initial positions (central differences),
the identity Xb_0 = F^T Xb(T) against the deformation gradient, a mixed window, the tape handling and checkpointing; the figures of the
float32 restatement from which the bars of tests/test_gpu_lagrangian.py are taken; the twin experiment on the reference; and the entry
points declared, exported, bound, with the argument checks that run before any HIP call.  No GPU needed."""
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
import deformation_numpy as D                                   # noqa: E402
import lagrangian_numpy as L                                    # noqa: E402
import obs_numpy as O                                           # noqa: E402
import particles_numpy as P                                     # noqa: E402

STEMS = ("particle_tape", "particle_tape_count", "set_particle_adjoint", "get_particle_adjoint")
NAMES = tuple("fb_%s_%s" % (k, n) for k in ("model", "slab") for n in STEMS)
METHODS = ("record_particles", "particles_recorded", "set_particle_adjoint", "particle_adjoint", "fourdvar", "fit_initial")
FB_EINVAL = 1
EPS = (1e-3, 1e-4, 1e-5, 1e-6)
FD_BAR = 1e-7


def _inputs(nx, ny):
    v, _, src, lam = A.adjoint_inputs(nx, ny, 3e-2)
    m = L.ref_model(nx, ny)
    m.src = src.astype(np.float64)
    return m, v.astype(np.float64), lam


def _final_position_sets(m, z0, xy0, steps, seed):
    """one "position" set at the last step: the model's own final positions plus noise of 0.3 of a cell, sigma a tenth of a cell"""
    cell = P.widen(L.LX) / m.nx
    m.set_vort(z0)
    m.set_particles(xy0)
    m.step(steps)
    y = m.particles() + 0.3 * cell * np.random.default_rng(seed).standard_normal(xy0.shape)
    return [L.Obs(steps, L.POSITION, None, y, 0.1 * cell)]


def _central(J, eps):
    return (J(+eps) - J(-eps)) / (2 * eps)


# ---- the gradient against central differences ----
@pytest.mark.parametrize("nx,ny,steps", [(64, 64, 6), (192, 64, 5)])
def test_gradient_against_central_finite_differences(nx, ny, steps):
    """J = 1/2 sum |X(T) - y|^2 / sigma^2 of 300 drifters.  <dJ/dzeta_0, d> with the drifters at obs_numpy.positions (grid points,
    wrapping stencils, far and negative positions, one position twice), and <dJ/dX_0, dx> with the drifters strictly inside cells
    (the interpolant's derivative jumps at cell faces: on a face a central difference is the mean of two one-sided slopes), each
    against (J(+eps) - J(-eps)) / (2 eps) over a sweep of eps: the best eps agrees to 1e-7 relative."""
    m, z0, _ = _inputs(nx, ny)
    rng = np.random.default_rng(5)
    d = rng.standard_normal((nx, ny))
    d *= np.abs(z0).max() / np.abs(d).max()
    for what, xy0 in (("zeta_0", O.positions(nx, ny)), ("X_0", L.interior_positions(nx, ny))):
        sets = _final_position_sets(m, z0, xy0, steps, 7)
        J, g, xb0 = L.fourdvar(m, z0, sets, None, xy0)
        assert xb0.shape == xy0.shape and g.shape == (nx, ny)
        if what == "zeta_0":
            want = float(np.vdot(g, d))
            errs = {e: abs(_central(lambda s: L.fourdvar(m, z0 + s * d, sets, None, xy0)[0], e) / want - 1) for e in EPS}
            assert abs(want) > 1e-3 * np.linalg.norm(g) * np.linalg.norm(d)
        else:
            dx = rng.standard_normal(xy0.shape) * P.widen(L.LX) / nx
            want = float(np.vdot(xb0, dx))
            errs = {e: abs(_central(lambda s: L.fourdvar(m, z0, sets, None, xy0 + s * dx)[0], e) / want - 1) for e in EPS}
            assert abs(want) > 1e-3 * np.linalg.norm(xb0) * np.linalg.norm(dx)
        print("gradient with respect to %s against central differences, %dx%d, %d steps: J = %.6g, relative error per eps: %s"
              % (what, nx, ny, steps, J, ", ".join("%g: %.2g" % kv for kv in errs.items())))
        assert min(errs.values()) <= FD_BAR


def test_mixed_window_against_central_finite_differences():
    """u and v sets at the steps 2, 4, 6 and position sets at 3 and 6, with a background term, at 64^2: <grad, d> against central
    differences to the same bar"""
    n = 64
    m = L.ref_model(n, n)
    v, src, xy0, sets = L.position_case(n, n, m, mixed=True)
    assert sorted(set((s.step, s.kind) for s in sets)) == [(2, "u"), (2, "v"), (3, "position"), (4, "u"), (4, "v"), (6, "position"), (6, "u"), (6, "v")]
    m.src = src.astype(np.float64)
    z0 = v.astype(np.float64)
    bg = (0.9 * z0, 1e-3)
    d = np.random.default_rng(6).standard_normal((n, n))
    d *= np.abs(z0).max() / np.abs(d).max()
    J, g, xb0 = L.fourdvar(m, z0, sets, bg, xy0)
    Jp = L.fourdvar(m, z0, [s for s in sets if s.kind == L.POSITION], None, xy0)[0]
    Jf = L.fourdvar(m, z0, [s for s in sets if s.kind != L.POSITION], None, xy0)[0]
    assert min(Jp, Jf) > 1e-2 * J                               # neither part is negligible
    want = float(np.vdot(g, d))
    errs = {e: abs(_central(lambda s: L.fourdvar(m, z0 + s * d, sets, bg, xy0)[0], e) / want - 1) for e in EPS}
    print("mixed window against central differences, 64^2: J = %.6g (positions %.4g, u and v %.4g), relative error per eps: %s"
          % (J, Jp, Jf, ", ".join("%g: %.2g" % kv for kv in errs.items())))
    assert min(errs.values()) <= FD_BAR


# ---- the identity against the deformation gradient ----
@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64)])
def test_initial_particle_adjoint_is_the_deformation_gradient_transposed(nx, ny):
    """Xb_0 = F^T Xb(T) for lam(T) = 0, F the deformation gradient of deformation_numpy.DeformationModel64 over the same steps: both are
    the exact Jacobian of the discrete map; 1e-12 of max |F^T Xb(T)|.  lam_0 is not zero: the positions depend on the vorticity."""
    ref = L.sweep_case(nx, ny)
    xy = O.positions(nx, ny)
    dm = D.DeformationModel64(nx, ny, nu=ref.nu, dt=ref.dt)
    dm.src = ref.src
    dm.set_vort(A.adjoint_inputs(nx, ny, 3e-2)[0])
    dm.set_particles(xy)
    dm.step(L.STEPS)
    assert np.array_equal(dm.particles(), ref.particles()) and np.array_equal(dm.F, ref.particle_deformation())
    want = np.einsum("nij,ni->nj", dm.F, L.xbar_T(L.NPTS))
    err = L.xbar_error(ref.particle_adjoint(), want)
    print("Xb_0 against F^T Xb(T), %dx%d, float64: %.3g" % (nx, ny, err))
    assert err <= 1e-12
    assert np.linalg.norm(ref.adjoint()) > 0


# ---- the tapes ----
def test_three_then_two_steps_equal_five_and_checkpointing_changes_nothing():
    nx, ny = 192, 64
    one = L.sweep_case(nx, ny, lam_T=A.adjoint_inputs(nx, ny, 3e-2)[3])
    v, _, src, lam = A.adjoint_inputs(nx, ny, 3e-2)
    xy = O.positions(nx, ny)

    def run(cls, on, parts):
        m = L.ref_model(nx, ny, cls)
        m.src = src.astype(np.float64)
        m.set_vort(v)
        m.set_particles(xy)
        on(m)
        m.record_particles(L.STEPS)
        m.step(2)
        m.step(3)
        assert m.particles_recorded() == (5, 5)
        m.set_adjoint(lam)
        m.set_particle_adjoint(L.xbar_T(L.NPTS))
        for k in parts:
            m.adjoint_back(k)
        assert m.particles_recorded() == (0, 5) and m.adjoint_recorded() == 0
        return m
    for cls, on, parts in ((L.LagrangianModel64, lambda m: m.record_adjoint(5), (3, 2)),
                           (L.CheckpointLagrangian64, lambda m: m.checkpoint_adjoint(2, 5), (5,)),
                           (L.CheckpointLagrangian64, lambda m: m.checkpoint_adjoint(2, 5), (1, 3, 1))):
        m = run(cls, on, parts)
        assert np.array_equal(m.adjoint(), one.adjoint()) and np.array_equal(m.particle_adjoint(), one.particle_adjoint()), (cls, parts)
        assert np.array_equal(m.particles(), one.particles()) and np.array_equal(m.vort(), one.vort())
    with pytest.raises(ValueError, match="overrun the particle tape"):
        m = L.ref_model(nx, ny)
        m.set_vort(v)
        m.set_particles(xy)
        m.record_particles(2)
        m.step(3)


def test_a_nan_position_poisons_that_drifter_alone():
    nx, ny = 64, 64
    xy = O.positions(nx, ny)
    bad = xy.copy()
    bad[11, 0] = np.nan
    a, b = L.sweep_case(nx, ny, xy=xy), L.sweep_case(nx, ny, xy=bad)
    keep = np.arange(L.NPTS) != 11
    assert np.isnan(b.particle_adjoint()[11]).all() and np.array_equal(b.particle_adjoint()[keep], a.particle_adjoint()[keep])
    # lam_0 lacks that drifter's deposit alone
    c = L.sweep_case(nx, ny, xy=xy[keep])                       # (another Xb(T) for the drifters behind it: only finiteness is compared)
    assert np.isfinite(b.adjoint()).all() and np.isfinite(c.adjoint()).all()
    assert rel_l2(b.adjoint(), a.adjoint()) > 0


# ---- the float32 restatement ----
@pytest.mark.parametrize("case", L.L_CASES, ids=lambda k: "%dx%d" % (k.nx, k.ny))
def test_float32_figures(case):
    """the float32 restatement's errors of lam_0 and Xb_0 against float64 on the path cases (lam(T) = 0: all of lam_0 comes from the
    drifters): at most the table's figures, which are held to the GPU's bars in turn (they vary a little between CPUs)"""
    nx, ny = case.nx, case.ny
    ref, f = L.sweep_case(nx, ny), L.sweep_case(nx, ny, L.Float32Lagrangian)
    xy = O.positions(nx, ny)
    moved = float(np.abs((ref.particles() - xy) / np.array([P.widen(L.LX) / nx, P.widen(L.LY) / ny])).max())
    lam, xbar = rel_l2(f.adjoint(), ref.adjoint()), L.xbar_error(f.particle_adjoint(), ref.particle_adjoint())
    print("float32 restatement %dx%d: lam_0 %.3g (table %.3g), Xb_0 %.3g (table %.3g); the drifters moved up to %.3g cells (table %.3g)"
          % (nx, ny, lam, case.lam, xbar, case.xbar, moved, case.moved))
    assert lam <= L.LAM_BAR and xbar <= L.XBAR_BAR
    assert lam <= 1.5 * case.lam and xbar <= 1.5 * case.xbar
    assert abs(moved / case.moved - 1) <= 0.01


@pytest.mark.parametrize("case", L.F_CASES, ids=lambda k: "%dx%d-%s" % (k.nx, k.ny, "mixed" if k.mixed else "positions"))
def test_float32_figures_of_fourdvar(case):
    """the float32 restatement's errors of J, grad and dJ/dX_0 on the fourdvar cases of tests/test_gpu_lagrangian.py: at most the
    table's figures, J and grad within the GPU's 1e-5, dJ/dX_0 within FOURDVAR_XBAR_BAR"""
    ref = L.ref_model(case.nx, case.ny)
    v, src, xy0, sets = L.position_case(case.nx, case.ny, ref, case.mixed)
    ref.src = src.astype(np.float64)
    J, g, xb = L.fourdvar(ref, v, sets, None, xy0)
    Jf, gf, xbf = L.fourdvar(L.Float32Lagrangian(ref, src), v, sets, None, xy0)
    eJ, eg, ex = abs(Jf / J - 1), rel_l2(gf, g), L.xbar_error(xbf, xb)
    print("float32 restatement, fourdvar %dx%d %s: J %.3g (table %.3g), grad %.3g (%.3g), dJ/dX_0 %.3g (%.3g)"
          % (case.nx, case.ny, "mixed" if case.mixed else "positions", eJ, case.J, eg, case.grad, ex, case.xbar))
    assert eJ <= 1e-5 and eg <= 1e-5 and ex <= L.FOURDVAR_XBAR_BAR
    assert eJ <= 1.5 * case.J and eg <= 1.5 * case.grad and ex <= 1.5 * case.xbar


def test_the_drifters_cross_cell_faces_and_the_bars_are_set():
    assert max(k.moved for k in L.L_CASES) > 1.0
    assert [(k.nx, k.ny) for k in L.L_CASES] == [(k.nx, k.ny) for k in A.PATH_CASES]
    assert L.XBAR_BAR == 4 * max(k.xbar for k in L.L_CASES) and 0 < L.XBAR_BAR < 1e-5
    assert L.FOURDVAR_XBAR_BAR == 4 * max(k.xbar for k in L.F_CASES) and L.XBAR_BAR < L.FOURDVAR_XBAR_BAR < 1e-5


# ---- the twin experiment ----
def test_twin_experiment_on_the_float64_reference():
    """fit_initial on the float64 reference with drifter positions as the only data (64^2, dt = 30 s, 256 drifters at the steps 2, 4,
    6, 8, sigma a tenth of their largest displacement; obs_numpy.twin_case's truth and first guess): J falls at every accepted
    iteration, J_K / J_0 after K = 10 is the recorded figure to 10 % and at most 0.1, and z0 ends closer to the truth"""
    import torch
    import xlab_fftbarotropic_amd as X
    truth, guess, xy0, sets, sigma = L.twin_case(X.make_field)
    model = L.Fourdvar64(L.LagrangianModel64(O.TWIN_N, O.TWIN_N, nu=O.TWIN_NU, dt=O.TWIN_DT))
    z, hist, evals = X.fit_initial(model, torch.from_numpy(guess.astype(np.float64)), sets, L.TWIN_ITERS, particles=xy0)
    e0, e1 = rel_l2(guess, truth), rel_l2(z.numpy(), truth)
    print("twin experiment with drifters, float64: sigma = %.4g m; J = %s; J_K / J_0 = %.4g (recorded %.4g); %d evaluations; z0 off by %.3g "
          "at the start, %.3g at the end" % (sigma, ["%.4g" % j for j in hist], hist[-1] / hist[0], L.TWIN_RATIO, evals, e0, e1))
    assert len(hist) == L.TWIN_ITERS + 1 and evals == model.calls
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] / hist[0] / L.TWIN_RATIO - 1) <= 0.1
    assert L.TWIN_RATIO <= 0.1                                  # else the case shows nothing
    assert e1 < e0


# ---- the entry points ----
def test_lagrangian_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    lib = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in X.EXPORTS and n in B.SIGNATURES, n
    assert set(B._LAGRANGIAN_PAIRS) == set(STEMS) and not set(B._LAGRANGIAN_PAIRS) & set(B._PAIRS)
    for stem in STEMS:
        assert len(B.SIGNATURES["fb_model_" + stem][0]) == 1 + len(B._LAGRANGIAN_PAIRS[stem])
    from importlib import import_module
    S = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (X.Model, S.EngineSlab):
        for n in METHODS:
            assert callable(getattr(cls, n, None)), (cls, n)
    assert X.POSITION == "position" and X.POSITION not in X.OBS_KINDS


def test_argument_errors_are_rejected_without_a_device():
    """every refusal that needs no handle comes before the NULL handle's, under the function's own name"""
    import xlab_fftbarotropic_amd as X
    lib = X.lib()
    p = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    i = ctypes.byref(ctypes.c_int())
    for k in ("model", "slab"):
        cases = [("particle_tape", (-1,), "depth outside"), ("particle_tape", ((1 << 20) + 1,), "depth outside"), ("particle_tape", (3,), "NULL " + k),
                 ("particle_tape", (0,), "NULL " + k), ("particle_tape_count", (None, i), "NULL output"), ("particle_tape_count", (i, None), "NULL output"),
                 ("particle_tape_count", (i, i), "NULL " + k), ("set_particle_adjoint", (p,), "NULL " + k), ("set_particle_adjoint", (None,), "NULL " + k),
                 ("get_particle_adjoint", (None,), "NULL output"), ("get_particle_adjoint", (p,), "NULL " + k)]
        for stem, args, phrase in cases:
            name = "fb_%s_%s" % (k, stem)
            assert getattr(lib, name)(None, *args) == FB_EINVAL, (name, args)
            msg = lib.fb_last_error().decode()
            assert msg.startswith(name + ": " + phrase), (name, args, msg)


def test_position_sets_refuse_bad_input_without_a_device():
    """what binding.fourdvar refuses before it touches the model: a "position" set without particles"""
    import xlab_fftbarotropic_amd as X

    class Set:
        step, kind = 2, X.POSITION

        def __len__(self):
            return 4
    class Nothing:                                              # (no method: fourdvar must refuse before it calls one)
        import torch
        device = "cpu"
    with pytest.raises(ValueError, match="needs particles"):
        X.fourdvar(Nothing(), np.zeros((8, 8)), [Set()])
    with pytest.raises(ValueError, match="4 drifters, 5 particles"):
        X.fourdvar(Nothing(), np.zeros((8, 8)), [Set()], particles=np.zeros((5, 2)))
    with pytest.raises(ValueError, match="no observations"):
        X.fourdvar(Nothing(), np.zeros((8, 8)), [], particles=np.zeros((4, 2)))
