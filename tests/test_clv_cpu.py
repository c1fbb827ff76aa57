"""CPU checks of the covariant Lyapunov vectors (clv_coefficients, clv; csrc/fb_clv.h): the backward recursion against a second
implementation, its refusals, the covariance identity T V_n = V_(n+1) D in float64 (it holds to rounding for ANY C_end: nothing here
depends on the convergence of a chaotic run), the conditioning and the probes that give the GPU's covariance bar its teeth, the figures
the GPU's comparison with the float64 run is held to, a fluid at rest, and the argument refusals of the new entry points (refused before
any HIP call: no GPU needed).  One line of figures per check (pytest -s); DESIGN.md, "Covariant Lyapunov vectors", has the tables."""
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

import clv_numpy as V                                           # noqa: E402
import lyapunov_numpy as Y                                      # noqa: E402
import tracer_numpy as T                                        # noqa: E402

FB_EINVAL = 1


@functools.lru_cache(maxsize=None)
def _run(kind, f32=False):
    """the recipe's Ginelli run, computed once per kind and storage"""
    return V.ginelli(kind, f32=f32)


def _factors(n, m, seed):
    """n random upper triangular factors with a diagonal in [0.5, 2]: well conditioned"""
    rng = np.random.default_rng(seed)
    R = np.triu(0.3 * rng.standard_normal((n, m, m)), 1)
    R[:, np.arange(m), np.arange(m)] = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (n, m)))
    return R


# ---- 1. the recursion ----
@pytest.mark.parametrize("m", [1, 3, 8])
def test_clv_coefficients_against_an_independent_solve(m):
    import xlab_fftbarotropic_amd as X
    R, ce = _factors(12, m, 7 + m), V.c_end(m, seed=3)
    Cg, lg = X.clv_coefficients(R, ce)
    Cw, lw = V.coefficients(R, ce)
    # element by element, too: row i of R_n C_(n-1) D_n^-1 against C_n
    worst = 0.0
    for n in range(12):
        back = np.array([[sum(R[n, i, k] * Cg[n, k, j] for k in range(i, m)) for j in range(m)] for i in range(m)]) * np.exp(-lg[n])
        worst = max(worst, float(np.abs(back - Cg[n + 1]).max()))
    print("clv_coefficients, M = %d, 12 factors: max |C - C_ref| = %.3g, max |log_growth - ref| = %.3g, max |R C D^-1 - C_next| = %.3g"
          % (m, np.abs(Cg - Cw).max(), np.abs(lg - lw).max(), worst))
    assert Cg.shape == (13, m, m) and lg.shape == (12, m)
    assert np.abs(Cg - Cw).max() <= 1e-12 and np.abs(lg - lw).max() <= 1e-12 and worst <= 1e-12
    assert np.array_equal(Cg, np.triu(Cg))
    assert np.abs(np.linalg.norm(Cg, axis=1) - 1).max() <= 1e-14
    if m > 1:
        assert np.abs(Cg[0, 0, 1]) > 1e-3                        # (the off-diagonal coefficients matter)


def test_clv_coefficients_default_end_is_seeded_upper_triangular_with_unit_columns():
    import xlab_fftbarotropic_amd as X
    R = _factors(1, 4, 1)
    a, b, c = (X.clv_coefficients(R, seed=s)[0][-1] for s in (0, 0, 1))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a, np.triu(a)) and np.abs(np.linalg.norm(a, axis=0) - 1).max() <= 1e-15 and (np.diagonal(a) != 0).all()


# ---- 2. refusals of bad factors ----
def test_clv_coefficients_refuses_bad_factors():
    import xlab_fftbarotropic_amd as X
    good = _factors(3, 3, 2)
    X.clv_coefficients(good)
    for what, (i, j), value in (("triangular", (2, 0), 1e-3), ("finite", (0, 1), np.nan), ("finite", (1, 1), np.inf), ("positive", (1, 1), 0.0),
                                ("positive", (2, 2), -1.0)):
        bad = good.copy()
        bad[1][i, j] = value
        with pytest.raises(ValueError, match=what):
            X.clv_coefficients(bad)
    with pytest.raises(ValueError):
        X.clv_coefficients(good[0])
    with pytest.raises(ValueError, match="C_end"):
        X.clv_coefficients(good, C_end=np.ones((3, 3)))
    for steps, every, settle in ((0, 1, 0), (1, 0, 0), (1, 1, -1)):
        with pytest.raises(ValueError):
            X.clv(None, steps, every, settle)


# ---- 3. the covariance identity in float64 ----
@pytest.mark.parametrize("kind", Y.KINDS)
def test_covariance_identity_in_float64(kind):
    """T V_n = V_(n+1) D for every window slot and column: sine <= 1e-12, ln growth against log_growth <= 1e-10"""
    run = _run(kind)
    worst_s = worst_g = 0.0
    for n in range(V.WINDOW):
        for j in range(3):
            s, g = V.covariance_defect(run, n, j)
            worst_s, worst_g = max(worst_s, s), max(worst_g, abs(g))
    print("covariance in float64, %s, 64^2, M = 3, %d steps per interval, %d + %d intervals: largest sine = %.3g, largest |ln growth - log_growth| = %.3g; "
          "log_growth = %s" % (kind, V.EVERY, V.WINDOW, V.SETTLE, worst_s, worst_g, np.array2string(run.log_growth, precision=6)))
    assert worst_s <= 1e-12
    assert worst_g <= 1e-10


def test_covariance_holds_for_any_end():
    """another C_end gives other vectors; they are covariant all the same"""
    run = V.ginelli("enstrophy", C_end=V.c_end(3, seed=11))
    assert np.abs(run.C[0] - _run("enstrophy").C[0]).max() > 1e-3
    for j in range(3):
        s, g = V.covariance_defect(run, 1, j)
        assert s <= 1e-12 and abs(g) <= 1e-10


# ---- 4. conditioning ----
@pytest.mark.parametrize("kind", Y.KINDS)
def test_coefficients_are_well_conditioned_on_every_window_slot(kind):
    """cond(C_n) <= 10: the precondition of the GPU's covariance bar (an error of the bases enters V times at most that)"""
    run = _run(kind)
    conds = [float(np.linalg.cond(c)) for c in run.C]
    print("cond(C_n), %s: %s" % (kind, ["%.3g" % c for c in conds]))
    assert len(conds) == V.WINDOW + 1 and max(conds) <= 10.0


# ---- 5. the probes ----
@pytest.mark.parametrize("kind", Y.KINDS)
def test_probes_give_the_gpu_bar_teeth(kind):
    """V_n stored as complex64 (float32 storage of the vectors alone): the right C leaves a sine <= 1e-6; the next slot's C, the
    transpose and the identity each move column 1 or 2 by >= 1e-3, a thousand times the GPU's bar of 1e-5 and more.  Column 0 is Q_0
    under every upper triangular choice and proves nothing: it is not looked at."""
    run = _run(kind)
    n = 1

    def moved(Cm):
        """the sines of the columns 1 and 2 of T (Q_n Cm, stored as complex64) against V_(n+1)"""
        stored = [v.astype(np.complex64).astype(np.complex128) for v in V.combine(run.Q[n], Cm)]
        out, _ = V.step_from_slot(run, n, stored)
        want = V.vectors(run, n + 1)
        return [V.sine(run.m, out[j], want[j], kind) for j in (1, 2)]
    right = moved(run.C[n])
    wrong = {"C of the next slot": moved(run.C[n + 1]), "the transpose": moved(run.C[n].T / np.linalg.norm(run.C[n].T, axis=0)), "the identity": moved(np.eye(3))}
    print("probes, %s, slot %d: right C, complex64 storage: sines %s; %s" % (kind, n, ["%.3g" % s for s in right],
                                                                             "; ".join("%s: %s" % (k, ["%.3g" % s for s in v]) for k, v in wrong.items())))
    assert max(right) <= 1e-6
    for k, v in wrong.items():
        assert max(v) >= 1e-3, k


# ---- the figures behind the GPU's comparison with the float64 run ----
def test_float32_storage_against_float64_stays_inside_the_recorded_figures():
    """the same recipe and C_end in float64 and in float32 storage (mgs_f32, combine_f32, bases rounded to complex64 after every step):
    the differences of log_r and log_growth and the sines between the vectors, per kind; clv_numpy.F32_* hold the largest, and the
    GPU's bars are 4 times those"""
    for kind in Y.KINDS:
        a, b = _run(kind), _run(kind, True)
        dr, dg = float(np.abs(a.log_r - b.log_r).max()), float(np.abs(a.log_growth - b.log_growth).max())
        ds = max(V.sine(a.m, x, y, kind) for n in range(V.WINDOW + 1) for x, y in zip(V.vectors(a, n), V.vectors(b, n)))
        print("float32 storage against float64, %s: max |log_r - log_r64| = %.3g, max |log_growth - log_growth64| = %.3g, largest sine = %.3g" % (kind, dr, dg, ds))
        assert dr <= V.F32_LOG_R and dg <= V.F32_LOG_GROWTH and ds <= V.F32_SINE


# ---- 6. a fluid at rest ----
@pytest.mark.parametrize("kind", Y.KINDS)
def test_fluid_at_rest(kind):
    """zeta = 0 and the set A, A + B, A + B + C of three modes in the order of their decay: Q_n is (A, B, C) up to sign, R_n is
    diagonal, and after REST_SETTLE intervals the recursion has forgotten C_end: C_n is the identity up to sign (off-diagonal <= 1e-10)
    and log_growth is ln rk4_factor(nu lap dt) times the interval, to 1e-12"""
    n = 64
    m = Y.SubspaceModel64(n, n, nu=V.REST_NU, dt=V.REST_DT)
    m.set_vort(np.zeros((n, n)))
    z = np.array([m.nu * m.lap[mx, my] * m.dt for mx, my in V.REST_MODES])
    want = V.REST_EVERY * np.log(T.rk4_factor(z))
    assert all(m.mask[mx, my] == 1.0 for mx, my in V.REST_MODES)
    assert (np.abs(z) <= 0.5).all() and np.abs(z / V.rest_z() - 1).max() <= 1e-6     # (inside RK4's stability range of 2.78; the float32 table)
    assert (-np.diff(want) >= 0.64).all()
    big = Y.SubspaceModel64(256, 256, nu=V.REST_NU, dt=V.REST_DT)    # (tables only) the GPU's grid: every mode that evolves there is stable
    assert all(big.mask[mx, my] == 1.0 for mx, my in V.REST_MODES) and float(np.abs(big.nu * big.lap * big.dt * big.mask).max()) <= 2.78
    A, B, Cm = V.rest_spectra(n)
    assert max(np.abs(np.fft.rfft2(f) - s).max() for f, s in zip(V.rest_fields(n), (A, B, Cm))) <= 1e-9 * n * n
    m.dcs = [A, A + B, A + B + Cm]
    run = V.ginelli(kind, model=m, every=V.REST_EVERY, window=3, settle=V.REST_SETTLE)
    import xlab_fftbarotropic_amd as X
    Cg, lg = X.clv_coefficients(run.R, V.c_end(3))
    off = max(float(np.abs(c - np.diag(np.diagonal(c))).max()) for c in Cg[:4])
    err = float(np.abs(lg[:3] - want).max())
    print("fluid at rest, %s: z = %s per step, ln r_ii per interval = %s; window slots: largest off-diagonal |C_ij| = %.3g, max |log_growth - %d ln R(z)| = %.3g"
          % (kind, z, want, off, V.REST_EVERY, err))
    assert np.abs(run.log_r - want).max() <= 1e-12
    assert off <= 1e-10
    assert err <= 1e-12
    assert np.abs(np.abs(np.diagonal(Cg[0])) - 1).max() <= 1e-12


# ---- the entry points' argument checks ----
def _both(stem):
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    return L, [(name, getattr(L, name)) for name in ("fb_model_" + stem, "fb_slab_" + stem)]


def test_the_new_pairs_are_in_a_table_of_their_own():
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    assert sorted(B._CLV_PAIRS) == ["tangent_combine", "tangent_tape", "tangent_tape_count", "tangent_tape_push"]
    assert not set(B._CLV_PAIRS) & set(B._PAIRS)
    for stem in B._CLV_PAIRS:
        assert "fb_model_" + stem in B.SIGNATURES and "fb_slab_" + stem in B.SIGNATURES
    for name in ("tangent_tape", "push_tangents", "tangent_tape_count", "combine_tangents", "clv", "clv_vectors"):
        assert hasattr(B.ModelSurface, name) and name not in vars(X.Model)


def test_tangent_tape_names_a_negative_depth_before_the_null_handle():
    L, fns = _both("tangent_tape")
    for name, fn in fns:
        assert fn(None, -1) == FB_EINVAL, name
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and "depth" in msg and "NULL" not in msg, (name, msg)
        assert fn(None, 0) == FB_EINVAL and L.fb_last_error().decode().startswith(name + ": NULL ")


def test_null_outputs_and_coefficients_are_named_before_the_null_handle():
    L, fns = _both("tangent_tape_count")
    one = C.c_int()
    for name, fn in fns:
        for args in ((None, C.byref(one)), (C.byref(one), None)):
            assert fn(None, *args) == FB_EINVAL, name
            msg = L.fb_last_error().decode()
            assert msg.startswith(name + ": NULL output"), (name, msg)
    L, fns = _both("tangent_combine")
    for name, fn in fns:
        assert fn(None, -1, None) == FB_EINVAL, name
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": NULL coefficients"), (name, msg)
        buf = (C.c_double * 64)()
        assert fn(None, -5, C.cast(buf, C.c_void_p)) == FB_EINVAL and L.fb_last_error().decode().startswith(name + ": NULL ")   # (the slot's range needs the model)
