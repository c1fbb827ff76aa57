"""CPU checks of the point observations and the 4D-Var gradient: the float64 reference (tests/obs_numpy.py) shown to hold the
dot-product identity of H for every kind, its gradient checked against central finite differences of J, the L-BFGS of
binding.fit_initial run on it for the twin experiment; the figures of the float32 restatement from which the bars of
tests/test_gpu_obs.py are taken; and the entry points declared, exported, bound, with the argument checks that run before any HIP
call.  No GPU needed."""
import ctypes
import functools
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
import obs_numpy as O                                           # noqa: E402
import tracer_numpy as T                                        # noqa: E402

STEMS = ("scatter", "observe", "obs_misfit", "adjoint_add_obs")
NAMES = tuple("fb_%s_%s" % (k, n) for k in ("model", "slab") for n in STEMS)
METHODS = ("scatter", "observe", "obs_misfit", "adjoint_add_obs", "fourdvar", "fit_initial")
FB_EINVAL = 1


def _ref(nx, ny, cls=O.ObsModel64):
    return cls(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))


# ---- H and its transpose ----
@pytest.mark.parametrize("n", [1, O.NPTS])
@pytest.mark.parametrize("kind", O.KINDS)
def test_dot_product_identity_of_h_in_float64(kind, n):
    """|<H zeta, w> - <zeta, H^T w>| / (|H zeta| |w|) <= 1e-12 for every kind at 192 x 64 (an odd-factor and a short axis), zeta white
    noise plus the vortex, never dealiased; the positions of obs_numpy.positions: grid points, wrapping stencils, far and negative
    positions, one position twice; and a single point"""
    nx, ny = 192, 64
    zeta = A.adjoint_inputs(nx, ny, 3e-2)[0].astype(np.float64)
    xy, w = O.positions(nx, ny, n), O.weights(n)
    res = O.h_identity(_ref(nx, ny), kind, zeta, xy, w)
    print("identity of H, float64, %s, n = %d: %.3g" % (kind, n, res))
    assert res <= 1e-12


def test_positions_cover_the_edge_cases():
    nx, ny = 192, 64
    xy = O.positions(nx, ny)
    lx, dx, dy = O.P.widen(O.LX), O.P.widen(O.LX) / nx, O.P.widen(O.LY) / ny
    sx, sy = xy[:, 0] / dx, xy[:, 1] / dy
    assert ((sx == np.floor(sx)) & (sy == np.floor(sy))).sum() >= 4                          # on grid points
    for s, n in ((sx, nx), (sy, ny)):
        assert ((s > 0) & (s < 1)).any() and ((s > n - 1) & (s < n)).any()                   # the first and the last cell: the stencil wraps
    assert (xy < 0).any() and (np.abs(xy[:, 0]) > 2 * lx).any()                              # negative, and many domain lengths away
    assert np.array_equal(xy[-1], xy[40])                                                     # one stencil added to twice


def test_scatter_is_the_transpose_of_sample_and_skips_what_is_not_finite():
    nx, ny = 64, 96
    rng = np.random.default_rng(3)
    f = rng.standard_normal((nx, ny))
    xy, w = O.positions(nx, ny), O.weights(O.NPTS)
    g, a = O.scatter64(xy, w, nx, ny, terms=True)
    assert abs(np.vdot(O.sample64(f, xy), w) - np.vdot(f, g)) <= 1e-12 * np.linalg.norm(f) * np.linalg.norm(w)
    assert abs(g.sum() - w.sum()) <= 1e-13 * a.sum()                                          # the weights of a point sum to 1
    xy2, w2 = xy.copy(), w.copy()
    xy2[7, 1], w2[9] = np.nan, np.inf
    keep = np.ones(O.NPTS, bool)
    keep[[7, 9]] = False
    assert np.array_equal(O.scatter64(xy2, w2, nx, ny), O.scatter64(xy[keep], w[keep], nx, ny))
    assert np.isnan(O.sample64(f, xy2)[7])


# ---- the gradient ----
@functools.lru_cache(maxsize=None)
def _gradient_case(nx, ny):
    m = _ref(nx, ny)
    v, src, sets, d = O.gradient_case(nx, ny, m)
    m.src = src.astype(np.float64)
    J, g, res = O.fourdvar(m, v, sets)
    return m, v, src, sets, d, J, g, res


def test_gradient_against_central_finite_differences():
    """<grad, d> of the float64 reference against (J(z0 + eps d) - J(z0 - eps d)) / (2 eps) over a sweep of eps, at 64^2 with the
    gradient case's sets (u and v at the steps 2, 4, 6, zeta at step 0; noisy data, so no residual is small): the best eps agrees to
    1e-7 relative"""
    n = 64
    m = _ref(n, n)
    v, src, sets, d = O.gradient_case(n, n, m)
    m.src = src.astype(np.float64)
    z0 = v.astype(np.float64)
    d = d.astype(np.float64) / np.abs(d).max() * np.abs(z0).max()
    J, g, _ = O.fourdvar(m, z0, sets)
    want = float(np.vdot(g, d))
    errs = {}
    for eps in (1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        fd = (O.fourdvar(m, z0 + eps * d, sets)[0] - O.fourdvar(m, z0 - eps * d, sets)[0]) / (2 * eps)
        errs[eps] = abs(fd / want - 1)
    print("gradient against central differences, 64^2: J = %.6g, <grad, d> = %.6g, relative error per eps: %s"
          % (J, want, ", ".join("%g: %.2g" % kv for kv in errs.items())))
    assert min(errs.values()) <= 1e-7
    assert abs(want) > 1e-3 * np.linalg.norm(g) * np.linalg.norm(d)                          # not an accident of a vanishing product


def test_gradient_with_a_background_term_and_a_set_at_step_zero_alone():
    n = 64
    m = _ref(n, n)
    v, src, sets, d = O.gradient_case(n, n, m)
    z0, d = v.astype(np.float64), d.astype(np.float64)
    zb = 0.9 * z0
    only0 = [s for s in sets if s.step == 0]
    for obs, bg in ((sets, (zb, 1e-3)), (only0, None)):
        g = O.fourdvar(m, z0, obs, bg)[1]
        eps = 1e-3
        fd = (O.fourdvar(m, z0 + eps * d, obs, bg)[0] - O.fourdvar(m, z0 - eps * d, obs, bg)[0]) / (2 * eps)
        assert abs(fd / float(np.vdot(g, d)) - 1) <= 1e-6


@pytest.mark.parametrize("nx,ny", O.GRAD_GRIDS)
def test_gradient_case_float32_figures(nx, ny):
    """The float32 restatement of the gradient case on the grids of the GPU test: grad and J against float64 (the GPU's bars are 1e-5),
    and the residual of <grad, d> = sum <r, H T_k d> against the restatement's own tangent.  The GPU's bar, GRAD_DOT_BAR, is 4 x the
    largest figure recorded in obs_numpy.GRAD_F32 (measured once on one CPU).  The figure is a draw of rounding errors that depends on
    the FFT library's summation order, which differs between CPUs and thread counts (3.2e-12 and 6.4e-12 were measured for the 256^2
    case on two machines), so what is asserted here is what the GPU is held to: any float32 evaluation stays within the bar"""
    m, v, src, sets, d, J, g, res = _gradient_case(nx, ny)
    assert O.tangent_residual(m, v, sets, d, g, res) <= 1e-12
    f = O.Float32Obs(m, src)
    J32, g32, r32 = O.fourdvar(f, v, sets)
    fig = O.tangent_residual(f, v, sets, d, g32, r32)
    print("gradient case %dx%d, float32 on the CPU: grad rel L2 %.3g, J rel %.3g, tangent residual %.3g (recorded %.3g)"
          % (nx, ny, rel_l2(g32, g), abs(J32 / J - 1), fig, O.GRAD_F32[(nx, ny)]))
    assert rel_l2(g32, g) <= 2.5e-6 and abs(J32 / J - 1) <= 2.5e-6
    assert fig <= O.GRAD_DOT_BAR
    assert O.GRAD_DOT_BAR == 4 * max(O.GRAD_F32.values())


@pytest.mark.parametrize("case", O.H_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in O.H_CASES])
def test_h_identity_float32_figures(case):
    """The residual of the identity of H for the float32 restatement, every kind, on the grids of the GPU test.  The GPU's bar, H_DOT_BAR,
    is 4 x the largest figure recorded in obs_numpy.H_CASES (measured once on one CPU).  The figure depends on the FFT library's
    summation order, which differs between CPUs and thread counts (1.0e-8 and 4.6e-8 were measured for zeta at 64 x 4096 on two
    machines), so what is asserted here is what the GPU is held to: any float32 evaluation stays within the bar"""
    nx, ny = case.nx, case.ny
    zeta = A.adjoint_inputs(nx, ny, 3e-2)[0]
    xy, w = O.positions(nx, ny), O.weights(O.NPTS)
    ref = _ref(nx, ny)
    f = O.Float32Obs(ref)
    figs = {k: O.h_identity(f, k, zeta, xy, w) for k in O.KINDS}
    print("identity of H %dx%d, float32 on the CPU: %s (recorded %.3g)" % (nx, ny, ", ".join("%s %.3g" % kv for kv in figs.items()), case.f32))
    assert max(figs.values()) <= O.H_DOT_BAR
    assert O.H_DOT_BAR == 4 * max(k.f32 for k in O.H_CASES)


# ---- the minimiser ----
class _Quadratic:
    """J = 1/2 (z - a)^T D (z - a) + c with a diagonal D of condition 1e3: fit_initial on something with a fourdvar and nothing else"""

    def __init__(self, n=40):
        import torch
        self.torch = torch
        g = torch.Generator().manual_seed(5)
        self.a = torch.randn(n, dtype=torch.float64, generator=g)
        self.D = torch.logspace(0, 3, n, dtype=torch.float64)

    def fourdvar(self, z, obs, background=None):
        r = z - self.a
        return float(0.5 * (r * self.D * r).sum()) + 0.25, self.D * r


def test_fit_initial_minimises_a_quadratic():
    import torch
    import xlab_fftbarotropic_amd as X
    q = _Quadratic()
    z, hist, evals = X.fit_initial(q, torch.zeros(40, dtype=torch.float64), None, 200, history=8)
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert hist[-1] - 0.25 <= 1e-10 * (hist[0] - 0.25)
    assert float((z - q.a).norm() / q.a.norm()) <= 1e-5
    assert evals >= len(hist) and isinstance(evals, int)
    z1, hist1, evals1 = X.fit_initial(q, np.zeros(40), None, 0)
    assert len(hist1) == 1 and evals1 == 1 and float(z1.abs().max()) == 0.0


def test_twin_experiment_on_the_float64_reference():
    """fit_initial on the float64 reference for the twin experiment of tests/test_gpu_obs.py (64^2, the truth's u and v at 256 points
    at four times, the first guess the truth scaled by 0.8 and shifted by two cells): the truth's vorticity changes by >= 10 % over
    the window, J falls at every accepted iteration, J_K / J_0 after K = 10 is the recorded figure to 10 %, and z0 ends closer to
    the truth than it started"""
    import torch
    import xlab_fftbarotropic_amd as X
    truth, guess, sets, change = O.twin_case(X.make_field)
    assert change >= 0.1 and abs(change / O.TWIN_CHANGE - 1) <= 0.01
    model = O.Fourdvar64(O.twin_model())
    z, hist, evals = X.fit_initial(model, torch.from_numpy(guess.astype(np.float64)), sets, O.TWIN_ITERS)
    e0, e1 = rel_l2(guess, truth), rel_l2(z.numpy(), truth)
    print("twin experiment, float64: the truth changes by %.3g over the window; J = %s; J_K / J_0 = %.4g (recorded %.4g); %d evaluations; "
          "z0 off by %.3g at the start, %.3g at the end" % (change, ["%.4g" % j for j in hist], hist[-1] / hist[0], O.TWIN_RATIO, evals, e0, e1))
    assert len(hist) == O.TWIN_ITERS + 1 and evals == model.calls
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] / hist[0] / O.TWIN_RATIO - 1) <= 0.1
    assert e1 < e0


# ---- the entry points ----
def test_obs_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None, n
    assert set(B._OBS_PAIRS) == set(STEMS) and not set(B._OBS_PAIRS) & set(B._PAIRS)
    from importlib import import_module
    S = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (X.Model, S.EngineSlab):
        for n in METHODS:
            assert callable(getattr(cls, n, None)), (cls, n)
    assert callable(X.fourdvar) and callable(X.fit_initial) and X.OBS_KINDS == {"vort": 0, "u": 1, "v": 2, "psi": 3}


def test_obs_argument_errors_are_rejected_without_a_device():
    """every refusal that needs no handle comes before the NULL handle's, under the function's own name: kind outside [0, 3], a NULL
    pointer, n = 0 and n = 2^24 + 1; sigma alone may be NULL"""
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    p = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    big = (1 << 24) + 1
    for k in ("model", "slab"):
        cases = [("scatter", (p, p, 0, p), "n outside"), ("scatter", (p, p, big, p), "n outside"), ("scatter", (None, p, 1, p), "NULL positions"),
                 ("scatter", (p, None, 1, p), "NULL positions"), ("scatter", (p, p, 1, None), "NULL positions"),
                 ("observe", (4, p, 1, p), "kind"), ("observe", (-1, p, 1, p), "kind"), ("observe", (0, None, 1, p), "NULL positions"),
                 ("observe", (0, p, 1, None), "NULL positions"), ("observe", (0, p, 0, p), "n outside"), ("observe", (3, p, big, p), "n outside"),
                 ("obs_misfit", (None, p, p, 1, p, p), "NULL values"), ("obs_misfit", (p, None, p, 1, p, p), "NULL values"),
                 ("obs_misfit", (p, p, p, 1, None, p), "NULL values"), ("obs_misfit", (p, p, p, 1, p, None), "NULL values"),
                 ("obs_misfit", (p, p, None, 0, p, p), "n outside"), ("obs_misfit", (p, p, None, big, p, p), "n outside"),
                 ("adjoint_add_obs", (4, p, p, 1), "kind"), ("adjoint_add_obs", (0, None, p, 1), "NULL positions"),
                 ("adjoint_add_obs", (0, p, None, 1), "NULL positions"), ("adjoint_add_obs", (0, p, p, 0), "n outside"),
                 ("adjoint_add_obs", (0, p, p, big), "n outside")]
        for stem, args, phrase in cases:
            name = "fb_%s_%s" % (k, stem)
            assert getattr(L, name)(None, *args) == FB_EINVAL, (name, args)
            msg = L.fb_last_error().decode()
            assert msg.startswith(name + ": " + phrase), (name, args, msg)
        assert getattr(L, "fb_%s_obs_misfit" % k)(None, p, p, None, 1, p, p) == FB_EINVAL                # sigma == NULL is an argument like any other
        assert L.fb_last_error().decode().startswith("fb_%s_obs_misfit: NULL %s" % (k, k))


def test_observations_and_kinds_refuse_bad_input_without_a_device():
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    with pytest.raises(ValueError, match="kind"):
        B.obs_kind("zeta")
    assert [B.obs_kind(k) for k in O.KINDS] == [0, 1, 2, 3] and B.obs_kind(2) == 2
    with pytest.raises(ValueError, match="iters"):
        X.fit_initial(_Quadratic(), np.zeros(40), None, -1)
