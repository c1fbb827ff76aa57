"""CPU checks of the tangent replay and of Gauss-Newton 4D-Var: the float64 reference (tests/replay_numpy.py) shown to replay the live
tangent, its Hessian-vector product against a dense A^T R^-1 A of a small grid, symmetric and positive, the background term; binding's
gauss_newton_hvp and fit_incremental run on the float64 model and give what the reference loops give; the twin experiment; the
figures of the float32 restatement from which the bars of tests/test_gpu_replay.py are taken; and the entry points declared,
exported, bound, with the argument checks that run before any HIP call.  No GPU needed."""
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
import replay_numpy as R                                        # noqa: E402
import singular_numpy as S                                      # noqa: E402

STEMS = ("tangent_replay", "adjoint_rewind", "observe_tangent")
NAMES = tuple("fb_%s_%s" % (k, n) for k in ("model", "slab") for n in STEMS)
METHODS = ("tangent_replay", "adjoint_rewind", "observe_tangent", "fourdvar", "gauss_newton_hvp", "fit_incremental", "singular_vectors")
FB_EINVAL = 1


# ---- the replay ----
@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64)])
def test_replay_over_the_tape_is_the_live_tangent(nx, ny):
    """5 steps recorded with the tangent riding along; the same perturbation replayed over the tape, in one piece and as 3 + 2 steps,
    equals it to 1e-12; the vorticity, the tape and its fill mark are as they were; and a sweep after the replay gives lam_0's bits"""
    v, dz, src, lam = A.adjoint_inputs(nx, ny, 3e-2)
    m = A.recipe_model(nx, ny, v, dz, src, cls=R.ReplayModel64)
    m.record_adjoint(5)
    m.step(5)
    live, vort = m.tangent(), m.vort()
    m.set_tangent(dz)
    m.tangent_replay(0, 5)
    whole = m.tangent()
    m.set_tangent(dz)
    m.tangent_replay(0, 3)
    m.tangent_replay(3, 2)
    assert rel_l2(whole, live) <= 1e-12 and rel_l2(m.tangent(), whole) <= 1e-12
    assert rel_l2(live, dz) > 1e-3                              # the tangent has moved
    assert np.array_equal(m.vort(), vort) and m.adjoint_recorded() == 5
    m.set_adjoint(lam)
    m.adjoint_back(5)
    want = A.run_case(nx, ny, v, dz, src, lam, 5).adjoint()
    assert np.array_equal(m.adjoint(), want)
    m.adjoint_rewind(-1)
    m.set_adjoint(lam)
    m.adjoint_back(5)
    assert np.array_equal(m.adjoint(), want) and m.adjoint_recorded() == 0
    m.tangent_replay(0, 0)
    with pytest.raises(ValueError):
        m.tangent_replay(3, 3)


def test_rewind_of_the_reference_tape():
    m = A.recipe_model(64, 64, *A.adjoint_inputs(64, 64, 3e-2)[:3], cls=R.ReplayModel64)
    m.record_adjoint(5)
    m.step(5)
    m.set_adjoint(np.zeros((64, 64)))
    m.adjoint_back(2)
    with pytest.raises(ValueError):
        m.adjoint_rewind(3)
    m.adjoint_rewind(1)
    assert m.adjoint_recorded() == 4
    m.adjoint_back(1)
    m.step(1)                                                   # overwrites slot 3; slot 4 is gone
    assert m.adjoint_recorded() == 4 and m.adjoint_top() == 4
    with pytest.raises(ValueError):
        m.adjoint_rewind(1)


# ---- the Hessian-vector product against a dense matrix ----
DENSE_NPTS = 40


@functools.lru_cache(maxsize=None)
def _dense():
    """32^2, 4 steps of 20 s (singular_numpy's dense case): zeta at step 0, u at step 2, v at step 4, 40 points each with their own sigma;
    A = R^-1/2 H T column by column from the float64 tangent model and observe_tangent"""
    n = S.DENSE_N
    v = A.adjoint_inputs(n, n, A.PATH_CASES[0].vort_noise)[0]
    rng = np.random.default_rng(O.SEED + 50)
    sets = [O.Obs(step, kind, O.positions(n, n, DENSE_NPTS, seed=O.SEED + 51 + step), rng.standard_normal(DENSE_NPTS), 0.5 + rng.random(DENSE_NPTS))
            for step, kind in ((0, "vort"), (2, "u"), (4, "v"))]
    m = R.ReplayModel64(n, n, nu=A.G.NU, dt=S.DENSE_DT)
    m.set_vort(v)
    z0 = m.spectrum()
    a = np.empty((3 * DENSE_NPTS, n * n))
    e = np.zeros(n * n)
    for j in range(n * n):
        e[j] = 1.0
        m.set_spectrum(z0)
        m.set_tangent(e.reshape(n, n))
        rows, at = [], 0
        for o in sets:
            m.step(o.step - at)
            at = o.step
            rows.append(m.observe_tangent(o.kind, o.xy) / o.sigma)
        a[:, j] = np.concatenate(rows)
        e[j] = 0.0
    m.dc = None
    R.fourdvar_keep(m, v, sets)
    return m, v, sets, a


def test_hessian_vector_product_against_the_dense_matrix():
    """H_GN v = A^T A v to 1e-10; <w, H v> = <v, H w> to 1e-12 of |H v| |w|; v^T H v > 0; twice the same; the background term adds
    v / sigma_b^2; the tape is whole after every product"""
    m, v0, sets, a = _dense()
    n = S.DENSE_N
    rng = np.random.default_rng(O.SEED + 60)
    v, w = (rng.standard_normal((n, n)).astype(np.float32).astype(np.float64) for _ in range(2))
    hv, hw = R.gauss_newton_hvp(m, v, sets), R.gauss_newton_hvp(m, w, sets)
    want = (a.T @ (a @ v.ravel())).reshape(n, n)
    err, sym = rel_l2(hv, want), R.symmetry_residual(hv, hw, v, w)
    print("H_GN v against the dense A^T A v at %d^2: %.3g; symmetry residual %.3g; v^T H v = %.6g" % (n, err, sym, float(np.vdot(v, hv))))
    assert err <= 1e-10
    assert sym <= 1e-12
    assert float(np.vdot(v, hv)) > 0.0
    assert np.array_equal(R.gauss_newton_hvp(m, v, sets), hv)
    assert m.adjoint_recorded() == 4 and m.dc is None
    sb = 0.37
    hb = R.gauss_newton_hvp(m, v, sets, (np.zeros((n, n)), sb))
    assert np.array_equal(hb, hv + v / sb ** 2)


def test_binding_helpers_on_the_float64_model_give_the_reference_s_results():
    """binding.fourdvar(keep_tape=True), binding.gauss_newton_hvp and binding.fit_incremental, run on the float64 model behind
    replay_numpy.Torch64, return exactly what the reference loops return; keep_tape changes neither J nor grad and leaves the tape;
    the product steps nothing nonlinear; fit_incremental frees the tape"""
    import torch
    import xlab_fftbarotropic_amd as X
    m, v0, sets, _ = _dense()
    n = S.DENSE_N
    tsets = R.torch_obs(sets)
    zb, sb = (0.9 * v0).astype(np.float32), 0.5
    other = R.ReplayModel64(n, n, nu=A.G.NU, dt=S.DENSE_DT)
    tm = R.Torch64(other)
    z = torch.from_numpy(v0.astype(np.float64))
    J0, g0 = X.fourdvar(tm, z, tsets, (torch.from_numpy(zb), sb))
    assert other.adjoint_recorded() == 0 and other.depth == 0
    J1, g1 = X.fourdvar(tm, z, tsets, (torch.from_numpy(zb), sb), keep_tape=True)
    assert other.adjoint_recorded() == 4 and other.adjoint_top() == 4
    Jr, gr = R.fourdvar_keep(m, v0, sets, (zb, sb))
    assert J0 == J1 == Jr and torch.equal(g0, g1) and np.array_equal(g1.numpy(), gr)
    v = np.random.default_rng(O.SEED + 61).standard_normal((n, n))
    tm.calls.clear()
    hv = X.gauss_newton_hvp(tm, torch.from_numpy(v), tsets, (None, sb))
    assert hv.dtype == torch.float64 and np.array_equal(hv.numpy(), R.gauss_newton_hvp(m, v, sets, (None, sb)))
    assert "step" not in tm.calls and "set_vort" not in tm.calls and tm.calls["tangent_replay"] == 2
    assert other.adjoint_recorded() == 4 and other.dc is None
    guess = (0.8 * v0.astype(np.float64))
    got = X.fit_incremental(tm, torch.from_numpy(guess), tsets, 2, 3, (torch.from_numpy(zb), sb))
    want = R.fit_incremental(m, guess, sets, 2, 3, (zb, sb))
    assert other.depth == 0 and m.depth == 0
    assert np.array_equal(got[0].numpy(), want[0]) and got[1] == want[1] and got[2:] == want[2:]
    assert len(got[1]) == 3 and got[1][2] < got[1][1] < got[1][0] and got[3] == 6
    R.fourdvar_keep(m, v0, sets)                                # (the cached case's tape, for whichever test comes next)


def test_python_argument_checks_raise_before_the_library_is_called():
    import torch
    import xlab_fftbarotropic_amd as X

    class Untouched:
        device = "cpu"

        def __getattr__(self, name):
            raise AssertionError("the model was asked for %s" % name)
    u = Untouched()
    u.torch = torch
    sets = R.torch_obs([O.Obs(2, "u", np.zeros((4, 2)), np.zeros(4), None)])
    drift = [R.TObs(2, X.POSITION, None, torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64))]
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match="keep_tape"):
        X.fourdvar(u, z, sets, keep_tape=True, checkpoint_every=2)
    with pytest.raises(ValueError, match="keep_tape"):
        X.fourdvar(u, z, drift, keep_tape=True, particles=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="gauss_newton_hvp"):
        X.gauss_newton_hvp(u, z, [])
    with pytest.raises(ValueError, match="gauss_newton_hvp"):
        X.gauss_newton_hvp(u, z, drift)
    for kw in (dict(outer=-1, inner=2), dict(outer=1, inner=0)):
        with pytest.raises(ValueError, match="fit_incremental"):
            X.fit_incremental(u, z, sets, **kw)
    with pytest.raises(ValueError, match="replay"):
        X.singular_vectors(u, 2, 2, 1, replay=True, checkpoint_every=2)
    short = R.Torch64(R.ReplayModel64(32, 32))
    with pytest.raises(ValueError, match="keep_tape=True"):     # no tape: the window is not there
        X.gauss_newton_hvp(short, np.zeros((32, 32), np.float32), sets)
    assert not short.calls


# ---- the twin experiment ----
def test_twin_experiment_on_the_reference():
    """obs_numpy.twin_case: fit_incremental(outer=3, inner=8) on float64 brings J to GN_TWIN_RATIO of its start (to 10 %) in 4 nonlinear
    evaluations and 24 products, below what fit_initial reaches in 13 evaluations (TWIN_RATIO): the claim of the feature"""
    truth, guess, sets, _ = O.twin_case()
    m = R.ReplayModel64(O.TWIN_N, O.TWIN_N, nu=O.TWIN_NU, dt=O.TWIN_DT)
    z, hist, evals, hvps = R.fit_incremental(m, guess, sets, R.GN_TWIN_OUTER, R.GN_TWIN_INNER)
    ratio = hist[-1] / hist[0]
    print("Gauss-Newton twin on float64: J = %s; J_K / J_0 = %.4g (recorded %.4g; L-BFGS %.4g); %d evaluations, %d products"
          % (["%.4g" % j for j in hist], ratio, R.GN_TWIN_RATIO, O.TWIN_RATIO, evals, hvps))
    assert len(hist) == R.GN_TWIN_OUTER + 1 and all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(ratio / R.GN_TWIN_RATIO - 1) <= 0.1
    assert ratio < O.TWIN_RATIO
    assert (evals, hvps) == (4, 24)
    assert rel_l2(z, truth) < rel_l2(guess, truth)


# ---- the float32 restatement ----
@pytest.mark.parametrize("nx,ny", O.GRAD_GRIDS)
def test_float32_restatement_of_the_hessian_vector_product(nx, ny):
    """the gradient case with its source: H_GN d and H_GN w (w white noise of d's rms) of the float32 restatement against float64, and its
    symmetry residual.  Its figures are draws of rounding, so it is held to the GPU's bars, not to its own table; the recorded figures
    are printed beside what this run gives"""
    ref = R.gradient_model(nx, ny)
    v, src, sets, d = O.gradient_case(nx, ny, ref)
    w = R.white_like(d)
    ref = R.gradient_model(nx, ny)
    ref.src = src.astype(np.float64)
    R.fourdvar_keep(ref, v, sets)
    h64 = [R.gauss_newton_hvp(ref, a, sets) for a in (d, w)]
    f = R.Float32Replay(ref, src)
    R.fourdvar_keep(f, v, sets)
    h32 = [R.gauss_newton_hvp(f, a, sets) for a in (d, w)]
    err = max(rel_l2(a, b) for a, b in zip(h32, h64))
    sym, sym64 = R.symmetry_residual(h32[0], h32[1], d, w), R.symmetry_residual(h64[0], h64[1], d, w)
    print("float32 restatement of H_GN v at %dx%d: error %.3g (recorded %.3g, bar %.3g); symmetry residual %.3g (recorded %.3g, bar %.3g; float64 %.3g)"
          % (nx, ny, err, R.HVP_F32[(nx, ny)], R.HVP_BAR, sym, R.HVP_SYM_F32[(nx, ny)], R.HVP_SYM_BAR, sym64))
    assert sym64 <= 1e-12
    assert err <= R.HVP_BAR
    assert sym <= R.HVP_SYM_BAR


def test_float32_figure_of_the_replayed_singular_vectors():
    """singular_numpy's case with every T v a replay over the tape of one forward run: float64 gives the subspace and the sigma of the
    stepped iteration; the float32 restatement's final subspace lies within SV_REPLAY_ANGLE_F32 of float64's (recorded, an upper
    bound to 1.5) and its sigma within SV_BAR; the GPU's bar is 4 x the angle's figure"""
    s64, v64 = S.sv_reference()
    r64, w64 = R.sv_replay_reference()
    r32, w32 = R.sv_replay_reference(float32=True)
    ang, err = S.principal_sine(w32, v64), float(np.max(np.abs(r32 / s64 - 1)))
    print("singular vectors by replay: float64 replay against the stepped iteration: sigma off by %.3g, angle %.3g; float32 on the CPU: sigma off by %.3g, sine of the largest principal angle %.3g"
          % (float(np.max(np.abs(r64 / s64 - 1))), S.principal_sine(w64, v64), err, ang))
    assert np.max(np.abs(r64 / s64 - 1)) <= 1e-12 and S.principal_sine(w64, v64) <= 1e-9
    assert err <= S.SV_BAR
    assert ang <= 1.5 * R.SV_REPLAY_ANGLE_F32


# ---- the entry points ----
def test_replay_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    B = sys.modules[X.Model.__module__]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    lib = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(lib, n), n
        assert n in X.EXPORTS and n in B.SIGNATURES, n
    assert set(B._REPLAY_PAIRS) == set(STEMS) and not set(B._REPLAY_PAIRS) & set(B._PAIRS)
    for stem in STEMS:                                          # the header's parameters after the handle, one for one
        decl = re.search(r"\bint\s+fb_model_%s\s*\(([^)]*)\)" % stem, src).group(1)
        assert len(decl.split(",")) == 1 + len(B._REPLAY_PAIRS[stem]) == len(B.SIGNATURES["fb_slab_" + stem][0]), stem
    from importlib import import_module
    slab = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (X.Model, slab.EngineSlab):
        for n in METHODS:
            assert callable(getattr(cls, n, None)), (cls, n)
    assert callable(X.gauss_newton_hvp) and callable(X.fit_incremental)


def test_argument_errors_are_rejected_without_a_device():
    """every refusal that needs no handle comes before the NULL handle's, under the function's own name"""
    import xlab_fftbarotropic_amd as X
    lib = X.lib()
    p = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    for k in ("model", "slab"):
        cases = [("tangent_replay", (-1, 1), "first < 0"), ("tangent_replay", (0, -1), "nsteps < 0"), ("tangent_replay", (0, 0), "NULL " + k),
                 ("tangent_replay", (0, 3), "NULL " + k), ("adjoint_rewind", (-2,), "n < -1"), ("adjoint_rewind", (-1,), "NULL " + k),
                 ("adjoint_rewind", (2,), "NULL " + k), ("observe_tangent", (0, 4, p, 4, p), "kind"), ("observe_tangent", (0, -1, p, 4, p), "kind"),
                 ("observe_tangent", (0, 0, None, 4, p), "NULL positions"), ("observe_tangent", (0, 0, p, 4, None), "NULL positions"),
                 ("observe_tangent", (0, 0, p, 0, p), "n outside"), ("observe_tangent", (0, 0, p, (1 << 24) + 1, p), "n outside"),
                 ("observe_tangent", (-1, 0, p, 4, p), "index < 0"), ("observe_tangent", (0, 0, p, 4, p), "NULL " + k)]
        for stem, args, phrase in cases:
            name = "fb_%s_%s" % (k, stem)
            assert getattr(lib, name)(None, *args) == FB_EINVAL, (name, args)
            msg = lib.fb_last_error().decode()
            assert msg.startswith(name + ": ") and phrase in msg, (name, args, msg)
