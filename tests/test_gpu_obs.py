"""Point observations and the 4D-Var gradient on the GPU (fb_model_scatter, fb_model_observe, fb_model_obs_misfit,
fb_model_adjoint_add_obs; kernels csrc/fb_obs.h; Model.fourdvar and Model.fit_initial) against the float64 reference
(tests/obs_numpy.py) on the adjoint's path cases, whose grids take different branches of the record path and of the r2c that the
adjoint's forcing goes through.

The positions are obs_numpy.positions (grid points, stencils that wrap, negative and far positions, one position twice), the fields
tangent_inputs' never-dealiased noise.  The bars that are not fixed numbers are 4 x the float32 restatement's figure on the CPU
(obs_numpy.H_CASES, GRAD_F32; tests/test_obs_cpu.py asserts them), set before the GPU ran.  One line of figures per case (pytest -s);
DESIGN.md, "Point observations and the 4D-Var gradient", has the tables."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adjoint_numpy as A                                       # noqa: E402
import obs_numpy as O                                           # noqa: E402
import particles_numpy as P                                     # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

GRIDS = [(k.nx, k.ny) for k in O.H_CASES]
GRID_IDS = ["%dx%d" % g for g in GRIDS]
U23 = 2.0 ** -23
FB_EINVAL = 1


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    out = A.adjoint_inputs(nx, ny, 3e-2)
    for a in out:
        a.setflags(write=False)
    return out


def _model(nx, ny, vort=None, source=None, dt=None, nu=A.G.NU):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, nu=nu, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    if vort is not None:
        m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    return m


def _ref(nx, ny):
    return O.ObsModel64(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))


# ---- 1. the scatter ----
def _check_scatter(m, nx, ny, xy, w, what):
    got = _np(m.scatter(w, xy)).astype(np.float64)
    want, terms = O.scatter64(xy, w, nx, ny, terms=True)
    err = np.abs(got - want)
    worst = float((err / np.where(terms > 0, terms, 1.0)).max())
    esum = abs(got.sum() - np.sum(w[np.isfinite(w)])) / terms.sum()
    print("scatter %dx%d, %s, n = %d: worst cell error %.3g of the sum of its |contributions| (bar %.3g); the field's sum off by %.3g of all of them"
          % (nx, ny, what, len(w), worst, U23, esum))
    assert (err <= U23 * terms).all()                           # (a cell that nothing was added to must hold 0)
    assert esum <= U23
    return got


@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_scatter_against_float64(nx, ny):
    """per cell |got - np.add.at in float64| <= 2^-23 x the sum of the |contributions| to that cell; the field's sum against the sum of
    w to the same bound summed; two equal calls and a permutation of the points give the same bits; a NaN position (and a weight
    that is not finite) leaves the field as it is without that point; and a single point"""
    m = _model(nx, ny)
    xy, w = O.positions(nx, ny), O.weights(O.NPTS)
    got = _check_scatter(m, nx, ny, xy, w, "the edge-case positions")
    assert _same32(_np(m.scatter(w, xy)), got)
    perm = np.random.default_rng(11).permutation(O.NPTS)
    assert _same32(_np(m.scatter(w[perm], xy[perm])), got)
    xy2, w2 = xy.copy(), w.copy()
    xy2[7, 0], xy2[8, 1], w2[9] = np.nan, np.inf, np.nan
    keep = np.ones(O.NPTS, bool)
    keep[[7, 8, 9]] = False
    assert _same32(_np(m.scatter(w2, xy2)), _np(m.scatter(w[keep], xy[keep])))
    _check_scatter(m, nx, ny, xy[5:6], w[5:6], "one point")
    _check_scatter(m, nx, ny, xy, 1e-12 * w, "small weights")
    m.close()


def test_scatter_of_many_points_over_the_grid_cap():
    """n = 600001 at 64 x 192: more points than the capped grid has threads (the grid-stride loop), about 50 points per cell (every
    cell is added to some 800 times), weights over many orders of magnitude; the bound, equal bits for two calls and for a permutation"""
    nx, ny, n = 64, 192, 600001
    rng = np.random.default_rng(5)
    xy = (rng.random((n, 2)) * 3 - 1) * np.array([P.widen(O.LX), P.widen(O.LY)])
    w = rng.standard_normal(n) * np.exp(4 * rng.standard_normal(n))
    m = _model(nx, ny)
    got = _check_scatter(m, nx, ny, xy, w, "random")
    perm = rng.permutation(n)
    assert _same32(_np(m.scatter(w, xy)), got) and _same32(_np(m.scatter(w[perm], xy[perm])), got)
    m.close()


# ---- 2. the observation operator ----
@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_observe_is_sample_of_the_record_and_close_to_float64(nx, ny):
    """observe(kind, xy) equals sample(vort(), xy) and sample(diag()[k], xy) bit for bit, straight after set_vort and two steps on; it is
    within 1e-5 of the float64 reference of the same state, relative to max |h|"""
    v = _inputs(nx, ny)[0]
    xy = O.positions(nx, ny)
    m, ref = _model(nx, ny, v), _ref(nx, ny)
    ref.set_vort(v)
    for stepped in (False, True):
        if stepped:
            m.step(2)
        psi, u, vv = m.diag()
        fields = {"vort": m.vort(), "u": u, "v": vv, "psi": psi}
        for kind in O.KINDS:
            h = _np(m.observe(kind, xy))
            assert _same64(h, _np(m.sample(fields[kind], xy))), kind
            if not stepped:
                want = ref.observe(kind, xy)
                err = np.abs(h - want).max() / np.abs(want).max()
                print("observe %dx%d %s: max error %.3g of max |h|" % (nx, ny, kind, err))
                assert err <= 1e-5
    h = _np(m.observe("u", np.array([[np.nan, 1.0], [5.0, 7.0]])))
    assert np.isnan(h[0]) and np.isfinite(h[1])
    m.close()


# ---- 3. the identity ----
@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_dot_product_identity_of_h(nx, ny):
    """|<observe(kind, xy) of zeta, w> - <zeta, lam>| / (|H zeta| |w|) with lam what set_adjoint(0) then adjoint_add_obs(kind, xy, w)
    leave, for every kind: at most H_DOT_BAR, 4 x the largest figure of the float32 restatement on the CPU over these grids"""
    import torch
    v = _inputs(nx, ny)[0]
    xy, w = O.positions(nx, ny), O.weights(O.NPTS)
    m = _model(nx, ny, v)
    zero = torch.zeros((nx, ny), dtype=torch.float32, device="cuda")
    figs = {}
    for kind in O.KINDS:
        h = _np(m.observe(kind, xy))
        m.set_adjoint(zero)
        m.adjoint_add_obs(kind, xy, w)
        figs[kind] = O.dot_residual_h(h, w, v, _np(m.adjoint()))
    m.close()
    print("identity of H %dx%d on the GPU: %s; float32 on the CPU %.3g, bar %.3g"
          % (nx, ny, ", ".join("%s %.3g" % kv for kv in figs.items()), [k.f32 for k in O.H_CASES if (k.nx, k.ny) == (nx, ny)][0], O.H_DOT_BAR))
    assert max(figs.values()) <= O.H_DOT_BAR


def test_adjoint_add_obs_adds_to_what_is_there():
    """lam = lam_0 + H^T w: the increment over a non-zero lam equals, to float32 rounding of the sum, what it is over lam = 0"""
    import torch
    nx = ny = 256
    v, _, _, lam = _inputs(nx, ny)
    xy, w = O.positions(nx, ny), O.weights(O.NPTS) * 1e3
    m = _model(nx, ny, v)
    m.set_adjoint(torch.zeros((nx, ny), dtype=torch.float32, device="cuda"))
    m.adjoint_add_obs("u", xy, w)
    inc = _np(m.adjoint()).astype(np.float64)
    m.set_adjoint(lam)
    m.adjoint_add_obs("u", xy, w)
    got = _np(m.adjoint()).astype(np.float64)
    m.close()
    assert rel_l2(got - lam, inc) <= 1e-5 and np.linalg.norm(inc) > 1e-3 * np.linalg.norm(lam)


# ---- 4. the gradient ----
@functools.lru_cache(maxsize=None)
def _gradient_reference(nx, ny):
    ref = _ref(nx, ny)
    v, src, sets, d = O.gradient_case(nx, ny, ref)
    ref.src = src.astype(np.float64)
    J, g, res = O.fourdvar(ref, v, sets)
    return v, src, sets, d, J, g, res


def _observations(sets):
    import xlab_fftbarotropic_amd as X
    return [X.Observations(s.step, s.kind, s.xy, s.y, s.sigma) for s in sets]


@functools.lru_cache(maxsize=None)
def _gradient_gpu(nx, ny):
    v, src, sets, _, _, _, _ = _gradient_reference(nx, ny)
    m = _model(nx, ny, None, src)
    J, g = m.fourdvar(v, _observations(sets))
    assert m.adjoint_recorded() == 0
    m.close()
    return J, _np(g)


@pytest.mark.parametrize("nx,ny", O.GRAD_GRIDS)
def test_gradient_against_float64(nx, ny):
    """6 steps, sets of u and v at the steps 2, 4, 6 and one of zeta at step 0: grad within 1e-5 relative L2 of the float64 reference's,
    J within 1e-5 relative; two equal calls (one on a fresh model, one on a model that has just made the call) return the same bits"""
    v, src, sets, _, J64, g64, _ = _gradient_reference(nx, ny)
    J, g = _gradient_gpu(nx, ny)
    print("gradient %dx%d: grad rel L2 = %.3g, J rel = %.3g (J = %.6g)" % (nx, ny, rel_l2(g, g64), abs(J / J64 - 1), J))
    assert g.dtype == np.float64 and g.shape == (nx, ny)
    assert rel_l2(g, g64) <= 1e-5
    assert abs(J / J64 - 1) <= 1e-5
    m = _model(nx, ny, None, src)
    obs = _observations(sets)
    for _ in range(2):
        J2, g2 = m.fourdvar(v, obs)
        assert J2 == J and _same64(_np(g2), g)
    m.close()


def test_gradient_with_a_background_term():
    nx = ny = 256
    v, src, sets, _, _, _, _ = _gradient_reference(nx, ny)
    ref = _ref(nx, ny)
    ref.src = src.astype(np.float64)
    zb, sb = (0.9 * v).astype(np.float32), 1e-3
    J64, g64, _ = O.fourdvar(ref, v, sets, (zb, sb))
    m = _model(nx, ny, None, src)
    J, g = m.fourdvar(v, _observations(sets), (zb, sb))
    m.close()
    assert rel_l2(_np(g), g64) <= 1e-5 and abs(J / J64 - 1) <= 1e-5
    assert rel_l2(_np(g), _gradient_gpu(nx, ny)[1]) > 1e-3


# ---- 5. against the engine's own tangent ----
@pytest.mark.parametrize("nx,ny", O.GRAD_GRIDS)
def test_gradient_against_the_gpu_tangent(nx, ny):
    """<grad, d> = sum over the sets of <r, H T_k d> with T_k d from set_tangent / step, H applied to it by a second model that holds
    T_k d as its state (observe is linear in the state), r from obs_misfit on the same run; the residual over |(H T_k d)_k| |(r_k)_k| is
    at most GRAD_DOT_BAR, 4 x the float32 restatement's largest figure on the CPU"""
    import torch
    v, src, sets, d, _, _, _ = _gradient_reference(nx, ny)
    _, g = _gradient_gpu(nx, ny)
    m, lin = _model(nx, ny, v, src), _model(nx, ny)
    m.set_tangent(d)
    cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    at, tot, hs, rs = 0, 0.0, [], []
    for when in sorted(set(s.step for s in sets)):
        m.step(when - at)
        at = when
        lin.set_vort(m.tangent())
        for s in sets:
            if s.step == when:
                sig = None if s.sigma is None else np.broadcast_to(np.asarray(s.sigma, dtype=np.float64), (len(s.y),)).copy()
                r = _np(m.obs_misfit(m.observe(s.kind, s.xy), s.y, sig, cost))
                h = _np(lin.observe(s.kind, s.xy))
                tot += float(np.vdot(r, h))
                hs.append(h)
                rs.append(r)
    m.close()
    lin.close()
    res = abs(float(np.vdot(g, d.astype(np.float64))) - tot) / (np.linalg.norm(np.concatenate(hs)) * np.linalg.norm(np.concatenate(rs)))
    print("gradient against the GPU's tangent %dx%d: residual %.3g; float32 on the CPU %.3g, bar %.3g" % (nx, ny, res, O.GRAD_F32[(nx, ny)], O.GRAD_DOT_BAR))
    assert abs(float(cost.item()) / _gradient_gpu(nx, ny)[0] - 1) <= 1e-12
    assert res <= O.GRAD_DOT_BAR


# ---- 6. nothing else moves ----
@pytest.mark.parametrize("nx,ny", O.GRAD_GRIDS)
def test_the_vorticity_steps_on_as_if_fourdvar_had_not_been_called(nx, ny):
    """fourdvar leaves the model at step 6 of the run from z0; three steps on, the vorticity equals, bit for bit, that of a model that
    was set to z0 and stepped nine times and never made the call"""
    v, src, sets, _, _, _, _ = _gradient_reference(nx, ny)
    a, b = _model(nx, ny, None, src), _model(nx, ny, v, src)
    a.fourdvar(v, _observations(sets))
    a.step(3)
    b.step(O.GRAD_STEPS + 3)
    assert _same32(_np(a.vort()), _np(b.vort()))
    assert rel_l2(_np(b.vort()), v) > 1e-6
    a.close()
    b.close()


def test_observing_leaves_tracer_particles_and_tangent_bit_equal():
    import torch
    import xlab_fftbarotropic_amd as X
    n, steps = 256, 2
    v0, d0, src, lam = _inputs(n, n)
    c0 = T.noisy_inputs(n, n, 3e-2)[1]
    x0 = P.seed_positions(n, n, O.LX, O.LY, 64, seed=5)
    xy, w = O.positions(n, n), O.weights(O.NPTS)

    def run(observing):
        m = X.Model(n, n, nu=A.G.NU, dt=3.0)
        m.set_vort(v0)
        m.set_source(src)
        m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
        m.set_particles(x0)
        m.set_tangent(d0)
        m.step(steps)
        if observing:
            m.set_adjoint(lam)
            cost = torch.zeros(1, dtype=torch.float64, device="cuda")
            for kind in O.KINDS:
                m.adjoint_add_obs(kind, xy, m.obs_misfit(m.observe(kind, xy), w, None, cost))
            m.scatter(w, xy)
        m.step(steps)
        out = (_np(m.vort()), _np(m.tracer()), _np(m.particles()), _np(m.tangent()))
        m.close()
        return out
    a, b = run(False), run(True)
    assert _same32(a[0], b[0]) and _same32(a[1], b[1]) and _same32(a[3], b[3])
    assert _same64(a[2], b[2])


def test_slab_of_one_rank_returns_the_bits_of_the_model():
    import torch
    S = _slab()
    nx = ny = 256
    v, src, sets, _, _, _, _ = _gradient_reference(nx, ny)
    xy, w = O.positions(nx, ny), O.weights(O.NPTS)
    m = _model(nx, ny, v, src)
    s = S.EngineSlab(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))
    s.set_vort(v)
    s.set_source(src)
    zero = torch.zeros((nx, ny), dtype=torch.float32, device="cuda")
    assert _same32(_np(s.scatter(w, xy)), _np(m.scatter(w, xy)))
    for e in (m, s):
        e.set_adjoint(zero)
    for kind in O.KINDS:
        assert _same64(_np(s.observe(kind, xy)), _np(m.observe(kind, xy)))
        s.adjoint_add_obs(kind, xy, w)
        m.adjoint_add_obs(kind, xy, w)
    assert _same32(_np(s.adjoint()), _np(m.adjoint()))
    J, g = s.fourdvar(v, _observations(sets))
    Jm, gm = _gradient_gpu(nx, ny)
    assert J == Jm and _same64(_np(g), gm)
    s.close()
    m.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every new call raises with the engine's "several ranks" message"""
    import threading
    import torch
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n, world = 256, 2
    xy, w = O.positions(n, n), O.weights(O.NPTS)
    obs = [X.Observations(1, "u", xy, w)]
    cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    hub = S.local_hub(world)
    msgs, errs = [[] for _ in range(world)], [None] * world

    def work(r):
        try:
            s = S.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                z = np.zeros((s.XL, n), np.float32)
                calls = (lambda: s.scatter(w, xy), lambda: s.observe("vort", xy), lambda: s.obs_misfit(w, w, None, cost),
                         lambda: s.adjoint_add_obs("psi", xy, w), lambda: s.fourdvar(z, obs), lambda: s.fit_initial(z, obs, 1))
                for call in calls:
                    try:
                        call()
                        msgs[r].append(None)
                    except X.FftBaroError as e:
                        msgs[r].append(str(e))
            finally:
                s.close()
        except BaseException as e:                                          # noqa: BLE001 -- re-raised below
            errs[r] = e
    try:
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        S.local_hub_destroy(hub)
    for e in errs:
        if e is not None:
            raise e
    for r in range(world):
        assert len(msgs[r]) == 6
        for msg in msgs[r]:
            assert msg is not None and "invalid argument" in msg.lower() and "several ranks" in msg, msg


def test_bad_arguments_are_refused_under_the_function_s_own_name_before_anything_is_launched():
    """on a live model: n = 0, n = 2^24 + 1, kind 4, a NULL pointer, and adjoint_add_obs before set_adjoint; the field, the outputs and lam
    are untouched"""
    import torch
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    nx = ny = 256
    m = _model(nx, ny, _inputs(nx, ny)[0])
    buf = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    fld = torch.full((nx, ny), 7.0, dtype=torch.float32, device="cuda")
    p, f, big = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(fld.data_ptr()), (1 << 24) + 1
    cases = [("scatter", (p, p, 0, f), "n outside"), ("scatter", (p, p, big, f), "n outside"), ("scatter", (p, p, 4, None), "NULL"),
             ("observe", (4, p, 4, p), "kind"), ("observe", (0, p, 0, p), "n outside"), ("observe", (0, None, 4, p), "NULL"),
             ("obs_misfit", (p, p, None, big, p, p), "n outside"), ("obs_misfit", (p, p, None, 4, p, None), "NULL"),
             ("adjoint_add_obs", (4, p, p, 4), "kind"), ("adjoint_add_obs", (0, p, p, 0), "n outside"), ("adjoint_add_obs", (0, p, None, 4), "NULL"),
             ("adjoint_add_obs", (0, p, p, 4), "no adjoint is set")]
    for stem, args, phrase in cases:
        name = "fb_model_" + stem
        assert getattr(L, name)(m._h, *args) == FB_EINVAL, (name, args)
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and phrase in msg, (name, args, msg)
    with pytest.raises(X.FftBaroError, match="fb_model_adjoint_add_obs: no adjoint is set"):
        m.adjoint_add_obs("u", np.zeros((4, 2)), np.zeros(4))
    with pytest.raises(ValueError, match="sigma"):
        m.obs_misfit(np.zeros(4), np.zeros(4), np.array([1.0, 0.0, 1.0, 1.0]), torch.zeros(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="sigma"):
        X.Observations(0, "u", np.zeros((4, 2)), np.zeros(4), np.array([1.0, np.inf, 1.0, 1.0]))
    with pytest.raises(ValueError, match="kind"):
        m.observe("zeta", np.zeros((4, 2)))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((fld == 7.0).all())
    m.close()


# ---- 7. the twin experiment ----
def test_twin_experiment():
    """64^2, dt = 30 s: the truth is make_field("kuo2004") (two vortices), whose vorticity changes by 37.6 % in relative L2 over the
    window of 8 steps (float64: obs_numpy.TWIN_CHANGE, asserted >= 10 % in tests/test_obs_cpu.py), so the gradient depends on the
    dynamics; the observations are the truth's u and v (float64 reference) at 256 fixed random points at the steps 2, 4, 6, 8,
    sigma = 1; the first guess is the truth scaled by 0.8 and shifted by two cells.  fit_initial with K = 10: J falls at every
    accepted iteration, J_K / J_0 <= 10 x the float64 reference's 0.01457 (obs_numpy.TWIN_RATIO), and z0 ends closer to the truth"""
    import xlab_fftbarotropic_amd as X
    truth, guess, sets, change = O.twin_case(X.make_field)
    assert change >= 0.1
    m = _model(O.TWIN_N, O.TWIN_N, dt=O.TWIN_DT, nu=O.TWIN_NU)
    z, hist, evals = m.fit_initial(guess, _observations(sets), O.TWIN_ITERS)
    m.close()
    e0, e1 = rel_l2(guess, truth), rel_l2(_np(z), truth)
    print("twin experiment on the GPU: J = %s; J_K / J_0 = %.4g (float64: %.4g, bar %.4g); %d evaluations; z0 off by %.4g at the start, %.4g at the end"
          % (["%.4g" % j for j in hist], hist[-1] / hist[0], O.TWIN_RATIO, 10 * O.TWIN_RATIO, evals, e0, e1))
    assert len(hist) >= 2 and all(b < a for a, b in zip(hist, hist[1:]))
    assert hist[-1] / hist[0] <= 10 * O.TWIN_RATIO
    assert e1 < e0
