"""Lagrangian (drifter) observations on the GPU: the particle tape, the particle adjoint and the sweep of the coupled step
(fb_model_particle_tape, fb_model_set_particle_adjoint, fb_model_get_particle_adjoint, what fb_model_adjoint_back runs while a particle
adjoint is set; kernels csrc/fb_lagrangian.h; Model.fourdvar and Model.fit_initial with particles) against the float64 reference
(tests/lagrangian_numpy.py) on the adjoint's path cases, whose grids take the three branches of stage_vstate and the row and column
dispatch.

The drifters start at obs_numpy.positions (grid points, stencils that wrap, negative and far positions, one position twice), the
vorticity is adjoint_inputs' never-dealiased noise, 5 steps.  The bar of lam_0 is the adjoint's own 1e-5; the bar of Xb_0 is 4 x the
float32 restatement's largest figure on the CPU (lagrangian_numpy.L_CASES; tests/test_lagrangian_cpu.py asserts them), set before the
GPU ran.  One line of figures per case (pytest -s); DESIGN.md, "Lagrangian observations", has the tables."""
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
import lagrangian_numpy as L                                    # noqa: E402
import obs_numpy as O                                           # noqa: E402
import particles_numpy as P                                     # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

GRIDS = [(k.nx, k.ny) for k in L.L_CASES]
GRID_IDS = ["%dx%d" % g for g in GRIDS]
FB_EINVAL, FB_EUNSUPPORTED = 1, 5


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


def _model(nx, ny, vort=None, source=None, dt=None, nu=A.G.NU, cls=None):
    import xlab_fftbarotropic_amd as X
    m = (cls or X.Model)(nx, ny, nu=nu, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    if vort is not None:
        m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    return m


@functools.lru_cache(maxsize=None)
def _reference(nx, ny):
    """the float64 sweep of the path case with lam(T) = 0: (lam_0, Xb_0, X(T))"""
    ref = L.sweep_case(nx, ny)
    return ref.adjoint(), ref.particle_adjoint(), ref.particles()


@functools.lru_cache(maxsize=None)
def _reference_field_only(nx, ny):
    """lam_0 in float64 of lam(T) = adjoint_inputs' white noise with no drifters: the field's own part of a sweep, which is linear"""
    v, dz, src, lam = _inputs(nx, ny)
    return A.run_case(nx, ny, v, dz, src, lam, L.STEPS).adjoint()


def _sweep(nx, ny, lam_T=None, xy=None, steps=L.STEPS, parts=None, record=None, deformation=False, cls=None, xb=None):
    """the sweep of lagrangian_numpy.sweep_case on the engine: (lam_0 float32, Xb_0, X(T), F or None)"""
    import torch
    v, _, src, _ = _inputs(nx, ny)
    xy = O.positions(nx, ny) if xy is None else xy
    m = _model(nx, ny, v, src, cls=cls)
    m.set_particles(xy)
    if deformation:
        m.set_particle_deformation()
    (record or (lambda e: e.record_adjoint(steps)))(m)
    m.record_particles(steps)
    m.step(steps)
    assert m.particles_recorded() == (steps, steps)
    F = _np(m.particle_deformation()) if deformation else None
    x = _np(m.particles())
    m.set_adjoint(torch.zeros((nx, ny), dtype=torch.float32, device="cuda") if lam_T is None else lam_T)
    m.set_particle_adjoint(L.xbar_T(xy.shape[0]) if xb is None else xb)
    for k in parts or (steps,):
        m.adjoint_back(k)
    assert m.particles_recorded() == (0, steps) and m.adjoint_recorded() == 0
    out = _np(m.adjoint()), _np(m.particle_adjoint()), x, F
    m.close()
    return out


@functools.lru_cache(maxsize=None)
def _sweep_256(noise):
    return _sweep(256, 256, lam_T=_inputs(256, 256)[3] if noise else None)


# ---- 1. the sweep against float64 ----
@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_sweep_against_float64(nx, ny):
    """lam(T) = 0 and Xb(T) = white noise, so that all of lam_0 comes through the drifters: lam_0 within 1e-5 relative L2 of float64,
    Xb_0 within XBAR_BAR of max |Xb_0|, and Xb_0 = F^T Xb(T) with the engine's own F (float64 arithmetic on the same float32 u, v on
    both sides) to 1e-12 of max |F^T Xb(T)|; then lam(T) = white noise and Xb(T) scaled so that the drifters' part of lam_0 is as
    large as the field's own: lam_0 to 1e-5 again, against the sum of the two float64 parts (the sweep is linear)"""
    lam64, xb64, x64 = _reference(nx, ny)
    lam, xb, x, F = _sweep(nx, ny, deformation=True)
    e_lam, e_xb = rel_l2(lam, lam64), L.xbar_error(xb, xb64)
    want = np.einsum("nij,ni->nj", F, L.xbar_T(L.NPTS))
    e_f = L.xbar_error(xb, want)
    cells = np.array([P.widen(L.LX) / nx, P.widen(L.LY) / ny])
    moved = float(np.abs((x - O.positions(nx, ny)) / cells).max())
    case = L.lcase_of(nx, ny)
    print("sweep %dx%d, lam(T) = 0: lam_0 rel L2 %.3g (float32 on the CPU %.3g, bar %.3g); Xb_0 %.3g (CPU %.3g, bar %.3g); Xb_0 against F^T Xb(T) "
          "%.3g (bar 1e-12); the drifters moved up to %.3g cells" % (nx, ny, e_lam, case.lam, L.LAM_BAR, e_xb, case.xbar, L.XBAR_BAR, e_f, moved))
    assert np.linalg.norm(lam64) > 0 and abs(moved / case.moved - 1) <= 0.01
    assert np.abs((x - x64) / cells).max() <= 1e-4
    assert e_lam <= L.LAM_BAR
    assert e_xb <= L.XBAR_BAR
    assert e_f <= 1e-12
    own = _reference_field_only(nx, ny)
    scale = float(np.linalg.norm(own) / np.linalg.norm(lam64))
    lam64n = own + scale * lam64
    lam_n, xb_n, _, _ = _sweep(nx, ny, lam_T=_inputs(nx, ny)[3], xb=scale * L.xbar_T(L.NPTS))
    print("sweep %dx%d, lam(T) = noise, Xb(T) times %.3g: lam_0 rel L2 %.3g, Xb_0 %.3g; the drifters' part is %.3g of lam_0, the field's %.3g"
          % (nx, ny, scale, rel_l2(lam_n, lam64n), L.xbar_error(xb_n, scale * xb64), scale * np.linalg.norm(lam64) / np.linalg.norm(lam64n),
             np.linalg.norm(own) / np.linalg.norm(lam64n)))
    assert rel_l2(lam_n, lam64n) <= L.LAM_BAR
    assert L.xbar_error(xb_n, scale * xb64) <= L.XBAR_BAR


def test_the_drifters_cross_cell_faces():
    assert max(k.moved for k in L.L_CASES) > 1.0                # (each case's figure is asserted against the engine's positions above)


# ---- 2. fourdvar with position sets ----
@functools.lru_cache(maxsize=None)
def _position_reference(nx, ny, mixed):
    ref = L.ref_model(nx, ny)
    v, src, xy0, sets = L.position_case(nx, ny, ref, mixed)
    ref.src = src.astype(np.float64)
    J, g, xb0 = L.fourdvar(ref, v, sets, None, xy0)
    return v, src, xy0, sets, J, g, xb0


def _observations(sets):
    import xlab_fftbarotropic_amd as X
    return [X.Observations(s.step, s.kind, s.xy, s.y, s.sigma) for s in sets]


@pytest.mark.parametrize("mixed", [False, True], ids=["positions", "mixed"])
@pytest.mark.parametrize("nx,ny", L.GRAD_GRIDS)
def test_fourdvar_with_position_sets(nx, ny, mixed):
    """position sets at the steps 3 and 6 (mixed: with u and v sets at 2, 4, 6): J and grad within 1e-5 of the float64 reference, dJ/dX_0
    in particle_adjoint() within FOURDVAR_XBAR_BAR; two equal calls return the same bits of all three, and both tapes are freed.
    The bar of dJ/dX_0 is not the sweep's XBAR_BAR: here Xb(T) is the residual of the run's own float32 positions, whose error over
    the misfit enters before the sweep (lagrangian_numpy.F_CASES: the float32 restatement on the CPU is off by 1.4e-6, and the
    engine measured 1.6e-6 against the sweep's bar of 7.4e-7 before this bar was set from that table by the same rule)"""
    v, src, xy0, sets, J64, g64, xb64 = _position_reference(nx, ny, mixed)
    m = _model(nx, ny, None, src)
    obs = _observations(sets)
    J, g = m.fourdvar(v, obs, particles=xy0)
    g, xb = _np(g), _np(m.particle_adjoint())
    print("fourdvar %dx%d, %s: grad rel L2 %.3g, J rel %.3g (J = %.6g), dJ/dX_0 %.3g (bar %.3g)"
          % (nx, ny, "mixed" if mixed else "positions", rel_l2(g, g64), abs(J / J64 - 1), J, L.xbar_error(xb, xb64), L.FOURDVAR_XBAR_BAR))
    assert m.adjoint_recorded() == 0 and m.particles_recorded() == (0, 0)
    assert g.dtype == np.float64 and g.shape == (nx, ny) and xb.shape == (L.NPTS, 2)
    assert rel_l2(g, g64) <= 1e-5 and abs(J / J64 - 1) <= 1e-5
    assert L.xbar_error(xb, xb64) <= L.FOURDVAR_XBAR_BAR
    J2, g2 = m.fourdvar(v, obs, particles=xy0)
    assert J2 == J and _same64(_np(g2), g) and _same64(_np(m.particle_adjoint()), xb)
    m.close()


def test_fourdvar_without_particles_returns_what_it_always_has():
    """obs_numpy.gradient_case through the unchanged path: with particles=None, and with drifters that carry no data, J and grad are the
    bits of a walk through observe, obs_misfit, adjoint_add_obs and adjoint_back by hand"""
    import torch
    nx = ny = 256
    ref = O.ObsModel64(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))
    v, src, sets, _ = O.gradient_case(nx, ny, ref)
    obs = _observations(sets)
    m = _model(nx, ny, None, src)
    J, g = m.fourdvar(v, obs)
    Jp, gp = m.fourdvar(v, obs, particles=O.positions(nx, ny))
    assert Jp == J and _same64(_np(gp), _np(g))
    m.set_particles(None)
    m.set_vort(v)
    m.record_adjoint(O.GRAD_STEPS)
    cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    times, res, at = sorted(set(o.step for o in obs)), {}, 0
    for when in times:
        m.step(when - at)
        at = when
        for k, o in enumerate(obs):
            if o.step == when:
                res[k] = m.obs_misfit(m.observe(o.kind, o.xy), o.y, o.sigma, cost)
    m.set_adjoint(torch.zeros((nx, ny), dtype=torch.float32, device="cuda"))
    for when, before in zip(times[::-1], times[-2::-1] + [0]):
        for k, o in enumerate(obs):
            if o.step == when:
                m.adjoint_add_obs(o.kind, o.xy, res[k])
        m.adjoint_back(when - before)
    assert float(cost.item()) == J and _same64(_np(m.adjoint().double()), _np(g))
    m.close()


# ---- 3. bit for bit ----
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_the_particle_tape_changes_no_bit_of_what_is_stepped(graph):
    """vorticity, positions, F, tracer and tangent after 6 steps with the particle tape on and off (with use_graph the run without the
    tape replays the captured step, the run with it steps eagerly)"""
    import torch
    import xlab_fftbarotropic_amd as X
    n, steps = 256, 6
    v0, d0, src, _ = _inputs(n, n)
    c0 = T.noisy_inputs(n, n, 3e-2)[1]
    xy = O.positions(n, n)

    def run(tape):
        with torch.cuda.stream(torch.cuda.Stream()):            # (a captured step needs a stream of its own)
            return run_on_stream(tape)

    def run_on_stream(tape):
        m = X.Model(n, n, nu=A.G.NU, dt=T.recipe_dt(n, n))
        m.fop.use_current_stream()
        m.use_graph(graph)
        m.set_vort(v0)
        m.set_source(src)
        m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
        m.set_particles(xy)
        m.set_particle_deformation()
        m.set_tangent(d0)
        if tape:
            m.record_particles(steps)
        m.step(2)
        m.step(4)
        assert m.particles_recorded() == ((steps, steps) if tape else (0, 0))
        out = (_np(m.vort()), _np(m.tracer()), _np(m.tangent()), _np(m.particles()), _np(m.particle_deformation()))
        if tape:
            with pytest.raises(X.FftBaroError, match="fb_model_step: the particle tape has room for 0 more steps"):
                m.step(1)
            m.record_particles(0)
            m.step(1)
        m.close()
        return out
    a, b = run(False), run(True)
    assert all(_same32(p, q) for p, q in zip(a[:3], b[:3])) and _same64(a[3], b[3]) and _same64(a[4], b[4])
    assert rel_l2(a[0], v0) > 1e-6


def test_sweeps_are_reproducible_and_independent_of_the_order_of_the_drifters():
    """two equal runs give the same bits of lam_0 and Xb_0; the drifters permuted give the same lam_0 and Xb_0 permuted; 3 + 2 steps
    equal 5; checkpoint_adjoint(2, 5) gives the bits of record_adjoint(5); an EngineSlab of one rank equals the Model; and without
    a particle adjoint lam_0 is the same bits with the particle tape on and off"""
    import torch
    nx = ny = 256
    lamT = _inputs(nx, ny)[3]
    lam, xb, x, _ = _sweep_256(True)
    again = _sweep(nx, ny, lam_T=lamT)
    assert _same32(again[0], lam) and _same64(again[1], xb) and _same64(again[2], x)
    perm = np.random.default_rng(11).permutation(L.NPTS)
    pl, pxb, _, _ = _sweep(nx, ny, lam_T=lamT, xy=O.positions(nx, ny)[perm], xb=L.xbar_T(L.NPTS)[perm])
    assert _same32(pl, lam) and _same64(pxb, xb[perm])
    parts = _sweep(nx, ny, lam_T=lamT, parts=(3, 2))
    assert _same32(parts[0], lam) and _same64(parts[1], xb)
    for pieces in ((5,), (1, 3, 1)):
        ck = _sweep(nx, ny, lam_T=lamT, record=lambda e: e.checkpoint_adjoint(2, 5), parts=pieces)
        assert _same32(ck[0], lam) and _same64(ck[1], xb) and _same64(ck[2], x), pieces
    sl = _sweep(nx, ny, lam_T=lamT, cls=_slab().EngineSlab)
    assert _same32(sl[0], lam) and _same64(sl[1], xb) and _same64(sl[2], x)
    assert not _same32(lam, _sweep_256(False)[0]) and _same64(xb, _sweep_256(False)[1])     # Xb never depends on lam
    assert _same64(_sweep(nx, ny, deformation=True)[1], xb)                                  # nor on whether F is carried
    # no particle adjoint: the sweep is the one it has always been
    v, _, src, _ = _inputs(nx, ny)
    outs = []
    for tape in (False, True):
        m = _model(nx, ny, v, src)
        m.set_particles(O.positions(nx, ny))
        m.record_adjoint(L.STEPS)
        if tape:
            m.record_particles(L.STEPS)
        m.step(L.STEPS)
        m.set_adjoint(lamT)
        m.adjoint_back(L.STEPS)
        outs.append(_np(m.adjoint()))
        assert m.particles_recorded() == ((L.STEPS, L.STEPS) if tape else (0, 0))     # a sweep without a particle adjoint pops nothing
        m.close()
    assert _same32(outs[0], outs[1]) and not _same32(outs[0], lam)
    m = _model(nx, ny, v, src)                                  # ... and the one of a model that has no particles at all
    m.record_adjoint(L.STEPS)
    m.step(L.STEPS)
    m.set_adjoint(torch.from_numpy(np.array(lamT)).cuda())
    m.adjoint_back(L.STEPS)
    assert _same32(_np(m.adjoint()), outs[0])
    m.close()


def test_many_drifters_on_a_small_grid():
    """n = 600001 over three domain lengths at 64 x 192, one step: more drifters than the capped grid has threads, some 800 deposits
    per cell and stage; lam_0 within 1e-5 of float64, Xb_0 within XBAR_BAR, and equal bits for two runs"""
    nx, ny, n, steps = 64, 192, 600001, 1
    xy = (np.random.default_rng(5).random((n, 2)) * 3 - 1) * np.array([P.widen(L.LX), P.widen(L.LY)])
    ref = L.sweep_case(nx, ny, xy=xy, steps=steps)
    lam, xb, x, _ = _sweep(nx, ny, xy=xy, steps=steps)
    print("many drifters, %dx%d, n = %d: lam_0 rel L2 %.3g, Xb_0 %.3g" % (nx, ny, n, rel_l2(lam, ref.adjoint()), L.xbar_error(xb, ref.particle_adjoint())))
    assert rel_l2(lam, ref.adjoint()) <= L.LAM_BAR
    assert L.xbar_error(xb, ref.particle_adjoint()) <= L.XBAR_BAR
    again = _sweep(nx, ny, xy=xy, steps=steps)
    assert _same32(again[0], lam) and _same64(again[1], xb)


def test_a_drifter_with_a_nan_position():
    """its Xb_0 is NaN; every other drifter's Xb_0 and lam_0 are the bits of the run without it (whose Xb(T) for the others is the same)"""
    nx = ny = 256
    xy, xbT = O.positions(nx, ny), L.xbar_T(L.NPTS)
    bad = xy.copy()
    bad[11, 0] = np.nan
    keep = np.arange(L.NPTS) != 11
    lam_b, xb_b, x_b, _ = _sweep(nx, ny, xy=bad)
    lam_k, xb_k, _, _ = _sweep(nx, ny, xy=xy[keep], xb=xbT[keep])
    assert np.isnan(xb_b[11]).all() and np.isnan(x_b[11]).all()
    assert np.isfinite(lam_b).all() and _same32(lam_b, lam_k) and _same64(xb_b[keep], xb_k)
    # a particle adjoint that is not finite poisons that drifter alone too
    xbad = xbT.copy()
    xbad[11, 1] = np.inf
    lam_i, xb_i, _, _ = _sweep(nx, ny, xb=xbad)
    assert not np.isfinite(xb_i[11]).any() and np.isfinite(lam_i).all() and _same32(lam_i, lam_k) and _same64(xb_i[keep], xb_k)


# ---- 4. refusals ----
def test_life_cycle_and_refusals():
    import torch
    import xlab_fftbarotropic_amd as X
    n = 64
    m = X.Model(n, n)
    m.set_vort(X.make_field("kuo2004", n))
    lib = X.lib()
    buf = torch.full((8, 2), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = ctypes.c_void_p(buf.data_ptr())

    def refused(name, args, phrase, code=FB_EINVAL):
        fn = "fb_model_" + name
        assert getattr(lib, fn)(m._h, *args) == code, fn
        msg = lib.fb_last_error().decode()
        assert msg.startswith(fn + ": ") and phrase in msg, msg
    # before particles are set
    refused("particle_tape", (3,), "no particles are set")
    refused("set_particle_adjoint", (ptr,), "no particles are set")
    refused("set_particle_adjoint", (None,), "no particles are set")
    refused("get_particle_adjoint", (ptr,), "no particles are set")
    refused("get_particle_adjoint", (None,), "NULL output")
    refused("particle_tape", (-1,), "depth outside")
    assert lib.fb_model_particle_tape(m._h, 0) == 0 and m.particles_recorded() == (0, 0)
    x0 = np.array([[1.0e5, 2.0e5], [3.0e5, 4.0e5], [5.0e5, 1.0e5]])
    m.set_particles(x0)
    hbm0 = m.info()["hbm_bytes"]
    refused("get_particle_adjoint", (ptr,), "no particle adjoint is set")
    m.record_particles(4)
    assert m.info()["hbm_bytes"] == hbm0 + 4 * 4 * 3 * 16 and m.particles_recorded() == (0, 4)
    m.record_adjoint(5)
    m.step(3)
    refused("step", (2,), "the particle tape has room for 1 more steps")
    assert m.particles_recorded() == (3, 4)
    m.set_adjoint(torch.zeros((n, n), dtype=torch.float32, device="cuda"))
    hbm1 = m.info()["hbm_bytes"]
    m.set_particle_adjoint(np.ones((3, 2)))
    assert m.info()["hbm_bytes"] == hbm1 + 8 * 3 * 8 + (4 * n * n + 2) * 8
    with pytest.raises(ValueError, match="one row per particle"):
        m.set_particle_adjoint(np.ones((4, 2)))
    refused("adjoint_back", (4,), "4 steps asked for, 3 recorded")
    m.adjoint_back(1)
    assert m.particles_recorded() == (2, 4) and m.adjoint_recorded() == 2
    # the tapes out of step: a sweep without the particle adjoint pops the field's tape alone
    m.set_particle_adjoint(None)
    m.adjoint_back(1)
    m.set_particle_adjoint(np.ones((3, 2)))
    refused("adjoint_back", (1,), "the particle tape holds 2 steps, the adjoint's window 1")
    # a new state empties both tapes; a particle tape shorter than the sweep
    m.set_vort(X.make_field("kuo2004", n))
    assert m.particles_recorded() == (0, 4) and m.adjoint_recorded() == 0
    m.record_particles(0)
    m.step(2)
    m.record_particles(4)
    m.step(1)
    refused("adjoint_back", (2,), "2 steps asked for, 1 on the particle tape")
    # a set of several adjoint variables
    m.set_adjoints(np.zeros((2, n, n), dtype=np.float32))
    refused("adjoint_back", (1,), "a particle adjoint is set beside a set of 2 adjoint variables")
    m.set_adjoint(torch.zeros((n, n), dtype=torch.float32, device="cuda"))
    # new particles empty the tape and remove the particle adjoint; another count frees the tape
    m.set_particles(x0)
    assert m.particles_recorded() == (0, 4)
    refused("get_particle_adjoint", (ptr,), "no particle adjoint is set")
    m.set_particles(x0[:2])
    assert m.particles_recorded() == (0, 0)
    m.set_particles(None)
    refused("particle_tape", (1,), "no particles are set")
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    m.step(1)
    m.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every new entry point raises the particles' unsupported error under its own name"""
    import threading
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n, world = 256, 2
    hub = S.local_hub(world)
    msgs, errs = [[] for _ in range(world)], [None] * world

    def work(r):
        try:
            s = S.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                calls = (("particle_tape", lambda: s.record_particles(3)), ("particle_tape", lambda: s.record_particles(0)),
                         ("particle_tape_count", lambda: s.particles_recorded()), ("set_particle_adjoint", lambda: s.set_particle_adjoint(np.zeros((4, 2)))),
                         ("set_particle_adjoint", lambda: s.set_particle_adjoint(None)), ("get_particle_adjoint", lambda: s.particle_adjoint()))
                for name, call in calls:
                    try:
                        call()
                        msgs[r].append((name, None))
                    except X.FftBaroError as e:
                        msgs[r].append((name, str(e)))
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
        for name, msg in msgs[r]:
            assert msg is not None and "fb_slab_" + name + ": particles are not supported" in msg and "world > 1" in msg, (name, msg)


# ---- 5. the twin experiment ----
def test_twin_experiment():
    """64^2, dt = 30 s, obs_numpy.twin_case's truth and first guess; the only data are the positions of 256 drifters at the steps 2, 4,
    6, 8 (float64 reference), sigma a tenth of their largest displacement.  fit_initial with K = 10: J falls at every accepted
    iteration, J_K / J_0 <= 10 x the float64 reference's 0.02973 (lagrangian_numpy.TWIN_RATIO), and z0 ends closer to the truth"""
    import xlab_fftbarotropic_amd as X
    truth, guess, xy0, sets, sigma = L.twin_case(X.make_field)
    m = _model(O.TWIN_N, O.TWIN_N, dt=O.TWIN_DT, nu=O.TWIN_NU)
    z, hist, evals = m.fit_initial(guess, _observations(sets), L.TWIN_ITERS, particles=xy0)
    assert m.particles_recorded() == (0, 0) and m.adjoint_recorded() == 0
    m.close()
    e0, e1 = rel_l2(guess, truth), rel_l2(_np(z), truth)
    print("twin experiment with drifters on the GPU: J = %s; J_K / J_0 = %.4g (float64: %.4g, bar %.4g); %d evaluations; z0 off by %.4g at the start, "
          "%.4g at the end" % (["%.4g" % j for j in hist], hist[-1] / hist[0], L.TWIN_RATIO, 10 * L.TWIN_RATIO, evals, e0, e1))
    assert len(hist) >= 2 and all(b < a for a, b in zip(hist, hist[1:]))
    assert hist[-1] / hist[0] <= 10 * L.TWIN_RATIO
    assert e1 < e0
