"""CPU tests of the float64 reference of the Lagrangian particles (tests/particles_numpy.py): the interpolation that
fb_model_sample is tested against, the coupled RK4 of ParticleModel64, and the conditions on the particles' path matrix
(particles_numpy.PATH_CASES, tests/test_gpu_particle_paths.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import particles_numpy as P  # noqa: E402
from tracer_numpy import cellular_flow  # noqa: E402


def test_bicubic_patch_is_reproduced():
    """a polynomial of degree 3 in x and in y is reproduced to rounding wherever the stencil does not wrap"""
    nx, ny, lx, ly = 64, 96, 64.0, 48.0
    x = np.arange(nx)[:, None] * (lx / nx)
    y = np.arange(ny)[None, :] * (ly / ny)

    def poly(x, y):
        return (1.0 + 0.5 * x - 0.02 * x ** 2 + 3e-4 * x ** 3) * (2.0 - 0.3 * y + 0.01 * y ** 2 - 2e-4 * y ** 3)
    f = poly(x, y)
    rng = np.random.default_rng(1)
    xy = np.stack([rng.uniform(1.0, nx - 3.0, 500) * (lx / nx), rng.uniform(1.0, ny - 3.0, 500) * (ly / ny)], axis=1)
    got = P.lagrange4_sample(f, xy, lx, ly)
    want = poly(xy[:, 0], xy[:, 1])
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(f))


def test_wraps_in_both_axes_and_far_away():
    """first and last cell of both axes against the same interpolation on a 3 x 3 tiling of the field, where no stencil wraps (an
    independent check of the modulus); positions 3 domain lengths away, on either side, give what the folded position gives.  dx = dy = 1
    and positions on a binary grid, so that every division is exact and the comparison is bitwise."""
    nx, ny = 64, 128
    lx, ly = float(nx), float(ny)
    rng = np.random.default_rng(2)
    f = rng.standard_normal((nx, ny)).astype(np.float32)
    q = lambda a: np.round(a * 1024.0) / 1024.0
    edge = np.array([[0.25, 17.5], [63.75, 40.125], [31.5, 0.5], [12.25, 127.625], [63.5, 127.5], [0.125, 0.875], [63.875, 0.25], [0.5, 127.25]])
    xy = np.concatenate([edge, q(rng.random((200, 2)) * np.array([lx, ly]))])
    got = P.lagrange4_sample(f, xy, lx, ly)
    tiled = np.tile(f, (3, 3))
    want = P.lagrange4_sample(tiled, xy + np.array([lx, ly]), 3 * lx, 3 * ly)
    assert np.array_equal(got, want)
    for sx, sy in ((3, 0), (-3, 0), (0, 3), (0, -3), (3, -3), (-3, 3)):
        far = P.lagrange4_sample(f, xy + np.array([sx * lx, sy * ly]), lx, ly)
        assert np.array_equal(far, got), (sx, sy)
    # a domain whose spacing is no binary fraction: far positions agree to the rounding of the shifted position
    lx2, ly2 = 600000.0, 600000.0
    xy2 = rng.random((200, 2)) * np.array([lx2, ly2])
    near = P.lagrange4_sample(f, xy2, lx2, ly2)
    for s in (3, -3):
        far = P.lagrange4_sample(f, xy2 + s * np.array([lx2, ly2]), lx2, ly2)
        assert np.max(np.abs(far - near)) <= 1e-10 * np.max(np.abs(f))


def test_grid_points_get_the_grid_value():
    for nx, ny, lx, ly in ((64, 64, 600000.0, 600000.0), (192, 64, 600000.0, 300000.0), (64, 192, 2 * np.pi, 2 * np.pi)):
        rng = np.random.default_rng(3)
        f = rng.standard_normal((nx, ny)).astype(np.float32)
        g = P.grid_points(nx, ny, lx, ly, 64)
        assert g.shape[0] >= 32
        dx, dy = P.widen(lx) / nx, P.widen(ly) / ny
        i, j = np.mod((g[:, 0] / dx).astype(np.int64), nx), np.mod((g[:, 1] / dy).astype(np.int64), ny)
        assert np.array_equal(P.lagrange4_sample(f, g, lx, ly), f[i, j].astype(np.float64))


def test_fourth_order_convergence():
    """the error on one Fourier mode falls by about 16 per halving of dx"""
    lx = ly = 2 * np.pi
    rng = np.random.default_rng(4)
    xy = rng.random((2000, 2)) * lx
    errs = []
    for n in (32, 64, 128, 256):
        x = np.arange(n)[:, None] * (P.widen(lx) / n)
        y = np.arange(n)[None, :] * (P.widen(ly) / n)
        f = np.sin(3 * x) * np.cos(2 * y)
        errs.append(np.max(np.abs(P.lagrange4_sample(f, xy, lx, ly) - np.sin(3 * xy[:, 0]) * np.cos(2 * xy[:, 1]))))
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("lagrange4 errors", errs, "ratios", ratios)
    assert all(12.0 <= r <= 20.0 for r in ratios), ratios


def test_cellular_flow_keeps_psi_at_the_particle():
    """ParticleModel64 on the steady cellular flow with nu = 0: psi at a particle is constant along the exact trajectory, because the
    velocity is perpendicular to grad psi.  The computed one drifts by grad psi . dU with dU the error of the interpolated velocity:
        |psi(T) - psi(0)| <= max|grad psi| * max|dU| * T.
    max|dU| is MEASURED here (cubic Lagrange interpolation of the model's own u, v against the analytic velocity at 4000 random
    points; theory: 9/384 (k dx)^4 per axis and unit amplitude), max|grad psi| = A sqrt(kx^2 + ky^2) analytically.  A factor 2 covers
    the sampling of the maximum; the RK4 truncation error per step, (|u| K dt)^5 / 120 of a displacement, is ten orders below."""
    nx = ny = 64
    lx = ly = 600000.0
    amp, mx, my, dt, steps = 1.0e6, 2, 3, 3.0, 50
    psi, zeta, k2 = cellular_flow(nx, ny, lx, ly, amp, mx, my)
    m = P.ParticleModel64(nx, ny, lx, ly, nu=0.0, dt=dt)
    m.set_vort(zeta)
    rng = np.random.default_rng(5)
    probe = rng.random((4000, 2)) * lx
    u, v = m.velocity(m.vc)
    du = np.max(np.abs(P.sample_uv(u, v, probe, lx, ly) - P.cellular_velocity(probe, lx, ly, amp, mx, my)))
    theory = 9.0 / 384.0 * ((2 * np.pi * mx / nx) ** 4 + (2 * np.pi * my / ny) ** 4) * amp * 2 * np.pi * my / ly
    assert du <= 1.5 * theory, (du, theory)
    bound = 2.0 * amp * np.sqrt(k2) * du * (steps * dt)

    def psi_at(x):
        return amp * np.cos(2 * np.pi * mx / lx * x[:, 0]) * np.cos(2 * np.pi * my / ly * x[:, 1])
    x0 = rng.random((1000, 2)) * lx
    m.set_particles(x0)
    m.step(steps)
    x1 = m.particles()
    drift = np.max(np.abs(psi_at(x1) - psi_at(x0)))
    moved = np.max(np.abs(x1 - x0))
    print("cellular flow: max|dU| = %.3e m/s (theory %.3e), psi drift %.3e of a bound %.3e (psi amplitude %.1e), moved up to %.1f m" % (du, theory, drift, bound, amp, moved))
    assert moved > 1000.0
    assert drift <= bound
    assert bound < 1e-3 * amp                                   # the bound itself is tight: a thousandth of psi's range


# ---- the path matrix ----
def test_path_matrix_has_the_tracers_grids():
    import tracer_numpy as T
    assert [(k.nx, k.ny) for k in P.PATH_CASES] == [(k.nx, k.ny) for k in T.PATH_CASES]
    assert len(P.PATH_CASES) == 12
    for k in P.PATH_CASES:
        assert 2 <= k.steps <= 56 and k.what


def test_probes_ride_on_the_unmodified_run():
    """ProbedParticleModel64 at 96 x 64, 3 steps of the path matrix's inputs: its vorticity is Model64's and its true particles are
    ParticleModel64's, bit for bit (the probes change no state of the run), both probes move the particles, and they differ from each
    other; the positions hold grid points, first and last cells and points 3 domain lengths away"""
    from ref_numpy import Model64
    import tracer_numpy as T
    nx, ny, steps = 96, 64, 3
    vort, source, xy = P.particle_inputs(nx, ny, 3e-2)
    assert xy.shape == (P.NPART, 2) and xy.dtype == np.float64
    cell = np.floor(xy / (P.widen(600000.0) / np.array([nx, ny]))).astype(np.int64)
    for ax, n in ((0, nx), (1, ny)):
        assert (cell[:, ax] == 0).any() and (cell[:, ax] == n - 1).any() and (np.abs(xy[:, ax]) > 2.5 * 600000.0).any()
    assert np.array_equal(xy[:6], P.grid_points(nx, ny, 600000.0, 600000.0, 8, P.PARTICLE_SEED)[:6])
    m = P.particle_model(nx, ny, vort, source, xy, cls=P.ProbedParticleModel64)
    r = P.particle_model(nx, ny, vort, source, xy)
    b = Model64(nx, ny, nu=T.RECIPE_NU, dt=T.recipe_dt(nx, ny))
    b.set_vort(vort)
    b.src = source.astype(np.float64)
    for q in (m, r, b):
        q.step(steps)
    assert np.array_equal(m.vc, b.vc) and np.array_equal(r.vc, b.vc)
    assert np.array_equal(m.xy, r.xy)
    shifts = {k: P.max_shift(m.probe[k], m.xy) for k in P.PROBES}
    print("probes at %dx%d, %d steps: %s; apart by %.3g m" % (nx, ny, steps, shifts, P.max_shift(m.probe["masked"], m.probe["base"])))
    assert all(v > 1.0 for v in shifts.values())
    assert P.max_shift(m.probe["masked"], m.probe["base"]) > 1.0


def _check_conditions(case, f32, masked, base, moved, finite):
    bar = P.BAR_FACTOR * f32
    print("%dx%d, noise %g, %d steps: float32 %.3g m, bar %.3g m, probes %.3g (masked) / %.3g (base) m, moved %.3g m"
          % (case.nx, case.ny, case.vort_noise, case.steps, f32, bar, masked, base, moved))
    assert finite
    assert f32 > 0
    assert masked >= P.PROBE_FACTOR * bar and base >= P.PROBE_FACTOR * bar
    assert moved >= P.MOVED_FACTOR * bar
    for got, row in ((f32, case.f32), (masked, case.masked), (base, case.base), (moved, case.moved)):
        assert 0.5 <= got / row <= 2.0, (got, row)                  # a stale row of the table fails
    # and the row's own figures, which the GPU test of a live case takes its bar from, meet the conditions as well
    assert min(case.masked, case.base) >= P.PROBE_FACTOR * P.BAR_FACTOR * case.f32 and case.moved >= P.MOVED_FACTOR * P.BAR_FACTOR * case.f32


LIVE_CASES = [k for k in P.PATH_CASES if not k.fixture]
FIXTURE_CASES = [k for k in P.PATH_CASES if k.fixture]


@pytest.mark.parametrize("case", LIVE_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in LIVE_CASES])
def test_path_case_conditions_live(case):
    """The conditions on the inputs of the GPU path matrix, for every case whose float64 run takes under about 20 s: one float64 run
    with both probes and the float32 restatement.  The bar is 10 x the float32 figure; each probe (stage velocities at the stages 1 to
    3 from the stage state times the mask; from the base) shifts the float64 positions by >= 10 bars; the particles moved by >= 100
    bars; every position is finite; the figures are those of the case's row within a factor 2."""
    r = P.path_figures(case.nx, case.ny, case.vort_noise, case.steps)
    _check_conditions(case, r["f32"], r["masked"], r["base"], r["moved"], r["finite"])


@pytest.mark.parametrize("case", FIXTURE_CASES, ids=["%dx%d" % (k.nx, k.ny) for k in FIXTURE_CASES])
def test_path_case_conditions_stored(case):
    """the same conditions for the slow cases, from the figures that tests/golden/make_particle_fixtures.py stored with the float64
    positions; the stored parameters are the case's and the fixture is small"""
    import tracer_numpy as T
    path = os.path.join(HERE, "golden", P.fixture_name(case))
    assert os.path.getsize(path) <= 64 * 1024
    G = np.load(path)
    assert (int(G["seed"]), float(G["vort_noise"]), int(G["steps"])) == (P.PARTICLE_SEED, case.vort_noise, case.steps)
    assert (float(G["dt"]), float(G["nu"])) == (T.recipe_dt(case.nx, case.ny), T.RECIPE_NU)
    xy = G["xy"]
    assert xy.shape == (P.NPART, 2) and xy.dtype == np.float64
    x0 = P.seed_positions(case.nx, case.ny, 600000.0, 600000.0, P.NPART, int(G["seed"]))
    assert abs(P.max_shift(xy, x0) / float(G["moved"]) - 1) <= 1e-12
    _check_conditions(case, float(G["f32"]), float(G["shift_masked"]), float(G["shift_base"]), float(G["moved"]), bool(np.isfinite(xy).all()))
