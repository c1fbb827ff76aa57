"""CPU checks of the float64 reference of the particles' deformation gradient (tests/deformation_numpy.py), which the GPU tests
(tests/test_gpu_deformation.py) compare the engine with: F against finite differences of the particle map, the parallel shear that RK4
integrates exactly, the closed-form 2 x 2 decomposition against numpy.linalg.svd, and the Python surface.  No GPU."""
import inspect
import os
import sys
from importlib import import_module

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

EPS64 = float(np.finfo(np.float64).eps)


def _cellular_uv(nx, ny, lx, ly, amp=1.0e6, mx=2, my=3):
    """u, v of tracer_numpy.cellular_flow on the grid, as float32 fields (the frozen flow: nu = 0, the fields never change)"""
    import particles_numpy as P
    x, y = np.meshgrid(np.arange(nx) * (lx / nx), np.arange(ny) * (ly / ny), indexing="ij")
    uv = P.cellular_velocity(np.stack([x.ravel(), y.ravel()], axis=1), lx, ly, amp, mx, my)
    return uv[:, 0].reshape(nx, ny).astype(np.float32), uv[:, 1].reshape(nx, ny).astype(np.float32)


@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64)])
def test_F_against_finite_differences(nx, ny):
    """F of rk4_deformation against central finite differences of particles_numpy.rk4_particles in the frozen cellular flow, u and v
    float32 fields: dt = 3, 40 steps, h = 1e-2 m, 1000 uniform positions.  The difference quotient's float64 noise is
    eps64 L / h ~ 1e-8; the bar is 1e-6.  A particle whose two displaced copies lie in different cells at any stage position of the
    run straddles a face, where the map is not differentiable: it is left out, at most 1 % may be (measured here: none, max
    |F_fd - F| 4.2e-8 and 4.6e-8, median 9e-9, max |F - I| 0.117, det F in [0.99987, 1.00013])."""
    import deformation_numpy as D
    import particles_numpy as P
    lx = ly = P.widen(600000.0)
    dt, steps, h, n = 3.0, 40, 1e-2, 1000
    u, v = _cellular_uv(nx, ny, lx, ly)
    x0 = np.random.default_rng(3).random((n, 2)) * np.array([lx, ly])
    _, F = D.rk4_deformation(x0, D.identity(n), lambda k, s, x: D.sample_uv_grad(u, v, x, lx, ly), dt, steps)
    cells = {}

    def run(tag, start):
        cells[tag] = []

        def vel(k, s, x):
            cells[tag].append(np.floor(x / np.array([lx / nx, ly / ny])))
            return P.sample_uv(u, v, x, lx, ly)
        return P.rk4_particles(start, vel, dt, steps)
    Ffd = np.empty((n, 2, 2))
    straddle = np.zeros(n, dtype=bool)
    for j in range(2):
        e = np.zeros(2)
        e[j] = h
        Ffd[:, :, j] = (run("+", x0 + e) - run("-", x0 - e)) / (2 * h)
        for a, b in zip(cells["+"], cells["-"]):
            straddle |= (a != b).any(axis=1)
    err = np.abs(Ffd - F).max(axis=(1, 2))
    det = np.linalg.det(F)
    print("F vs finite differences %dx%d: left out %d, max err %.3e, median %.3e, max|F - I| %.3f, det in [%.5f, %.5f]" %
          (nx, ny, int(straddle.sum()), float(err[~straddle].max()), float(np.median(err)), float(np.abs(F - np.eye(2)).max()), det.min(), det.max()))
    assert straddle.sum() <= n // 100
    assert float(err[~straddle].max()) <= 1e-6
    assert float(np.abs(F - np.eye(2)).max()) > 0.05            # the flow deforms: the identity would not pass
    assert 0.999 < det.min() and det.max() < 1.001 and not np.all(det == 1.0)


def test_parallel_shear_is_exact():
    """psi = A cos(k y), steady: u = A k sin(k y), v = 0.  With the interpolated field held fixed y never changes, A = [[0, u_y], [0, 0]]
    is the same at every stage, A^2 = 0, and RK4 gives F = [[1, T u_y(y0)], [0, 1]] exactly, u_y the interpolant's own derivative.
    Within 64 eps64 max|F| (40 steps of one multiply-add each)."""
    import deformation_numpy as D
    import particles_numpy as P
    nx, ny, n = 64, 64, 500
    lx = ly = P.widen(600000.0)
    dt, steps = 3.0, 40
    k = 2 * np.pi / ly
    y = np.arange(ny) * (ly / ny)
    u = np.tile((1.0e6 * k * np.sin(k * y))[None, :], (nx, 1)).astype(np.float32)
    v = np.zeros_like(u)
    x0 = np.random.default_rng(5).random((n, 2)) * np.array([lx, ly])
    x, F = D.rk4_deformation(x0, D.identity(n), lambda kk, s, xx: D.sample_uv_grad(u, v, xx, lx, ly), dt, steps)
    _, _, uy = D.lagrange4_sample_grad(u, x0, lx, ly)
    want = D.identity(n)
    want[:, 0, 1] = steps * dt * uy
    err = float(np.max(np.abs(F - want)))
    print("parallel shear: max|F12| %.4f, err %.3e, bar %.3e" % (float(np.abs(want[:, 0, 1]).max()), err, 64 * EPS64 * float(np.abs(want).max())))
    assert np.array_equal(x[:, 1], x0[:, 1])
    assert float(np.abs(want[:, 0, 1]).max()) > 0.01
    assert err <= 64 * EPS64 * float(np.abs(want).max())


def test_svd2x2_against_numpy():
    """svd2x2 against numpy.linalg.svd on 2000 random matrices (normal entries; a quarter of them scaled by 10^U(-100, 100)) and on the
    hard cases: the bars of deformation_numpy.check_stretching.  Non-finite rows give NaN; theta_in is the direction that is stretched
    most: |F v| = sigma1 for v = (cos theta_in, sin theta_in)."""
    import deformation_numpy as D
    rng = np.random.default_rng(17)
    F = rng.standard_normal((2000, 2, 2))
    F[::4] *= 10.0 ** rng.uniform(-100, 100, (500, 1, 1))
    worst = D.check_stretching(D.svd2x2(F), F, "random")
    names, H = D.hard_matrices()
    assert names == ["identity", "rotation", "det < 0", "singular", "zero", "1e200", "1e-200", "ratio 1e12"]
    table = D.svd2x2(H)
    worst_h = D.check_stretching(table, H, "hard")
    print("svd2x2: random ln s1 %.2e, ln s2 %.2e, reconstruction %.2e; hard %.2e, %.2e, %.2e" % tuple(worst + worst_h))
    assert table[names.index("singular"), 1] == -np.inf and np.isfinite(table[names.index("singular"), 0])
    assert abs(table[names.index("ratio 1e12"), 0] - np.log(1e6)) < 1e-12 and abs(table[names.index("ratio 1e12"), 1] - np.log(1e-6)) < 1e-4
    assert abs(table[names.index("identity")][:2]).max() == 0.0
    bad = np.array([[[np.nan, 0.0], [0.0, 1.0]], [[1.0, np.inf], [0.0, 1.0]], [[1.0, 0.0], [-np.inf, 1.0]]])
    assert np.isnan(D.svd2x2(bad)).all()
    t = D.svd2x2(F[1::4])
    vin = np.stack([np.cos(t[:, 2]), np.sin(t[:, 2])], axis=1)
    grown = np.linalg.norm(np.einsum("pij,pj->pi", F[1::4], vin), axis=1)
    assert np.max(np.abs(grown / np.exp(t[:, 0]) - 1.0)) < 1e-12
    vout = np.stack([np.cos(t[:, 3]), np.sin(t[:, 3])], axis=1)
    cross = np.einsum("pij,pj->pi", F[1::4], vin)
    assert np.max(np.abs(cross[:, 0] * vout[:, 1] - cross[:, 1] * vout[:, 0]) / np.exp(t[:, 0])) < 1e-12     # F v_in is parallel to v_out


def test_surface():
    import xlab_fftbarotropic_amd as X
    B = import_module("xlab-fftbarotropic_amd.binding")
    slab = import_module("xlab-fftbarotropic_amd.slab")
    for stem in ("set_particle_deformation", "get_particle_deformation", "particle_stretching"):
        assert "fb_model_" + stem in X.EXPORTS and "fb_slab_" + stem in X.EXPORTS, stem
        assert stem in B._DEFORMATION_PAIRS and stem not in B._PAIRS
    for name in ("set_particle_deformation", "particle_deformation", "particle_deformation_time", "particle_stretching", "ftle"):
        m, e = getattr(B.Model, name), getattr(slab.EngineSlab, name)
        assert m is e is getattr(B.ModelSurface, name), name
        assert inspect.signature(m) == inspect.signature(e)
    assert X.PARTICLE_STRETCHING_COLUMNS == ("ln_sigma1", "ln_sigma2", "theta_in", "theta_out")
