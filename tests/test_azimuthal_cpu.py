"""No GPU: the numpy evaluation of the azimuthal-mean table (tests/azimuthal_numpy.py) on analytic fields, so that the yardstick of
tests/test_gpu_azimuthal.py is itself pinned; and the host logic of the C ABI (fb_azimuthal_cols)."""
import ctypes

import numpy as np

import azimuthal_numpy as A

L = 600000.0


def _polar(nx, ny, ic, jc):
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    xc, yc = ic * dx, jc * dy
    r, c1, s1, b = A.geometry(nx, ny, L, L, xc, yc, max(dx, dy))
    return xc, yc, r, c1, s1


def test_rigid_rotation():
    """u = -Omega y', v = Omega x' about a grid point: v_t = Omega r, v_r = 0 at every point, so <v_t> = Omega <r>, <v_r> = 0, and the
    constant zeta = 2 Omega has no azimuthal wavenumber on a lattice that is symmetric about the centre."""
    nx = ny = 64
    om = 1.0e-3
    xc, yc, r, c1, s1 = _polar(nx, ny, 20, 33)
    u, v = (-om * r * s1).astype(np.float32), (om * r * c1).astype(np.float32)
    zeta = np.full((nx, ny), 2 * om, np.float32)
    nbins, dr = 24, L / nx
    t, _ = A.table(zeta, u, v, L, L, xc, yc, nbins, dr, 3)
    assert np.all(t[:, 2] > 0)
    vmax = om * nbins * dr
    assert np.max(np.abs(t[:, 5] - om * t[:, 3])) <= 4e-7 * vmax          # float32 u, v
    assert np.max(np.abs(t[:, 6])) <= 4e-7 * vmax
    assert np.max(np.abs(t[:, 4] - np.float64(np.float32(2 * om)))) <= 1e-15
    assert np.max(np.abs(t[1:, 12:])) <= 1e-15 * 2 * om * 64              # sums of c_m, s_m over a symmetric ring vanish to rounding (bin 0: the centre alone)
    assert np.all(t[:, 8] >= t[:, 5] ** 2 * (1 - 1e-12)) and np.max(np.abs(t[:, 9])) <= (4e-7 * vmax) ** 2


def test_wavenumber_two():
    """zeta = cos(2 theta) f(r) about a grid point of a square grid: zeta_2 is real with <cos^2 2 theta f>, zeta_1 = zeta_3 = 0 (the
    lattice is symmetric under rotation by 90 degrees and under reflection)."""
    nx = ny = 64
    xc, yc, r, c1, s1 = _polar(nx, ny, 32, 32)
    c2 = c1 * c1 - s1 * s1
    f = np.exp(-(r / 1.0e5) ** 2)
    zeta = (c2 * f).astype(np.float32)
    zero = np.zeros_like(zeta)
    nbins, dr = 28, L / nx
    t, _ = A.table(zeta, zero, zero, L, L, xc, yc, nbins, dr, 3)
    b = A.geometry(nx, ny, L, L, xc, yc, dr)[3]
    want = np.array([np.mean((zeta.astype(np.float64) * c2)[b == k]) for k in range(nbins)])
    assert np.max(np.abs(t[:, 14] - want)) <= 1e-15
    assert np.max(np.abs(t[1:, 14])) > 0.3
    for col in (12, 13, 15, 16, 17):
        assert np.max(np.abs(t[1:, col])) <= 1e-15, col                      # (bin 0 is the centre alone: c_m = 1, s_m = 0 there)
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    assert np.max(np.abs(t[1:, 4])) <= 1e-15 and np.max(np.abs(t[:, 11] - dx * dy)) <= 1e-15 * L * L


def test_counts_sum_to_the_disc():
    for nx, ny, ic, jc in ((64, 64, 3, 60), (192, 64, 100, 0), (64, 256, 63, 255)):
        lx, ly, dx, dy = A.grid_steps(nx, ny, L, L)
        nbins, dr = A.default_bins(nx, ny, L, L)
        xc, yc = ic * dx, jc * dy
        z = np.ones((nx, ny), np.float32)
        t, _ = A.table(z, z, z, L, L, xc, yc, nbins, dr, 0)
        ix = (np.arange(nx) - ic + nx // 2) % nx - nx // 2                  # the minimum image in whole grid steps
        iy = (np.arange(ny) - jc + ny // 2) % ny - ny // 2
        r2 = (ix[:, None] * dx) ** 2 + (iy[None, :] * dy) ** 2
        assert t[:, 2].sum() == np.count_nonzero(r2 < (nbins * dr) ** 2)
        assert t.shape == (nbins, 12) and np.array_equal(t[:, 0], np.arange(nbins) * dr)
        assert t[-1, 11] == dx * dy * t[:, 2].sum()                          # Gamma of zeta = 1: the area of the points counted


def test_find_center_ties():
    f = np.zeros((8, 16), np.float32)
    assert A.find_center(f, L, L, False)[2] == 0 and A.find_center(f, L, L, True)[2] == 0
    f[3, 5] = f[6, 1] = -2.0
    c = A.find_center(f, L, L, False)
    assert c[2] == 3 * 16 + 5 and c[3] == -2.0 and c[0] == 3 * (np.float64(np.float32(L)) / 8)


def test_azimuthal_cols_host_logic():
    import xlab_fftbarotropic_amd as X
    Lb = X.lib()
    for m in range(9):
        assert X.azimuthal_cols(m) == 12 + 2 * m
    n = ctypes.c_int(7)
    assert Lb.fb_azimuthal_cols(9, ctypes.byref(n)) == 1 and n.value == 0 and b"nmodes" in Lb.fb_last_error()
    assert Lb.fb_azimuthal_cols(-1, ctypes.byref(n)) == 1
    assert Lb.fb_azimuthal_cols(4, None) == 1
    assert Lb.fb_version() == 201
