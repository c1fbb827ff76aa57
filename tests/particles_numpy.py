"""float64 numpy reference of the Lagrangian particles: the 4-point cubic Lagrange interpolation of include/fftbaro.h
(fb_model_sample), the RK4 of particles in given stage velocities, and ref_numpy.Model64 extended by particles that are advanced
with the velocity of its own stage states, coupled stage by stage.  Used ONLY by tests."""
import numpy as np

from ref_numpy import Model64


def widen(l):
    """a length as the engine takes it: float32, widened"""
    return float(np.float32(l))


def lagrange4_axis(x, d, n):
    """indices [npts, 4] and weights [npts, 4] of one axis: s = x / d, i0 = floor(s) as a 64-bit integer, t = s - i0, the rows
    (i0 - 1 .. i0 + 2) mod n as a non-negative modulus"""
    s = np.asarray(x, dtype=np.float64) / d
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    t = s - fl
    idx = np.mod(i0[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], n)
    w = np.stack([-t * (t - 1.0) * (t - 2.0) / 6.0,
                  (t + 1.0) * (t - 1.0) * (t - 2.0) / 2.0,
                  -(t + 1.0) * t * (t - 2.0) / 2.0,
                  (t + 1.0) * t * (t - 1.0) / 6.0], axis=1)
    return idx, w


def lagrange4_sample(field, xy, lx, ly):
    """The [nx][ny] field (grid point (i, j) at x = i dx, y = j dy, dx = lx / nx, dy = ly / ny with the float32 lengths widened)
    interpolated to the positions xy [npts, 2] by the tensor product of 4-point cubic Lagrange polynomials, in float64: per x row of
    the stencil the sum over y, then the sum over the rows."""
    f = np.asarray(field)
    nx, ny = f.shape
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ix, wx = lagrange4_axis(xy[:, 0], widen(lx) / nx, nx)
    jy, wy = lagrange4_axis(xy[:, 1], widen(ly) / ny, ny)
    acc = np.zeros(xy.shape[0])
    for a in range(4):
        q = f[ix[:, a, None], jy].astype(np.float64)                       # [npts, 4]
        r = ((wy[:, 0] * q[:, 0] + wy[:, 1] * q[:, 1]) + wy[:, 2] * q[:, 2]) + wy[:, 3] * q[:, 3]
        acc = acc + wx[:, a] * r
    return acc


def rk4_particles(xy, stage_velocity, dt, steps):
    """RK4 of the positions xy [npts, 2]: stage_velocity(step, stage, X) -> U [npts, 2] is the velocity of stage 0..3 of that step at
    the positions X; k1 = U_0(X0), k2 = U_1(X0 + dt/2 k1), k3 = U_2(X0 + dt/2 k2), k4 = U_3(X0 + dt k3),
    X <- X0 + dt/6 (k1 + 2 k2 + 2 k3 + k4).  Positions stay unwrapped."""
    x = np.array(xy, dtype=np.float64).reshape(-1, 2)
    for n in range(steps):
        k1 = stage_velocity(n, 0, x)
        k2 = stage_velocity(n, 1, x + (dt / 2) * k1)
        k3 = stage_velocity(n, 2, x + (dt / 2) * k2)
        k4 = stage_velocity(n, 3, x + dt * k3)
        x = x + (dt / 6) * (((k1 + 2 * k2) + 2 * k3) + k4)
    return x


def sample_uv(u, v, x, lx, ly):
    return np.stack([lagrange4_sample(u, x, lx, ly), lagrange4_sample(v, x, lx, ly)], axis=1)


class ParticleModel64(Model64):
    """Model64 with particles: every step advances them by the RK4 scheme of the step itself, stage s with u = -psi_y, v = psi_x of
    the vorticity's state of stage s (float64 fields), interpolated by lagrange4_sample."""

    def __init__(self, nx, ny, lx=600000.0, ly=600000.0, nu=6.5, dt=3.0):
        super().__init__(nx, ny, lx, ly, nu, dt)
        self.lx, self.ly = lx, ly
        self.xy = None

    def set_particles(self, xy):
        self.xy = np.array(xy, dtype=np.float64).reshape(-1, 2)

    def velocity(self, vc):
        psi = vc / self.lapi
        return -self._c2r(self.iky * psi), self._c2r(self.ikx * psi)

    def _U(self, vc, x):
        u, v = self.velocity(vc)
        return sample_uv(u, v, x, self.lx, self.ly)

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, x0 = self.vc, self.xy
            k1, p1 = self.tendency(v0), self._U(v0, x0)
            v1 = v0 + k1 * (dt / 2)
            k2, p2 = self.tendency(v1), self._U(v1, x0 + (dt / 2) * p1)
            v2 = v0 + k2 * (dt / 2)
            k3, p3 = self.tendency(v2), self._U(v2, x0 + (dt / 2) * p2)
            v3 = v0 + k3 * dt
            k4, p4 = self.tendency(v3), self._U(v3, x0 + dt * p3)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.xy = x0 + (dt / 6) * (((p1 + 2 * p2) + 2 * p3) + p4)

    def particles(self):
        return self.xy


def cellular_velocity(x, lx, ly, amp, mx, my):
    """u = -psi_y, v = psi_x of tracer_numpy.cellular_flow's psi = A cos(kx x) cos(ky y), analytically, at the positions x [npts, 2]"""
    kx, ky = 2 * np.pi * mx / lx, 2 * np.pi * my / ly
    return np.stack([amp * ky * np.cos(kx * x[:, 0]) * np.sin(ky * x[:, 1]),
                     -amp * kx * np.sin(kx * x[:, 0]) * np.cos(ky * x[:, 1])], axis=1)


def stage_factors(z):
    """the vorticity's stage states of one RK4 step of y' = lambda y over its base, z = lambda dt"""
    return (1.0, 1 + z / 2, 1 + z / 2 + z * z / 4, 1 + z + z * z / 2 + z ** 3 / 4)


def seed_positions(nx, ny, lx, ly, n, seed=7):
    """n positions that cover what the interpolation must get right: grid points, the first and the last cell of both axes, positions
    3 domain lengths away on either side, the rest uniform in the domain.  The leading min(n, 8) are grid points (exact: see
    grid_points)."""
    lx, ly = widen(lx), widen(ly)
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * np.array([lx, ly])
    g = grid_points(nx, ny, lx, ly, min(n, 8), seed)
    xy[:g.shape[0]] = g
    dx, dy = lx / nx, ly / ny
    special = [(0.3 * dx, 0.6 * ly), (lx - 0.4 * dx, 0.2 * ly), (0.5 * lx, 0.7 * dy), (0.1 * lx, ly - 0.2 * dy), (lx - 0.5 * dx, ly - 0.5 * dy),
               (0.25 * dx, 0.75 * dy), (3 * lx + 0.37 * lx, 0.4 * ly), (-3 * lx + 0.11 * lx, 0.9 * ly), (0.6 * lx, 3 * ly + 0.21 * ly),
               (0.8 * lx, -3 * ly + 0.43 * ly), (-3 * lx + 0.2 * dx, -3 * ly + 0.3 * dy), (3 * lx - 0.2 * dx, 3 * ly - 0.3 * dy)]
    k = g.shape[0]
    for p in special:
        if k < n:
            xy[k] = p
            k += 1
    return xy


def grid_points(nx, ny, lx, ly, n, seed=7):
    """up to n positions ON grid points (i dx, j dy), among them the corners and points 3 domain lengths away, kept only where the
    float64 division of the position by the spacing gives the integer back exactly, so that t == 0 on both axes"""
    lx, ly = widen(lx), widen(ly)
    dx, dy = lx / nx, ly / ny
    rng = np.random.default_rng(seed + 1)
    ij = np.concatenate([np.array([[0, 0], [nx - 1, ny - 1], [0, ny - 1], [nx - 1, 0], [3 * nx + 5, 7], [-3 * nx + 2, -3 * ny + 9]]),
                         np.stack([rng.integers(0, nx, 4 * n + 8), rng.integers(0, ny, 4 * n + 8)], axis=1)]).astype(np.float64)
    xy = ij * np.array([dx, dy])
    keep = (xy[:, 0] / dx == ij[:, 0]) & (xy[:, 1] / dy == ij[:, 1])
    return xy[keep][:n]
