"""float64 numpy reference of the Lagrangian particles: the 4-point cubic Lagrange interpolation of include/fftbaro.h
(fb_model_sample), the RK4 of particles in given stage velocities, and ref_numpy.Model64 extended by particles that are advanced
with the velocity of its own stage states, coupled stage by stage.  Used ONLY by tests."""
from collections import namedtuple

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


# ---- the particles' path matrix: inputs, sensitivity probes, float32 restatement (tests/test_gpu_particle_paths.py) ----
PARTICLE_SEED = 7
NPART = 1000
PROBES = ("masked", "base")


def particle_inputs(nx, ny, vort_noise, seed=PARTICLE_SEED, make_field=None):
    """(vort, source, xy): the vorticity and the source of tracer_numpy.noisy_inputs (the elliptic vortex plus never-dealiased white noise
    of the amplitude vort_noise, a white-noise source of 1e-9 s^-2) and seed_positions(nx, ny, 600000, 600000, 1000, seed).  To be run
    with nu = tracer_numpy.RECIPE_NU and dt = tracer_numpy.recipe_dt(nx, ny); the source stays on."""
    from tracer_numpy import noisy_inputs
    vort, _, source = noisy_inputs(nx, ny, vort_noise, make_field=make_field)
    return vort, source, seed_positions(nx, ny, 600000.0, 600000.0, NPART, seed)


class ProbedParticleModel64(ParticleModel64):
    """ParticleModel64 that carries, beside the true particles, two sets whose stage velocities at the stages 1 to 3 are formed wrongly:
      "masked"  from the stage state times the dealiasing mask: the stage array read at a masked mode (the engine never writes it there);
      "base"    from the base state v0: the base read everywhere, the stage array never picked.
    All three ride on ONE vorticity trajectory, whose step is Model64's formula for formula (the stage velocity of the true particles is
    the u, v that the tendency forms anyway), so a large grid costs one float64 run.  xy is the true set, probe[name] a wrong one."""

    def set_particles(self, xy):
        super().set_particles(xy)
        self.probe = {k: self.xy.copy() for k in PROBES}

    def _tendency_uv(self, vc):
        lv = vc * self.lap
        dzdx = self._c2r(self.ikx * vc)
        dzdy = self._c2r(self.iky * vc)
        psi = vc / self.lapi
        u = -self._c2r(self.iky * psi)
        v = self._c2r(self.ikx * psi)
        t = -u * dzdx - v * dzdy + self.src
        return (np.fft.rfft2(t) + lv * self.nu) * self.mask, u, v

    def step(self, n=1):
        dt = self.dt
        h = (None, dt / 2, dt / 2, dt)
        for _ in range(n):
            v0 = self.vc
            sets = {"true": self.xy, **self.probe}
            x = dict(sets)
            acc = {k: 0.0 for k in sets}
            ks, vs = [], v0
            for s in range(4):
                k, u, v = self._tendency_uv(vs)
                ks.append(k)
                if s == 0:
                    uv = {name: (u, v) for name in sets}
                    base = (u, v)
                else:
                    uv = {"true": (u, v), "masked": self.velocity(vs * self.mask), "base": base}
                for name in sets:
                    p = sample_uv(uv[name][0], uv[name][1], x[name], self.lx, self.ly)
                    acc[name] = p if s == 0 else (acc[name] + (2 * p if s < 3 else p))
                    if s < 3:
                        x[name] = sets[name] + h[s + 1] * p
                del uv, u, v
                if s < 3:
                    vs = v0 + k * h[s + 1]
            self.vc = v0 + (ks[0] + 2 * ks[1] + 2 * ks[2] + ks[3]) * dt / 6
            self.xy = sets["true"] + (dt / 6) * acc["true"]
            self.probe = {k: sets[k] + (dt / 6) * acc[k] for k in PROBES}


def particle_model(nx, ny, vort, source, xy, cls=ParticleModel64):
    """the float64 reference (cls=ProbedParticleModel64: with the two probes) loaded with the path matrix's inputs"""
    from tracer_numpy import RECIPE_NU, recipe_dt
    m = cls(nx, ny, nu=RECIPE_NU, dt=recipe_dt(nx, ny))
    m.set_vort(vort)
    m.src = np.asarray(source).astype(np.float64)
    m.set_particles(xy)
    return m


def float32_positions(nx, ny, vort, source, xy, steps, ref):
    """The positions of the ordinary float32 evaluation of the coupled run: the model stepped with torch's float32 / complex64 FFTs on
    the CPU in the formula order of Model64 (ref supplies the tables, nu and dt), u and v float32 fields, the interpolation and the
    positions in float64, as the engine does.  What a correct float32 engine can be expected to reach."""
    import torch
    f, c64 = torch.float32, torch.complex64
    ikx, iky = torch.from_numpy(ref.ikx).to(c64), torch.from_numpy(ref.iky).to(c64)
    lap, lapi, mask = (torch.from_numpy(a).to(f) for a in (ref.lap, ref.lapi, ref.mask))
    src = torch.from_numpy(np.asarray(source, dtype=np.float32))
    nu, dt = float(np.float32(ref.nu)), float(np.float32(ref.dt))
    lx, ly = ref.lx, ref.ly

    def c2r(a):
        return torch.fft.irfft2(a, s=(nx, ny))

    def tend(vc, x):
        psi = vc / lapi
        u, v = -c2r(iky * psi), c2r(ikx * psi)
        tv = -u * c2r(ikx * vc) - v * c2r(iky * vc) + src
        return (torch.fft.rfft2(tv) + vc * lap * nu) * mask, sample_uv(u.numpy(), v.numpy(), x, lx, ly)
    vc = torch.fft.rfft2(torch.from_numpy(np.asarray(vort, dtype=np.float32)))
    x0 = np.array(xy, dtype=np.float64).reshape(-1, 2)
    for _ in range(steps):
        k1, p1 = tend(vc, x0)
        k2, p2 = tend(vc + k1 * (dt / 2), x0 + (dt / 2) * p1)
        k3, p3 = tend(vc + k2 * (dt / 2), x0 + (dt / 2) * p2)
        k4, p4 = tend(vc + k3 * dt, x0 + dt * p3)
        vc = vc + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
        x0 = x0 + (dt / 6) * (((p1 + 2 * p2) + 2 * p3) + p4)
    return x0


def max_shift(a, b):
    """max |a - b| over particles and both coordinates, in metres"""
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def path_figures(nx, ny, vort_noise, steps, progress=None):
    """One float64 run of a case with both probes, and its float32 restatement: a dict of the final float64 positions `xy`, the final
    float64 vorticity `vort`, `f32` (the float32 figure), `masked` and `base` (the probes' shifts), `moved` (all max |.| in metres) and
    `finite`."""
    vort, source, xy = particle_inputs(nx, ny, vort_noise)
    m = particle_model(nx, ny, vort, source, xy, cls=ProbedParticleModel64)
    for k in range(steps):
        m.step(1)
        if progress:
            progress(k + 1)
    x32 = float32_positions(nx, ny, vort, source, xy, steps, m)
    return {"xy": m.xy, "vort": m.vort(), "f32": max_shift(x32, m.xy), "masked": max_shift(m.probe["masked"], m.xy),
            "base": max_shift(m.probe["base"], m.xy), "moved": max_shift(m.xy, xy), "finite": bool(np.isfinite(m.xy).all())}


# The path matrix: one row per grid class of the engine, the grids, noise and step counts of tracer_numpy.PATH_CASES.
# f32: max |X_f32 - X_64| of float32_positions against the float64 run; the bar of the GPU test is BAR_FACTOR * f32 (the factor is the
# margin for the engine's FFT factorisations and operation order, which differ from torch's; the tracer's suite allows 40 on the same
# grounds, 1e-5 against 2.5e-7).  masked / base: the shifts of the two probes of ProbedParticleModel64; moved: the largest displacement.
# All in metres, measured on the CPU, never taken from the engine.  Conditions (tests/test_particles_cpu.py): each probe >= PROBE_FACTOR
# bars, moved >= MOVED_FACTOR bars, every position finite.  fixture: the float64 run takes over 20 s, so the positions and the figures are
# read from tests/golden (tests/golden/make_particle_fixtures.py); the others run live.
ParticleCase = namedtuple("ParticleCase", "nx ny vort_noise steps fixture f32 masked base moved what")
BAR_FACTOR, PROBE_FACTOR, MOVED_FACTOR = 10.0, 10.0, 100.0
PATH_CASES = (
    ParticleCase(256, 256, 3e-2, 5, False, 0.000391, 257, 60, 2.66e+03, "ZA/ZB read in place (N2 = 16 < 32), plain row kernels"),
    ParticleCase(192, 192, 3e-2, 5, False, 0.000545, 304, 91.5, 2.97e+03, "ZA/ZB read in place; k_row3; N1 = 24, N2 = 8"),
    ParticleCase(3072, 64, 3e-2, 5, False, 7.27e-05, 15.5, 6.44, 489, "k_tracer_vstate_tm at N1 = 24, N2 = 128"),
    ParticleCase(1024, 64, 3e-2, 5, False, 0.000429, 98.2, 115, 2.59e+03, "k_tracer_vstate_tm at N2 = 32; the slab's entry points"),
    ParticleCase(4096, 64, 3e-2, 5, False, 5.09e-05, 7.51, 3.04, 304, "k_tracer_vstate_tm, N1 = N2 = 64; the three-kernel x pass (live Nyquist column)"),
    ParticleCase(8192, 64, 3e-2, 12, False, 5.32e-05, 3.5, 3.61, 421, "k_tracer_vstate_tm, N1 = 128, N2 = 64"),
    ParticleCase(16384, 64, 3e-2, 56, True, 0.000159, 3.73, 2.32, 852, "k_tracer_vstate_tm, N1 = N2 = 128"),
    ParticleCase(64, 4096, 3e-2, 5, False, 5.35e-05, 7.73, 5.19, 335, "ZA/ZB read in place; ROW_INV through k_rowq (FB_ROWQ=0: k_row8)"),
    ParticleCase(64, 8192, 3e-2, 12, False, 4.81e-05, 5.29, 2.41, 425, "ZA/ZB read in place; ROW_INV through k_rowh<1>"),
    ParticleCase(128, 16384, 3e-2, 56, True, 0.000309, 5.31, 3.11, 851, "ZA/ZB read in place; ROW_INV through k_rowh<2>"),
    ParticleCase(4096, 4096, 3e-2, 3, True, 2.22e-05, 2.98, 2.03, 185, "XP_FULL1: k_tracer_vstate_full at nsub = 1; ROW_INV through k_rowq"),
    ParticleCase(8192, 8192, 3e-2, 2, True, 6.47e-06, 0.369, 0.196, 58.6, "XP_FULL2: k_tracer_vstate_full at nsub = 2; ROW_INV through k_rowh<1>"),
)


def path_case(nx, ny):
    return [k for k in PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]


def fixture_name(case):
    return "particles_%dx%d_step%d.npz" % (case.nx, case.ny, case.steps)
