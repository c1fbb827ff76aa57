"""float64 numpy reference of the coupled system vorticity + passive tracer: ref_numpy.Model64 extended by a tracer c with a
diffusivity kappa of its own.  Each RK4 stage computes the tracer's tendency with the streamfunction of the vorticity's state of
that stage,

    tend_c = mask * ( r2c(-u c_x - v c_y) + kappa * laplacian_coe * c_c ),   u = -psi_y, v = psi_x, psi_c = vort_c / laplacian_coe

in the formula order of ref_numpy.Model64.tendency with c in the place of zeta and no source.  Also the inputs of the tracer's path
matrix (noisy_inputs: state in the masked modes of both fields, and a vorticity source) and the sensitivity probe that shows those
inputs make the parity bar decisive (ProbeModel64).  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

from ref_numpy import Model64, rel_l2


class TracerModel64(Model64):
    """self.src (Model64: the vorticity source, a real [nx][ny] field, zero by default) enters the vorticity's tendency only.  That is
    the intended semantics: the source forces the flow, so it reaches the tracer through the velocity of every later stage, and it is
    no term of the tracer's own tendency (the engine runs the tracer's row pass without a source)."""

    def __init__(self, nx, ny, lx=600000.0, ly=600000.0, nu=6.5, dt=3.0, kappa=0.0):
        super().__init__(nx, ny, lx, ly, nu, dt)
        self.kappa = float(np.float32(kappa))
        self.cc = None

    def set_tracer(self, c, kappa=None):
        self.cc = np.fft.rfft2(np.asarray(c).astype(np.float64))
        if kappa is not None:
            self.kappa = float(np.float32(kappa))

    def tracer_tendency(self, vc, cc):
        lc = cc * self.lap
        dcdx = self._c2r(self.ikx * cc)
        dcdy = self._c2r(self.iky * cc)
        psi = vc / self.lapi
        u = -self._c2r(self.iky * psi)
        v = self._c2r(self.ikx * psi)
        t = -u * dcdx - v * dcdy
        return (np.fft.rfft2(t) + lc * self.kappa) * self.mask

    def stage_tracer_tendency(self, vc, cc):
        """the tracer's tendency at the stages 1 to 3, from the stage states (ProbeModel64 overrides it)"""
        return self.tracer_tendency(vc, cc)

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, c0 = self.vc, self.cc
            k1, l1 = self.tendency(v0), self.tracer_tendency(v0, c0)
            v1, c1 = v0 + k1 * (dt / 2), c0 + l1 * (dt / 2)
            k2, l2 = self.tendency(v1), self.stage_tracer_tendency(v1, c1)
            v2, c2 = v0 + k2 * (dt / 2), c0 + l2 * (dt / 2)
            k3, l3 = self.tendency(v2), self.stage_tracer_tendency(v2, c2)
            v3, c3 = v0 + k3 * dt, c0 + l3 * dt
            k4, l4 = self.tendency(v3), self.stage_tracer_tendency(v3, c3)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.cc = c0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6

    def tracer(self):
        return self._c2r(self.cc)


class ProbeModel64(TracerModel64):
    """The sensitivity probe: TracerModel64 whose TRACER tendency at the stages 1 to 3 sees the modes outside the dealiasing circle as
    zero, in the vorticity's stage state (blind_vort), in the tracer's (blind_tracer), or in both.  The engine stores a stage state
    only where a mode can change and reads a masked mode from the base; a kernel that picked the stage array there, or a stage array
    that was never filled, would do what this model does.  The vorticity's own step and stage 0 are those of TracerModel64, so the
    vorticity is the unmodified run's and the shift of the tracer against that run measures how much the masked modes matter."""

    def __init__(self, *args, blind_vort=False, blind_tracer=False, **kw):
        super().__init__(*args, **kw)
        self.blind_vort, self.blind_tracer = bool(blind_vort), bool(blind_tracer)

    def stage_tracer_tendency(self, vc, cc):
        return self.tracer_tendency(vc * self.mask if self.blind_vort else vc, cc * self.mask if self.blind_tracer else cc)


RECIPE_SEED = 20240
RECIPE_KAPPA, RECIPE_NU = 20.0, 6.5
TRACER_NOISE = 0.05


# The path matrix: one row per grid class of the engine.  vort_noise and steps are chosen so that BOTH probes (ProbeModel64) shift
# the float64 tracer by >= 1e-4 relative L2, ten times the parity bar of 1e-5, while the float32 evaluation of the same system stays
# near 2.5e-7 (measured with a float32 torch restatement on the CPU; at a noise of 3e-1 it reaches 2e-6 to 5e-6, too close to the
# bar, so the amplitude stays at 3e-2 and the long grids take more steps: the shift grows linearly with the step count).
# shift_vort / shift_tracer: the measured shifts (CPU, float64).  fixture: the reference is read from tests/golden (made by
# tests/golden/make_tracer_fixtures.py, which stores the shifts it measured) because it takes over 20 s; the others run live and
# tests/test_tracer_cpu.py asserts their shifts.
PathCase = namedtuple("PathCase", "nx ny vort_noise steps fixture shift_vort shift_tracer what")
PATH_CASES = (
    PathCase(256, 256, 3e-2, 5, False, 3.5e-2, 6.9e-2, "masked-mode logic on the plain path: N2 = 16 < 32, state in the 3-pass layout"),
    PathCase(192, 192, 3e-2, 5, False, 3.5e-2, 6.9e-2, "k_row3; N1 = 24, N2 = 8"),
    PathCase(3072, 64, 3e-2, 5, False, 3.9e-4, 1.4e-2, "N1 = 24 with tile-major state, N2 = 128"),
    PathCase(1024, 64, 3e-2, 5, False, 3.4e-3, 4.0e-2, "k_tracer_vstate_tm at N2 = 32"),
    PathCase(4096, 64, 3e-2, 5, False, 2.2e-4, 1.1e-2, "tile-major, N1 = N2 = 64; the three-kernel x pass (live Nyquist column)"),
    PathCase(8192, 64, 3e-2, 12, False, 1.25e-4, 1.2e-2, "N1 = 128, N2 = 64"),
    PathCase(16384, 64, 3e-2, 56, True, 1.11e-4, 1.34e-2, "N1 = N2 = 128"),
    PathCase(64, 4096, 3e-2, 5, False, 2.3e-4, 1.1e-2, "k_rowq (FB_ROWQ=0: k_row8)"),
    PathCase(64, 8192, 3e-2, 12, False, 1.29e-4, 1.2e-2, "k_rowh<1>"),
    PathCase(128, 16384, 3e-2, 56, True, 2.23e-4, 1.35e-2, "k_rowh<2>"),
    PathCase(4096, 4096, 3e-2, 3, True, 5.3e-3, 1.1e-2, "k_col_full<., 1> and k_tracer_vstate_full at nsub = 1; k_rowq"),
    PathCase(8192, 8192, 3e-2, 2, True, 1.78e-3, 3.87e-3, "k_col_full<., 2>, k_rowh2 and k_tracer_vstate_full at nsub = 2; the tracer's rows through k_rowh<1>"),
)
SHIFT_BAR = 1e-4


def offset_gaussian(nx, ny=None, make_field=None):
    """the gaussian of make_field("gaussian"), moved off the vortices by a quarter of the domain in x and an eighth in y"""
    if make_field is None:
        from oracle_py import make_field
    g = make_field("gaussian", nx, ny or nx)
    return np.ascontiguousarray(np.roll(np.roll(g, g.shape[0] // 4, axis=0), g.shape[1] // 8, axis=1))


def recipe_dt(nx, ny):
    """the project's scaling of the time step with the grid: 3 s at 1024 points and below"""
    return 3.0 * min(1.0, 1024.0 / max(nx, ny))


def noisy_inputs(nx, ny, vort_noise, seed=RECIPE_SEED, make_field=None):
    """The inputs of the tracer's path matrix on any supported nx x ny, as float32 fields (vort, tracer, source):
      vort    the elliptic vortex plus white noise of the amplitude vort_noise (s^-1, absolute: the vortex's maximum is 5e-3), NOT dealiased;
      tracer  the offset gaussian plus white noise of TRACER_NOISE = 5 % of its maximum, NOT dealiased;
      source  white noise of amplitude 1e-9 (s^-2).
    White noise that was never dealiased has state at every wavenumber outside the dealiasing circle, in the ky = ny/2 column and in
    the kx = nx/2 row.  To be run with dt = recipe_dt(nx, ny), kappa = RECIPE_KAPPA, nu = RECIPE_NU.  The three noise fields are drawn
    in this order from one generator, so a field does not depend on whether the others are used."""
    if make_field is None:
        from oracle_py import make_field
    rng = np.random.default_rng(seed)
    vort = (make_field("elliptic", nx, ny) + vort_noise * rng.standard_normal((nx, ny))).astype(np.float32)
    c = offset_gaussian(nx, ny, make_field)
    tracer = (c + (TRACER_NOISE * float(np.abs(c).max())) * rng.standard_normal((nx, ny))).astype(np.float32)
    return vort, tracer, (1e-9 * rng.standard_normal((nx, ny))).astype(np.float32)


def noisy_vort(nx, ny, vort_noise, seed=RECIPE_SEED, make_field=None):
    """noisy_inputs(...)[0] alone (the generator's first draw), for the large grids of the twin check"""
    if make_field is None:
        from oracle_py import make_field
    rng = np.random.default_rng(seed)
    return (make_field("elliptic", nx, ny) + vort_noise * rng.standard_normal((nx, ny))).astype(np.float32)


def recipe_model(nx, ny, vort, tracer, source, cls=TracerModel64, **kw):
    """the float64 reference (or a probe variant: cls=ProbeModel64, blind_vort= / blind_tracer=) loaded with the recipe's inputs"""
    m = cls(nx, ny, nu=RECIPE_NU, dt=recipe_dt(nx, ny), kappa=RECIPE_KAPPA, **kw)
    m.set_vort(vort)
    m.set_tracer(tracer)
    if source is not None:
        m.src = np.asarray(source).astype(np.float64)
    return m


def float32_errors(nx, ny, vort, tracer, source, steps, ref):
    """(tracer, vorticity) rel L2 against the float64 model `ref` of the ordinary float32 evaluation of the same system: torch's
    float32 / complex64 FFTs on the CPU, the formula order of TracerModel64.  What a correct float32 engine can be expected to reach."""
    import torch
    f, c64 = torch.float32, torch.complex64
    ikx, iky = torch.from_numpy(ref.ikx).to(c64), torch.from_numpy(ref.iky).to(c64)
    lap, lapi, mask = (torch.from_numpy(a).to(f) for a in (ref.lap, ref.lapi, ref.mask))
    src = torch.from_numpy(np.asarray(source, dtype=np.float32))
    nu, kappa, dt = float(np.float32(ref.nu)), float(np.float32(ref.kappa)), float(np.float32(ref.dt))

    def c2r(a):
        return torch.fft.irfft2(a, s=(nx, ny))

    def tend(vc, cc):
        psi = vc / lapi
        u, v = -c2r(iky * psi), c2r(ikx * psi)
        tv = -u * c2r(ikx * vc) - v * c2r(iky * vc) + src
        tc = -u * c2r(ikx * cc) - v * c2r(iky * cc)
        return (torch.fft.rfft2(tv) + vc * lap * nu) * mask, (torch.fft.rfft2(tc) + cc * lap * kappa) * mask
    vc, cc = torch.fft.rfft2(torch.from_numpy(np.asarray(vort, dtype=np.float32))), torch.fft.rfft2(torch.from_numpy(np.asarray(tracer, dtype=np.float32)))
    for _ in range(steps):
        k1, l1 = tend(vc, cc)
        k2, l2 = tend(vc + k1 * (dt / 2), cc + l1 * (dt / 2))
        k3, l3 = tend(vc + k2 * (dt / 2), cc + l2 * (dt / 2))
        k4, l4 = tend(vc + k3 * dt, cc + l3 * dt)
        vc, cc = vc + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6, cc + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6
    return rel_l2(c2r(cc).numpy(), ref.tracer()), rel_l2(c2r(vc).numpy(), ref.vort())


def masked_share(m):
    """the share of the tracer's L2 norm that lies outside the dealiasing circle (Parseval over the half spectrum)"""
    w = np.full(m.cc.shape, 2.0)
    w[:, 0] = 1.0
    if m.ny % 2 == 0:
        w[:, -1] = 1.0
    p = w * np.abs(m.cc) ** 2
    return float(np.sqrt((p * (1 - m.mask)).sum() / p.sum()))


def cellular_flow(nx, ny, lx=600000.0, ly=600000.0, amp=1.0e6, mx=2, my=3):
    """psi = A cos(2 pi mx x / Lx) cos(2 pi my y / Ly) on the grid and zeta = laplacian(psi), analytically; k2 = the squared wavenumber.
    J(psi, f(psi)) = 0: the flow is steady and a tracer c = psi is only diffused."""
    x = np.arange(nx)[:, None] * (lx / nx)
    y = np.arange(ny)[None, :] * (ly / ny)
    kx, ky = 2 * np.pi * mx / lx, 2 * np.pi * my / ly
    psi = amp * np.cos(kx * x) * np.cos(ky * y)
    k2 = kx * kx + ky * ky
    return psi, -k2 * psi, k2


def rk4_factor(z):
    """the amplification factor of one RK4 step of y' = lambda y, z = lambda dt"""
    return 1 + z + z * z / 2 + z ** 3 / 6 + z ** 4 / 24
