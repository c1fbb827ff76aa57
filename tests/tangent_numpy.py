"""float64 numpy reference of the coupled system vorticity + tangent-linear perturbation: ref_numpy.Model64 extended by a perturbation
dz that every RK4 stage advances with the linearisation of the stage's own tendency about the vorticity's state of that stage,

    tend_dz = mask * ( r2c(-u dz_x - v dz_y - du zeta_x - dv zeta_y) + nu * laplacian_coe * dz_c ),
    u = -psi_y, v = psi_x, du = -dpsi_y, dv = dpsi_x,  psi_c = vort_c / laplacian_coe, dpsi_c = dz_c / laplacian_coe ((0, 0): / 1)

in the formula order of ref_numpy.Model64.tendency.  This is the tangent of the DISCRETE step (tests/test_tangent_cpu.py: the Taylor
test).  Also the inputs of the tangent's path matrix (tangent_inputs: state in the masked modes of both fields, and a vorticity source,
which has no term in the tangent), the sensitivity probe that shows those inputs make the parity bar decisive (ProbeTangent64) and the
float64 norms.  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

import tracer_numpy as T
from ref_numpy import Model64, rel_l2


class TangentModel64(Model64):
    def __init__(self, nx, ny, lx=600000.0, ly=600000.0, nu=6.5, dt=3.0):
        super().__init__(nx, ny, lx, ly, nu, dt)
        self.dc = None

    def set_tangent(self, dz):
        self.dc = np.fft.rfft2(np.asarray(dz).astype(np.float64))

    def tangent_tendency(self, vc, dc):
        ld = dc * self.lap
        psi, dpsi = vc / self.lapi, dc / self.lapi
        u, v = -self._c2r(self.iky * psi), self._c2r(self.ikx * psi)
        du, dv = -self._c2r(self.iky * dpsi), self._c2r(self.ikx * dpsi)
        t = -u * self._c2r(self.ikx * dc) - v * self._c2r(self.iky * dc) - du * self._c2r(self.ikx * vc) - dv * self._c2r(self.iky * vc)
        return (np.fft.rfft2(t) + ld * self.nu) * self.mask

    def stage_tangent_tendency(self, vc, dc):
        """the perturbation's tendency at the stages 1 to 3, from the stage states (ProbeTangent64 overrides it)"""
        return self.tangent_tendency(vc, dc)

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, d0 = self.vc, self.dc
            k1, l1 = self.tendency(v0), self.tangent_tendency(v0, d0)
            v1, d1 = v0 + k1 * (dt / 2), d0 + l1 * (dt / 2)
            k2, l2 = self.tendency(v1), self.stage_tangent_tendency(v1, d1)
            v2, d2 = v0 + k2 * (dt / 2), d0 + l2 * (dt / 2)
            k3, l3 = self.tendency(v2), self.stage_tangent_tendency(v2, d2)
            v3, d3 = v0 + k3 * dt, d0 + l3 * dt
            k4, l4 = self.tendency(v3), self.stage_tangent_tendency(v3, d3)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.dc = d0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6

    def tangent(self):
        return self._c2r(self.dc)

    def tangent_norm(self, kind="enstrophy"):
        return spectrum_norm(self, self.dc, kind)


class ProbeTangent64(TangentModel64):
    """The sensitivity probe, as tracer_numpy.ProbeModel64: the PERTURBATION's tendency at the stages 1 to 3 sees the modes outside the
    dealiasing circle as zero, in the vorticity's stage state (blind_vort) or in the perturbation's (blind_tangent).  The engine stores
    a stage state only where a mode can change and reads a masked mode from the base; a kernel that picked the stage array there would
    do what this model does.  The vorticity's own step is untouched."""

    def __init__(self, *args, blind_vort=False, blind_tangent=False, **kw):
        super().__init__(*args, **kw)
        self.blind_vort, self.blind_tangent = bool(blind_vort), bool(blind_tangent)

    def stage_tangent_tendency(self, vc, dc):
        return self.tangent_tendency(vc * self.mask if self.blind_vort else vc, dc * self.mask if self.blind_tangent else dc)


def spectrum_norm(m, dc, kind="enstrophy"):
    """<dz^2> / 2 ("enstrophy") or <|grad dpsi|^2> / 2 ("energy", the (0, 0) mode left out) of a half spectrum (unnormalised, as rfft2
    leaves it) in float64: Hermitian weights 1 in the columns ky = 0 and ky = ny/2, 2 elsewhere; <.> the mean over the grid."""
    w = np.full(dc.shape, 2.0)
    w[:, 0] = 1.0
    w[:, -1] = 1.0
    p = w * np.abs(dc) ** 2
    if kind == "energy":
        k2 = (m.ikx.imag ** 2 + m.iky.imag ** 2) / m.lapi ** 2
        k2[0, 0] = 0.0
        p = p * k2
    elif kind != "enstrophy":
        raise ValueError(kind)
    return float(0.5 * p.sum() / (float(m.nx) * m.ny) ** 2)


SEED = T.RECIPE_SEED + 1
NU = T.RECIPE_NU
DZ_NOISE = 0.2           # white noise of 20 % of the shape's maximum
DZ_RMS = 1e-3            # the perturbation's rms, of the vorticity's

# The path matrix: the ten strip and small grids of tracer_numpy.PATH_CASES with their step counts, and 4096^2 at 2 steps (the
# tracer's row has 3).  One step count differs: 128 x 16384 takes 32 steps, not the tracer's 56, at which the float32 restatement
# reaches 2.9e-6, above F32_BAR (at DZ_NOISE = 5 % its perturbation shift was 5.7e-5, below SHIFT_BAR, too: hence the 20 %).
# shift_vort / shift_tangent: the shift of the float64 perturbation under ProbeTangent64 (measured on the CPU;
# tests/test_tangent_cpu.py asserts them for the live cases, tests/golden/make_tangent_fixtures.py stores them for the others);
# f32: the float32 torch restatement's error of the perturbation against the float64 run.  Both bars: SHIFT_BAR and F32_BAR.
TangentCase = namedtuple("TangentCase", "nx ny vort_noise steps fixture shift_vort shift_tangent f32 what")
SHIFT_BAR = T.SHIFT_BAR
F32_BAR = 2.5e-6
PATH_CASES = (
    TangentCase(256, 256, 3e-2, 5, False, 0.116, 0.0187, 3.5e-07, "masked-mode logic on the plain path: N2 = 16 < 32, state in the 3-pass layout"),
    TangentCase(192, 192, 3e-2, 5, False, 0.128, 0.0249, 2.6e-07, "k_row3; N1 = 24, N2 = 8"),
    TangentCase(3072, 64, 3e-2, 5, False, 0.0394, 0.00359, 4.3e-07, "N1 = 24 with tile-major state, N2 = 128"),
    TangentCase(1024, 64, 3e-2, 5, False, 0.0715, 0.00967, 5.7e-07, "k_tracer_vstate_tm at N2 = 32"),
    TangentCase(4096, 64, 3e-2, 5, False, 0.0349, 0.00289, 5e-07, "tile-major, N1 = N2 = 64; the three-kernel x pass (live Nyquist column)"),
    TangentCase(8192, 64, 3e-2, 12, False, 0.0223, 0.00124, 6.2e-07, "N1 = 128, N2 = 64"),
    TangentCase(16384, 64, 3e-2, 56, True, 0.0112, 0.000415, 2.13e-06, "N1 = N2 = 128"),
    TangentCase(64, 4096, 3e-2, 5, False, 0.0193, 0.0014, 4.2e-07, "k_rowq"),
    TangentCase(64, 8192, 3e-2, 12, False, 0.0137, 0.000689, 5.6e-07, "k_rowh<1>"),
    TangentCase(128, 16384, 3e-2, 32, True, 0.00546, 0.000282, 1.14e-06, "k_rowh<2>"),
    TangentCase(4096, 4096, 3e-2, 2, True, 0.0256, 0.00132, 4.7e-07, "k_col_full<., 1> and k_tracer_vstate_full at nsub = 1; k_rowq"),
)

# the float64 residual of the translation mode at 256^2 (tests/test_tangent_cpu.py measures and asserts it; the GPU test's bar is
# max(1e-5, 10 x this)): dz_0 = gradx(zeta_0) of the noise-free elliptic vortex, TRANSLATION_STEPS steps of 3 s, no source
TRANSLATION_STEPS = 20
TRANSLATION_RESIDUAL = 5.623e-4


def tangent_inputs(nx, ny, vort_noise, make_field=None):
    """The inputs of the tangent's path matrix, float32 fields (vort, dz, source): vort and source are those of
    tracer_numpy.noisy_inputs; dz is the centred x difference of the offset gaussian plus white noise of DZ_NOISE of its maximum,
    NOT dealiased (so dz has state in every masked mode), scaled to an rms of DZ_RMS of the vorticity's.  To be run with
    dt = tracer_numpy.recipe_dt(nx, ny) and nu = NU."""
    vort, _, src = T.noisy_inputs(nx, ny, vort_noise, make_field=make_field)
    g = T.offset_gaussian(nx, ny, make_field).astype(np.float64)
    shape = (np.roll(g, -1, axis=0) - np.roll(g, 1, axis=0)) / 2
    dz = shape + DZ_NOISE * np.abs(shape).max() * np.random.default_rng(SEED).standard_normal((nx, ny))
    dz *= DZ_RMS * np.sqrt(np.mean(vort.astype(np.float64) ** 2)) / np.sqrt(np.mean(dz ** 2))
    return vort, dz.astype(np.float32), src


def recipe_model(nx, ny, vort, dz, source, cls=TangentModel64, **kw):
    m = cls(nx, ny, nu=NU, dt=T.recipe_dt(nx, ny), **kw)
    m.set_vort(vort)
    m.set_tangent(dz)
    if source is not None:
        m.src = np.asarray(source).astype(np.float64)
    return m


def probe_shifts(nx, ny, vort, dz, source, steps, ref):
    """(shift_vort, shift_tangent): the perturbation of the two probe runs against the stepped reference `ref`, rel L2"""
    out = []
    for which in ("blind_vort", "blind_tangent"):
        p = recipe_model(nx, ny, vort, dz, source, cls=ProbeTangent64, **{which: True})
        p.step(steps)
        assert rel_l2(p.vort(), ref.vort()) == 0.0
        out.append(rel_l2(p.tangent(), ref.tangent()))
    return tuple(out)


def float32_errors(nx, ny, vort, dz, source, steps, ref):
    """(perturbation, vorticity) rel L2 against the stepped float64 model `ref` of the ordinary float32 evaluation of the same system:
    torch's float32 / complex64 FFTs on the CPU, the formula order of TangentModel64.  What a correct float32 engine can reach."""
    import torch
    f, c64 = torch.float32, torch.complex64
    ikx, iky = torch.from_numpy(ref.ikx).to(c64), torch.from_numpy(ref.iky).to(c64)
    lap, lapi, mask = (torch.from_numpy(a).to(f) for a in (ref.lap, ref.lapi, ref.mask))
    src = torch.from_numpy(np.asarray(source, dtype=np.float32))
    nu, dt = float(np.float32(ref.nu)), float(np.float32(ref.dt))

    def c2r(a):
        return torch.fft.irfft2(a, s=(nx, ny))

    def tend(vc, dc):
        psi, dpsi = vc / lapi, dc / lapi
        u, v, du, dv = -c2r(iky * psi), c2r(ikx * psi), -c2r(iky * dpsi), c2r(ikx * dpsi)
        zx, zy = c2r(ikx * vc), c2r(iky * vc)
        tv = -u * zx - v * zy + src
        td = -u * c2r(ikx * dc) - v * c2r(iky * dc) - du * zx - dv * zy
        return (torch.fft.rfft2(tv) + vc * lap * nu) * mask, (torch.fft.rfft2(td) + dc * lap * nu) * mask
    vc, dc = torch.fft.rfft2(torch.from_numpy(np.asarray(vort, dtype=np.float32))), torch.fft.rfft2(torch.from_numpy(np.asarray(dz, dtype=np.float32)))
    for _ in range(steps):
        k1, l1 = tend(vc, dc)
        k2, l2 = tend(vc + k1 * (dt / 2), dc + l1 * (dt / 2))
        k3, l3 = tend(vc + k2 * (dt / 2), dc + l2 * (dt / 2))
        k4, l4 = tend(vc + k3 * dt, dc + l3 * dt)
        vc, dc = vc + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6, dc + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6
    return rel_l2(c2r(dc).numpy(), ref.tangent()), rel_l2(c2r(vc).numpy(), ref.vort())
