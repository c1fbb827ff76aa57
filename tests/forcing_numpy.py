"""float64 numpy restatement of the split stage that follows every RK4 step once forcing is set (fb_model_set_forcing): stochastic forcing
in a wavenumber ring, linear drag and hyperviscosity,

    zeta_new = D zeta + Delta_n                     for every stored mode inside the dealiasing circle (a masked mode keeps its bits),
    D        = fl32( exp(-(mu + nu_p K^2p) dt) ),   K^2 = -laplacian_coe (the float32 table value, ref_numpy.tables),
    Delta_n  = fl32( GRIDS sqrt(2 eps dt K^2 / N_ring) e^{i theta} ) on the ring | sqrt(K^2) - k_f | <= dk, 0 elsewhere,
    theta    = 2 pi u / 2^32,  u = word 0 of Philox4x32-10 with counter (i, j, n_lo, n_hi) and key (seed_lo, seed_hi),

n the forcing clock (split stages applied since the forcing was set).  On the lines j = 0 and j = ny/2 a mode with i > nx/2 takes the
conjugate of mode (nx - i, j), so the field stays real; the four self-conjugate modes are never forced.  N_ring counts the ring's
modes over the FULL spectrum (a stored mode with 0 < j < ny/2 twice), so one stage from rest adds eps dt of energy exactly,
E = sum over the full spectrum of |zeta / GRIDS|^2 / (2 K^2).  The tangent of the split system: every perturbation's base times D inside
the circle, no increment (the forcing is additive).

Philox4x32-10 is Salmon, Moraes, Dror and Shaw (2011), "Parallel random numbers: as easy as 1, 2, 3", transcribed here from the
paper's description: ten rounds, multipliers D2511F53 and CD9E8D57, Weyl constants 9E3779B9 and BB67AE85.

Also the cases of the GPU path matrix with the two probe shifts that make its parity bar decisive (a forcing without the conjugate
rule on j = 0; a forcing whose clock stays at 0).  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

import adjoint_numpy as A
import tangent_numpy as G
import tracer_numpy as T
from ref_numpy import rel_l2, tables

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
# (counter, key, output) of the issue's table
PHILOX_KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32(counter, key, rounds=10):
    """the four output words (uint64 arrays holding 32-bit values) for arrays or scalars of the four counter and two key words"""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in np.broadcast_arrays(*counter)]
    k = [np.asarray(x, dtype=np.uint64) & M32 for x in key]
    for _ in range(rounds):
        p0, p1 = PHILOX_M[0] * c[0], PHILOX_M[1] * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + PHILOX_W[0]) & M32, (k[1] + PHILOX_W[1]) & M32]
    return c


class Forcing:
    """the split stage on an nx x ny grid: D, the ring, N_ring, the increment and the budget's two quadratic forms"""

    def __init__(self, nx, ny, dt, rate=0.0, k=None, width=None, seed=0, drag=0.0, hyper_nu=0.0, hyper_order=1, lx=600000.0, ly=600000.0):
        self.nx, self.ny, self.hy = nx, ny, ny // 2 + 1
        self.grids = float(nx) * ny
        _, _, lap, _, mask = tables(nx, ny, lx, ly)
        self.K2 = -lap.astype(np.float64)
        self.live = mask != 0
        self.dt = float(np.float32(dt))
        self.rate, self.seed = float(rate), int(seed)
        self.mu, self.nu_p, self.p = float(drag), float(hyper_nu), int(hyper_order)
        if not 1 <= self.p <= 8:
            raise ValueError("hyper_order outside [1, 8]")
        with np.errstate(over="ignore"):
            self.D = np.exp(-(self.mu + self.nu_p * self.K2 ** self.p) * self.dt).astype(np.float32).astype(np.float64)
        self.w = np.full((nx, self.hy), 2.0)
        self.w[:, 0] = 1.0
        self.w[:, -1] = 1.0
        self.ring = np.zeros((nx, self.hy), dtype=bool)
        self.n_ring = 0
        if self.rate > 0.0:
            if not (k - width > 0.0):
                raise ValueError("k - width <= 0")
            self.ring = np.abs(np.sqrt(self.K2) - k) <= width
            for i in (0, nx // 2):
                for j in (0, ny // 2):
                    self.ring[i, j] = False
            if not self.ring.any():
                raise ValueError("the ring is empty")
            if (self.ring & ~self.live).any():
                raise ValueError("the ring holds a masked mode")
            self.n_ring = int(self.w[self.ring].sum())

    def increment(self, n, conj_rule=True, round32=True):
        """Delta_n, complex128 [nx, hy] holding float32 values (round32=False: before that rounding); conj_rule=False: the broken
        forcing of the first probe"""
        out = np.zeros((self.nx, self.hy), dtype=np.complex128)
        if self.rate <= 0.0:
            return out
        i, j = np.nonzero(self.ring)
        mirror = ((j == 0) | (j == self.ny // 2)) & (i > self.nx // 2) & bool(conj_rule)
        src = np.where(mirror, self.nx - i, i)
        n = int(n)
        u = philox4x32((src, j, n & 0xFFFFFFFF, n >> 32), (self.seed & 0xFFFFFFFF, self.seed >> 32))[0]
        theta = 2.0 * np.pi * u.astype(np.float64) / 4294967296.0
        amp = self.grids * np.sqrt(2.0 * self.rate * self.dt * self.K2[i, j] / self.n_ring)
        re, im = amp * np.cos(theta), amp * np.sin(theta)
        if round32:
            re, im = re.astype(np.float32), im.astype(np.float32)
        out[i, j] = re.astype(np.float64) + 1j * np.where(mirror, -im, im).astype(np.float64)
        return out

    def decay(self, zc):
        """D zeta inside the circle, the masked modes as they are"""
        return np.where(self.live, self.D * zc, zc)

    def energy(self, zc):
        k2 = np.where(self.K2 > 0.0, self.K2, 1.0)
        return float((self.w * np.abs(zc / self.grids) ** 2 / (2.0 * k2) * (self.K2 > 0.0)).sum())

    def enstrophy(self, zc):
        return float((0.5 * self.w * np.abs(zc / self.grids) ** 2).sum())


class ForcedModel64(G.TangentModel64):
    """ref_numpy.Model64 (+ the perturbation of tangent_numpy.TangentModel64, if one is set) with the split stage after every step; the
    budget as fb_model_forcing_budget returns it.  conj_rule=False / frozen_clock=True: the two probes."""

    def __init__(self, nx, ny, nu=6.5, dt=3.0, conj_rule=True, frozen_clock=False, **forcing):
        super().__init__(nx, ny, nu=nu, dt=dt)
        self.f = Forcing(nx, ny, dt, **forcing)
        self.conj_rule, self.frozen_clock = conj_rule, frozen_clock
        self.clock = 0
        self.dE_forc = self.dE_diss = self.dZ_forc = self.dZ_diss = 0.0

    def tangent_tendency(self, vc, dc):
        return None if dc is None else super().tangent_tendency(vc, dc)

    def step(self, n=1):
        f = self.f
        for _ in range(n):
            if self.dc is None:
                G.Model64.step(self, 1)
            else:
                super().step(1)
            z0 = self.vc
            z1 = f.decay(z0)
            z2 = z1 + f.increment(0 if self.frozen_clock else self.clock, self.conj_rule)
            self.dE_diss += f.energy(z1) - f.energy(z0)
            self.dE_forc += f.energy(z2) - f.energy(z1)
            self.dZ_diss += f.enstrophy(z1) - f.enstrophy(z0)
            self.dZ_forc += f.enstrophy(z2) - f.enstrophy(z1)
            self.vc = z2
            if self.dc is not None:
                self.dc = f.decay(self.dc)
            self.clock += 1

    def budget(self):
        return {"clock": self.clock, "dE_forc": self.dE_forc, "dE_diss": self.dE_diss, "dZ_forc": self.dZ_forc, "dZ_diss": self.dZ_diss,
                "n_ring": self.f.n_ring}


K1 = 2.0 * np.pi / 600000.0          # the box's fundamental wavenumber [rad/m]
SHIFT_BAR = T.SHIFT_BAR
STEPS = 5
SEED = 0x1234567887654321            # both key words in use
DRAG = 1.0e-2                        # [1/s]: 3 % per step of 3 s
HYPER_ORDER = 4


def hyper_nu(nx, ny, dt):
    """nu_4 that damps the edge of the dealiasing circle by exp(-0.3) per step"""
    dxw, dyw = int(np.ceil(nx / 3.0)), int(np.ceil(ny / 3.0))
    kmax2 = float(dxw * dxw + dyw * dyw) * K1 * K1
    return 0.3 / (float(np.float32(dt)) * kmax2 ** HYPER_ORDER)


# The GPU path matrix: the six grids of adjoint_numpy.PATH_CASES, 5 steps each, on the noisy, never-dealiased inputs of tangent_numpy,
# with forcing, drag and nabla^8 hyperviscosity all on.  The ring: k_f = 33 k1 with a half width of 2 k1, which on the strips of 64
# columns holds modes of the live Nyquist column j = 32 as well as of j = 0; rate [m^2 s^-3] chosen so that five increments are a
# per-cent-size part of the noisy vorticity.  shift_conj / shift_clock: the shift of the float64 vorticity, rel L2, when the forcing
# omits the conjugate rule on j = 0 and j = ny/2, and when its clock stays at 0 (measured on the CPU; tests/test_forcing_cpu.py
# computes and asserts them, against SHIFT_BAR = 1e-4, ten times the parity bar).
ForcingCase = namedtuple("ForcingCase", "nx ny steps rate k width shift_conj shift_clock")
RATE, RING_K, RING_WIDTH = 2.0, 33.0 * K1, 2.0 * K1
SHIFTS = {(256, 256): (0.00448, 0.214), (192, 192): (0.00578, 0.213), (3072, 64): (0.00984, 0.119), (1024, 64): (0.0179, 0.208),
          (4096, 64): (0.0105, 0.103), (64, 4096): (0.00169, 0.102)}
PATH_CASES = tuple(ForcingCase(a.nx, a.ny, STEPS, RATE, RING_K, RING_WIDTH, *SHIFTS[(a.nx, a.ny)]) for a in A.PATH_CASES)


def case_of(nx, ny):
    return [k for k in PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]


def case_forcing(case):
    """the keyword arguments of Model.set_forcing and of ForcedModel64 for a case of the matrix"""
    dt = T.recipe_dt(case.nx, case.ny)
    return dict(rate=case.rate, k=case.k, width=case.width, seed=SEED, drag=DRAG, hyper_nu=hyper_nu(case.nx, case.ny, dt), hyper_order=HYPER_ORDER)


def recipe_model(case, vort, dz, source, **kw):
    m = ForcedModel64(case.nx, case.ny, nu=G.NU, dt=T.recipe_dt(case.nx, case.ny), **case_forcing(case), **kw)
    m.set_vort(vort)
    if dz is not None:
        m.set_tangent(dz)
    if source is not None:
        m.src = np.asarray(source).astype(np.float64)
    return m


def probe_shifts(case, vort, source, ref):
    """(shift_conj, shift_clock) of the vorticity against the stepped reference `ref`"""
    out = []
    for kw in ({"conj_rule": False}, {"frozen_clock": True}):
        p = recipe_model(case, vort, None, source, **kw)
        p.step(case.steps)
        out.append(rel_l2(p.vort(), ref.vort()))
    return tuple(out)
