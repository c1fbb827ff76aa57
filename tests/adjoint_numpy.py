"""float64 numpy reference of the adjoint model: tangent_numpy.TangentModel64 extended by a tape of the stage states of every step taken
while recording, an adjoint variable lam, and the backward sweep that applies the transpose of the discrete tangent step, newest
step first.  With <a, b> the sum over the grid of a b, M the dealiasing mask and mu~ = M mu, the transpose of the stage tendency
(tangent_numpy.TangentModel64.tangent_tendency) about the stage state zeta is

    L^T mu = gradx(u mu~) + grady(v mu~) + invertLaplacian( gradx(zeta_y mu~) - grady(zeta_x mu~) ) + nu laplacian(mu~),

the products in physical space, the result NOT masked again, and one step backward is

    k4b = dt/6 lam, k3b = k2b = dt/3 lam, k1b = dt/6 lam, acc = lam
    a = L3^T k4b: acc += a, k3b += dt a;  a = L2^T k3b: acc += a, k2b += dt/2 a;  a = L1^T k2b: acc += a, k1b += dt/2 a;  acc += L0^T k1b

(tests/test_adjoint_cpu.py: the dot-product identity against TangentModel64 holds to 1e-12).  In the spectral inner product with the
Hermitian weights the transpose of c2r is r2c and the reverse, that of a multiplier its complex conjugate: so the whole sweep stays
in half spectra, r2c on the way in, c2r on the way out.  Also the case table of the GPU path matrix, the probe that makes its parity
bar decisive (ProbeAdjoint64), the float32 restatement on the CPU and the float64 power iteration.  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

import tangent_numpy as G
import tracer_numpy as T
from ref_numpy import rel_l2


class AdjointModel64(G.TangentModel64):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.depth, self.tape, self.lc = 0, [], None

    # ---- the tape ----
    def record_adjoint(self, depth):
        if depth < 0:
            raise ValueError("depth < 0")
        self.depth, self.tape = int(depth), []

    def adjoint_recorded(self):
        return len(self.tape)

    def set_vort(self, vort):
        super().set_vort(vort)
        self.tape = []

    def stage_states(self, v0, v1, v2, v3):
        """what a step records (ProbeAdjoint64 overrides it)"""
        return (v0, v1, v2, v3)

    def step(self, n=1):
        if self.depth and len(self.tape) + n > self.depth:
            raise ValueError("the step would overrun the tape")
        dt = self.dt
        for _ in range(n):
            v0, d0 = self.vc, self.dc
            tl = d0 is not None
            k1 = self.tendency(v0)
            v1 = v0 + k1 * (dt / 2)
            k2 = self.tendency(v1)
            v2 = v0 + k2 * (dt / 2)
            k3 = self.tendency(v2)
            v3 = v0 + k3 * dt
            k4 = self.tendency(v3)
            if tl:
                l1 = self.tangent_tendency(v0, d0)
                l2 = self.stage_tangent_tendency(v1, d0 + l1 * (dt / 2))
                l3 = self.stage_tangent_tendency(v2, d0 + l2 * (dt / 2))
                l4 = self.stage_tangent_tendency(v3, d0 + l3 * dt)
                self.dc = d0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            if self.depth:
                self.tape.append(self.stage_states(v0, v1, v2, v3))

    # ---- the adjoint variable and the sweep ----
    def set_adjoint(self, lam):
        self.lc = None if lam is None else np.fft.rfft2(np.asarray(lam).astype(np.float64))

    def adjoint(self):
        return self._c2r(self.lc)

    def adjoint_tendency(self, vc, mu):
        mt = mu * self.mask
        m = self._c2r(mt)
        psi = vc / self.lapi
        u, v = -self._c2r(self.iky * psi), self._c2r(self.ikx * psi)
        zx, zy = self._c2r(self.ikx * vc), self._c2r(self.iky * vc)
        r = np.fft.rfft2
        return self.ikx * r(u * m) + self.iky * r(v * m) + (self.ikx * r(zy * m) - self.iky * r(zx * m)) / self.lapi + mt * self.lap * self.nu

    def adjoint_back(self, n=1):
        if n < 0 or n > len(self.tape):
            raise ValueError("more steps than are recorded")
        dt = self.dt
        for _ in range(n):
            v0, v1, v2, v3 = self.tape.pop()
            lam = self.lc
            a = self.adjoint_tendency(v3, lam * (dt / 6))
            acc = lam + a
            a = self.adjoint_tendency(v2, lam * (dt / 3) + a * dt)
            acc = acc + a
            a = self.adjoint_tendency(v1, lam * (dt / 3) + a * (dt / 2))
            acc = acc + a
            a = self.adjoint_tendency(v0, lam * (dt / 6) + a * (dt / 2))
            self.lc = acc + a


class ProbeAdjoint64(AdjointModel64):
    """The sensitivity probe: every stage of a step is linearised about the step's base state, as an engine would that recorded only
    the state a step starts from (or read slot 0 of the tape at every stage)."""

    def stage_states(self, v0, v1, v2, v3):
        return (v0, v0, v0, v0)


AdjointCase = namedtuple("AdjointCase", "nx ny vort_noise steps shift f32 f32_dot what")
SHIFT_BAR = G.SHIFT_BAR
F32_BAR = G.F32_BAR
SEED = G.SEED + 1
STEPS = 5
# The GPU path matrix: the rows of tangent_numpy.PATH_CASES without a fixture that the three branches of stage_vstate and the row and
# column dispatch need, 5 steps each.  shift: the shift of the float64 lam_0 under ProbeAdjoint64; f32: the float32 torch restatement's
# error of lam_0 against float64; f32_dot: its dot-product residual |<T d, lam> - <d, T^T lam>| / (|T d| |lam|) (all measured on the
# CPU, asserted in tests/test_adjoint_cpu.py to 10 % for the shift and as upper bounds for the other two).
PATH_CASES = (
    AdjointCase(256, 256, 3e-2, STEPS, 0.0306, 3e-07, 1.7e-10, "state in the 3-pass layout, read in place: k_adjoint_merge"),
    AdjointCase(192, 192, 3e-2, STEPS, 0.0248, 2.62e-07, 3.05e-10, "k_row3; N1 = 24, N2 = 8; k_adjoint_merge"),
    AdjointCase(3072, 64, 3e-2, STEPS, 0.0696, 3.36e-07, 9.66e-10, "N1 = 24 with tile-major state: k_tracer_vstate_tm"),
    AdjointCase(1024, 64, 3e-2, STEPS, 0.1075, 4.7e-07, 1.65e-09, "k_tracer_vstate_tm at N2 = 32"),
    AdjointCase(4096, 64, 3e-2, STEPS, 0.0592, 3.84e-07, 3.42e-10, "tile-major, N1 = N2 = 64; live Nyquist column"),
    AdjointCase(64, 4096, 3e-2, STEPS, 0.0429, 3.65e-07, 3.77e-10, "k_rowq's grid class; live Nyquist row"),
)
# the bar of the dot-product identity on the GPU: 4 x the largest f32_dot of the table (the factor: the GPU's other summation order)
DOT_BAR = 4 * max(k.f32_dot for k in PATH_CASES)


def case_of(nx, ny):
    return [k for k in PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]


def adjoint_inputs(nx, ny, vort_noise, make_field=None):
    """(vort, dz, source, lam), float32: tangent_numpy.tangent_inputs and lam as white noise, never dealiased, of the vorticity's rms"""
    vort, dz, src = G.tangent_inputs(nx, ny, vort_noise, make_field=make_field)
    lam = np.random.default_rng(SEED).standard_normal((nx, ny)) * np.sqrt(np.mean(vort.astype(np.float64) ** 2))
    return vort, dz, src, lam.astype(np.float32)


def recipe_model(nx, ny, vort, dz, source, cls=AdjointModel64, **kw):
    return G.recipe_model(nx, ny, vort, dz, source, cls=cls, **kw)


def run_case(nx, ny, vort, dz, source, lam, steps, cls=AdjointModel64):
    """record, step, set lam, sweep back: the stepped model (adjoint(): lam_0, tangent(): T dz, vort())"""
    m = recipe_model(nx, ny, vort, dz, source, cls=cls)
    m.record_adjoint(steps)
    m.step(steps)
    m.set_adjoint(lam)
    m.adjoint_back(steps)
    return m


def dot_residual(td, lam, d, tl):
    """|<T d, lam> - <d, T^T lam>| / (|T d| |lam|) in float64"""
    td, lam, d, tl = (np.asarray(a, dtype=np.float64) for a in (td, lam, d, tl))
    return float(abs(np.vdot(td, lam) - np.vdot(d, tl)) / (np.linalg.norm(td) * np.linalg.norm(lam)))


class Float32Model:
    """The ordinary float32 evaluation of the same system (torch's float32 / complex64 FFTs on the CPU, the formula order of
    AdjointModel64): what a correct float32 engine can reach.  Fields in and out as numpy arrays."""

    def __init__(self, ref, source=None):
        import torch
        self.t = torch
        f, c64 = torch.float32, torch.complex64
        self.nx, self.ny = ref.nx, ref.ny
        self.ikx, self.iky = torch.from_numpy(ref.ikx).to(c64), torch.from_numpy(ref.iky).to(c64)
        self.lap, self.lapi, self.mask = (torch.from_numpy(a).to(f) for a in (ref.lap, ref.lapi, ref.mask))
        self.src = torch.zeros((self.nx, self.ny), dtype=f) if source is None else torch.from_numpy(np.asarray(source, dtype=np.float32))
        self.nu, self.dt = float(np.float32(ref.nu)), float(np.float32(ref.dt))
        self.vc = self.dc = self.lc = None
        self.depth, self.tape = 0, []

    def _r2c(self, a):
        return self.t.fft.rfft2(self.t.from_numpy(np.asarray(a, dtype=np.float32)))

    def _c2r(self, a):
        return self.t.fft.irfft2(a, s=(self.nx, self.ny))

    def set_vort(self, v): self.vc = self._r2c(v); self.tape = []
    def set_spectrum(self, vc): self.vc = vc.clone(); self.tape = []
    def spectrum(self): return self.vc.clone()
    def set_tangent(self, d): self.dc = None if d is None else self._r2c(d)
    def set_adjoint(self, lam): self.lc = None if lam is None else self._r2c(lam)
    def record_adjoint(self, depth): self.depth, self.tape = int(depth), []
    def vort(self): return self._c2r(self.vc).numpy()
    def tangent(self): return self._c2r(self.dc).numpy()
    def adjoint(self): return self._c2r(self.lc).numpy()

    def _tend(self, vc, dc):
        c2r, ikx, iky = self._c2r, self.ikx, self.iky
        psi = vc / self.lapi
        u, v, zx, zy = -c2r(iky * psi), c2r(ikx * psi), c2r(ikx * vc), c2r(iky * vc)
        kv = (self.t.fft.rfft2(-u * zx - v * zy + self.src) + vc * self.lap * self.nu) * self.mask
        if dc is None:
            return kv, None
        dpsi = dc / self.lapi
        du, dv = -c2r(iky * dpsi), c2r(ikx * dpsi)
        td = -u * c2r(ikx * dc) - v * c2r(iky * dc) - du * zx - dv * zy
        return kv, (self.t.fft.rfft2(td) + dc * self.lap * self.nu) * self.mask

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, d0 = self.vc, self.dc
            tl = d0 is not None
            k1, l1 = self._tend(v0, d0)
            v1 = v0 + k1 * (dt / 2)
            k2, l2 = self._tend(v1, d0 + l1 * (dt / 2) if tl else None)
            v2 = v0 + k2 * (dt / 2)
            k3, l3 = self._tend(v2, d0 + l2 * (dt / 2) if tl else None)
            v3 = v0 + k3 * dt
            k4, l4 = self._tend(v3, d0 + l3 * dt if tl else None)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            if tl:
                self.dc = d0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6
            if self.depth:
                self.tape.append((v0, v1, v2, v3))

    def _atend(self, vc, mu):
        c2r, ikx, iky, r = self._c2r, self.ikx, self.iky, self.t.fft.rfft2
        mt = mu * self.mask
        m = c2r(mt)
        psi = vc / self.lapi
        u, v, zx, zy = -c2r(iky * psi), c2r(ikx * psi), c2r(ikx * vc), c2r(iky * vc)
        return ikx * r(u * m) + iky * r(v * m) + (ikx * r(zy * m) - iky * r(zx * m)) / self.lapi + mt * self.lap * self.nu

    def adjoint_back(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, v1, v2, v3 = self.tape.pop()
            lam = self.lc
            a = self._atend(v3, lam * (dt / 6))
            acc = lam + a
            a = self._atend(v2, lam * (dt / 3) + a * dt)
            acc = acc + a
            a = self._atend(v1, lam * (dt / 3) + a * (dt / 2))
            acc = acc + a
            a = self._atend(v0, lam * (dt / 6) + a * (dt / 2))
            self.lc = acc + a


def float32_figures(nx, ny, vort, dz, source, lam, steps, ref):
    """(error of lam_0, dot-product residual) of the float32 restatement; ref: the float64 model of run_case"""
    f = Float32Model(ref, source)
    f.set_vort(vort)
    f.set_tangent(dz)
    f.record_adjoint(steps)
    f.step(steps)
    f.set_adjoint(lam)
    f.adjoint_back(steps)
    return rel_l2(f.adjoint(), ref.adjoint()), dot_residual(f.tangent(), lam, dz, f.adjoint())


def singular_values(model, spectrum0, steps, iters, start, norm=None):
    """Power iteration on T^T T in the L2 norm on anything with the methods of binding.Model (a float64 or float32 model here): per
    iteration the base state is restored, the tangent set to the unit vector v, `steps` steps taken with recording on, lam = T v set
    and swept back; sigma = |T v|, v <- T^T T v normalised.  Returns (the sigmas, the final v)."""
    v = np.asarray(start, dtype=np.float64)
    v = v / np.linalg.norm(v)
    sig = []
    for _ in range(iters):
        model.set_spectrum(spectrum0)
        model.set_tangent(v)
        model.record_adjoint(steps)
        model.step(steps)
        w = np.asarray(model.tangent(), dtype=np.float64)
        sig.append(float(np.linalg.norm(w)))
        model.set_adjoint(w)
        model.adjoint_back(steps)
        v = np.asarray(model.adjoint(), dtype=np.float64)
        v = v / np.linalg.norm(v)
    model.record_adjoint(0)
    return sig, v


def _spectrum_methods(cls):
    cls.spectrum = lambda self: self.vc.copy()

    def set_spectrum(self, vc):
        self.vc = np.array(vc, dtype=np.complex128)
        self.tape = []
    cls.set_spectrum = set_spectrum


_spectrum_methods(AdjointModel64)

# singular_values at 256^2, 3 steps, 4 iterations from SV_START (the tangent inputs' dz): what the float32 restatement holds against
# float64, the largest relative error of a singular value over the iterations (tests/test_adjoint_cpu.py asserts it as an upper bound)
SV_N, SV_STEPS, SV_ITERS = 256, 3, 4
SV_F32 = 2.4e-07
SV_BAR = 1e-4
