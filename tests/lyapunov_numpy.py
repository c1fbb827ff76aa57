"""float64 numpy reference of the tangent subspace: M perturbations carried along ONE base trajectory by tangent_numpy.TangentModel64's
linearised step, the inner product whose <a, a> is tangent_numpy.spectrum_norm, modified Gram-Schmidt in that inner product (mgs), and
its float32-storage restatement (mgs_f32: what the engine's tangent_qr does to its float32 half spectra, csrc/fb_tangent.h).  Also the
inputs of the subspace's tests (subspace_inputs) and the figure the GPU's orthonormality bar is derived from (MGS_F32_DEFECT).
Perturbations are handled as half spectra (unnormalised, as rfft2 leaves them).  Used ONLY by tests."""
import numpy as np

import tangent_numpy as G
import tracer_numpy as T

KINDS = ("enstrophy", "energy")


class SubspaceModel64(G.TangentModel64):
    """TangentModel64 with a list of perturbations self.dcs in the place of the one self.dc"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.dcs = []

    def set_tangents(self, fields):
        self.dcs = [np.fft.rfft2(np.asarray(f).astype(np.float64)) for f in fields]

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0 = self.vc
            k1 = self.tendency(v0)
            v1 = v0 + k1 * (dt / 2)
            k2 = self.tendency(v1)
            v2 = v0 + k2 * (dt / 2)
            k3 = self.tendency(v2)
            v3 = v0 + k3 * dt
            k4 = self.tendency(v3)
            out = []
            for d0 in self.dcs:                                  # the formula order of TangentModel64.step, per perturbation
                l1 = self.tangent_tendency(v0, d0)
                l2 = self.stage_tangent_tendency(v1, d0 + l1 * (dt / 2))
                l3 = self.stage_tangent_tendency(v2, d0 + l2 * (dt / 2))
                l4 = self.stage_tangent_tendency(v3, d0 + l3 * dt)
                out.append(d0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.dcs = out

    def tangents(self):
        return np.array([self._c2r(d) for d in self.dcs])


def spectra(fields):
    return [np.fft.rfft2(np.asarray(f).astype(np.float64)) for f in fields]


def weights(m, kind):
    """w q of the inner product per mode of the half spectrum, the factor 1 / (2 GRIDS^2) included: spectrum_norm's"""
    w = np.full((m.nx, m.ny // 2 + 1), 2.0)
    w[:, 0] = 1.0
    w[:, -1] = 1.0
    if kind == "energy":
        k2 = (m.ikx.imag ** 2 + m.iky.imag ** 2) / m.lapi ** 2
        k2[0, 0] = 0.0
        w = w * k2
    elif kind != "enstrophy":
        raise ValueError(kind)
    return w * (0.5 / (float(m.nx) * m.ny) ** 2)


def inner(m, a, b, kind="enstrophy", w=None):
    """<a, b> of two half spectra in float64: the sum of w q Re(a conj(b)) / (2 GRIDS^2); inner(m, a, a, kind) is spectrum_norm"""
    w = weights(m, kind) if w is None else w
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    return float((w * (a.real * b.real + a.imag * b.imag)).sum())


def gram(m, V, kind="enstrophy"):
    w = weights(m, kind)
    return np.array([[inner(m, a, b, kind, w) for b in V] for a in V])


def condition(m, V, kind="enstrophy"):
    """the square root of the ratio of the extreme eigenvalues of the float64 Gram matrix"""
    ev = np.linalg.eigvalsh(gram(m, V, kind))
    return float(np.sqrt(ev[-1] / ev[0]))


def mgs(m, V, kind="enstrophy"):
    """(Q, R): modified Gram-Schmidt on the list of half spectra V in vector order, in float64; V_j = sum over i <= j of R[i, j] Q_i"""
    w = weights(m, kind)
    M = len(V)
    Q, R = [np.array(v, dtype=np.complex128) for v in V], np.zeros((M, M))
    for j in range(M):
        for i in range(j):
            R[i, j] = inner(m, Q[i], Q[j], kind, w)
            Q[j] = Q[j] - R[i, j] * Q[i]
        R[j, j] = np.sqrt(inner(m, Q[j], Q[j], kind, w))
        Q[j] = Q[j] / R[j, j]
    return Q, R


def mgs_f32(m, V, kind="enstrophy"):
    """mgs as the engine runs it: the half spectra stored as complex64; every sum and coefficient in float64; each element formed in
    float64 and rounded once to float32 per axpy and once per scaling.  Returns (Q as complex64 arrays, R float64)."""
    w = weights(m, kind)
    M = len(V)
    Q, R = [np.array(v).astype(np.complex64) for v in V], np.zeros((M, M))
    f64 = lambda a: a.view(np.float32).astype(np.float64)       # noqa: E731 -- (re, im interleaved) widened
    c64 = lambda a: a.astype(np.float32).view(np.complex64)     # noqa: E731 -- rounded once per component
    for j in range(M):
        for i in range(j):
            R[i, j] = inner(m, Q[i], Q[j], kind, w)
            Q[j] = c64(f64(Q[j]) - R[i, j] * f64(Q[i]))
        R[j, j] = np.sqrt(inner(m, Q[j], Q[j], kind, w))
        Q[j] = c64(f64(Q[j]) / R[j, j])
    return Q, R


def defect(m, Q, kind="enstrophy"):
    """max |Q^T W Q - I|"""
    return float(np.abs(gram(m, Q, kind) - np.eye(len(Q))).max())


# The grids of the QR checks, CPU and GPU, and the largest orthonormality defect max |Q^T W Q - I| that mgs_f32 leaves on
# subspace_inputs over these grids and both kinds (measured on the CPU: tests/test_lyapunov_cpu.py prints every figure and asserts
# that none exceeds this): enstrophy 5.7e-9 (192^2) to 9.2e-8 (64 x 4096), energy 2.1e-8 (1024 x 64) to 2.41e-7 (256^2).  The GPU's
# bar is 4 times this (tests/test_gpu_lyapunov.py), fixed before the GPU ran.
QR_GRIDS = ((64, 64), (256, 256), (192, 192), (1024, 64), (64, 4096))
MGS_F32_DEFECT = 2.5e-7
NOISE = G.PATH_CASES[0].vort_noise


def _scaled(shape, vort, seed):
    """tangent_inputs' recipe for a perturbation from a shape: white noise of DZ_NOISE of its maximum, rms DZ_RMS of the vorticity's"""
    d = shape + G.DZ_NOISE * np.abs(shape).max() * np.random.default_rng(seed).standard_normal(shape.shape)
    return d * (G.DZ_RMS * np.sqrt(np.mean(vort.astype(np.float64) ** 2)) / np.sqrt(np.mean(d ** 2)))


def subspace_inputs(nx, ny, vort_noise=NOISE, make_field=None):
    """(vort, W, source): vort and source of tangent_numpy.tangent_inputs and three perturbations W [3, nx, ny] float32 that are
    neither orthogonal nor nearly dependent: with u_0 tangent_inputs' dz, u_1 and u_2 built by its recipe from the centred y
    difference of the offset gaussian and from the gaussian itself (noise seeds SEED + 1, SEED + 2),
        w_0 = u_0,  w_1 = u_0 + 0.3 u_1,  w_2 = u_0 - u_1 + 0.2 u_2.
    None is dealiased: each has state in every masked mode."""
    vort, u0, src = G.tangent_inputs(nx, ny, vort_noise, make_field=make_field)
    g = T.offset_gaussian(nx, ny, make_field).astype(np.float64)
    u0 = u0.astype(np.float64)
    u1 = _scaled((np.roll(g, -1, axis=1) - np.roll(g, 1, axis=1)) / 2, vort, G.SEED + 1)
    u2 = _scaled(g, vort, G.SEED + 2)
    W = np.array([u0, u0 + 0.3 * u1, u0 - u1 + 0.2 * u2]).astype(np.float32)
    return vort, W, src
