"""float64 numpy reference of the point observations and of the 4D-Var cost and gradient built on them: adjoint_numpy.AdjointModel64
extended by the observation operator H (a field of the state, zeta, u, v or psi, interpolated to points by
particles_numpy.lagrange4_sample), its transpose H^T (np.add.at with the weights of particles_numpy.lagrange4_axis, then r2c and the
complex conjugate of the kind's spectral multiplier, added into lam), and

    J(z0) = 1/2 sum over the observation sets k of |H_k zeta(step_k) - y_k|^2 / sigma_k^2   (+ 1/2 |z0 - zb|^2 / sigma_b^2),

whose gradient is what the backward sweep leaves in lam when every set's H^T r, r = (h - y) / sigma^2, is added at its own time.  In
the spectral inner product with the Hermitian weights the transpose of c2r is r2c (adjoint_numpy), so H^T w = conj(M) r2c(S^T w) for
H = S c2r M.  Also the float32 torch restatement on the CPU (what a correct float32 engine can reach), the inputs and case tables
of tests/test_gpu_obs.py, and the twin experiment.  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

import adjoint_numpy as A
import particles_numpy as P
from ref_numpy import rel_l2

KINDS = ("vort", "u", "v", "psi")
Obs = namedtuple("Obs", "step kind xy y sigma")             # sigma: None (1), a float or an array of n
LX = LY = 600000.0


def multiplier(ref, kind):
    """the spectral multiplier M of a kind, [nx, ny/2+1] complex: field = c2r(M zeta_c), with the tables of ref (a Model64)"""
    one = np.ones_like(ref.lapi)
    return {"vort": one + 0j, "psi": 1.0 / ref.lapi + 0j, "u": -ref.iky / ref.lapi, "v": ref.ikx / ref.lapi}[kind]


def scatter64(xy, w, nx, ny, lx=LX, ly=LY, terms=False):
    """field[i, j] = sum over the points of w wx_a wy_b, float64, by np.add.at; a point whose position or weight is not finite deposits
    nothing.  terms=True: also the sum of the |contributions| per cell (what the engine's error bound is relative to)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).ravel()
    ok = np.isfinite(xy).all(axis=1) & np.isfinite(w)
    xy, w = xy[ok], w[ok]
    ix, wx = P.lagrange4_axis(xy[:, 0], P.widen(lx) / nx, nx)
    jy, wy = P.lagrange4_axis(xy[:, 1], P.widen(ly) / ny, ny)
    c = w[:, None, None] * (wx[:, :, None] * wy[:, None, :])                # [n, 4, 4]
    cells = (ix[:, :, None] * ny + jy[:, None, :]).ravel()
    f, a = np.zeros(nx * ny), np.zeros(nx * ny)
    np.add.at(f, cells, c.ravel())
    if not terms:
        return f.reshape(nx, ny)
    np.add.at(a, cells, np.abs(c).ravel())
    return f.reshape(nx, ny), a.reshape(nx, ny)


def sample64(field, xy, lx=LX, ly=LY):
    """particles_numpy.lagrange4_sample with NaN where a position is not finite"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ok = np.isfinite(xy).all(axis=1)
    out = np.full(xy.shape[0], np.nan)
    out[ok] = P.lagrange4_sample(field, xy[ok], lx, ly)
    return out


class ObsModel64(A.AdjointModel64):
    """AdjointModel64 with point observations"""

    def set_tangent(self, dz):
        self.dc = None if dz is None else np.fft.rfft2(np.asarray(dz).astype(np.float64))

    def field(self, kind, spec=None):
        return self._c2r(multiplier(self, kind) * (self.vc if spec is None else spec))

    def observe(self, kind, xy):
        return sample64(self.field(kind), xy)

    def observe_tangent(self, kind, xy):
        """H applied to the perturbation of the tangent-linear model"""
        return sample64(self.field(kind, self.dc), xy)

    def scatter(self, w, xy):
        return scatter64(xy, w, self.nx, self.ny)

    def adjoint_add_obs(self, kind, xy, w):
        self.lc = self.lc + np.conj(multiplier(self, kind)) * np.fft.rfft2(self.scatter(w, xy))


def sigma_of(o, n):
    return np.ones(n) if o.sigma is None else np.broadcast_to(np.asarray(o.sigma, dtype=np.float64), (n,))


def fourdvar(m, z0, obs, background=None):
    """(J, grad, residuals) on a model with the methods of ObsModel64 (the float32 restatement too): the forward run from z0 with the tape
    on, the misfits at the observation steps, lam = 0 and the walk backward that adds every set's H^T r at its own step.  residuals:
    r per set, in the order of obs."""
    T_ = max(o.step for o in obs)
    m.set_vort(np.asarray(z0))
    m.record_adjoint(T_)
    times = sorted(set(o.step for o in obs))
    J, res, at = 0.0, [None] * len(obs), 0
    for t in times:
        m.step(t - at)
        at = t
        for k, o in enumerate(obs):
            if o.step == t:
                d = np.asarray(m.observe(o.kind, o.xy), dtype=np.float64) - np.asarray(o.y, dtype=np.float64)
                s = sigma_of(o, d.size)
                res[k] = d / s ** 2
                J += 0.5 * float(np.sum(d * res[k]))
    m.set_adjoint(np.zeros((m.nx, m.ny)))
    for t, prev in zip(times[::-1], times[-2::-1] + [0]):
        for k, o in enumerate(obs):
            if o.step == t:
                m.adjoint_add_obs(o.kind, o.xy, res[k])
        m.adjoint_back(t - prev)
    grad = np.asarray(m.adjoint(), dtype=np.float64)
    m.record_adjoint(0)
    if background is not None:
        zb, sb = background
        d = np.asarray(z0, dtype=np.float64) - np.asarray(zb, dtype=np.float64)
        J += 0.5 * float(np.sum(d * d)) / sb ** 2
        grad = grad + d / sb ** 2
    return J, grad, res


class Float32Obs(A.Float32Model):
    """adjoint_numpy.Float32Model with point observations: float32 fields and spectra, the interpolation and the scatter in float64, as
    the engine has them"""

    def __init__(self, ref, source=None):
        super().__init__(ref, source)
        self.mult = {k: self.t.from_numpy(multiplier(ref, k)).to(self.t.complex64) for k in KINDS}

    def field(self, kind, spec=None):
        return self._c2r(self.mult[kind] * (self.vc if spec is None else spec)).numpy()

    def observe(self, kind, xy):
        return sample64(self.field(kind), xy)

    def observe_tangent(self, kind, xy):
        return sample64(self.field(kind, self.dc), xy)

    def adjoint_add_obs(self, kind, xy, w):
        self.lc = self.lc + self.t.conj(self.mult[kind]) * self._r2c(scatter64(xy, w, self.nx, self.ny).astype(np.float32))


class Fourdvar64:
    """what fit_initial needs, on the float64 reference: fourdvar(z0, obs, background) -> (J, grad) with torch float64 tensors on the CPU"""

    def __init__(self, model):
        import torch
        self.torch, self.m, self.calls = torch, model, 0

    def fourdvar(self, z0, obs, background=None):
        self.calls += 1
        J, g, _ = fourdvar(self.m, z0.detach().cpu().numpy().astype(np.float64), obs, background)
        return J, self.torch.from_numpy(g)


# ---- inputs of tests/test_obs_cpu.py and tests/test_gpu_obs.py ----
NPTS = 300
SEED = A.SEED + 1


def positions(nx, ny, n=NPTS, seed=SEED):
    """n positions from a fixed seed (particles_numpy.seed_positions: grid points first, the first and last cell of both axes, negative
    positions and positions 3 domain lengths away, the rest uniform), the last a copy of one in the middle: one stencil added to twice"""
    xy = P.seed_positions(nx, ny, LX, LY, n, seed=seed)
    if n > 40:
        xy[-1] = xy[40]
    return xy


def weights(n, seed=SEED):
    return np.random.default_rng(seed + 17).standard_normal(n)


def dot_residual_h(h, w, zeta, lam):
    """|<H zeta, w> - <zeta, H^T w>| / (|H zeta| |w|) in float64"""
    h, w, zeta, lam = (np.asarray(a, dtype=np.float64) for a in (h, w, zeta, lam))
    return float(abs(np.vdot(h, w) - np.vdot(zeta, lam)) / (np.linalg.norm(h) * np.linalg.norm(w)))


def h_identity(m, kind, zeta, xy, w):
    """the residual of the identity on a model (float64 or the float32 restatement): the state set to zeta, lam = 0 + H^T w"""
    m.set_vort(zeta)
    h = m.observe(kind, xy)
    m.set_adjoint(np.zeros((m.nx, m.ny), dtype=np.float32))
    m.adjoint_add_obs(kind, xy, w)
    return dot_residual_h(h, w, zeta, m.adjoint())


# The identity <H zeta, w> = <zeta, H^T w> on the adjoint's path cases (zeta: tangent_inputs' never-dealiased vorticity): f32 is the
# largest residual over the four kinds of the float32 restatement on the CPU, measured once; the GPU's bar is 4 x the largest of the
# table (the factor: another summation order), set before the GPU ran, and tests/test_obs_cpu.py holds the restatement itself to it.
HCase = namedtuple("HCase", "nx ny f32")
H_CASES = (HCase(256, 256, 2.6e-8), HCase(192, 192, 1.16e-8), HCase(3072, 64, 1.88e-8), HCase(1024, 64, 1.15e-8), HCase(4096, 64, 2.89e-8),
           HCase(64, 4096, 1.8e-8))
H_DOT_BAR = 4 * max(k.f32 for k in H_CASES)


# ---- the gradient case: 6 steps, u and v at the steps 2, 4, 6 and zeta at step 0 ----
GRAD_STEPS = 6
GRAD_GRIDS = ((256, 256), (1024, 64))
# the float32 restatement's residual of <grad, d> = sum over the sets of <r, H T_k d> (tangent_residual) on GRAD_GRIDS, as H_CASES' f32
GRAD_F32 = {(256, 256): 3.19e-12, (1024, 64): 1.31e-12}
GRAD_DOT_BAR = 4 * max(GRAD_F32.values())


def gradient_case(nx, ny, model):
    """(z0 float32, the source, the observation sets, d) of the gradient case: z0 and the direction d are tangent_inputs' vorticity and dz;
    the data are what `model` (float64, at z0 plus a smooth offset) gives, plus noise, so that no residual is small"""
    v, d, src, _ = A.adjoint_inputs(nx, ny, 3e-2)
    rng = np.random.default_rng(SEED + 3)
    truth = v.astype(np.float64) * 1.1 + 1e-4 * rng.standard_normal((nx, ny))
    model.set_vort(truth)
    sets, at = [], 0
    xy0 = positions(nx, ny, seed=SEED + 5)
    y0 = model.observe("vort", xy0)
    sets.append(Obs(0, "vort", xy0, y0 + 1e-5 * rng.standard_normal(NPTS), 2e-4))
    for k, step in enumerate((2, 4, 6)):
        model.step(step - at)
        at = step
        for kind in ("u", "v"):
            xy = positions(nx, ny, seed=SEED + 10 + k)
            y = model.observe(kind, xy)
            sets.append(Obs(step, kind, xy, y + 0.05 * rng.standard_normal(NPTS), 0.5 + rng.random(NPTS)))
    return v, src, sets, d


def tangent_residual(m, z0, obs, d, grad, res):
    """|<grad, d> - sum over the sets of <r, H T_k d>| / (|(H T_k d)_k| |(r_k)_k|) with T_k d from the model's own tangent"""
    m.set_vort(np.asarray(z0))
    m.record_adjoint(0)
    m.set_tangent(np.asarray(d))
    at, tot, hs = 0, 0.0, []
    for t in sorted(set(o.step for o in obs)):
        m.step(t - at)
        at = t
        for k, o in enumerate(obs):
            if o.step == t:
                h = np.asarray(m.observe_tangent(o.kind, o.xy), dtype=np.float64)
                tot += float(np.vdot(res[k], h))
                hs.append(h)
    m.set_tangent(None)
    lhs = float(np.vdot(np.asarray(grad, dtype=np.float64), np.asarray(d, dtype=np.float64)))
    return abs(lhs - tot) / (np.linalg.norm(np.concatenate(hs)) * np.linalg.norm(np.concatenate(res)))


# ---- the twin experiment at 64^2 ----
TWIN_N, TWIN_DT, TWIN_NU = 64, 30.0, 6.5
TWIN_STEPS = (2, 4, 6, 8)
TWIN_NPTS, TWIN_ITERS = 256, 10
# J_K / J_0 of fit_initial on the float64 reference after K = TWIN_ITERS iterations (tests/test_obs_cpu.py measures and asserts it to
# 10 %); the GPU test holds the engine to 10 x this
TWIN_RATIO = 0.01457
# the relative L2 change of the truth's vorticity over the window, float64 (asserted >= 0.1 in tests/test_obs_cpu.py)
TWIN_CHANGE = 0.3764


def twin_truth(make_field=None):
    if make_field is None:
        from oracle_py import make_field
    return make_field("kuo2004", TWIN_N, TWIN_N)


def twin_model():
    return ObsModel64(TWIN_N, TWIN_N, nu=TWIN_NU, dt=TWIN_DT)


def twin_case(make_field=None):
    """(truth float32, first guess float32, the observation sets): the truth's u and v at TWIN_NPTS fixed random points at the four
    steps of TWIN_STEPS, from the float64 reference, sigma = 1; the first guess is the truth scaled by 0.8 and shifted by two cells"""
    truth = twin_truth(make_field)
    m = twin_model()
    m.set_vort(truth)
    xy = np.random.default_rng(SEED + 30).random((TWIN_NPTS, 2)) * np.array([P.widen(LX), P.widen(LY)])
    sets, at = [], 0
    for step in TWIN_STEPS:
        m.step(step - at)
        at = step
        for kind in ("u", "v"):
            sets.append(Obs(step, kind, xy, m.observe(kind, xy), None))
    guess = (0.8 * np.roll(truth.astype(np.float64), 2, axis=0)).astype(np.float32)
    return truth, guess, sets, rel_l2(m.vort(), truth)
