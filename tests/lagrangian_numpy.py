"""float64 numpy reference of the Lagrangian (drifter) observations: obs_numpy.ObsModel64 extended by particles that are advanced with
the velocity of the model's own stage states (the step of particles_numpy.ParticleModel64, with the deformation gradient of
deformation_numpy.DeformationModel64 carried along), a tape of the positions every stage started from, a particle adjoint Xb, and the
backward sweep of the coupled step.  With x_s the position stage s started from, A_s = grad U_s(x_s) = [[u_x, u_y], [v_x, v_y]] of the
interpolant (deformation_numpy.sample_uv_grad; on a cell face the cell to the right) and A^T p = (u_x p_x + v_x p_y, u_y p_x + v_y p_y):

    p = dt/6 Xb;            q = A_3^T p; acc = Xb + q;   G_3 = (x_3, p)
    p = dt/3 Xb + dt q;     q = A_2^T p; acc += q;       G_2 = (x_2, p)
    p = dt/3 Xb + dt/2 q;   q = A_1^T p; acc += q;       G_1 = (x_1, p)
    p = dt/6 Xb + dt/2 q;   q = A_0^T p; Xb <- acc + q;  G_0 = (x_0, p)

and the pair G_s forces the adjoint of the stage state: the stage's transpose tendency (adjoint_numpy.AdjointModel64.adjoint_tendency)
gains conj(M_u) r2c(S_u) + conj(M_v) r2c(S_v), S_u = scatter(p_x at x_s), S_v = scatter(p_y at x_s), M the multipliers of
obs_numpy.multiplier.  The particles do not act on the flow: Xb never depends on lam.

Also the float32 torch restatement on the CPU (what a correct float32 engine can reach), a fourdvar that knows the kind "position",
the case tables and the inputs of tests/test_lagrangian_cpu.py and tests/test_gpu_lagrangian.py, and the twin experiment.  Used ONLY
by tests."""
from collections import namedtuple

import numpy as np

import adjoint_numpy as A
import checkpoint_numpy as C
import deformation_numpy as D
import obs_numpy as O
import particles_numpy as P
import tracer_numpy as T

LX = LY = O.LX
POSITION = "position"


def scatter64(xy, w, nx, ny):
    """obs_numpy.scatter64 (field[i, j] = sum over the points of w wx_a wy_b; what is not finite deposits nothing) by np.bincount, which
    six hundred thousand drifters need: the same float64 products, summed per cell in the order of the points"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).ravel()
    ok = np.isfinite(xy).all(axis=1) & np.isfinite(w)
    xy, w = xy[ok], w[ok]
    ix, wx = P.lagrange4_axis(xy[:, 0], P.widen(LX) / nx, nx)
    jy, wy = P.lagrange4_axis(xy[:, 1], P.widen(LY) / ny, ny)
    c = w[:, None, None] * (wx[:, :, None] * wy[:, None, :])
    cells = (ix[:, :, None] * ny + jy[:, None, :]).ravel()
    return np.bincount(cells, weights=c.ravel(), minlength=nx * ny).reshape(nx, ny)


def particle_backward(xb, xs, grads, dt):
    """one step of the particle recurrences: xb [n, 2], xs the four stage positions, grads(s, x) -> A [n, 2, 2] of stage s at x.
    Returns (the new Xb, [p_3, p_2, p_1, p_0]): p in the order the stages are swept."""
    At = lambda s, p: np.einsum("nij,ni->nj", grads(s, xs[s]), p)           # noqa: E731 -- A^T p
    p3 = (dt / 6) * xb
    q = At(3, p3)
    acc = xb + q
    p2 = (dt / 3) * xb + dt * q
    q = At(2, p2)
    acc = acc + q
    p1 = (dt / 3) * xb + (dt / 2) * q
    q = At(1, p1)
    acc = acc + q
    p0 = (dt / 6) * xb + (dt / 2) * q
    q = At(0, p0)
    return acc + q, [p3, p2, p1, p0]


class Lagrangian:
    """the mixin: in front of ObsModel64 (or Float32Obs); the class supplies _uv(vc) -> (u, v) real fields, _stage_states() of the step
    about to be taken, and _forcing(su, sv) -> the spectrum added to the stage's transpose tendency"""

    xy = F = xb = None
    pdepth = 0
    ptape = ()
    _force = ()

    def set_particles(self, xy):
        self.xy = None if xy is None else np.array(xy, dtype=np.float64).reshape(-1, 2)
        self.F = None if xy is None else D.identity(self.xy.shape[0])
        self.ptape, self.xb = [], None

    def particles(self):
        return self.xy

    def particle_deformation(self):
        return self.F

    def record_particles(self, depth):
        if depth and self.xy is None:
            raise ValueError("no particles are set")
        self.pdepth, self.ptape = int(depth), []

    def particles_recorded(self):
        return len(self.ptape), self.pdepth

    def set_particle_adjoint(self, xb):
        self.xb = None if xb is None else np.array(xb, dtype=np.float64).reshape(-1, 2)

    def particle_adjoint(self):
        return self.xb

    def set_vort(self, vort):
        super().set_vort(vort)
        self.ptape = []

    def _UA(self, vc, x):
        u, v = self._uv(vc)
        ok = np.isfinite(x).all(axis=1)
        U, Am = np.full((x.shape[0], 2), np.nan), np.full((x.shape[0], 2, 2), np.nan)
        if ok.any():
            U[ok], Am[ok] = D.sample_uv_grad(u, v, x[ok], LX, LY)
        return U, Am

    def step(self, n=1):
        """the particles' stages from the stage states of the step, then the step itself (the field's own code: its bits do not depend
        on the particles)"""
        if self.xy is None:
            return super().step(n)
        if self.pdepth and len(self.ptape) + n > self.pdepth:
            raise ValueError("the step would overrun the particle tape")
        dt = self.dt
        for _ in range(n):
            v = self._stage_states()
            x0, F0 = self.xy, self.F
            p1, a = self._UA(v[0], x0)
            K1 = a @ F0
            x1 = x0 + (dt / 2) * p1
            p2, a = self._UA(v[1], x1)
            K2 = a @ (F0 + (dt / 2) * K1)
            x2 = x0 + (dt / 2) * p2
            p3, a = self._UA(v[2], x2)
            K3 = a @ (F0 + (dt / 2) * K2)
            x3 = x0 + dt * p3
            p4, a = self._UA(v[3], x3)
            K4 = a @ (F0 + dt * K3)
            self.xy = x0 + (dt / 6) * (((p1 + 2 * p2) + 2 * p3) + p4)
            self.F = F0 + (dt / 6) * (((K1 + 2 * K2) + 2 * K3) + K4)
            if self.pdepth:
                self.ptape.append((x0, x1, x2, x3))
            super().step(1)

    def adjoint_back(self, n=1):
        if self.xb is None:
            return super().adjoint_back(n)
        if n > len(self.ptape):
            raise ValueError("more steps than the particle tape holds")
        for _ in range(n):
            vs, xs = self.tape[-1], self.ptape.pop()
            self.xb, ps = particle_backward(self.xb, xs, lambda s, x: self._UA(vs[s], x)[1], self.dt)
            self._force = []
            for s, p in zip((3, 2, 1, 0), ps):
                fin = np.isfinite(p).all(axis=1)                # a particle whose k-bar is not finite deposits nothing
                self._force.append(self._forcing(scatter64(xs[s][fin], p[fin, 0], self.nx, self.ny), scatter64(xs[s][fin], p[fin, 1], self.nx, self.ny)))
            super().adjoint_back(1)
            assert not self._force


class LagrangianModel64(Lagrangian, O.ObsModel64):
    def _uv(self, vc):
        psi = vc / self.lapi
        return -self._c2r(self.iky * psi), self._c2r(self.ikx * psi)

    def _stage_states(self):
        dt, v0 = self.dt, self.vc
        v1 = v0 + self.tendency(v0) * (dt / 2)
        v2 = v0 + self.tendency(v1) * (dt / 2)
        v3 = v0 + self.tendency(v2) * dt
        return v0, v1, v2, v3

    def _forcing(self, su, sv):
        return np.conj(O.multiplier(self, "u")) * np.fft.rfft2(su) + np.conj(O.multiplier(self, "v")) * np.fft.rfft2(sv)

    def adjoint_tendency(self, vc, mu):
        a = super().adjoint_tendency(vc, mu)
        return a + self._force.pop(0) if self._force else a


class CheckpointLagrangian64(C.Checkpointing, LagrangianModel64):
    """under checkpointing the particle tape still holds the whole window: a segment run again steps the vorticity alone"""


class Float32Lagrangian(Lagrangian, O.Float32Obs):
    """the float32 restatement: u and v float32 fields, the particles, the gradient of the interpolant and the scatter in float64, as the
    engine has them"""

    def _uv(self, vc):
        psi = vc / self.lapi
        return (-self._c2r(self.iky * psi)).numpy(), self._c2r(self.ikx * psi).numpy()

    def _stage_states(self):
        dt, v0 = self.dt, self.vc
        v1 = v0 + self._tend(v0, None)[0] * (dt / 2)
        v2 = v0 + self._tend(v1, None)[0] * (dt / 2)
        v3 = v0 + self._tend(v2, None)[0] * dt
        return v0, v1, v2, v3

    def _forcing(self, su, sv):
        return self.t.conj(self.mult["u"]) * self._r2c(su.astype(np.float32)) + self.t.conj(self.mult["v"]) * self._r2c(sv.astype(np.float32))

    def _atend(self, vc, mu):
        a = super()._atend(vc, mu)
        return a + self._force.pop(0) if self._force else a


# ---- the 4D-Var cost with drifter positions ----
Obs = O.Obs


def fourdvar(m, z0, obs, background=None, particles=None):
    """obs_numpy.fourdvar with sets of the kind "position" (xy None, y [n, 2], sigma None, a number or [n]): (J, grad, dJ/dX0 or None)"""
    T_ = max(o.step for o in obs)
    drift = any(o.kind == POSITION for o in obs)
    if drift and particles is None:
        raise ValueError("a 'position' set needs particles")
    m.set_vort(np.asarray(z0))
    if particles is not None:
        m.set_particles(particles)
    m.record_adjoint(T_)
    if drift:
        m.record_particles(T_)
    times = sorted(set(o.step for o in obs))
    J, res, at = 0.0, [None] * len(obs), 0
    for t in times:
        m.step(t - at)
        at = t
        for k, o in enumerate(obs):
            if o.step != t:
                continue
            if o.kind == POSITION:
                d = m.particles() - np.asarray(o.y, dtype=np.float64)
                s = O.sigma_of(o, d.shape[0])[:, None]
            else:
                d = np.asarray(m.observe(o.kind, o.xy), dtype=np.float64) - np.asarray(o.y, dtype=np.float64)
                s = O.sigma_of(o, d.size)
            res[k] = d / s ** 2
            J += 0.5 * float(np.sum(d * res[k]))
    m.set_adjoint(np.zeros((m.nx, m.ny)))
    if drift:
        m.set_particle_adjoint(np.zeros_like(m.particles()))
    for t, prev in zip(times[::-1], times[-2::-1] + [0]):
        for k, o in enumerate(obs):
            if o.step == t and o.kind == POSITION:
                m.set_particle_adjoint(m.particle_adjoint() + res[k])
            elif o.step == t:
                m.adjoint_add_obs(o.kind, o.xy, res[k])
        m.adjoint_back(t - prev)
    grad = np.asarray(m.adjoint(), dtype=np.float64)
    xb0 = m.particle_adjoint() if drift else None
    m.record_adjoint(0)
    m.record_particles(0)
    m.set_particle_adjoint(None)
    if background is not None:
        zb, sb = background
        d = np.asarray(z0, dtype=np.float64) - np.asarray(zb, dtype=np.float64)
        J += 0.5 * float(np.sum(d * d)) / sb ** 2
        grad = grad + d / sb ** 2
    return J, grad, xb0


class Fourdvar64:
    """what binding.fit_initial needs, on the float64 reference: fourdvar(z0, obs, background, particles=) -> (J, grad) with torch
    float64 tensors on the CPU"""

    def __init__(self, model):
        import torch
        self.torch, self.m, self.calls = torch, model, 0

    def fourdvar(self, z0, obs, background=None, particles=None):
        self.calls += 1
        J, g, _ = fourdvar(self.m, z0.detach().cpu().numpy().astype(np.float64), obs, background, particles)
        return J, self.torch.from_numpy(g)


# ---- inputs ----
NPTS = O.NPTS
SEED = O.SEED + 100
STEPS = A.STEPS


def ref_model(nx, ny, cls=LagrangianModel64):
    return cls(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))


def xbar_T(n, seed=SEED):
    """the particle adjoint a sweep starts from: white noise of unit variance, float64 [n, 2]"""
    return np.random.default_rng(seed).standard_normal((n, 2))


def interior_positions(nx, ny, n=NPTS, seed=SEED):
    """n positions strictly inside cells, 0.1 ... 0.9 of a cell from the lower face on both axes: where the discrete map is
    differentiable with respect to the position (the interpolant's derivative jumps at the faces)"""
    rng = np.random.default_rng(seed + 1)
    ij = np.stack([rng.integers(0, nx, n), rng.integers(0, ny, n)], axis=1)
    return (ij + 0.1 + 0.8 * rng.random((n, 2))) * np.array([P.widen(LX) / nx, P.widen(LY) / ny])


def sweep_case(nx, ny, cls=LagrangianModel64, lam_T=None, xy=None, steps=STEPS, source=True):
    """The sweep of the path cases on a reference model: adjoint_inputs' never-dealiased vorticity (and its source), the drifters at
    obs_numpy.positions, both tapes on, `steps` steps, lam(T) = lam_T (None: 0) and Xb(T) = xbar_T, swept back.  Returns the model:
    adjoint() is lam_0, particle_adjoint() Xb_0, particles() X(T), particle_deformation() F."""
    v, _, src, _ = A.adjoint_inputs(nx, ny, 3e-2)
    xy = O.positions(nx, ny) if xy is None else xy
    if cls is Float32Lagrangian:
        m = cls(ref_model(nx, ny), src if source else None)
    else:
        m = ref_model(nx, ny, cls)
        if source:
            m.src = src.astype(np.float64)
    m.set_vort(v)
    m.set_particles(xy)
    m.record_adjoint(steps)
    m.record_particles(steps)
    m.step(steps)
    m.set_adjoint(np.zeros((nx, ny), dtype=np.float32) if lam_T is None else lam_T)
    m.set_particle_adjoint(xbar_T(xy.shape[0]))
    m.adjoint_back(steps)
    return m


def xbar_error(got, want):
    """max |got - want| over the finite entries of want, relative to max |want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want)
    return float(np.abs(got[ok] - want[ok]).max() / np.abs(want[ok]).max())


# The sweep on the adjoint's path cases (adjoint_numpy.PATH_CASES' grids, 5 steps, 300 drifters, lam(T) = 0 and Xb(T) = xbar_T): lam and
# xbar are the float32 restatement's errors of lam_0 (relative L2) and of Xb_0 (xbar_error) against float64, measured once on the CPU;
# moved: the drifters' largest displacement over the window in cells.  tests/test_lagrangian_cpu.py asserts the two as upper bounds
# where it runs the case.  The GPU's bar for Xb_0 is 4 x the largest xbar of the table (the factor: another summation order), set
# before the GPU ran; for lam_0 it is the adjoint's own 1e-5.
LCase = namedtuple("LCase", "nx ny lam xbar moved")
L_CASES = (LCase(256, 256, 1.69e-07, 6.69e-08, 0.997), LCase(192, 192, 1.65e-07, 7.04e-08, 0.809), LCase(3072, 64, 1.92e-07, 7.7e-08, 2.6),
           LCase(1024, 64, 2.02e-07, 1.84e-07, 4.07), LCase(4096, 64, 1.9e-07, 6.29e-08, 2.24), LCase(64, 4096, 1.92e-07, 7.64e-08, 2.01))
XBAR_BAR = 4 * max(k.xbar for k in L_CASES)
LAM_BAR = 1e-5


def lcase_of(nx, ny):
    return [k for k in L_CASES if (k.nx, k.ny) == (nx, ny)][0]


# ---- the fourdvar cases: position sets alone, and mixed with u and v ----
GRAD_GRIDS = O.GRAD_GRIDS


# The float32 restatement's errors of J, grad and dJ/dX_0 against float64 on the fourdvar cases below, measured once on the CPU.  There
# Xb(T) is not given but is the residual (X(T) - y) / sigma^2 of the float32 run's own positions, so the positions' float32 error,
# divided by the misfit, enters dJ/dX_0 before the sweep begins: the figures are some twenty times the sweep's (L_CASES), on the CPU
# as on the GPU, and dJ/dX_0 of fourdvar has a bar of its own by the same rule, 4 x the largest figure of this table.
FCase = namedtuple("FCase", "nx ny mixed J grad xbar")
F_CASES = (FCase(256, 256, False, 1.71e-06, 1.37e-06, 1.4e-06), FCase(256, 256, True, 1.63e-06, 1.06e-06, 1.4e-06),
           FCase(1024, 64, False, 1.28e-06, 1.53e-06, 1.43e-06), FCase(1024, 64, True, 1.26e-06, 1.45e-06, 1.43e-06))
FOURDVAR_XBAR_BAR = 4 * max(k.xbar for k in F_CASES)


def position_case(nx, ny, model, mixed):
    """(z0 float32, the source, xy0, the observation sets): the drifters start at obs_numpy.positions; the data are what `model` (float64,
    at z0 times 1.1 plus a smooth offset) gives for the positions at the steps 3 and 6, plus noise of a two-hundredth of a cell, sigma a
    hundredth of a cell (per drifter: 0.5 ... 1.5 of it; so that the drifters' part of J weighs some percent of the u and v sets'); mixed: also obs_numpy.gradient_case's sets of u and v at the steps 2, 4, 6"""
    v, src, sets, _ = O.gradient_case(nx, ny, model)
    rng = np.random.default_rng(SEED + 3)
    truth = v.astype(np.float64) * 1.1 + 1e-4 * rng.standard_normal((nx, ny))
    xy0 = O.positions(nx, ny)
    cell = P.widen(LX) / nx
    model.set_vort(truth)
    model.set_particles(xy0)
    out, at = [], 0
    for step in (3, 6):
        model.step(step - at)
        at = step
        out.append(Obs(step, POSITION, None, model.particles() + 0.005 * cell * rng.standard_normal((NPTS, 2)), 0.01 * cell * (0.5 + rng.random(NPTS))))
    model.set_particles(None)
    if mixed:
        out += [s for s in sets if s.step > 0]
    return v, src, xy0, out


# ---- the twin experiment at 64^2: drifter positions alone ----
TWIN_NPTS, TWIN_ITERS = O.TWIN_NPTS, O.TWIN_ITERS
TWIN_STEPS = O.TWIN_STEPS
# J_K / J_0 of fit_initial on the float64 reference after TWIN_ITERS iterations (tests/test_lagrangian_cpu.py measures and asserts it to
# 10 %); the GPU test holds the engine to 10 x this
TWIN_RATIO = 0.02973


def twin_case(make_field=None):
    """(truth, first guess, xy0, the position sets, sigma): obs_numpy.twin_case's truth and first guess; the only data are the positions of
    TWIN_NPTS drifters, started at fixed random points, at the steps of TWIN_STEPS from the float64 reference; sigma is a tenth of the
    drifters' largest displacement over the window"""
    truth, guess, _, _ = O.twin_case(make_field)
    m = LagrangianModel64(O.TWIN_N, O.TWIN_N, nu=O.TWIN_NU, dt=O.TWIN_DT)
    m.set_vort(truth)
    xy0 = np.random.default_rng(SEED + 30).random((TWIN_NPTS, 2)) * np.array([P.widen(LX), P.widen(LY)])
    m.set_particles(xy0)
    ys, at = [], 0
    for step in TWIN_STEPS:
        m.step(step - at)
        at = step
        ys.append(m.particles().copy())
    sigma = 0.1 * float(np.sqrt(((ys[-1] - xy0) ** 2).sum(axis=1)).max())
    return truth, guess, xy0, [Obs(s, POSITION, None, y, sigma) for s, y in zip(TWIN_STEPS, ys)], sigma
