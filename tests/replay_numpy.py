"""float64 numpy reference of the tangent replay over the adjoint's tape and of Gauss-Newton 4D-Var built on it: obs_numpy.ObsModel64 with
a tape that a sweep does not destroy (adjoint_back moves a fill mark, adjoint_rewind moves it back, a step recorded after a pop
overwrites what lay above it) and tangent_replay(first, n), the tangent step of the taped steps applied to the perturbation from the
recorded stage states, with no nonlinear step.  On it the Gauss-Newton Hessian-vector product

    H_GN v = v / sigma_b^2 + sum over the sets k of T_k^T H_k^T R_k^-1 H_k T_k v

and the incremental 4D-Var loop (conjugate gradients on the quadratic model inside, a nonlinear Armijo search outside), both written
against the model's methods alone, so that they run on the float32 torch restatement too (Float32Replay: what a correct float32
engine can reach).  Also the adapters that let binding.gauss_newton_hvp and binding.fit_incremental run on the float64 model, the
measured constants and the inputs of tests/test_gpu_replay.py.  Used ONLY by tests."""
from collections import namedtuple

import numpy as np

import obs_numpy as O


class _ReplayTape:
    """The tape discipline shared by the float64 model and the float32 restatement: self.tape holds every recorded step that has not
    been overwritten, self.fill of them are unswept."""

    def record_adjoint(self, depth):
        super().record_adjoint(depth)
        self.fill = 0

    def set_vort(self, v):
        super().set_vort(v)
        self.fill = 0

    def set_spectrum(self, vc):
        super().set_spectrum(vc)
        self.fill = 0

    def adjoint_recorded(self):
        return self.fill

    def adjoint_top(self):
        return len(self.tape)

    def step(self, n=1):
        if self.depth:
            self.tape = self.tape[:self.fill]               # a step recorded after a pop overwrites the slots above it
        super().step(n)
        if self.depth:
            self.fill = len(self.tape)

    def adjoint_back(self, n=1):
        if n < 0 or n > self.fill:
            raise ValueError("more steps than are recorded")
        whole = self.tape
        self.tape = list(whole[:self.fill])
        try:
            super().adjoint_back(n)                         # (it pops its copy)
        finally:
            self.tape = whole
        self.fill -= n

    def adjoint_rewind(self, n=-1):
        popped = len(self.tape) - self.fill
        if n < -1 or n > popped:
            raise ValueError("more steps than were popped")
        self.fill += popped if n < 0 else n

    def tangent_replay(self, first, n):
        if self.dc is None:
            raise ValueError("no tangent is set")
        if first < 0 or n < 0 or first + n > len(self.tape):
            raise ValueError("beyond the recorded steps")
        dt = self.dt
        for v0, v1, v2, v3 in self.tape[first:first + n]:
            d0 = self.dc
            l1 = self._replay_tend(v0, d0)
            l2 = self._replay_tend(v1, d0 + l1 * (dt / 2))
            l3 = self._replay_tend(v2, d0 + l2 * (dt / 2))
            l4 = self._replay_tend(v3, d0 + l3 * dt)
            self.dc = d0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6


class ReplayModel64(_ReplayTape, O.ObsModel64):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.fill = 0

    def _replay_tend(self, vc, dc):
        return self.tangent_tendency(vc, dc)


class Float32Replay(_ReplayTape, O.Float32Obs):
    """obs_numpy.Float32Obs with the replay: the tangent tendency as ONE product in physical space, the form of the engine's kernel"""

    def __init__(self, ref, source=None):
        super().__init__(ref, source)
        self.fill = 0

    def _replay_tend(self, vc, dc):
        c2r, ikx, iky = self._c2r, self.ikx, self.iky
        psi, dpsi = vc / self.lapi, dc / self.lapi
        u, v, zx, zy = -c2r(iky * psi), c2r(ikx * psi), c2r(ikx * vc), c2r(iky * vc)
        du, dv = -c2r(iky * dpsi), c2r(ikx * dpsi)
        td = (((-u * c2r(ikx * dc)) - v * c2r(iky * dc)) - du * zx) - dv * zy
        return (self.t.fft.rfft2(td) + dc * self.lap * self.nu) * self.mask


# ---- 4D-Var that keeps the tape, the Hessian-vector product and the incremental loop ----
def fourdvar_keep(m, z0, obs, background=None):
    """obs_numpy.fourdvar with the tape kept and rewound in the place of freed, z0 set as float32 as the engine takes it: (J, grad)"""
    T_ = max(o.step for o in obs)
    m.set_vort(np.asarray(z0).astype(np.float32))
    m.record_adjoint(T_)
    times = sorted(set(o.step for o in obs))
    J, res, at = 0.0, [None] * len(obs), 0
    for t in times:
        m.step(t - at)
        at = t
        for k, o in enumerate(obs):
            if o.step == t:
                d = np.asarray(m.observe(o.kind, o.xy), dtype=np.float64) - np.asarray(o.y, dtype=np.float64)
                res[k] = d / O.sigma_of(o, d.size) ** 2
                J += 0.5 * float(np.sum(d * res[k]))
    m.set_adjoint(np.zeros((m.nx, m.ny)))
    for t, prev in zip(times[::-1], times[-2::-1] + [0]):
        for k, o in enumerate(obs):
            if o.step == t:
                m.adjoint_add_obs(o.kind, o.xy, res[k])
        m.adjoint_back(t - prev)
    grad = np.asarray(m.adjoint(), dtype=np.float64)
    m.adjoint_rewind(-1)
    if background is not None:
        zb, sb = background
        d = np.asarray(z0, dtype=np.float64) - np.asarray(zb, dtype=np.float64)
        J += 0.5 * _dot(d, d) / sb ** 2
        grad = grad + d / sb ** 2
    return J, grad


def gauss_newton_hvp(m, v, obs, background=None):
    """H_GN v about the trajectory on m's tape (fourdvar_keep), float64 [nx, ny]: replay to every observation time, w = H dz / sigma^2,
    lam = 0, the walk backward with H^T w, the rewind.  v is set as float32, as the engine takes it; the tangent is removed at the end."""
    times = sorted(set(o.step for o in obs))
    v = np.asarray(v, dtype=np.float64)
    m.set_tangent(v.astype(np.float32))
    w, at = {}, 0
    for t in times:
        m.tangent_replay(at, t - at)
        at = t
        for k, o in enumerate(obs):
            if o.step == t:
                h = np.asarray(m.observe_tangent(o.kind, o.xy), dtype=np.float64)
                w[k] = h / O.sigma_of(o, h.size) ** 2
    m.set_adjoint(np.zeros((m.nx, m.ny)))
    for t, prev in zip(times[::-1], times[-2::-1] + [0]):
        for k, o in enumerate(obs):
            if o.step == t:
                m.adjoint_add_obs(o.kind, o.xy, w[k])
        m.adjoint_back(t - prev)
    hv = np.asarray(m.adjoint(), dtype=np.float64)
    m.adjoint_rewind(-1)
    m.dc = None
    if background is not None:
        hv = hv + v / background[1] ** 2
    return hv


def _dot(a, b):
    """sum of a b in torch's summation order, so that the loop below and binding.fit_incremental take the same path bit for bit"""
    import torch
    return float(torch.from_numpy(a * b).sum())


def fit_incremental(m, z0, obs, outer, inner, background=None, cg_tol=1e-2, armijo=1e-4, shrink=0.5, max_backtracks=25):
    """(z, J_history, evaluations, hvps): the incremental loop on a model with the methods of ReplayModel64, in numpy"""
    x = np.array(z0, dtype=np.float64)
    J, g = fourdvar_keep(m, x, obs, background)
    evals, hvps, hist = 1, 0, [J]
    for _ in range(outer):
        gg = _dot(g, g)
        if not gg > 0.0:
            break
        d, r = np.zeros_like(g), -g
        p, rr = r.copy(), gg
        for it in range(inner):
            hp = gauss_newton_hvp(m, p, obs, background)
            hvps += 1
            php = _dot(p, hp)
            if not php > 0.0:
                if it == 0:
                    d = r.copy()
                break
            a = rr / php
            d = d + a * p
            r = r - a * hp
            rn = _dot(r, r)
            if np.sqrt(rn) <= cg_tol * np.sqrt(gg):
                break
            p = r + (rn / rr) * p
            rr = rn
        slope = _dot(g, d)
        if not slope < 0.0:
            break
        step, found = 1.0, None
        for _ in range(max_backtracks):
            xn = x + step * d
            Jn, gn = fourdvar_keep(m, xn, obs, background)
            evals += 1
            if np.isfinite(Jn) and Jn <= J + armijo * step * slope:
                found = (xn, Jn, gn)
                break
            step *= shrink
        if found is None:
            break
        x, J, g = found
        hist.append(J)
    m.record_adjoint(0)
    return x, hist, evals, hvps


# ---- binding's helpers on the float64 model ----
TObs = namedtuple("TObs", "step kind xy y sigma")            # obs_numpy.Obs as binding's helpers read a set: sigma a float64 tensor


def torch_obs(obs):
    import torch
    return [TObs(o.step, o.kind, o.xy, torch.from_numpy(np.asarray(o.y, dtype=np.float64)),
                 torch.from_numpy(np.array(O.sigma_of(o, len(o.y)), dtype=np.float64))) for o in obs]


class Torch64:
    """ReplayModel64 behind the tensor-facing methods that binding.fourdvar, binding.gauss_newton_hvp and binding.fit_incremental call
    (torch float64 / float32 tensors on the CPU in and out); `calls` counts what reached the model, by name."""

    device = "cpu"

    def __init__(self, model):
        import torch
        self.torch, self.m, self.calls = torch, model, {}
        self._shape = (model.nx, model.ny)

    def _np(self, a):
        return None if a is None else a.detach().cpu().numpy().astype(np.float64)

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def set_vort(self, z): self._count("set_vort"); self.m.set_vort(self._np(z))
    def record_adjoint(self, depth): self.m.record_adjoint(depth)
    def adjoint_recorded(self): return self.m.adjoint_recorded()
    def step(self, n=1): self._count("step"); self.m.step(n)
    def observe(self, kind, xy): return self.torch.from_numpy(self.m.observe(kind, xy))
    def observe_tangent(self, kind, xy, k=0): return self.torch.from_numpy(self.m.observe_tangent(kind, xy))

    def obs_misfit(self, h, y, sigma, cost, check=True):
        d = h - y
        r = d / sigma ** 2
        cost += 0.5 * float(np.sum(d.numpy() * r.numpy()))
        return r

    def set_tangent(self, dz):
        if dz is None:
            self.m.dc = None
        else:
            self.m.set_tangent(self._np(dz))

    def tangent_replay(self, first, n): self._count("tangent_replay"); self.m.tangent_replay(first, n)
    def set_adjoint(self, lam): self.m.set_adjoint(self._np(lam))
    def adjoint_add_obs(self, kind, xy, w): self.m.adjoint_add_obs(kind, xy, self._np(w))
    def adjoint_back(self, n=1): self.m.adjoint_back(n)
    def adjoint_rewind(self, n=-1): self.m.adjoint_rewind(n)
    def adjoint(self): return self.torch.from_numpy(np.asarray(self.m.adjoint(), dtype=np.float64))

    def fourdvar(self, z0, obs, background=None, keep_tape=False):
        import xlab_fftbarotropic_amd as X
        self._count("fourdvar")
        return X.fourdvar(self, z0, obs, background, keep_tape=keep_tape)

    def gauss_newton_hvp(self, v, obs, background=None):
        import xlab_fftbarotropic_amd as X
        self._count("gauss_newton_hvp")
        return X.gauss_newton_hvp(self, v, obs, background)


def symmetry_residual(hd, hw, d, w):
    """|<w, H d> - <d, H w>| / (|H d| |w|) in float64"""
    hd, hw, d, w = (np.asarray(a, dtype=np.float64) for a in (hd, hw, d, w))
    return float(abs(np.vdot(w, hd) - np.vdot(d, hw)) / (np.linalg.norm(hd) * np.linalg.norm(w)))


def white_like(d, seed=O.SEED + 40):
    """white noise, never dealiased, of d's rms, float32"""
    d = np.asarray(d, dtype=np.float64)
    return (np.random.default_rng(seed).standard_normal(d.shape) * np.sqrt(np.mean(d ** 2))).astype(np.float32)


def gradient_model(nx, ny, cls=ReplayModel64):
    """the model of obs_numpy.gradient_case at (nx, ny), as tests/test_gpu_obs.py sets it up: the recipe's nu and dt"""
    import tracer_numpy as T
    import tangent_numpy as G
    return cls(nx, ny, nu=G.NU, dt=T.recipe_dt(nx, ny))


# ---- singular vectors by replay ----
def singular_vectors_replay(model, spectrum0, steps, k, iters, start):
    """singular_numpy.singular_vectors with the forward run made once, with the tape on and no tangent, and every T v_i a replay over that
    tape (binding.singular_vectors(replay=True)): (sigma [iters, k], the final V [k, nx, ny])"""
    import singular_numpy as S
    start = np.asarray(start, dtype=np.float64)
    shape = start.shape[1:]
    v = S.orthonormal_rows(start.reshape(k, -1))
    model.set_spectrum(spectrum0)
    model.dc = None
    model.record_adjoint(steps)
    model.step(steps)
    sig = []
    for _ in range(iters):
        u, w = np.empty_like(v), np.empty_like(v)
        for i in range(k):
            model.set_tangent(v[i].reshape(shape))
            model.tangent_replay(0, steps)
            ui = np.asarray(model.tangent(), dtype=np.float64)
            u[i] = ui.ravel()
            model.set_adjoint(ui)
            model.adjoint_back(steps)
            w[i] = np.asarray(model.adjoint(), dtype=np.float64).ravel()
            model.adjoint_rewind(-1)
        lam, e = np.linalg.eigh(u @ u.T)
        order = np.argsort(lam)[::-1]
        sig.append(np.sqrt(np.maximum(lam[order], 0.0)))
        v = S.orthonormal_rows(e[:, order].T @ w)
    model.dc = None
    model.record_adjoint(0)
    model.set_spectrum(spectrum0)
    return np.array(sig), v.reshape((k,) + tuple(shape))


def sv_replay_reference(float32=False):
    """singular_numpy.sv_reference's case by replay, in float64 or in the float32 restatement"""
    import singular_numpy as S
    v, s, start = S.sv_inputs()
    ref = gradient_model(S.SV_N, S.SV_N)
    ref.set_vort(v)
    ref.src = s.astype(np.float64)
    if not float32:
        return singular_vectors_replay(ref, ref.spectrum(), S.SV_STEPS, S.SV_K, S.SV_ITERS, start)
    f = Float32Replay(ref, s)
    f.set_vort(v)
    return singular_vectors_replay(f, f.spectrum(), S.SV_STEPS, S.SV_K, S.SV_ITERS, start)


# ---- measured on the CPU (tests/test_replay_cpu.py measures them again) ----
# J_K / J_0 of fit_incremental(outer=3, inner=8) on the float64 reference on obs_numpy.twin_case (asserted to 10 %), with 4 nonlinear
# evaluations and 24 Hessian-vector products; the GPU test holds the engine to 10 x this, as the L-BFGS twin is held to 10 x TWIN_RATIO
GN_TWIN_RATIO = 0.003148
GN_TWIN_OUTER, GN_TWIN_INNER = 3, 8
# the float32 restatement of H_GN v on obs_numpy's gradient case (source on), v the case's direction d and w = white_like(d): the larger
# of the two relative L2 errors against float64, and the symmetry residual |<w, H d> - <d, H w>| / (|H d| |w|) (float64: 4e-18).  Draws
# of rounding: the CPU test holds the restatement to the GPU's bars, HVP_BAR (the bar of lam_0 and of the 4D-Var gradient) and
# HVP_SYM_BAR (4 x the largest figure: the GPU's other summation order, set before the GPU ran), not to its own table
HVP_F32 = {(256, 256): 2.47e-7, (1024, 64): 3.80e-7}
HVP_SYM_F32 = {(256, 256): 4.80e-10, (1024, 64): 1.27e-9}
HVP_BAR = 1e-5
HVP_SYM_BAR = 4 * max(HVP_SYM_F32.values())
# singular vectors by replay on singular_numpy's case (256^2, 3 steps, k = 4, 4 iterations): the sine of the largest principal angle
# between the final subspace of the float32 restatement of the REPLAYED iteration and float64's (which the float64 replay reproduces to
# 5e-16), asserted in tests/test_replay_cpu.py as an upper bound to 1.5 (singular_numpy.SV_ANGLE_F32's margin for another FFT library);
# the GPU's bar is 4 x this figure.  Its sigma are 3.3e-7 off float64
SV_REPLAY_ANGLE_F32 = 2.56e-07
SV_REPLAY_ANGLE_BAR = 4 * SV_REPLAY_ANGLE_F32
# the background term of the Hessian-vector product's cases: sigma_b of the size that makes v / sigma_b^2 comparable to the data term
HVP_SIGMA_B = 2e-4
