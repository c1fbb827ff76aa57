"""float64 numpy reference of the deformation gradient along the particles (include/fftbaro.h, fb_model_set_particle_deformation): the
gradient of the cubic Lagrange interpolant itself, the RK4 of positions and F = dX(t) / dX(t0) in given stage velocities, the float64
model coupled to it stage by stage, and the closed-form 2 x 2 singular value decomposition of fb_model_particle_stretching.  Builds
on particles_numpy.  Used ONLY by tests."""
import numpy as np

from particles_numpy import ParticleModel64, lagrange4_axis, widen

# sum |w'| <= 2.34 and sum |w| <= 1.25 over t in [0, 1): the bound of one entry of A by max |field| / spacing (tolerances of the GPU tests)
DW_SUM, W_SUM = 2.34, 1.25


def lagrange4_axis_d(x, d, n):
    """lagrange4_axis with the weights' derivatives with respect to t, [npts, 4] (over d: with respect to x, of the cell t lies in; at
    t == 0 the cell to the right)"""
    idx, w = lagrange4_axis(x, d, n)
    s = np.asarray(x, dtype=np.float64) / d
    t = s - np.floor(s)
    t3 = 3.0 * t * t
    dw = np.stack([-((t3 - 6.0 * t) + 2.0) / 6.0, ((t3 - 4.0 * t) - 1.0) / 2.0, -((t3 - 2.0 * t) - 2.0) / 2.0, (t3 - 1.0) / 6.0], axis=1)
    return idx, w, dw


def lagrange4_sample_grad(field, xy, lx, ly):
    """(value, d/dx, d/dy) of particles_numpy.lagrange4_sample's interpolant at xy [npts, 2], each [npts]: the same stencil, on each
    axis the value weights or their derivatives over the spacing"""
    f = np.asarray(field)
    nx, ny = f.shape
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    dx, dy = widen(lx) / nx, widen(ly) / ny
    ix, wx, dwx = lagrange4_axis_d(xy[:, 0], dx, nx)
    jy, wy, dwy = lagrange4_axis_d(xy[:, 1], dy, ny)
    acc, gx, gy = np.zeros(xy.shape[0]), np.zeros(xy.shape[0]), np.zeros(xy.shape[0])
    for a in range(4):
        q = f[ix[:, a, None], jy].astype(np.float64)
        r = ((wy[:, 0] * q[:, 0] + wy[:, 1] * q[:, 1]) + wy[:, 2] * q[:, 2]) + wy[:, 3] * q[:, 3]
        ry = ((dwy[:, 0] * q[:, 0] + dwy[:, 1] * q[:, 1]) + dwy[:, 2] * q[:, 2]) + dwy[:, 3] * q[:, 3]
        acc = acc + wx[:, a] * r
        gx = gx + dwx[:, a] * r
        gy = gy + wx[:, a] * ry
    return acc, gx / dx, gy / dy


def sample_uv_grad(u, v, x, lx, ly):
    """(U [npts, 2], A [npts, 2, 2]) of the fields u, v at x: A = [[u_x, u_y], [v_x, v_y]] of the interpolant"""
    uu, ux, uy = lagrange4_sample_grad(u, x, lx, ly)
    vv, vx, vy = lagrange4_sample_grad(v, x, lx, ly)
    return np.stack([uu, vv], axis=1), np.stack([np.stack([ux, uy], axis=1), np.stack([vx, vy], axis=1)], axis=1)


def rk4_deformation(xy, F, stage_velocity_and_gradient, dt, steps):
    """RK4 of the positions xy [npts, 2] (particles_numpy.rk4_particles, expression for expression) and of F [npts, 2, 2]:
    stage_velocity_and_gradient(step, stage, X) -> (U [npts, 2], A [npts, 2, 2]);
    K1 = A_0(X0) F0, K2 = A_1(X0 + dt/2 k1) (F0 + dt/2 K1), K3 = A_2(X0 + dt/2 k2) (F0 + dt/2 K2), K4 = A_3(X0 + dt k3) (F0 + dt K3),
    F <- F0 + dt/6 (((K1 + 2 K2) + 2 K3) + K4).  Returns (positions, F)."""
    x = np.array(xy, dtype=np.float64).reshape(-1, 2)
    F = np.array(F, dtype=np.float64).reshape(-1, 2, 2)
    for n in range(steps):
        k1, a = stage_velocity_and_gradient(n, 0, x)
        K1 = a @ F
        k2, a = stage_velocity_and_gradient(n, 1, x + (dt / 2) * k1)
        K2 = a @ (F + (dt / 2) * K1)
        k3, a = stage_velocity_and_gradient(n, 2, x + (dt / 2) * k2)
        K3 = a @ (F + (dt / 2) * K2)
        k4, a = stage_velocity_and_gradient(n, 3, x + dt * k3)
        K4 = a @ (F + dt * K3)
        x = x + (dt / 6) * (((k1 + 2 * k2) + 2 * k3) + k4)
        F = F + (dt / 6) * (((K1 + 2 * K2) + 2 * K3) + K4)
    return x, F


def identity(n):
    return np.tile(np.eye(2), (n, 1, 1))


class DeformationModel64(ParticleModel64):
    """ParticleModel64 whose particles carry F, advanced with the gradient of the interpolated velocity of the model's own stage states"""

    def set_particles(self, xy):
        super().set_particles(xy)
        self.F = identity(self.xy.shape[0])

    def _UA(self, vc, x):
        u, v = self.velocity(vc)
        return sample_uv_grad(u, v, x, self.lx, self.ly)

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, x0, F0 = self.vc, self.xy, self.F
            k1, (p1, a) = self.tendency(v0), self._UA(v0, x0)
            K1 = a @ F0
            v1 = v0 + k1 * (dt / 2)
            k2, (p2, a) = self.tendency(v1), self._UA(v1, x0 + (dt / 2) * p1)
            K2 = a @ (F0 + (dt / 2) * K1)
            v2 = v0 + k2 * (dt / 2)
            k3, (p3, a) = self.tendency(v2), self._UA(v2, x0 + (dt / 2) * p2)
            K3 = a @ (F0 + (dt / 2) * K2)
            v3 = v0 + k3 * dt
            k4, (p4, a) = self.tendency(v3), self._UA(v3, x0 + dt * p3)
            K4 = a @ (F0 + dt * K3)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.xy = x0 + (dt / 6) * (((p1 + 2 * p2) + 2 * p3) + p4)
            self.F = F0 + (dt / 6) * (((K1 + 2 * K2) + 2 * K3) + K4)


def cellular_gradient(x, lx, ly, amp, mx, my):
    """A [npts, 2, 2] = [[u_x, u_y], [v_x, v_y]] of particles_numpy.cellular_velocity, analytically"""
    kx, ky = 2 * np.pi * mx / lx, 2 * np.pi * my / ly
    cx, sx, cy, sy = np.cos(kx * x[:, 0]), np.sin(kx * x[:, 0]), np.cos(ky * x[:, 1]), np.sin(ky * x[:, 1])
    return np.stack([np.stack([-amp * ky * kx * sx * sy, amp * ky * ky * cx * cy], axis=1),
                     np.stack([-amp * kx * kx * cx * cy, amp * kx * ky * sx * sy], axis=1)], axis=1)


def fold(theta):
    """an angle in (-pi, pi] folded into (-pi/2, pi/2]: the axis it names"""
    theta = np.where(theta > np.pi / 2, theta - np.pi, theta)
    return np.where(theta <= -np.pi / 2, theta + np.pi, theta)


def svd2x2(F):
    """The closed-form singular value decomposition of F [npts, 2, 2] (or [npts, 4]) -> [npts, 4] = ln sigma1, ln sigma2, theta_in,
    theta_out with F = Rot(theta_out) diag(sigma1, sign(det) sigma2) Rot(theta_in)^T up to the overall sign.  F is divided by its
    largest |entry| s; E = (a + d) / 2, F = (a - d) / 2, G = (c + b) / 2, H = (c - b) / 2, Q = hypot(E, H), R = hypot(F, G),
    sigma1 = Q + R, sigma2 = |det| / sigma1, a1 = atan2(G, F), a2 = atan2(H, E), theta_out = (a2 + a1) / 2, theta_in = (a1 - a2) / 2, both
    folded into (-pi/2, pi/2].  s == 0: -inf, -inf, 0, 0; an entry that is not finite: NaN."""
    M = np.array(F, dtype=np.float64).reshape(-1, 4)
    out = np.full((M.shape[0], 4), np.nan)
    s = np.max(np.abs(M), axis=1)
    zero = s == 0.0
    out[zero] = (-np.inf, -np.inf, 0.0, 0.0)
    ok = np.isfinite(M).all(axis=1) & ~zero
    with np.errstate(divide="ignore"):
        m = M[ok] / s[ok, None]
        a, b, c, d = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
        E, Fm, G, H = (a + d) / 2, (a - d) / 2, (c + b) / 2, (c - b) / 2
        s1 = np.hypot(E, H) + np.hypot(Fm, G)
        s2 = np.abs(a * d - b * c) / s1
        a1, a2 = np.arctan2(G, Fm), np.arctan2(H, E)
        ls = np.log(s[ok])
        out[ok] = np.stack([np.log(s1) + ls, np.where(s2 > 0.0, np.log(s2) + ls, -np.inf), fold((a1 - a2) / 2), fold((a2 + a1) / 2)], axis=1)
    return out


def rot(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([np.stack([c, -s], axis=-1), np.stack([s, c], axis=-1)], axis=-2)


def reconstruct(table, F):
    """Rot(theta_out) diag(sigma1, sign(det F) sigma2) Rot(theta_in)^T of the rows of a stretching table, [npts, 2, 2], each in units of
    its own sigma1 (so that 1e200 F does not overflow): to be compared with +-F / sigma1"""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 2, 2)
    s = np.max(np.abs(F), axis=(1, 2))
    m = F / s[:, None, None]
    sg = np.sign(m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0])
    D = np.zeros_like(F)
    D[:, 0, 0] = 1.0
    D[:, 1, 1] = sg * np.exp(table[:, 1] - table[:, 0])
    return rot(table[:, 3]) @ D @ np.swapaxes(rot(table[:, 2]), 1, 2)


def hard_matrices():
    """(names, [n, 2, 2]): the matrices a 2 x 2 decomposition can go wrong on"""
    th = 0.7
    base = np.array([[2.0, 1.0], [1.0, 1.0]])
    cases = [("identity", np.eye(2)), ("rotation", rot(np.array(th))), ("det < 0", np.array([[1.0, 2.0], [3.0, -1.5]])),
             ("singular", np.array([[1.0, 2.0], [2.0, 4.0]])), ("zero", np.zeros((2, 2))), ("1e200", 1e200 * base), ("1e-200", 1e-200 * base),
             ("ratio 1e12", rot(np.array(0.3)) @ np.diag([1e6, 1e-6]) @ rot(np.array(-1.1)).T)]
    return [n for n, _ in cases], np.stack([m for _, m in cases])


def check_stretching(table, F, label=""):
    """the bars of the stretching table against numpy.linalg.svd, for svd2x2 and for the GPU kernel alike: both ln sigma within 1e-12
    (|ln sigma2| within 1e-4 where sigma1 / sigma2 >= 1e11: det carries the loss), ln sigma2 = -inf exactly where numpy's sigma2 is 0
    or below sigma1 eps64 / 4, and the reconstruction within 1e-12 sigma1, up to the sign, wherever sigma1 - sigma2 > 1e-8 sigma1.
    Returns the largest errors (ln sigma1, ln sigma2 at ordinary ratios, reconstruction / sigma1)."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 2, 2)
    s = np.max(np.abs(F), axis=(1, 2))
    worst = [0.0, 0.0, 0.0]
    for p in range(F.shape[0]):
        if s[p] == 0.0:
            assert np.array_equal(table[p], np.array([-np.inf, -np.inf, 0.0, 0.0])), (label, p, table[p])
            continue
        sv = np.linalg.svd(F[p] / s[p], compute_uv=False)
        e1 = abs(table[p, 0] - (np.log(sv[0]) + np.log(s[p])))
        assert e1 <= 1e-12, (label, p, e1)
        worst[0] = max(worst[0], e1)
        if sv[1] <= sv[0] * np.finfo(np.float64).eps / 4:
            assert table[p, 1] == -np.inf or table[p, 1] < table[p, 0] + np.log(np.finfo(np.float64).eps), (label, p, table[p])
        else:
            e2 = abs(table[p, 1] - (np.log(sv[1]) + np.log(s[p])))
            strong = sv[0] >= 1e11 * sv[1]
            assert e2 <= (1e-4 if strong else 1e-12), (label, p, e2)
            if not strong:
                worst[1] = max(worst[1], e2)
        assert -np.pi / 2 < table[p, 2] <= np.pi / 2 and -np.pi / 2 < table[p, 3] <= np.pi / 2, (label, p, table[p])
        if sv[0] - sv[1] > 1e-8 * sv[0]:
            rec = reconstruct(table[p:p + 1], F[p:p + 1])[0]
            m = F[p] / s[p] / sv[0]
            e3 = min(float(np.max(np.abs(rec - m))), float(np.max(np.abs(rec + m))))
            assert e3 <= 1e-12, (label, p, e3)
            worst[2] = max(worst[2], e3)
    return worst
