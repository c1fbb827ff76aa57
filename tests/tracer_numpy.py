"""float64 numpy reference of the coupled system vorticity + passive tracer: ref_numpy.Model64 extended by a tracer c with a
diffusivity kappa of its own.  Each RK4 stage computes the tracer's tendency with the streamfunction of the vorticity's state of
that stage,

    tend_c = mask * ( r2c(-u c_x - v c_y) + kappa * laplacian_coe * c_c ),   u = -psi_y, v = psi_x, psi_c = vort_c / laplacian_coe

in the formula order of ref_numpy.Model64.tendency with c in the place of zeta and no source.  Used ONLY by tests."""
import numpy as np

from ref_numpy import Model64


class TracerModel64(Model64):
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

    def step(self, n=1):
        dt = self.dt
        for _ in range(n):
            v0, c0 = self.vc, self.cc
            k1, l1 = self.tendency(v0), self.tracer_tendency(v0, c0)
            v1, c1 = v0 + k1 * (dt / 2), c0 + l1 * (dt / 2)
            k2, l2 = self.tendency(v1), self.tracer_tendency(v1, c1)
            v2, c2 = v0 + k2 * (dt / 2), c0 + l2 * (dt / 2)
            k3, l3 = self.tendency(v2), self.tracer_tendency(v2, c2)
            v3, c3 = v0 + k3 * dt, c0 + l3 * dt
            k4, l4 = self.tendency(v3), self.tracer_tendency(v3, c3)
            self.vc = v0 + (k1 + 2 * k2 + 2 * k3 + k4) * dt / 6
            self.cc = c0 + (l1 + 2 * l2 + 2 * l3 + l4) * dt / 6

    def tracer(self):
        return self._c2r(self.cc)


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
