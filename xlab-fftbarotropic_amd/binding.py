"""ctypes binding of include/fftbaro.h (the C-ABI drop-in boundary).

Host-side mirror of the reference's operator interface: `FftwfOperation` carries the method
names of `fftwf_operation<XPTS,YPTS>` (fftwfop.hpp:9-29) and `Model` the surface of the
main.cpp RK4 driver.  Arrays on the GPU are torch tensors (device memory + streams only);
the compute is entirely in libfftbaro.so.  There is no CPU fallback: a missing library or a
missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_lib = None
# fb_alltoall_fn (include/fftbaro.h): user, send, recv, stride, offset, count, hip stream
ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p)


class FftBaroError(RuntimeError):
    pass


def lib():
    """Loads libfftbaro.so (building it if the sources are newer); raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime: it must be in the process before libfftbaro.so is
    # dlopen'ed, so that both resolve to ONE libamdhip64 (two runtimes cannot share a device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("FFTBARO_LIB") or _build.LIB      # developer hook: A/B a differently built library
    if path == _build.LIB and _build.stale():
        # atomic + locked (build.py): ranks of one job never see a half-written library.  A stale library that
        # cannot be rebuilt is an error -- tests must not run against old kernels (FFTBARO_ALLOW_STALE=1 overrides).
        try:
            _build.build_lib()
        except Exception as e:
            if not (os.environ.get("FFTBARO_ALLOW_STALE") and os.path.exists(path)):
                raise FftBaroError("libfftbaro.so is missing or stale and could not be rebuilt: %s" % e)
    L = C.CDLL(path)
    vp, fp, ip = C.c_void_p, C.c_void_p, C.c_int
    L.fb_strerror.restype = C.c_char_p
    L.fb_strerror.argtypes = [ip]
    L.fb_last_error.restype = C.c_char_p
    L.fb_version.restype = ip
    L.fb_size_supported.argtypes = [ip, ip]
    L.fb_device_count.argtypes = [C.POINTER(ip)]
    L.fb_set_device.argtypes = [ip]
    L.fb_create.argtypes = [C.POINTER(vp), ip, ip, C.c_float, C.c_float]
    L.fb_destroy.argtypes = [vp]
    L.fb_set_stream.argtypes = [vp, vp]
    L.fb_synchronize.argtypes = [vp]
    L.fb_get_tables.argtypes = [vp] + [C.c_void_p] * 5
    L.fb_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.fb_free.argtypes = [vp]
    L.fb_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.fb_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.fb_memset0.argtypes = [vp, vp, C.c_size_t]
    for n in ("fb_gradx", "fb_grady", "fb_laplacian", "fb_invert_laplacian", "fb_dealiase"):
        getattr(L, n).argtypes = [vp, fp, fp]
    L.fb_r2c.argtypes = [vp, fp, fp]
    L.fb_c2r.argtypes = [vp, fp, fp, ip]
    L.fb_backward_normalize.argtypes = [vp, fp]
    L.fb_negate.argtypes = [vp, fp]
    L.fb_jacobian.argtypes = [vp, fp, fp, fp, fp, fp, fp]
    L.fb_spec_axpy.argtypes = [vp, fp, fp, C.c_float]
    L.fb_spec_evolve.argtypes = [vp, fp, fp, C.c_float, fp]
    L.fb_spec_rk4_combine.argtypes = [vp, fp, fp, fp, fp, fp, C.c_float, fp]
    L.fb_model_create.argtypes = [C.POINTER(vp), vp, C.c_float, C.c_float]
    L.fb_model_destroy.argtypes = [vp]
    L.fb_model_set_vort.argtypes = [vp, fp]
    L.fb_model_set_source.argtypes = [vp, fp]
    L.fb_model_step.argtypes = [vp, ip]
    L.fb_model_use_graph.argtypes = [vp, ip]
    L.fb_model_get_vort.argtypes = [vp, fp]
    L.fb_model_get_diag.argtypes = [vp, fp, fp, fp]
    L.fb_model_get_okubo_weiss.argtypes = [vp, fp, fp]
    L.fb_model_get_eddy_diffusivity.argtypes = [vp, ip, vp, fp, fp]
    L.fb_model_get_spectrum.argtypes = [vp, fp]
    L.fb_model_set_spectrum.argtypes = [vp, fp]
    L.fb_model_info.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.fb_model_time_steps.argtypes = [vp, ip, C.POINTER(C.c_float)]
    L.fb_model_profile_steps.argtypes = [vp, ip, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.fb_make_field.argtypes = [C.c_char_p, ip, ip, C.c_float, C.c_float, C.c_void_p]
    L.fb_make_source_kuo2004.argtypes = [ip, ip, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.fb_create_slab.argtypes = [C.POINTER(vp), ip, ip, C.c_float, C.c_float, ip, ip]
    L.fb_slab_unique_id.argtypes = [C.c_char_p]
    L.fb_slab_create.argtypes = [C.POINTER(vp), ip, ip, C.c_float, C.c_float, C.c_float, C.c_float, ip, ip]
    L.fb_slab_destroy.argtypes = [vp]
    L.fb_slab_connect_rccl.argtypes = [vp, C.c_char_p]
    L.fb_local_hub_create.argtypes = [C.POINTER(vp), ip]
    L.fb_local_hub_destroy.argtypes = [vp]
    L.fb_slab_connect_local.argtypes = [vp, vp]
    L.fb_slab_connect_callback.argtypes = [vp, ALLTOALL_FN, vp]
    L.fb_slab_set_vort_local.argtypes = [vp, fp]
    L.fb_slab_set_source_local.argtypes = [vp, fp]
    L.fb_slab_get_vort_local.argtypes = [vp, fp]
    L.fb_slab_get_diag_local.argtypes = [vp, fp, fp, fp]
    L.fb_slab_get_okubo_weiss_local.argtypes = [vp, fp, fp]
    L.fb_slab_get_eddy_diffusivity.argtypes = [vp, ip, vp, fp, fp]
    # (an older build chosen through FFTBARO_LIB for an A/B run lacks the pressure record: calling it there is an AttributeError)
    for n in ("fb_model_get_pressure", "fb_slab_get_pressure_local"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, C.c_float, C.c_float, ip, ip, fp]
    # (likewise the spectra record)
    for n in ("fb_model_get_spectra", "fb_slab_get_spectra"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, vp]
    if hasattr(L, "fb_spectra_shells"):
        L.fb_spectra_shells.argtypes = [ip, ip, C.c_float, C.c_float, C.POINTER(ip)]
    # (likewise the passive tracer)
    for n in ("fb_model_set_tracer", "fb_slab_set_tracer_local"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, fp, C.c_float]
    for n in ("fb_model_get_tracer", "fb_slab_get_tracer_local"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, fp]
    for n in ("fb_model_get_tracer_eddy_diffusivity", "fb_slab_get_tracer_eddy_diffusivity"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, ip, vp, fp, fp]
    # (likewise the azimuthal-mean record)
    for n in ("fb_model_get_azimuthal", "fb_slab_get_azimuthal"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, ip, C.c_double, C.c_double, ip, C.c_double, ip, vp, vp]
    if hasattr(L, "fb_azimuthal_cols"):
        L.fb_azimuthal_cols.argtypes = [ip, C.POINTER(ip)]
    # (likewise the Lagrangian particles)
    for n in ("fb_model_set_particles", "fb_slab_set_particles"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, vp, ip]
    for n in ("fb_model_get_particles", "fb_slab_get_particles"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, vp]
    for n in ("fb_model_particle_count", "fb_slab_particle_count"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, C.POINTER(ip)]
    for n in ("fb_model_sample", "fb_slab_sample"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, fp, vp, ip, vp]
    # (likewise the tangent-linear model)
    for n in ("fb_model_set_tangent", "fb_model_get_tangent", "fb_slab_set_tangent", "fb_slab_get_tangent"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, fp]
    for n in ("fb_model_tangent_norm", "fb_slab_tangent_norm"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, ip, vp]
    for n in ("fb_model_tangent_scale", "fb_slab_tangent_scale"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, C.c_float]
    # (likewise the adjoint model)
    for n in ("fb_model_adjoint_record", "fb_model_adjoint_back", "fb_slab_adjoint_record", "fb_slab_adjoint_back"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, ip]
    for n in ("fb_model_adjoint_recorded", "fb_slab_adjoint_recorded"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, C.POINTER(ip)]
    for n in ("fb_model_set_adjoint", "fb_model_get_adjoint", "fb_slab_set_adjoint", "fb_slab_get_adjoint"):
        if hasattr(L, n):
            getattr(L, n).argtypes = [vp, fp]
    L.fb_slab_step.argtypes = [vp, ip]
    L.fb_slab_synchronize.argtypes = [vp]
    L.fb_slab_time_steps.argtypes = [vp, ip, C.POINTER(C.c_float)]
    L.fb_slab_transport_selftest.argtypes = [vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.fb_slab_info.argtypes = [vp] + [C.POINTER(ip)] * 7
    L.fb_slab_transport_info.argtypes = [vp, C.c_char_p, C.c_size_t] + [C.POINTER(ip)] * 4
    L.fb_slab_geometry.argtypes = [ip, ip, ip] + [C.POINTER(ip)] * 3
    L.fb_slab_plan.argtypes = [ip, ip, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), ip]
    L.fb_write_field.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    L.fb_read_field.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    _lib = L
    return L


EXPORTS = [
    "fb_strerror", "fb_last_error", "fb_version", "fb_size_supported", "fb_device_count", "fb_set_device", "fb_create", "fb_destroy", "fb_set_stream",
    "fb_synchronize", "fb_get_tables", "fb_malloc", "fb_free", "fb_memcpy_h2d", "fb_memcpy_d2h", "fb_memset0",
    "fb_gradx", "fb_grady", "fb_laplacian", "fb_invert_laplacian", "fb_dealiase", "fb_r2c", "fb_c2r",
    "fb_backward_normalize", "fb_negate", "fb_jacobian", "fb_spec_axpy", "fb_spec_evolve", "fb_spec_rk4_combine",
    "fb_model_create", "fb_model_destroy", "fb_model_set_vort", "fb_model_set_source", "fb_model_step",
    "fb_model_use_graph", "fb_model_get_vort", "fb_model_get_diag", "fb_model_get_okubo_weiss", "fb_model_get_eddy_diffusivity", "fb_model_get_pressure", "fb_model_get_spectra", "fb_spectra_shells", "fb_model_get_spectrum", "fb_model_set_spectrum", "fb_model_info",
    "fb_model_time_steps", "fb_model_profile_steps", "fb_write_field", "fb_read_field", "fb_make_field", "fb_make_source_kuo2004",
    "fb_create_slab", "fb_slab_unique_id", "fb_slab_create", "fb_slab_destroy", "fb_slab_connect_rccl", "fb_local_hub_create",
    "fb_local_hub_destroy", "fb_slab_connect_local", "fb_slab_connect_callback", "fb_slab_set_vort_local", "fb_slab_set_source_local",
    "fb_slab_get_vort_local", "fb_slab_get_diag_local", "fb_slab_get_okubo_weiss_local", "fb_slab_get_eddy_diffusivity", "fb_slab_get_pressure_local", "fb_slab_get_spectra", "fb_slab_step", "fb_slab_synchronize", "fb_slab_time_steps", "fb_slab_transport_selftest", "fb_slab_transport_info", "fb_slab_info", "fb_slab_geometry", "fb_slab_plan", "fb_slab_col_groups",
    "fb_malloc_host", "fb_free_host", "fb_stream_create", "fb_stream_destroy", "fb_stream_synchronize", "fb_event_create", "fb_event_create_timing", "fb_event_elapsed_ms",
    "fb_model_set_tracer", "fb_model_get_tracer", "fb_model_get_tracer_eddy_diffusivity", "fb_slab_set_tracer_local", "fb_slab_get_tracer_local", "fb_slab_get_tracer_eddy_diffusivity",
    "fb_azimuthal_cols", "fb_model_get_azimuthal", "fb_slab_get_azimuthal",
    "fb_model_set_particles", "fb_model_get_particles", "fb_model_particle_count", "fb_model_sample",
    "fb_slab_set_particles", "fb_slab_get_particles", "fb_slab_particle_count", "fb_slab_sample",
    "fb_model_set_tangent", "fb_model_get_tangent", "fb_model_tangent_norm", "fb_model_tangent_scale",
    "fb_slab_set_tangent", "fb_slab_get_tangent", "fb_slab_tangent_norm", "fb_slab_tangent_scale",
    "fb_model_adjoint_record", "fb_model_adjoint_recorded", "fb_model_set_adjoint", "fb_model_get_adjoint", "fb_model_adjoint_back",
    "fb_slab_adjoint_record", "fb_slab_adjoint_recorded", "fb_slab_set_adjoint", "fb_slab_get_adjoint", "fb_slab_adjoint_back",
    "fb_event_destroy", "fb_event_record", "fb_stream_wait_event", "fb_event_synchronize", "fb_memcpy_d2h_async", "fb_memcpy_h2d_async", "fb_slab_record_event", "fb_slab_wait_event",
]


def check(status):
    if status != 0:
        L = lib()
        raise FftBaroError("%s: %s" % (L.fb_strerror(status).decode(), L.fb_last_error().decode()))


# the columns of the effective eddy diffusivity table (fb_model_get_eddy_diffusivity, include/fftbaro.h), one row per bin of zeta
EDDY_DIFFUSIVITY_COLUMNS = ("Q_lo", "Q_hi", "n", "A", "A_ge", "S", "Le2", "r_e", "K_eff")

# the columns of the shell spectra table (fb_model_get_spectra, include/fftbaro.h), one row per wavenumber shell
SPECTRA_COLUMNS = ("k_lo", "k_hi", "n", "E", "Z", "T_E", "T_Z", "Pi_E", "Pi_Z", "D_Z")


def spectra_shells(nx, ny=None, Lx=600000.0, Ly=600000.0):
    """The number of wavenumber shells (rows) of the spectra table of an nx x ny grid on an Lx x Ly domain; host logic, no GPU."""
    n = C.c_int()
    check(lib().fb_spectra_shells(nx, ny or nx, Lx, Ly, C.byref(n)))
    return n.value


# the first twelve columns of the azimuthal-mean table (fb_model_get_azimuthal, include/fftbaro.h), one row per radial bin; then
# Re, Im of the azimuthal Fourier coefficient of zeta for m = 1 .. nmodes
AZIMUTHAL_COLUMNS = ("r_lo", "r_hi", "n", "r", "zeta", "v_t", "v_r", "zeta2", "v_t2", "v_r2", "v_r_zeta", "Gamma")
CENTER_MODES = {"fixed": 0, "psi-min": 1, "vort-max": 2}


def azimuthal_cols(nmodes):
    """The number of columns of the azimuthal-mean table with nmodes azimuthal wavenumbers, 12 + 2 nmodes; host logic, no GPU."""
    n = C.c_int()
    check(lib().fb_azimuthal_cols(nmodes, C.byref(n)))
    return n.value


def azimuthal_args(nx, ny, Lx, Ly, center, nbins, dr):
    """(mode, xc, yc, nbins, dr) of an azimuthal() call: center "psi-min" | "vort-max" | (xc, yc); the defaults dr = max(dx, dy) and
    nbins = floor(min(Lx, Ly) / 2 / dr), at most 4096, with dx, dy from the float32 lengths as the engine takes them."""
    lx, ly = float(np.float32(Lx)), float(np.float32(Ly))
    if isinstance(center, str):
        if center not in ("psi-min", "vort-max"):
            raise ValueError("center: 'psi-min', 'vort-max' or (xc, yc)")
        mode, xc, yc = CENTER_MODES[center], 0.0, 0.0
    else:
        mode, (xc, yc) = 0, center
    if dr is None:
        dr = max(lx / nx, ly / ny)
    if nbins is None:
        nbins = min(4096, int(np.floor(min(lx, ly) / 2 / dr))) if dr > 0 else 0
        while nbins > 2 and nbins * dr > min(lx, ly) / 2:
            nbins -= 1
    return mode, float(xc), float(yc), int(nbins), float(dr)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise FftBaroError("no GPU visible: the engine has no CPU fallback")
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr())


PARTICLES_MAX = 1 << 24
TANGENT_NORMS = {"enstrophy": 0, "energy": 1}


def tangent_kind(kind):
    """the C ABI's number of a tangent norm: "enstrophy" | "energy" (an int is passed on for the engine to judge)"""
    if isinstance(kind, str):
        if kind not in TANGENT_NORMS:
            raise ValueError("kind: 'enstrophy' or 'energy'")
        return TANGENT_NORMS[kind]
    return int(kind)


def lyapunov(model, steps, renorm_every, kind="enstrophy"):
    """Steps `model` (anything with step, tangent_norm, rescale_tangent and dt) by `steps` steps; after every renorm_every steps the
    perturbation is rescaled to the norm it had at the call.  Returns (the sum of ln(growth factors) / (steps dt) [s^-1], the list of
    the growth factors sqrt(norm after / norm before) per interval)."""
    if steps < 1 or renorm_every < 1:
        raise ValueError("lyapunov: steps and renorm_every must be >= 1")
    n0 = model.tangent_norm(kind)
    if not (n0 > 0.0 and np.isfinite(n0)):
        raise FftBaroError("lyapunov: the tangent's norm is %r" % n0)
    before, total, factors, done = n0, 0.0, [], 0
    while done < steps:
        k = min(renorm_every, steps - done)
        model.step(k)
        done += k
        after = model.tangent_norm(kind)
        g = float(np.sqrt(after / before))
        factors.append(g)
        total += 0.5 * float(np.log(after / before))
        model.rescale_tangent(float(np.sqrt(n0 / after)))
        before = model.tangent_norm(kind)
    return total / (steps * model.dt), factors


def singular_values(model, steps, iters, start, save=None, restore=None):
    """Power iteration on T^T T in the L2 (enstrophy) norm on `model` (anything with set_tangent, tangent, record_adjoint, step,
    set_adjoint, adjoint_back, adjoint; save / restore: how its state is kept and put back, by default spectrum / set_spectrum,
    which restores every bit), T the tangent of `steps` steps from the model's current state.  Each
    iteration restores that state, sets the tangent to the unit vector v (from `start`, an [nx, ny] field), steps with recording on,
    sets lam = T v, sweeps back and normalises v = T^T T v.  Returns (sigma = |T v| per iteration, the final v as a tensor); the model
    is left at its starting state with the tape freed, the tangent set to the last v and lam to T^T T of it."""
    if steps < 1 or iters < 1:
        raise ValueError("singular_values: steps and iters must be >= 1")
    t = model.torch
    save, restore = save or model.spectrum, restore or model.set_spectrum
    z0 = save()
    if isinstance(start, np.ndarray):
        start = t.from_numpy(np.ascontiguousarray(start, dtype=np.float64))
    v = start.cuda().double()
    v = v / v.norm()
    sig = []
    model.record_adjoint(steps)
    try:
        for _ in range(iters):
            restore(z0)
            model.set_tangent(v.float().contiguous())
            model.step(steps)
            w = model.tangent()
            t.cuda.current_stream().synchronize()
            sig.append(float(w.double().norm()))
            model.set_adjoint(w)
            model.adjoint_back(steps)
            v = model.adjoint().double()
            v = v / v.norm()
        restore(z0)
    finally:
        model.record_adjoint(0)
    return sig, v.float()


def particles_dev(torch, xy):
    """Particle positions, numpy or torch float64 [n, 2], as a contiguous tensor on the GPU that has landed there."""
    if isinstance(xy, np.ndarray):
        xy = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float64))
    if xy.dtype != torch.float64 or xy.dim() != 2 or xy.shape[1] != 2:
        raise ValueError("particle positions: float64 [n, 2]")
    xy = xy.cuda().contiguous()
    torch.cuda.current_stream().synchronize()                   # the engine reads them on ITS stream
    return xy


def wrap_positions(torch, xy, Lx, Ly):
    """Unwrapped positions [n, 2] folded into [0, Lx) x [0, Ly), the float32 lengths widened as the engine takes them."""
    out = torch.empty_like(xy)
    for k, L in enumerate((float(np.float32(Lx)), float(np.float32(Ly)))):
        r = torch.remainder(xy[:, k], L)
        out[:, k] = torch.where(r >= L, torch.zeros_like(r), r)     # (a tiny negative position folds to L itself in rounding)
    return out


class FftwfOperation:
    """Mirror of `fftwf_operation<XPTS,YPTS>` (fftwfop.hpp:9-29) on device buffers.

    Spectra are torch complex64 tensors [nx, ny/2+1] on the GPU; `in is out` is allowed.
    """

    def __init__(self, nx, ny, Lx, Ly, stream=None):
        self.torch = _torch()
        self.nx, self.ny, self.hy = nx, ny, ny // 2 + 1
        h = C.c_void_p()
        check(lib().fb_create(C.byref(h), nx, ny, Lx, Ly))
        self._h = h
        self.use_current_stream()

    def use_current_stream(self):
        s = self.torch.cuda.current_stream().cuda_stream
        check(lib().fb_set_stream(self._h, C.c_void_p(s)))

    def close(self):
        if getattr(self, "_h", None):
            lib().fb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def empty_spec(self):
        return self.torch.empty((self.nx, self.hy), dtype=self.torch.complex64, device="cuda")

    def empty_real(self):
        return self.torch.empty((self.nx, self.ny), dtype=self.torch.float32, device="cuda")

    def _spec(self, t):
        assert t.is_cuda and t.dtype == self.torch.complex64 and t.is_contiguous() and tuple(t.shape) == (self.nx, self.hy)
        return _ptr(t)

    def _real(self, t):
        assert t.is_cuda and t.dtype == self.torch.float32 and t.is_contiguous() and tuple(t.shape) == (self.nx, self.ny)
        return _ptr(t)

    def _op(self, fn, a, out):
        out = self.empty_spec() if out is None else out
        check(fn(self._h, self._spec(a), self._spec(out)))
        return out

    # -- fftwfop.hpp:20-24
    def gradx(self, a, out=None): return self._op(lib().fb_gradx, a, out)
    def grady(self, a, out=None): return self._op(lib().fb_grady, a, out)
    def laplacian(self, a, out=None): return self._op(lib().fb_laplacian, a, out)
    def invertLaplacian(self, a, out=None): return self._op(lib().fb_invert_laplacian, a, out)
    def dealiase(self, a, out=None): return self._op(lib().fb_dealiase, a, out)

    # -- fftwfop.hpp:26-28
    def reflectedXWavenumberIndex(self, i):
        assert i >= 1
        return self.nx - i

    def HIDX(self, i, j): return self.hy * i + j
    def R_HIDX(self, i, j): return self.HIDX(self.reflectedXWavenumberIndex(i), j)

    # -- what the driver takes from FFTW (main.cpp:126-135,154,...)
    def r2c(self, real, out=None):
        out = self.empty_spec() if out is None else out
        check(lib().fb_r2c(self._h, self._real(real), self._spec(out)))
        return out

    def c2r(self, spec, out=None, normalize=False):
        out = self.empty_real() if out is None else out
        check(lib().fb_c2r(self._h, self._spec(spec), self._real(out), 1 if normalize else 0))
        return out

    # -- driver lambdas
    def backward_normalize(self, real): check(lib().fb_backward_normalize(self._h, self._real(real))); return real
    def negate(self, real): check(lib().fb_negate(self._h, self._real(real))); return real

    def jacobian(self, u, v, dzdx, dzdy, src=None, out=None):
        out = self.empty_real() if out is None else out
        check(lib().fb_jacobian(self._h, self._real(u), self._real(v), self._real(dzdx), self._real(dzdy),
                                self._real(src) if src is not None else None, self._real(out)))
        return out

    def spec_axpy(self, acc, x, a): check(lib().fb_spec_axpy(self._h, self._spec(acc), self._spec(x), a)); return acc

    def spec_evolve(self, base, rk, a, out=None):
        out = self.empty_spec() if out is None else out
        check(lib().fb_spec_evolve(self._h, self._spec(base), self._spec(rk), a, self._spec(out)))
        return out

    def spec_rk4_combine(self, base, k1, k2, k3, k4, dt, out=None):
        out = self.empty_spec() if out is None else out
        check(lib().fb_spec_rk4_combine(self._h, self._spec(base), self._spec(k1), self._spec(k2), self._spec(k3),
                                        self._spec(k4), dt, self._spec(out)))
        return out

    def tables(self):
        n, h = self.nx, self.hy
        gx = np.empty(n, np.float32); gy = np.empty(h, np.float32)
        lap = np.empty((n, h), np.float32); lapi = np.empty((n, h), np.float32); mask = np.empty((n, h), np.float32)
        check(lib().fb_get_tables(self._h, gx.ctypes.data, gy.ctypes.data, lap.ctypes.data, lapi.ctypes.data, mask.ctypes.data))
        return gx, gy, lap, lapi, mask

    def synchronize(self): check(lib().fb_synchronize(self._h))


class Model:
    """The main.cpp RK4 driver state (main.cpp:103-317) resident in HBM, fused stepping."""

    def __init__(self, nx, ny=None, Lx=600000.0, Ly=600000.0, nu=6.5, dt=3.0):
        ny = ny or nx
        self.fop = FftwfOperation(nx, ny, Lx, Ly)
        self.torch = self.fop.torch
        self.nx, self.ny, self.hy = nx, ny, ny // 2 + 1
        self.Lx, self.Ly = Lx, Ly
        self.nu, self.dt = float(np.float32(nu)), float(np.float32(dt))
        h = C.c_void_p()
        check(lib().fb_model_create(C.byref(h), self.fop._h, nu, dt))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().fb_model_destroy(self._h)
            self._h = None
        self.fop.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, a):
        t = self.torch
        if isinstance(a, np.ndarray):
            a = t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        assert a.is_cuda and a.dtype == t.float32 and a.is_contiguous() and tuple(a.shape) == (self.nx, self.ny)
        # the engine reads the buffer on ITS stream: whatever torch still has queued for it (a fill, a copy) must have landed
        t.cuda.current_stream().synchronize()
        return a

    def set_vort(self, vort): a = self._dev(vort); check(lib().fb_model_set_vort(self._h, _ptr(a))); self.fop.synchronize()

    def set_source(self, src):
        if src is None:
            check(lib().fb_model_set_source(self._h, None))
        else:
            a = self._dev(src); check(lib().fb_model_set_source(self._h, _ptr(a))); self.fop.synchronize()

    def step(self, n=1): check(lib().fb_model_step(self._h, n))

    def use_graph(self, enable=True):
        """hipGraph replay of the step; call under a non-default torch stream (after fop.use_current_stream())."""
        check(lib().fb_model_use_graph(self._h, 1 if enable else 0))

    def time_steps(self, n):
        ms = C.c_float()
        check(lib().fb_model_time_steps(self._h, n, C.byref(ms)))
        return ms.value

    KERNEL_CLASSES = ("k_col_strided_bwd4", "k_row_fused", "k_col_strided_fwd1", "k_col_mid")

    def profile_steps(self, n):
        """HIP-event time per kernel class over n steps: {class: (total_ms, launches)}."""
        ms = (C.c_float * 4)(); cnt = (C.c_int * 4)()
        check(lib().fb_model_profile_steps(self._h, n, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNEL_CLASSES)}

    def vort(self):
        out = self.fop.empty_real(); check(lib().fb_model_get_vort(self._h, _ptr(out))); return out

    def diag(self):
        psi, u, v = self.fop.empty_real(), self.fop.empty_real(), self.fop.empty_real()
        check(lib().fb_model_get_diag(self._h, _ptr(psi), _ptr(u), _ptr(v)))
        return psi, u, v

    def okubo_weiss(self):
        """(W, tau_fil): the Okubo-Weiss parameter [s^-2] and the filamentation time [s] (+inf where W <= 0), [nx, ny] tensors."""
        w, tau = self.fop.empty_real(), self.fop.empty_real()
        check(lib().fb_model_get_okubo_weiss(self._h, _ptr(w), _ptr(tau)))
        return w, tau

    def eddy_diffusivity(self, nbins=256, fields=False):
        """The effective eddy diffusivity table, float64 [nbins, 9] (columns EDDY_DIFFUSIVITY_COLUMNS), of the vorticity binned in
        nbins contour intervals; with fields=True also (zeta, grad2): the vorticity and |grad zeta|^2, [nx, ny] tensors."""
        t = self.torch
        table = t.empty((nbins, 9), dtype=t.float64, device="cuda")
        zeta, g = (self.fop.empty_real(), self.fop.empty_real()) if fields else (None, None)
        check(lib().fb_model_get_eddy_diffusivity(self._h, nbins, _ptr(table), _ptr(zeta) if fields else None, _ptr(g) if fields else None))
        return (table, zeta, g) if fields else table

    def pressure(self, rho=1.0, f=1e-5, ref=(0, 0)):
        """The nonlinear-balance pressure of the current state (invert_pres.cpp:135-185), an [nx, ny] tensor, minus its value at the
        reference point ref = (ref_x, ref_y): the element ref_x + nx * ref_y of the flattened field, as the reference indexes it."""
        out = self.fop.empty_real()
        check(lib().fb_model_get_pressure(self._h, rho, f, int(ref[0]), int(ref[1]), _ptr(out)))
        return out

    def spectra(self):
        """The shell spectra and cascade fluxes of the current state, float64 [nshells, 10] (columns SPECTRA_COLUMNS): energy and
        enstrophy spectra, advective transfers and fluxes, enstrophy dissipation per wavenumber shell."""
        t = self.torch
        table = t.empty((spectra_shells(self.nx, self.ny, self.Lx, self.Ly), 10), dtype=t.float64, device="cuda")
        check(lib().fb_model_get_spectra(self._h, _ptr(table)))
        return table

    def azimuthal(self, center="psi-min", nbins=None, dr=None, nmodes=4):
        """(table, center): the azimuthal means about a vortex centre (fb_model_get_azimuthal).  center: "psi-min" (grid point of the
        smallest psi), "vort-max" (of the largest zeta) or a fixed (xc, yc) [m]; nbins radial bins of the width dr [m] (defaults:
        dr = max(dx, dy), nbins = floor(min(Lx, Ly) / 2 / dr), at most 4096); table float64 [nbins, 12 + 2 nmodes] (columns
        AZIMUTHAL_COLUMNS, then Re, Im of the azimuthal wavenumbers 1 .. nmodes of zeta), center float64 [4] = xc, yc, flat index,
        value; both on the GPU."""
        t = self.torch
        mode, xc, yc, nbins, dr = azimuthal_args(self.nx, self.ny, self.Lx, self.Ly, center, nbins, dr)
        table = t.empty((max(nbins, 0), 12 + 2 * max(int(nmodes), 0)), dtype=t.float64, device="cuda")
        cen = t.empty(4, dtype=t.float64, device="cuda")
        t.cuda.current_stream().synchronize()                   # the engine writes them on ITS stream
        check(lib().fb_model_get_azimuthal(self._h, mode, xc, yc, nbins, dr, int(nmodes), _ptr(table), _ptr(cen)))
        return table, cen

    def set_tracer(self, c, kappa=0.0):
        """Sets the passive tracer, an [nx, ny] field advected by the model's flow with the diffusivity kappa [m^2 s^-1] (it is stepped
        beside the vorticity from now on); c=None removes it."""
        if c is None:
            check(lib().fb_model_set_tracer(self._h, None, 0.0))
        else:
            a = self._dev(c); check(lib().fb_model_set_tracer(self._h, _ptr(a), float(kappa))); self.fop.synchronize()

    def tracer(self):
        out = self.fop.empty_real(); check(lib().fb_model_get_tracer(self._h, _ptr(out))); return out

    def tracer_eddy_diffusivity(self, nbins=256, fields=False):
        """eddy_diffusivity() of the passive tracer, with its kappa in the place of nu; with fields=True also (c, |grad c|^2)."""
        t = self.torch
        table = t.empty((nbins, 9), dtype=t.float64, device="cuda")
        c, g = (self.fop.empty_real(), self.fop.empty_real()) if fields else (None, None)
        check(lib().fb_model_get_tracer_eddy_diffusivity(self._h, nbins, _ptr(table), _ptr(c) if fields else None, _ptr(g) if fields else None))
        return (table, c, g) if fields else table

    def set_particles(self, xy):
        """Sets the Lagrangian particles, float64 [n, 2] positions (x, y) [m] (numpy or torch), advected by the model's flow from now
        on with the RK4 scheme of the step itself; xy=None removes them."""
        if xy is None:
            check(lib().fb_model_set_particles(self._h, None, 0))
        else:
            a = particles_dev(self.torch, xy)
            check(lib().fb_model_set_particles(self._h, _ptr(a), int(a.shape[0]))); self.fop.synchronize()

    def particle_count(self):
        n = C.c_int()
        check(lib().fb_model_particle_count(self._h, C.byref(n)))
        return n.value

    def particles(self, wrap=False):
        """The particles' positions, a float64 [n, 2] tensor: unwrapped (a particle that left through one side keeps counting), or with
        wrap=True folded into [0, Lx) x [0, Ly)."""
        t = self.torch
        out = t.empty((max(self.particle_count(), 1), 2), dtype=t.float64, device="cuda")
        t.cuda.current_stream().synchronize()                   # the engine writes them on ITS stream
        check(lib().fb_model_get_particles(self._h, _ptr(out)))
        self.fop.synchronize()
        return wrap_positions(t, out, self.Lx, self.Ly) if wrap else out

    def sample(self, field, xy=None):
        """An [nx, ny] float32 field (numpy or torch: the vorticity, the tracer, W, the pressure ...) interpolated to the positions
        xy, float64 [n, 2], or to the particles (xy=None), by the particles' cubic Lagrange scheme: a float64 [n] tensor."""
        t = self.torch
        f = self._dev(field)
        a = self.particles() if xy is None else particles_dev(t, xy)
        out = t.empty(a.shape[0], dtype=t.float64, device="cuda")
        t.cuda.current_stream().synchronize()
        check(lib().fb_model_sample(self._h, _ptr(f), _ptr(a), int(a.shape[0]), _ptr(out)))
        self.fop.synchronize()
        return out

    def set_tangent(self, dz):
        """Sets the perturbation of the tangent-linear model, an [nx, ny] field carried along the evolving vorticity by the
        linearisation of the step itself (it is stepped beside the vorticity from now on); dz=None removes it."""
        if dz is None:
            check(lib().fb_model_set_tangent(self._h, None))
        else:
            a = self._dev(dz); check(lib().fb_model_set_tangent(self._h, _ptr(a))); self.fop.synchronize()

    def tangent(self):
        out = self.fop.empty_real(); check(lib().fb_model_get_tangent(self._h, _ptr(out))); return out

    def tangent_norm(self, kind="enstrophy"):
        """The perturbation's norm, a float: "enstrophy" <dz^2> / 2 or "energy" <|grad dpsi|^2> / 2, summed in float64 on the GPU."""
        t = self.torch
        out = t.empty(1, dtype=t.float64, device="cuda")
        t.cuda.current_stream().synchronize()                   # the engine writes it on ITS stream
        check(lib().fb_model_tangent_norm(self._h, tangent_kind(kind), _ptr(out)))
        self.fop.synchronize()
        return float(out.item())

    def rescale_tangent(self, a):
        """dz *= a (a finite and not zero)"""
        check(lib().fb_model_tangent_scale(self._h, float(a)))

    def lyapunov(self, steps, renorm_every, kind="enstrophy"):
        """(exponent [s^-1], growth factors): steps the model, renormalising the perturbation every renorm_every steps (lyapunov())."""
        return lyapunov(self, steps, renorm_every, kind)

    def record_adjoint(self, depth):
        """Turns the adjoint's tape on (depth >= 1: room for depth steps; every step from now on records its four stage states, and a
        step call beyond depth is refused) or off (depth = 0, the tape freed).  Either way the tape starts empty."""
        check(lib().fb_model_adjoint_record(self._h, int(depth)))

    def adjoint_recorded(self):
        n = C.c_int()
        check(lib().fb_model_adjoint_recorded(self._h, C.byref(n)))
        return n.value

    def set_adjoint(self, lam):
        """Sets the adjoint variable, an [nx, ny] field (the gradient of a scalar of the state with respect to the vorticity, at the
        time of the newest recorded step); lam=None removes it."""
        if lam is None:
            check(lib().fb_model_set_adjoint(self._h, None))
        else:
            a = self._dev(lam); check(lib().fb_model_set_adjoint(self._h, _ptr(a))); self.fop.synchronize()

    def adjoint(self):
        out = self.fop.empty_real(); check(lib().fb_model_get_adjoint(self._h, _ptr(out))); return out

    def adjoint_back(self, n=1):
        """lam <- T^T lam over the last n recorded steps, newest first (the transpose of the tangent-linear step); they leave the tape."""
        check(lib().fb_model_adjoint_back(self._h, int(n)))

    def singular_values(self, steps, iters, start):
        """(sigmas, v): power iteration on T^T T over `steps` steps from the current state in the L2 norm (singular_values())."""
        return singular_values(self, steps, iters, start)

    def spectrum(self):
        out = self.fop.empty_spec(); check(lib().fb_model_get_spectrum(self._h, _ptr(out))); return out

    def set_spectrum(self, spec): check(lib().fb_model_set_spectrum(self._h, self.fop._spec(spec)))

    def info(self):
        a, b = C.c_size_t(), C.c_size_t()
        check(lib().fb_model_info(self._h, C.byref(a), C.byref(b)))
        return {"hbm_bytes": a.value, "alg_bytes_per_step": b.value}


def write_field(path, data):
    data = np.ascontiguousarray(data, dtype=np.float32)
    check(lib().fb_write_field(path.encode(), data.ctypes.data, data.size))


def read_field(path, n):
    out = np.empty(n, dtype=np.float32)
    check(lib().fb_read_field(path.encode(), out.ctypes.data, n))
    return out


def make_field(kind, nx, ny=None, Lx=600000.0, Ly=600000.0):
    """Host-side initial vorticity (makefield-*.cpp restated with run-time grid size)."""
    ny = ny or nx
    out = np.empty((nx, ny), dtype=np.float32)
    check(lib().fb_make_field(kind.encode(), nx, ny, Lx, Ly, out.ctypes.data))
    return out


def make_source_kuo2004(nx, ny=None, Lx=600000.0, Ly=600000.0, duration=10800.0):
    ny = ny or nx
    out = np.empty((nx, ny), dtype=np.float32)
    check(lib().fb_make_source_kuo2004(nx, ny, Lx, Ly, duration, out.ctypes.data))
    return out
