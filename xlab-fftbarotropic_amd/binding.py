"""ctypes binding of include/fftbaro.h (the C-ABI drop-in boundary).

Host-side mirror of the reference's operator interface: `FftwfOperation` carries the method
names of `fftwf_operation<XPTS,YPTS>` (fftwfop.hpp:9-29) and `Model` the surface of the
main.cpp RK4 driver.  Arrays on the GPU are torch tensors (device memory + streams only);
the compute is entirely in libfftbaro.so.  There is no CPU fallback: a missing library or a
missing GPU raises.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np

from . import build as _build

_lib = None
# fb_alltoall_fn (include/fftbaro.h): user, send, recv, stride, offset, count, hip stream
ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p)


class FftBaroError(RuntimeError):
    pass


# The C ABI of include/fftbaro.h: name -> (argtypes, restype; None: the int status).  A data pointer is a c_void_p (it takes byref(...),
# ctypes arrays and buffers, bytes, None, ints and c_void_p alike), or a POINTER(...) where the callers pass byref.
_vp, _ip, _fl, _db, _sz, _cp = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_char_p
_pvp, _pip, _pfl, _psz = C.POINTER(_vp), C.POINTER(_ip), C.POINTER(_fl), C.POINTER(_sz)
SIGNATURES = {
    "fb_strerror": ([_ip], _cp), "fb_last_error": ([], _cp), "fb_version": ([], None),
    "fb_device_count": ([_pip], None), "fb_set_device": ([_ip], None), "fb_size_supported": ([_ip, _ip], None),
    "fb_create": ([_pvp, _ip, _ip, _fl, _fl], None), "fb_destroy": ([_vp], None),
    "fb_set_stream": ([_vp, _vp], None), "fb_synchronize": ([_vp], None), "fb_get_tables": ([_vp] * 6, None),
    "fb_malloc": ([_pvp, _sz], None), "fb_free": ([_vp], None),
    "fb_memcpy_h2d": ([_vp, _vp, _vp, _sz], None), "fb_memcpy_d2h": ([_vp, _vp, _vp, _sz], None), "fb_memset0": ([_vp, _vp, _sz], None),
    "fb_malloc_host": ([_vp, _sz], None), "fb_free_host": ([_vp], None),
    "fb_stream_create": ([_vp], None), "fb_stream_destroy": ([_vp], None), "fb_stream_synchronize": ([_vp], None),
    "fb_event_create": ([_vp], None), "fb_event_create_timing": ([_vp], None), "fb_event_destroy": ([_vp], None),
    "fb_event_record": ([_vp, _vp], None), "fb_stream_wait_event": ([_vp, _vp], None), "fb_event_synchronize": ([_vp], None),
    "fb_event_elapsed_ms": ([_vp, _vp, _vp], None),
    "fb_memcpy_d2h_async": ([_vp, _vp, _vp, _sz], None), "fb_memcpy_h2d_async": ([_vp, _vp, _vp, _sz], None),
    "fb_gradx": ([_vp] * 3, None), "fb_grady": ([_vp] * 3, None), "fb_laplacian": ([_vp] * 3, None),
    "fb_invert_laplacian": ([_vp] * 3, None), "fb_dealiase": ([_vp] * 3, None),
    "fb_r2c": ([_vp] * 3, None), "fb_c2r": ([_vp, _vp, _vp, _ip], None),
    "fb_backward_normalize": ([_vp, _vp], None), "fb_negate": ([_vp, _vp], None), "fb_jacobian": ([_vp] * 7, None),
    "fb_spec_axpy": ([_vp, _vp, _vp, _fl], None), "fb_spec_evolve": ([_vp, _vp, _vp, _fl, _vp], None),
    "fb_spec_rk4_combine": ([_vp] * 6 + [_fl, _vp], None),
    "fb_model_create": ([_pvp, _vp, _fl, _fl], None), "fb_model_use_graph": ([_vp, _ip], None),
    "fb_model_get_spectrum": ([_vp, _vp], None), "fb_model_set_spectrum": ([_vp, _vp], None),
    "fb_model_info": ([_vp, _psz, _psz], None), "fb_model_profile_steps": ([_vp, _ip, _pfl, _pip], None),
    "fb_spectra_shells": ([_ip, _ip, _fl, _fl, _pip], None), "fb_azimuthal_cols": ([_ip, _pip], None),
    "fb_slab_unique_id": ([_cp], None), "fb_slab_create": ([_pvp, _ip, _ip, _fl, _fl, _fl, _fl, _ip, _ip], None),
    "fb_slab_connect_rccl": ([_vp, _cp], None), "fb_local_hub_create": ([_pvp, _ip], None), "fb_local_hub_destroy": ([_vp], None),
    "fb_slab_connect_local": ([_vp, _vp], None), "fb_slab_connect_callback": ([_vp, ALLTOALL_FN, _vp], None),
    "fb_slab_synchronize": ([_vp], None), "fb_slab_record_event": ([_vp, _vp], None), "fb_slab_wait_event": ([_vp, _vp], None),
    "fb_slab_transport_selftest": ([_vp, _sz, _psz], None), "fb_slab_transport_info": ([_vp, _cp, _sz] + [_pip] * 4, None),
    "fb_slab_info": ([_vp] + [_pip] * 7, None), "fb_slab_geometry": ([_ip, _ip, _ip] + [_pip] * 3, None),
    "fb_slab_col_groups": ([_ip, _ip, _ip, _pip, _pip], None), "fb_slab_plan": ([_ip, _ip, _ip, _pip, _pip, _pip, _ip], None),
    "fb_create_slab": ([_pvp, _ip, _ip, _fl, _fl, _ip, _ip], None),
    "fb_write_field": ([_cp, _vp, _sz], None), "fb_read_field": ([_cp, _vp, _sz], None),
    "fb_make_field": ([_cp, _ip, _ip, _fl, _fl, _vp], None), "fb_make_source_kuo2004": ([_ip, _ip, _fl, _fl, _fl, _vp], None),
}
# fb_model_X and fb_slab_X (fb_slab_X_local where the slab's call works on this rank's rows) take the same parameters after the handle
_PAIRS = {
    "destroy": [], "step": [_ip], "time_steps": [_ip, _pfl],
    "set_vort_local": [_vp], "set_source_local": [_vp], "get_vort_local": [_vp], "get_diag_local": [_vp] * 3,
    "get_okubo_weiss_local": [_vp, _vp], "get_eddy_diffusivity": [_ip, _vp, _vp, _vp], "get_pressure_local": [_fl, _fl, _ip, _ip, _vp],
    "get_spectra": [_vp], "get_azimuthal": [_ip, _db, _db, _ip, _db, _ip, _vp, _vp],
    "set_tracer_local": [_vp, _fl], "get_tracer_local": [_vp], "get_tracer_eddy_diffusivity": [_ip, _vp, _vp, _vp],
    "set_particles": [_vp, _ip], "get_particles": [_vp], "particle_count": [_pip], "sample": [_vp, _vp, _ip, _vp],
    "set_tangent": [_vp], "get_tangent": [_vp], "tangent_norm": [_ip, _vp], "tangent_scale": [_fl],
    "set_tangents": [_vp, _ip], "get_tangents": [_vp], "tangent_count": [_pip], "tangent_gram": [_ip, _vp], "tangent_qr": [_ip, _vp],
    "adjoint_record": [_ip], "adjoint_recorded": [_pip], "set_adjoint": [_vp], "get_adjoint": [_vp], "adjoint_back": [_ip],
}
# the particle deformation's pairs, in a table of their own: _PAIRS is the set that the recorded refusal table
# (tests/golden/entry_refusals.json) covers name by name, and that recording predates these
_pdb = C.POINTER(_db)
_DEFORMATION_PAIRS = {
    "set_particle_deformation": [_ip], "get_particle_deformation": [_vp, _pdb], "particle_stretching": [_vp, _ip, _vp],
}
# the vortex census's pair, likewise
_CENSUS_PAIRS = {"census": [_vp, _vp, _ip, _fl, _ip, _ip, _vp, _vp, _vp]}
# the covariant Lyapunov vectors' pairs, likewise: the basis tape and the combination
_CLV_PAIRS = {"tangent_tape": [_ip], "tangent_tape_push": [], "tangent_tape_count": [_pip, _pip], "tangent_combine": [_ip, _vp]}
# the point observations' pairs, likewise: the scatter, the observation operator, the misfit and the adjoint's forcing
_OBS_PAIRS = {"scatter": [_vp, _vp, _ip, _vp], "observe": [_ip, _vp, _ip, _vp], "obs_misfit": [_vp, _vp, _vp, _ip, _vp, _vp],
              "adjoint_add_obs": [_ip, _vp, _vp, _ip]}
# the adjoint subspace's pairs, likewise: the set in and out and its count
_ADJOINTS_PAIRS = {"set_adjoints": [_vp, _ip], "get_adjoints": [_vp], "adjoint_count": [_pip]}
# adjoint checkpointing's pairs, likewise: the mode on and off, and what the window holds
_CHECKPOINT_PAIRS = {"adjoint_checkpoint": [_ip, _ip], "adjoint_checkpoint_info": [_pip, _pip, _pip, C.POINTER(C.c_longlong)]}
# the Lagrangian observations' pairs, likewise: the particle tape and the particle adjoint
_LAGRANGIAN_PAIRS = {"particle_tape": [_ip], "particle_tape_count": [_pip, _pip], "set_particle_adjoint": [_vp], "get_particle_adjoint": [_vp]}
# the tangent replay's pairs, likewise: the replay over the adjoint's tape, the rewind of a sweep and H applied to a perturbation
_REPLAY_PAIRS = {"tangent_replay": [_ip, _ip], "adjoint_rewind": [_ip], "observe_tangent": [_ip, _ip, _vp, _ip, _vp]}
# the split stage's pairs, likewise: ring forcing, drag and hyperviscosity on and off, the budget and the increment
_FORCING_PAIRS = {"set_forcing": [_db, _db, _db, _sz, _db, _db, _ip], "forcing_budget": [_pdb], "forcing_increment": [_sz, _vp]}
for _name, _args in (list(_PAIRS.items()) + list(_DEFORMATION_PAIRS.items()) + list(_CENSUS_PAIRS.items()) + list(_CLV_PAIRS.items())
                     + list(_OBS_PAIRS.items()) + list(_ADJOINTS_PAIRS.items()) + list(_CHECKPOINT_PAIRS.items())
                     + list(_LAGRANGIAN_PAIRS.items()) + list(_REPLAY_PAIRS.items()) + list(_FORCING_PAIRS.items())):
    SIGNATURES["fb_model_" + _name.replace("_local", "")] = SIGNATURES["fb_slab_" + _name] = ([_vp] + _args, None)
EXPORTS = list(SIGNATURES)


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
    # (an older build chosen through FFTBARO_LIB for an A/B run lacks the newer entry points: calling one there is an AttributeError)
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            if restype is not None:
                fn.restype = restype
    _lib = L
    return L


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


# the columns of the vortex census table (fb_model_census, include/fftbaro.h), one row per structure
CENSUS_COLUMNS = ("label", "n", "S_w", "S_wx", "S_wy", "S_wxx", "S_wyy", "S_wxy", "S_x", "S_y", "peak", "peak_index")
CENSUS_MAX = 65536
# what census_shapes derives from a row
CENSUS_SHAPE_COLUMNS = ("area", "circulation", "xc", "yc", "xg", "yg", "a", "b", "phi", "aspect")


def census_shapes(table, nx, ny, Lx, Ly):
    """The shapes of the structures of a census table (numpy float64 [rows, 12], columns CENSUS_COLUMNS): float64 [rows, 10] with the
    columns CENSUS_SHAPE_COLUMNS.  area = n dx dy [m^2]; circulation = S_w dx dy; (xc, yc) the weighted centroid, anchor + (S_wx,
    S_wy) / S_w folded into [0, Lx) x [0, Ly), NaN where S_w = 0; (xg, yg) the geometric centroid, anchor + (S_x, S_y) / n; a >= b
    the semi-axes 2 sqrt(lambda) of the central weighted second-moment matrix M (exact for a uniform elliptic patch; NaN where M is
    not positive semi-definite, as a weight of mixed sign can make it); phi = atan2(2 M_xy, M_xx - M_yy) / 2 in (-pi/2, pi/2], the
    angle of the major axis from the x axis (the first index); aspect = a / b.  A row with label -1 gives NaN.  dx, dy from the
    float32 lengths widened, as the engine takes them.  Meaningful for structures that span less than half the domain per axis.
    Host logic, no GPU."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, len(CENSUS_COLUMNS))
    lx, ly = float(np.float32(Lx)), float(np.float32(Ly))
    dx, dy = lx / nx, ly / ny
    out = np.full((t.shape[0], len(CENSUS_SHAPE_COLUMNS)), np.nan)
    ok = t[:, 0] >= 0
    label = np.where(ok, t[:, 0], 0.0).astype(np.int64)
    x0, y0 = (label // ny) * dx, (label % ny) * dy
    n, sw = t[:, 1], t[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        mx, my = t[:, 3] / sw, t[:, 4] / sw
        mxx, myy, mxy = t[:, 5] / sw - mx * mx, t[:, 6] / sw - my * my, t[:, 7] / sw - mx * my
        half, mean = np.hypot((mxx - myy) / 2, mxy), (mxx + myy) / 2
        a, b = 2 * np.sqrt(mean + half), 2 * np.sqrt(mean - half)
        phi = 0.5 * np.arctan2(2 * mxy, mxx - myy)
        phi = np.where(phi <= -np.pi / 2, np.pi / 2, phi)
        cols = (n * dx * dy, sw * dx * dy, np.mod(x0 + mx, lx), np.mod(y0 + my, ly), np.mod(x0 + t[:, 8] / n, lx), np.mod(y0 + t[:, 9] / n, ly),
                a, b, phi, a / b)
    for k, v in enumerate(cols):
        out[ok, k] = v[ok]
    for k, L in ((2, lx), (3, ly), (4, lx), (5, ly)):           # (a tiny negative offset folds to L itself in rounding)
        out[out[:, k] >= L, k] = 0.0
    return out


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise FftBaroError("no GPU visible: the engine has no CPU fallback")
    return torch


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _entry(prefix, name):
    """the C function prefix + name + "_local" where the library has it (a slab's calls on this rank's rows), else prefix + name"""
    fn = getattr(lib(), prefix + name + "_local", None)
    return fn if fn is not None else getattr(lib(), prefix + name)


PARTICLES_MAX = 1 << 24
# the columns of the stretching table (fb_model_particle_stretching, include/fftbaro.h), one row per particle (or matrix):
# F = Rot(theta_out) diag(sigma1, sign(det F) sigma2) Rot(theta_in)^T up to the overall sign, the angles in (-pi/2, pi/2]
PARTICLE_STRETCHING_COLUMNS = ("ln_sigma1", "ln_sigma2", "theta_in", "theta_out")
TANGENTS_MAX = 32
# orthonormalize_tangents: an update v -= r q rounds every element of v to float32, an error of up to eps32 / 2 of |v| + |r q|, about
# eps32 |v|; what is left of a v that lay in the span of the q is that noise.  8 eps32 of its length: below this nothing but it is left.
RANK_TOL = 8 * float(np.finfo(np.float32).eps)
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


def lyapunov_spectrum(model, steps, renorm_every, kind="enstrophy"):
    """The leading Lyapunov exponents from the tangent subspace of `model` (anything with step, orthonormalize_tangents and dt): one QR
    first (its R discarded: the set as given need not be orthonormal), then per interval of renorm_every steps the model is stepped,
    the perturbations are orthonormalised again and ln r_ii is accumulated.  Returns (exponents, float64 [M] in s^-1: the sums of
    ln r_ii / (steps dt), in the order of the perturbations; log_growth, float64 [intervals, M]: ln r_ii per interval).  The
    perturbations are left orthonormal: the backward Lyapunov vectors of the run so far."""
    if steps < 1 or renorm_every < 1:
        raise ValueError("lyapunov_spectrum: steps and renorm_every must be >= 1")
    model.orthonormalize_tangents(kind)
    rows, done = [], 0
    while done < steps:
        k = min(renorm_every, steps - done)
        model.step(k)
        done += k
        rows.append(np.log(np.diagonal(model.orthonormalize_tangents(kind))))
    log_growth = np.array(rows, dtype=np.float64)
    return log_growth.sum(axis=0) / (steps * model.dt), log_growth


def _solve_upper(r, b):
    """x with r x = b for an upper triangular r, by back substitution over all columns of b at once (no inverse is formed)"""
    m = r.shape[0]
    x = np.zeros_like(b)
    for i in range(m - 1, -1, -1):
        x[i] = (b[i] - r[i, i + 1:] @ x[i + 1:]) / r[i, i]
    return x


def clv_coefficients(R, C_end=None, seed=0):
    """The backward recursion of Ginelli's algorithm on the factors of N consecutive QR intervals.  R: float64 [N, M, M], R[n - 1] the
    upper triangular factor R_n of interval n, T Q_(n-1) = Q_n R_n with T the tangent step over the interval and Q_n the orthonormal
    bases after it.  C_end: the coefficients C_N after the last interval (default: a random upper triangular matrix from `seed`);
    its columns are scaled to unit length.  C_(n-1) = R_n^-1 C_n D_n by triangular solve, D_n diagonal so that every column of
    C_(n-1) has unit Euclidean length.  The columns of V_n = Q_n C_n are the covariant Lyapunov vectors at slot n, as far as the
    recursion has converged: T V_(n-1) = V_n D_n^-1 holds for ANY C_end.  Returns (C float64 [N + 1, M, M], log_growth float64 [N, M]):
    log_growth[n - 1, j] = -ln |R_n^-1 c_j| is ln of the factor by which covariant vector j grows over interval n.  Raises ValueError
    for a factor that is not finite, not upper triangular or has a diagonal element that is not positive.  Host logic, no GPU."""
    R = np.asarray(R, dtype=np.float64)
    if R.ndim != 3 or R.shape[1] != R.shape[2] or R.shape[1] < 1:
        raise ValueError("clv_coefficients: R must be [N, M, M]")
    N, M = R.shape[0], R.shape[1]
    for n in range(N):
        if not np.isfinite(R[n]).all():
            raise ValueError("clv_coefficients: factor %d is not finite" % n)
        if not np.array_equal(R[n], np.triu(R[n])):
            raise ValueError("clv_coefficients: factor %d is not upper triangular" % n)
        if not (np.diagonal(R[n]) > 0.0).all():
            raise ValueError("clv_coefficients: factor %d has a diagonal element that is not positive" % n)
    if C_end is None:
        C_end = np.triu(np.random.default_rng(seed).standard_normal((M, M)))
        C_end[np.diag_indices(M)] += np.sign(np.diagonal(C_end)) + (np.diagonal(C_end) == 0.0)   # (no column close to the span of the ones before)
    C_end = np.array(C_end, dtype=np.float64)
    if C_end.shape != (M, M) or not np.isfinite(C_end).all() or not np.array_equal(C_end, np.triu(C_end)) or (np.diagonal(C_end) == 0.0).any():
        raise ValueError("clv_coefficients: C_end must be a finite upper triangular [M, M] matrix with a non-zero diagonal")
    C = np.empty((N + 1, M, M))
    log_growth = np.empty((N, M))
    C[N] = C_end / np.sqrt((C_end * C_end).sum(axis=0))
    for n in range(N, 0, -1):
        x = _solve_upper(R[n - 1], C[n])
        length = np.sqrt((x * x).sum(axis=0))
        C[n - 1] = x / length
        log_growth[n - 1] = -np.log(length)
    return C, log_growth


ClvResult = collections.namedtuple("ClvResult", "C log_growth log_r cosines kind")
ClvResult.__doc__ = """What clv() returns.  With K window intervals, `settle` further ones and M perturbations: C float64 [K + 1, M, M], the
coefficients of the covariant Lyapunov vectors V_n = Q_n C_n in the bases of tape slot n; log_growth [K, M], ln of the growth of vector
j over window interval n; log_r [K + settle, M], ln r_ii of every QR (what lyapunov_spectrum accumulates); cosines [K + 1, M, M] =
C_n^T C_n, the cosines of the angles between the vectors of slot n in the inner product of `kind` (Q_n is orthonormal in it)."""


def clv(model, steps, renorm_every, settle, kind="enstrophy", seed=0, C_end=None):
    """Ginelli's algorithm on the tangent subspace of `model` (anything with step, orthonormalize_tangents, tangent_tape and
    push_tangents).  One QR (its R discarded) and the bases pushed as slot 0; then K = ceil(steps / renorm_every) window intervals of
    step, QR, push; then `settle` further intervals of step and QR whose R alone is kept (the recursion needs no fields there, only
    room to converge before it reaches the window); then clv_coefficients over all K + settle factors from C_end (default: random from
    `seed`).  Returns a ClvResult.  The model is left at the end of the run with the tape full: clv_vectors(result, n) puts the vectors
    of slot n into the live set."""
    if steps < 1 or renorm_every < 1 or settle < 0:
        raise ValueError("clv: steps and renorm_every must be >= 1, settle >= 0")
    K = -(-steps // renorm_every)
    model.orthonormalize_tangents(kind)
    model.tangent_tape(K + 1)
    model.push_tangents()
    factors, done = [], 0
    for n in range(K + settle):
        k = min(renorm_every, steps - done) if n < K else renorm_every
        model.step(k)
        done += k
        factors.append(model.orthonormalize_tangents(kind))
        if n < K:
            model.push_tangents()
    R = np.array(factors, dtype=np.float64)
    C, log_growth = clv_coefficients(R, C_end, seed)
    C = C[:K + 1]
    return ClvResult(C, log_growth[:K], np.log(np.diagonal(R, axis1=1, axis2=2)), np.einsum("nki,nkj->nij", C, C), kind)


def kaplan_yorke(exponents):
    """The Kaplan-Yorke (Lyapunov) dimension of a set of exponents, in any order: with them sorted downward and j the largest count
    whose partial sum is >= 0, j + (that sum) / |lambda_(j+1)|; 0.0 when the largest is negative, float(M) when the whole sum is >= 0
    (the M exponents do not reach the attractor's dimension).  Host logic, no GPU."""
    lam = np.sort(np.asarray(exponents, dtype=np.float64).ravel())[::-1]
    if lam.size == 0 or lam[0] < 0.0:
        return 0.0
    sums = np.cumsum(lam)
    j = int(np.nonzero(sums >= 0.0)[0].max()) + 1
    if j == lam.size:
        return float(j)
    return j + float(sums[j - 1]) / abs(float(lam[j]))


def checkpoint_every(steps):
    """The checkpoint spacing K >= 1 that minimises the half spectra a checkpointed window of `steps` steps holds, ceil(steps / K)
    checkpoints + 4 K of the tape segment (about sqrt(steps) / 2, for about 4 sqrt(steps)); of equal ones the smallest K."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("checkpoint_every: steps must be >= 1")
    best, k = (steps + 4, 1), 2
    while 4 * k < best[0]:                                      # beyond that the segment alone takes more
        best = min(best, (-(-steps // k) + 4 * k, k))
        k += 1
    return best[1]


_checkpoint_every = checkpoint_every                            # (the helpers below have a keyword of that name)


def _device(model):
    """where a helper keeps its tensors: the GPU, or what a stand-in for the engine (a float64 model on the CPU) names as .device"""
    return getattr(model, "device", "cuda")


def adjoint_window(model, every):
    """(on, off): how a helper keeps the adjoint's record on `model`.  on(steps) turns it on for a window of `steps` steps: every=None
    the full tape (record_adjoint(steps)); an int K >= 1 checkpointing with a checkpoint every K steps (checkpoint_adjoint(K, steps));
    "sqrt" that with K = checkpoint_every(steps).  off() turns off that mode (and with it whichever was on before)."""
    if every is None:
        return model.record_adjoint, lambda: model.record_adjoint(0)
    if isinstance(every, str) and every == "sqrt":
        return lambda steps: model.checkpoint_adjoint(_checkpoint_every(steps), steps), lambda: model.checkpoint_adjoint(0, 0)
    if isinstance(every, str) or int(every) != every or every < 1:
        raise ValueError("checkpoint_every: None, an int >= 1 or 'sqrt'")
    return lambda steps: model.checkpoint_adjoint(int(every), steps), lambda: model.checkpoint_adjoint(0, 0)


def singular_values(model, steps, iters, start, save=None, restore=None):
    """Power iteration on T^T T in the L2 (enstrophy) norm on `model` (anything with set_tangent, tangent, record_adjoint, step,
    set_adjoint, adjoint_back, adjoint; save / restore: how its state is kept and put back, by default spectrum / set_spectrum,
    which restores every bit), T the tangent of `steps` steps from the model's current state.  Each
    iteration restores that state, sets the tangent to the unit vector v (from `start`, an [nx, ny] field), steps with recording on,
    sets lam = T v, sweeps back and normalises v = T^T T v.  Returns (sigma = |T v| per iteration, the final v as a tensor); the model
    is left at its starting state with the tape freed, the tangent set to the last v and lam to T^T T of it.  It works through
    set_tangent, which replaces whatever set of perturbations was there (a tangent subspace too) by the one."""
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


ADJOINTS_MAX = 32
SV_SEED = 20240229          # singular_vectors(start=None): the seed of its start vectors


def fields_arg(a, shape, what, most):
    """Checks a set of M real fields, numpy or torch, [M, *shape] with 1 <= M <= most, float32 (numpy: float32 or float64, converted);
    raises ValueError, before anything is handed to the engine.  Returns M."""
    if isinstance(a, np.ndarray):
        ok_dtype = a.dtype in (np.float32, np.float64)
    else:
        ok_dtype = str(getattr(a, "dtype", None)) == "torch.float32"
    if not hasattr(a, "shape") or len(a.shape) != 1 + len(shape) or tuple(a.shape[1:]) != tuple(shape):
        raise ValueError("%s: [M, %s] fields" % (what, ", ".join(str(n) for n in shape)))
    if not ok_dtype:
        raise ValueError("%s: float32 fields (numpy: float32 or float64)" % what)
    if not 1 <= int(a.shape[0]) <= most:
        raise ValueError("%s: 1 to %d fields, not %d" % (what, most, int(a.shape[0])))
    return int(a.shape[0])


def _orthonormal_rows(t, w):
    """The rows of w, float64 [k, n] on any device, orthonormalised in their order: a QR by modified Gram-Schmidt, run twice (the
    second pass removes what the rounding of the first left), on the tensor where it lives."""
    q = w.clone()
    for _ in range(2):
        for j in range(q.shape[0]):
            for i in range(j):
                q[j] -= (q[i] @ q[j]) * q[i]
            q[j] /= q[j].norm()
    return q


def singular_vectors(model, steps, k, iters, start=None, save=None, restore=None, checkpoint_every=None, replay=False):
    """Orthogonal (block power) iteration on T^T T in the L2 norm on `model` (anything with set_tangents, tangents, record_adjoint,
    step, set_adjoints, adjoint_back, adjoints; save / restore as in singular_values), T the tangent of `steps` steps from the model's
    current state: the k leading singular values and right singular vectors from one tangent subspace and one adjoint set of k.  V,
    [k, nx, ny], starts as the orthonormalised `start` ([k, nx, ny], numpy or torch; None: normal deviates from a fixed seed, drawn on
    the GPU, so that two calls agree).  Per iteration: the state is restored bit for bit and set_tangents(V); `steps` steps with the
    tape on and U = tangents(); Rayleigh-Ritz on the k x k Gram matrix of U in float64 gives sigma_i, sorted descending, and the
    rotation E; set_adjoints(U), adjoint_back(steps), W = adjoints() rotated by E; W orthonormalised in float64 (a QR by Gram-Schmidt
    on the device tensors) is the next V.  No field crosses to the host: the Gram matrix alone is read, once per iteration.  Returns
    (sigma float64 [iters, k] numpy, the final V float32 [k, nx, ny] tensor, row i converging to the i-th right singular vector).
    The model is left as singular_values leaves it: at its starting state, the tape freed; the tangent set holds the last V it
    stepped and the adjoint set the last sweep.  Convergence of sigma_i goes like (sigma_(k+1) / sigma_i)^(2 iters).  checkpoint_every:
    None keeps the full tape of `steps` steps; an int K or "sqrt" keeps checkpoints instead (adjoint_window; checkpoint_adjoint on the
    model): the tangent subspace rides the forward run and not the steps a sweep takes again, and sigma and V are the same bits.
    replay=True (the full tape only): the forward run is made once, with the tape on and no tangent set, and each iteration is
    set_tangents(V), tangent_replay(0, steps), set_adjoints(U), adjoint_back(steps), adjoint_rewind(-1): no nonlinear step per
    iteration, and 4 + 5 k fields transformed per stage where the stepped subspace takes 10 k.  The replayed tangent is the live
    one's operator, not its bits: sigma and V agree with replay=False to float32 rounding.  A tangent set the user had is removed."""
    if steps < 1 or iters < 1:
        raise ValueError("singular_vectors: steps and iters must be >= 1")
    if replay and checkpoint_every is not None:
        raise ValueError("singular_vectors: replay needs the full tape (checkpoint_every=None)")
    if int(k) != k or not 1 <= k <= min(TANGENTS_MAX, ADJOINTS_MAX):
        raise ValueError("singular_vectors: k must be in [1, %d]" % min(TANGENTS_MAX, ADJOINTS_MAX))
    k = int(k)
    if start is not None:
        if not hasattr(start, "shape") or len(start.shape) != 3 or int(start.shape[0]) != k:
            raise ValueError("singular_vectors: start must be [k, nx, ny]")
    t, dev = model.torch, _device(model)
    save, restore = save or model.spectrum, restore or model.set_spectrum
    record_on, record_off = adjoint_window(model, checkpoint_every)
    if start is None:
        gen = t.Generator(device=dev)
        gen.manual_seed(SV_SEED)
        v = t.randn((k,) + tuple(model._shape), generator=gen, dtype=t.float64, device=dev)
    else:
        if isinstance(start, np.ndarray):
            start = t.from_numpy(np.ascontiguousarray(start, dtype=np.float64))
        v = start.to(dev).double()
    shape = tuple(v.shape)
    v = _orthonormal_rows(t, v.reshape(k, -1))
    z0 = save()
    sig = np.empty((iters, k))
    record_on(steps)
    try:
        if replay:                                              # the one forward run: the vorticity alone, its stage states onto the tape
            model.set_tangents(None)
            model.step(steps)
        for it in range(iters):
            if replay:
                if it:
                    model.adjoint_rewind(-1)
                model.set_tangents(v.float().reshape(shape).contiguous())
                model.tangent_replay(0, steps)
            else:
                restore(z0)
                model.set_tangents(v.float().reshape(shape).contiguous())
                model.step(steps)
            u32 = model.tangents()
            u = u32.double().reshape(k, -1)
            w, e = np.linalg.eigh((u @ u.T).cpu().numpy())
            order = np.argsort(w)[::-1]
            sig[it] = np.sqrt(np.maximum(w[order], 0.0))
            rot = t.from_numpy(np.ascontiguousarray(e[:, order].T)).to(dev)
            model.set_adjoints(u32)
            model.adjoint_back(steps)
            v = _orthonormal_rows(t, rot @ model.adjoints().double().reshape(k, -1))
        restore(z0)
    finally:
        record_off()
    return sig, v.float().reshape(shape)


OBS_KINDS = {"vort": 0, "u": 1, "v": 2, "psi": 3}
# a host address that is not NULL, for asking a slab of several ranks for its refusal: the engine refuses before it reads anything
_SOME = (C.c_double * 2)()


# the kind of an Observations set that holds drifter positions: no number of the C ABI, it never reaches observe or adjoint_add_obs
POSITION = "position"


def obs_kind(kind):
    """the C ABI's number of an observed quantity: "vort" | "u" | "v" | "psi" (an int is passed on for the engine to judge)"""
    if isinstance(kind, str):
        if kind not in OBS_KINDS:
            raise ValueError("kind: 'vort', 'u', 'v' or 'psi'")
        return OBS_KINDS[kind]
    return int(kind)


def values_dev(torch, a, n, what="values"):
    """n point values, numpy or torch, as a contiguous float64 [n] tensor on the GPU that has landed there"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if a.dtype != torch.float64 or a.dim() != 1 or a.shape[0] != n:
        raise ValueError("%s: float64 [%d]" % (what, n))
    a = a.cuda().contiguous()
    torch.cuda.current_stream().synchronize()                   # the engine reads them on ITS stream
    return a


def sigma_ok(sigma):
    """every sigma positive and finite (one read of a flag from the GPU): the engine itself does not look"""
    return bool(((sigma > 0) & sigma.isfinite()).all().item())


class Observations:
    """One set of point observations of one kind at one time: `step` (int >= 0, counted from the start of the window), `kind` ("vort",
    "u", "v" or "psi"), `xy` float64 [n, 2] positions [m] (unwrapped), `y` float64 [n] the observed values, `sigma` their standard
    errors (None: 1; a number; or float64 [n]), every one positive and finite.  Numpy or torch in; everything held is a tensor on the
    GPU after construction.
    kind "position" is Lagrangian data: `y` float64 [n, 2], the observed unwrapped positions of the n drifters that fourdvar is given as
    `particles`, in their order; `xy` must be None; `sigma` None, a number or float64 [n], one per drifter for both components.  Held as
    y flattened to [2 n] (x0, y0, x1, y1, ...) with sigma repeated per component: what obs_misfit takes."""

    def __init__(self, step, kind, xy, y, sigma=None):
        t = _torch()
        if int(step) != step or step < 0:
            raise ValueError("Observations: step must be an int >= 0")
        self.step, self.kind = int(step), kind
        if kind == POSITION:
            if xy is not None:
                raise ValueError("Observations: kind 'position' takes xy=None (the drifters are fourdvar's particles)")
            self.xy = None
            y = particles_dev(t, y)
            n = int(y.shape[0])
        else:
            obs_kind(kind)
            self.xy = particles_dev(t, xy)
            n = int(self.xy.shape[0])
        if n < 1 or n > PARTICLES_MAX:
            raise ValueError("Observations: 1 to 2^24 points")
        self.n = n
        self.y = y.reshape(-1) if kind == POSITION else values_dev(t, y, n, "y")
        if sigma is None or np.isscalar(sigma):
            self.sigma = t.full((n,), 1.0 if sigma is None else float(sigma), dtype=t.float64, device="cuda")
        else:
            self.sigma = values_dev(t, sigma, n, "sigma")
        if not sigma_ok(self.sigma):
            raise ValueError("Observations: every sigma must be positive and finite")
        if kind == POSITION:
            self.sigma = self.sigma.repeat_interleave(2).contiguous()

    def __len__(self):
        return self.n


def fourdvar(model, z0, obs, background=None, checkpoint_every=None, particles=None, keep_tape=False):
    """(J, grad) of the 4D-Var cost of the initial vorticity z0 (an [nx, ny] field, numpy or torch; it is set as float32) on `model`
    (anything with set_vort, record_adjoint, step, observe, obs_misfit, set_adjoint, adjoint_add_obs, adjoint_back, adjoint):
      J = 1/2 sum over the sets of obs and their points of (H zeta(step) - y)^2 / sigma^2   (+ 1/2 |z0 - zb|^2 / sigma_b^2),
    obs a sequence of Observations, background = (zb, sigma_b) with zb an [nx, ny] field and sigma_b a number.  The model is set to z0
    and stepped with the adjoint's tape on to the last observation step T, from one observation time to the next; at each, observe and
    obs_misfit keep h, the residuals r = (h - y) / sigma^2 and J on the GPU.  Then lam = 0 and the times are walked backward:
    adjoint_add_obs for every set of that time, adjoint_back to the time before, sets at step 0 included; grad is what is left in lam,
    float64 [nx, ny] on the GPU.  No field crosses to the host; J, a float, is read once at the end.  Tape memory: T x 4 half spectra
    (4 nx (ny/2 + 1) 8 bytes per step, 271 MB per step at 4096^2); where record_adjoint cannot allocate it, its FftBaroError is raised
    and nothing stays allocated.  A window that does not fit is what checkpoint_every is for: an int K keeps a checkpoint every K
    steps and a tape segment of K steps instead (checkpoint_adjoint(K, T): ceil(T / K) + 4 K + 1 half spectra), "sqrt" takes K =
    checkpoint_every(T), about 4 sqrt(T) half spectra; the piecewise sweeps between the observation times fill the segment again
    from the checkpoints, one more forward step per backward step, and J and grad are the same bits as with the full tape.  The record
    is freed at the end, whatever happens; one that was on before is gone.  The model is left at step T of the run from z0, with
    lam = grad's float32 form set.
    particles = xy0, float64 [n, 2]: the drifters' initial positions, set by set_particles after set_vort; sets of kind "position" then
    add 1/2 sum |X(step) - y|^2 / sigma^2 over the drifters to J (obs_misfit on the flattened positions).  With such a set the particle
    tape is on over the window (record_particles(T), 64 bytes per drifter and step, freed at the end with the field's), Xb starts at 0,
    gains r at every set's time (get, add, set on the GPU) and is swept back with lam by adjoint_back; what is left in
    model.particle_adjoint() is dJ/dX0, float64 [n, 2], as grad's float32 form is left in lam.  A "position" set without particles is a
    ValueError.  With particles=None and no such set nothing here differs from what it was.
    keep_tape=True: the tape is not freed at the end but rewound (adjoint_rewind(-1)), so the linearisation about z0 stays resident for
    gauss_newton_hvp; J and grad are the same bits.  An error frees it all the same.  Only with the full tape and without "position"
    sets (ValueError otherwise): checkpointed and Lagrangian Gauss-Newton are not there."""
    t, dev = model.torch, _device(model)
    obs = list(obs)
    if not obs:
        raise ValueError("fourdvar: no observations")
    drift = any(o.kind == POSITION for o in obs)
    if keep_tape and (checkpoint_every is not None or drift):
        raise ValueError("fourdvar: keep_tape needs the full tape (checkpoint_every=None) and no 'position' set")
    if drift and particles is None:
        raise ValueError("fourdvar: a 'position' set needs particles (the drifters' initial positions)")
    if particles is not None:
        particles = particles_dev(t, particles) if dev != "cpu" else particles
        for o in obs:
            if o.kind == POSITION and len(o) != int(particles.shape[0]):
                raise ValueError("fourdvar: a 'position' set of %d drifters, %d particles" % (len(o), int(particles.shape[0])))
    record_on, record_off = adjoint_window(model, checkpoint_every)
    if isinstance(z0, np.ndarray):
        z0 = t.from_numpy(np.ascontiguousarray(z0))
    z0 = z0.to(dev)
    times = sorted(set(o.step for o in obs))
    cost = t.zeros(1, dtype=t.float64, device=dev)
    res = {}
    kept = False                                                # keep_tape, once the sweep has gone through
    try:
        model.set_vort(z0.float().contiguous())
        if particles is not None:
            model.set_particles(particles)
        if times[-1]:
            record_on(times[-1])
            if drift:
                model.record_particles(times[-1])
        at = 0
        for when in times:
            model.step(when - at)
            at = when
            for k, o in enumerate(obs):
                if o.step == when:
                    h = model.particles().reshape(-1) if o.kind == POSITION else model.observe(o.kind, o.xy)
                    res[k] = model.obs_misfit(h, o.y, o.sigma, cost, check=False)
        model.set_adjoint(t.zeros(tuple(z0.shape), dtype=t.float32, device=dev))
        if drift:
            model.set_particle_adjoint(t.zeros(tuple(particles.shape), dtype=t.float64, device=dev))
        for when, before in zip(times[::-1], times[-2::-1] + [0]):
            for k, o in enumerate(obs):
                if o.step == when and o.kind == POSITION:
                    model.set_particle_adjoint(model.particle_adjoint() + res[k].reshape(-1, 2))
                elif o.step == when:
                    model.adjoint_add_obs(o.kind, o.xy, res[k])
            model.adjoint_back(when - before)
        grad = model.adjoint().double()
        kept = keep_tape
        if kept:
            model.adjoint_rewind(-1)
    finally:
        try:
            if not kept:
                record_off()
        finally:
            if drift:
                model.record_particles(0)
    if background is not None:
        zb, sb = background
        if isinstance(zb, np.ndarray):
            zb = t.from_numpy(np.ascontiguousarray(zb))
        d = z0.double() - zb.to(dev).double()
        cost += 0.5 * (d * d).sum() / float(sb) ** 2
        grad = grad + d / float(sb) ** 2
    return float(cost.item()), grad


def fit_initial(model, z0, obs, iters, background=None, history=8, armijo=1e-4, shrink=0.5, max_backtracks=25, checkpoint_every=None,
                particles=None):
    """Minimises model.fourdvar(z, obs, background) -> (J, grad) over the initial field z from z0 by L-BFGS (the two-loop recursion over
    the last `history` pairs) with a backtracking Armijo line search: a step t d is accepted when J(z + t d) <= J(z) + armijo t <grad, d>,
    t from 1 (the first iteration: from the step 2 J / |grad|^2 along -grad, the exact minimiser of a one-dimensional quadratic
    that touches zero), times `shrink` per rejection, at most max_backtracks times.  Host logic on float64 tensors wherever z0 lives
    (the GPU for the engine; anything with a fourdvar will do).  It stops after `iters` accepted iterations, or at the first whose
    line search finds no acceptable step, or when the gradient is zero.  Returns (z, J_history, evaluations): the final field, float64;
    J at the start and after every accepted iteration (it falls at every one); the number of fourdvar calls.  checkpoint_every, where
    it is not None, is handed to every model.fourdvar call (fourdvar(): windows whose full tape does not fit), and so is particles
    (the drifters' initial positions, for sets of kind "position")."""
    t = model.torch
    if iters < 0 or history < 1:
        raise ValueError("fit_initial: iters must be >= 0, history >= 1")
    if isinstance(z0, np.ndarray):
        z0 = t.from_numpy(np.ascontiguousarray(z0))
    x = z0.double().clone()
    how = {} if checkpoint_every is None else {"checkpoint_every": checkpoint_every}
    if particles is not None:
        how["particles"] = particles

    def evaluate(z):
        J, g = model.fourdvar(z, obs, background, **how)
        return float(J), g.double().to(x.device)

    def dot(a, b):
        return float((a * b).sum())
    J, g = evaluate(x)
    hist, evals, pairs = [J], 1, []                             # pairs: (s, y, 1 / <s, y>), oldest first
    for _ in range(iters):
        gg = dot(g, g)
        if not gg > 0.0:
            break
        q, alphas = g.clone(), []
        for s, y, rho in reversed(pairs):
            a = rho * dot(s, q)
            alphas.append(a)
            q -= a * y
        if pairs:
            s, y, _ = pairs[-1]
            q *= dot(s, y) / dot(y, y)
        else:
            q *= 2.0 * J / gg
        for (s, y, rho), a in zip(pairs, reversed(alphas)):
            q += (a - rho * dot(y, q)) * s
        d = -q
        slope = dot(g, d)
        if not slope < 0.0:                                     # not a descent direction: steepest descent, the memory dropped
            pairs, d, slope = [], -g * (2.0 * J / gg), -2.0 * J
        step, found = 1.0, None
        for _ in range(max_backtracks):
            xn = x + step * d
            Jn, gn = evaluate(xn)
            evals += 1
            if np.isfinite(Jn) and Jn <= J + armijo * step * slope:
                found = (xn, Jn, gn)
                break
            step *= shrink
        if found is None:
            break
        xn, Jn, gn = found
        s, y = xn - x, gn - g
        sy = dot(s, y)
        if sy > 1e-12 * np.sqrt(dot(s, s) * dot(y, y)):         # curvature condition: keep the memory positive definite
            pairs = (pairs + [(s, y, 1.0 / sy)])[-history:]
        x, J, g = xn, Jn, gn
        hist.append(J)
    return x, hist, evals


def gauss_newton_hvp(model, v, obs, background=None):
    """The Gauss-Newton Hessian-vector product of the 4D-Var cost about the trajectory that model.fourdvar(z0, obs, ..., keep_tape=True)
    has left on the tape,
      H_GN v = v / sigma_b^2 + sum over the sets k of T_k^T H_k^T R_k^-1 H_k T_k v,
    T_k the tangent from step 0 to the set's step, on `model` (anything with set_tangent, tangent_replay, observe_tangent, set_adjoint,
    adjoint_add_obs, adjoint_back, adjoint, adjoint_rewind, adjoint_recorded).  v, an [nx, ny] field (numpy or torch), is set as the
    tangent (float32) and replayed over the tape from observation time to observation time by absolute step index; at each,
    observe_tangent gives w = h / sigma^2 on the GPU (sets at step 0 see v itself).  Then lam = 0 and the times are walked backward as
    fourdvar walks them, adjoint_add_obs with w and adjoint_back; the tape is rewound (adjoint_rewind(-1)), so the next product finds
    it whole.  Returns float64 [nx, ny] on the GPU.  No field crosses to the host and nothing nonlinear is stepped: one product costs a
    replay and a sweep of the window.  It works through set_tangent and set_adjoint: a tangent set or an adjoint set that the user
    had is REPLACED, and the tangent set is removed at the end; lam is left at the product's float32 form without the background
    term.  'position' sets are a ValueError, and so is a tape that does not hold the window."""
    t, dev = model.torch, _device(model)
    obs = list(obs)
    if not obs:
        raise ValueError("gauss_newton_hvp: no observations")
    if any(o.kind == POSITION for o in obs):
        raise ValueError("gauss_newton_hvp: 'position' sets are not supported")
    times = sorted(set(o.step for o in obs))
    if model.adjoint_recorded() < times[-1]:
        raise ValueError("gauss_newton_hvp: the tape holds %d steps, the window %d: call fourdvar(..., keep_tape=True) first"
                         % (model.adjoint_recorded(), times[-1]))
    if isinstance(v, np.ndarray):
        v = t.from_numpy(np.ascontiguousarray(v))
    v = v.to(dev)
    w = {}
    try:
        model.set_tangent(v.float().contiguous())
        at = 0
        for when in times:
            if when > at:
                model.tangent_replay(at, when - at)
            at = when
            for k, o in enumerate(obs):
                if o.step == when:
                    w[k] = model.observe_tangent(o.kind, o.xy) / o.sigma ** 2
        model.set_adjoint(t.zeros(tuple(v.shape), dtype=t.float32, device=dev))
        for when, before in zip(times[::-1], times[-2::-1] + [0]):
            for k, o in enumerate(obs):
                if o.step == when:
                    model.adjoint_add_obs(o.kind, o.xy, w[k])
            model.adjoint_back(when - before)
        hv = model.adjoint().double()
    finally:
        model.adjoint_rewind(-1)
        model.set_tangent(None)
    if background is not None:
        hv = hv + v.double() / float(background[1]) ** 2
    return hv


def fit_incremental(model, z0, obs, outer, inner, background=None, cg_tol=1e-2, armijo=1e-4, shrink=0.5, max_backtracks=25):
    """Incremental (Gauss-Newton) 4D-Var on `model` (anything with fourdvar(z, obs, background, keep_tape=True) -> (J, grad),
    gauss_newton_hvp(v, obs, background) and record_adjoint): per outer iteration one nonlinear run gives J, g and leaves the
    linearisation on the tape; conjugate gradients from 0 on H_GN delta = -g, stopped after `inner` products, or when
    |r| <= cg_tol |g|, or at a direction of non-positive curvature (the first one: steepest descent); then a backtracking Armijo search
    on the nonlinear J along delta, t from 1, times `shrink` per rejection, at most max_backtracks times, whose accepted evaluation is
    the next outer iteration's J, g and tape.  Host logic on float64 tensors wherever z0 lives.  It stops after `outer` accepted
    iterations, or at the first whose search finds no acceptable step, or when the gradient is zero.  Returns (z, J_history,
    evaluations, hvps): the final field, float64; J at the start and after every accepted iteration; the numbers of fourdvar calls and
    of Hessian-vector products.  The tape is freed at the end, whatever happens; the tangent set and the adjoint variable are
    gauss_newton_hvp's."""
    t = model.torch
    if outer < 0 or inner < 1:
        raise ValueError("fit_incremental: outer must be >= 0, inner >= 1")
    if isinstance(z0, np.ndarray):
        z0 = t.from_numpy(np.ascontiguousarray(z0))
    x = z0.double().clone()

    def evaluate(z):
        J, g = model.fourdvar(z, obs, background, keep_tape=True)
        return float(J), g.double().to(x.device)

    def dot(a, b):
        return float((a * b).sum())
    evals = hvps = 0
    hist = []
    try:
        J, g = evaluate(x)
        evals, hist = 1, [J]
        for _ in range(outer):
            gg = dot(g, g)
            if not gg > 0.0:
                break
            d, r = t.zeros_like(g), -g
            p, rr = r.clone(), gg
            for it in range(inner):
                hp = model.gauss_newton_hvp(p, obs, background).double().to(x.device)
                hvps += 1
                php = dot(p, hp)
                if not php > 0.0:
                    if it == 0:
                        d = r.clone()
                    break
                a = rr / php
                d = d + a * p
                r = r - a * hp
                rn = dot(r, r)
                if np.sqrt(rn) <= cg_tol * np.sqrt(gg):
                    break
                p = r + (rn / rr) * p
                rr = rn
            slope = dot(g, d)
            if not slope < 0.0:
                break
            step, found = 1.0, None
            for _ in range(max_backtracks):
                xn = x + step * d
                Jn, gn = evaluate(xn)
                evals += 1
                if np.isfinite(Jn) and Jn <= J + armijo * step * slope:
                    found = (xn, Jn, gn)
                    break
                step *= shrink
            if found is None:
                break
            x, J, g = found
            hist.append(J)
    finally:
        model.record_adjoint(0)
    return x, hist, evals, hvps


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


class ModelSurface:
    """What Model (fb_model_*, the whole [nx, ny] grid) and slab.EngineSlab (fb_slab_*, this rank's [XL, ny] rows; its calls are
    collective) share: every call of the C ABI that both have, written once.  A subclass supplies _PREFIX, the handle _h, _shape
    (of a real field), _wait() (until the engine has finished what it was handed) and, where it can have several ranks, _one_rank().
    The engine works on ITS streams: torch's current stream is waited for before any call that is handed a tensor."""

    _PREFIX = None
    _STATE = None           # (getter, setter) of the state that singular_values keeps and puts back

    def _call(self, name, *args):
        """check(fb_<PREFIX>_<name>_local(handle, *args)), or fb_<PREFIX>_<name> where the library has no _local form"""
        check(_entry(self._PREFIX, name)(self._h, *args))

    def _hand(self, name, *args):
        """_call with tensors among the arguments, handed over as they are so that they live until the engine is done with them: what
        torch has queued for them lands first, and the engine is waited for after"""
        self.torch.cuda.current_stream().synchronize()
        self._call(name, *[_ptr(a) if isinstance(a, self.torch.Tensor) else a for a in args])
        self._wait()

    def _one_rank(self, name, *nulls):
        """for a call that only one rank supports, before any buffer is shaped: nothing to refuse here"""

    def _dev(self, a):
        """a real field (numpy or torch; None passes through) as a contiguous float32 tensor of _shape on the GPU"""
        t = self.torch
        if isinstance(a, np.ndarray):
            a = t.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
        assert a is None or (a.is_cuda and a.dtype == t.float32 and a.is_contiguous() and tuple(a.shape) == self._shape)
        return a

    def _get(self, name, k, *args):
        """k fresh real fields filled by fb_*_get_<name>(handle, *args, fields ...)"""
        out = tuple(self.torch.empty(self._shape, dtype=self.torch.float32, device="cuda") for _ in range(k))
        self._hand("get_" + name, *args, *out)
        return out

    def _count(self, name):
        n = C.c_int()
        self._call(name, C.byref(n))
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._PREFIX + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_vort(self, vort): self._hand("set_vort", self._dev(vort))

    def set_source(self, src):
        if src is None:
            self._call("set_source", None)
        else:
            self._hand("set_source", self._dev(src))

    def step(self, n=1): self._call("step", n)

    def time_steps(self, n):
        ms = C.c_float()
        self._call("time_steps", n, C.byref(ms))
        return ms.value

    def vort(self): return self._get("vort", 1)[0]

    def diag(self):
        """psi, u, v (the stage-0 record dumps, main.cpp:181-222)"""
        return self._get("diag", 3)

    def okubo_weiss(self):
        """(W, tau_fil): the Okubo-Weiss parameter [s^-2] and the filamentation time [s] (+inf where W <= 0)."""
        return self._get("okubo_weiss", 2)

    def _eddy(self, name, nbins, fields):
        t = self.torch
        table = t.empty((nbins, 9), dtype=t.float64, device="cuda")
        a, g = (t.empty(self._shape, dtype=t.float32, device="cuda") for _ in range(2)) if fields else (None, None)
        self._hand(name, nbins, table, a, g)
        return (table, a, g) if fields else table

    def eddy_diffusivity(self, nbins=256, fields=False):
        """The effective eddy diffusivity table of the whole domain, float64 [nbins, 9] (columns EDDY_DIFFUSIVITY_COLUMNS), of the
        vorticity binned in nbins contour intervals; with fields=True also (zeta, grad2): the vorticity and |grad zeta|^2."""
        return self._eddy("get_eddy_diffusivity", nbins, fields)

    def pressure(self, rho=1.0, f=1e-5, ref=(0, 0)):
        """The nonlinear-balance pressure of the current state (invert_pres.cpp:135-185) minus its value at the reference point
        ref = (ref_x, ref_y): the element ref_x + nx * ref_y of the flattened [nx, ny] field, as the reference indexes it."""
        return self._get("pressure", 1, rho, f, int(ref[0]), int(ref[1]))[0]

    def spectra(self):
        """The shell spectra and cascade fluxes of the current state, float64 [nshells, 10] (columns SPECTRA_COLUMNS): energy and
        enstrophy spectra, advective transfers and fluxes, enstrophy dissipation per wavenumber shell of the whole domain."""
        t = self.torch
        table = t.empty((spectra_shells(self.nx, self.ny, self.Lx, self.Ly), 10), dtype=t.float64, device="cuda")
        self._hand("get_spectra", table)
        return table

    def azimuthal(self, center="psi-min", nbins=None, dr=None, nmodes=4):
        """(table, center): the azimuthal means about a vortex centre (fb_model_get_azimuthal).  center: "psi-min" (grid point of the
        smallest psi), "vort-max" (of the largest zeta) or a fixed (xc, yc) [m]; nbins radial bins of the width dr [m] (defaults:
        dr = max(dx, dy), nbins = floor(min(Lx, Ly) / 2 / dr), at most 4096); table float64 [nbins, 12 + 2 nmodes] (columns
        AZIMUTHAL_COLUMNS, then Re, Im of the azimuthal wavenumbers 1 .. nmodes of zeta), center float64 [4] = xc, yc, flat index,
        value; both on the GPU, of the whole domain."""
        t = self.torch
        mode, xc, yc, nbins, dr = azimuthal_args(self.nx, self.ny, self.Lx, self.Ly, center, nbins, dr)
        table = t.empty((max(nbins, 0), 12 + 2 * max(int(nmodes), 0)), dtype=t.float64, device="cuda")
        cen = t.empty(4, dtype=t.float64, device="cuda")
        self._hand("get_azimuthal", mode, xc, yc, nbins, dr, int(nmodes), table, cen)
        return table, cen

    def census(self, field=None, threshold=0.0, below=False, weight=None, min_cells=1, max_structures=1024, labels=False):
        """(table, found): the vortex census (fb_model_census) of `field`, an [nx, ny] float32 field (numpy or torch; None: the model's
        vorticity): the 4-connected structures of field > threshold (below=True: < threshold) on the doubly periodic grid with at
        least min_cells cells, in the order of their smallest flat index.  table: float64 [min(found, max_structures), 12] on the GPU
        (columns CENSUS_COLUMNS: label, cells, the raw moments of `weight` (None: the field itself) about the anchor cell, the peak);
        found: the number of structures kept, which may exceed max_structures.  labels=True adds the int32 [nx, ny] map of dense
        ids (-1 off the structures).  census_shapes turns the table into areas, circulations, centroids and axes.  One rank only."""
        t = self.torch
        self._one_rank("census", None, None, 0, 0.0, 1, 1, None, None, None)
        f = self.vort() if field is None else self._dev(field)
        w = self._dev(weight)
        m = int(max_structures)
        table = t.empty((min(max(m, 1), CENSUS_MAX), len(CENSUS_COLUMNS)), dtype=t.float64, device="cuda")
        count = t.empty(2, dtype=t.int32, device="cuda")
        ids = t.empty(self._shape, dtype=t.int32, device="cuda") if labels else None
        self._hand("census", f, w, 1 if below else 0, float(threshold), int(min_cells), m, table, count, ids)
        found = int(count[0].item())
        table = table[:min(found, m)]
        return (table, found, ids) if labels else (table, found)

    def set_tracer(self, c, kappa=0.0):
        """Sets the passive tracer, a field advected by the model's flow with the diffusivity kappa [m^2 s^-1] (it is stepped beside
        the vorticity from now on); c=None removes it."""
        self._hand("set_tracer", self._dev(c), 0.0 if c is None else float(kappa))

    def tracer(self): return self._get("tracer", 1)[0]

    def tracer_eddy_diffusivity(self, nbins=256, fields=False):
        """eddy_diffusivity() of the passive tracer, with its kappa in the place of nu; with fields=True also (c, |grad c|^2)."""
        return self._eddy("get_tracer_eddy_diffusivity", nbins, fields)

    def set_particles(self, xy):
        """Sets the Lagrangian particles, float64 [n, 2] positions (x, y) [m] (numpy or torch), advected by the model's flow from now
        on with the RK4 scheme of the step itself; xy=None removes them.  One rank only: on several ranks this and the three methods
        below raise FftBaroError with the engine's message."""
        a = None if xy is None else particles_dev(self.torch, xy)
        self._hand("set_particles", a, 0 if a is None else int(a.shape[0]))

    def particle_count(self): return self._count("particle_count")

    def particles(self, wrap=False):
        """The particles' positions, a float64 [n, 2] tensor: unwrapped (a particle that left through one side keeps counting), or with
        wrap=True folded into [0, Lx) x [0, Ly)."""
        t = self.torch
        out = t.empty((max(self.particle_count(), 1), 2), dtype=t.float64, device="cuda")
        self._hand("get_particles", out)
        return wrap_positions(t, out, self.Lx, self.Ly) if wrap else out

    def sample(self, field, xy=None):
        """An [nx, ny] float32 field (numpy or torch: the vorticity, the tracer, W, the pressure ...) interpolated to the positions
        xy, float64 [n, 2], or to the particles (xy=None), by the particles' cubic Lagrange scheme: a float64 [n] tensor."""
        t = self.torch
        self._one_rank("sample", None, None, 0, None)
        f = self._dev(field)
        a = self.particles() if xy is None else particles_dev(t, xy)
        out = t.empty(a.shape[0], dtype=t.float64, device="cuda")
        self._hand("sample", f, a, int(a.shape[0]), out)
        return out

    def set_particle_deformation(self, on=True):
        """Switches the particles' deformation gradient on: every particle carries F = dX(t) / dX(t0), float64 2 x 2, advanced by the
        exact linearisation of the particles' own RK4 step (the Jacobian of the discrete map, with the gradient of the cubic Lagrange
        interpolant itself).  on=True sets F = I and the elapsed time to 0, so it is the reset too (F grows like exp(lambda t));
        on=False frees it.  set_particles switches it off.  det F is close to 1, not equal: the interpolated velocity is not exactly
        non-divergent.  One rank only, as the particles."""
        self._call("set_particle_deformation", int(on))

    def _deformation(self):
        """(F as float64 [n, 4] on the GPU, the elapsed time in seconds)"""
        t = self.torch
        out = t.empty((max(self.particle_count(), 1), 4), dtype=t.float64, device="cuda")
        el = C.c_double()
        self._hand("get_particle_deformation", out, C.byref(el))
        return out, el.value

    def particle_deformation(self):
        """The particles' deformation gradient, a float64 [n, 2, 2] tensor: F[p] = [[F11, F12], [F21, F22]]."""
        return self._deformation()[0].view(-1, 2, 2)

    def particle_deformation_time(self):
        """The time F has been carried for [s]: (steps since set_particle_deformation) x dt."""
        return self._deformation()[1]

    def particle_stretching(self, F=None):
        """The closed-form 2 x 2 singular value decomposition, on the GPU, of the particles' F (F=None) or of ANY matrices F, float64
        [n, 2, 2] or [n, 4] (numpy or torch): a float64 [n, 4] tensor with the columns PARTICLE_STRETCHING_COLUMNS, ln sigma1,
        ln sigma2, theta_in (the direction of strongest stretching at the initial time) and theta_out (its image), the angles folded
        into (-pi/2, pi/2].  The zero matrix gives -inf, -inf, 0, 0; a singular one ln sigma2 = -inf; an entry that is not finite NaN."""
        t = self.torch
        self._one_rank("particle_stretching", None, 1, None)
        if F is None:
            out = t.empty((max(self.particle_count(), 1), 4), dtype=t.float64, device="cuda")
            self._hand("particle_stretching", None, 0, out)
            return out
        if isinstance(F, np.ndarray):
            F = t.from_numpy(np.ascontiguousarray(F, dtype=np.float64))
        if F.dtype != t.float64 or F.dim() not in (2, 3) or F.shape[0] == 0 or F.shape[1:].numel() != 4:
            raise ValueError("particle_stretching: float64 [n, 2, 2] or [n, 4], n >= 1")
        F = F.cuda().contiguous().view(-1, 4)
        out = t.empty((F.shape[0], 4), dtype=t.float64, device="cuda")
        self._hand("particle_stretching", F, int(F.shape[0]), out)
        return out

    def ftle(self):
        """The forward finite-time Lyapunov exponent of every particle [s^-1], float64 [n]: ln sigma1 / T, T the time since
        set_particle_deformation.  Raises while T = 0."""
        T = self.particle_deformation_time()
        if not T > 0.0:
            raise FftBaroError("ftle: no step since set_particle_deformation (T = 0)")
        ln1 = self.particle_stretching()[:, 0]
        return ln1 / self.torch.full_like(ln1, T)               # (a tensor divisor: torch multiplies by the reciprocal of a scalar one)

    def set_tangent(self, dz):
        """Sets the perturbation of the tangent-linear model, a field carried along the evolving vorticity by the linearisation of the
        step itself (it is stepped beside the vorticity from now on); dz=None removes it.  One rank only: on several ranks this and the
        four methods below raise FftBaroError with the engine's message."""
        self._one_rank("set_tangent", None)
        self._hand("set_tangent", self._dev(dz))

    def tangent(self): return self._get("tangent", 1)[0]

    def tangent_norm(self, kind="enstrophy"):
        """The perturbation's norm, a float: "enstrophy" <dz^2> / 2 or "energy" <|grad dpsi|^2> / 2, summed in float64 on the GPU."""
        return float(self._tangent_pairs("tangent_norm", kind, 1).item())

    def rescale_tangent(self, a):
        """dz *= a (a finite and not zero)"""
        self._call("tangent_scale", float(a))

    def lyapunov(self, steps, renorm_every, kind="enstrophy"):
        """(exponent [s^-1], growth factors): steps the model, renormalising the perturbation every renorm_every steps (lyapunov())."""
        return lyapunov(self, steps, renorm_every, kind)

    def set_tangents(self, dz):
        """Sets a tangent subspace: M perturbations, [M, nx, ny] (numpy or torch, 1 <= M <= TANGENTS_MAX), carried along the ONE
        trajectory, each as set_tangent carries its one (perturbation k is bit for bit what set_tangent of dz[k] gives); whatever set
        was there is replaced; dz=None removes all.  tangent(), tangent_norm() and rescale_tangent() act on perturbation 0.  Modes
        outside the dealiasing circle never evolve but count in every inner product: dealiase a set that is meant for exponents.  One
        rank only, as set_tangent."""
        t = self.torch
        self._one_rank("set_tangents", None, 1)
        if dz is None:
            return self._hand("set_tangents", None, 0)
        if isinstance(dz, np.ndarray):
            dz = t.from_numpy(np.ascontiguousarray(dz, dtype=np.float32)).cuda()
        assert dz.is_cuda and dz.dtype == t.float32 and dz.is_contiguous() and dz.dim() == 3 and tuple(dz.shape[1:]) == self._shape
        self._hand("set_tangents", dz, int(dz.shape[0]))

    def tangent_count(self): return self._count("tangent_count")

    def _tangent_rows(self):
        """the number of perturbations for an output's shape; with none set 1, so that the engine's own refusal is what is raised"""
        return max(self.tangent_count(), 1)

    def tangents(self):
        """every perturbation, float32 [M, nx, ny]"""
        out = self.torch.empty((self._tangent_rows(),) + self._shape, dtype=self.torch.float32, device="cuda")
        self._hand("get_tangents", out)
        return out

    def _tangent_pairs(self, name, kind, m=None):
        """the float64 [m, m] output of fb_*_<name>(kind, out), m the number of perturbations unless given"""
        m = m or self._tangent_rows()
        out = self.torch.empty((m, m), dtype=self.torch.float64, device="cuda")
        self._hand(name, tangent_kind(kind), out)
        return out

    def tangent_gram(self, kind="enstrophy"):
        """The Gram matrix of the perturbations, a float64 [M, M] tensor on the GPU: <v_i, v_j> in the inner product whose <v, v> is
        tangent_norm(kind), summed in float64 on the GPU; symmetric bit for bit."""
        return self._tangent_pairs("tangent_gram", kind)

    def orthonormalize_tangents(self, kind="enstrophy"):
        """Orthonormalises the perturbations in place in that inner product (modified Gram-Schmidt on the GPU, in their order) and
        returns R, float64 [M, M] numpy, upper triangular, with v_j (before) = sum over i <= j of R[i, j] q_i.  Raises FftBaroError
        for a rank-deficient set: R's diagonal is not finite and positive, or r_jj <= RANK_TOL |v_j (before)|, which in float32 storage
        is what an exactly dependent v_j leaves (the rounding of its updates, not zero).  The perturbations are then not finite, or
        noise: set them again."""
        r = self._tangent_pairs("tangent_qr", kind).cpu().numpy()
        d = np.diagonal(r)
        if not (np.isfinite(r).all() and (d > RANK_TOL * np.sqrt((r * r).sum(axis=0))).all()):
            raise FftBaroError("orthonormalize_tangents: the perturbations are not linearly independent in the %s inner product (diagonal of R: %s)" % (kind, d))
        return r

    def lyapunov_spectrum(self, steps, renorm_every, kind="enstrophy"):
        """(exponents [M] in s^-1, log_growth [intervals, M]): steps the model, orthonormalising the perturbations every renorm_every
        steps (lyapunov_spectrum())."""
        return lyapunov_spectrum(self, steps, renorm_every, kind)

    def tangent_tape(self, depth):
        """Allocates the basis tape: depth >= 1 slots, each the bases of every perturbation of the current set (M half spectra; info()
        counts them), and leaves it empty; depth = 0 frees it.  set_tangents with another count, or with None, frees it too; set_vort
        and set_spectrum leave it alone.  One rank only, as set_tangent."""
        self._call("tangent_tape", int(depth))

    def push_tangents(self):
        """Copies the perturbations' bases into the next slot of the tape, on the GPU; a full tape raises.  Nothing is allocated, and
        the captured step (use_graph) stays."""
        self._call("tangent_tape_push")

    def tangent_tape_count(self):
        """(slots pushed, slots allocated); (0, 0) while there is no tape"""
        n, d = C.c_int(), C.c_int()
        self._call("tangent_tape_count", C.byref(n), C.byref(d))
        return n.value, d.value

    _COMBINE_KEEP = 64

    def combine_tangents(self, Cm, slot=None):
        """The perturbations become V = Q C on the GPU: v_j = sum over i of C[i, j] q_i for all j in one pass, with Q the bases of
        tape slot `slot`, or the live set itself (slot=None, in place).  Cm: float64 [M, M], numpy or torch; it is uploaded to the GPU,
        and nothing is waited for beyond that upload (the engine works on its stream; the uploaded coefficients are kept until it has
        read them).  Every element is summed in float64 in the order of i and rounded once to float32."""
        t = self.torch
        m = self._tangent_rows()
        if isinstance(Cm, np.ndarray):
            Cm = t.from_numpy(np.ascontiguousarray(Cm, dtype=np.float64))
        if Cm.dtype != t.float64 or tuple(Cm.shape) != (m, m):
            raise ValueError("combine_tangents: float64 [%d, %d]" % (m, m))
        Cm = Cm.cuda().contiguous()
        t.cuda.current_stream().synchronize()                   # the engine reads them on ITS stream
        keep = self.__dict__.setdefault("_combine_kept", [])
        if len(keep) >= self._COMBINE_KEEP:                     # (a wait once in _COMBINE_KEEP calls: what is dropped here has been read)
            self._wait()
            del keep[:]
        keep.append(Cm)
        self._call("tangent_combine", -1 if slot is None else int(slot), _ptr(Cm))

    def clv(self, steps, renorm_every, settle, kind="enstrophy", seed=0, C_end=None):
        """The covariant Lyapunov vectors over the next `steps` steps by Ginelli's algorithm (clv()): a ClvResult with the coefficients
        C [K + 1, M, M], log_growth [K, M], log_r [K + settle, M] and cosines [K + 1, M, M], K = ceil(steps / renorm_every).  Needs a
        set of at most TANGENTS_MAX perturbations and room for a tape of K + 1 slots (it allocates the tape and raises FftBaroError
        where that fails).  The model is left at the end of the run, steps + settle * renorm_every steps on, with the tape full."""
        return clv(self, steps, renorm_every, settle, kind, seed, C_end)

    def clv_vectors(self, result, n):
        """The covariant Lyapunov vectors at slot n of a clv() result, float32 [M, nx, ny]: combine_tangents(result.C[n], slot=n), then
        tangents().  It REPLACES the live set of perturbations by these vectors (the tape keeps the bases)."""
        self.combine_tangents(result.C[n], slot=n)
        return self.tangents()

    def record_adjoint(self, depth):
        """Turns the adjoint's tape on (depth >= 1: room for depth steps; every step from now on records its four stage states, and a
        step call beyond depth is refused) or off (depth = 0, the tape freed).  Either way the tape starts empty.  One rank only: on
        several ranks this and the five methods below raise FftBaroError with the engine's message."""
        self._call("adjoint_record", int(depth))

    def adjoint_recorded(self): return self._count("adjoint_recorded")

    def checkpoint_adjoint(self, every, max_steps=0):
        """Adjoint checkpointing on (every >= 1: a checkpoint of the state before every step of the window whose index is a multiple of
        `every`, a tape segment of `every` steps, a window of at most max_steps steps) or off (every = 0, everything freed); it and
        record_adjoint replace each other, and either way the window starts empty.  The forward run writes no tape; adjoint_back fills
        the segment again from the checkpoints, one more forward step per backward step, and gives the bits of the full tape.  Memory:
        ceil(max_steps / every) + 4 every + 1 half spectra (checkpoint_every(max_steps) minimises it) where record_adjoint takes
        4 max_steps.  One rank only, as record_adjoint."""
        self._call("adjoint_checkpoint", int(every), int(max_steps))

    def adjoint_checkpoints(self):
        """(every, max_steps, checkpoints, replayed): the mode's two settings, the checkpoints the window holds and the steps taken
        again by sweeps since it began (a window swept completely has replayed its own length); all 0 while the mode is off."""
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
        self._call("adjoint_checkpoint_info", C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return a.value, b.value, c.value, d.value

    def set_adjoint(self, lam):
        """Sets the adjoint variable, a field (the gradient of a scalar of the state with respect to the vorticity, at the time of the
        newest recorded step); lam=None removes it."""
        self._one_rank("set_adjoint", None)
        self._hand("set_adjoint", self._dev(lam))

    def adjoint(self): return self._get("adjoint", 1)[0]

    def adjoint_back(self, n=1):
        """lam <- T^T lam over the last n recorded steps, newest first (the transpose of the tangent-linear step); they leave the tape."""
        self._call("adjoint_back", int(n))

    def adjoint_rewind(self, n=-1):
        """Un-pops the last n steps that adjoint_back popped (n = -1: every one still on the tape): a sweep does not erase a slot, so
        the same steps can be swept again, with the same bits.  A step recorded after a pop overwrites the slots above it.  Refused under
        checkpoint_adjoint and while a particle adjoint is set.  Nothing is launched."""
        self._call("adjoint_rewind", int(n))

    def tangent_replay(self, first, n):
        """Applies the tangent step of the taped steps first .. first + n - 1 (0: the oldest step on record_adjoint's tape), oldest first,
        to every perturbation of the tangent set, from the recorded stage states: nothing nonlinear is stepped, and the vorticity, a
        tracer, particles, the tape and adjoint_recorded() stay as they are.  The base flow's fields are formed once per stage for the
        whole set (4 + 5 M fields transformed per stage, where M perturbations stepped beside the vorticity take 10 M).  The operator of
        the live tangent, not its bits; perturbation k of a set has the bits of the replayed set of one.  Steps that a sweep has popped
        can still be replayed.  It needs a tangent set and the full tape; n = 0 does nothing."""
        self._call("tangent_replay", int(first), int(n))

    def observe_tangent(self, kind, xy, k=0):
        """h = H dz_k: observe() of perturbation k of the tangent set in the place of the resident state, a float64 [n] tensor; for
        "vort" bit for bit sample(tangents()[k], xy).  It changes nothing."""
        t = self.torch
        self._one_rank("observe_tangent", 0, 0, _SOME, 1, _SOME)
        a = particles_dev(t, xy)
        out = t.empty(a.shape[0], dtype=t.float64, device="cuda")
        self._hand("observe_tangent", int(k), obs_kind(kind), a, int(a.shape[0]), out)
        return out

    def singular_values(self, steps, iters, start):
        """(sigmas, v): power iteration on T^T T over `steps` steps from the current state in the L2 norm (singular_values()); the
        state is kept and put back through _STATE."""
        self._one_rank("adjoint_record", int(steps))
        return singular_values(self, steps, iters, start, save=getattr(self, self._STATE[0]), restore=getattr(self, self._STATE[1]))

    def set_adjoints(self, lam):
        """Sets an adjoint subspace: M adjoint variables, [M, nx, ny] (numpy or torch, 1 <= M <= ADJOINTS_MAX), swept back over the ONE
        tape by adjoint_back, each as set_adjoint's one (variable k is bit for bit what set_adjoint of lam[k] and the same sweep give);
        whatever set was there is replaced, set_adjoint's one too; lam=None removes all.  set_adjoint replaces a set by its one, and
        adjoint() returns variable 0.  adjoint_add_obs is refused while a set of several is there.  One rank only, as set_adjoint."""
        t = self.torch
        self._one_rank("set_adjoints", None, 1)
        if lam is None:
            return self._hand("set_adjoints", None, 0)
        m = fields_arg(lam, self._shape, "set_adjoints", ADJOINTS_MAX)
        if isinstance(lam, np.ndarray):
            lam = t.from_numpy(np.ascontiguousarray(lam, dtype=np.float32))
        self._hand("set_adjoints", lam.cuda().contiguous(), m)

    def adjoint_count(self): return self._count("adjoint_count")

    def adjoints(self):
        """every adjoint variable, float32 [M, nx, ny] (with none set the engine's refusal is raised)"""
        out = self.torch.empty((max(self.adjoint_count(), 1),) + self._shape, dtype=self.torch.float32, device="cuda")
        self._hand("get_adjoints", out)
        return out

    def singular_vectors(self, steps, k, iters, start=None, checkpoint_every=None, replay=False):
        """(sigma [iters, k], V [k, nx, ny]): the k leading singular values and right singular vectors of the tangent over `steps`
        steps from the current state, by block power iteration with a tangent subspace and an adjoint set of k (singular_vectors());
        the state is kept and put back through _STATE.  checkpoint_every: None the full tape, an int K or "sqrt" checkpoints.
        replay=True: one forward run, then tangent_replay over its tape in every iteration (no nonlinear step per iteration)."""
        self._one_rank("adjoint_record", int(steps))
        return singular_vectors(self, steps, k, iters, start, save=getattr(self, self._STATE[0]), restore=getattr(self, self._STATE[1]),
                                checkpoint_every=checkpoint_every, replay=replay)

    def scatter(self, w, xy):
        """The transpose of sample(): n point values w, float64 [n], at the positions xy, float64 [n, 2], spread onto the grid with the
        cubic Lagrange weights of sample(), field[i, j] = sum over the points of w wx wy: a float32 [nx, ny] tensor with
        <sample(f, xy), w> = <f, scatter(w, xy)>.  Bitwise reproducible, in any order of the points (fixed-point accumulation,
        include/fftbaro.h); a point whose position or weight is not finite deposits nothing.  It needs nothing set: it is also how a
        quantity carried by particles is deposited on the grid.  One rank only: on several ranks this and the three methods below raise
        FftBaroError with the engine's message."""
        t = self.torch
        self._one_rank("scatter", _SOME, _SOME, 1, _SOME)
        a = particles_dev(t, xy)
        out = t.empty(self._shape, dtype=t.float32, device="cuda")
        self._hand("scatter", a, values_dev(t, w, int(a.shape[0]), "w"), int(a.shape[0]), out)
        return out

    def observe(self, kind, xy):
        """h = H zeta: the resident state's "vort", "u", "v" or "psi" at the positions xy, float64 [n, 2]: a float64 [n] tensor, bit for
        bit sample(vort(), xy) or sample(diag()[k], xy), without the field leaving the engine.  It changes nothing."""
        t = self.torch
        self._one_rank("observe", 0, _SOME, 1, _SOME)
        a = particles_dev(t, xy)
        out = t.empty(a.shape[0], dtype=t.float64, device="cuda")
        self._hand("observe", obs_kind(kind), a, int(a.shape[0]), out)
        return out

    def obs_misfit(self, h, y, sigma, cost, check=True):
        """r = (h - y) / sigma^2, a float64 [n] tensor, and cost += 1/2 sum (h - y)^2 / sigma^2 on the GPU, summed in a fixed order;
        h, y float64 [n], sigma float64 [n] or None (1), cost a float64 tensor of one element on the GPU.  Every sigma must be positive
        and finite: checked here on the tensor unless check=False (the engine does not look)."""
        t = self.torch
        self._one_rank("obs_misfit", _SOME, _SOME, None, 1, _SOME, _SOME)
        n = int(h.shape[0])
        h, y = values_dev(t, h, n, "h"), values_dev(t, y, n, "y")
        sigma = None if sigma is None else values_dev(t, sigma, n, "sigma")
        if check and sigma is not None and not sigma_ok(sigma):
            raise ValueError("obs_misfit: every sigma must be positive and finite")
        assert cost.is_cuda and cost.dtype == t.float64 and cost.numel() == 1 and cost.is_contiguous()
        r = t.empty(n, dtype=t.float64, device="cuda")
        self._hand("obs_misfit", h, y, sigma, n, r, cost)
        return r

    def adjoint_add_obs(self, kind, xy, w):
        """lam += H^T w for the adjoint variable set by set_adjoint: the forcing of the backward sweep by n point values w (the misfits
        r of obs_misfit) of the kind observed at xy.  Between two adjoint_back calls it is a cost term at an intermediate time."""
        t = self.torch
        self._one_rank("adjoint_add_obs", 0, _SOME, _SOME, 1)
        a = particles_dev(t, xy)
        self._hand("adjoint_add_obs", obs_kind(kind), a, values_dev(t, w, int(a.shape[0]), "w"), int(a.shape[0]))

    def fourdvar(self, z0, obs, background=None, checkpoint_every=None, particles=None, keep_tape=False):
        """(J, grad): the 4D-Var cost of the initial vorticity z0 against the Observations in obs, and its gradient with respect to z0,
        float64 [nx, ny] on the GPU (fourdvar()).  The tape takes T x 4 half spectra, T the last observation step; with
        checkpoint_every = K (or "sqrt": checkpoint_every(T)) ceil(T / K) + 4 K + 1 of them, for windows whose tape does not fit.
        particles: the drifters' initial positions for sets of kind "position"; dJ/dX0 is left in particle_adjoint().
        keep_tape=True leaves the tape, rewound, for gauss_newton_hvp (the same J and grad; the full tape only)."""
        self._one_rank("adjoint_record", 1)
        return fourdvar(self, z0, obs, background, checkpoint_every, particles, keep_tape)

    def gauss_newton_hvp(self, v, obs, background=None):
        """H_GN v, float64 [nx, ny] on the GPU: the Gauss-Newton Hessian-vector product of the 4D-Var cost about the trajectory that
        fourdvar(..., keep_tape=True) left on the tape (gauss_newton_hvp()): one tangent replay and one sweep, nothing nonlinear stepped.
        It REPLACES a tangent set and an adjoint set the user had, and removes the tangent set at the end."""
        self._one_rank("tangent_replay", 0, 0)
        return gauss_newton_hvp(self, v, obs, background)

    def fit_incremental(self, z0, obs, outer, inner, background=None, cg_tol=1e-2):
        """(z, J_history, evaluations, hvps): incremental (Gauss-Newton) 4D-Var from the first guess z0 (fit_incremental()): `outer`
        nonlinear runs, each followed by at most `inner` conjugate-gradient steps on the quadratic model; z0 goes to the GPU first."""
        self._one_rank("tangent_replay", 0, 0)
        if isinstance(z0, np.ndarray):
            z0 = self.torch.from_numpy(np.ascontiguousarray(z0))
        return fit_incremental(self, z0.cuda(), obs, outer, inner, background, cg_tol)

    def fit_initial(self, z0, obs, iters, background=None, history=8, checkpoint_every=None, particles=None):
        """(z, J_history, evaluations): L-BFGS on fourdvar from the first guess z0 (fit_initial()); z0 goes to the GPU first, so the
        iterate, the gradients and the memory of the recursion stay there.  checkpoint_every, particles: as fourdvar's."""
        self._one_rank("adjoint_record", 1)
        if isinstance(z0, np.ndarray):
            z0 = self.torch.from_numpy(np.ascontiguousarray(z0))
        return fit_initial(self, z0.cuda(), obs, iters, background, history, checkpoint_every=checkpoint_every, particles=particles)

    def record_particles(self, depth):
        """Turns the particle tape on (depth >= 1: room for depth steps; every step from now on records the positions its four stages
        start from, 64 bytes per particle and step, and a step call beyond depth is refused) or off (depth = 0, the tape freed).
        Either way it starts empty.  It needs particles; set_vort and set_particles empty it.  While it is on the model steps eagerly.
        The positions and everything else stepped are the same bits with and without.  One rank only, as the particles."""
        self._call("particle_tape", int(depth))

    def particles_recorded(self):
        """(steps on the particle tape, its depth); (0, 0) while it is off"""
        a, b = C.c_int(), C.c_int()
        self._call("particle_tape_count", C.byref(a), C.byref(b))
        return a.value, b.value

    def set_particle_adjoint(self, xbar):
        """Sets the particle adjoint Xb, float64 [n, 2] (numpy or torch): the gradient of a scalar with respect to the particles'
        positions at the time of the newest recorded step; xbar=None removes it.  While it is set adjoint_back sweeps it back with
        lam through the transpose of the coupled step, popping the particle tape too: Xb <- its value at the earlier time, and lam
        gains the sensitivity of the positions to the vorticity.  Bitwise reproducible, in any order of the particles."""
        self._one_rank("set_particle_adjoint", _SOME)
        if xbar is None:
            return self._hand("set_particle_adjoint", None)
        a = particles_dev(self.torch, xbar)
        if int(a.shape[0]) != self.particle_count():
            raise ValueError("set_particle_adjoint: float64 [%d, 2], one row per particle" % self.particle_count())
        self._hand("set_particle_adjoint", a)

    def particle_adjoint(self):
        """The particle adjoint Xb, a float64 [n, 2] tensor."""
        t = self.torch
        self._one_rank("get_particle_adjoint", _SOME)
        out = t.empty((max(self.particle_count(), 1), 2), dtype=t.float64, device="cuda")
        self._hand("get_particle_adjoint", out)
        return out

    def set_forcing(self, rate=0.0, k=None, width=None, seed=0, drag=0.0, hyper_nu=0.0, hyper_order=1):
        """Stochastic ring forcing, linear drag and hyperviscosity as a split stage after every step (include/fftbaro.h,
        fb_model_set_forcing): zeta <- D zeta + Delta_n, D = exp(-(drag + hyper_nu K^(2 hyper_order)) dt), Delta_n white in time on
        the ring |K - k| <= width [rad/m], injecting `rate` [m^2 s^-3] of energy per unit time, from Philox4x32-10 keyed on (mode,
        forcing clock, seed).  rate = drag = hyper_nu = 0 (the defaults) removes the stage; rate = 0 alone is pure dissipation and
        needs no ring.  The perturbations of the tangent set are multiplied by D.  One rank only; refused while the adjoint's tape
        or a checkpointed window exists, and record_adjoint / checkpoint_adjoint are refused while forcing is set."""
        none = rate == 0
        self._call("set_forcing", float(rate), 0.0 if none and k is None else float(k), 0.0 if none and width is None else float(width),
                   int(seed) & 0xFFFFFFFFFFFFFFFF, float(drag), float(hyper_nu), int(hyper_order))

    FORCING_BUDGET = ("clock", "dE_forc", "dE_diss", "dZ_forc", "dZ_diss", "n_ring")

    def forcing_budget(self):
        """{"clock": split stages since set_forcing, "dE_forc", "dE_diss", "dZ_forc", "dZ_diss": the running totals of the energy
        E = <|u|^2> / 2 and the enstrophy Z = <zeta^2> / 2 that the increments added and the factor D removed (float64, summed in
        the stage's own pass in a fixed order: the bits repeat), "n_ring": the ring's modes over the full spectrum}"""
        out = (C.c_double * 6)()
        self._call("forcing_budget", out)
        d = dict(zip(self.FORCING_BUDGET, out))
        d["clock"], d["n_ring"] = int(d["clock"]), int(d["n_ring"])
        return d

    def forcing_increment(self, n):
        """Delta_n of the forcing clock's value n, a complex64 tensor [nx, ny/2+1] in the layout of the spectrum (zeros off the ring)"""
        t = self.torch
        self._one_rank("forcing_increment", 0, _SOME)
        out = t.empty((self.nx, self.ny // 2 + 1), dtype=t.complex64, device="cuda")
        self._hand("forcing_increment", int(n), out)
        return out


class Model(ModelSurface):
    """The main.cpp RK4 driver state (main.cpp:103-317) resident in HBM, fused stepping."""

    _PREFIX, _STATE = "fb_model_", ("spectrum", "set_spectrum")      # (the spectrum restores every bit)

    def __init__(self, nx, ny=None, Lx=600000.0, Ly=600000.0, nu=6.5, dt=3.0):
        ny = ny or nx
        self.fop = FftwfOperation(nx, ny, Lx, Ly)
        self.torch = self.fop.torch
        self.nx, self.ny, self.hy = nx, ny, ny // 2 + 1
        self._shape = (nx, ny)
        self.Lx, self.Ly = Lx, Ly
        self.nu, self.dt = float(np.float32(nu)), float(np.float32(dt))
        h = C.c_void_p()
        check(lib().fb_model_create(C.byref(h), self.fop._h, nu, dt))
        self._h = h

    def close(self):
        ModelSurface.close(self)
        self.fop.close()

    def _wait(self): self.fop.synchronize()

    def use_graph(self, enable=True):
        """hipGraph replay of the step; call under a non-default torch stream (after fop.use_current_stream())."""
        self._call("use_graph", 1 if enable else 0)

    KERNEL_CLASSES = ("k_col_strided_bwd4", "k_row_fused", "k_col_strided_fwd1", "k_col_mid")

    def profile_steps(self, n):
        """HIP-event time per kernel class over n steps: {class: (total_ms, launches)}."""
        ms = (C.c_float * 4)(); cnt = (C.c_int * 4)()
        self._call("profile_steps", n, ms, cnt)
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.KERNEL_CLASSES)}

    def spectrum(self):
        out = self.fop.empty_spec(); self._call("get_spectrum", _ptr(out)); return out

    def set_spectrum(self, spec): self._call("set_spectrum", self.fop._spec(spec))

    def info(self):
        a, b = C.c_size_t(), C.c_size_t()
        self._call("info", C.byref(a), C.byref(b))
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
