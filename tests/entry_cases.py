"""The refusal table of the model/slab entry points of the C ABI (tests/test_gpu_entry.py, tests/golden/make_entry_fixture.py): the
calls, the handles they are made on and how an argument recipe becomes ctypes arguments.

The handles are one Model(64) and one unconnected slab, rank 0 of world 2 on the one GPU.  An entry is (function, arguments, phrase);
the arguments are JSON values, with the tokens
  "M" / "S"   the model's / the slab's handle
  "buf"       a zeroed device buffer, large enough for any output at 64 x 64 (no case gets as far as writing it)
  "field"     a zeroed float32 [64, 64] field on the device (a valid input of the set-up calls)
  "host"      a small host buffer (an int or float output)
  null        a NULL pointer
Every entry has exactly one thing wrong and is refused before anything is launched.  An entry whose phrase is "" is a set-up call with
valid arguments that must return FB_OK: the tape and the adjoint variable that the last two range checks need."""
import ctypes

N = 64
DX = 6.0e5 / N
PMAX = 1 << 24

GETTER_BEFORE_SET = [
    ("fb_model_get_tracer", ["M", "buf"], "no tracer is set"),
    ("fb_model_get_tracer_eddy_diffusivity", ["M", 16, "buf", None, None], "no tracer is set"),
    ("fb_slab_get_tracer_local", ["S", "buf"], "no tracer is set"),
    ("fb_slab_get_tracer_eddy_diffusivity", ["S", 16, "buf", None, None], "no tracer is set"),
    ("fb_model_get_tangent", ["M", "buf"], "no tangent is set"),
    ("fb_model_tangent_norm", ["M", 0, "buf"], "no tangent is set"),
    ("fb_model_tangent_scale", ["M", 2.0], "no tangent is set"),
    ("fb_model_get_particles", ["M", "buf"], "no particles are set"),
    ("fb_model_get_adjoint", ["M", "buf"], "no adjoint is set"),
    ("fb_model_adjoint_back", ["M", 1], "no adjoint is set"),
    ("fb_model_get_tangents", ["M", "buf"], "no tangent is set"),
    ("fb_model_tangent_gram", ["M", 0, "buf"], "no tangent is set"),
    ("fb_model_tangent_qr", ["M", 0, "buf"], "no tangent is set"),
]
ONE_RANK_ONLY = [(fn, args, "several ranks") for fn, args in [
    ("fb_slab_set_tangent", ["S", "field"]), ("fb_slab_get_tangent", ["S", "buf"]),
    ("fb_slab_tangent_norm", ["S", 0, "buf"]), ("fb_slab_tangent_scale", ["S", 2.0]),
    ("fb_slab_set_particles", ["S", "buf", 100]), ("fb_slab_get_particles", ["S", "buf"]), ("fb_slab_sample", ["S", "field", "buf", 100, "buf"]),
    ("fb_slab_adjoint_record", ["S", 1]), ("fb_slab_adjoint_recorded", ["S", "host"]), ("fb_slab_set_adjoint", ["S", "field"]),
    ("fb_slab_get_adjoint", ["S", "buf"]), ("fb_slab_adjoint_back", ["S", 1]),
    ("fb_slab_set_tangents", ["S", "field", 1]), ("fb_slab_get_tangents", ["S", "buf"]), ("fb_slab_tangent_count", ["S", "host"]),
    ("fb_slab_tangent_gram", ["S", 0, "buf"]), ("fb_slab_tangent_qr", ["S", 0, "buf"]),
]]
NOT_CONNECTED = [(fn, args, "not connected") for fn, args in [
    ("fb_slab_set_vort_local", ["S", "field"]), ("fb_slab_step", ["S", 1]), ("fb_slab_time_steps", ["S", 1, "host"]),
    ("fb_slab_get_vort_local", ["S", "buf"]), ("fb_slab_get_diag_local", ["S", "buf", "buf", "buf"]),
    ("fb_slab_get_okubo_weiss_local", ["S", "buf", "buf"]), ("fb_slab_get_eddy_diffusivity", ["S", 16, "buf", None, None]),
    ("fb_slab_get_pressure_local", ["S", 1.0, 1e-5, 0, 0, "buf"]), ("fb_slab_get_spectra", ["S", "buf"]),
    ("fb_slab_get_azimuthal", ["S", 1, 0.0, 0.0, 16, DX, 4, "buf", "buf"]), ("fb_slab_set_tracer_local", ["S", "field", 0.0]),
]]
RANGE_CHECKS = [
    ("fb_model_get_eddy_diffusivity", ["M", 1, "buf", None, None], "nbins"),
    ("fb_model_get_eddy_diffusivity", ["M", 4097, "buf", None, None], "nbins"),
    ("fb_model_get_tracer_eddy_diffusivity", ["M", 1, "buf", None, None], "nbins"),
    ("fb_model_get_tracer_eddy_diffusivity", ["M", 4097, "buf", None, None], "nbins"),
    ("fb_model_get_azimuthal", ["M", 1, 0.0, 0.0, 1, DX, 4, "buf", "buf"], "nbins"),
    ("fb_model_get_azimuthal", ["M", 1, 0.0, 0.0, 4097, DX, 4, "buf", "buf"], "nbins"),
    ("fb_slab_get_azimuthal", ["S", 1, 0.0, 0.0, 1, DX, 4, "buf", "buf"], "nbins"),
    ("fb_model_get_azimuthal", ["M", 1, 0.0, 0.0, 16, DX, 9, "buf", "buf"], "nmodes"),
    ("fb_slab_get_azimuthal", ["S", 1, 0.0, 0.0, 16, DX, 9, "buf", "buf"], "nmodes"),
    ("fb_model_get_azimuthal", ["M", 1, 0.0, 0.0, 16, 0.0, 4, "buf", "buf"], "dr below"),
    ("fb_slab_get_azimuthal", ["S", 1, 0.0, 0.0, 16, 0.0, 4, "buf", "buf"], "dr below"),
    ("fb_model_get_pressure", ["M", 1.0, 1e-5, -1, 0, "buf"], "reference point"),
    ("fb_model_get_pressure", ["M", 1.0, 1e-5, 0, N, "buf"], "reference point"),
    ("fb_slab_get_pressure_local", ["S", 1.0, 1e-5, -1, 0, "buf"], "reference point"),
    ("fb_slab_get_pressure_local", ["S", 1.0, 1e-5, 0, N, "buf"], "reference point"),
    ("fb_model_set_particles", ["M", "buf", 0], "n outside"),
    ("fb_model_set_particles", ["M", "buf", PMAX + 1], "n outside"),
    ("fb_model_sample", ["M", "field", "buf", 0, "buf"], "n outside"),
    ("fb_model_sample", ["M", "field", "buf", PMAX + 1, "buf"], "n outside"),
    ("fb_model_set_tracer", ["M", "field", -1.0], "kappa"),
    ("fb_slab_set_tracer_local", ["S", "field", -1.0], "kappa"),
    ("fb_model_tangent_norm", ["M", 2, "buf"], "kind"),
    ("fb_model_tangent_scale", ["M", 0.0], "finite"),
    ("fb_model_step", ["M", -1], "bad argument"),
    ("fb_model_adjoint_record", ["M", -1], "depth"),
    ("fb_model_adjoint_back", ["M", -1], "nsteps"),
    ("fb_model_set_tangents", ["M", "field", 0], "count outside"),
    ("fb_model_set_tangents", ["M", "field", 33], "count outside"),
    ("fb_model_tangent_gram", ["M", 2, "buf"], "kind"),
    ("fb_model_tangent_qr", ["M", 2, "buf"], "kind"),
    # a tape of one step, then two steps asked for; an adjoint variable, then one recorded step asked back of none
    ("fb_model_adjoint_record", ["M", 1], ""),
    ("fb_model_step", ["M", 2], "tape"),
    ("fb_model_set_adjoint", ["M", "field"], ""),
    ("fb_model_adjoint_back", ["M", 1], "recorded"),
    ("fb_model_set_adjoint", ["M", None], ""),
    ("fb_model_adjoint_record", ["M", 0], ""),
]
ENTRIES = GETTER_BEFORE_SET + ONE_RANK_ONLY + NOT_CONNECTED + RANGE_CHECKS


class Handles:
    """Model(64), the unconnected slab and the buffers the recipes name"""

    def __init__(self):
        import xlab_fftbarotropic_amd as X
        self.L = X.lib()
        self.model = X.Model(N, N)
        t = self.model.torch
        self.buf = t.zeros(4 * N * N, dtype=t.float64, device="cuda")
        self.field = t.zeros((N, N), dtype=t.float32, device="cuda")
        self.host = (ctypes.c_double * 4)()
        t.cuda.synchronize()
        self.slab = ctypes.c_void_p()
        if self.L.fb_slab_create(ctypes.byref(self.slab), N, N, 6e5, 6e5, 6.5, 3.0, 0, 2) != 0:
            raise X.FftBaroError(self.L.fb_last_error().decode())

    def close(self):
        self.model.torch.cuda.synchronize()
        self.L.fb_slab_destroy(self.slab)
        self.model.close()

    def arg(self, a, argtype):
        if a == "M":
            return self.model._h
        if a == "S":
            return self.slab
        if a in ("buf", "field"):
            return ctypes.c_void_p(getattr(self, a).data_ptr())
        if a == "host":
            return ctypes.cast(self.host, argtype)
        return a

    def call(self, fn, args):
        """(return code, fb_last_error()) of one entry"""
        f = getattr(self.L, fn)
        rc = f(*[self.arg(a, t) for a, t in zip(args, f.argtypes)])
        return rc, self.L.fb_last_error().decode()
