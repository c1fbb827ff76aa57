"""CPU checks of the Python boundary: binding.SIGNATURES against every prototype of include/fftbaro.h, and the one model surface that
binding.Model and slab.EngineSlab share.  No GPU, no compute call."""
import ctypes as C
import inspect
import os
import re
from importlib import import_module

from test_abi import _declared
from test_slab_cpu import _PLANS, _geometry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


def _prototypes():
    """[(return type, name, [parameter, ...])] of every function the header declares; (void) is no parameter"""
    src = open(os.path.join(ROOT, "include", "fftbaro.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith(("typedef", "#", "extern", "}")))
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(fb_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = [" ".join(p.split()) for p in params.split(",")]
        out.append((" ".join(ret.split()), name, [] if params == ["void"] else params))
    return out


def _is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_signatures_match_the_header():
    B = import_module("xlab-fftbarotropic_amd.binding")
    protos = _prototypes()
    checked = 0
    for ret, name, params in protos:
        assert name in B.SIGNATURES, name
        argtypes, restype = B.SIGNATURES[name]
        assert len(argtypes) == len(params), (name, params)
        for p, t in zip(params, argtypes):
            words = p.replace("const ", "").split()
            if "*" in p:
                assert _is_pointer_type(t), (name, p, t)
            elif words[0] == "fb_alltoall_fn":
                assert t is B.ALLTOALL_FN, (name, p, t)
            else:
                assert len(words) == 2 and t is SCALARS[words[0]], (name, p, t)
        if ret == "const char *":
            assert restype is C.c_char_p, name
        else:
            assert ret == "int" and restype in (None, C.c_int), (name, ret)
        checked += 1
    declared = _declared()
    assert sorted(n for _, n, _ in protos) == declared and checked == len(declared) >= 45
    assert B.EXPORTS == list(B.SIGNATURES) and set(B.EXPORTS) == set(declared)
    L = B.lib()
    for name, (argtypes, restype) in B.SIGNATURES.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == list(argtypes), name
        assert fn.restype is (restype or C.c_int), name


# the public callables of the two classes before they shared a surface
MODEL = ["close", "set_vort", "set_source", "step", "use_graph", "time_steps", "profile_steps", "vort", "diag", "okubo_weiss",
         "eddy_diffusivity", "pressure", "spectra", "azimuthal", "set_tracer", "tracer", "tracer_eddy_diffusivity", "set_particles",
         "particle_count", "particles", "sample", "set_tangent", "tangent", "tangent_norm", "rescale_tangent", "lyapunov",
         "record_adjoint", "adjoint_recorded", "set_adjoint", "adjoint", "adjoint_back", "singular_values", "spectrum", "set_spectrum",
         "info"]
ENGINE_SLAB = ["set_vort_local", "set_source_local", "step", "vort_local", "diag_local", "okubo_weiss_local", "eddy_diffusivity",
               "pressure_local", "spectra", "azimuthal", "set_tracer_local", "tracer_local", "tracer_eddy_diffusivity", "set_particles",
               "particle_count", "particles", "sample", "set_tangent", "tangent", "tangent_norm", "rescale_tangent", "lyapunov",
               "record_adjoint", "adjoint_recorded", "set_adjoint", "adjoint", "adjoint_back", "singular_values", "transport_selftest",
               "transport_info", "time_steps", "synchronize", "close"]
# a shared method that a class defines again, and why
OVERRIDES = {("Model", "close"): "the model owns its operator context (fop) and closes it after itself"}


def _public_callables(cls):
    return {n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n))}


def test_one_model_surface(monkeypatch):
    B = import_module("xlab-fftbarotropic_amd.binding")
    slab = import_module("xlab-fftbarotropic_amd.slab")
    M, E = B.Model, slab.EngineSlab
    assert set(MODEL) <= _public_callables(M), set(MODEL) - _public_callables(M)
    assert set(ENGINE_SLAB) <= _public_callables(E), set(ENGINE_SLAB) - _public_callables(E)
    pairs = [(n, n) for n in MODEL if n in ENGINE_SLAB] + [(n[:-len("_local")], n) for n in ENGINE_SLAB if n.endswith("_local")]
    assert len(pairs) == 30 and all(m in MODEL for m, _ in pairs)
    for m, e in pairs:
        assert inspect.signature(getattr(M, m)) == inspect.signature(getattr(E, e)), (m, e)
        if getattr(M, m) is not getattr(E, e):                      # defined once, or a named override of the shared definition
            base = getattr(B.ModelSurface, m)
            assert [(c.__name__, m) for c, f in ((M, getattr(M, m)), (E, getattr(E, e))) if f is not base] \
                == [k for k in OVERRIDES if k[1] == m], (m, e)
    assert len(OVERRIDES) <= 5
    # the slab module needs no GPU, and its plan is the engine's
    for env in [k for k in os.environ if k.startswith("FB_SLAB_")]:
        monkeypatch.delenv(env)
    p = slab.plan(4096, 4096, 4)
    assert (p.XL, p.KA, p.KF) == _geometry(4096, 4096, 4)
    assert (p.col_groups, p.field_groups, p.row_chunks, p.ops) == _PLANS[(4096, 4096, 4)]
