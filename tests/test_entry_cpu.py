"""CPU checks of the entry layer of the C ABI (csrc/fb_entry.h): every fb_model_* / fb_slab_* function that takes a handle refuses a
NULL one under its own name, and the two halves of a pair check their arguments in the same order.  No GPU needed: every call here is
refused before any HIP call."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

FB_EINVAL = 1
# no handle to refuse: constructors, destroy (NULL is fine) and the host-side plan functions
SKIPPED = ("fb_model_create", "fb_slab_create", "fb_model_destroy", "fb_slab_destroy", "fb_slab_unique_id", "fb_slab_plan", "fb_slab_geometry",
           "fb_slab_col_groups")
# the int parameters that 1 is not a valid value of: nbins
INT_ARGS = {"get_eddy_diffusivity": {1: 16}, "get_tracer_eddy_diffusivity": {1: 16}, "get_azimuthal": {4: 16}}


def _binding():
    import xlab_fftbarotropic_amd as X
    return X, sys.modules[X.Model.__module__]


def _stem(name):
    return name.replace("fb_model_", "").replace("fb_slab_", "").replace("_local", "")


def _valid_args(B, name, argtypes, keep):
    """otherwise valid arguments after the handle: non-NULL pointers, kind / mode 1, counts 1 (16 bins), factors 1.0"""
    out = []
    for i, t in enumerate(argtypes[1:], 1):
        if t is C.c_int:
            out.append(INT_ARGS.get(_stem(name), {}).get(i, 1))
        elif t in (C.c_float, C.c_double):
            out.append(1.0)
        elif t is C.c_size_t:
            out.append(1)
        elif t is C.c_char_p:
            keep.append(C.create_string_buffer(b"x", 128))
            out.append(keep[-1])
        elif t is B.ALLTOALL_FN:
            keep.append(B.ALLTOALL_FN(lambda *a: 0))
            out.append(keep[-1])
        else:                                                    # c_void_p or POINTER(...): a host buffer that nothing gets to write
            keep.append((C.c_double * 64)())
            out.append(C.cast(keep[-1], t))
    return out


def test_every_handle_taking_entry_point_refuses_a_null_handle_under_its_own_name():
    X, B = _binding()
    L = X.lib()
    walked, keep = [], []
    for name, (argtypes, restype) in B.SIGNATURES.items():
        if not name.startswith(("fb_model_", "fb_slab_")) or name in SKIPPED:
            continue
        assert argtypes[0] is C.c_void_p and restype is None, name
        rc = getattr(L, name)(None, *_valid_args(B, name, argtypes, keep))
        msg = L.fb_last_error().decode()
        assert rc == FB_EINVAL, (name, rc, msg)
        assert msg.startswith(name + ": NULL " + ("model" if name.startswith("fb_model_") else "slab")), (name, msg)
        walked.append(name)
    assert len(walked) >= 68, len(walked)
    for stem in B._PAIRS:
        if stem != "destroy":
            assert "fb_slab_" + stem in walked and "fb_model_" + stem.replace("_local", "") in walked, stem


# (pair, arguments after the handle with one of them wrong, the phrase that names it)
BAD_ARGS = [("tangent_norm", (2, "out"), "kind"),
            ("tangent_scale", (0.0,), "finite"), ("tangent_scale", (float("nan"),), "finite"), ("tangent_scale", (float("inf"),), "finite"),
            ("set_tracer", ("out", -1.0), "kappa"), ("adjoint_record", (-1,), "depth"), ("adjoint_back", (-1,), "nsteps"),
            ("get_eddy_diffusivity", (1, "out", None, None), "nbins")]


@pytest.mark.parametrize("stem,args,phrase", BAD_ARGS, ids=["%s%r" % (s, a) for s, a, _ in BAD_ARGS])
def test_both_halves_of_a_pair_report_the_argument_before_the_null_handle(stem, args, phrase):
    X, B = _binding()
    L = X.lib()
    buf = (C.c_double * 64)()
    args = [C.cast(buf, C.c_void_p) if a == "out" else a for a in args]
    slab = [n for n in B._PAIRS if n.replace("_local", "") == stem][0]
    for name in ("fb_model_" + stem, "fb_slab_" + slab):
        assert getattr(L, name)(None, *args) == FB_EINVAL, name
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and phrase in msg and "NULL" not in msg, (name, msg)
