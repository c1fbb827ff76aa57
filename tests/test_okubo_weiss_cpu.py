"""CPU checks of the Okubo-Weiss record output (fb_model_get_okubo_weiss, fb_slab_get_okubo_weiss_local): declared, exported,
bound, argument checks that run before any HIP call, and the drop-in driver that calls them still links.  No GPU needed."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
NAMES = ("fb_model_get_okubo_weiss", "fb_slab_get_okubo_weiss_local")
FB_EINVAL = 1


def test_okubo_weiss_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None, n
    assert L.fb_version() == 201


def test_okubo_weiss_null_handles_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    buf = (ctypes.c_float * 4)()
    w = ctypes.cast(buf, ctypes.c_void_p)
    assert L.fb_model_get_okubo_weiss(None, w, w) == FB_EINVAL
    assert L.fb_model_get_okubo_weiss(None, None, None) == FB_EINVAL
    assert b"fb_model_get_okubo_weiss" in L.fb_last_error()
    assert L.fb_slab_get_okubo_weiss_local(None, w, w) == FB_EINVAL
    assert L.fb_slab_get_okubo_weiss_local(None, None, None) == FB_EINVAL


def test_driver_links_the_okubo_weiss_path():
    import xlab_fftbarotropic_amd as X
    X.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "barotropic_main.out")
    assert os.access(exe, os.X_OK)
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    for n in NAMES:
        assert n in und, n
    assert b"dump-okubo-weiss" in open(exe, "rb").read()
