"""CPU checks of the balanced-pressure record output (fb_model_get_pressure, fb_slab_get_pressure_local): declared, exported, bound,
argument checks that run before any HIP call, the drop-in driver links the path and refuses a reference point outside the grid at
option parsing (exit status 2).  No GPU needed."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
NAMES = ("fb_model_get_pressure", "fb_slab_get_pressure_local")
FB_EINVAL = 1


def test_pressure_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    from importlib import import_module
    slab = import_module("xlab-fftbarotropic_amd.slab")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == 6, n
    assert callable(X.Model.pressure)
    assert callable(slab.EngineSlab.pressure_local)


def test_pressure_null_handles_and_outputs_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.fb_model_get_pressure(None, 1.0, 1e-5, 0, 0, p) == FB_EINVAL
    assert b"fb_model_get_pressure" in L.fb_last_error()
    assert L.fb_model_get_pressure(None, 1.0, 1e-5, 0, 0, None) == FB_EINVAL
    assert L.fb_model_get_pressure(None, 1.0, 1e-5, -1, 0, p) == FB_EINVAL
    assert L.fb_slab_get_pressure_local(None, 1.0, 1e-5, 0, 0, p) == FB_EINVAL
    assert b"fb_slab_get_pressure_local" in L.fb_last_error()
    assert L.fb_slab_get_pressure_local(None, 1.0, 1e-5, 0, 0, None) == FB_EINVAL
    assert L.fb_slab_get_pressure_local(None, 1.0, 1e-5, 0, -1, p) == FB_EINVAL


def _driver():
    import xlab_fftbarotropic_amd as X
    X.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "barotropic_main.out")
    assert os.access(exe, os.X_OK)
    return exe


def test_driver_links_the_pressure_path():
    exe = _driver()
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    for n in NAMES:
        assert n in und, n
    blob = open(exe, "rb").read()
    for opt in (b"dump-pressure", b"pres-rho", b"pres-f", b"pres-ref-x", b"pres-ref-y"):
        assert opt in blob, opt


def test_driver_refuses_a_reference_point_outside_the_grid(tmp_path):
    """exit status 2 at option parsing, before any file or device is touched: a negative coordinate, a flat index ref_x + npts * ref_y
    beyond the field, wherever --npts stands on the command line; a point inside the grid passes the option check (the run then
    ends for another reason: no device, or no input file)."""
    exe = _driver()

    def run(*args):
        return subprocess.run([exe, "-I", str(tmp_path), "-O", str(tmp_path), "--steps", "1", "--dump-pressure"] + list(args), cwd=str(tmp_path),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for args in (("--pres-ref-x", "-1"), ("--pres-ref-y", "-1"), ("--npts", "256", "--pres-ref-x", "0", "--pres-ref-y", "256"),
                 ("--pres-ref-x", "256", "--pres-ref-y", "255", "--npts", "256"), ("--npts", "256", "--pres-ref-x", "65536"),
                 ("--pres-ref-x", "3x"), ("--pres-ref-y", "")):
        r = run(*args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "pres-ref" in r.stderr, (args, r.stderr)
        assert not os.path.exists(os.path.join(str(tmp_path), "log")), args
    r = run("--npts", "256", "--pres-ref-x", "255", "--pres-ref-y", "255")
    assert r.returncode != 2 and "pres-ref" not in r.stderr, (r.returncode, r.stderr)
