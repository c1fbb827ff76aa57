"""CPU checks of the effective eddy diffusivity record output (fb_model_get_eddy_diffusivity, fb_slab_get_eddy_diffusivity): declared,
exported, bound, argument checks that run before any HIP call, and the drop-in driver that calls them links and refuses a bad
--keff-bins before it touches a device.  No GPU needed."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
NAMES = ("fb_model_get_eddy_diffusivity", "fb_slab_get_eddy_diffusivity")
FB_EINVAL = 1


def test_eddy_diffusivity_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None, n
    assert X.EDDY_DIFFUSIVITY_COLUMNS == ("Q_lo", "Q_hi", "n", "A", "A_ge", "S", "Le2", "r_e", "K_eff")


def test_eddy_diffusivity_null_handles_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    buf = (ctypes.c_double * 16)()
    t = ctypes.cast(buf, ctypes.c_void_p)
    assert L.fb_model_get_eddy_diffusivity(None, 256, t, None, None) == FB_EINVAL
    assert b"fb_model_get_eddy_diffusivity" in L.fb_last_error()
    assert L.fb_model_get_eddy_diffusivity(None, 256, None, None, None) == FB_EINVAL
    assert L.fb_slab_get_eddy_diffusivity(None, 256, t, None, None) == FB_EINVAL
    assert L.fb_slab_get_eddy_diffusivity(None, 1, None, None, None) == FB_EINVAL


def test_driver_links_the_eddy_diffusivity_path_and_checks_the_bin_count(tmp_path):
    import xlab_fftbarotropic_amd as X
    X.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "barotropic_main.out")
    assert os.access(exe, os.X_OK)
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    for n in NAMES:
        assert n in und, n
    blob = open(exe, "rb").read()
    assert b"dump-eddy-diffusivity" in blob and b"keff-bins" in blob
    for bad in ("1", "4097", "0", "-3", "12x", ""):
        r = subprocess.run([exe, "--npts", "64", "--steps", "1", "--dump-eddy-diffusivity", "--keff-bins", bad], cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
        assert b"--keff-bins" in r.stderr
    assert not os.path.exists(str(tmp_path / "log"))
