"""CPU checks of the shell spectra record output (fb_spectra_shells, fb_model_get_spectra, fb_slab_get_spectra): declared, exported,
bound, argument checks that run before any HIP call, the shell count, the numpy restatement's own geometry, the drop-in driver links
the path.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
NAMES = ("fb_spectra_shells", "fb_model_get_spectra", "fb_slab_get_spectra")
FB_EINVAL = 1
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def test_spectra_entry_points_declared_exported_and_bound():
    import xlab_fftbarotropic_amd as X
    from importlib import import_module
    slab = import_module("xlab-fftbarotropic_amd.slab")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    L = X.lib()
    for n, nargs in zip(NAMES, (5, 2, 2)):
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
        assert hasattr(L, n), n
        assert n in X.EXPORTS, n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == nargs, n
    assert callable(X.Model.spectra) and callable(X.spectra_shells)
    assert callable(slab.EngineSlab.spectra)
    assert len(X.SPECTRA_COLUMNS) == 10


def test_spectra_null_handles_and_tables_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    buf = (ctypes.c_double * 20)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.fb_model_get_spectra(None, p) == FB_EINVAL
    assert b"fb_model_get_spectra" in L.fb_last_error()
    assert L.fb_model_get_spectra(None, None) == FB_EINVAL
    assert b"fb_model_get_spectra" in L.fb_last_error()
    assert L.fb_slab_get_spectra(None, p) == FB_EINVAL
    assert b"fb_slab_get_spectra" in L.fb_last_error()
    assert L.fb_slab_get_spectra(None, None) == FB_EINVAL
    assert b"fb_slab_get_spectra" in L.fb_last_error()


def test_shell_count():
    import xlab_fftbarotropic_amd as X
    import spectra_numpy as SN
    L = X.lib()
    assert X.spectra_shells(256, 256, 6e5, 6e5) == 182
    assert X.spectra_shells(16384, 16384, 6e5, 6e5) == 11586
    assert X.spectra_shells(768) == 544 and X.spectra_shells(4096) == 2897
    for nx, ny, lx, ly, want in ((256, 128, 6e5, 3e5, 182), (256, 128, 3e5, 6e5, 265), (128, 16384, 6e5, 6e5, None), (16384, 64, 6e5, 6e5, None)):
        got = X.spectra_shells(nx, ny, lx, ly)
        assert got == SN.nshells(nx, ny, lx, ly), (nx, ny, lx, ly)
        assert want is None or got == want
    n = ctypes.c_int(7)
    assert L.fb_spectra_shells(256, 256, 6e5, 6e5, None) == FB_EINVAL
    assert b"fb_spectra_shells" in L.fb_last_error()
    for args in ((256, 256, 0.0, 6e5), (256, 256, 6e5, -1.0), (256, 250, 6e5, 6e5), (32, 256, 6e5, 6e5), (32768, 256, 6e5, 6e5)):
        assert L.fb_spectra_shells(*args, ctypes.byref(n)) == FB_EINVAL, args
        assert b"fb_spectra_shells" in L.fb_last_error()


def test_restatement_geometry():
    """the numpy restatement: every mode of the full spectrum is counted once, the corner mode lies in the last shell, shell 0 holds the
    mean mode only, and no mode of the grids the GPU tests use lies within 1e-9 shells of a shell edge"""
    import spectra_numpy as SN
    for nx, ny, lx, ly in ((256, 256, 6e5, 6e5), (768, 768, 6e5, 6e5), (256, 128, 6e5, 3e5), (256, 128, 3e5, 6e5), (128, 16384, 6e5, 6e5),
                           (16384, 64, 6e5, 6e5)):
        k2, b, w, dk, edge = SN.geometry(nx, ny, lx, ly)
        ns = SN.nshells(nx, ny, lx, ly)
        n = np.bincount(b.ravel(), weights=w.ravel(), minlength=ns)
        assert n.sum() == nx * ny and len(n) == ns and n[0] == 1.0 and n[-1] >= 1.0
        assert b[nx // 2, ny // 2] == ns - 1
        assert edge >= 1e-9, (nx, ny, edge)


def _driver():
    import xlab_fftbarotropic_amd as X
    X.build_lib()
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "barotropic_main.out")
    assert os.access(exe, os.X_OK)
    return exe


def test_driver_links_the_spectra_path():
    exe = _driver()
    und = subprocess.run(["nm", "-D", "--undefined-only", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    for n in NAMES:
        assert n in und, n
    assert b"dump-spectra" in open(exe, "rb").read()
