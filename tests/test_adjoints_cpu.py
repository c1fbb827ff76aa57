"""CPU checks of the adjoint subspace: the pair table of its entry points, the Python argument checks that run before the library is
called, the float64 block power iteration (tests/singular_numpy.py) against a dense SVD of the tangent matrix of a small grid, and the
float32 figure from which the GPU test's principal-angle bar is taken (tests/test_gpu_adjoints.py).  No GPU needed."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adjoint_numpy as A                                       # noqa: E402
import singular_numpy as S                                      # noqa: E402

STEMS = ("set_adjoints", "get_adjoints", "adjoint_count")
FB_EINVAL = 1


def _binding():
    return import_module("xlab-fftbarotropic_amd.binding")


# ---- the pair table ----
def test_pair_table_holds_exactly_the_new_stems():
    import xlab_fftbarotropic_amd as X
    B = _binding()
    assert set(B._ADJOINTS_PAIRS) == set(STEMS) and not set(B._ADJOINTS_PAIRS) & set(B._PAIRS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    want = {"set_adjoints": r"const float \*d_lambda_real, int count", "get_adjoints": r"float \*d_real", "adjoint_count": r"int \*count"}
    for stem in STEMS:
        for kind, handle in (("model", r"fb_model \*m"), ("slab", r"fb_slab \*s")):
            name = "fb_%s_%s" % (kind, stem)
            assert re.search(r"\bint\s+%s\s*\(%s, %s\)\s*;" % (name, handle, want[stem]), src), name
            assert name in X.EXPORTS and name in B.SIGNATURES, name
            assert len(B.SIGNATURES[name][0]) == 1 + len(B._ADJOINTS_PAIRS[stem]), name
    assert re.search(r"#define\s+FB_ADJOINTS_MAX\s+32\b", src) and B.ADJOINTS_MAX == 32 == X.ADJOINTS_MAX
    slab = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (X.Model, slab.EngineSlab):
        for n in ("set_adjoints", "adjoints", "adjoint_count", "singular_vectors"):
            assert callable(getattr(cls, n, None)), (cls, n)
    assert callable(X.singular_vectors)


def test_argument_errors_are_refused_by_the_engine_without_a_device():
    """NULL handles, a NULL output and a count outside [1, 32]: FB_EINVAL and a message that starts with the function's name, before
    any HIP call (there is no device here)"""
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    w = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    cnt = ctypes.c_int(7)
    for kind in ("model", "slab"):
        for stem, args, word in (("set_adjoints", (None, w, 2), b"NULL " + kind.encode()), ("get_adjoints", (None, w), b"NULL " + kind.encode()),
                                 ("adjoint_count", (None, ctypes.byref(cnt)), b"NULL " + kind.encode()),
                                 ("set_adjoints", (None, w, 0), b"count outside [1, 32]"), ("set_adjoints", (None, w, 33), b"count outside [1, 32]"),
                                 ("get_adjoints", (None, None), b"NULL output"), ("adjoint_count", (None, None), b"NULL output")):
            name = "fb_%s_%s" % (kind, stem)
            assert getattr(L, name)(*args) == FB_EINVAL, (name, args)
            msg = L.fb_last_error()
            assert msg.startswith(name.encode() + b": ") and word in msg, (name, msg)
    assert cnt.value == 7


# ---- the Python argument checks ----
def _model_without_a_library(monkeypatch):
    import torch
    B = _binding()

    def called(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(B, "_entry", called)
    monkeypatch.setattr(B, "lib", called)
    m = B.Model.__new__(B.Model)
    m.torch, m._shape, m._h, m.nx, m.ny = torch, (8, 8), None, 8, 8
    return B, m, torch


def test_python_argument_checks_raise_before_the_library_is_called(monkeypatch):
    B, m, torch = _model_without_a_library(monkeypatch)
    bad = [np.zeros((8, 8), np.float32),                        # rank
           np.zeros((2, 2, 8, 8), np.float32),
           np.zeros((2, 8, 9), np.float32),                     # another grid
           np.zeros((2, 8, 8), np.int32),                       # dtype
           np.zeros((2, 8, 8), np.complex64),
           torch.zeros((2, 8, 8), dtype=torch.float64),
           np.zeros((0, 8, 8), np.float32),                     # M out of range
           np.zeros((33, 8, 8), np.float32),
           torch.zeros((33, 8, 8), dtype=torch.float32)]
    for a in bad:
        with pytest.raises(ValueError, match="set_adjoints"):
            m.set_adjoints(a)
    for kw in (dict(steps=2, k=33, iters=1), dict(steps=2, k=0, iters=1), dict(steps=0, k=2, iters=1), dict(steps=2, k=2, iters=0),
               dict(steps=2, k=2, iters=1, start=np.zeros((3, 8, 8))), dict(steps=2, k=2, iters=1, start=np.zeros((8, 8)))):
        with pytest.raises(ValueError, match="singular_vectors"):
            m.singular_vectors(**kw)
        with pytest.raises(ValueError, match="singular_vectors"):
            B.singular_vectors(m, **kw)
    with pytest.raises(AssertionError, match="the library was called"):
        m.adjoint_count()                                       # (the patch is live: a call that does reach the library shows)


# ---- the reference iteration ----
def test_principal_sine():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((3, 50))
    mix = rng.standard_normal((3, 3))
    assert S.principal_sine(a, mix @ a) <= 1e-12               # the same span in another basis
    q = S.orthonormal_rows(rng.standard_normal((4, 50)))
    th = 0.3
    b = np.array([q[0], q[1], np.cos(th) * q[2] + np.sin(th) * q[3]])
    assert abs(S.principal_sine(q[:3], b) - np.sin(th)) <= 1e-12
    assert abs(np.abs(q @ q.T - np.eye(4)).max()) <= 1e-14


def test_block_power_iteration_against_a_dense_svd():
    """32^2, 4 steps of 20 s: T column by column from the float64 tangent model and numpy's SVD of it; k = 4 with sigma_4 / sigma_5 >=
    1.05 in that spectrum; the iteration from white noise until every sigma moves by less than 1e-12 relative stops before the cap of
    200 iterations and agrees with the SVD to 1e-9; the subspace is the SVD's to 1e-5 (the angle goes like the square root of sigma's
    error)"""
    m = S.dense_model()
    z0 = m.spectrum()
    tm = S.tangent_matrix(m, z0, S.DENSE_STEPS)
    _, sv, vt = np.linalg.svd(tm)
    k = S.DENSE_K
    gap = sv[k - 1] / sv[k]
    start = np.random.default_rng(S.DENSE_SEED).standard_normal((k, S.DENSE_N, S.DENSE_N))
    sig, v = S.singular_vectors(m, z0, S.DENSE_STEPS, k, S.DENSE_CAP, start, tol=1e-12)
    err = float(np.max(np.abs(sig[-1] / sv[:k] - 1)))
    ang = S.principal_sine(v, vt[:k])
    print("dense SVD, %d^2, %d steps of %g s: sigma_1..%d = %s, gap %.4f; %d iterations, sigma off by %.3g, the subspace by %.3g"
          % (S.DENSE_N, S.DENSE_STEPS, S.DENSE_DT, k + 1, np.round(sv[:k + 1], 3), gap, len(sig), err, ang))
    assert gap >= 1.05
    assert len(sig) < S.DENSE_CAP
    assert err <= 1e-9
    assert ang <= 1e-5
    assert np.array_equal(m.spectrum(), z0) and m.adjoint_recorded() == 0       # the state restored, the tape off


def test_float32_figure_of_the_principal_angle():
    """The case of the GPU test (256^2, SV_STEPS steps, SV_ITERS iterations, k = 4, white-noise start): the float32 restatement's final
    subspace lies within SV_ANGLE_F32 of float64's (the sine of the largest principal angle; recorded, an upper bound to 1.5 for
    another FFT library's summation order) and its sigma within SV_SIGMA_F32; the GPU's bar is 4 x the angle's figure"""
    s64, v64 = S.sv_reference()
    s32, v32 = S.sv_reference(A.Float32Model)
    ang = S.principal_sine(v32, v64)
    err = float(np.max(np.abs(s32 / s64 - 1)))
    print("block power iteration, %d^2, %d steps, %d iterations, k = %d: sigma (float64) =\n%s\nfloat32 on the CPU: sigma off by %.3g, sine of the largest principal angle %.3g"
          % (S.SV_N, S.SV_STEPS, S.SV_ITERS, S.SV_K, s64, err, ang))
    assert s64.shape == (S.SV_ITERS, S.SV_K) and v64.shape == (S.SV_K, S.SV_N, S.SV_N)
    assert (np.diff(s64, axis=1) <= 0).all()                    # sorted descending
    assert (s64[-1] >= s64[0]).all()                            # the iteration moves towards the leading subspace
    assert ang <= 1.5 * S.SV_ANGLE_F32
    assert err <= 1.5 * S.SV_SIGMA_F32 and S.SV_SIGMA_F32 <= S.SV_BAR / 4
    assert S.SV_ANGLE_BAR == 4 * S.SV_ANGLE_F32
