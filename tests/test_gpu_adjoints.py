"""The adjoint subspace on the GPU (fb_model_set_adjoints, fb_model_get_adjoints, fb_model_adjoint_count; kernels csrc/fb_adjoint.h:
k_adjoint_base, k_adjoint_mu, k_adjoint_prod_set; host side csrc/fb_beside_adjoint.h, adjoint_stage_set): variable k of a set against the single
adjoint variable bit for bit on every kernel path of adjoint_numpy.PATH_CASES, the set's bounds and sweep arithmetic, its isolation
from the step, the transpose as a matrix against the tangent subspace, Model.singular_vectors against the float64 block power iteration
(tests/singular_numpy.py), the slab of one rank, the refusals and fb_model_info.  DESIGN.md, "Adjoint subspace", has the tables."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adjoint_numpy as A                                       # noqa: E402
import singular_numpy as S                                      # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in A.PATH_CASES]
M_SET = 3
FB_EINVAL = 1


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _noise_set(nx, ny, m, rms, seed=A.SEED + 10):
    """m fields of white noise, never dealiased, of the rms given, float32 [m, nx, ny]"""
    return (np.random.default_rng(seed).standard_normal((m, nx, ny)) * rms).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny, m=M_SET):
    """(vort, dz, source, lams [m, nx, ny]): the inputs of adjoint_numpy (its case's noise; 3e-2 off the table); lams[0] is its lam"""
    noise = [k.vort_noise for k in A.PATH_CASES if (k.nx, k.ny) == (nx, ny)] or [A.PATH_CASES[0].vort_noise]
    v, d, s, lam = A.adjoint_inputs(nx, ny, noise[0])
    lams = _noise_set(nx, ny, m, np.sqrt(np.mean(v.astype(np.float64) ** 2)))
    lams[0] = lam
    out = (v, d, s, lams)
    for a in out:
        a.setflags(write=False)
    return out


def _model(nx, ny, cls=None, **kw):
    import xlab_fftbarotropic_amd as X
    v, _, s, _ = _inputs(nx, ny)
    m = (cls or X.Model)(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny), **kw)
    m.set_vort(v)
    m.set_source(s)
    return m


def _sweep(m, nx, ny, steps, lam, back=None):
    """the model set to the case's vorticity again (which empties the tape), `steps` steps recorded, lam set (a [M, nx, ny] set or one
    [nx, ny] field), swept back in the pieces of `back` (default: at once): the adjoint variables as numpy"""
    m.set_vort(_inputs(nx, ny)[0])
    m.record_adjoint(steps)
    m.step(steps)
    if lam.ndim == 3:
        m.set_adjoints(lam)
    else:
        m.set_adjoint(lam)
    for n in back or (steps,):
        m.adjoint_back(n)
    assert m.adjoint_recorded() == 0
    return _np(m.adjoints()) if lam.ndim == 3 else _np(m.adjoint())


@functools.lru_cache(maxsize=None)
def _set_and_singles(nx, ny, steps, m_set=M_SET, which=(0, 1, 2)):
    """(the set's sweep [m_set, nx, ny], {k: the single variable's sweep from lams[k]}) on one model, once per case"""
    lams = _inputs(nx, ny, m_set)[3]
    m = _model(nx, ny)
    got = _sweep(m, nx, ny, steps, lams)
    assert m.adjoint_count() == m_set
    singles = {}
    for k in which:
        singles[k] = _sweep(m, nx, ny, steps, lams[k])
        assert m.adjoint_count() == 1
    m.close()
    return got, singles


# ---- 1. bit equality on every kernel path ----
@pytest.mark.parametrize("case", A.PATH_CASES, ids=CASE_IDS)
def test_set_is_bit_equal_to_single_variables_on_every_path(case):
    """a set of 3 white-noise lam, never dealiased, swept back over the case's 5 steps: adjoints()[k] has the bits of adjoint() of a run
    with set_adjoint(lam[k]) over the same tape, k = 0, 1, 2; and the sweep is not the identity"""
    got, singles = _set_and_singles(case.nx, case.ny, case.steps)
    lams = _inputs(case.nx, case.ny)[3]
    assert got.shape == (M_SET, case.nx, case.ny)
    for k in range(M_SET):
        assert _same32(got[k], singles[k]), (case.what, k)
        assert rel_l2(got[k], lams[k]) > 1e-3
    assert not _same32(got[0], got[1])


# ---- 2. the bounds of the count ----
def test_bounds_of_the_count():
    """64^2, 2 steps, M = 32: variables 0, 17 and 31 bit-equal to their single runs; M = 33 and M = 0 refused before any HIP call, by the
    engine (the C call on a live model) and by the Python surface"""
    import xlab_fftbarotropic_amd as X
    n = 64
    got, singles = _set_and_singles(n, n, 2, 32, (0, 17, 31))
    assert got.shape == (32, n, n)
    for k, one in singles.items():
        assert _same32(got[k], one), k
    m = _model(n, n)
    lams = _inputs(n, n, 32)[3]
    m.set_adjoints(lams[:2])
    big = m.torch.zeros((33, n, n), dtype=m.torch.float32, device="cuda")
    L = X.lib()
    for count in (33, 0, -1):
        assert L.fb_model_set_adjoints(m._h, ctypes.c_void_p(big.data_ptr()), count) == FB_EINVAL
        assert L.fb_last_error().startswith(b"fb_model_set_adjoints: count outside [1, 32]")
        assert m.adjoint_count() == 2                           # the set that was there stays
    for bad in (big, big[:0]):
        with pytest.raises(ValueError, match="set_adjoints"):
            m.set_adjoints(bad)
    m.close()


# ---- 3. sweep arithmetic ----
def test_sweep_arithmetic():
    import xlab_fftbarotropic_amd as X
    n = 256
    steps = A.case_of(n, n).steps
    lams = _inputs(n, n)[3]
    whole = _set_and_singles(n, n, steps)[0]
    m = _model(n, n)
    assert m.adjoint_count() == 0
    with pytest.raises(X.FftBaroError, match="no adjoint is set"):
        m.adjoints()
    assert _same32(_sweep(m, n, n, steps, lams, back=(3, 2)), whole)        # 3 then 2 == 5 at once
    assert _same32(_sweep(m, n, n, steps, lams), whole)                     # two equal runs give the same bits
    m.set_adjoints(lams)
    back = _np(m.adjoints())
    for k in range(M_SET):
        assert rel_l2(back[k], lams[k]) <= 1e-6                             # in and out
    assert _same32(_np(m.adjoint()), back[0])                               # adjoint() is variable 0 of a set
    m.set_adjoint(lams[1])
    assert m.adjoint_count() == 1 and _same32(_np(m.adjoint()), back[1]) and _np(m.adjoints()).shape == (1, n, n)
    m.set_adjoints(lams)
    assert m.adjoint_count() == M_SET
    m.set_adjoints(lams[:2])
    assert m.adjoint_count() == 2 and _same32(_np(m.adjoints()), back[:2])
    m.set_adjoints(None)
    assert m.adjoint_count() == 0
    with pytest.raises(X.FftBaroError, match="no adjoint is set"):
        m.adjoint_back(0)
    m.close()


# ---- 4. isolation ----
@pytest.mark.parametrize("nx,ny", [(256, 256), (1024, 64)])
def test_step_is_bit_equal_with_and_without_a_set(nx, ny):
    """vorticity, tracer, particles and a tangent after 6 steps, with a set of 3 that comes after 3 of them and without, each with and
    without use_graph"""
    import torch
    import particles_numpy as P
    v, d, s, lams = _inputs(nx, ny)
    c0 = T.noisy_inputs(nx, ny, 3e-2)[1]
    x0 = P.seed_positions(nx, ny, 600000.0, 600000.0, 64, seed=5)
    out = []
    for graph in (False, True):
        for with_set in (False, True):
            with torch.cuda.stream(torch.cuda.Stream()):
                m = _model(nx, ny)
                m.fop.use_current_stream()
                m.use_graph(graph)
                m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
                m.set_particles(x0)
                m.set_tangent(d)
                m.step(3)
                if with_set:
                    m.set_adjoints(lams)
                m.step(3)
                assert m.adjoint_count() == (M_SET if with_set else 0)
                out.append((_np(m.vort()), _np(m.tracer()), _np(m.particles()), _np(m.tangent())))
                m.close()
    for o in out[1:]:
        assert _same32(out[0][0], o[0]) and _same32(out[0][1], o[1]) and _same32(out[0][3], o[3])
        assert np.array_equal(out[0][2].view(np.uint64), o[2].view(np.uint64))
    assert rel_l2(out[0][0], v) > 1e-6 and rel_l2(out[0][3], d) > 1e-4


# ---- 5. the transpose as a matrix ----
@pytest.mark.parametrize("n", [256, 192])
def test_transpose_as_a_matrix_against_the_tangent_subspace(n):
    """a tangent subspace of 3 and an adjoint set of 3 over 5 steps: every |<T d_i, lam_j> - <d_i, T^T lam_j>| / (|T d_i| |lam_j|), the dot
    products in float64 on the host, at most adjoint_numpy.DOT_BAR"""
    steps = A.case_of(n, n).steps
    v, d, s, lams = _inputs(n, n)
    ds = _noise_set(n, n, M_SET, np.sqrt(np.mean(d.astype(np.float64) ** 2)), seed=A.SEED + 20)
    ds[0] = d
    m = _model(n, n)
    m.set_tangents(ds)
    m.record_adjoint(steps)
    m.step(steps)
    td = _np(m.tangents())
    m.set_adjoints(lams)
    m.adjoint_back(steps)
    tl = _np(m.adjoints())
    m.close()
    res = np.array([[A.dot_residual(td[i], lams[j], ds[i], tl[j]) for j in range(M_SET)] for i in range(M_SET)])
    print("transpose as a matrix %d^2, %d steps: residuals\n%s\nbar %.3g" % (n, steps, res, A.DOT_BAR))
    assert res.max() <= A.DOT_BAR


# ---- 6. singular vectors ----
def test_singular_vectors_against_float64():
    """Model.singular_vectors at 256^2, SV_STEPS steps, SV_ITERS iterations, k = 4 from the white-noise start of singular_numpy against the
    same iteration in float64: every sigma of every iteration within SV_BAR; the final subspaces within SV_ANGLE_BAR (the sine of the
    largest principal angle; 4 x the float32 restatement's figure on the CPU, tests/test_adjoints_cpu.py); the state restored bit for
    bit and the tape freed; two calls with start=None agree"""
    n, k = S.SV_N, S.SV_K
    s64, v64 = S.sv_reference()
    start = S.sv_start()
    m = _model(n, n)
    before = _np(m.vort())
    sg, vg = m.singular_vectors(S.SV_STEPS, k, S.SV_ITERS, start)
    assert m.adjoint_recorded() == 0
    assert _same32(_np(m.vort()), before)
    vg = _np(vg)
    err = np.abs(sg / s64 - 1)
    ang = S.principal_sine(vg, v64)
    print("singular_vectors %d^2, %d steps, %d iterations, k = %d: GPU sigma\n%s\nfloat64\n%s\noff by at most %.3g (bar %.3g); sine of the largest principal angle %.3g"
          " (float32 on the CPU %.3g, bar %.3g)" % (n, S.SV_STEPS, S.SV_ITERS, k, sg, s64, err.max(), S.SV_BAR, ang, S.SV_ANGLE_F32, S.SV_ANGLE_BAR))
    assert sg.shape == (S.SV_ITERS, k) and vg.shape == (k, n, n) and vg.dtype == np.float32
    q = vg.reshape(k, -1).astype(np.float64)
    assert np.abs(q @ q.T - np.eye(k)).max() <= 1e-6            # orthonormal (rounded to float32 on the way out)
    a = m.singular_vectors(1, 2, 1)
    b = m.singular_vectors(1, 2, 1)
    assert np.array_equal(a[0], b[0]) and _same32(_np(a[1]), _np(b[1]))
    assert _same32(_np(m.vort()), before)
    m.close()
    assert err.max() <= S.SV_BAR
    assert ang <= S.SV_ANGLE_BAR


# ---- 7. the slab ----
def test_slab_of_one_rank_matches_the_model():
    S_ = _slab()
    n = 256
    steps = A.case_of(n, n).steps
    v, _, src, lams = _inputs(n, n)
    s = S_.EngineSlab(n, n, nu=A.G.NU, dt=T.recipe_dt(n, n))
    s.set_vort_local(v)
    s.set_source_local(src)
    s.record_adjoint(steps)
    s.step(steps)
    s.set_adjoints(lams)
    assert s.adjoint_count() == M_SET
    s.adjoint_back(steps)
    assert _same32(_np(s.adjoints()), _set_and_singles(n, n, steps)[0])
    s.set_adjoints(None)
    assert s.adjoint_count() == 0
    s.record_adjoint(0)
    s.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: the three new entry points raise with the engine's message"""
    import threading
    import torch
    import xlab_fftbarotropic_amd as X
    S_ = _slab()
    n, world = 256, 2
    hub = S_.local_hub(world)
    msgs, errs = [[] for _ in range(world)], [None] * world

    def work(r):
        try:
            s = S_.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                buf = torch.zeros((2, s.XL, n), dtype=torch.float32, device="cuda")
                calls = (lambda: s.set_adjoints(np.zeros((2, s.XL, n), np.float32)), lambda: s.set_adjoints(None), lambda: s._hand("get_adjoints", buf),
                         s.adjoint_count, s.adjoints, lambda: s.singular_vectors(1, 2, 1, np.zeros((2, s.XL, n), np.float32)))
                for call in calls:
                    try:
                        call()
                        msgs[r].append(None)
                    except X.FftBaroError as e:
                        msgs[r].append(str(e))
            finally:
                s.close()
        except BaseException as e:                                          # noqa: BLE001 -- re-raised below
            errs[r] = e
    try:
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        S_.local_hub_destroy(hub)
    for e in errs:
        if e is not None:
            raise e
    names = ("set_adjoints", "set_adjoints", "get_adjoints", "adjoint_count", "adjoint_count", "adjoint_record")
    for r in range(world):
        assert len(msgs[r]) == len(names)
        for msg, name in zip(msgs[r], names):
            assert msg is not None and "invalid argument" in msg.lower() and "fb_slab_" + name in msg, msg
            assert "the adjoint model is not supported on a slab of several ranks (world > 1)" in msg, msg


# ---- 8. refusals ----
def test_refusals_under_each_entry_points_own_name():
    """status FB_EINVAL and a message that starts with the function's name: the NULL handle, a NULL pointer, the count out of range, get
    without a set, adjoint_add_obs with a set of 2; fb_model_* on a model and fb_slab_* on a slab of one rank"""
    import torch
    import xlab_fftbarotropic_amd as X
    S_ = _slab()
    L = X.lib()
    n = 64
    v, _, _, lams = _inputs(n, n, 32)
    m = X.Model(n, n)
    s = S_.EngineSlab(n, n)
    buf = torch.zeros((2, n, n), dtype=torch.float32, device="cuda")
    xy = torch.full((1, 2), 1000.0, dtype=torch.float64, device="cuda")
    w = torch.ones(1, dtype=torch.float64, device="cuda")
    cnt = ctypes.c_int(-5)
    p, pc = ctypes.c_void_p(buf.data_ptr()), ctypes.byref(cnt)
    pxy, pw = ctypes.c_void_p(xy.data_ptr()), ctypes.c_void_p(w.data_ptr())
    torch.cuda.synchronize()
    for prefix, obj, null in (("fb_model_", m, "NULL model"), ("fb_slab_", s, "NULL slab")):
        h = obj._h
        obj.set_vort(v) if prefix == "fb_model_" else obj.set_vort_local(v)
        table = [                                                # (entry point, arguments, what the message holds)
            ("set_adjoints", (None, p, 2), null), ("get_adjoints", (None, p), null), ("adjoint_count", (None, pc), null),
            ("get_adjoints", (h, None), "NULL output"), ("adjoint_count", (h, None), "NULL output"),
            ("set_adjoints", (h, p, 0), "count outside [1, 32]"), ("set_adjoints", (h, p, 33), "count outside [1, 32]"),
            ("get_adjoints", (h, p), "no adjoint is set"),
        ]
        for stem, args, word in table:
            name = prefix + stem
            assert getattr(L, name)(*args) == FB_EINVAL, (name, args)
            msg = L.fb_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (name, msg)
        assert getattr(L, prefix + "adjoint_count")(h, pc) == 0 and cnt.value == 0          # (no set: 0, not a refusal)
        assert getattr(L, prefix + "set_adjoints")(h, p, 2) == 0
        name = prefix + "adjoint_add_obs"
        assert getattr(L, name)(h, 0, pxy, pw, 1) == FB_EINVAL
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and "a set of 2 adjoint variables" in msg, msg
        with pytest.raises(X.FftBaroError, match="a set of 2 adjoint variables"):
            obj.adjoint_add_obs("vort", xy, w)
        assert getattr(L, prefix + "set_adjoint")(h, p) == 0                                # the one: the forcing is taken again
        assert getattr(L, name)(h, 0, pxy, pw, 1) == 0
        obj._wait()
    m.close()
    s.close()


# ---- 9. fb_model_info ----
def test_info_counts_the_set_and_its_workspace():
    """hbm_bytes grows by what DESIGN.md, "Adjoint subspace", says a set of M costs: M x 3 half spectra, (4 + 5 C) real fields and C half
    spectra with C = min(M, 8) (the set of one: 3 half spectra and 5 real fields), and returns to its value after set_adjoints(None);
    the half spectrum's padded size is taken from the tracer's 3"""
    n = 256
    v, _, _, _ = _inputs(n, n)
    lams = _noise_set(n, n, 10, 1.0)
    m = _model(n, n)
    h0 = m.info()["hbm_bytes"]
    m.set_tracer(v)
    half, rem = divmod(m.info()["hbm_bytes"] - h0, 3)
    m.set_tracer(None)
    assert rem == 0 and half >= n * (n // 2 + 1) * 8 and m.info()["hbm_bytes"] == h0
    real = n * n * 4
    for count in (3, 1, 10, 8):
        c = min(count, 8)
        want = count * 3 * half + (5 * real if count == 1 else (4 + 5 * c) * real + c * half)
        if count == 1:
            m.set_adjoint(lams[0])
        else:
            m.set_adjoints(lams[:count])
        assert m.info()["hbm_bytes"] == h0 + want, count
    m.set_adjoints(None)
    assert m.info()["hbm_bytes"] == h0
    m.close()
