"""The adjoint model on the GPU (fb_model_adjoint_record, fb_model_set_adjoint, fb_model_adjoint_back; kernels csrc/fb_adjoint.h) against the
float64 reference (tests/adjoint_numpy.py) on the grid classes that take different branches of stage_vstate and of the row and column
dispatch, and against the GPU's own tangent-linear model (the dot-product identity).

The inputs are adjoint_numpy.adjoint_inputs: tangent_numpy.tangent_inputs (never-dealiased noise on zeta and dz, a vorticity source)
and lam as white noise, never dealiased, so every field carries state in every masked mode.  adjoint_numpy.PATH_CASES holds per
case the probe shift and the float32 figures that make the bars decisive (asserted on the CPU in tests/test_adjoint_cpu.py).  One
line of figures per case (pytest -s); DESIGN.md, "Adjoint model", has the tables."""
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
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in A.PATH_CASES]


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    out = A.adjoint_inputs(nx, ny, A.case_of(nx, ny).vort_noise)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(nx, ny):
    """(lam_0, vort) of the float64 run of a case, computed once"""
    case = A.case_of(nx, ny)
    r = A.run_case(nx, ny, *_inputs(nx, ny), case.steps)
    out = (r.adjoint(), r.vort())
    for a in out:
        a.setflags(write=False)
    return out


def _gpu_model(nx, ny, vort, dz, source, dt=None):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    if dz is not None:
        m.set_tangent(dz)
    return m


@functools.lru_cache(maxsize=None)
def _gpu_run(nx, ny):
    """record, step, set lam, sweep back on the GPU, once per case: (lam straight after set_adjoint, lam_0, vort, T dz)"""
    case = A.case_of(nx, ny)
    v, d, s, lam = _inputs(nx, ny)
    m = _gpu_model(nx, ny, v, d, s)
    m.record_adjoint(case.steps)
    m.step(case.steps)
    assert m.adjoint_recorded() == case.steps
    m.set_adjoint(lam)
    l_in = _np(m.adjoint())
    m.adjoint_back(case.steps)
    assert m.adjoint_recorded() == 0
    out = (l_in, _np(m.adjoint()), _np(m.vort()), _np(m.tangent()))
    m.close()
    return out


# ---- 1. the path matrix ----
@pytest.mark.parametrize("case", A.PATH_CASES, ids=CASE_IDS)
def test_path_against_float64(case):
    """record, step, set lam, sweep back: lam_0 within 1e-5 relative L2 of AdjointModel64, the vorticity within 1e-5, adjoint() straight
    after set_adjoint within 1e-6 of the input"""
    nx, ny = case.nx, case.ny
    lam = _inputs(nx, ny)[3]
    l_in, l0, gv, _ = _gpu_run(nx, ny)
    rl, rv = _reference(nx, ny)
    e0, el, ev = rel_l2(l_in, lam), rel_l2(l0, rl), rel_l2(gv, rv)
    print("path %dx%d (%s), %d steps: lam_0 rel L2 = %.3g, vorticity rel L2 = %.3g, lam in and out %.3g; probe shift %.3g, float32 on the CPU %.3g"
          % (nx, ny, case.what, case.steps, el, ev, e0, case.shift, case.f32))
    assert e0 <= 1e-6
    assert el <= 1e-5
    assert ev <= 1e-5
    assert rel_l2(rl, lam) > 1e-3


# ---- 2. the dot-product identity against the GPU's own tangent ----
@pytest.mark.parametrize("case", A.PATH_CASES, ids=CASE_IDS)
def test_dot_product_identity_against_the_gpu_tangent(case):
    """|<T dz, lam> - <dz, T^T lam>| / (|T dz| |lam|) with T dz from the engine's tangent-linear model and T^T lam from its adjoint, the
    dot products in float64 on the host, at most DOT_BAR: 4 times the largest figure that the float32 restatement gives on the CPU
    over these cases (adjoint_numpy.PATH_CASES, f32_dot; tests/test_adjoint_cpu.py asserts them)"""
    nx, ny = case.nx, case.ny
    _, d, _, lam = _inputs(nx, ny)
    _, l0, _, td = _gpu_run(nx, ny)
    res = A.dot_residual(td, lam, d, l0)
    print("dot-product identity %dx%d, %d steps: GPU %.3g, float32 on the CPU %.3g, bar %.3g" % (nx, ny, case.steps, res, case.f32_dot, A.DOT_BAR))
    assert res <= A.DOT_BAR


# ---- 3. bit-equality ----
@pytest.mark.parametrize("nx,ny", [(256, 256), (1024, 64)])
def test_vorticity_is_bit_equal_with_and_without_recording(nx, ny):
    """the vorticity after 6 steps is the same with recording on and off, each with and without use_graph"""
    import torch
    v, _, s, _ = _inputs(nx, ny)
    out = []
    for graph in (False, True):
        for depth in (0, 6):
            with torch.cuda.stream(torch.cuda.Stream()):
                m = _gpu_model(nx, ny, v, None, s)
                m.fop.use_current_stream()
                m.use_graph(graph)
                if depth:
                    m.record_adjoint(depth)
                m.step(6)
                assert m.adjoint_recorded() == depth
                out.append(_np(m.vort()))
                m.close()
    for o in out[1:]:
        assert _same32(out[0], o)
    assert rel_l2(out[0], v) > 1e-6


def test_two_equal_runs_give_the_same_bits():
    nx = ny = 256
    case = A.case_of(nx, ny)
    v, d, s, lam = _inputs(nx, ny)
    m = _gpu_model(nx, ny, v, None, s)
    m.record_adjoint(case.steps)
    m.step(case.steps)
    m.set_adjoint(lam)
    m.adjoint_back(case.steps)
    again = _np(m.adjoint())
    m.close()
    assert _same32(again, _gpu_run(nx, ny)[1])                 # (that run carried a tangent as well: lam_0 does not depend on it)


# ---- 4. tape discipline ----
def test_tape_discipline():
    import xlab_fftbarotropic_amd as X
    nx = ny = 256
    v, d, s, lam = _inputs(nx, ny)
    m = _gpu_model(nx, ny, v, None, s)
    with pytest.raises(X.FftBaroError, match="no adjoint is set"):
        m.adjoint()
    m.record_adjoint(5)
    m.step(3)
    m.set_adjoint(lam)
    with pytest.raises(X.FftBaroError, match="recorded"):
        m.adjoint_back(4)                                       # more than recorded
    before = _np(m.vort())
    with pytest.raises(X.FftBaroError, match="tape"):
        m.step(3)                                               # beyond depth: refused, state and tape unchanged
    assert m.adjoint_recorded() == 3
    assert _same32(_np(m.vort()), before)
    m.step(2)
    assert m.adjoint_recorded() == 5
    m.adjoint_back(3)
    assert m.adjoint_recorded() == 2
    m.adjoint_back(2)
    l32 = _np(m.adjoint())
    assert _same32(l32, _gpu_run(nx, ny)[1])                    # 3 then 2 == 5 at once, bitwise
    m.set_vort(v)
    m.step(2)
    assert m.adjoint_recorded() == 2
    m.set_vort(v)                                               # empties the tape
    assert m.adjoint_recorded() == 0
    with pytest.raises(X.FftBaroError, match="recorded"):
        m.adjoint_back(1)
    m.step(1)
    m.set_spectrum(m.spectrum())
    assert m.adjoint_recorded() == 0
    m.record_adjoint(0)
    m.step(7)                                                   # no tape, no limit
    m.set_adjoint(None)
    with pytest.raises(X.FftBaroError, match="no adjoint is set"):
        m.adjoint_back(0)
    m.close()


def test_recording_leaves_tracer_particles_and_tangent_bit_equal():
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    n, steps = 256, 4
    v0, d0, src, _ = _inputs(n, n)
    c0 = T.noisy_inputs(n, n, A.case_of(n, n).vort_noise)[1]
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, 64, seed=5)

    def run(depth):
        m = X.Model(n, n, nu=A.G.NU, dt=3.0)
        m.set_vort(v0)
        m.set_source(src)
        m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
        m.set_particles(x0)
        m.set_tangent(d0)
        if depth:
            m.record_adjoint(depth)
        m.step(steps)
        out = (_np(m.vort()), _np(m.tracer()), _np(m.particles()), _np(m.tangent()))
        m.close()
        return out
    a, b = run(0), run(steps)
    assert _same32(a[0], b[0]) and _same32(a[1], b[1]) and _same32(a[3], b[3])
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert rel_l2(a[3], d0) > 1e-4


# ---- 5. singular values ----
def test_singular_values_against_float64():
    """Model.singular_values at 256^2, 3 steps, 4 iterations from a fixed start vector against the same iteration in float64: every
    iterate's singular value to 1e-4 relative (the float32 restatement on the CPU holds SV_F32 = 2.4e-7, tests/test_adjoint_cpu.py).
    The final vector to 1e-4 as well: eight applications of T or T^T, each held to the parity bar of 1e-5, between start and end."""
    n = A.SV_N
    v, d, s, _ = _inputs(n, n)
    ref = A.recipe_model(n, n, v, d, s)
    s64, v64 = A.singular_values(ref, ref.spectrum(), A.SV_STEPS, A.SV_ITERS, d)
    m = _gpu_model(n, n, v, None, s)
    before = _np(m.vort())
    sg, vg = m.singular_values(A.SV_STEPS, A.SV_ITERS, d)
    assert m.adjoint_recorded() == 0
    assert _same32(_np(m.vort()), before)                       # the state is restored bit for bit
    m.close()
    err = [abs(a / b - 1) for a, b in zip(sg, s64)]
    print("singular_values 256^2, %d steps, %d iterations: GPU %s, float64 %s, off by %s; the vector by %.3g"
          % (A.SV_STEPS, A.SV_ITERS, sg, s64, ["%.2g" % e for e in err], rel_l2(_np(vg), v64)))
    assert len(sg) == A.SV_ITERS
    assert max(err) <= A.SV_BAR
    assert rel_l2(_np(vg), v64) <= 1e-4


# ---- 6. the slab ----
def test_slab_of_one_rank_matches_the_model():
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n = 256
    case = A.case_of(n, n)
    v, d, src, lam = _inputs(n, n)
    s = S.EngineSlab(n, n, nu=A.G.NU, dt=T.recipe_dt(n, n))
    s.set_vort_local(v)
    s.set_source_local(src)
    s.record_adjoint(case.steps)
    s.step(case.steps)
    assert s.adjoint_recorded() == case.steps
    with pytest.raises(X.FftBaroError, match="tape"):
        s.step(1)
    s.set_adjoint(lam)
    s.adjoint_back(case.steps)
    assert _same32(_np(s.adjoint()), _gpu_run(n, n)[1])
    s.set_adjoint(None)
    with pytest.raises(X.FftBaroError):
        s.adjoint()
    s.record_adjoint(0)
    s.close()


def test_slab_of_one_rank_singular_values_match_the_model():
    """EngineSlab.singular_values on one rank at 64^2 against Model.singular_values.  The slab keeps and puts back its state as a field
    of rows (one c2r and one r2c, each rounding to float32) where the model keeps the spectrum bit for bit, so the two iterations are
    not the same bits; the bars are the ones this file holds singular values and the final vector to, SV_BAR and 1e-4."""
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n = 64
    v, d, src, _ = A.adjoint_inputs(n, n, A.PATH_CASES[0].vort_noise)
    m = _gpu_model(n, n, v, None, src, dt=3.0)
    sm, vm = m.singular_values(A.SV_STEPS, A.SV_ITERS, d)
    m.close()
    s = S.EngineSlab(n, n, nu=A.G.NU, dt=3.0)
    s.set_vort_local(v)
    s.set_source_local(src)
    before = _np(s.vort_local())
    ss, vs = s.singular_values(A.SV_STEPS, A.SV_ITERS, d)
    assert s.adjoint_recorded() == 0
    assert rel_l2(_np(s.vort_local()), before) <= 1e-5          # (the parity bar: the state went through the field round trip)
    s.close()
    vs, vm = _np(vs), _np(vm)
    print("singular_values 64^2 on one rank: slab %s, model %s; the vector off by %.3g" % (ss, sm, rel_l2(vs, vm)))
    assert len(ss) == A.SV_ITERS and all(isinstance(x, float) and np.isfinite(x) for x in ss)
    assert vs.shape == (n, n) and vs.dtype == np.float32 and np.isfinite(vs).all()
    assert max(abs(a / b - 1) for a, b in zip(ss, sm)) <= A.SV_BAR
    assert rel_l2(vs, vm) <= 1e-4


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every adjoint entry point raises with the engine's message"""
    import threading
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n, world = 256, 2
    hub = S.local_hub(world)
    msgs, errs = [[] for _ in range(world)], [None] * world

    def work(r):
        try:
            s = S.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                calls = (lambda: s.record_adjoint(2), s.adjoint_recorded, lambda: s.set_adjoint(np.zeros((s.XL, n), np.float32)), lambda: s.set_adjoint(None),
                         s.adjoint, lambda: s.adjoint_back(1), lambda: s.singular_values(1, 1, np.zeros((s.XL, n), np.float32)))
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
        S.local_hub_destroy(hub)
    for e in errs:
        if e is not None:
            raise e
    for r in range(world):
        assert len(msgs[r]) == 7
        for msg in msgs[r]:
            assert msg is not None and "invalid argument" in msg.lower() and "not supported" in msg and "world > 1" in msg, msg
