"""The covariant Lyapunov vectors on the GPU (fb_model_tangent_tape, fb_model_tangent_tape_push, fb_model_tangent_tape_count,
fb_model_tangent_combine; kernel csrc/fb_clv.h, host side csrc/fb_beside_tangent.h): the combination bit for bit and against float64, the basis
tape, the covariance identity T V_n = V_(n+1) D through the engine's own tangent step, the float64 Ginelli run of tests/clv_numpy.py and
a fluid at rest.  Every bar is fixed by reasoning or by a CPU figure (tests/test_clv_cpu.py), none by what the GPU gave; one line of
figures per case (pytest -s); DESIGN.md, "Covariant Lyapunov vectors", has the tables."""
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

import clv_numpy as V                                           # noqa: E402
import entry_cases as E                                         # noqa: E402
import lyapunov_numpy as Y                                      # noqa: E402
import tangent_numpy as G                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

# the QR checks' layouts, and the counts: 3, 5 (no instance of k_tangent_combine has that bound) and the largest, 32
GRIDS = ((64, 64), (192, 192), (1024, 64), (64, 4096))
CASES = [(nx, ny, M) for nx, ny in GRIDS for M in (3, 5)] + [(64, 64, 32)]
CASE_IDS = ["%dx%d-M%d" % c for c in CASES]


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """the same bits, the sign of a zero apart (x + 0.0 makes every zero +0)"""
    a, b = np.ascontiguousarray(a) + 0.0, np.ascontiguousarray(b) + 0.0
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    out = Y.subspace_inputs(nx, ny)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _fields(nx, ny, M):
    """M perturbations: subspace_inputs' three in turn, scaled, each with white noise of twice its rms, so that the fields are far from
    dependent: a combination then has about the length of its terms, which the relative bar of test_combination_values presumes (it
    asserts so), as test_orthonormalisation's Q R does with an orthonormal Q"""
    W = _inputs(nx, ny)[1].astype(np.float64)
    rng = np.random.default_rng(100 + M)
    F = np.array([(1 + 0.1 * k) * W[k % 3] + 2.0 * np.sqrt(np.mean(W[k % 3] ** 2)) * rng.standard_normal((nx, ny)) for k in range(M)]).astype(np.float32)
    F.setflags(write=False)
    return F


def _gpu_model(nx, ny, vort, source=None, nu=G.NU, dt=None):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, nu=nu, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    return m


def _with_tape(nx, ny, M):
    """a model with M perturbations whose bases are slot 0 of a tape of one: (model, tangents() as pushed, vort())"""
    m = _gpu_model(nx, ny, _inputs(nx, ny)[0])
    m.set_tangents(_fields(nx, ny, M))
    m.tangent_tape(1)
    m.push_tangents()
    return m, _np(m.tangents()), _np(m.vort())


# ---- 1. the combination, bit level ----
@pytest.mark.parametrize("nx,ny,M", CASES, ids=CASE_IDS)
def test_combination_bit_level(nx, ny, M):
    """C = I returns the bits, a permutation permutes them, diag(2, -1, 0.5, ...) scales every bit pattern exactly, a column of zeros
    gives a field that is exactly zero; from a slot and in place; vort() keeps its bits"""
    m, q0, v0 = _with_tape(nx, ny, M)
    eye = np.eye(M)
    perm = np.roll(np.arange(M), 1)
    P = np.zeros((M, M))
    P[perm, np.arange(M)] = 1.0                                   # v_j = q_perm[j]
    d = np.array([(2.0, -1.0, 0.5, -4.0, 0.25)[k % 5] for k in range(M)])
    Z = np.eye(M)
    Z[:, 1] = 0.0
    for slot in (0, None):
        def combined(Cm):
            if slot is None:
                m.combine_tangents(eye, slot=0)                  # (the live set back to the pushed bases: the first assertion below)
            m.combine_tangents(Cm, slot=slot)
            return _np(m.tangents())
        assert _same(combined(eye), q0), slot
        assert _same(combined(P), q0[perm]), slot
        assert _same(combined(np.diag(d)), d.astype(np.float32)[:, None, None] * q0), slot
        z = combined(Z)
        assert not z[1].any() and _same(np.delete(z, 1, axis=0), np.delete(q0, 1, axis=0)), slot
    assert rel_l2(q0[1], q0[0]) > 1e-2                           # (the fields differ: a permutation is seen)
    assert m.tangent_tape_count() == (1, 1) and m.tangent_count() == M
    assert _same(_np(m.vort()), v0)
    m.close()


# ---- 2. the combination, values ----
@pytest.mark.parametrize("nx,ny,M", CASES, ids=CASE_IDS)
def test_combination_values(nx, ny, M):
    """a random dense C and a random upper triangular C with unit columns, in place and from a slot, against the float64 combination
    of the fields that tangents() returned before: rel L2 per field <= 1e-6, the bar test_orthonormalisation holds Q R to"""
    m, q0, v0 = _with_tape(nx, ny, M)
    rng = np.random.default_rng(7 * M + nx)
    dense = rng.standard_normal((M, M))
    tri = np.triu(rng.standard_normal((M, M)))
    tri[np.diag_indices(M)] += np.where(np.diagonal(tri) < 0, -1.0, 1.0)
    tri /= np.linalg.norm(tri, axis=0)
    q64 = q0.astype(np.float64)
    worst, kept = {}, 1.0
    for name, Cm in (("dense", dense), ("triangular", tri)):
        want = np.einsum("ij,ixy->jxy", Cm, q64)
        terms = np.sqrt(np.einsum("ij,i->j", Cm ** 2, (q64 ** 2).sum(axis=(1, 2))))
        kept = min(kept, float((np.sqrt((want ** 2).sum(axis=(1, 2))) / terms).min()))     # |v_j| over the root sum of squares of its terms
        for slot in (0, None):
            if slot is None:
                m.combine_tangents(np.eye(M), slot=0)
            m.combine_tangents(m.torch.from_numpy(Cm) if slot is None else Cm, slot=slot)     # (a torch tensor is taken too)
            got = _np(m.tangents())
            worst[name, slot] = max(rel_l2(got[j], want[j]) for j in range(M))
    print("combine_tangents %dx%d, M = %d: largest rel L2 per field against float64: %s; smallest |v_j| / rss of its terms = %.3g"
          % (nx, ny, M, {k: "%.3g" % e for k, e in worst.items()}, kept))
    assert kept >= 0.5                                           # (no cancellation: the relative bar is about the kernel)
    assert max(worst.values()) <= 1e-6
    assert rel_l2(np.einsum("ij,ixy->jxy", dense, q64)[0], q64[0]) > 1e-2
    assert _same(_np(m.vort()), v0)
    with pytest.raises(ValueError):
        m.combine_tangents(np.eye(M + 1))
    m.close()


# ---- 3. the tape ----
def test_tape_keeps_the_pushed_bits_in_order():
    n = 64
    v0, W, src = _inputs(n, n)
    m = _gpu_model(n, n, v0, src)
    m.set_tangents(W)
    assert m.tangent_tape_count() == (0, 0)
    m.tangent_tape(3)
    assert m.tangent_tape_count() == (0, 3)
    pushed = []
    for k in range(3):
        pushed.append(_np(m.tangents()))
        m.push_tangents()
        m.step(2)
    assert m.tangent_tape_count() == (3, 3)
    live = _np(m.tangents())
    assert all(rel_l2(pushed[k + 1][0], pushed[k][0]) > 1e-4 for k in range(2)) and rel_l2(live[0], pushed[2][0]) > 1e-4
    for slot in (2, 0, 1):
        m.combine_tangents(np.eye(3), slot=slot)
        assert _same(_np(m.tangents()), pushed[slot]), slot
    m.tangent_tape(2)                                            # a new tape starts empty
    assert m.tangent_tape_count() == (0, 2)
    m.tangent_tape(0)
    assert m.tangent_tape_count() == (0, 0)
    m.close()


def test_refusals_change_nothing():
    import xlab_fftbarotropic_amd as X
    n = 64
    v0, W, _ = _inputs(n, n)
    m = _gpu_model(n, n, v0)
    eye = m.torch.eye(3, dtype=m.torch.float64, device="cuda")
    for call, name in ((lambda: m.combine_tangents(np.eye(1)), "tangent_combine"), (lambda: m._call("tangent_combine", -1, eye.data_ptr()), "tangent_combine"),
                       (m.push_tangents, "tangent_tape_push"), (lambda: m.tangent_tape(2), "tangent_tape")):
        with pytest.raises(X.FftBaroError, match="fb_model_%s: no tangent is set" % name):
            call()
    m.tangent_tape(0)                                            # (freeing needs no set)
    assert m.tangent_tape_count() == (0, 0)
    m.set_tangents(W)
    with pytest.raises(X.FftBaroError, match="fb_model_tangent_tape_push: no basis tape"):
        m.push_tangents()
    m.tangent_tape(2)
    m.push_tangents()
    before = _np(m.tangents())
    for slot in (1, 2, -2):
        with pytest.raises(X.FftBaroError, match="invalid argument: fb_model_tangent_combine: slot"):
            m.combine_tangents(np.eye(3), slot=slot)
    with pytest.raises(X.FftBaroError, match="invalid argument: fb_model_tangent_combine: NULL coefficients"):
        m._call("tangent_combine", 0, None)
    m.push_tangents()
    with pytest.raises(X.FftBaroError, match="invalid argument: fb_model_tangent_tape_push: the basis tape is full"):
        m.push_tangents()
    with pytest.raises(X.FftBaroError, match="invalid argument: fb_model_tangent_tape: depth"):
        m.tangent_tape(-1)
    assert m.tangent_tape_count() == (2, 2) and m.tangent_count() == 3
    assert _same(_np(m.tangents()), before)
    m.combine_tangents(np.eye(3), slot=1)
    assert _same(_np(m.tangents()), before)
    m.close()


def test_the_tape_goes_with_the_set_and_stays_with_the_state():
    n = 64
    v0, W, _ = _inputs(n, n)
    m = _gpu_model(n, n, v0)
    m.set_tangents(W)
    m.tangent_tape(2)
    m.push_tangents()
    pushed = _np(m.tangents())
    z = m.spectrum()
    m.step(2)
    m.set_spectrum(z)                                            # the state put back while the tape holds a slot
    m.set_vort(v0)
    assert m.tangent_tape_count() == (1, 2)
    m.set_tangents(W[::-1].copy())                               # the same count: the tape stays
    assert m.tangent_tape_count() == (1, 2)
    m.combine_tangents(np.eye(3), slot=0)
    assert _same(_np(m.tangents()), pushed)
    m.set_tangents(W[:2])                                        # another count
    assert m.tangent_tape_count() == (0, 0) and m.tangent_count() == 2
    m.tangent_tape(1)
    m.set_tangents(None)
    assert m.tangent_tape_count() == (0, 0)
    m.step(1)                                                    # stepping goes on
    assert np.isfinite(_np(m.vort())).all()
    m.close()


def test_info_counts_the_tape():
    n = 64
    v0, W, _ = _inputs(n, n)
    m = _gpu_model(n, n, v0)

    def grown(M, depth):
        m.set_tangents(W[:M])
        h0 = m.info()["hbm_bytes"]
        m.tangent_tape(depth)
        h1 = m.info()["hbm_bytes"]
        m.tangent_tape(0)
        assert m.info()["hbm_bytes"] == h0
        return h1 - h0
    base = grown(1, 1)                                           # one base: [nx][the padded columns] complex64, every column group
    hy = n // 2 + 1
    assert 8 * n * hy <= base <= 8 * n * (hy + 31) and base % (8 * 16) == 0
    assert grown(3, 4) == 4 * 3 * base and grown(2, 5) == 5 * 2 * base and grown(3, 1) == 3 * base
    m.close()


def test_captured_step_gives_the_same_bits_with_and_without_pushes():
    import torch
    n = 256
    v0, W, src = _inputs(n, n)
    out = []
    for graph, push in ((True, True), (True, False), (False, True)):
        with torch.cuda.stream(torch.cuda.Stream()):
            m = _gpu_model(n, n, v0, src)
            m.fop.use_current_stream()
            m.use_graph(graph)
            m.set_tangents(W)
            m.tangent_tape(2)
            m.step(3)
            m.step(3)                                           # captured and replayed
            slots = []
            for _ in range(2):
                if push:
                    slots.append(_np(m.tangents()))
                    m.push_tangents()                           # between replays, on the model's stream
                m.step(3)
            live = (_np(m.tangents()), _np(m.vort()))
            if push:
                for k in (1, 0):
                    m.combine_tangents(np.eye(3), slot=k)
                    assert _same(_np(m.tangents()), slots[k])
            out.append(live)
            m.close()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert _same(a, b)


def test_tracer_particles_and_the_adjoint_do_not_see_the_tape():
    import particles_numpy as P
    n, steps = 256, 4
    v0, W, src = _inputs(n, n)
    c0 = T.noisy_inputs(n, n, Y.NOISE)[1]
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, 64, seed=5)
    Cm = np.random.default_rng(3).standard_normal((3, 3))

    def run(clv):
        m = _gpu_model(n, n, v0, src, dt=3.0)
        m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
        m.set_particles(x0)
        m.record_adjoint(steps)
        m.set_tangents(W)
        if clv:
            m.tangent_tape(2)
            m.push_tangents()
        m.step(steps // 2)
        if clv:
            m.push_tangents()
            m.combine_tangents(Cm)
            m.combine_tangents(np.eye(3), slot=0)
        m.step(steps - steps // 2)
        m.set_adjoint(v0)
        m.adjoint_back(steps)
        out = (_np(m.vort()), _np(m.tracer()), _np(m.particles()), _np(m.adjoint()), m.adjoint_recorded())
        m.close()
        return out
    for a, b in zip(run(True), run(False)):
        assert _same(np.asarray(a), np.asarray(b))


def test_slab_of_one_rank_matches_the_model():
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n = 64
    v0, W, _ = _inputs(n, n)
    Cm = np.triu(np.random.default_rng(5).standard_normal((3, 3))) + np.eye(3)
    out = []
    for m in (X.Model(n, n, nu=G.NU, dt=3.0), S.EngineSlab(n, n, nu=G.NU, dt=3.0)):
        (m.set_vort if isinstance(m, X.Model) else m.set_vort_local)(v0)
        m.set_tangents(W)
        m.orthonormalize_tangents()
        m.tangent_tape(2)
        m.push_tangents()
        m.step(2)
        R = m.orthonormalize_tangents()
        m.push_tangents()
        m.combine_tangents(Cm, slot=0)
        a = _np(m.tangents())
        m.combine_tangents(Cm)
        out.append((a, _np(m.tangents()), R, np.array(m.tangent_tape_count())))
        m.close()
    for a, b in zip(*out):
        assert _same(a.astype(np.float64) if a.dtype.kind == "i" else a, b.astype(np.float64) if b.dtype.kind == "i" else b)
    assert tuple(out[0][3]) == (2, 2) and rel_l2(out[0][0][1], out[0][1][1]) > 1e-3


def test_slab_of_two_ranks_refuses_all_four():
    """an unconnected slab, rank 0 of world 2 (tests/entry_cases.py): the tangent's refusal of several ranks, under each function's own name"""
    h = E.Handles()
    try:
        calls = [("fb_slab_tangent_tape", ["S", 1]), ("fb_slab_tangent_tape", ["S", 0]), ("fb_slab_tangent_tape_push", ["S"]),
                 ("fb_slab_tangent_tape_count", ["S", "host", "host"]), ("fb_slab_tangent_combine", ["S", -1, "buf"])]
        for fn, args in calls:
            rc, msg = h.call(fn, args)
            assert rc == 1 and msg.startswith(fn + ": ") and "several ranks" in msg, (fn, rc, msg)
        for fn, args in (("fb_model_tangent_tape", ["M", 1]), ("fb_model_tangent_tape_push", ["M"]), ("fb_model_tangent_combine", ["M", -1, "buf"])):
            rc, msg = h.call(fn, args)
            assert rc == 1 and msg.startswith(fn + ": ") and "no tangent is set" in msg, (fn, rc, msg)
    finally:
        h.close()


# ---- 4. the covariance identity on the engine, and the float64 Ginelli run ----
@functools.lru_cache(maxsize=None)
def _reference(kind):
    return V.ginelli(kind, C_end=V.c_end(3))


def _unit_spectra(ref, fields):
    return [np.fft.rfft2(f.astype(np.float64)) for f in fields]


@functools.lru_cache(maxsize=None)
def _engine_run(kind):
    """clv() on the recipe of tests/clv_numpy.py, spectrum() kept at every slot; then, for every window slot n, the state put back,
    V_n carried over one interval by the engine's own step and compared with V_(n+1).  Returns the figures of both tests below."""
    n, K = V.N, V.WINDOW
    v0, W, src = _inputs(n, n)
    ref = _reference(kind)
    m = _gpu_model(n, n, v0, src)
    m.set_tangents(W)
    states, push = [], m.push_tangents

    def push_and_keep():
        states.append(m.spectrum().clone())
        push()
    m.push_tangents = push_and_keep
    res = m.clv(K * V.EVERY, V.EVERY, V.SETTLE, kind, C_end=V.c_end(3))
    assert m.tangent_tape_count() == (K + 1, K + 1) and len(states) == K + 1
    vec = [_np(m.clv_vectors(res, k)) for k in range(K + 1)]
    sines, growth = np.zeros((K, 3)), np.zeros((K, 3))
    for k in range(K):
        m.set_spectrum(states[k])
        m.clv_vectors(res, k)
        before = np.diagonal(_np(m.tangent_gram(kind)))
        m.step(V.EVERY)
        after = np.diagonal(_np(m.tangent_gram(kind)))
        out = _unit_spectra(ref, _np(m.tangents()))
        want = _unit_spectra(ref, vec[k + 1])
        sines[k] = [V.sine(ref.m, out[j], want[j], kind) for j in range(3)]
        growth[k] = 0.5 * np.log(after / before) - res.log_growth[k]
    m.close()
    against = max(V.sine(ref.m, a, b, kind) for k in range(K + 1) for a, b in zip(_unit_spectra(ref, vec[k]), V.vectors(ref, k)))
    return dict(res=res, sines=sines, growth=growth, against=against, d_log_r=float(np.abs(res.log_r - ref.log_r).max()),
                d_log_growth=float(np.abs(res.log_growth - ref.log_growth).max()))


@pytest.mark.parametrize("kind", Y.KINDS)
def test_covariance_on_the_engine(kind):
    """T V_n against V_(n+1), both through the engine's own tangent step, so that only rounding separates them: for every window slot
    and column the sine <= 1e-5 and the ln growth within 1e-5 of log_growth (the bar the engine's dz is held to against float64; the
    smallest wrong-C probe of tests/test_clv_cpu.py moves a column by 1e-3 and more)"""
    f = _engine_run(kind)
    res = f["res"]
    print("covariance on the engine, %s, 64^2, M = 3: sines per slot and column =\n%s\nln growth - log_growth =\n%s\nlargest sine %.3g, largest growth difference %.3g"
          % (kind, np.array2string(f["sines"], precision=3), np.array2string(f["growth"], precision=3), f["sines"].max(), np.abs(f["growth"]).max()))
    assert res.C.shape == (V.WINDOW + 1, 3, 3) and res.log_growth.shape == (V.WINDOW, 3) and res.log_r.shape == (V.WINDOW + V.SETTLE, 3)
    assert np.abs(res.cosines - np.einsum("nki,nkj->nij", res.C, res.C)).max() == 0.0 and np.abs(np.diagonal(res.cosines, axis1=1, axis2=2) - 1).max() <= 1e-14
    assert max(np.linalg.cond(c) for c in res.C) <= 10.0
    assert f["sines"].max() <= 1e-5
    assert np.abs(f["growth"]).max() <= 1e-5


@pytest.mark.parametrize("kind", Y.KINDS)
def test_against_the_float64_ginelli_run(kind):
    """the same recipe and C_end on the engine and in float64: |log_r - log_r64|, |log_growth - log_growth64| and the sine between
    the engine's vectors and the reference's at every window slot, each within 4 times what float32 storage alone costs on the CPU
    (clv_numpy.F32_*; the factor covers the GPU's other summation order, as for MGS_F32_DEFECT)"""
    f = _engine_run(kind)
    print("engine against the float64 Ginelli run, %s: max |log_r - log_r64| = %.3g (bar %.3g), max |log_growth - log_growth64| = %.3g (bar %.3g), "
          "largest sine = %.3g (bar %.3g)" % (kind, f["d_log_r"], 4 * V.F32_LOG_R, f["d_log_growth"], 4 * V.F32_LOG_GROWTH, f["against"], 4 * V.F32_SINE))
    assert f["d_log_r"] <= 4 * V.F32_LOG_R
    assert f["d_log_growth"] <= 4 * V.F32_LOG_GROWTH
    assert f["against"] <= 4 * V.F32_SINE


# ---- 5. a fluid at rest ----
@pytest.mark.parametrize("kind", Y.KINDS)
def test_fluid_at_rest(kind):
    """The CPU test's three modes at 256^2, the set A, A + B, A + B + C: R_n is diagonal up to the engine's orthonormality, so with
    C_end = I every |C_n[i, j]|, i != j, is at most 1e-6 / (1 - max_j r_(j+1)(j+1) / r_jj), the project's orthonormality bar carried
    through the geometric sum of the recursion (the ratio from the R the run gave); and vector j is the pure mode j to 1e-5.
    C_end is the identity and the run is short (2 + 4 intervals) because the engine's fields are float32: what r2c's rounding leaves in
    the modes outside the dealiasing circle never decays, the vectors do and are rescaled at every interval, so that noise grows in
    the fastest vector by e^1.58 per interval, and over the 40 intervals that a random C_end needs to be forgotten it would outgrow the
    vectors themselves (tests/clv_numpy.py, rest_spectra)."""
    n, K, settle = 256, 2, 4
    modes = V.rest_fields(n)
    m = _gpu_model(n, n, np.zeros((n, n), np.float32), nu=V.REST_NU, dt=V.REST_DT)
    m.set_tangents((1.0e-6 * np.array([modes[0], modes[0] + modes[1], modes[0] + modes[1] + modes[2]])).astype(np.float32))
    res = m.clv(K * V.REST_EVERY, V.REST_EVERY, settle, kind, C_end=np.eye(3))
    vec = [_np(m.clv_vectors(res, k)).astype(np.float64) for k in range(K + 1)]
    m.close()
    ratio = float(np.exp(np.diff(res.log_r, axis=1).max()))
    bar = 1e-6 / (1 - ratio)
    off = max(float(np.abs(c - np.diag(np.diagonal(c))).max()) for c in res.C)
    want = V.REST_EVERY * np.log(T.rk4_factor(V.rest_z()))
    err = 0.0
    for k in range(K + 1):
        for j in range(3):
            a = (vec[k][j] * modes[j]).sum() / (modes[j] ** 2).sum()
            err = max(err, rel_l2(vec[k][j], a * modes[j]))
    print("fluid at rest on the engine, %s, 256^2: ln r_ii per interval = %s (analytic %s); largest ratio r_(j+1)(j+1) / r_jj = %.3g; largest off-diagonal "
          "|C_ij| = %.3g (bar %.3g); vector j against the pure mode j, rel L2 = %.3g" % (kind, res.log_r[0], want, ratio, off, bar, err))
    assert ratio < 1.0 and np.abs(res.log_r[:K] - want).max() <= 1e-3
    assert off <= bar
    assert err <= 1e-5
