"""The tangent replay over the adjoint's tape and Gauss-Newton 4D-Var on the GPU (fb_model_tangent_replay, fb_model_adjoint_rewind,
fb_model_observe_tangent; kernels csrc/fb_replay.h; Model.gauss_newton_hvp, Model.fit_incremental, singular_vectors(replay=True))
against the float64 reference (tests/replay_numpy.py) on the adjoint's path cases, 5 steps each.

The bars that are not fixed numbers are 4 x the float32 restatement's figure on the CPU (replay_numpy.HVP_SYM_F32,
SV_REPLAY_ANGLE_F32, adjoint_numpy.DOT_BAR; tests/test_replay_cpu.py has them), set before the GPU ran.  One line of figures per case
(pytest -s); DESIGN.md, "Tangent replay and Gauss-Newton 4D-Var", has the tables."""
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
import obs_numpy as O                                           # noqa: E402
import particles_numpy as P                                     # noqa: E402
import replay_numpy as R                                        # noqa: E402
import singular_numpy as S                                      # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

GRIDS = [(k.nx, k.ny) for k in A.PATH_CASES]
GRID_IDS = ["%dx%d" % g for g in GRIDS]
TWO = [(256, 256), (1024, 64)]
STEPS = A.STEPS
FB_EINVAL = 1


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    out = A.adjoint_inputs(nx, ny, 3e-2)
    for a in out:
        a.setflags(write=False)
    return out


def _model(nx, ny, vort=None, source=None, dt=None, nu=A.G.NU, cls=None):
    import xlab_fftbarotropic_amd as X
    m = (cls or X.Model)(nx, ny, nu=nu, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    if vort is not None:
        m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    return m


def _recorded(nx, ny, cls=None):
    """a model of the path case that has recorded STEPS steps with no tangent set"""
    v, _, src, _ = _inputs(nx, ny)
    m = _model(nx, ny, v, src, cls=cls)
    m.record_adjoint(STEPS)
    m.step(STEPS)
    return m


def _fields(nx, ny, count):
    """`count` perturbations, float32 [count, nx, ny]: the case's dz, white noise of its rms, dz shifted, ..., never dealiased"""
    dz = _inputs(nx, ny)[1]
    out = [dz, R.white_like(dz)] + [np.roll(dz, 3 * k, axis=k % 2) + 0.5 * R.white_like(dz, seed=O.SEED + 41 + k) for k in range(2, count)]
    return np.ascontiguousarray(np.stack(out[:count]), dtype=np.float32)


def _replayed(m, f, pieces=((0, STEPS),)):
    """the field f set as the single tangent and replayed over m's tape"""
    m.set_tangent(f)
    for first, n in pieces:
        m.tangent_replay(first, n)
    return _np(m.tangent())


@functools.lru_cache(maxsize=None)
def _tangent64(nx, ny):
    v, dz, src, _ = _inputs(nx, ny)
    m = A.recipe_model(nx, ny, v, dz, src, cls=A.G.TangentModel64)
    m.step(STEPS)
    return m.tangent()


# ---- 1. the replay against float64 and against the live tangent; 4. the transpose ----
@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_replay_against_float64_the_live_tangent_and_the_sweep(nx, ny):
    """STEPS steps recorded with no tangent set, then set_tangent(dz) and tangent_replay(0, STEPS): within 1e-5 relative L2 of
    TangentModel64 (the live tangent's bar) and within 2e-5 of the engine's live tangent (the triangle of the two bars; not its bits);
    <T d, lam> against <d, T^T lam>, T by replay and T^T by adjoint_back over the same tape, to adjoint_numpy.DOT_BAR"""
    v, dz, src, lam = _inputs(nx, ny)
    m = _recorded(nx, ny)
    td = _replayed(m, dz)
    m.set_adjoint(lam)
    m.adjoint_back(STEPS)
    tl = _np(m.adjoint())
    m.close()
    live = _model(nx, ny, v, src)
    live.set_tangent(dz)
    live.step(STEPS)
    tlive = _np(live.tangent())
    live.close()
    e64, elive, res = rel_l2(td, _tangent64(nx, ny)), rel_l2(td, tlive), A.dot_residual(td, lam, dz, tl)
    print("replay %dx%d: against float64 %.3g (the live tangent: %.3g), against the live tangent %.3g; <T d, lam> - <d, T^T lam>: %.3g (bar %.3g)"
          % (nx, ny, e64, rel_l2(tlive, _tangent64(nx, ny)), elive, res, A.DOT_BAR))
    assert rel_l2(td, dz) > 1e-3
    assert e64 <= 1e-5
    assert elive <= 2e-5
    assert res <= A.DOT_BAR


def test_transpose_of_a_replayed_set_against_an_adjoint_set():
    """256^2: all nine residuals of a replayed set of 3 against an adjoint set of 3 swept over the same tape"""
    nx = ny = 256
    m = _recorded(nx, ny)
    d = _fields(nx, ny, 3)
    lam = np.ascontiguousarray(np.stack([_inputs(nx, ny)[3], R.white_like(_inputs(nx, ny)[3], seed=O.SEED + 70), np.roll(_inputs(nx, ny)[3], 5, axis=0)]))
    m.set_tangents(d)
    m.tangent_replay(0, STEPS)
    td = _np(m.tangents())
    m.set_adjoints(lam)
    m.adjoint_back(STEPS)
    tl = _np(m.adjoints())
    m.close()
    res = np.array([[A.dot_residual(td[i], lam[j], d[i], tl[j]) for j in range(3)] for i in range(3)])
    print("replayed set against adjoint set at 256^2: residuals\n%s\nbar %.3g" % (res, A.DOT_BAR))
    assert res.max() <= A.DOT_BAR


# ---- 2. nothing else moves ----
@pytest.mark.parametrize("nx,ny", TWO)
def test_replay_moves_nothing_but_the_tangent(nx, ny):
    """the vorticity, a tracer, the particles, adjoint_recorded() and the step count (the deformation's elapsed time) are the same bits
    before and after a replay; three further steps after freeing the tape equal a run that never replayed, with and without use_graph"""
    import torch
    v, dz, src, _ = _inputs(nx, ny)
    c0 = T.noisy_inputs(nx, ny, 3e-2)[1]
    x0 = P.seed_positions(nx, ny, O.LX, O.LY, 64, seed=5)
    out = {}
    for graph in (False, True):
        for replay in (False, True):
            with torch.cuda.stream(torch.cuda.Stream()):
                m = _model(nx, ny, v, src)
                m.fop.use_current_stream()
                m.use_graph(graph)
                m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
                m.set_particles(x0)
                m.set_particle_deformation(True)
                m.record_adjoint(STEPS)
                m.step(STEPS)
                if replay:
                    def state():
                        return (_np(m.vort()), _np(m.tracer()), _np(m.particles()), m.adjoint_recorded(), m.particle_deformation_time())
                    before = state()
                    m.set_tangent(dz)
                    m.tangent_replay(0, STEPS)
                    moved = _np(m.tangent())
                    after = state()
                    assert _same32(before[0], after[0]) and _same32(before[1], after[1]) and _same64(before[2], after[2])
                    assert before[3:] == after[3:] and before[3] == STEPS and before[4] > 0.0
                    assert rel_l2(moved, dz) > 1e-3
                    m.set_tangent(None)
                m.record_adjoint(0)
                m.step(3)
                out[(graph, replay)] = (_np(m.vort()), _np(m.tracer()), _np(m.particles()))
                m.close()
    ref = out[(False, False)]
    for o in out.values():
        assert _same32(o[0], ref[0]) and _same32(o[1], ref[1]) and _same64(o[2], ref[2])


# ---- 3. sets ----
@pytest.mark.parametrize("nx,ny", GRIDS, ids=GRID_IDS)
def test_perturbation_k_of_a_replayed_set_has_the_bits_of_the_replayed_single(nx, ny):
    """M = 3: every perturbation bit-equal to the single replayed from the same field; 3 then 2 steps equal 5; two runs give equal bits"""
    m = _recorded(nx, ny)
    f = _fields(nx, ny, 3)
    single = [_replayed(m, f[k]) for k in range(3)]
    assert _same32(_replayed(m, f[1], ((0, 3), (3, 2))), single[1])
    for pieces in (((0, STEPS),), ((0, 3), (3, 2))):
        m.set_tangents(f)
        for first, n in pieces:
            m.tangent_replay(first, n)
        got = _np(m.tangents())
        for k in range(3):
            assert _same32(got[k], single[k]), (pieces, k)
    assert m.adjoint_recorded() == STEPS
    m.close()
    assert not _same32(single[0], single[1]) and rel_l2(single[1], f[1]) > 1e-3


@pytest.mark.parametrize("count,which", [(9, (0, 7, 8)), (32, (0, 17, 31))])
def test_sets_of_several_chunks(count, which):
    """64^2: M = 9 is two chunks, 8 + 1, M = 32 four whole ones; the perturbations `which` bit-equal to their replayed singles"""
    nx = ny = 64
    m = _recorded(nx, ny)
    f = _fields(nx, ny, count)
    m.set_tangents(f)
    m.tangent_replay(0, STEPS)
    got = _np(m.tangents())
    for k in which:
        assert _same32(got[k], _replayed(m, f[k])), k
    m.close()


# ---- 5. the rewind ----
def test_rewind():
    """sweep 5, adjoint_rewind(-1), the same lam, sweep 5 again: the same bits of lam_0; rewinding more than was popped, and onto a slot
    that a new step has overwritten, is refused; so is any rewind under checkpoint_adjoint and while a particle adjoint is set"""
    import xlab_fftbarotropic_amd as X
    nx = ny = 256
    lam = _inputs(nx, ny)[3]
    m = _recorded(nx, ny)
    m.set_adjoint(lam)
    m.adjoint_back(STEPS)
    first = _np(m.adjoint())
    assert m.adjoint_recorded() == 0
    m.adjoint_rewind()
    assert m.adjoint_recorded() == STEPS
    m.set_adjoint(lam)
    m.adjoint_back(2)
    m.adjoint_back(3)
    assert _same32(_np(m.adjoint()), first) and rel_l2(first, lam) > 1e-3
    m.adjoint_rewind(2)
    assert m.adjoint_recorded() == 2
    with pytest.raises(X.FftBaroError, match="fb_model_adjoint_rewind: 4 steps asked for, 3 popped"):
        m.adjoint_rewind(4)
    m.adjoint_rewind(3)
    m.adjoint_back(2)                                           # 3 left; one new step goes into slot 3 and slot 4 is gone
    m.step(1)
    assert m.adjoint_recorded() == 4
    with pytest.raises(X.FftBaroError, match="fb_model_adjoint_rewind: 1 steps asked for, 0 popped"):
        m.adjoint_rewind(1)
    m.adjoint_rewind(-1)                                        # nothing to un-pop: not a refusal
    with pytest.raises(X.FftBaroError, match="fb_model_tangent_replay: no tangent is set"):
        m.tangent_replay(0, 4)
    m.set_tangent(_inputs(nx, ny)[1])
    m.tangent_replay(0, 4)
    with pytest.raises(X.FftBaroError, match="fb_model_tangent_replay: steps 0 .. 5 asked for, 4 on the tape"):
        m.tangent_replay(0, 5)
    m.set_particles(P.seed_positions(nx, ny, O.LX, O.LY, 16, seed=5))
    m.set_particle_adjoint(np.zeros((16, 2)))
    with pytest.raises(X.FftBaroError, match="fb_model_adjoint_rewind: a particle adjoint is set"):
        m.adjoint_rewind(0)
    m.set_particle_adjoint(None)
    m.checkpoint_adjoint(2, 6)
    with pytest.raises(X.FftBaroError, match="fb_model_adjoint_rewind: not under adjoint checkpointing"):
        m.adjoint_rewind(-1)
    with pytest.raises(X.FftBaroError, match="fb_model_tangent_replay: not under adjoint checkpointing"):
        m.tangent_replay(0, 0)
    m.close()


# ---- 6. observe_tangent ----
@pytest.mark.parametrize("nx,ny", TWO)
def test_observe_tangent(nx, ny):
    """the four kinds of the single tangent, and of perturbation 2 of a set of 3, after a replay: within 1e-5 of max |h| of the float64
    H applied to the same field (observe's bar); kind "vort" bit for bit sample(the tangent field, xy)"""
    xy = O.positions(nx, ny)
    m = _recorded(nx, ny)
    ref = R.gradient_model(nx, ny)
    f = _fields(nx, ny, 3)
    for count, k in ((1, 0), (3, 2)):
        m.set_tangents(f[:count])
        m.tangent_replay(0, 2)
        field = m.tangents()[k]
        spec = np.fft.rfft2(_np(field).astype(np.float64))
        for kind in O.KINDS:
            h = _np(m.observe_tangent(kind, xy, k))
            want = O.sample64(ref.field(kind, spec), xy)
            err = np.abs(h - want).max() / np.abs(want).max()
            print("observe_tangent %dx%d, perturbation %d of %d, %s: max error %.3g of max |h|" % (nx, ny, k, count, kind, err))
            assert err <= 1e-5
            if kind == "vort":
                assert _same64(h, _np(m.sample(field, xy)))
    m.close()


# ---- 7. the Hessian-vector product ----
@functools.lru_cache(maxsize=None)
def _hvp_reference(nx, ny, background=False):
    ref = R.gradient_model(nx, ny)
    v, src, sets, d = O.gradient_case(nx, ny, ref)
    w = R.white_like(d)
    ref = R.gradient_model(nx, ny)
    ref.src = src.astype(np.float64)
    bg = ((0.9 * v).astype(np.float32), R.HVP_SIGMA_B) if background else None
    R.fourdvar_keep(ref, v, sets, bg)
    return v, src, sets, d, w, bg, R.gauss_newton_hvp(ref, d, sets, bg), R.gauss_newton_hvp(ref, w, sets, bg)


def _observations(sets):
    import xlab_fftbarotropic_amd as X
    return [X.Observations(s.step, s.kind, s.xy, s.y, s.sigma) for s in sets]


def _check_hvp(nx, ny, background, cls=None):
    v, src, sets, d, w, bg, h64d, h64w = _hvp_reference(nx, ny, background)
    obs = _observations(sets)
    m = _model(nx, ny, None, src, cls=cls)
    J0, g0 = m.fourdvar(v, obs, bg)
    assert m.adjoint_recorded() == 0
    J, g = m.fourdvar(v, obs, bg, keep_tape=True)
    assert J == J0 and _same64(_np(g), _np(g0)) and m.adjoint_recorded() == O.GRAD_STEPS
    vort = _np(m.vort())
    hd, hw = _np(m.gauss_newton_hvp(d, obs, bg)), _np(m.gauss_newton_hvp(w, obs, bg))
    assert hd.dtype == np.float64 and hd.shape == (nx, ny)
    assert _same64(_np(m.gauss_newton_hvp(d, obs, bg)), hd)
    assert m.adjoint_recorded() == O.GRAD_STEPS and m.tangent_count() == 0 and _same32(_np(m.vort()), vort)
    m.close()
    err, sym = max(rel_l2(hd, h64d), rel_l2(hw, h64w)), R.symmetry_residual(hd, hw, d, w)
    print("H_GN v %dx%d%s: against float64 %.3g (float32 on the CPU %.3g, bar %.3g); symmetry residual %.3g (float32 on the CPU %.3g, bar %.3g)"
          % (nx, ny, " with a background term" if background else "", err, R.HVP_F32[(nx, ny)], R.HVP_BAR, sym, R.HVP_SYM_F32[(nx, ny)], R.HVP_SYM_BAR))
    assert err <= R.HVP_BAR
    assert sym <= R.HVP_SYM_BAR
    return hd


@pytest.mark.parametrize("nx,ny", TWO)
def test_hessian_vector_product_against_float64(nx, ny):
    """the gradient case with its source: H_GN d and H_GN w within 1e-5 relative L2 of float64; the symmetry residual at most 4 x the
    float32 restatement's recorded figure; two equal calls give the same bits; fourdvar(keep_tape=True) returns the bits of fourdvar()
    and leaves the tape; the product leaves the tape whole, no tangent set and the vorticity where it was"""
    _check_hvp(nx, ny, False)


def test_hessian_vector_product_with_a_background_term():
    hb = _check_hvp(256, 256, True)
    assert rel_l2(hb, _hvp_reference(256, 256)[6]) > 0.1        # the term is of the data term's size


def test_hessian_vector_product_needs_the_tape():
    import xlab_fftbarotropic_amd as X
    v, src, sets, d = _hvp_reference(256, 256)[:4]
    m = _model(256, 256, v, src)
    with pytest.raises(ValueError, match="keep_tape=True"):
        m.gauss_newton_hvp(d, _observations(sets))
    with pytest.raises(ValueError, match="keep_tape"):
        m.fourdvar(v, _observations(sets), keep_tape=True, checkpoint_every=2)
    with pytest.raises(ValueError, match="position"):
        m.gauss_newton_hvp(d, [X.Observations(2, X.POSITION, None, np.zeros((4, 2)))])
    m.close()


# ---- 8. the twin experiment ----
def test_twin_experiment_by_gauss_newton():
    """obs_numpy.twin_case: fit_incremental(outer=3, inner=8) on the GPU reaches J_K / J_0 <= 10 x the float64 reference's
    GN_TWIN_RATIO (the factor of the L-BFGS twin: a float32 gradient may send the search down another path), J falls at every outer
    iteration, z0 ends closer to the truth, and the tape is freed"""
    import xlab_fftbarotropic_amd as X
    truth, guess, sets, _ = O.twin_case(X.make_field)
    m = _model(O.TWIN_N, O.TWIN_N, dt=O.TWIN_DT, nu=O.TWIN_NU)
    z, hist, evals, hvps = m.fit_incremental(guess, _observations(sets), R.GN_TWIN_OUTER, R.GN_TWIN_INNER)
    assert m.adjoint_recorded() == 0
    m.close()
    e0, e1 = rel_l2(guess, truth), rel_l2(_np(z), truth)
    print("Gauss-Newton twin on the GPU: J = %s; J_K / J_0 = %.4g (float64: %.4g, bar %.4g; L-BFGS on float64: %.4g); %d evaluations, %d products; z0 off by %.4g at the start, %.4g at the end"
          % (["%.4g" % j for j in hist], hist[-1] / hist[0], R.GN_TWIN_RATIO, 10 * R.GN_TWIN_RATIO, O.TWIN_RATIO, evals, hvps, e0, e1))
    assert len(hist) >= 2 and all(b < a for a, b in zip(hist, hist[1:]))
    assert hist[-1] / hist[0] <= 10 * R.GN_TWIN_RATIO
    assert e1 < e0


# ---- 9. singular vectors by replay ----
def test_singular_vectors_by_replay():
    """256^2, 3 steps, k = 4, 4 iterations (singular_numpy's case): sigma within SV_BAR of the float64 values at every iteration; the sine
    of the largest principal angle between the final subspace and float64's at most 4 x the figure the float32 restatement of the
    replayed iteration leaves on the CPU; the state is put back and the tape freed"""
    v, src, start = S.sv_inputs()
    s64, v64 = S.sv_reference()
    m = _model(S.SV_N, S.SV_N, v, src)
    z0 = _np(m.vort())
    sig, vv = m.singular_vectors(S.SV_STEPS, S.SV_K, S.SV_ITERS, start=start, replay=True)
    assert _same32(_np(m.vort()), z0) and m.adjoint_recorded() == 0
    m.close()
    err, ang = float(np.max(np.abs(sig / s64 - 1))), S.principal_sine(_np(vv), v64)
    print("singular_vectors(replay=True): sigma =\n%s\noff float64 by %.3g (bar %.3g); sine of the largest principal angle %.3g (float32 on the CPU %.3g, bar %.3g)"
          % (sig, err, S.SV_BAR, ang, R.SV_REPLAY_ANGLE_F32, R.SV_REPLAY_ANGLE_BAR))
    assert err <= S.SV_BAR
    assert ang <= R.SV_REPLAY_ANGLE_BAR


# ---- 10. refusals, the slab, the memory ----
def test_refusals_under_the_function_s_own_name_before_anything_is_launched():
    import torch
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    nx = ny = 256
    v, dz = _inputs(nx, ny)[:2]
    m = _model(nx, ny, v)
    buf = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())

    def refused(stem, args, phrase):
        name = "fb_model_" + stem
        assert getattr(L, name)(m._h, *args) == FB_EINVAL, (name, args)
        msg = L.fb_last_error().decode()
        assert msg.startswith(name + ": ") and phrase in msg, (name, args, msg)
    refused("tangent_replay", (0, 1), "no tangent is set")
    refused("observe_tangent", (0, 0, p, 4, p), "no tangent is set")
    m.set_tangents(_fields(nx, ny, 3))
    refused("tangent_replay", (0, 1), "no tape")
    refused("tangent_replay", (0, 0), "no tape")
    m.record_adjoint(4)
    m.step(2)                                                   # (the set rides along: the live tangent)
    before = _np(m.tangents())
    for args, phrase in (((0, 3), "2 on the tape"), ((2, 1), "2 on the tape"), ((3, 0), "2 on the tape"), ((-1, 1), "first < 0"), ((0, -1), "nsteps < 0"),
                         ((2 ** 31 - 1, 2 ** 31 - 1), "on the tape")):
        refused("tangent_replay", args, phrase)
    for args, phrase in (((3, 0, p, 4, p), "perturbation 3 of a set of 3"), ((0, 4, p, 4, p), "kind"), ((-1, 0, p, 4, p), "index < 0"),
                         ((0, 0, p, 0, p), "n outside"), ((0, 0, None, 4, p), "NULL")):
        refused("observe_tangent", args, phrase)
    refused("adjoint_rewind", (-2,), "n < -1")
    refused("adjoint_rewind", (1,), "0 popped")
    m.tangent_replay(2, 0)                                      # an empty range at the top: no refusal, nothing launched
    torch.cuda.synchronize()
    assert _same32(_np(m.tangents()), before) and bool((buf == 7.0).all())
    m.checkpoint_adjoint(2, 4)
    refused("tangent_replay", (0, 0), "not under adjoint checkpointing")
    m.close()


def test_slab_of_one_rank_returns_the_bits_of_the_model():
    S_ = _slab()
    nx = ny = 256
    dz = _inputs(nx, ny)[1]
    xy = O.positions(nx, ny)
    m, s = _recorded(nx, ny), _recorded(nx, ny, cls=S_.EngineSlab)
    assert _same32(_replayed(s, dz), _replayed(m, dz))
    for kind in O.KINDS:
        assert _same64(_np(s.observe_tangent(kind, xy)), _np(m.observe_tangent(kind, xy)))
    lam = _inputs(nx, ny)[3]
    for e in (m, s):
        e.set_adjoint(lam)
        e.adjoint_back(STEPS)
        e.adjoint_rewind()
        e.set_adjoint(lam)
        e.adjoint_back(STEPS)
    assert _same32(_np(s.adjoint()), _np(m.adjoint()))
    m.close()
    s.close()
    v, src, sets, d, w, bg = _hvp_reference(nx, ny)[:6]
    obs = _observations(sets)
    out = []
    for cls in (None, S_.EngineSlab):
        e = _model(nx, ny, None, src, cls=cls)
        e.fourdvar(v, obs, keep_tape=True)
        out.append(_np(e.gauss_newton_hvp(d, obs)))
        e.close()
    assert _same64(out[0], out[1])


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every new call raises with the engine's "several ranks" message"""
    import threading
    import xlab_fftbarotropic_amd as X
    S_ = _slab()
    n, world = 256, 2
    xy, w = O.positions(n, n), O.weights(O.NPTS)
    obs = [X.Observations(1, "u", xy, w)]
    hub = S_.local_hub(world)
    msgs, errs = [[] for _ in range(world)], [None] * world

    def work(r):
        try:
            s = S_.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                z = np.zeros((s.XL, n), np.float32)
                calls = (lambda: s.tangent_replay(0, 1), lambda: s.adjoint_rewind(-1), lambda: s.observe_tangent("vort", xy),
                         lambda: s.gauss_newton_hvp(z, obs), lambda: s.fit_incremental(z, obs, 1, 1))
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
    for r in range(world):
        assert len(msgs[r]) == 5
        for msg in msgs[r]:
            assert msg is not None and "invalid argument" in msg.lower() and "several ranks" in msg, msg


def test_model_info_counts_the_replay_workspace():
    """hbm_bytes grows at the first replay of a set by (4 + 5 min(M, 8)) real fields, for M = 1 and M = 9 at 256^2, and falls back when
    the set goes or changes its count"""
    n = 256
    m = _recorded(n, n)
    field = n * n * 4
    for count in (1, 9):
        m.set_tangents(_fields(n, n, count))
        h0 = m.info()["hbm_bytes"]
        m.tangent_replay(0, 1)
        assert m.info()["hbm_bytes"] == h0 + (4 + 5 * min(count, 8)) * field, count
        m.tangent_replay(1, 1)
        m.set_tangents(_fields(n, n, count))                    # the same count keeps the workspace
        assert m.info()["hbm_bytes"] == h0 + (4 + 5 * min(count, 8)) * field, count
    assert (4 + 5 * 1) * field == 2359296 and (4 + 5 * 8) * field == 11534336
    h1 = m.info()["hbm_bytes"]
    m.set_tangents(None)
    m.set_tangents(_fields(n, n, 9))
    assert m.info()["hbm_bytes"] == h1 - 44 * field
    m.close()
