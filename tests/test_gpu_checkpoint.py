"""Adjoint checkpointing on the GPU (fb_model_adjoint_checkpoint, fb_model_adjoint_checkpoint_info and what fb_model_step and
fb_model_adjoint_back do while the mode is on; host layer csrc/fb_beside_adjoint.h) against the engine's own full tape: every comparison is by
bits.  The inputs are adjoint_numpy.adjoint_inputs with the source set (never-dealiased noise on every field).  The grids are those of
adjoint_numpy.PATH_CASES (the three-kernel x pass in its layouts) and 4096^2 (k_col_full); DESIGN.md, "Adjoint checkpointing", has
the scheme, the continuity probe that a checkpoint of the state arrays alone rests on, and the memory table."""
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
import entry_cases as E                                         # noqa: E402
import obs_numpy as O                                           # noqa: E402
import particles_numpy as P                                     # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

STEPS = 5
BIG = (4096, 4096)
PATH_GRIDS = [(k.nx, k.ny) for k in A.PATH_CASES]


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


def _model(nx, ny, cls=None):
    """the vorticity and the source of the inputs set"""
    import xlab_fftbarotropic_amd as X
    v, _, s, _ = _inputs(nx, ny)
    m = (cls or X.Model)(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))
    m.set_vort(v)
    m.set_source(s)
    return m


@functools.lru_cache(maxsize=None)
def _full_tape(nx, ny):
    """lam_0 of STEPS steps swept over the full tape, once per grid"""
    m = _model(nx, ny)
    m.record_adjoint(STEPS)
    m.step(STEPS)
    m.set_adjoint(_inputs(nx, ny)[3])
    m.adjoint_back(STEPS)
    out = _np(m.adjoint())
    m.close()
    out.setflags(write=False)
    return out


# ---- 1. continuity ----
@pytest.mark.parametrize("nx,ny", [(256, 256), (3072, 64), (64, 4096), BIG])
def test_stepping_on_after_a_checkpointed_sweep_is_stepping_on(nx, ny):
    """step(3); a checkpointed window of 4 steps, swept; the mode off; step(2): the vorticity is that of step(9) on an untouched model.
    The sweep puts a checkpoint back twice and the live state once, each by a copy and the priming pass"""
    lam = _inputs(nx, ny)[3]
    a, b = _model(nx, ny), _model(nx, ny)
    a.step(3)
    a.checkpoint_adjoint(2, 4)
    a.step(4)
    a.set_adjoint(lam)
    a.adjoint_back(4)
    assert a.adjoint_checkpoints() == (2, 4, 2, 4)
    a.checkpoint_adjoint(0)
    a.step(2)
    b.step(9)
    va, vb = _np(a.vort()), _np(b.vort())
    a.close()
    b.close()
    assert _same32(va, vb)
    assert rel_l2(vb, _inputs(nx, ny)[0]) > 1e-6


# ---- 2. the checkpointed sweep is the full tape's ----
SWEEPS = [(nx, ny, 2) for nx, ny in PATH_GRIDS] + [(256, 256, 1), (256, 256, 5), (256, 256, 7), BIG + (2,)]


@pytest.mark.parametrize("nx,ny,every", SWEEPS, ids=["%dx%d-K%d" % k for k in SWEEPS])
def test_checkpointed_sweep_equals_full_tape_sweep(nx, ny, every):
    """T = 5 (K = 2: segments of 2, 2 and a partial one of 1; K = 7: one segment that never fills): lam_0 has the full tape's bits,
    adjoint_recorded counts down, the checkpoints are ceil(T / K) and the sweep has taken T steps again"""
    lam = _inputs(nx, ny)[3]
    m = _model(nx, ny)
    m.checkpoint_adjoint(every, STEPS)
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (every, STEPS, 0, 0)
    m.step(STEPS)
    nck = -(-STEPS // every)
    assert m.adjoint_recorded() == STEPS and m.adjoint_checkpoints() == (every, STEPS, nck, 0)
    before = _np(m.vort())
    m.set_adjoint(lam)
    m.adjoint_back(1)
    assert m.adjoint_recorded() == STEPS - 1
    m.adjoint_back(STEPS - 1)
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (every, STEPS, nck, STEPS)
    l0, after = _np(m.adjoint()), _np(m.vort())
    m.close()
    assert _same32(l0, _full_tape(nx, ny))
    assert _same32(after, before)                               # the live state is back
    assert rel_l2(l0, lam) > 1e-3


# ---- 3. split sweeps ----
def test_split_sweeps_replay_nothing_twice():
    """256^2, K = 2: 3 then 2 is 5 at once (the second piece starts on what the first left of its segment) with replayed == 5; and with
    adjoint_add_obs between the pieces it is the same on the full tape"""
    n = 256
    lam = _inputs(n, n)[3]
    xy, w = O.positions(n, n), O.weights(O.NPTS)
    out = {}
    for how in ("checkpoints", "tape"):
        for forced in (False, True):
            m = _model(n, n)
            if how == "tape":
                m.record_adjoint(STEPS)
            else:
                m.checkpoint_adjoint(2, STEPS)
            m.step(STEPS)
            m.set_adjoint(lam)
            m.adjoint_back(3)
            assert m.adjoint_recorded() == 2
            if how == "checkpoints":
                assert m.adjoint_checkpoints()[3] == 3          # the segments of step 4 and of steps 2, 3; step 2 stays on the tape
            if forced:
                m.adjoint_add_obs("u", xy, w)
            m.adjoint_back(2)
            assert m.adjoint_recorded() == 0
            if how == "checkpoints":
                assert m.adjoint_checkpoints()[3] == STEPS
            out[how, forced] = _np(m.adjoint())
            m.close()
    assert _same32(out["checkpoints", False], _full_tape(n, n)) and _same32(out["tape", False], _full_tape(n, n))
    assert _same32(out["checkpoints", True], out["tape", True])
    assert rel_l2(out["tape", True], out["tape", False]) > 1e-6


# ---- 4. a set ----
def test_a_set_of_three_is_swept_as_on_the_full_tape():
    n = 256
    rms = np.sqrt(np.mean(_inputs(n, n)[0].astype(np.float64) ** 2))
    lams = (np.random.default_rng(A.SEED + 10).standard_normal((3, n, n)) * rms).astype(np.float32)
    out = []
    for every in (0, 2):
        m = _model(n, n)
        if every:
            m.checkpoint_adjoint(every, STEPS)
        else:
            m.record_adjoint(STEPS)
        m.step(STEPS)
        m.set_adjoints(lams)
        m.adjoint_back(STEPS)
        out.append(_np(m.adjoints()))
        m.close()
    for k in range(3):
        assert _same32(out[0][k], out[1][k]), k
    assert rel_l2(out[0][1], out[0][2]) > 1e-3


# ---- 5. bystanders ----
def test_tracer_particles_deformation_and_tangent_never_see_the_mode():
    """256^2, 6 steps with K = 4, a tracer, particles with their deformation gradient, a tangent and the source set: with use_graph off
    and on (a stream of its own) everything equals the run with the mode off, and after the sweep everything is unchanged again, the
    deformation's elapsed time included"""
    import torch
    import xlab_fftbarotropic_amd as X
    n, steps = 256, 6
    v0, d0, src, lam = _inputs(n, n)
    c0 = T.noisy_inputs(n, n, 3e-2)[1]
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, 64, seed=5)

    def state(m):
        return (_np(m.vort()), _np(m.tracer()), _np(m.tangent()), _np(m.particles()), _np(m.particle_deformation()), m.particle_deformation_time())

    def same(a, b):
        return _same32(a[0], b[0]) and _same32(a[1], b[1]) and _same32(a[2], b[2]) and _same64(a[3], b[3]) and _same64(a[4], b[4]) and a[5] == b[5]
    out = {}
    for graph in (False, True):
        for every in (0, 4):
            with torch.cuda.stream(torch.cuda.Stream()):
                m = X.Model(n, n, nu=A.G.NU, dt=3.0)
                m.fop.use_current_stream()
                m.use_graph(graph)
                m.set_vort(v0)
                m.set_source(src)
                m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
                m.set_particles(x0)
                m.set_particle_deformation()
                m.set_tangent(d0)
                if every:
                    m.checkpoint_adjoint(every, steps)
                m.step(steps)
                out[graph, every] = state(m)
                if every:
                    m.set_adjoint(lam)
                    m.adjoint_back(steps)
                    assert m.adjoint_checkpoints() == (every, steps, 2, steps)
                    assert same(state(m), out[graph, every])
                    out[graph, "lam"] = _np(m.adjoint())
                m.close()
    for key in ((False, 4), (True, 0), (True, 4)):
        assert same(out[key], out[False, 0]), key
    assert _same32(out[False, "lam"], out[True, "lam"])
    assert rel_l2(out[False, 0][2], d0) > 1e-4 and out[False, 0][5] == steps * 3.0


# ---- 6. the helpers ----
def test_fourdvar_with_checkpoints_returns_the_full_tape_s_bits():
    """the gradient case of tests/test_gpu_obs.py at 256^2 (zeta at step 0, u and v at the steps 2, 4, 6): J and grad of
    fourdvar(z0, obs, checkpoint_every=2) and of "sqrt" are those of fourdvar(z0, obs), and the mode is off afterwards"""
    import xlab_fftbarotropic_amd as X
    n = 256
    ref = O.ObsModel64(n, n, nu=A.G.NU, dt=T.recipe_dt(n, n))
    v, src, sets, _ = O.gradient_case(n, n, ref)
    obs = [X.Observations(s.step, s.kind, s.xy, s.y, s.sigma) for s in sets]
    m = X.Model(n, n, nu=A.G.NU, dt=T.recipe_dt(n, n))
    m.set_source(src)
    J0, g0 = m.fourdvar(v, obs)
    for every in (2, "sqrt"):
        J, g = m.fourdvar(v, obs, checkpoint_every=every)
        assert J == J0 and _same64(_np(g), _np(g0)), every
        assert m.adjoint_checkpoints() == (0, 0, 0, 0) and m.adjoint_recorded() == 0
    assert J0 > 0 and float(g0.abs().max()) > 0
    with pytest.raises(ValueError, match="checkpoint_every"):
        m.fourdvar(v, obs, checkpoint_every=0)
    m.close()


def test_singular_vectors_with_checkpoints_returns_the_full_tape_s_bits():
    """singular_vectors(3, 2, 2, checkpoint_every=2) returns the sigma and the V of singular_vectors(3, 2, 2): the tangent subspace rides
    the forward run and not the steps the sweep takes again"""
    n = 256
    m = _model(n, n)
    before = _np(m.vort())
    s0, v0 = m.singular_vectors(3, 2, 2)
    s1, v1 = m.singular_vectors(3, 2, 2, checkpoint_every=2)
    assert np.array_equal(s0, s1) and _same32(_np(v0), _np(v1))
    assert _same32(_np(m.vort()), before) and m.adjoint_checkpoints() == (0, 0, 0, 0)
    m.close()


# ---- 7. discipline ----
def test_window_discipline():
    import xlab_fftbarotropic_amd as X
    n = 256
    v, _, s, lam = _inputs(n, n)
    m = _model(n, n)

    def refused(call, *words):
        with pytest.raises(X.FftBaroError) as e:
            call()
        msg = str(e.value)
        assert "invalid argument" in msg.lower() and all(w in msg for w in words), msg
    m.checkpoint_adjoint(2, 3)
    m.set_source(s)                                             # an empty window: allowed
    m.step(2)
    before = _np(m.vort())
    refused(lambda: m.step(2), "fb_model_step", "room for 1 more steps")   # past max_steps: nothing launched, nothing counted
    assert m.adjoint_recorded() == 2 and m.adjoint_checkpoints() == (2, 3, 1, 0)
    assert _same32(_np(m.vort()), before)
    refused(lambda: m.set_source(s), "fb_model_set_source", "checkpointed window holds 2 steps")
    refused(lambda: m.set_source(None), "fb_model_set_source", "checkpointed window holds 2 steps")
    refused(lambda: m.profile_steps(1), "fb_model_profile_steps", "checkpointing is on")
    m.step(1)
    m.set_adjoint(lam)
    refused(lambda: m.adjoint_back(4), "fb_model_adjoint_back", "4 steps asked for, 3 recorded")
    m.adjoint_back(1)
    refused(lambda: m.step(1), "fb_model_step", "the window has been swept: start a new one")
    m.set_vort(v)                                               # empties the window
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (2, 3, 0, 0)
    m.step(3)
    assert m.adjoint_checkpoints() == (2, 3, 2, 0)
    m.set_spectrum(m.spectrum())
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (2, 3, 0, 0)
    # the bounds, with the bound in the text; a refused call leaves the mode as it was
    refused(lambda: m.checkpoint_adjoint(-1, 4), "fb_model_adjoint_checkpoint", "every outside [0, 2^20]")
    refused(lambda: m.checkpoint_adjoint(2, 0), "fb_model_adjoint_checkpoint", "max_steps < 1")
    refused(lambda: m.checkpoint_adjoint(1, (1 << 20) + 1), "fb_model_adjoint_checkpoint", "more than 2^20 checkpoints")
    assert m.adjoint_checkpoints() == (2, 3, 0, 0)
    # the two modes replace each other
    h0 = m.info()["hbm_bytes"]
    m.record_adjoint(3)
    assert m.adjoint_checkpoints() == (0, 0, 0, 0)
    m.step(3)
    assert m.adjoint_recorded() == 3
    refused(lambda: m.step(1), "fb_model_step", "tape has room for 0 more steps")
    m.set_source(s)                                             # the full tape does not mind
    m.checkpoint_adjoint(2, 3)
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (2, 3, 0, 0) and m.info()["hbm_bytes"] == h0
    m.checkpoint_adjoint(0)
    m.step(7)                                                   # neither mode: no limit
    assert m.adjoint_recorded() == 0
    m.close()


def test_slab_of_one_rank_gives_the_bits_of_the_model():
    n = 256
    lam = _inputs(n, n)[3]
    s = _model(n, n, cls=_slab().EngineSlab)
    s.checkpoint_adjoint(2, STEPS)
    s.step(STEPS)
    before = _np(s.vort_local())
    s.set_adjoint(lam)
    s.adjoint_back(3)
    s.adjoint_back(2)
    assert s.adjoint_recorded() == 0 and s.adjoint_checkpoints() == (2, STEPS, 3, STEPS)
    assert _same32(_np(s.adjoint()), _full_tape(n, n))
    assert _same32(_np(s.vort_local()), before)
    s.checkpoint_adjoint(0)
    s.step(2)
    m = _model(n, n)
    m.step(STEPS + 2)
    assert _same32(_np(s.vort_local()), _np(m.vort()))
    s.close()
    m.close()


def test_slab_of_two_ranks_refuses_both():
    """an unconnected slab, rank 0 of world 2 (tests/entry_cases.py): the adjoint's refusal of several ranks, under each function's own name"""
    h = E.Handles()
    try:
        for fn, args in (("fb_slab_adjoint_checkpoint", ["S", 2, 4]), ("fb_slab_adjoint_checkpoint", ["S", 0, 0]),
                         ("fb_slab_adjoint_checkpoint_info", ["S", "host", "host", "host", "host"])):
            rc, msg = h.call(fn, args)
            assert rc == 1 and msg.startswith(fn + ": ") and "the adjoint model is not supported on a slab of several ranks (world > 1)" in msg, (fn, rc, msg)
        rc, msg = h.call("fb_model_adjoint_checkpoint_info", ["M", "host", "host", "host", "host"])
        assert rc == 0, msg
    finally:
        h.close()


# ---- 8. memory ----
def test_info_counts_the_checkpoints_the_segment_and_the_live_copy():
    """256^2, checkpoint_adjoint(4, 64): hbm_bytes grows by 16 checkpoints + 16 slots of the segment + the live copy, one half spectrum
    each (a checkpoint is the state arrays alone: DESIGN.md, "Adjoint checkpointing"; the half spectrum's padded size is taken from
    the tracer's 3), which is less than a quarter of the 256 that record_adjoint(64) adds"""
    n = 256
    m = _model(n, n)
    h0 = m.info()["hbm_bytes"]
    m.set_tracer(_inputs(n, n)[0])
    half, rem = divmod(m.info()["hbm_bytes"] - h0, 3)
    m.set_tracer(None)
    assert rem == 0 and half >= n * (n // 2 + 1) * 8 and m.info()["hbm_bytes"] == h0
    m.checkpoint_adjoint(4, 64)
    ck = m.info()["hbm_bytes"] - h0
    m.record_adjoint(64)
    tape = m.info()["hbm_bytes"] - h0
    m.record_adjoint(0)
    assert m.info()["hbm_bytes"] == h0
    m.close()
    assert ck == (16 + 4 * 4 + 1) * half
    assert tape == 4 * 64 * half
    assert ck / tape < 0.25
