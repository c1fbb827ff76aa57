"""CPU checks of adjoint checkpointing: the float64 reference (tests/checkpoint_numpy.py) gives lam_0 of the full tape exactly for every
spacing, swept at once and in pieces, and runs every step of the window again exactly once; binding.checkpoint_every against a
brute-force argmin; binding.fourdvar and binding.singular_vectors on float64 models return with checkpoint_every = K exactly what they
return without; the pair table of the two new entry points and the argument checks that run before any HIP call.  No GPU needed."""
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
import checkpoint_numpy as K                                    # noqa: E402
import obs_numpy as O                                           # noqa: E402
import singular_numpy as S                                      # noqa: E402
import tracer_numpy as T                                        # noqa: E402

STEMS = ("adjoint_checkpoint", "adjoint_checkpoint_info")
FB_EINVAL = 1
N, STEPS = 64, 7
EVERY = (1, 2, 3, 7, 9)


def _binding():
    return import_module("xlab-fftbarotropic_amd.binding")


@pytest.fixture(scope="module")
def inputs():
    out = A.adjoint_inputs(N, N, 3e-2)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def full_tape(inputs):
    """(lam_0, the tangent, the vorticity) of the full tape's run, computed once"""
    m = A.run_case(N, N, *inputs, STEPS, cls=K.CheckpointModel64)
    return m.adjoint(), m.tangent(), m.vort()


# ---- the float64 reference ----
@pytest.mark.parametrize("pieces", [(STEPS,), (3, 4)], ids=["at once", "3 + 4"])
@pytest.mark.parametrize("every", EVERY)
def test_checkpointed_sweep_is_the_full_tape_sweep_exactly(inputs, full_tape, every, pieces):
    """64^2, 7 steps with a source and a tangent: lam_0 is exactly the full tape's, the tangent and the vorticity the model carries are
    what they were before the sweep, adjoint_recorded counts down, the checkpoints are ceil(T / K) and replayed == T"""
    v, d, s, lam = inputs
    m = A.recipe_model(N, N, v, d, s, cls=K.CheckpointModel64)
    m.checkpoint_adjoint(every, STEPS)
    m.step(STEPS)
    assert m.adjoint_recorded() == STEPS and not m.tape
    assert m.adjoint_checkpoints() == (every, STEPS, -(-STEPS // every), 0)
    td, vt = m.tangent(), m.vort()
    m.set_adjoint(lam)
    left = STEPS
    for n in pieces:
        m.adjoint_back(n)
        left -= n
        assert m.adjoint_recorded() == left
    assert np.array_equal(m.adjoint(), full_tape[0])
    assert np.array_equal(m.tangent(), td) and np.array_equal(td, full_tape[1])
    assert np.array_equal(m.vort(), vt) and np.array_equal(vt, full_tape[2])
    assert m.adjoint_checkpoints() == (every, STEPS, -(-STEPS // every), STEPS)
    with pytest.raises(ValueError, match="swept"):
        m.step(1)
    m.checkpoint_adjoint(0)
    assert m.adjoint_checkpoints() == (0, 0, 0, 0)


def test_window_discipline_of_the_reference(inputs):
    v, d, s, lam = inputs
    m = A.recipe_model(N, N, v, d, s, cls=K.CheckpointModel64)
    m.checkpoint_adjoint(2, 3)
    m.step(2)
    with pytest.raises(ValueError, match="max_steps"):
        m.step(2)
    assert m.adjoint_recorded() == 2
    m.set_vort(v)
    assert m.adjoint_recorded() == 0 and m.adjoint_checkpoints() == (2, 3, 0, 0)
    m.record_adjoint(2)
    assert m.adjoint_checkpoints() == (0, 0, 0, 0)
    m.step(2)
    assert m.adjoint_recorded() == 2


# ---- checkpoint_every ----
def test_checkpoint_every_is_the_argmin():
    """for every T in 1..2000 the K >= 1 that minimises ceil(T / K) + 4 K, the smallest of equal ones"""
    import xlab_fftbarotropic_amd as X
    for steps in range(1, 2001):
        assert X.checkpoint_every(steps) == K.checkpoint_every_brute(steps), steps
    assert X.checkpoint_every(10000) == 50 and K.slots(10000, 50) == 400
    for bad in (0, -3):
        with pytest.raises(ValueError):
            X.checkpoint_every(bad)


# ---- the helpers of the binding on float64 models ----
def _torch_sets(sets):
    import torch
    out = []
    for o in sets:
        n = len(o.y)
        sigma = None if o.sigma is None else torch.from_numpy(np.broadcast_to(np.asarray(o.sigma, dtype=np.float64), (n,)).copy())
        out.append(O.Obs(o.step, o.kind, torch.from_numpy(np.asarray(o.xy, dtype=np.float64)), torch.from_numpy(np.asarray(o.y, dtype=np.float64)), sigma))
    return out


def test_fourdvar_with_checkpoints_returns_what_it_returns_without():
    """binding.fourdvar on the float64 model with observations (the gradient case of tests/obs_numpy.py at 64^2: zeta at step 0, u and v
    at the steps 2, 4, 6, so the sweep goes in pieces of 2): J and the gradient with checkpoint_every = 1, 4, 7 and "sqrt" are exactly
    those of the full tape, with and without a background term, and the mode is off afterwards"""
    import torch
    B = _binding()
    m = K.CheckpointObs64(N, N, nu=A.G.NU, dt=T.recipe_dt(N, N))
    v, src, sets, _ = O.gradient_case(N, N, m)
    m.src = src.astype(np.float64)
    face, sets = K.TorchFace(m), _torch_sets(sets)
    z0 = torch.from_numpy(v.astype(np.float64))
    for bg in (None, (v * 0.9, 1e-3)):
        J0, g0 = B.fourdvar(face, z0, sets, bg)
        assert J0 > 0 and float(g0.abs().max()) > 0
        for every in (1, 4, 7, "sqrt"):
            J, g = B.fourdvar(face, z0, sets, bg, checkpoint_every=every)
            assert J == J0 and torch.equal(g, g0), every
            assert m.adjoint_checkpoints() == (0, 0, 0, 0) and m.depth == 0
    for bad in (0, -1, 1.5, "root"):
        with pytest.raises(ValueError, match="checkpoint_every"):
            B.fourdvar(face, z0, sets, checkpoint_every=bad)


def test_fit_initial_hands_the_keyword_on():
    import torch
    B = _binding()
    seen = []

    class Q:
        def __init__(self):
            self.torch = torch

        def fourdvar(self, z, obs, background=None, **kw):
            seen.append(kw)
            return float(0.5 * (z * z).sum()), z.clone()
    B.fit_initial(Q(), np.ones(4), None, 1)
    assert seen and all(kw == {} for kw in seen)
    del seen[:]
    B.fit_initial(Q(), np.ones(4), None, 1, checkpoint_every=3)
    assert seen and all(kw == {"checkpoint_every": 3} for kw in seen)


def test_singular_vectors_with_checkpoints_returns_what_it_returns_without():
    """binding.singular_vectors on the float64 model of the dense check (tests/singular_numpy.py: 32^2, 4 steps): sigma and V with
    checkpoint_every = 1, 3 and 5 are exactly those of the full tape.  The tangent subspace rides the forward run only: a replay that
    carried it would move the tangents that the next iteration's Gram matrix is made of"""
    import torch
    B = _binding()
    start = np.random.default_rng(S.DENSE_SEED).standard_normal((3, S.DENSE_N, S.DENSE_N))
    out = []
    for every in (None, 1, 3, 5):
        v = A.adjoint_inputs(S.DENSE_N, S.DENSE_N, A.PATH_CASES[0].vort_noise)[0]
        m = K.CheckpointModel64(S.DENSE_N, S.DENSE_N, nu=A.G.NU, dt=S.DENSE_DT)
        m.set_vort(v)
        z0 = m.spectrum()
        sig, vec = B.singular_vectors(K.TorchFace(m), S.DENSE_STEPS, 3, 3, start, checkpoint_every=every)
        assert np.array_equal(m.spectrum(), z0) and m.adjoint_checkpoints() == (0, 0, 0, 0) and m.depth == 0
        out.append((sig, vec))
    assert np.all(out[0][0][-1] > 1.0)
    for sig, vec in out[1:]:
        assert np.array_equal(sig, out[0][0]) and torch.equal(vec, out[0][1])


# ---- the entry points ----
def test_pair_table_holds_exactly_the_new_stems():
    import xlab_fftbarotropic_amd as X
    B = _binding()
    assert set(B._CHECKPOINT_PAIRS) == set(STEMS) and not set(B._CHECKPOINT_PAIRS) & set(B._PAIRS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fftbaro.h")).read(), flags=re.S)
    want = {"adjoint_checkpoint": r"int every, int max_steps",
            "adjoint_checkpoint_info": r"int \*every, int \*max_steps, int \*checkpoints, long long \*replayed"}
    for stem in STEMS:
        for kind, handle in (("model", r"fb_model \*m"), ("slab", r"fb_slab \*s")):
            name = "fb_%s_%s" % (kind, stem)
            assert re.search(r"\bint\s+%s\s*\(%s, %s\)\s*;" % (name, handle, want[stem]), src), name
            assert name in X.EXPORTS and name in B.SIGNATURES, name
            assert len(B.SIGNATURES[name][0]) == 1 + len(B._CHECKPOINT_PAIRS[stem]), name
    assert B.SIGNATURES["fb_model_adjoint_checkpoint_info"][0][-1] is ctypes.POINTER(ctypes.c_longlong)
    slab = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (X.Model, slab.EngineSlab):
        for n in ("checkpoint_adjoint", "adjoint_checkpoints"):
            assert callable(getattr(cls, n, None)), (cls, n)
    assert callable(X.checkpoint_every)


def test_argument_errors_are_refused_by_the_engine_without_a_device():
    """every outside [0, 2^20], max_steps < 1, more than 2^20 checkpoints and NULL handles: FB_EINVAL and a message that starts with the
    function's name and names the bound, before any HIP call (there is no device here)"""
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    for kind in ("model", "slab"):
        fn = getattr(L, "fb_%s_adjoint_checkpoint" % kind)
        # (the arguments are refused before the handle is looked at)
        for args, word in (((-1, 4), b"every outside [0, 2^20]"), (((1 << 20) + 1, 4), b"every outside [0, 2^20]"),
                           ((2, 0), b"max_steps < 1"), ((1, (1 << 20) + 1), b"more than 2^20 checkpoints"),
                           ((2, 4), b"NULL " + kind.encode()), ((0, 0), b"NULL " + kind.encode())):
            assert fn(None, *args) == FB_EINVAL, (kind, args)
            msg = L.fb_last_error()
            assert msg.startswith(b"fb_%s_adjoint_checkpoint: " % kind.encode()) and word in msg, msg
        info = getattr(L, "fb_%s_adjoint_checkpoint_info" % kind)
        assert info(None, None, None, None, None) == FB_EINVAL
        assert L.fb_last_error().startswith(b"fb_%s_adjoint_checkpoint_info: NULL %s" % (kind.encode(), kind.encode()))
