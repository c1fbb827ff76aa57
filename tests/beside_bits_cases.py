"""The bits of everything stepped beside the vorticity on fixed inputs (tests/test_gpu_beside_bits.py, tests/golden/make_beside_bits_fixture.py):
the grids, and the one sequence of calls that the recording and the test both make.

The recording was made before the host paths of the tracer, the tangent set, the particles, the adjoint and its set, the checkpoints,
the replay and the observations were rephrased through shared helpers (csrc/fb_beside*.h): every entry point issues the same kernels,
memsets and copies in the same order as before, so every output has the bits it had.  All of these paths are deterministic by
construction: one stream, and integer atomics in the deposits."""
import hashlib

import numpy as np

import adjoint_numpy as A
import lagrangian_numpy as L
import lyapunov_numpy as Y
import obs_numpy as O
import tracer_numpy as T

# adjoint_numpy.PATH_CASES: the smallest grids that reach the three branches of stage_vstate and every row and column dispatch class
GRIDS = tuple((k.nx, k.ny) for k in A.PATH_CASES)
SLAB_GRIDS = ((256, 256), (1024, 64))                           # also on an EngineSlab of one rank, which must give the Model's digests
CHUNK_GRID = (256, 256)                                         # also sets of CHUNK + 1, so that the second chunk is a chunk of one
CHUNK = 8                                                       # ADJOINT_CHUNK (csrc/fb_adjoint.h) and REPLAY_CHUNK (csrc/fb_replay.h)
STEPS = A.STEPS
NOISE = A.PATH_CASES[0].vort_noise
SEED = L.SEED + 1000


def _sha(x):
    a = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _noise(count, nx, ny, seed):
    return np.random.default_rng(seed).standard_normal((count, nx, ny)).astype(np.float32)


def digests(m, nx, ny):
    """On the fresh model m (Model or EngineSlab of one rank; nu = tangent_numpy.NU, dt = tracer_numpy.recipe_dt): the SHA-256 of the
    bytes of every output of the sequence below, by name, in the order they are taken."""
    import torch
    v, _, src, lam = A.adjoint_inputs(nx, ny, NOISE)
    W = Y.subspace_inputs(nx, ny, NOISE)[1]
    c0 = T.noisy_inputs(nx, ny, NOISE)[1]
    xy, xbT = O.positions(nx, ny), L.xbar_T(L.NPTS)
    zeros = torch.zeros((nx, ny), dtype=torch.float32, device="cuda")
    wide = (nx, ny) == CHUNK_GRID
    out = {}
    # 1. everything that steps beside the vorticity
    m.set_vort(v)
    m.set_source(src)
    m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
    m.set_tangents(W)
    m.set_particles(xy)
    m.set_particle_deformation()
    m.step(STEPS)
    for name in ("vort", "tracer", "tangents", "particles", "particle_deformation"):
        out["stepped." + name] = _sha(getattr(m, name)())
    # 2. the single adjoint over the full tape
    m.record_adjoint(STEPS)
    m.step(STEPS)
    m.set_adjoint(lam)
    m.adjoint_back(STEPS)
    out["adjoint.adjoint"], out["adjoint.vort"] = _sha(m.adjoint()), _sha(m.vort())
    # 3. a set of adjoints over the same tape
    for count in (3, CHUNK + 1) if wide else (3,):
        m.adjoint_rewind()
        m.set_adjoints(_noise(count, nx, ny, SEED + count))
        m.adjoint_back(STEPS)
        out["adjoints.%d" % count] = _sha(m.adjoints())
    # 4. the tangent replay over it
    for count in (3, CHUNK + 1) if wide else (3,):
        m.set_tangents(W if count == 3 else _noise(count, nx, ny, SEED + 100 + count))
        m.tangent_replay(0, STEPS)
        out["replay.%d" % count] = _sha(m.tangents())
    m.set_tangents(W)
    # 5. the observations and the forcing of a single adjoint by each kind
    m.set_adjoint(lam)
    w = np.random.default_rng(SEED + 200).standard_normal(xy.shape[0])
    for kind in O.KINDS:
        out["observe." + kind] = _sha(m.observe(kind, xy))
        m.adjoint_add_obs(kind, xy, w)
        out["add_obs." + kind] = _sha(m.adjoint())
    # 6. the drifters' sweep
    m.record_particles(STEPS)
    m.record_adjoint(STEPS)
    m.step(STEPS)
    m.set_adjoint(zeros)
    m.set_particle_adjoint(xbT)
    m.adjoint_back(STEPS)
    out["drifters.adjoint"], out["drifters.particle_adjoint"] = _sha(m.adjoint()), _sha(m.particle_adjoint())
    m.set_particle_adjoint(None)
    m.record_particles(0)
    # 7. a checkpointed window: the segment is filled again three times, and the live state put back
    m.checkpoint_adjoint(2, STEPS)
    m.step(STEPS)
    m.set_adjoint(lam)
    m.adjoint_back(STEPS)
    out["checkpoint.adjoint"], out["checkpoint.vort"] = _sha(m.adjoint()), _sha(m.vort())
    return out


def model(nx, ny, slab=False):
    from importlib import import_module
    mod = import_module("xlab-fftbarotropic_amd.slab" if slab else "xlab_fftbarotropic_amd")
    return (mod.EngineSlab if slab else mod.Model)(nx, ny, nu=A.G.NU, dt=T.recipe_dt(nx, ny))
