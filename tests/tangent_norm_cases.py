"""The bits of the tangent's norm and of the Gram matrix on fixed inputs (tests/test_gpu_lyapunov.py, tests/golden/make_tangent_norm_fixture.py):
the grids, and the one sequence of calls that the recording and the test both make.

The norm is the inner product of perturbation 0 with itself, one kernel (k_tangent_dot, csrc/fb_tangent.h); the recording was made
while the norm had a kernel of its own, so equal bits say that the merged kernel sums what the norm's did, in its order."""
import numpy as np

import lyapunov_numpy as Y
import tangent_numpy as G
import tracer_numpy as T

# 64^2: one workgroup row; 192^2: the radix-3 size; 1024 x 64: a strip, several workgroups; 2048 x 1024: the smallest grid at which
# the grid of partial sums is capped (nx P / 2 = 540672 > 256 * 8 CUs * 256), so that the grid-stride loop runs a second time and the
# final kernel strides over 2048 partial sums
GRIDS = ((64, 64), (192, 192), (1024, 64), (2048, 1024))
GRAM_GRIDS = GRIDS[:3]
STEPS, FACTOR = 2, -1.75


def _u64(x):
    return [int(v) for v in np.ascontiguousarray(x, dtype=np.float64).ravel().view(np.uint64)]


def bits(m, nx, ny):
    """On the fresh model m (Model or EngineSlab of one rank; nu = tangent_numpy.NU, dt = tracer_numpy.recipe_dt), with the inputs of
    tangent_numpy.tangent_inputs: per kind the uint64 bits of tangent_norm right after set_tangent, after STEPS steps and after
    rescale_tangent(FACTOR); on GRAM_GRIDS also those of tangent_gram (row-major) of lyapunov_numpy.subspace_inputs' three."""
    v0, d0, _ = G.tangent_inputs(nx, ny, Y.NOISE)
    m.set_vort(v0)
    m.set_tangent(d0)
    out = {kind: {} for kind in Y.KINDS}
    for when in ("set", "stepped", "rescaled"):
        if when == "stepped":
            m.step(STEPS)
        elif when == "rescaled":
            m.rescale_tangent(FACTOR)
        for kind in Y.KINDS:
            out[kind][when] = _u64(m.tangent_norm(kind))[0]
    if (nx, ny) in GRAM_GRIDS:
        m.set_tangents(Y.subspace_inputs(nx, ny)[1])
        for kind in Y.KINDS:
            out[kind]["gram"] = _u64(m.tangent_gram(kind).cpu().numpy())
    return out


def model(nx, ny, slab=False):
    from importlib import import_module
    mod = import_module("xlab-fftbarotropic_amd.slab" if slab else "xlab_fftbarotropic_amd")
    return (mod.EngineSlab if slab else mod.Model)(nx, ny, nu=G.NU, dt=T.recipe_dt(nx, ny))
