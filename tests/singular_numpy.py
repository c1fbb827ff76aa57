"""float64 numpy reference of binding.singular_vectors: orthogonal (block power) iteration on T^T T in the L2 norm, T the tangent of
`steps` steps of adjoint_numpy.AdjointModel64 (or its float32 restatement, adjoint_numpy.Float32Model) from a kept state.  The k
vectors are carried one at a time: per vector the state is restored, the tangent stepped with the tape on, lam = T v_i set and swept
back; nothing needs a subspace on the CPU.  Per iteration, with V [k, nx, ny] orthonormal:

    U_i = T v_i;   G = U U^T (k x k), G = E diag(sigma^2) E^T sorted descending;   W_i = T^T U_i;   V <- orthonormalise(E^T W)

so sigma depends on span(V) alone.  Also the principal angle between two subspaces, the dense tangent matrix of a small grid, the case
of the GPU test and the float32 figure its bar is taken from.  Used ONLY by tests."""
import numpy as np

import adjoint_numpy as A


def orthonormal_rows(w):
    """the rows of w [k, n] orthonormalised in their order in float64: modified Gram-Schmidt, run twice"""
    q = np.array(w, dtype=np.float64)
    for _ in range(2):
        for j in range(q.shape[0]):
            for i in range(j):
                q[j] -= (q[i] @ q[j]) * q[i]
            q[j] /= np.linalg.norm(q[j])
    return q


def singular_vectors(model, spectrum0, steps, k, iters, start, tol=None):
    """(sigma float64 [iterations done, k], the final V float64 [k, nx, ny]) on anything with the methods of the float64 model (set_spectrum,
    set_tangent, tangent, record_adjoint, step, set_adjoint, adjoint_back, adjoint).  tol: stop after the first iteration whose sigma all
    moved by less than tol relative to the iteration before (iters is then the cap)."""
    start = np.asarray(start, dtype=np.float64)
    shape = start.shape[1:]
    assert start.shape[0] == k
    v = orthonormal_rows(start.reshape(k, -1))
    sig = []
    for _ in range(iters):
        u, w = np.empty_like(v), np.empty_like(v)
        for i in range(k):
            model.set_spectrum(spectrum0)
            model.set_tangent(v[i].reshape(shape))
            model.record_adjoint(steps)
            model.step(steps)
            ui = np.asarray(model.tangent(), dtype=np.float64)
            u[i] = ui.ravel()
            model.set_adjoint(ui)
            model.adjoint_back(steps)
            w[i] = np.asarray(model.adjoint(), dtype=np.float64).ravel()
        lam, e = np.linalg.eigh(u @ u.T)
        order = np.argsort(lam)[::-1]
        sig.append(np.sqrt(np.maximum(lam[order], 0.0)))
        v = orthonormal_rows(e[:, order].T @ w)
        if tol is not None and len(sig) > 1 and np.max(np.abs(sig[-1] / sig[-2] - 1)) < tol:
            break
    model.record_adjoint(0)
    model.set_spectrum(spectrum0)
    return np.array(sig), v.reshape((k,) + tuple(shape))


def principal_sine(a, b):
    """the sine of the largest principal angle between span(a) and span(b), a and b [k, ...] in any basis: with Qa, Qb orthonormal, the
    largest singular value of (I - Qa Qa^T) Qb, in float64"""
    k = a.shape[0]
    qa = orthonormal_rows(np.asarray(a, dtype=np.float64).reshape(k, -1))
    qb = orthonormal_rows(np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1))
    r = qb - (qb @ qa.T) @ qa
    return float(np.linalg.svd(r, compute_uv=False)[0])


def tangent_matrix(model, spectrum0, steps):
    """T as a dense real matrix [nx ny, nx ny], column by column from the tangent model: column j is the tangent of the unit field e_j"""
    n = model.nx * model.ny
    t = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        model.set_spectrum(spectrum0)
        model.set_tangent(e.reshape(model.nx, model.ny))
        model.step(steps)
        t[:, j] = np.asarray(model.tangent(), dtype=np.float64).ravel()
        e[j] = 0.0
    model.set_spectrum(spectrum0)
    return t


# ---- the case of the GPU test (tests/test_gpu_adjoints.py): adjoint_numpy's singular-value case with a subspace of SV_K ----
SV_N, SV_STEPS, SV_ITERS, SV_BAR = A.SV_N, A.SV_STEPS, A.SV_ITERS, A.SV_BAR
SV_K = 4
SV_SEED = A.SEED + 7
# the sine of the largest principal angle between the final subspaces of the float32 restatement (Float32Model on the CPU) and of
# float64, from the same start: measured on the CPU, asserted in tests/test_adjoints_cpu.py as an upper bound (to 1.5, for another FFT
# library's summation order); the GPU's bar is 4 x this figure, the margin of adjoint_numpy.DOT_BAR for the GPU's other summation order
SV_ANGLE_F32 = 2.56e-07
SV_ANGLE_BAR = 4 * SV_ANGLE_F32
# the float32 restatement's largest relative error of a sigma over the iterations of the case (measured with the angle; SV_BAR holds it)
SV_SIGMA_F32 = 3.3e-07

# ---- the dense check (tests/test_adjoints_cpu.py): a grid small enough for T as a matrix ----
# 32^2, 4 steps of 20 s from the path matrix's inputs: sigma_1..5 = 19.40, 18.97, 18.49, 17.25, 13.74, so k = 4 has the gap
# sigma_4 / sigma_5 = 1.256 and the iteration settles to 1e-12 in 30 iterations (measured; the cap is 200)
DENSE_N, DENSE_DT, DENSE_STEPS, DENSE_K, DENSE_CAP = 32, 20.0, 4, 4, 200
DENSE_SEED = 5


def dense_model():
    v = A.adjoint_inputs(DENSE_N, DENSE_N, A.PATH_CASES[0].vort_noise)[0]
    m = A.AdjointModel64(DENSE_N, DENSE_N, nu=A.G.NU, dt=DENSE_DT)
    m.set_vort(v)
    return m


def sv_start(n=SV_N, k=SV_K):
    """the start vectors of the case, float32 [k, n, n]: white noise, never dealiased"""
    return np.random.default_rng(SV_SEED).standard_normal((k, n, n)).astype(np.float32)


def sv_inputs():
    """(vort, source, start) of the case, float32"""
    v, _, s, _ = A.adjoint_inputs(SV_N, SV_N, A.case_of(SV_N, SV_N).vort_noise)
    return v, s, sv_start()


def sv_reference(cls=None):
    """(sigma [SV_ITERS, SV_K], V [SV_K, n, n]) of the case in float64, or with cls=Float32Model in the float32 restatement"""
    v, s, start = sv_inputs()
    ref = A.AdjointModel64(SV_N, SV_N, nu=A.G.NU, dt=A.T.recipe_dt(SV_N, SV_N))
    ref.set_vort(v)
    ref.src = s.astype(np.float64)
    if cls is None:
        return singular_vectors(ref, ref.spectrum(), SV_STEPS, SV_K, SV_ITERS, start)
    f = cls(ref, s)
    f.set_vort(v)
    return singular_vectors(f, f.spectrum(), SV_STEPS, SV_K, SV_ITERS, start)
