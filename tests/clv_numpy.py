"""float64 numpy reference of the covariant Lyapunov vectors: Ginelli's algorithm on lyapunov_numpy.SubspaceModel64 with modified
Gram-Schmidt (mgs), keeping the bases Q_n, the factors R_n and the base state of every window slot; the float32-storage restatement of
what the engine does to its float32 half spectra (mgs_f32, combine_f32, bases rounded to complex64 after every step); the recursion
written a second time (coefficients: numpy's general solver in the place of the product's back substitution); the covariance defect
that the tests are tied to; and the bars of the GPU's comparison with the float64 run (F32_*: measured on the CPU by
tests/test_clv_cpu.py, which asserts that they hold; written here before the GPU ran).

Indices: T Q_(n-1) = Q_n R_n over window interval n = 1 .. K (R[n - 1] in arrays), slot n holds Q_n and the base state at its time;
C_(n-1) = R_n^-1 C_n D_n; V_n = Q_n C_n; log_growth[n - 1, j] = ln of the growth of vector j over interval n.  Perturbations are half
spectra (unnormalised, as rfft2 leaves them).  Used ONLY by tests."""
from types import SimpleNamespace

import numpy as np

import lyapunov_numpy as Y
import tangent_numpy as G
import tracer_numpy as T

# the recipe of the covariance tests, CPU and GPU: subspace_inputs at 64^2 (M = 3), 5 steps per interval, 4 window + 4 settle intervals
N, EVERY, WINDOW, SETTLE = 64, 5, 4, 4

# The engine against the float64 Ginelli run, same recipe and same C_end: the largest figure over both kinds between `ginelli` in
# float64 and its float32-storage restatement (f32=True), measured on the CPU (tests/test_clv_cpu.py prints every figure and asserts
# that none exceeds these): |log_r - log_r64| enstrophy 5.34e-8, energy 2.14e-8; |log_growth - log_growth64| 5.31e-8 and 3.66e-8; the
# sine between a vector and the float64 run's 8.41e-7 and 7.24e-7 (storage rounds by 6e-8; eight intervals of a flow that
# stretches the set carry it further).  The GPU's bars are 4 times these (tests/test_gpu_clv.py): its other summation order.
F32_LOG_R = 5.4e-8
F32_LOG_GROWTH = 5.4e-8
F32_SINE = 8.5e-7


def coefficients(R, C_end):
    """the backward recursion with numpy's general solver: (C [N + 1, M, M], log_growth [N, M])"""
    R = np.asarray(R, dtype=np.float64)
    n, m = R.shape[0], R.shape[1]
    C, lg = np.empty((n + 1, m, m)), np.empty((n, m))
    C[n] = np.asarray(C_end, dtype=np.float64) / np.linalg.norm(C_end, axis=0)
    for k in range(n, 0, -1):
        x = np.linalg.solve(R[k - 1], C[k])
        length = np.linalg.norm(x, axis=0)
        C[k - 1], lg[k - 1] = x / length, -np.log(length)
    return C, lg


def c_end(m=3, seed=0):
    """a random upper triangular matrix with unit columns, its diagonal pushed away from zero"""
    c = np.triu(np.random.default_rng(seed).standard_normal((m, m)))
    c[np.diag_indices(m)] += np.where(np.diagonal(c) < 0, -1.0, 1.0)
    return c / np.linalg.norm(c, axis=0)


def _f64(a):
    return a.view(np.float32).astype(np.float64)                # (re, im interleaved) widened


def combine_f32(Q, C):
    """V_j = sum over i of C[i, j] Q_i as the engine's k_tangent_combine forms it: Q complex64, every element summed in float64 in the
    order of i, rounded once to float32"""
    out = []
    for j in range(len(Q)):
        acc = C[0, j] * _f64(Q[0])
        for i in range(1, len(Q)):
            acc = acc + C[i, j] * _f64(Q[i])
        out.append(acc.astype(np.float32).view(np.complex64))
    return out


def combine(Q, C):
    return [sum(C[i, j] * np.asarray(Q[i], dtype=np.complex128) for i in range(len(Q))) for j in range(len(Q))]


def ginelli(kind="enstrophy", f32=False, C_end=None, n=N, every=EVERY, window=WINDOW, settle=SETTLE, inputs=None, model=None):
    """Ginelli's algorithm on the recipe (or on `model`, a SubspaceModel64 with its state and perturbations set).  f32: the bases are
    stored as complex64 (rounded after every step), orthonormalised by mgs_f32 and combined by combine_f32; the base state and every
    sum stay float64.  Returns a namespace: m (the model, at the end of the run), kind, f32, every, Q [window + 1] lists of M half
    spectra, states [window + 1] (the base state's spectrum per slot), R [window + settle, M, M], C [window + 1, M, M], log_growth
    [window, M], log_r [window + settle, M]."""
    if model is None:
        vort, W, src = inputs if inputs is not None else Y.subspace_inputs(n, n)
        m = Y.SubspaceModel64(n, n, nu=G.NU, dt=T.recipe_dt(n, n))
        m.set_vort(vort)
        m.src = np.asarray(src).astype(np.float64)
        m.set_tangents(W)
    else:
        m = model
    qr = Y.mgs_f32 if f32 else Y.mgs
    m.dcs, _ = qr(m, m.dcs, kind)
    Q, states, R = [list(m.dcs)], [m.vc.copy()], []
    for k in range(window + settle):
        m.dcs = [np.asarray(d, dtype=np.complex128) for d in m.dcs]
        for _ in range(every):
            m.step(1)
            if f32:
                m.dcs = [d.astype(np.complex64).astype(np.complex128) for d in m.dcs]
        m.dcs, r = qr(m, m.dcs, kind)
        R.append(r)
        if k < window:
            Q.append(list(m.dcs))
            states.append(m.vc.copy())
    R = np.array(R)
    C, lg = coefficients(R, c_end(R.shape[1]) if C_end is None else C_end)
    return SimpleNamespace(m=m, kind=kind, f32=f32, every=every, Q=Q, states=states, R=R, C=C[:window + 1], log_growth=lg[:window],
                           log_r=np.log(np.diagonal(R, axis1=1, axis2=2)))


def vectors(run, n, C=None):
    """V_n = Q_n C (C_n unless given): float64 sums, or combine_f32 on a float32-storage run"""
    C = run.C[n] if C is None else C
    return combine_f32(run.Q[n], C) if run.f32 else combine(run.Q[n], C)


def sine(m, a, b, kind):
    """the sine of the angle between two half spectra in the inner product of `kind`: the length of what is left of a / |a| when its
    component along b / |b| is taken out (accurate for small angles, where sqrt(1 - cos^2) is not)"""
    w = Y.weights(m, kind)
    a, b = np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)
    a, b = a / np.sqrt(Y.inner(m, a, a, kind, w)), b / np.sqrt(Y.inner(m, b, b, kind, w))
    r = a - Y.inner(m, a, b, kind, w) * b
    return float(np.sqrt(Y.inner(m, r, r, kind, w)))


def step_from_slot(run, n, V):
    """the set V carried over interval n + 1 from the base state of slot n: (the half spectra after, ln of each one's growth in the
    inner product of the run's kind); the run's model is used and left there"""
    m = run.m
    m.vc = run.states[n].copy()
    m.dcs = [np.asarray(v, dtype=np.complex128) for v in V]
    before = [Y.inner(m, d, d, run.kind) for d in m.dcs]
    m.step(run.every)
    after = [Y.inner(m, d, d, run.kind) for d in m.dcs]
    return list(m.dcs), 0.5 * np.log(np.array(after) / np.array(before))


def covariance_defect(run, n, j, C=None):
    """T V_n against V_(n+1) D, column j: (the sine of the angle between T v_j and column j of V_(n+1), the measured ln growth minus
    log_growth[n, j]).  C: coefficients in the place of C_n (the probes of tests/test_clv_cpu.py)."""
    out, growth = step_from_slot(run, n, vectors(run, n, C))
    return sine(run.m, out[j], vectors(run, n + 1)[j], run.kind), float(growth[j] - run.log_growth[n, j])


# ---- a fluid at rest ----
# zeta = 0: every Fourier mode decays on its own by rk4_factor(nu lap dt) per step.  Three modes inside the dealiasing circle of 64^2
# whose ln r_ii differ by 0.77 and more per interval of REST_EVERY steps (0.4 is what the recursion needs to converge at all within
# REST_SETTLE intervals to the GPU's bar; the CPU's 1e-10 needs e^(-40 d) <= 1e-11: d >= 0.64).  nu keeps |nu k^2 dt| inside RK4's
# stability range of 2.78 for EVERY mode inside the circle at 256^2, 2.43 at its edge (tests/test_clv_cpu.py asserts it): the engine's
# float32 fields have rounding noise in all of them, and one unstable mode would outgrow everything.  The three modes' own
# |nu k^2 dt| are 0.0008, 0.033 and 0.066.
REST_MODES = ((1, 2), (10, 10), (12, 16))                       # mx^2 + my^2 = 5, 200, 400
REST_NU, REST_DT, REST_EVERY, REST_SETTLE = 5.0e5, 3.0, 24, 40


def rest_z(lx=600000.0, ly=600000.0):
    """nu lap dt of the three modes (float64; negative)"""
    return np.array([-REST_NU * REST_DT * ((2 * np.pi * mx / lx) ** 2 + (2 * np.pi * my / ly) ** 2) for mx, my in REST_MODES])


def rest_fields(n):
    """the three modes as real fields [3, n, n] float64, cos(kx x) cos(ky y) of unit amplitude"""
    return np.array([T.cellular_flow(n, n, amp=1.0, mx=mx, my=my)[0] for mx, my in REST_MODES])


def rest_spectra(n):
    """the half spectra of rest_fields with nothing but the modes themselves (rfft2 would leave rounding noise in every other mode, which
    in the masked modes never decays and outgrows a decaying vector that is rescaled at every interval)"""
    out = []
    for mx, my in REST_MODES:
        s = np.zeros((n, n // 2 + 1), dtype=np.complex128)
        s[mx, my] = s[n - mx, my] = n * n / 4.0
        out.append(s)
    return out
