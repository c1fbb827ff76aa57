"""CPU checks of the split stage (stochastic ring forcing, linear drag, hyperviscosity): the float64 restatement tests/forcing_numpy.py
against the known answers of Philox4x32-10 and against what the stage is meant to do (a real field, eps dt of energy per stage,
N_ring, the exact decay of a single mode); the probe condition on the inputs of the GPU path matrix (tests/test_gpu_forcing.py); and
the entry points declared, exported, bound, with the argument checks that run before any HIP call.  No GPU needed."""
import ctypes
import functools
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import forcing_numpy as F                                       # noqa: E402
import tangent_numpy as G                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

FB_EINVAL = 1
CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in F.PATH_CASES]


def test_philox_known_answers():
    for counter, key, want in F.PHILOX_KNOWN:
        assert tuple(int(x) for x in F.philox4x32(counter, key)) == want
    # vectorised over the counter: the same words as one call per counter
    i = np.arange(5)
    many = F.philox4x32((i, 7, 3, 1), (11, 13))
    for a in range(5):
        assert [int(w[a]) for w in many] == [int(x) for x in F.philox4x32((a, 7, 3, 1), (11, 13))]


@pytest.mark.parametrize("nx,ny,k,width", [(64, 64, 12.0, 1.5), (1024, 64, 33.0, 2.0), (64, 4096, 33.0, 2.0)])
def test_increment_is_hermitian_on_the_two_real_lines(nx, ny, k, width):
    """on j = 0 and j = ny/2 mode (nx - i, j) is the conjugate of mode (i, j), bit for bit, and the self-conjugate modes are zero: the
    inverse transform of Delta_n alone is a real field whose spectrum is Delta_n again"""
    f = F.Forcing(nx, ny, 3.0, rate=1.0, k=k * F.K1, width=width * F.K1, seed=F.SEED)
    lines = [0] + ([ny // 2] if f.ring[:, ny // 2].any() else [])
    assert f.ring[:, 0].any() and ((nx, ny) != (1024, 64) or len(lines) == 2)        # the strip's ring reaches the live Nyquist column
    for n in (0, 1, 2 ** 32 + 5):
        d = f.increment(n)
        assert np.array_equal(d != 0, f.ring)
        for j in lines:
            assert np.array_equal(d[1:nx // 2, j], np.conj(d[:nx // 2:-1, j]))
            assert d[0, j] == 0 and d[nx // 2, j] == 0
        back = np.fft.rfft2(np.fft.irfft2(d, s=(nx, ny)))
        assert np.abs(back - d).max() <= 1e-12 * np.abs(d).max()
    assert not np.array_equal(f.increment(0), f.increment(1)) and not np.array_equal(f.increment(5), f.increment(2 ** 32 + 5))
    other = F.Forcing(nx, ny, 3.0, rate=1.0, k=k * F.K1, width=width * F.K1, seed=F.SEED + 1)
    assert not np.array_equal(f.increment(0), other.increment(0))


@pytest.mark.parametrize("nx,ny,k,width", [(64, 64, 12.0, 1.5), (192, 192, 33.0, 2.0), (4096, 64, 33.0, 2.0)])
def test_one_stage_from_rest_adds_rate_times_dt(nx, ny, k, width):
    rate, dt = 0.37, 3.0
    f = F.Forcing(nx, ny, dt, rate=rate, k=k * F.K1, width=width * F.K1, seed=5)
    for n in (0, 9):
        assert abs(f.energy(f.increment(n, round32=False)) / (rate * dt) - 1) <= 1e-12
        assert abs(f.energy(f.increment(n)) / (rate * dt) - 1) <= 1e-7                  # the float32 values the engine adds
    m = F.ForcedModel64(nx, ny, nu=0.0, dt=dt, rate=rate, k=k * F.K1, width=width * F.K1, seed=5)
    m.set_vort(np.zeros((nx, ny)))
    m.step(1)
    b = m.budget()
    assert abs(b["dE_forc"] / (rate * dt) - 1) <= 1e-7 and b["dE_diss"] == 0.0 and b["dZ_diss"] == 0.0 and b["clock"] == 1
    assert abs(b["dZ_forc"] / f.enstrophy(f.increment(0)) - 1) <= 1e-12


def test_n_ring_is_the_count_over_the_full_spectrum():
    nx = ny = 64
    k, width = 12.0 * F.K1, 1.5 * F.K1
    f = F.Forcing(nx, ny, 3.0, rate=1.0, k=k, width=width)
    count = 0
    for i in range(nx):
        for jj in range(ny):
            j = jj if jj <= ny // 2 else ny - jj                # K^2 of the full spectrum's mode from the stored half's table
            ii = i if jj <= ny // 2 else (nx - i) % nx
            if ii in (0, nx // 2) and j in (0, ny // 2):
                continue
            count += abs(np.sqrt(f.K2[ii, j]) - k) <= width
    assert f.n_ring == count > 0
    for bad in (dict(k=40.0 * F.K1, width=F.K1), dict(k=12.3 * F.K1, width=1e-3 * F.K1), dict(k=F.K1, width=F.K1)):
        with pytest.raises(ValueError):                         # a masked mode in the ring; an empty ring; k - width <= 0
            F.Forcing(nx, ny, 3.0, rate=1.0, **bad)


def test_a_single_mode_decays_by_D_per_step():
    """psi = A cos cos has J(psi, zeta) = 0; with nu = 0, drag and nabla^8 hyperviscosity its amplitude after n steps is D^n"""
    nx, ny, dt, steps = 128, 64, 3.0, 7
    psi, zeta, k2 = T.cellular_flow(nx, ny, mx=5, my=7)
    nu_p = 0.05 / (dt * F.Forcing(nx, ny, dt).K2[5, 7] ** 4)      # the hyperviscosity takes 5 % per step off this mode, the drag 0.9 %
    m = F.ForcedModel64(nx, ny, nu=0.0, dt=dt, drag=3e-3, hyper_nu=nu_p, hyper_order=4)
    m.set_vort(zeta)
    m.step(steps)
    D = m.f.D[5, 7]
    assert 0.5 < D < 0.999 and abs(-np.log(D) / ((3e-3 + nu_p * m.f.K2[5, 7] ** 4) * dt) - 1) <= 1e-6
    assert rel_l2(m.vort(), zeta * D ** steps) <= 1e-12
    b = m.budget()
    e0 = m.f.energy(np.fft.rfft2(zeta))
    assert abs(b["dE_diss"] / (e0 * (D ** (2 * steps) - 1)) - 1) <= 1e-10 and b["dE_forc"] == 0.0 and b["n_ring"] == 0


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    return G.tangent_inputs(nx, ny, 3e-2)


@pytest.mark.parametrize("case", F.PATH_CASES, ids=CASE_IDS)
def test_probe_condition_of_the_gpu_matrix(case):
    """A forcing without the conjugate rule on the two real lines, and a forcing whose clock stays at 0, each move the float64
    vorticity of the matrix's run by at least 1e-4 relative L2, ten times the GPU test's bar; the stored shifts are the measured ones"""
    v, _, src = _inputs(case.nx, case.ny)
    ref = F.recipe_model(case, v, None, src)
    ref.step(case.steps)
    conj, clock = F.probe_shifts(case, v, src, ref)
    print("%dx%d: N_ring = %d, shift without the conjugate rule %.3g, with a frozen clock %.3g (stored %.3g, %.3g)"
          % (case.nx, case.ny, ref.f.n_ring, conj, clock, case.shift_conj, case.shift_clock))
    assert min(conj, clock, case.shift_conj, case.shift_clock) >= F.SHIFT_BAR
    assert abs(conj / case.shift_conj - 1) <= 0.02 and abs(clock / case.shift_clock - 1) <= 0.02
    assert ref.f.ring[:, 0].any() and (case.ny != 64 or ref.f.ring[:, case.ny // 2].any())
    assert not (ref.f.ring & ~ref.f.live).any()


def test_tangent_of_the_split_system_is_linear_and_decays():
    """the perturbation of ForcedModel64 is the derivative of the forced run with respect to its initial state: the increments are the
    same in both runs, so they cancel"""
    nx = ny = 64
    case = F.ForcingCase(nx, ny, 3, 0.5, 12.0 * F.K1, 1.5 * F.K1, 0.0, 0.0)
    v, dz, _ = G.tangent_inputs(nx, ny, 3e-2)
    v, dz = v.astype(np.float64), dz.astype(np.float64)
    a = F.recipe_model(case, v, dz, None)
    a.step(case.steps)
    res = []
    for eps in (1e-2, 1e-3):
        b = F.recipe_model(case, v + eps * dz, None, None)
        b.step(case.steps)
        res.append(rel_l2((b.vort() - a.vort()) / eps, a.tangent()))
    assert res[1] < res[0] / 5 and res[1] < 1e-3


NAMES = [p + n for p in ("fb_model_", "fb_slab_") for n in ("set_forcing", "forcing_budget", "forcing_increment")]


def test_entry_points_are_declared_exported_and_bound():
    from importlib import import_module
    import xlab_fftbarotropic_amd as X
    B = import_module("xlab-fftbarotropic_amd.binding")
    header = open(os.path.join(ROOT, "include", "fftbaro.h")).read()
    L = X.lib()
    for name in NAMES:
        assert name + "(" in header and hasattr(L, name) and name in B.SIGNATURES
    assert sorted(B._FORCING_PAIRS) == ["forcing_budget", "forcing_increment", "set_forcing"] and not set(B._FORCING_PAIRS) & set(B._PAIRS)
    sig = inspect.signature(B.ModelSurface.set_forcing)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("rate", 0.0), ("k", None), ("width", None), ("seed", 0), ("drag", 0.0), ("hyper_nu", 0.0), ("hyper_order", 1)]
    slab = import_module("xlab-fftbarotropic_amd.slab")
    for cls in (B.Model, slab.EngineSlab):
        for meth in ("set_forcing", "forcing_budget", "forcing_increment"):
            assert getattr(cls, meth) is getattr(B.ModelSurface, meth)


def test_argument_errors_are_rejected_without_a_device():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    nan, inf = float("nan"), float("inf")
    good = dict(rate=1.0, k=1e-4, dk=1e-5, seed=1, mu=0.0, nu_p=0.0, p=1)
    bad = [("rate", -1.0, b"rate"), ("rate", nan, b"rate"), ("rate", inf, b"rate"), ("mu", -1e-3, b"mu"), ("mu", nan, b"mu"), ("nu_p", -1.0, b"nu_p"),
           ("nu_p", inf, b"nu_p"), ("p", 0, b"p outside"), ("p", 9, b"p outside"), ("k", nan, b"k_f"), ("k", -1e-4, b"k_f"), ("dk", inf, b"k_f"),
           ("dk", 1e-4, b"NULL"), ("dk", 2e-4, b"NULL")]          # (k_f - dk <= 0 is refused with the ring: after the handle)
    for fn, name in ((L.fb_model_set_forcing, b"fb_model_set_forcing"), (L.fb_slab_set_forcing, b"fb_slab_set_forcing")):
        for key, value, word in bad:
            a = dict(good, **{key: value})
            assert fn(None, a["rate"], a["k"], a["dk"], a["seed"], a["mu"], a["nu_p"], a["p"]) == FB_EINVAL, (key, value)
            msg = L.fb_last_error()
            assert msg.startswith(name + b": ") and word in msg, msg
        a = good
        assert fn(None, a["rate"], a["k"], a["dk"], a["seed"], a["mu"], a["nu_p"], a["p"]) == FB_EINVAL
        assert L.fb_last_error().startswith(name + b": NULL ")
        assert fn(None, 0.0, nan, nan, 0, 1e-3, 0.0, 1) == FB_EINVAL and b"NULL" in L.fb_last_error()      # no ring needed: k_f, dk not read
    out = (ctypes.c_double * 6)()
    for fn, name in ((L.fb_model_forcing_budget, b"fb_model_forcing_budget"), (L.fb_slab_forcing_budget, b"fb_slab_forcing_budget")):
        assert fn(None, None) == FB_EINVAL and L.fb_last_error().startswith(name + b": NULL output")
        assert fn(None, out) == FB_EINVAL and L.fb_last_error().startswith(name + b": NULL ")
    w = ctypes.cast((ctypes.c_float * 4)(), ctypes.c_void_p)
    for fn, name in ((L.fb_model_forcing_increment, b"fb_model_forcing_increment"), (L.fb_slab_forcing_increment, b"fb_slab_forcing_increment")):
        assert fn(None, 0, None) == FB_EINVAL and L.fb_last_error().startswith(name + b": NULL output")
        assert fn(None, 0, w) == FB_EINVAL and L.fb_last_error().startswith(name + b": NULL ")
