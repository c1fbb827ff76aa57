"""The tangent-linear model on the GPU (fb_model_set_tangent; kernels csrc/fb_tracer.h, csrc/fb_tangent.h) against the float64 reference of the coupled
system (tests/tangent_numpy.py), on every kernel path of the engine.

The inputs of the path matrix are tangent_numpy.tangent_inputs: the elliptic vortex and a perturbation, each with white noise that was
never dealiased, and a vorticity source.  So both fields carry state in every mode outside the dealiasing circle, where the kernels
have logic of their own (k_tracer_vstate_* and k_advect_deriv pick the base or the stage array per mode, k_beside_update leaves a
masked mode alone and runs on the active column tiles only), and the source must reach the velocity and not the perturbation.
tangent_numpy.PATH_CASES holds one row per grid class, with the probe shifts and the float32 figure that make the parity bar of 1e-5
decisive (asserted on the CPU in tests/test_tangent_cpu.py, stored in the fixture for the slow cases).  One line of figures per case
(pytest -s); DESIGN.md, "Tangent-linear model", has the tables."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tangent_numpy as G                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2                                    # noqa: E402

CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in G.PATH_CASES]
EPS32 = float(np.finfo(np.float32).eps)


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny, vort_noise):
    out = G.tangent_inputs(nx, ny, vort_noise)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _live_reference(nx, ny):
    """(perturbation, vort) of the float64 run of a case that is computed here, once"""
    case = [k for k in G.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]
    r = G.recipe_model(nx, ny, *_inputs(nx, ny, case.vort_noise))
    r.step(case.steps)
    out = (r.tangent(), r.vort())
    for a in out:
        a.setflags(write=False)
    return out


def _gpu_model(nx, ny, vort, dz, source, nu=G.NU, dt=None):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, nu=nu, dt=T.recipe_dt(nx, ny) if dt is None else dt)
    m.set_vort(vort)
    if source is not None:
        m.set_source(source)
    if dz is not None:
        m.set_tangent(dz)
    return m


# ---- 1. the path matrix ----
@pytest.mark.parametrize("case", G.PATH_CASES, ids=CASE_IDS)
def test_path_against_float64(case):
    """set_vort, set_source, set_tangent on the noisy inputs; tangent() at step 0 reproduces the input to 1e-6; after case.steps steps
    the perturbation is within 1e-5 relative L2 of TangentModel64 and within 4 times the vorticity's own error against the same run,
    and the vorticity within 1e-5.  The cases with a fixture (16384 x 64, 128 x 16384, 4096^2) compare every sub-th point and the
    full-field L2 norms, to 1e-5 as well, rebuild the inputs from the stored seed, and assert the stored probe shifts >= 1e-4."""
    nx, ny = case.nx, case.ny
    if case.fixture:
        F = np.load(os.path.join(HERE, "golden", "tangent_%dx%d_step%d.npz" % (nx, ny, case.steps)))
        assert (int(F["seed"]), float(F["vort_noise"]), int(F["steps"])) == (G.SEED, case.vort_noise, case.steps)
        assert (float(F["dt"]), float(F["nu"])) == (T.recipe_dt(nx, ny), G.NU)
        assert float(F["shift_vort"]) >= G.SHIFT_BAR and float(F["shift_tangent"]) >= G.SHIFT_BAR and float(F["f32_tangent"]) <= G.F32_BAR
    v0, d0, src = _inputs(nx, ny, case.vort_noise)
    m = _gpu_model(nx, ny, v0, d0, src)
    e0 = rel_l2(_np(m.tangent()), d0)
    m.step(case.steps)
    gt, gv = m.tangent(), m.vort()
    m.close()
    if case.fixture:
        sx, sy = (int(k) for k in F["sub"])
        et, ev = rel_l2(_np(gt[::sx, ::sy]), F["tangent_sub"]), rel_l2(_np(gv[::sx, ::sy]), F["vort_sub"])
        nt = abs(float(gt.double().pow(2).sum().sqrt()) / float(F["tangent_l2"]) - 1)
        nv = abs(float(gv.double().pow(2).sum().sqrt()) / float(F["vort_l2"]) - 1)
    else:
        rt, rv = _live_reference(nx, ny)
        et, ev = rel_l2(_np(gt), rt), rel_l2(_np(gv), rv)
        nt = nv = 0.0
    print("path %dx%d (%s), noise %g, %d steps: perturbation rel L2 = %.3g, vorticity rel L2 = %.3g, step 0 %.3g, norms off by %.2g / %.2g; "
          "probe shifts %.3g / %.3g, float32 on the CPU %.3g" % (nx, ny, case.what, case.vort_noise, case.steps, et, ev, e0, nt, nv, case.shift_vort, case.shift_tangent, case.f32))
    assert e0 <= 1e-6
    assert et <= 1e-5
    assert et <= 4 * ev
    assert ev <= 1e-5
    assert nt <= 1e-5 and nv <= 1e-5


# ---- 2. the step is untouched ----
@pytest.mark.parametrize("nx,ny", [(256, 256), (64, 4096)])
def test_vorticity_is_bit_equal_with_and_without_a_tangent(nx, ny):
    case = [k for k in G.PATH_CASES if (k.nx, k.ny) == (nx, ny)][0]
    v0, d0, src = _inputs(nx, ny, case.vort_noise)
    out = []
    for dz in (None, d0):
        m = _gpu_model(nx, ny, v0, dz, src)
        m.step(case.steps)
        out.append(_np(m.vort()))
        m.close()
    assert _same32(out[0], out[1])
    assert rel_l2(out[0], v0) > 1e-6


# ---- 3. linearity ----
def test_linearity_on_the_gpu():
    """two runs with d and 2 d differ by the factor 2 to <= 1e-6 relative L2 (a scaling by 2 is exact in float32 short of underflow)"""
    case = G.PATH_CASES[0]
    v0, d0, src = _inputs(case.nx, case.ny, case.vort_noise)
    out = []
    for a in (1.0, 2.0):
        m = _gpu_model(case.nx, case.ny, v0, (a * d0).astype(np.float32), src)
        m.step(case.steps)
        out.append(_np(m.tangent()).astype(np.float64))
        m.close()
    err = rel_l2(out[1], 2 * out[0])
    print("linearity on the GPU, %dx%d, %d steps: rel L2 (T(2 d), 2 T(d)) = %.3g" % (case.nx, case.ny, case.steps, err))
    assert err <= 1e-6
    assert rel_l2(out[0], d0) > 1e-4


# ---- 4. the translation mode ----
def test_translation_mode():
    """the noise-free elliptic vortex at 256^2, no source, dz_0 = gradx(zeta_0): after TRANSLATION_STEPS steps dz = gradx(zeta), formed
    by fb_gradx of the spectrum of vort(), to max(1e-5, 10 times the float64 residual that tests/test_tangent_cpu.py measures)"""
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("elliptic", n)
    m = X.Model(n, n)
    m.set_vort(v0)
    f = m.fop

    def gradx_of_vort():
        return f.c2r(f.gradx(f.r2c(m.vort())), normalize=True)
    d0 = gradx_of_vort()
    m.set_tangent(d0)
    m.step(G.TRANSLATION_STEPS)
    want, got = _np(gradx_of_vort()), _np(m.tangent())
    m.close()
    err, bar = rel_l2(got, want), max(1e-5, 10 * G.TRANSLATION_RESIDUAL)
    print("translation mode on the GPU, 256^2, %d steps: rel L2 = %.3g (bar %.3g; float64 residual %.3g)" % (G.TRANSLATION_STEPS, err, bar, G.TRANSLATION_RESIDUAL))
    assert err <= bar
    assert rel_l2(want, _np(d0)) > bar


# ---- 5. norms, rescaling, the Lyapunov helper ----
def test_norms_against_float64_and_rescaling():
    """tangent_norm of both kinds agrees with float64 numpy on the noisy perturbation to 1e-6, returns the same bits when called twice,
    and rescale_tangent(a) scales it by a^2 (to float32 rounding of the scaled spectrum: 4 eps)"""
    case = G.PATH_CASES[3]                                       # 1024 x 64: several workgroups, a strip
    nx, ny = case.nx, case.ny
    v0, d0, _ = _inputs(nx, ny, case.vort_noise)
    ref = G.TangentModel64(nx, ny)
    ref.set_tangent(d0)
    m = _gpu_model(nx, ny, v0, d0, None)
    for kind in ("enstrophy", "energy"):
        a, b, want = m.tangent_norm(kind), m.tangent_norm(kind), ref.tangent_norm(kind)
        print("tangent_norm(%s) %dx%d: %.17g, float64 numpy %.17g, off by %.3g" % (kind, nx, ny, a, want, abs(a / want - 1)))
        assert a == b
        assert abs(a / want - 1) <= 1e-6
    assert abs(m.tangent_norm("enstrophy") / (0.5 * np.mean(d0.astype(np.float64) ** 2)) - 1) <= 1e-6     # (Parseval)
    before = {k: m.tangent_norm(k) for k in ("enstrophy", "energy")}
    m.rescale_tangent(-1.75)
    for k, v in before.items():
        assert abs(m.tangent_norm(k) / (1.75 ** 2 * v) - 1) <= 4 * EPS32
    assert rel_l2(_np(m.tangent()), -1.75 * d0.astype(np.float64)) <= 1e-6
    m.step(2)                                                   # the stage and accumulator arrays hold no live data between steps
    assert np.isfinite(_np(m.tangent())).all()
    m.close()


def test_lyapunov_of_a_single_mode_in_a_fluid_at_rest():
    """zeta = 0, dz = A cos cos of wavenumber k, nu = 1e4: lyapunov() returns ln R(-nu k^2 dt) / dt = -nu k^2 (the RK4 factor's own
    truncation, z^5 / 120, is 1e-14 here) and the per-interval growth factors R^25.  The bar: every step rounds the mode a few times to
    float32, so the log of the amplitude after n steps is off by at most about 4 n eps, against a total of n z."""
    import xlab_fftbarotropic_amd as X
    n, nu, dt, steps, every = 256, 1.0e4, 3.0, 100, 25
    psi, _, k2 = T.cellular_flow(n, n, amp=1.0e-6, mx=20, my=30)
    z = -nu * k2 * dt
    m = X.Model(n, n, nu=nu, dt=dt)
    m.set_vort(np.zeros((n, n), np.float32))
    m.set_tangent(psi.astype(np.float32))
    n0 = m.tangent_norm()
    lam, factors = m.lyapunov(steps, every)
    n1 = m.tangent_norm()
    m.close()
    want = float(np.log(T.rk4_factor(z))) / dt
    bar = 4 * EPS32 / abs(z) + 1e-6                              # (+ the float32 wavenumber tables against the analytic k^2)
    print("lyapunov, 256^2, z = %.4g per step: %.8g s^-1, -nu k^2 = %.8g, ln R / dt = %.8g; off by %.3g (bar %.3g); factors %s"
          % (z, lam, -nu * k2, want, abs(lam / want - 1), bar, factors))
    assert abs(lam / want - 1) <= bar and abs(lam / (-nu * k2) - 1) <= bar
    assert len(factors) == steps // every
    for g in factors:
        assert abs(g / T.rk4_factor(z) ** every - 1) <= every * 4 * EPS32 + 1e-6
    assert abs(n1 / n0 - 1) <= 8 * EPS32                        # rescaled to the norm it had at the call


# ---- 6. combinations and refusals ----
def test_tracer_particles_and_tangent_together_match_each_alone():
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    n, steps = 256, 4
    v0, d0, src = _inputs(n, n, G.PATH_CASES[0].vort_noise)
    c0 = T.noisy_inputs(n, n, G.PATH_CASES[0].vort_noise)[1]
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, 64, seed=5)

    def run(tracer, particles, tangent):
        m = X.Model(n, n, nu=G.NU, dt=3.0)
        m.set_vort(v0)
        m.set_source(src)
        if tracer:
            m.set_tracer(c0, kappa=T.RECIPE_KAPPA)
        if particles:
            m.set_particles(x0)
        if tangent:
            m.set_tangent(d0)
        m.step(steps)
        out = (_np(m.vort()), _np(m.tracer()) if tracer else None, _np(m.particles()) if particles else None, _np(m.tangent()) if tangent else None)
        m.close()
        return out
    allv, allc, allp, alld = run(True, True, True)
    assert _same32(allv, run(False, False, False)[0])
    assert _same32(allc, run(True, False, False)[1])
    assert np.array_equal(allp.view(np.uint64), run(False, True, False)[2].view(np.uint64))
    assert _same32(alld, run(False, False, True)[3])
    assert rel_l2(alld, d0) > 1e-4


def test_removal_and_refusals():
    import xlab_fftbarotropic_amd as X
    n = 256
    v0, d0, _ = _inputs(n, n, G.PATH_CASES[0].vort_noise)
    m = _gpu_model(n, n, v0, None, None)
    for call in (m.tangent, m.tangent_norm, lambda: m.rescale_tangent(2.0)):
        with pytest.raises(X.FftBaroError, match="no tangent is set"):
            call()
    m.set_tangent(d0)
    m.step(2)
    for a in (0.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(X.FftBaroError, match="finite and not zero"):
            m.rescale_tangent(a)
    for kind in (2, -1):
        with pytest.raises(X.FftBaroError, match="kind"):
            m.tangent_norm(kind)
    with pytest.raises(ValueError):
        m.tangent_norm("palinstrophy")
    with_tangent = _np(m.vort())
    m.set_tangent(None)
    with pytest.raises(X.FftBaroError, match="no tangent is set"):
        m.tangent()
    m.step(2)                                                   # stepping goes on
    m.close()
    ref = _gpu_model(n, n, v0, None, None)
    ref.step(2)
    assert _same32(with_tangent, _np(ref.vort()))
    ref.close()


def test_slab_of_one_rank_matches_the_model():
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n, steps = 256, 3
    v0, d0, _ = _inputs(n, n, G.PATH_CASES[0].vort_noise)
    m = X.Model(n, n, nu=G.NU, dt=3.0)
    m.set_vort(v0)
    m.set_tangent(d0)
    m.step(steps)
    want, wn = _np(m.tangent()), m.tangent_norm("energy")
    m.close()
    s = S.EngineSlab(n, n, nu=G.NU, dt=3.0)
    s.set_vort_local(v0)
    s.set_tangent(d0)
    s.step(steps)
    assert _same32(_np(s.tangent()), want)
    assert s.tangent_norm("energy") == wn
    s.rescale_tangent(0.5)
    assert abs(s.tangent_norm("energy") / (0.25 * wn) - 1) <= 4 * EPS32
    s.set_tangent(None)
    with pytest.raises(X.FftBaroError):
        s.tangent()
    s.close()


def test_slab_of_one_rank_lyapunov_matches_the_model():
    """EngineSlab.lyapunov on one rank at 64^2 against Model.lyapunov.  The bar is the one the test above holds the slab's norm to
    against the model's, 4 eps32 relative: a growth factor is the root of a ratio of two norms, and the exponent the sum over the
    intervals of half the log of such ratios."""
    import xlab_fftbarotropic_amd as X
    S = _slab()
    n, steps, every = 64, 6, 2
    v0, d0, _ = _inputs(n, n, G.PATH_CASES[0].vort_noise)
    out = []
    for m in (X.Model(n, n, nu=G.NU, dt=3.0), S.EngineSlab(n, n, nu=G.NU, dt=3.0)):
        (m.set_vort if isinstance(m, X.Model) else m.set_vort_local)(v0)
        m.set_tangent(d0)
        lam, factors = m.lyapunov(steps, every)
        out.append((lam, factors, _np(m.tangent())))
        m.close()
    (lm, fm, tm), (ls, fs, ts) = out
    assert isinstance(ls, float) and np.isfinite(ls) and len(fs) == steps // every and all(isinstance(g, float) and np.isfinite(g) for g in fs)
    assert ts.shape == (n, n) and ts.dtype == np.float32 and np.isfinite(ts).all()
    print("lyapunov 64^2 on one rank: slab %.9g s^-1, model %.9g s^-1, factors %s against %s" % (ls, lm, fs, fm))
    for a, b in zip(fs, fm):
        assert abs(a / b - 1) <= 4 * EPS32
    assert abs(ls - lm) * steps * 3.0 <= len(fm) * 4 * EPS32
    assert rel_l2(ts, tm) <= 4 * EPS32


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every tangent entry point raises with the engine's message"""
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
                calls = (lambda: s.set_tangent(np.zeros((s.XL, n), np.float32)), lambda: s.set_tangent(None), s.tangent, s.tangent_norm,
                         lambda: s.rescale_tangent(2.0))
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
        assert len(msgs[r]) == 5
        for msg in msgs[r]:
            assert msg is not None and "invalid argument" in msg.lower() and "not supported" in msg and "world > 1" in msg, msg


# ---- 7. the driver ----
def _run_driver(d, n, v0, dz, extra, steps=21):
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    np.ascontiguousarray(dz, dtype="<f4").tofile(str(d / "input" / "dz.bin"))
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--record-step", "10", "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode(), (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_tangent(tmp_path):
    """barotropic_main.out --tangent dz.bin --tangent-renorm 5 at 256^2, 20 steps, a record every 10: tangent_step_N.bin and
    tangent_growth_step_N.bin are the last two files of each record in ./log and equal what the Python path gives with the same
    renormalisations, bit for bit; --world 2 --tangent ends with exit status 2 and one line on stderr."""
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, every = 256, 5
    v0 = X.make_field("kuo2004", n)
    d0 = _inputs(n, n, G.PATH_CASES[0].vort_noise)[1]
    rc, err, log = _run_driver(tmp_path / "run", n, v0, d0, ["--tangent", "dz.bin", "--tangent-renorm", str(every)])
    assert rc == 0, err
    names = ("vort_src_input", "vort", "psi", "u", "v", "tangent", "tangent_growth")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 10, 20) for name in names]
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_tangent(d0)
    n0 = ref = m.tangent_norm()
    total = 0.0
    for s in range(21):
        if s % 10 == 0:
            out = tmp_path / "run" / "output"
            assert _same32(np.fromfile(str(out / ("tangent_step_%d.bin" % s)), dtype="<f4").reshape(n, n), _np(m.tangent())), s
            assert _same32(np.fromfile(str(out / ("vort_step_%d.bin" % s)), dtype="<f4").reshape(n, n), _np(m.vort())), s
            g = np.fromfile(str(out / ("tangent_growth_step_%d.bin" % s)), dtype="<f8")
            now = m.tangent_norm()
            want = np.array([s * 3.0, now, total + 0.5 * np.log(now / ref)])
            print("driver, step %d: time, norm, sum of ln(growth) = %s" % (s, g))
            assert g.shape == (3,) and g[0] == want[0] and g[1] == want[1] and abs(g[2] - want[2]) <= 1e-12
        m.step(1)
        if (s + 1) % every == 0:
            now = m.tangent_norm()
            total += 0.5 * np.log(now / ref)
            m.rescale_tangent(float(np.float32(np.sqrt(n0 / now))))
            ref = m.tangent_norm()
    m.close()
    rc, err, _ = _run_driver(tmp_path / "world", n, v0, d0, ["--tangent", "dz.bin", "--world", "2", "--ranks-as-threads"], steps=1)
    assert rc == 2, (rc, err)
    assert len(err.strip().splitlines()) == 1 and "--tangent" in err, err
