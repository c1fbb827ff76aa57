"""GPU tests of the particles' deformation gradient and its stretching: fb_model_set_particle_deformation /
fb_model_get_particle_deformation / fb_model_particle_stretching (Model.set_particle_deformation, particle_deformation,
particle_deformation_time, particle_stretching, ftle), their slab counterparts and the driver's --particle-deformation.

Checked: positions, vorticity, tracer and tangent bit for bit what they are without; F against the float64 restatement
(tests/deformation_numpy.py, itself checked against finite differences in tests/test_deformation_cpu.py) in a frozen flow on every
kernel path of the particles, in a decaying flow with analytic stage states (the stage order) and in a fully time-dependent flow; the
stretching kernel against numpy.linalg.svd; the life cycle, the refusals and the driver.  The measured figures are printed, one line
per case (pytest -s)."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "xlab-fftbarotropic_amd", "host")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
EPS64 = float(np.finfo(np.float64).eps)
NPART = 1000
FB_EINVAL, FB_EUNSUPPORTED = 1, 5


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _same64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _grad_tol(dv, T, dx, dy, F):
    """The tolerance of F where the two sides' velocity fields differ by at most dv: an entry of A differs by at most
    sum|w'| sum|w| dv / spacing <= 2.34 * 1.25 dv / min(dx, dy) < 4 dv / min(dx, dy), F' = A F, allowed ten times over the elapsed time;
    plus 256 eps64 max|F| for the float64 rounding of F on either side."""
    import deformation_numpy as D
    assert D.DW_SUM * D.W_SUM <= 4.0
    fmax = float(np.max(np.abs(F)))
    return 10.0 * T * 4.0 * dv / min(dx, dy) * fmax + 256 * EPS64 * fmax


# ---- 1. nothing else moves ----
@pytest.mark.parametrize("n", [64, 256])
def test_nothing_else_moves(n):
    """5 steps with a tracer, a tangent and 1000 particles: positions, vorticity, tracer and tangent bit for bit with the deformation
    on and off; F bit for bit between graph replay and eager steps, and between Model and an EngineSlab of one rank."""
    import torch
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    S = _slab()
    v0 = X.make_field("kuo2004", n)
    c0 = np.ascontiguousarray(np.roll(X.make_field("gaussian", n), n // 4, axis=0))
    dz = np.random.default_rng(91).standard_normal((n, n)).astype(np.float32)
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, NPART, seed=91)

    def run(m, on, slab=False):
        (m.set_vort_local if slab else m.set_vort)(v0)
        (m.set_tracer_local if slab else m.set_tracer)(c0, kappa=20.0)
        m.set_tangent(dz)
        m.set_particles(x0)
        if on:
            m.set_particle_deformation()
        m.step(5)
        out = [_np(m.particles()), _np(m.vort_local() if slab else m.vort()), _np(m.tracer_local() if slab else m.tracer()), _np(m.tangent()),
               _np(m.particle_deformation()) if on else None, m.particle_deformation_time() if on else None]
        m.close()
        return out
    off, on = run(X.Model(n, n), False), run(X.Model(n, n), True)
    assert _same64(on[0], off[0]) and not _same64(on[0], x0)
    assert _same32(on[1], off[1]) and _same32(on[2], off[2]) and _same32(on[3], off[3])
    F = on[4]
    assert F.shape == (NPART, 2, 2) and np.isfinite(F).all() and float(np.abs(F - np.eye(2)).max()) > 1e-6
    assert on[5] == 5 * float(np.float32(3.0))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = X.Model(n, n)
        g.fop.use_current_stream()
        g.use_graph(True)
        gr = run(g, True)
    assert _same64(gr[4], F) and _same64(gr[0], on[0]) and gr[5] == on[5]
    sl = run(S.EngineSlab(n, n), True, slab=True)
    assert _same64(sl[4], F) and _same64(sl[0], on[0]) and sl[5] == on[5]


# ---- 2. a frozen flow on every kernel path of the particles ----
FROZEN = [(64, 64), (192, 64), (64, 192), (256, 256), (128, 16384), (16384, 64)]


@pytest.mark.parametrize("nx,ny", FROZEN)
def test_frozen_flow_deformation(nx, ny):
    """The steady cellular flow (nu = 0), as test_gpu_particles.test_frozen_flow_trajectories: the restatement rk4_deformation is driven
    with the diag() fields downloaded before the first step.  4 steps, 1000 seed_positions particles (grid points, first and last
    cells, positions 3 domain lengths away: both sides take the right-hand derivative on a face).
    Tolerance (_grad_tol): dv = the largest change of diag()'s u, v over the run; 10 T 4 dv / min(dx, dy) max|F| + 256 eps64 max|F|.
    Measured on MI355X: DESIGN.md, "Particle deformation and FTLE"."""
    import xlab_fftbarotropic_amd as X
    import deformation_numpy as D
    import particles_numpy as P
    from tracer_numpy import cellular_flow, recipe_dt
    lx = ly = 600000.0
    dt, steps = recipe_dt(nx, ny), 4
    psi, zeta, k2 = cellular_flow(nx, ny, lx, ly)
    m = X.Model(nx, ny, lx, ly, nu=0.0, dt=dt)
    m.set_vort(zeta.astype(np.float32))
    del psi, zeta
    _, u0, v0 = m.diag()
    x0 = P.seed_positions(nx, ny, lx, ly, NPART, seed=21)
    m.set_particles(x0)
    m.set_particle_deformation()
    dv = 0.0
    for _ in range(steps):
        m.step(1)
        _, u, v = m.diag()
        dv = max(dv, float((u - u0).abs().max().item()), float((v - v0).abs().max().item()))
    got, gotx = _np(m.particle_deformation()), _np(m.particles())
    un, vn = _np(u0), _np(v0)
    dtw = float(np.float32(dt))
    wantx, want = D.rk4_deformation(x0, D.identity(NPART), lambda n, s, x: D.sample_uv_grad(un, vn, x, lx, ly), dtw, steps)
    err = float(np.max(np.abs(got - want)))
    tol = _grad_tol(dv, steps * dtw, P.widen(lx) / nx, P.widen(ly) / ny, want)
    dev = float(np.max(np.abs(want - np.eye(2))))
    print("frozen F %dx%d: dv %.3e m/s, max|F - I| %.3e, err %.3e, tol %.3e" % (nx, ny, dv, dev, err, tol))
    assert m.particle_deformation_time() == steps * dtw
    assert dev > 10 * tol                                       # the identity is far outside the tolerance
    assert err <= tol
    assert float(np.max(np.abs(gotx - wantx))) <= 10.0 * dv * steps * dtw + 64 * EPS64 * float(np.max(np.abs(wantx)))
    m.close()


# ---- 3. the order of the stage gradients ----
def test_stage_order():
    """The decaying cellular flow of test_gpu_particles.test_stage_order (64^2, L = 2 pi, z = -0.13 per step, 10 steps): velocity AND
    velocity gradient of stage s of step k are the analytic ones times R^k stage_factors[s].  Reference: rk4_deformation with those.
    Tolerance: 10 x the difference DeformationModel64 shows against that analytic F (its interpolation error, computed here on the
    CPU).  A reference whose gradient is that of the stage-0 state at all four stages (the velocities right) is asserted to FAIL the
    tolerance, against the analytic F and against the GPU."""
    import xlab_fftbarotropic_amd as X
    import deformation_numpy as D
    import particles_numpy as P
    from tracer_numpy import cellular_flow, rk4_factor
    n, steps, amp, mx, my = 64, 10, 2.0, 5, 5
    L = P.widen(2 * np.pi)
    nu, dt = 1.0, float(np.float32(0.0026))
    psi, zeta, k2 = cellular_flow(n, n, L, L, amp, mx, my)
    z = -nu * k2 * dt
    assert abs(z + 0.13) < 1e-3
    fac, R = P.stage_factors(z), rk4_factor(z)
    x0 = P.seed_positions(n, n, L, L, NPART, seed=31)

    def flow(gradient_stage):
        return lambda k, s, x: (P.cellular_velocity(x, L, L, amp, mx, my) * (R ** k * fac[s]),
                                D.cellular_gradient(x, L, L, amp, mx, my) * (R ** k * fac[gradient_stage(s)]))
    _, want = D.rk4_deformation(x0, D.identity(NPART), flow(lambda s: s), dt, steps)
    _, wrong = D.rk4_deformation(x0, D.identity(NPART), flow(lambda s: 0), dt, steps)
    pm = D.DeformationModel64(n, n, L, L, nu=nu, dt=dt)
    pm.set_vort(zeta.astype(np.float32))
    pm.set_particles(x0)
    pm.step(steps)
    tol = 10.0 * float(np.max(np.abs(pm.F - want)))
    m = X.Model(n, n, L, L, nu=nu, dt=dt)
    m.set_vort(zeta.astype(np.float32))
    m.set_particles(x0)
    m.set_particle_deformation()
    m.step(steps)
    got = _np(m.particle_deformation())
    err, sep = float(np.max(np.abs(got - want))), float(np.max(np.abs(wrong - want)))
    print("stage order F: max|F - I| %.3e, DeformationModel64 vs analytic %.3e, tol %.3e, GPU err %.3e, wrong-stage reference off by %.3e (GPU vs wrong %.3e)" %
          (float(np.max(np.abs(want - np.eye(2)))), tol / 10, tol, err, sep, float(np.max(np.abs(got - wrong)))))
    assert sep > tol
    assert float(np.max(np.abs(got - wrong))) > tol
    assert err <= tol
    m.close()


# ---- 4. a fully time-dependent flow ----
@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64)])
def test_time_dependent_flow(nx, ny):
    """The inputs of test_gpu_particles.test_time_dependent_flow (the elliptic vortex plus weak noise) against DeformationModel64, 20
    steps.  Tolerance (_grad_tol): dv = the largest difference between the GPU model's float32 velocity (diag()) and Model64's over the
    run.  Measured on MI355X: DESIGN.md, "Particle deformation and FTLE"."""
    import xlab_fftbarotropic_amd as X
    import deformation_numpy as D
    import particles_numpy as P
    from tracer_numpy import noisy_vort
    lx = ly = 600000.0
    dt, steps = 3.0, 20
    v0 = noisy_vort(nx, ny, 1e-4, make_field=X.make_field)
    x0 = P.seed_positions(nx, ny, lx, ly, NPART, seed=41)
    m = X.Model(nx, ny, lx, ly, dt=dt)
    m.set_vort(v0)
    m.set_particles(x0)
    m.set_particle_deformation()
    pm = D.DeformationModel64(nx, ny, lx, ly, dt=dt)
    pm.set_vort(v0)
    pm.set_particles(x0)

    def vdiff():
        _, u, v = m.diag()
        ur, vr = pm.velocity(pm.vc)
        return max(float(np.max(np.abs(_np(u) - ur))), float(np.max(np.abs(_np(v) - vr))))
    dv = vdiff()
    for _ in range(steps):
        m.step(1)
        pm.step(1)
        dv = max(dv, vdiff())
    got, want = _np(m.particle_deformation()), pm.F
    err = float(np.max(np.abs(got - want)))
    tol = _grad_tol(dv, steps * dt, P.widen(lx) / nx, P.widen(ly) / ny, want)
    dev = float(np.max(np.abs(want - np.eye(2))))
    print("time-dependent F %dx%d: dv %.3e m/s, max|F - I| %.3e, err %.3e, tol %.3e" % (nx, ny, dv, dev, err, tol))
    assert dev > 10 * tol
    assert err <= tol
    m.close()


# ---- 5. the stretching kernel ----
def test_stretching_kernel():
    """particle_stretching(F) on the hard matrices of the CPU test, on 3000 random ones (more than one workgroup) and on NaN / inf rows:
    the bars of deformation_numpy.check_stretching against numpy.linalg.svd, the zero matrix's row exact, and within 1e-12 of svd2x2
    (angles too, wherever sigma1 - sigma2 > 1e-8 sigma1 and the angle is not within 1e-9 of the fold).  With the model's own F:
    particle_stretching() == particle_stretching(particle_deformation()) bit for bit, ftle() == column 0 / T."""
    import xlab_fftbarotropic_amd as X
    import deformation_numpy as D
    import particles_numpy as P
    n = 64
    m = X.Model(n, n)
    names, H = D.hard_matrices()
    rng = np.random.default_rng(17)
    R = rng.standard_normal((3000, 2, 2))
    R[::4] *= 10.0 ** rng.uniform(-100, 100, (750, 1, 1))
    bad = np.array([[[np.nan, 0.0], [0.0, 1.0]], [[1.0, np.inf], [0.0, 1.0]], [[1.0, 0.0], [-np.inf, 1.0]]])
    F = np.concatenate([H, R, bad])
    got = _np(m.particle_stretching(F))
    assert got.shape == (F.shape[0], 4)
    nh, nr = H.shape[0], R.shape[0]
    assert np.isnan(got[nh + nr:]).all()
    wh = D.check_stretching(got[:nh], H, "hard")
    wr = D.check_stretching(got[nh:nh + nr], R, "random")
    ref = D.svd2x2(F[:nh + nr])
    assert got[names.index("singular"), 1] == -np.inf
    fin = np.isfinite(ref[:, :2])
    assert np.array_equal(np.isfinite(got[:nh + nr, :2]), fin)
    with np.errstate(invalid="ignore"):                         # (the zero matrix: -inf - -inf)
        strong = (ref[:, 0] - ref[:, 1]) > np.log(1e11)
        ds = np.abs(np.where(fin, got[:nh + nr, :2] - ref[:, :2], 0.0))
        distinct = (1.0 - np.exp(np.where(fin[:, 1], ref[:, 1] - ref[:, 0], -np.inf)) > 1e-8) & (np.pi / 2 - np.abs(ref[:, 2:]).max(axis=1) > 1e-9)
    assert ds[:, 0].max() <= 1e-12 and ds[~strong, 1].max() <= 1e-12 and ds[strong, 1].max() <= 1e-4
    da = float(np.abs(got[:nh + nr, 2:] - ref[:, 2:])[distinct].max())
    print("stretching (ln s1, ln s2, reconstruction): hard %.1e %.1e %.1e, random %.1e %.1e %.1e; angles vs svd2x2 %.1e over %d rows" % (*wh, *wr, da, int(distinct.sum())))
    assert da <= 1e-9 and distinct.sum() > 2900
    assert _same64(_np(m.particle_stretching(F.reshape(-1, 4))), got)
    # the model's own F
    m.set_vort(X.make_field("kuo2004", n))
    m.set_particles(P.seed_positions(n, n, 600000.0, 600000.0, 300, seed=5))
    m.set_particle_deformation()
    with pytest.raises(X.FftBaroError, match="T = 0"):
        m.ftle()
    m.step(7)
    own = _np(m.particle_stretching())
    assert own.shape == (300, 4) and _same64(own, _np(m.particle_stretching(m.particle_deformation())))
    T = m.particle_deformation_time()
    assert T == 7 * float(np.float32(3.0))
    assert _same64(_np(m.ftle()), own[:, 0] / T)
    Fm = _np(m.particle_deformation())
    assert np.isfinite(own).all() and own[:, 0].max() > 1e-4 and (own[:, 0] >= own[:, 1]).all()
    assert np.max(np.abs(own[:, 0] + own[:, 1] - np.log(np.abs(np.linalg.det(Fm))))) < 1e-12        # sigma1 sigma2 = |det F| (close to 1, not 1)
    m.close()


# ---- 6. life cycle and refusals ----
def test_life_cycle_and_refusals():
    import torch
    import xlab_fftbarotropic_amd as X
    n = 64
    m = X.Model(n, n)
    m.set_vort(X.make_field("kuo2004", n))
    L = X.lib()
    buf = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
    out = torch.zeros((8, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    el = ctypes.c_double(-1.0)

    def refused(name, args, phrase, code=FB_EINVAL, h=None):
        fn = "fb_model_" + name
        assert getattr(L, fn)(m._h if h is None else h, *args) == code, fn
        msg = L.fb_last_error().decode()
        assert msg.startswith(fn + ": ") and phrase in msg, msg
    # before particles are set
    refused("set_particle_deformation", (1,), "no particles are set")
    refused("get_particle_deformation", (ptr(buf), ctypes.byref(el)), "no particles are set")
    refused("particle_stretching", (None, 0, ptr(out)), "no particles are set")
    refused("set_particle_deformation", (2,), "on must be 0 or 1")
    refused("set_particle_deformation", (-1,), "on must be 0 or 1")
    x0 = np.array([[1.0e5, 2.0e5], [3.0e5, 4.0e5], [5.0e5, 1.0e5]])
    m.set_particles(x0)
    hbm0 = m.info()["hbm_bytes"]
    # before the deformation is switched on
    refused("get_particle_deformation", (ptr(buf), ctypes.byref(el)), "deformation")
    refused("particle_stretching", (None, 0, ptr(out)), "deformation")
    with pytest.raises(X.FftBaroError, match="deformation"):
        m.particle_deformation()
    assert el.value == -1.0
    m.set_particle_deformation()
    assert m.info()["hbm_bytes"] == hbm0 + 12 * 8 * 3
    refused("set_particle_deformation", (2,), "on must be 0 or 1")
    refused("get_particle_deformation", (None, ctypes.byref(el)), "NULL output")
    refused("particle_stretching", (ptr(buf), 8, None), "NULL output")
    refused("particle_stretching", (ptr(buf), 0, ptr(out)), "n outside [1, 2^24]")
    refused("particle_stretching", (ptr(buf), (1 << 24) + 1, ptr(out)), "n outside [1, 2^24]")
    assert L.fb_model_get_particle_deformation(m._h, ptr(buf), None) == 0          # a NULL elapsed is fine
    m.fop.synchronize()
    eye = np.tile(np.eye(2), (3, 1, 1))
    assert _same64(_np(m.particle_deformation()), eye) and m.particle_deformation_time() == 0.0
    m.step(3)
    F3 = _np(m.particle_deformation())
    assert not _same64(F3, eye) and m.particle_deformation_time() == 3 * m.dt
    m.set_particle_deformation()                                # the reset: the exact identity, T = 0, the positions stay
    assert _same64(_np(m.particle_deformation()), eye) and m.particle_deformation_time() == 0.0
    assert m.info()["hbm_bytes"] == hbm0 + 12 * 8 * 3
    m.step(2)
    assert m.particle_deformation_time() == 2 * m.dt
    m.set_particle_deformation(False)
    assert m.info()["hbm_bytes"] == hbm0
    with pytest.raises(X.FftBaroError, match="deformation"):
        m.particle_stretching()
    m.step(1)                                                   # and the model steps on, with k_particle_stage
    m.set_particle_deformation(True)
    m.set_particles(x0[:2])                                     # a new set switches it off
    with pytest.raises(X.FftBaroError, match="deformation"):
        m.particle_deformation()
    assert m.info()["hbm_bytes"] == hbm0 - 6 * 8
    m.set_particle_deformation()
    m.set_particles(None)
    with pytest.raises(X.FftBaroError, match="no particles are set"):
        m.set_particle_deformation()
    assert _np(m.particle_stretching(np.eye(2)[None])).shape == (1, 4)      # any matrices: no particles needed
    m.step(1)
    m.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every entry point raises the particles' unsupported error under its own name"""
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
                calls = (("set_particle_deformation", lambda: s.set_particle_deformation()), ("get_particle_deformation", lambda: s.particle_deformation()),
                         ("get_particle_deformation", lambda: s.particle_deformation_time()), ("particle_stretching", lambda: s.particle_stretching()),
                         ("particle_stretching", lambda: s.particle_stretching(np.eye(2)[None])), ("get_particle_deformation", lambda: s.ftle()))
                for name, call in calls:
                    try:
                        call()
                        msgs[r].append((name, None))
                    except X.FftBaroError as e:
                        msgs[r].append((name, str(e)))
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
        assert len(msgs[r]) == 6
        for name, msg in msgs[r]:
            assert msg is not None and "fb_slab_" + name + ": particles are not supported" in msg and "world > 1" in msg, (name, msg)


# ---- 7. the driver ----
def _run_driver(d, n, v0, xy, extra, steps):
    import subprocess
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    if xy is not None:
        (d / "input" / "p.bin").write_bytes(np.ascontiguousarray(xy, dtype="<f8").tobytes())
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--record-step", "3", "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode(), (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_particle_deformation(tmp_path):
    """barotropic_main.out --particles p.bin --particle-deformation at 64^2, 100 particles, 6 steps, a record every 3: both new files
    follow particles_step_N.bin in ./log and equal Model.particle_deformation() and particle_stretching() at the same steps bit for
    bit; without --particles, and with --world 2, the run ends with exit status 2 and one line on stderr."""
    import subprocess
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, npart = 64, 100
    v0 = X.make_field("kuo2004", n)
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, npart, seed=81)
    rc, err, log = _run_driver(tmp_path / "run", n, v0, x0, ["--particles", "p.bin", "--particle-deformation"], 7)
    assert rc == 0, err
    names = ("vort_src_input", "vort", "psi", "u", "v", "particles", "particle_deformation", "particle_stretching")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 3, 6) for name in names]
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_particles(x0)
    m.set_particle_deformation()
    for s in (0, 3, 6):
        read = lambda name, k: np.fromfile(str(tmp_path / "run" / "output" / ("%s_step_%d.bin" % (name, s))), dtype="<f8").reshape(npart, k)
        assert _same64(read("particles", 2), _np(m.particles())), s
        assert _same64(read("particle_deformation", 4), _np(m.particle_deformation()).reshape(npart, 4)), s
        assert _same64(read("particle_stretching", 4), _np(m.particle_stretching())), s
        m.step(3)
    m.close()
    bad = {"alone": (None, ["--particle-deformation"]), "world": (x0, ["--particles", "p.bin", "--particle-deformation", "--world", "2", "--ranks-as-threads"])}
    for tag, (xy, extra) in bad.items():
        rc, err, _ = _run_driver(tmp_path / tag, n, v0, xy, extra, 1)
        assert rc == 2, (tag, rc, err)
        assert len(err.strip().splitlines()) == 1 and "--particle-deformation" in err, (tag, err)
