"""GPU tests of the Lagrangian particles: fb_model_set_particles / fb_model_get_particles / fb_model_particle_count / fb_model_sample
(Model.set_particles, particles, particle_count, sample), their slab counterparts and the driver's --particles.

Checked: the interpolation kernel against tests/particles_numpy.lagrange4_sample on identical float32 data; trajectories in a steady
flow on every kernel path of the step against a numpy RK4 in the downloaded diag() fields; the order of the stage velocities in a
decaying flow with analytic stage states; a fully time-dependent flow against the float64 model ParticleModel64; the vorticity, the
tracer and a captured step bit for bit what they are without particles; the plumbing and the driver.  The measured figures are
printed, one line per case (pytest -s)."""
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


def _np(t):
    return t.cpu().numpy()


def _same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


# ---- 1. the interpolation kernel ----
@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64), (64, 192), (256, 256)])
def test_sample_against_numpy(nx, ny):
    """fb_model_sample against lagrange4_sample on the same float32 field (random; Kuo2004), n in {1, 63, 257, 1000} positions that
    include grid points, the first and last cells of both axes and positions 3 domain lengths away: within 1e-12 max|field| (both
    sides are float64 arithmetic on identical data), and on grid points the float32 value itself, widened.  (make_field("kuo2004")
    is all zeros on the two non-square grids: the bound is 0 there and the sample must be exactly 0.)"""
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    lx = ly = 600000.0
    m = X.Model(nx, ny, lx, ly)
    rng = np.random.default_rng(11)
    fields = {"random": rng.standard_normal((nx, ny)).astype(np.float32), "kuo2004": X.make_field("kuo2004", nx, ny)}
    for name, f in fields.items():
        for n in (1, 63, 257, 1000):
            xy = P.seed_positions(nx, ny, lx, ly, n, seed=n)
            want = P.lagrange4_sample(f, xy, lx, ly)
            got = _np(m.sample(f, xy))
            err = float(np.max(np.abs(got - want)))
            scale = float(np.max(np.abs(f)))
            print("sample %dx%d %s n=%d: max err %.3e, max|f| %.3e" % (nx, ny, name, n, err, scale))
            assert got.shape == (n,)
            assert err <= 1e-12 * scale
        g = P.grid_points(nx, ny, lx, ly, 64)
        assert g.shape[0] >= 32
        i = np.mod(np.round(g[:, 0] / (P.widen(lx) / nx)).astype(np.int64), nx)
        j = np.mod(np.round(g[:, 1] / (P.widen(ly) / ny)).astype(np.int64), ny)
        assert _same64(_np(m.sample(f, g)), f[i, j].astype(np.float64))
    assert m.particle_count() == 0                              # sampling needs no particles and sets none
    m.close()


# ---- 2. a frozen flow on every kernel path ----
FROZEN = [(64, 64), (192, 64), (256, 256), (1024, 1024), (4096, 4096), (128, 16384), (16384, 64)]


@pytest.mark.parametrize("nx,ny", FROZEN)
def test_frozen_flow_trajectories(nx, ny):
    """The cellular flow with nu = 0 is a steady solution: every stage velocity equals diag()'s u, v up to the float32 rounding of a
    vanishing tendency.  Reference: numpy RK4 of the particles in the diag() fields downloaded before the first step, with
    lagrange4_sample.  4 steps, 1000 particles.
    Tolerance: dv = the largest change of diag()'s u, v over the run (measured here from diag() alone, at the start and after every
    step: the state the stage velocities are formed from lies between those), allowed ten times over the elapsed time, 10 dv T, plus
    64 eps64 max|X| for the float64 rounding of the positions on either side (4 steps of ~8 operations each, twice).  Measured on
    MI355X: DESIGN.md, "Lagrangian particles"."""
    import torch
    import xlab_fftbarotropic_amd as X
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
    assert m.particle_count() == NPART
    dv = 0.0
    for _ in range(steps):
        m.step(1)
        _, u, v = m.diag()
        dv = max(dv, float((u - u0).abs().max().item()), float((v - v0).abs().max().item()))
    got = _np(m.particles())
    un, vn = _np(u0), _np(v0)
    dtw = float(np.float32(dt))
    want = P.rk4_particles(x0, lambda n, s, x: P.sample_uv(un, vn, x, lx, ly), dtw, steps)
    err = float(np.max(np.abs(got - want)))
    tol = 10.0 * dv * steps * dtw + 64 * EPS64 * float(np.max(np.abs(want)))
    moved = float(np.max(np.abs(want - x0)))
    print("frozen %dx%d: max|u| %.3f m/s, dv %.3e m/s, moved %.1f m, err %.3e m, tol %.3e m" % (nx, ny, float(np.max(np.abs(un))), dv, moved, err, tol))
    assert moved > 10.0
    assert err <= tol
    m.close()


# ---- 3. the order of the stage velocities ----
def test_stage_order():
    """The cellular flow on Lx = Ly = 2 pi with strong viscosity: the nonlinear term vanishes, every mode of the flow decays with
    z = -nu K^2 dt = -0.13 per step, and the stage velocities are u0 {1, 1 + z/2, 1 + z/2 + z^2/4, 1 + z + z^2/2 + z^3/4} with u0 the
    velocity at the start of the step.  Reference: float64 RK4 of the particles with those ANALYTIC stage velocities.  mx = my = 5
    (K^2 = 50, nu dt = 0.0026) keeps every mode inside the dealiasing circle (K^2 < 968) in RK4's stability range: 0.0026 * 968 = 2.52
    < 2.78.  64^2, 10 steps.
    Tolerance: 10 x the difference ParticleModel64 shows against the analytic trajectories (its interpolation error, computed here on
    the CPU).  A reference that uses u0 at every stage is asserted to FAIL that tolerance, against the analytic reference and against
    the GPU: the test discriminates."""
    import xlab_fftbarotropic_amd as X
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
    want = P.rk4_particles(x0, lambda k, s, x: P.cellular_velocity(x, L, L, amp, mx, my) * (R ** k * fac[s]), dt, steps)
    wrong = P.rk4_particles(x0, lambda k, s, x: P.cellular_velocity(x, L, L, amp, mx, my) * (R ** k), dt, steps)
    pm = P.ParticleModel64(n, n, L, L, nu=nu, dt=dt)
    pm.set_vort(zeta.astype(np.float32))
    pm.set_particles(x0)
    pm.step(steps)
    tol = 10.0 * float(np.max(np.abs(pm.particles() - want)))
    m = X.Model(n, n, L, L, nu=nu, dt=dt)
    m.set_vort(zeta.astype(np.float32))
    m.set_particles(x0)
    m.step(steps)
    got = _np(m.particles())
    err = float(np.max(np.abs(got - want)))
    sep = float(np.max(np.abs(wrong - want)))
    print("stage order: moved %.3e, ParticleModel64 vs analytic %.3e, tol %.3e, GPU err %.3e, wrong-stage reference off by %.3e (GPU vs wrong %.3e)" %
          (float(np.max(np.abs(want - x0))), tol / 10, tol, err, sep, float(np.max(np.abs(got - wrong)))))
    assert sep > tol                                            # the wrong-stage reference fails the tolerance ...
    assert float(np.max(np.abs(got - wrong))) > tol             # ... and the GPU is told apart from it
    assert err <= tol
    m.close()


# ---- 4. a fully time-dependent flow ----
@pytest.mark.parametrize("nx,ny", [(64, 64), (192, 64)])
def test_time_dependent_flow(nx, ny):
    """The elliptic vortex plus weak noise (tracer_numpy.noisy_vort) against ParticleModel64, 20 steps.
    Tolerance: dv = the largest difference between the GPU model's float32 velocity (diag()) and Model64's over the same run (at the
    start and after every step), allowed ten times over the elapsed time, 10 dv T, plus 64 eps64 max|X| per step pair for the float64
    rounding of the positions.  Measured on MI355X: DESIGN.md, "Lagrangian particles"."""
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    from tracer_numpy import noisy_vort
    lx = ly = 600000.0
    dt, steps = 3.0, 20
    v0 = noisy_vort(nx, ny, 1e-4, make_field=X.make_field)
    x0 = P.seed_positions(nx, ny, lx, ly, NPART, seed=41)
    m = X.Model(nx, ny, lx, ly, dt=dt)
    m.set_vort(v0)
    m.set_particles(x0)
    pm = P.ParticleModel64(nx, ny, lx, ly, dt=dt)
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
    got, want = _np(m.particles()), pm.particles()
    err = float(np.max(np.abs(got - want)))
    tol = 10.0 * dv * steps * dt + 64 * EPS64 * float(np.max(np.abs(want))) * steps / 4
    print("time-dependent %dx%d: dv %.3e m/s, moved %.1f m, err %.3e m, tol %.3e m" % (nx, ny, dv, float(np.max(np.abs(want - x0))), err, tol))
    assert float(np.max(np.abs(want - x0))) > 100.0
    assert err <= tol
    m.close()


# ---- 5. non-interference and plumbing ----
@pytest.mark.parametrize("n,steps", [(256, 10), (4096, 2)])
def test_the_step_and_the_tracer_are_untouched(n, steps):
    """the vorticity bit for bit with and without particles; vorticity and tracer bit for bit with tracer plus particles against the
    tracer alone"""
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    from tracer_numpy import recipe_dt
    dt = recipe_dt(n, n)
    v0 = X.make_field("kuo2004", n)
    c0 = np.ascontiguousarray(np.roll(X.make_field("gaussian", n), n // 4, axis=0))
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, NPART, seed=51)

    def run(tracer, particles):
        m = X.Model(n, n, dt=dt)
        m.set_vort(v0)
        if tracer:
            m.set_tracer(c0, kappa=20.0)
        if particles:
            m.set_particles(x0)
        m.step(steps)
        out = (_np(m.vort()), _np(m.tracer()) if tracer else None, _np(m.particles()) if particles else None)
        m.close()
        return out
    plain, withp = run(False, False), run(False, True)
    assert _same32(plain[0], withp[0])
    assert not _same64(withp[2], x0)
    tr, both = run(True, False), run(True, True)
    assert _same32(tr[0], plain[0]) and _same32(both[0], plain[0])
    assert _same32(tr[1], both[1])
    assert _same64(both[2], withp[2])                           # and the tracer does not disturb the particles


def test_graph_replay_gives_the_same_positions():
    """positions bit for bit with use_graph on and off; particles set between two step calls drop the captured step, and removing them
    drops it again"""
    import torch
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    n = 256
    v0 = X.make_field("kuo2004", n)
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, NPART, seed=61)
    e = X.Model(n, n)
    e.set_vort(v0)
    e.step(6)
    e.set_particles(x0)
    e.step(12)
    want, wantv = _np(e.particles()), _np(e.vort())
    e.set_particles(None)
    e.step(4)
    wantv2 = _np(e.vort())
    e.close()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = X.Model(n, n)
        g.set_vort(v0)
        g.use_graph(True)
        g.step(6)
        g.set_particles(x0)
        g.step(12)
        got, gotv = _np(g.particles()), _np(g.vort())
        g.set_particles(None)
        g.step(4)
        gotv2 = _np(g.vort())
        g.fop.synchronize()
        g.close()
    assert _same64(got, want)
    assert _same32(gotv, wantv) and _same32(gotv2, wantv2)


def test_positions_are_unwrapped():
    """a particle in the x-directed shear flow psi = A cos(2 pi y / Ly) (steady, nu = 0) crosses x = Lx: particles() goes on counting,
    particles(wrap=True) lies in [0, Lx) and is the same point"""
    import xlab_fftbarotropic_amd as X
    from tracer_numpy import cellular_flow
    n, L = 64, 600000.0
    psi, zeta, k2 = cellular_flow(n, n, L, L, 1.0e6, 0, 1)
    m = X.Model(n, n, L, L, nu=0.0, dt=3.0)
    m.set_vort(zeta.astype(np.float32))
    x0 = np.array([[L - 50.0, L / 4], [10.0, 3 * L / 4]])        # u = +10.5 m/s at Ly/4, -10.5 m/s at 3 Ly/4
    m.set_particles(x0)
    m.step(10)
    p, w = _np(m.particles()), _np(m.particles(wrap=True))
    print("unwrapped: x = %.3f, %.3f; wrapped %.3f, %.3f" % (p[0, 0], p[1, 0], w[0, 0], w[1, 0]))
    assert p[0, 0] > L + 200.0 and p[1, 0] < -200.0
    assert np.all(w >= 0.0) and np.all(w[:, 0] < L) and np.all(w[:, 1] < L)
    assert abs(w[0, 0] - (p[0, 0] - L)) < 1e-6 and abs(w[1, 0] - (p[1, 0] + L)) < 1e-6
    m.close()


def test_arguments_and_removal():
    import ctypes
    import torch
    import xlab_fftbarotropic_amd as X
    n = 64
    m = X.Model(n, n)
    m.set_vort(X.make_field("kuo2004", n))
    L = X.lib()
    buf = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    fld = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    FB_EINVAL = 1
    assert L.fb_model_set_particles(m._h, ptr(buf), 0) == FB_EINVAL
    assert L.fb_model_set_particles(m._h, ptr(buf), (1 << 24) + 1) == FB_EINVAL
    assert L.fb_model_set_particles(m._h, ptr(buf), -1) == FB_EINVAL
    assert L.fb_model_set_particles(m._h, None, 4) == FB_EINVAL
    assert L.fb_model_set_particles(None, ptr(buf), 4) == FB_EINVAL
    assert L.fb_model_sample(m._h, ptr(fld), ptr(buf), 0, ptr(out)) == FB_EINVAL
    assert L.fb_model_sample(m._h, None, ptr(buf), 4, ptr(out)) == FB_EINVAL
    assert L.fb_model_get_particles(m._h, ptr(buf)) == FB_EINVAL          # none set
    assert m.particle_count() == 0
    with pytest.raises(X.FftBaroError):
        m.particles()
    hbm0 = m.info()["hbm_bytes"]
    m.set_particles(np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))
    assert m.particle_count() == 3
    assert m.info()["hbm_bytes"] > hbm0
    assert _same64(_np(m.particles()), np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))
    m.set_particles(torch.tensor([[7.0, 8.0]], dtype=torch.float64))         # replaces them
    assert m.particle_count() == 1 and _same64(_np(m.particles()), np.array([[7.0, 8.0]]))
    assert _np(m.sample(m.vort())).shape == (1,)                # xy=None: at the particles
    m.set_particles(None)
    assert m.particle_count() == 0 and m.info()["hbm_bytes"] == hbm0
    with pytest.raises(X.FftBaroError):
        m.particles()
    m.step(2)                                                   # and the model steps on
    m.close()


def test_slab_of_one_rank_matches_the_model():
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    S = _slab()
    n, steps = 256, 10
    v0 = X.make_field("kuo2004", n)
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, NPART, seed=71)
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_particles(x0)
    m.step(steps)
    want, f = _np(m.particles()), m.vort()
    ws = _np(m.sample(f))
    m.close()
    s = S.EngineSlab(n, n)
    s.set_vort_local(v0)
    s.set_particles(x0)
    assert s.particle_count() == NPART
    s.step(steps)
    got = _np(s.particles())
    assert _same64(got, want)
    assert _same64(_np(s.sample(s.vort_local())), ws)
    assert np.all(_np(s.particles(wrap=True)) >= 0.0)
    s.set_particles(None)
    with pytest.raises(X.FftBaroError):
        s.particles()
    s.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every particle entry point raises the engine's unsupported error"""
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
                calls = (lambda: s.set_particles(np.array([[1.0, 2.0]])), lambda: s.set_particles(None), lambda: s.particles(),
                         lambda: s.sample(np.zeros((s.XL, n), np.float32), np.array([[1.0, 2.0]])))
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
        assert len(msgs[r]) == 4
        for msg in msgs[r]:
            assert msg is not None and "not supported" in msg and "world > 1" in msg, msg


# ---- 6. the driver ----
def _run_driver(d, n, v0, xy, extra, steps=21):
    import subprocess
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    if xy is not None:
        (d / "input" / "p.bin").write_bytes(xy if isinstance(xy, bytes) else np.ascontiguousarray(xy, dtype="<f8").tobytes())
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--record-step", "10", "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode(), (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_particles(tmp_path):
    """barotropic_main.out --particles p.bin at 256^2, 20 steps, a record every 10: particles_step_N.bin is the last file of each record
    in ./log (after the azimuthal files), holds 16 n bytes and equals Model.particles() at the same steps bit for bit; a file whose
    size is no positive multiple of 16, n above 2^24 and --world 2 end with exit status 2 and one line on stderr."""
    import subprocess
    import xlab_fftbarotropic_amd as X
    import particles_numpy as P
    subprocess.check_call(["make", "-s", "-C", HOST])
    n = 256
    v0 = X.make_field("kuo2004", n)
    x0 = P.seed_positions(n, n, 600000.0, 600000.0, NPART, seed=81)
    rc, err, log = _run_driver(tmp_path / "run", n, v0, x0, ["--particles", "p.bin", "--dump-azimuthal"])
    assert rc == 0, err
    names = ("vort_src_input", "vort", "psi", "u", "v", "azimuthal", "azimuthal_center", "particles")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 10, 20) for name in names]
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_particles(x0)
    for s in (0, 10, 20):
        f = tmp_path / "run" / "output" / ("particles_step_%d.bin" % s)
        assert f.stat().st_size == 16 * NPART
        assert _same64(np.fromfile(str(f), dtype="<f8").reshape(NPART, 2), _np(m.particles())), s
        assert _same32(np.fromfile(str(tmp_path / "run" / "output" / ("vort_step_%d.bin" % s)), dtype="<f4").reshape(n, n), _np(m.vort())), s
        for _ in range(10):
            m.step(1)
    m.close()
    bad = {"odd": (b"\0" * 24, ["--particles", "p.bin"]), "empty": (b"", ["--particles", "p.bin"]), "world": (x0, ["--particles", "p.bin", "--world", "2", "--ranks-as-threads"])}
    for tag, (xy, extra) in bad.items():
        rc, err, _ = _run_driver(tmp_path / tag, n, v0, xy, extra, steps=1)
        assert rc == 2, (tag, rc, err)
        assert len(err.strip().splitlines()) == 1 and "--particles" in err, (tag, err)
    # n above the cap: a sparse file of 16 (2^24 + 1) bytes, never read
    d = tmp_path / "cap"
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    with open(str(d / "input" / "p.bin"), "wb") as fh:
        fh.truncate(16 * ((1 << 24) + 1))
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "1", "--no-timing", "--particles", "p.bin"],
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 2 and len(r.stderr.decode().strip().splitlines()) == 1
