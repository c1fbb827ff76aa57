"""GPU checks of the split stage: stochastic ring forcing, linear drag and hyperviscosity after every RK4 step (fb_model_set_forcing,
Model.set_forcing), against the float64 restatement tests/forcing_numpy.py.

  1. the increment Delta_n against numpy: ring membership, 2 float32 ulp of the amplitude, the two real lines bit-exactly conjugate
  2. the path matrix: the six grids of adjoint_numpy.PATH_CASES on the noisy, never-dealiased inputs with forcing, drag and nabla^8
     hyperviscosity all on, 5 steps, <= 1e-5 relative L2 against the float64 coupled run, masked modes bit-equal to their initial
     values; and 4096^2 (k_col_full's layout), 3 steps, against a subsampled fixture
  3. the budget against numpy; eps dt from rest; the totals' bits repeat
  4. a captured step against eager steps: the same bits in zeta, the budget and the clock
  5. the same seed gives the same bits, another seed others; a forcing that was removed leaves no trace
  6. a single mode decays by D R per step
  7. the tangent set: -(nu K^2 + mu + nu_p K^2p) from lyapunov() in a fluid at rest; tangent() against the float64 tangent of the
     split system
  8. refusals
and a slab of one rank runs the 256^2 row of the matrix bit-identically to Model.  tests/test_forcing_cpu.py shows that the matrix's
inputs make its bar decisive."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

import forcing_numpy as F                                       # noqa: E402
import tangent_numpy as G                                       # noqa: E402
import tracer_numpy as T                                        # noqa: E402
from ref_numpy import rel_l2, tables                            # noqa: E402

CASE_IDS = ["%dx%d" % (k.nx, k.ny) for k in F.PATH_CASES]
EPS32 = float(np.finfo(np.float32).eps)
EINVAL, EUNSUPPORTED = "invalid argument: ", "unsupported grid size: "          # fb_strerror of FB_EINVAL, FB_EUNSUPPORTED
FIXTURE = os.path.join(HERE, "golden", "forcing_4096x4096_step3.npz")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


@functools.lru_cache(maxsize=None)
def _inputs(nx, ny):
    out = G.tangent_inputs(nx, ny, 3e-2)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(nx, ny, tangent=False):
    """the float64 coupled run of a case of the matrix, computed here once: (vort, tangent or None, budget)"""
    case = F.case_of(nx, ny)
    v, dz, src = _inputs(nx, ny)
    r = F.recipe_model(case, v, dz if tangent else None, src)
    r.step(case.steps)
    out = (r.vort(), r.tangent() if tangent else None)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out + (r.budget(),)


def _gpu_model(case, cls=None, source=True, **kw):
    import xlab_fftbarotropic_amd as X
    v, _, src = _inputs(case.nx, case.ny)
    m = (cls or X.Model)(case.nx, case.ny, nu=G.NU, dt=T.recipe_dt(case.nx, case.ny))
    m.set_vort(v)
    if source:
        m.set_source(src)
    m.set_forcing(**dict(F.case_forcing(case), **kw))
    return m


def _raises(call, code, name):
    import xlab_fftbarotropic_amd as X
    with pytest.raises(X.FftBaroError) as e:
        call()
    assert str(e.value).startswith(code + name + ": "), str(e.value)
    return str(e.value)


# ---- 1. the increment ----
@pytest.mark.parametrize("nx,ny,k,width", [(64, 64, 12.0, 1.5), (192, 192, 33.0, 2.0), (64, 4096, 33.0, 2.0)])
def test_increment_against_numpy(nx, ny, k, width):
    import xlab_fftbarotropic_amd as X
    kw = dict(rate=0.7, k=k * F.K1, width=width * F.K1, seed=F.SEED)
    f = F.Forcing(nx, ny, 3.0, **kw)
    m = X.Model(nx, ny, nu=G.NU, dt=3.0)
    m.set_forcing(**kw)
    assert m.forcing_budget()["n_ring"] == f.n_ring
    i, j = np.nonzero(f.ring)
    amp = (f.grids * np.sqrt(2.0 * f.rate * f.dt * f.K2[i, j] / f.n_ring)).astype(np.float32)
    for n in (0, 1, 2 ** 32 + 5):
        got, want = _np(m.forcing_increment(n)), f.increment(n)
        assert np.array_equal(got != 0, f.ring)
        off = np.maximum(np.abs(got.real[i, j] - want.real[i, j]), np.abs(got.imag[i, j] - want.imag[i, j])) / np.spacing(amp)
        print("%dx%d, n = %d: %d ring modes (N_ring %d), largest difference %.3g ulp of the amplitude, %d values differ"
              % (nx, ny, n, len(i), f.n_ring, off.max(), int((got[i, j] != want[i, j]).sum())))
        assert off.max() <= 2.0
        for line in (0, ny // 2):
            assert np.array_equal(got[1:nx // 2, line], np.conj(got[:nx // 2:-1, line])) and got[0, line] == 0 and got[nx // 2, line] == 0
    m.close()


# ---- 2. the path matrix ----
@pytest.mark.parametrize("case", F.PATH_CASES, ids=CASE_IDS)
def test_path_against_float64(case):
    nx, ny = case.nx, case.ny
    masked = tables(nx, ny, 600000.0, 600000.0)[4] == 0
    m = _gpu_model(case)
    s0 = _np(m.spectrum())
    m.step(case.steps)
    got, s1, b = _np(m.vort()), _np(m.spectrum()), m.forcing_budget()
    m.close()
    want, _, rb = _reference(nx, ny)
    err = rel_l2(got, want)
    print("path %dx%d, %d steps, N_ring %d: vorticity rel L2 = %.3g (probe shifts %.3g / %.3g); masked modes %d"
          % (nx, ny, case.steps, b["n_ring"], err, case.shift_conj, case.shift_clock, int(masked.sum())))
    assert case.shift_conj >= F.SHIFT_BAR and case.shift_clock >= F.SHIFT_BAR
    assert b["clock"] == case.steps and b["n_ring"] == rb["n_ring"]
    assert err <= 1e-5
    assert masked.any() and np.array_equal(_bits(s0.real[masked]), _bits(s1.real[masked])) and np.array_equal(_bits(s0.imag[masked]), _bits(s1.imag[masked]))
    assert not np.array_equal(s0[~masked], s1[~masked])


def test_path_4096_against_the_fixture():
    """k_col_full's layout: 4096^2, 3 steps, every sub-th point and the full-field L2 norm of the float64 run
    (tests/golden/make_forcing_fixtures.py), inputs rebuilt from the stored seed"""
    import xlab_fftbarotropic_amd as X
    Z = np.load(FIXTURE)
    nx = ny = 4096
    case = F.ForcingCase(nx, ny, int(Z["steps"]), float(Z["rate"]), float(Z["k"]), float(Z["width"]), float(Z["shift_conj"]), float(Z["shift_clock"]))
    assert (case.steps, case.rate, case.k, case.width) == (3, F.RATE, F.RING_K, F.RING_WIDTH)
    assert (int(Z["seed"]), int(Z["forcing_seed"]), float(Z["vort_noise"]), float(Z["dt"]), float(Z["nu"])) == (T.RECIPE_SEED, F.SEED, 3e-2, T.recipe_dt(nx, ny), G.NU)
    kw = F.case_forcing(case)
    assert (float(Z["drag"]), float(Z["hyper_nu"]), int(Z["hyper_order"])) == (kw["drag"], kw["hyper_nu"], kw["hyper_order"])
    assert case.shift_conj >= F.SHIFT_BAR and case.shift_clock >= F.SHIFT_BAR
    v = T.noisy_vort(nx, ny, 3e-2, make_field=X.make_field)
    m = X.Model(nx, ny, nu=G.NU, dt=T.recipe_dt(nx, ny))
    m.set_vort(v)
    m.set_forcing(**kw)
    m.step(case.steps)
    g, b = m.vort(), m.forcing_budget()
    m.close()
    sx, sy = (int(k) for k in Z["sub"])
    err = rel_l2(_np(g[::sx, ::sy]), Z["vort_sub"])
    norm = abs(float(g.double().pow(2).sum().sqrt()) / float(Z["vort_l2"]) - 1)
    bud = max(abs(b[k] / float(Z[k]) - 1) for k in ("dE_forc", "dE_diss", "dZ_forc", "dZ_diss"))
    print("path 4096^2, 3 steps, N_ring %d: vorticity rel L2 on every (%d, %d)-th point = %.3g, norm off by %.2g, budget off by %.2g; probe shifts %.3g / %.3g"
          % (b["n_ring"], sx, sy, err, norm, bud, case.shift_conj, case.shift_clock))
    assert b["n_ring"] == int(Z["n_ring"]) and b["clock"] == 3
    assert err <= 1e-5 and norm <= 1e-5
    assert bud <= 1e-6


# ---- 3. the budget ----
def test_budget_against_float64_and_its_bits_repeat():
    case = F.case_of(256, 256)
    runs = []
    for _ in range(2):
        m = _gpu_model(case)
        m.step(case.steps)
        runs.append(m.forcing_budget())
        m.close()
    _, _, want = _reference(256, 256)
    for k in ("dE_forc", "dE_diss", "dZ_forc", "dZ_diss"):
        print("%s: %.12g on the GPU, %.12g in float64, off by %.3g" % (k, runs[0][k], want[k], abs(runs[0][k] / want[k] - 1)))
        assert abs(runs[0][k] / want[k] - 1) <= 1e-6
        assert np.float64(runs[0][k]).view(np.uint64) == np.float64(runs[1][k]).view(np.uint64)
    assert runs[0] == runs[1] and runs[0]["clock"] == case.steps and runs[0]["n_ring"] == want["n_ring"]


@pytest.mark.parametrize("nx,ny", [(256, 256), (1024, 64)])
def test_one_step_from_rest_adds_rate_times_dt(nx, ny):
    import xlab_fftbarotropic_amd as X
    rate, dt = 0.37, 3.0
    m = X.Model(nx, ny, nu=0.0, dt=dt)
    m.set_vort(np.zeros((nx, ny), np.float32))
    m.set_forcing(rate=rate, k=F.RING_K, width=F.RING_WIDTH, seed=3)
    m.step(1)
    b = m.forcing_budget()
    m.close()
    print("%dx%d from rest: dE_forc = %.10g, rate dt = %.10g" % (nx, ny, b["dE_forc"], rate * dt))
    assert abs(b["dE_forc"] / (rate * dt) - 1) <= 1e-6 and b["dE_diss"] == 0.0 and b["dZ_diss"] == 0.0 and b["clock"] == 1


# ---- 4. a captured step ----
@pytest.mark.parametrize("nx,ny", [(256, 256), (1024, 64)])
def test_graph_replay_is_bit_identical_to_eager_steps(nx, ny):
    """6 steps with use_graph(True) (one eager, one captured, replayed five times) and with use_graph(False): the clock is read from
    device memory, so every replay draws the noise of its own step"""
    import torch
    case = F.case_of(nx, ny)
    out = []
    for graph in (True, False):
        with torch.cuda.stream(torch.cuda.Stream()):
            import xlab_fftbarotropic_amd as X
            v, _, src = _inputs(nx, ny)
            m = X.Model(nx, ny, nu=G.NU, dt=T.recipe_dt(nx, ny))
            m.fop.use_current_stream()
            m.use_graph(graph)
            m.set_vort(v)
            m.set_source(src)
            m.set_forcing(**F.case_forcing(case))
            m.step(6)
            out.append((_np(m.vort()), m.forcing_budget()))
            m.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert out[0][1] == out[1][1] and out[0][1]["clock"] == 6


# ---- 5. reproducibility and removal ----
def test_seed_and_removal():
    import xlab_fftbarotropic_amd as X
    case = F.case_of(256, 256)
    runs = {}
    for name, kw in (("a", {}), ("b", {}), ("other", {"seed": F.SEED + 1})):
        m = _gpu_model(case, **kw)
        m.step(3)
        runs[name] = _np(m.vort())
        m.close()
    assert np.array_equal(_bits(runs["a"]), _bits(runs["b"]))
    assert not np.array_equal(runs["a"], runs["other"])
    v, _, src = _inputs(256, 256)
    out = []
    for forced in (True, False):
        m = X.Model(256, 256, nu=G.NU, dt=3.0)
        m.set_vort(v)
        m.set_source(src)
        before = m.info()["hbm_bytes"]
        if forced:
            m.set_forcing(**F.case_forcing(case))
            assert m.info()["hbm_bytes"] > before
            m.set_forcing()
            assert m.info()["hbm_bytes"] == before
            _raises(m.forcing_budget, EINVAL, "fb_model_forcing_budget")
        m.step(3)
        out.append(_np(m.vort()))
        m.close()
    assert np.array_equal(_bits(out[0]), _bits(out[1]))
    assert not np.array_equal(out[0], runs["a"])


# ---- 6. a single mode ----
def test_single_mode_decay():
    """256 x 128, zeta = A cos cos (J = 0), nu, drag and nabla^8 hyperviscosity: after 50 steps the amplitude is (D R(z))^50 of the
    initial one, z = nu laplacian_coe dt and R the RK4 factor, within 1e-5"""
    import xlab_fftbarotropic_amd as X
    nx, ny, dt, steps, nu, mx, my = 256, 128, 3.0, 50, 2.0e5, 9, 5
    _, zeta, _ = T.cellular_flow(nx, ny, amp=1.0e6, mx=mx, my=my)
    K2 = F.Forcing(nx, ny, dt).K2[mx, my]
    kw = dict(drag=2e-3, hyper_nu=4e-3 / K2 ** 4, hyper_order=4)
    f = F.Forcing(nx, ny, dt, **kw)
    m = X.Model(nx, ny, nu=nu, dt=dt)
    m.set_vort(zeta.astype(np.float32))
    m.set_forcing(**kw)
    z0 = _np(m.vort()).astype(np.float64)
    m.step(steps)
    z1 = _np(m.vort()).astype(np.float64)
    m.close()
    ratio = float((z1 * z0).sum() / (z0 * z0).sum())
    want = float(f.D[mx, my] * T.rk4_factor(-float(np.float32(nu)) * K2 * dt)) ** steps
    print("single mode, %d steps: amplitude ratio %.9g, (D R)^n = %.9g, off by %.3g; D = %.9g; shape off by %.3g"
          % (steps, ratio, want, abs(ratio / want - 1), f.D[mx, my], rel_l2(z1, ratio * z0)))
    assert 0.1 < want < 0.9
    assert abs(ratio / want - 1) <= 1e-5
    assert rel_l2(z1, ratio * z0) <= 1e-5


# ---- 7. the tangent set ----
def test_lyapunov_of_a_single_mode_in_a_fluid_at_rest():
    """zeta = 0, dz = A cos cos, nu, mu and nu_4 set, no forcing: lyapunov() returns (ln R(-nu K^2 dt) + ln D) / dt
    = -(nu K^2 + mu + nu_4 K^8), to the bar of tests/test_gpu_tangent.py's test of -nu K^2"""
    import xlab_fftbarotropic_amd as X
    n, nu, dt, steps, every, mx, my = 256, 1.0e4, 3.0, 100, 25, 20, 30
    psi, _, _ = T.cellular_flow(n, n, amp=1.0e-6, mx=mx, my=my)
    K2 = F.Forcing(n, n, dt).K2[mx, my]
    mu, nu4 = 1.0e-3, 2.0e-3 / K2 ** 4
    f = F.Forcing(n, n, dt, drag=mu, hyper_nu=nu4, hyper_order=4)
    m = X.Model(n, n, nu=nu, dt=dt)
    m.set_vort(np.zeros((n, n), np.float32))
    m.set_tangent(psi.astype(np.float32))
    m.set_forcing(drag=mu, hyper_nu=nu4, hyper_order=4)
    lam, factors = m.lyapunov(steps, every)
    b = m.forcing_budget()
    m.close()
    z = -nu * K2 * dt
    total = float(np.log(T.rk4_factor(z)) + np.log(f.D[mx, my]))
    want, analytic = total / dt, -(nu * K2 + mu + nu4 * K2 ** 4)
    bar = 4 * EPS32 / abs(total) + 1e-6
    print("lyapunov with drag and hyperviscosity, 256^2: %.8g s^-1, (ln R + ln D) / dt = %.8g, -(nu K^2 + mu + nu_4 K^8) = %.8g; off by %.3g / %.3g (bar %.3g)"
          % (lam, want, analytic, abs(lam / want - 1), abs(lam / analytic - 1), bar))
    assert abs(lam / want - 1) <= bar and abs(lam / analytic - 1) <= bar
    assert abs(analytic / (-nu * K2) - 1) > 100 * bar           # the two new terms are what is being measured
    assert len(factors) == steps // every and b["clock"] == steps and b["n_ring"] == 0


def test_tangent_of_the_split_system_against_float64():
    case = F.case_of(256, 256)
    v, dz, src = _inputs(256, 256)
    m = _gpu_model(case)
    m.set_tangent(dz)
    m.step(case.steps)
    gt, gv = _np(m.tangent()), _np(m.vort())
    m.close()
    rv, rt, _ = _reference(256, 256, tangent=True)
    plain = G.recipe_model(256, 256, v, dz, src)
    plain.step(case.steps)
    et, ev, moved = rel_l2(gt, rt), rel_l2(gv, rv), rel_l2(plain.tangent(), rt)
    print("tangent of the split system, 256^2, %d steps: perturbation rel L2 = %.3g, vorticity %.3g; the split stage moves the float64 perturbation by %.3g"
          % (case.steps, et, ev, moved))
    assert moved >= F.SHIFT_BAR
    assert et <= 1e-5 and ev <= 1e-5


# ---- 8. refusals ----
def test_refusals():
    import xlab_fftbarotropic_amd as X
    nx = ny = 64
    name = "fb_model_set_forcing"
    good = dict(rate=1.0, k=12.0 * F.K1, width=1.5 * F.K1, seed=1, drag=0.0, hyper_nu=0.0, hyper_order=1)
    m = X.Model(nx, ny)
    m.set_vort(np.zeros((nx, ny), np.float32))
    _raises(m.forcing_budget, EINVAL, "fb_model_forcing_budget")
    _raises(lambda: m.forcing_increment(0), EINVAL, "fb_model_forcing_increment")
    nan, inf = float("nan"), float("inf")
    for key, value in (("rate", -1.0), ("rate", nan), ("rate", inf), ("drag", -1.0), ("drag", nan), ("hyper_nu", -1.0), ("hyper_nu", inf),
                       ("hyper_order", 0), ("hyper_order", 9), ("k", nan), ("k", -1.0), ("width", inf), ("width", -1.0), ("width", 12.0 * F.K1),
                       ("width", 13.0 * F.K1)):
        _raises(lambda: m.set_forcing(**dict(good, **{key: value})), EINVAL, name)
    assert "holds no mode" in _raises(lambda: m.set_forcing(**dict(good, k=12.3 * F.K1, width=1e-3 * F.K1)), EINVAL, name)
    assert "outside the dealiasing circle" in _raises(lambda: m.set_forcing(**dict(good, k=40.0 * F.K1, width=F.K1)), EINVAL, name)
    _raises(m.forcing_budget, EINVAL, "fb_model_forcing_budget")                       # a refused call sets nothing
    m.set_forcing(**good)
    assert "forcing is set" in _raises(lambda: m.record_adjoint(4), EUNSUPPORTED, "fb_model_adjoint_record")
    assert "forcing is set" in _raises(lambda: m.checkpoint_adjoint(2, 4), EUNSUPPORTED, "fb_model_adjoint_checkpoint")
    m.record_adjoint(0)
    m.checkpoint_adjoint(0)                                      # turning either off is no tape
    m.set_forcing()
    for turn_on, turn_off in ((lambda: m.record_adjoint(4), lambda: m.record_adjoint(0)), (lambda: m.checkpoint_adjoint(2, 4), lambda: m.checkpoint_adjoint(0))):
        turn_on()
        assert "tape" in _raises(lambda: m.set_forcing(**good), EUNSUPPORTED, name)
        _raises(lambda: m.set_forcing(drag=1e-3), EUNSUPPORTED, name)
        turn_off()
        m.set_forcing(**good)
        m.set_forcing()
    m.close()


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: every entry point of the split stage returns FB_EUNSUPPORTED under its own name"""
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
                for name, call in (("set_forcing", lambda: s.set_forcing(rate=1.0, k=F.RING_K, width=F.RING_WIDTH)), ("set_forcing", lambda: s.set_forcing(drag=1e-3)),
                                   ("set_forcing", s.set_forcing), ("forcing_budget", s.forcing_budget), ("forcing_increment", lambda: s.forcing_increment(0))):
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
        assert len(msgs[r]) == 5
        for name, msg in msgs[r]:
            assert msg is not None and msg.startswith(EUNSUPPORTED + "fb_slab_" + name + ": ") and "world > 1" in msg, msg


def test_slab_of_one_rank_matches_the_model():
    S = _slab()
    case = F.case_of(256, 256)
    out = []
    for cls in (None, S.EngineSlab):
        m = _gpu_model(case, cls=cls)
        inc = _np(m.forcing_increment(3))
        m.step(case.steps)
        out.append((_np(m.vort()), m.forcing_budget(), inc))
        m.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert out[0][1] == out[1][1] and out[0][1]["clock"] == case.steps
    assert np.array_equal(out[0][2], out[1][2])
    assert rel_l2(out[1][0], _reference(256, 256)[0]) <= 1e-5


# ---- the driver ----
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")


def _run_driver(d, n, v0, extra, steps=11):
    import subprocess
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--record-step", "10", "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode(), (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_forcing(tmp_path):
    """barotropic_main.out with the forcing flags at 256^2, 11 steps, a record every 10: forcing_budget_step_N.bin is the last file of
    each record in ./log, and it and vort_step_N.bin equal what the Python path gives, bit for bit; without the flags ./log is as it
    was; bad values and --world 2 end with exit status 2 and one line on stderr"""
    import subprocess
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n = 256
    v0 = X.make_field("kuo2004", n)
    kw = dict(rate=0.5, k=F.RING_K, width=F.RING_WIDTH, seed=F.SEED, drag=1e-3, hyper_nu=F.hyper_nu(n, n, 3.0), hyper_order=4)
    flags = ["--forcing-rate", repr(kw["rate"]), "--forcing-k", repr(kw["k"]), "--forcing-width", repr(kw["width"]), "--forcing-seed", str(kw["seed"]),
             "--drag", repr(kw["drag"]), "--hyper-nu", repr(kw["hyper_nu"]), "--hyper-order", "4"]
    rc, err, log = _run_driver(tmp_path / "run", n, v0, flags)
    assert rc == 0, err
    plain = ("vort_src_input", "vort", "psi", "u", "v")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 10) for name in plain + ("forcing_budget",)]
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_forcing(**kw)
    for s in range(11):
        if s % 10 == 0:
            out = tmp_path / "run" / "output"
            assert np.array_equal(_bits(np.fromfile(str(out / ("vort_step_%d.bin" % s)), dtype="<f4").reshape(n, n)), _bits(_np(m.vort()))), s
            g, b = np.fromfile(str(out / ("forcing_budget_step_%d.bin" % s)), dtype="<f8"), m.forcing_budget()
            print("driver, step %d: clock, dE_forc, dE_diss, dZ_forc, dZ_diss, N_ring = %s" % (s, g))
            assert g.shape == (6,) and list(g) == [float(b[k]) for k in X.Model.FORCING_BUDGET] and g[0] == s
        m.step(1)
    m.close()
    rc, err, log = _run_driver(tmp_path / "plain", n, v0, [])
    assert rc == 0 and log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 10) for name in plain], err
    for name, extra in (("world", flags + ["--world", "2", "--ranks-as-threads"]), ("rate", ["--forcing-rate", "-1"]), ("nan", ["--drag", "nan"]),
                        ("order", ["--hyper-nu", "1", "--hyper-order", "9"]), ("noring", ["--forcing-rate", "1"]),
                        ("empty", ["--forcing-rate", "1", "--forcing-k", repr(12.3 * F.K1), "--forcing-width", repr(1e-3 * F.K1)]),
                        ("seed", flags + ["--forcing-seed", "-3"])):
        rc, err, _ = _run_driver(tmp_path / name, n, v0, extra, steps=1)
        assert rc == 2, (name, rc, err)
        lines = err.strip().splitlines()                           # (the ring is judged on the grid: after the initial field has been read)
        assert lines[-1].startswith("--") and (len(lines) == 1 or name == "empty"), (name, err)
