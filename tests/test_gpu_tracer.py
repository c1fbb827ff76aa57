"""GPU tests of the passive tracer: fb_model_set_tracer / fb_model_get_tracer / fb_model_get_tracer_eddy_diffusivity (Model.set_tracer,
Model.tracer, Model.tracer_eddy_diffusivity) and their slab counterparts (EngineSlab.set_tracer_local, tracer_local,
tracer_eddy_diffusivity).

Every test goes through Model.set_tracer or EngineSlab.set_tracer_local.  Checked: a tracer set to the vorticity with kappa = nu
follows the vorticity (the decisive check that each stage uses that stage's velocity); a tracer that is not the vorticity against the
float64 reference of the coupled system (tests/tracer_numpy.py); the analytic decay in a steady cellular flow; the invariants of pure
advection; the vorticity step, the records and a captured step bit for bit what they are without a tracer; a slab against one GPU
bit for bit; the tracer's eddy diffusivity table.  The measured figures are printed, one line per case (pytest -s)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "xlab-fftbarotropic_amd", "host")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
NU = 6.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _np(t):
    return t.cpu().numpy()


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _rel(a, b):
    from ref_numpy import rel_l2
    return rel_l2(a, b)


def _offset_gaussian(n, ny=None):
    """the gaussian of make_field("gaussian"), moved off the vortices by a quarter of the domain in x and an eighth in y"""
    import xlab_fftbarotropic_amd as X
    g = X.make_field("gaussian", n, ny)
    return np.ascontiguousarray(np.roll(np.roll(g, g.shape[0] // 4, axis=0), g.shape[1] // 8, axis=1))


def test_twin_tracer_follows_the_vorticity():
    """1024^2 Kuo2004, c = zeta, kappa = nu: rel L2 (tracer, vorticity) <= 1e-5, the project's parity bar, after 10, 100 and 1000 steps.
    The two fields go through different kernels.  Measured on MI355X: see DESIGN.md, "Passive tracer"."""
    import xlab_fftbarotropic_amd as X
    n = 1024
    v0 = X.make_field("kuo2004", n)
    m = X.Model(n, n, nu=NU)
    m.set_vort(v0)
    m.set_tracer(v0, kappa=NU)
    assert _same(_np(m.tracer()), _np(m.vort()))
    done, errs = 0, []
    for steps in (10, 100, 1000):
        m.step(steps - done)
        done = steps
        v = _np(m.vort())
        err = _rel(_np(m.tracer()), v)
        errs.append(err)
        print("twin 1024^2 step %d: rel L2 (tracer, vort) = %.3g; vort moved from its start by %.3g" % (steps, err, _rel(v, v0)))
    assert all(e <= 1e-5 for e in errs), errs


@pytest.mark.parametrize("kappa", [0.0, 20.0])
def test_against_float64(kappa):
    """256^2 Kuo2004 with a tracer that is not the vorticity: rel L2 against the float64 coupled run <= 1e-5 at steps 10 and 100, and no
    worse than 4 times the vorticity's own error against the same run"""
    import xlab_fftbarotropic_amd as X
    from tracer_numpy import TracerModel64
    n = 256
    v0, c0 = X.make_field("kuo2004", n), _offset_gaussian(n)
    m = X.Model(n, n, nu=NU)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=kappa)
    r = TracerModel64(n, n, nu=NU, kappa=kappa)
    r.set_vort(v0)
    r.set_tracer(c0)
    done, res = 0, []
    for steps in (10, 100):
        m.step(steps - done)
        r.step(steps - done)
        done = steps
        et, ev = _rel(_np(m.tracer()), r.tracer()), _rel(_np(m.vort()), r.vort())
        res.append((et, ev))
        print("float64 256^2 kappa=%g step %d: tracer rel L2 = %.3g, vorticity rel L2 = %.3g, tracer moved by %.3g"
              % (kappa, steps, et, ev, _rel(r.tracer(), c0)))
    for et, ev in res:
        assert et <= 1e-5
        assert et <= 4 * ev


@pytest.mark.parametrize("nx,ny", [(256, 128), (128, 256)])
def test_analytic_decay(nx, ny):
    """the steady cellular flow of the CPU test: nu = 0, kappa = 50, 200 steps, against c0 R(z)^n, <= 1e-5"""
    import xlab_fftbarotropic_amd as X
    from tracer_numpy import cellular_flow, rk4_factor
    psi, zeta, k2 = cellular_flow(nx, ny, amp=1.0e6)
    kappa, dt, steps = 50.0, 3.0, 200
    m = X.Model(nx, ny, nu=0.0, dt=dt)
    m.set_vort(zeta.astype(np.float32))
    m.set_tracer(psi.astype(np.float32), kappa=kappa)
    m.step(steps)
    fac = rk4_factor(-kappa * k2 * dt) ** steps
    err = _rel(_np(m.tracer()), psi.astype(np.float32).astype(np.float64) * fac)
    print("decay %dx%d: rel L2 = %.3g (factor %.6f)" % (nx, ny, err, fac))
    assert err <= 1e-5


def test_invariants():
    """kappa = 0: mean of c and <c^2> after 100 steps at 256^2 within the float64 run's own drift plus 1e-5 relative; kappa > 0: <c^2>
    does not grow"""
    import xlab_fftbarotropic_amd as X
    from tracer_numpy import TracerModel64
    n = 256
    v0, c0 = X.make_field("kuo2004", n), _offset_gaussian(n)
    r = TracerModel64(n, n, nu=NU, kappa=0.0)
    r.set_vort(v0)
    r.set_tracer(c0)
    m = X.Model(n, n, nu=NU)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=0.0)
    a0 = _np(m.tracer()).astype(np.float64)
    mean0, sq0 = a0.mean(), (a0 * a0).mean()
    r0 = r.tracer()
    r.step(100)
    m.step(100)
    r1, a1 = r.tracer(), _np(m.tracer()).astype(np.float64)
    drift_mean = abs(r1.mean() - r0.mean())
    drift_sq = abs((r1 * r1).mean() - (r0 * r0).mean())
    scale = np.sqrt(sq0)                                         # the mean is measured against the field's rms
    dm, ds = abs(a1.mean() - mean0), abs((a1 * a1).mean() - sq0)
    print("invariants 256^2 kappa=0: mean drift %.3g (float64 %.3g, rms %.3g), <c^2> drift %.3g relative (float64 %.3g)"
          % (dm, drift_mean, scale, ds / sq0, drift_sq / sq0))
    assert dm <= drift_mean + 1e-5 * scale
    assert ds <= drift_sq + 1e-5 * sq0
    m.set_tracer(c0, kappa=20.0)
    prev = sq0
    for _ in range(5):
        m.step(20)
        a = _np(m.tracer()).astype(np.float64)
        sq = (a * a).mean()
        assert sq <= prev, (sq, prev)
        prev = sq
    print("invariants 256^2 kappa=20: <c^2> %.6g -> %.6g" % (sq0, prev))
    assert prev < sq0


@pytest.mark.parametrize("n", [1024, 4096])
def test_the_step_is_untouched(n):
    """vort() bit for bit what a run that never had a tracer gives: with a tracer set, with a tracer set and then removed, and in graph
    mode on a non-null stream with the tracer set between two step calls; the tracer of the graph-mode run equals the eager tracer"""
    import torch
    import xlab_fftbarotropic_amd as X
    v0 = X.make_field("kuo2004", n)
    c0 = _offset_gaussian(n)
    plain = X.Model(n, n)
    plain.set_vort(v0)
    plain.step(20)
    want = _np(plain.vort())
    info0 = plain.info()["hbm_bytes"]
    plain.close()

    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=20.0)
    assert m.info()["hbm_bytes"] > info0
    m.step(20)
    assert _same(_np(m.vort()), want)
    eager_tracer = _np(m.tracer())
    assert not _same(eager_tracer, c0)
    m.close()

    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=20.0)
    m.step(7)
    m.set_tracer(None)
    assert m.info()["hbm_bytes"] == info0
    with pytest.raises(X.FftBaroError):
        m.tracer()
    m.step(13)
    assert _same(_np(m.vort()), want)
    m.close()

    # graph mode: 8 plain steps, then the tracer, then 20 steps with it; against eager runs of the same sequence
    e = X.Model(n, n)
    e.set_vort(v0)
    e.step(8)
    e.set_tracer(c0, kappa=20.0)
    e.step(12)
    assert _same(_np(e.vort()), want)
    e.step(8)
    want28, tr28 = _np(e.vort()), _np(e.tracer())
    e.close()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = X.Model(n, n)
        g.set_vort(v0)
        g.use_graph(True)
        g.step(8)
        g.set_tracer(c0, kappa=20.0)
        g.step(12)
        got20 = _np(g.vort())
        g.step(8)
        got28, gtr = _np(g.vort()), _np(g.tracer())
        g.set_tracer(None)
        g.step(4)
        g.fop.synchronize()
        g.close()
    assert _same(got20, want)
    assert _same(got28, want28)
    assert _same(gtr, tr28)


def test_records_and_tracer_do_not_disturb_each_other():
    import xlab_fftbarotropic_amd as X
    n = 512
    v0, c0 = X.make_field("kuo2004", n), _offset_gaussian(n)

    def records(m):
        out = [m.vort()] + list(m.diag()) + list(m.okubo_weiss()) + [m.eddy_diffusivity(64), m.pressure(), m.spectra()]
        return [_np(t) for t in out]

    a = X.Model(n, n)
    a.set_vort(v0)
    a.step(5)
    plain = records(a)
    b = X.Model(n, n)
    b.set_vort(v0)
    b.set_tracer(c0, kappa=20.0)
    b.step(5)
    t1 = _np(b.tracer())
    with_tracer = records(b)
    for k, (p, q) in enumerate(zip(plain, with_tracer)):
        if k == 6:
            # the eddy diffusivity table: its sums (columns 5-8) come from float64 LDS atomics and repeat from call to call "within
            # rounding" only, with or without a tracer (tests/test_gpu_eddy_diffusivity.py::test_record_has_no_side_effects): edges and
            # counts bit for bit, the sums to that record's own bar of 1e-9
            assert np.array_equal(p[:, :5].view(np.uint64), q[:, :5].view(np.uint64))
            assert np.all(np.abs(p[:, 5:] - q[:, 5:]) <= 1e-9 * np.abs(p[:, 5:]))
            continue
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8)), k
    assert _same(_np(b.tracer()), t1)                          # twice the same bits, with every record in between
    assert _same(_np(b.tracer()), t1)
    b.step(5)
    c = X.Model(n, n)
    c.set_vort(v0)
    c.set_tracer(c0, kappa=20.0)
    c.step(10)
    assert _same(_np(b.tracer()), _np(c.tracer()))
    assert _same(_np(b.vort()), _np(c.vort()))
    # fb_model_set_vort leaves the tracer in place
    before = _np(c.tracer())
    c.set_vort(v0)
    assert _same(_np(c.tracer()), before)


def _slab_run(nx, ny, world, steps, v0, c0, kappa, env, nbins, src=None, **model_kw):
    import threading
    S = _slab()
    hub = S.local_hub(world)
    out, errs = [None] * world, [None] * world

    def work(r):
        try:
            m = S.EngineSlab(nx, ny, rank=r, world=world, transport=hub, **model_kw)
            try:
                m.set_vort_local(S.local_rows(v0, r, world))
                if src is not None:
                    m.set_source_local(S.local_rows(src, r, world))
                m.set_tracer_local(S.local_rows(c0, r, world), kappa)
                m.step(steps)
                tr = m.tracer_local().cpu().numpy()
                m.okubo_weiss_local()                                     # another record in between, on the shared workspace
                out[r] = (tr, m.vort_local().cpu().numpy(), m.tracer_eddy_diffusivity(nbins).cpu().numpy(), m.tracer_local().cpu().numpy())
            finally:
                m.close()
        except BaseException as e:                                          # noqa: BLE001 -- re-raised below
            errs[r] = e
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        S.local_hub_destroy(hub)
    for e in errs:
        if e is not None:
            raise e
    return out


def _col_groups(nx, ny, world, env):
    """the number of active column groups of a rank in this plan (fb_slab_col_groups; 2 = the stage is pipelined by column groups)"""
    import ctypes
    import xlab_fftbarotropic_amd as X
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ng, cols = ctypes.c_int(), (ctypes.c_int * 2)()
        assert X.lib().fb_slab_col_groups(nx, ny, world, ctypes.byref(ng), cols) == 0
        return ng.value
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# The cases of NOISY run the inputs of the tracer's path matrix (tracer_numpy.noisy_inputs: never-dealiased noise on both fields, a
# vorticity source, the recipe's dt) in the place of Kuo2004 and the gaussian: 256^2 and 384 x 192 keep the state in the 3-pass layout
# (N2 < 32; 384: N1 = 24), 128 x 4096 has k_rowq on every rank.
NOISY = {(2, 256, 256), (4, 384, 192), (2, 128, 4096)}


# groups: the plan each case gets.  The default plan has one active column group at every size here; the stage pipelined by column
# groups (slab_stage_groups) is forced at 8192 x 256 on 2, 4 and 8 ranks.  8192 x 256 has frozen columns at every world size.
@pytest.mark.parametrize("world,nx,ny,env,groups", [(2, 1024, 1024, {}, 1), (4, 1024, 1024, {}, 1), (8, 1024, 1024, {}, 1),
                                                    (2, 8192, 256, {}, 1), (4, 8192, 256, {}, 1), (8, 8192, 256, {}, 1),
                                                    (2, 8192, 256, {"FB_SLAB_COL_GROUPS": "2"}, 2), (4, 8192, 256, {"FB_SLAB_COL_GROUPS": "2"}, 2),
                                                    (8, 8192, 256, {"FB_SLAB_COL_GROUPS": "2"}, 2),
                                                    (2, 256, 256, {}, 1), (4, 384, 192, {}, 1), (2, 128, 4096, {}, 1)])
def test_slab_equals_single_gpu(world, nx, ny, env, groups):
    """ranks as threads on one GPU: tracer_local() over the ranks equals the one-GPU tracer() bit for bit after 10 steps, so does the
    vorticity; the tracer's eddy diffusivity table has the one-GPU counts (columns 0-4) on every rank, columns 5-8 to 1e-9"""
    import xlab_fftbarotropic_amd as X
    assert _col_groups(nx, ny, world, env) == groups
    nbins, kappa = 64, 20.0
    if (world, nx, ny) in NOISY:
        import tracer_numpy as T
        v0, c0, src = T.noisy_inputs(nx, ny, 3e-2)
        kw = {"nu": T.RECIPE_NU, "dt": T.recipe_dt(nx, ny)}
    else:
        v0, c0, src, kw = X.make_field("kuo2004", nx, ny), _offset_gaussian(nx, ny), None, {}
    one = X.Model(nx, ny, **kw)
    one.set_vort(v0)
    if src is not None:
        one.set_source(src)
    one.set_tracer(c0, kappa=kappa)
    one.step(10)
    wt, wv, wk = _np(one.tracer()), _np(one.vort()), _np(one.tracer_eddy_diffusivity(nbins))
    one.close()
    assert np.isfinite(wt).all() and not _same(wt, c0)
    out = _slab_run(nx, ny, world, 10, v0, c0, kappa, env, nbins, src, **kw)
    tr = np.concatenate([o[0] for o in out], axis=0)
    vo = np.concatenate([o[1] for o in out], axis=0)
    again = np.concatenate([o[3] for o in out], axis=0)
    assert _same(tr, wt)
    assert _same(again, wt)
    assert _same(vo, wv)
    for r in range(world):
        t = out[r][2]
        assert np.isfinite(t).all()
        assert np.array_equal(t[:, :5].view(np.uint64), wk[:, :5].view(np.uint64)), r
        assert np.all(np.abs(t[:, 5:] - wk[:, 5:]) <= 1e-9 * np.abs(wk[:, 5:])), r
    print("slab world %d %dx%d: tracer, vorticity bitwise equal to one GPU; table counts equal" % (world, nx, ny))


def test_tracer_eddy_diffusivity():
    """c = zeta at step 0 and kappa = nu: the table of eddy_diffusivity(), columns 0-4 bit for bit and 5-8 to 1e-9; a circular gaussian
    tracer: K_eff = kappa within the tolerance tests/test_gpu_eddy_diffusivity.py uses for circular contours"""
    import xlab_fftbarotropic_amd as X
    n = 1024
    v0 = X.make_field("kuo2004", n)
    m = X.Model(n, n, nu=NU)
    m.set_vort(v0)
    m.set_tracer(v0, kappa=NU)
    want = _np(m.eddy_diffusivity(128))
    got, c, g = (_np(t) for t in m.tracer_eddy_diffusivity(128, fields=True))
    assert np.array_equal(got[:, :5].view(np.uint64), want[:, :5].view(np.uint64))
    assert np.all(np.abs(got[:, 5:] - want[:, 5:]) <= 1e-9 * np.abs(want[:, 5:]))
    assert _same(c, _np(m.tracer()))
    assert np.isfinite(got).all()
    lx = ly = 6e5
    kappa = 20.0
    x = ((np.arange(n) - n / 2) * (lx / n))[:, None]
    y = ((np.arange(n) - n / 2) * (ly / n))[None, :]
    r0 = lx / 8
    m.set_tracer(np.exp(-(x * x + y * y) / (r0 * r0)).astype(np.float32), kappa=kappa)
    t = _np(m.tracer_eddy_diffusivity(64))
    a, re, k = t[:, 3], t[:, 7], t[:, 8] / np.float32(kappa)
    sel = (re > 0.5 * r0) & (re < 2 * r0)
    mean = (k[sel] * a[sel]).sum() / a[sel].sum()
    print("tracer eddy diffusivity, circular gaussian: %d bins, area-weighted K/kappa %.5f, range %.4f-%.4f" % (int(sel.sum()), mean, k[sel].min(), k[sel].max()))
    assert sel.sum() >= 8
    assert abs(mean - 1) <= 0.01
    assert np.all(np.abs(k[sel] - 1) <= 0.25)


def test_errors():
    import xlab_fftbarotropic_amd as X
    n = 256
    m = X.Model(n, n)
    m.set_vort(X.make_field("kuo2004", n))
    with pytest.raises(X.FftBaroError):
        m.tracer()
    with pytest.raises(X.FftBaroError):
        m.tracer_eddy_diffusivity(16)
    c0 = _offset_gaussian(n)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(X.FftBaroError):
            m.set_tracer(c0, kappa=bad)
    m.set_tracer(c0, kappa=0.0)
    for nb in (1, 4097):
        with pytest.raises(X.FftBaroError):
            m.tracer_eddy_diffusivity(nb)
    m.step(2)
    assert np.isfinite(_np(m.tracer())).all()


def _run_driver(d, n, v0, c0, extra, steps=101):
    import subprocess
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    if c0 is not None:
        c0.tofile(str(d / "input" / "c.bin"))
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
    return r.returncode, r.stdout, (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_tracer(tmp_path):
    """barotropic_main.out --tracer c.bin --tracer-kappa 20 at 256^2: tracer_step_N.bin equals Model.tracer() at the same steps, on one
    GPU and with --world 2; ./log ends each record with the file (and with the tracer's table after it under --dump-eddy-diffusivity);
    K < 0 is refused with exit status 2.  Without the flag the run is what it was before the option existed: the same files and ./log
    lines as the driver has always written, each field file equal bit for bit to the record of a model that never had a tracer (what
    tests/test_host_cpp.py pins for the driver), and the same stdout as the run with the flag."""
    import subprocess
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, nbins, kappa = 256, 64, 20.0
    v0, c0 = X.make_field("kuo2004", n), _offset_gaussian(n)
    base = ("vort_src_input", "vort", "psi", "u", "v")
    rc, out_plain, log = _run_driver(tmp_path / "plain", n, v0, None, [])
    assert rc == 0
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in base]
    assert sorted(os.listdir(str(tmp_path / "plain" / "output"))) == sorted("%s_step_%d.bin" % (name, s) for s in (0, 100) for name in base)
    runs = {}
    for tag, extra in (("one", []), ("two", ["--world", "2", "--ranks-as-threads"])):
        rc, out, log = _run_driver(tmp_path / tag, n, v0, c0, ["--tracer", "c.bin", "--tracer-kappa", str(kappa)] + extra)
        assert rc == 0, tag
        assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in base + ("tracer",)], tag
        if tag == "one":
            assert out == out_plain
        runs[tag] = tmp_path / tag
    rc, _, log = _run_driver(tmp_path / "keff", n, v0, c0, ["--tracer", "c.bin", "--tracer-kappa", str(kappa), "--dump-eddy-diffusivity", "--keff-bins", str(nbins)])
    assert rc == 0
    order = base + ("eddy_diffusivity", "tracer", "tracer_eddy_diffusivity")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in order]
    rc2, _, log2 = _run_driver(tmp_path / "keff2", n, v0, c0, ["--tracer", "c.bin", "--tracer-kappa", str(kappa), "--dump-eddy-diffusivity", "--keff-bins", str(nbins),
                                                                "--world", "2", "--ranks-as-threads"])
    assert rc2 == 0 and log2 == log
    m = X.Model(n, n)
    m.set_vort(v0)
    m.set_tracer(c0, kappa=kappa)
    p = X.Model(n, n)
    p.set_vort(v0)
    for s in (0, 100):
        want = _np(m.tracer())
        for tag, d in list(runs.items()) + [("keff", tmp_path / "keff"), ("keff2", tmp_path / "keff2")]:
            got = np.fromfile(str(d / "output" / ("tracer_step_%d.bin" % s)), dtype="<f4").reshape(n, n)
            assert _same(got, want), (tag, s)
        wt = _np(m.tracer_eddy_diffusivity(nbins))
        for tag in ("keff", "keff2"):
            f = tmp_path / tag / "output" / ("tracer_eddy_diffusivity_step_%d.bin" % s)
            assert os.path.getsize(str(f)) == nbins * 9 * 8
            t = np.fromfile(str(f), dtype="<f8").reshape(nbins, 9)
            assert np.array_equal(t[:, :5].view(np.uint64), wt[:, :5].view(np.uint64)), (tag, s)
            assert np.all(np.abs(t[:, 5:] - wt[:, 5:]) <= 1e-9 * np.abs(wt[:, 5:])), (tag, s)
        psi, u, v = p.diag()
        for name, t in (("vort", p.vort()), ("psi", psi), ("u", u), ("v", v)):
            for tag in ("plain", "one"):
                got = np.fromfile(str(tmp_path / tag / "output" / ("%s_step_%d.bin" % (name, s))), dtype="<f4").reshape(n, n)
                assert _same(got, _np(t)), (name, tag, s)
        m.step(100)
        p.step(100)
    for bad in ("-1", "nan", "x"):
        rc, _, _ = _run_driver(tmp_path / ("bad" + bad), n, v0, c0, ["--tracer", "c.bin", "--tracer-kappa", bad], steps=1)
        assert rc == 2, bad
