"""GPU tests of the effective eddy diffusivity record output: fb_model_get_eddy_diffusivity (Model.eddy_diffusivity),
fb_slab_get_eddy_diffusivity (EngineSlab.eddy_diffusivity) and the driver's --dump-eddy-diffusivity.

The vorticity is the tracer (Nakamura 1996, Hendricks and Schubert 2009), kappa = nu.  Checked against the circular-vortex limit
K_eff = nu on anisotropic grids (both orientations, so that swapped x and y coefficients fail), against numpy's evaluation of the
definition (include/fftbaro.h) on the returned fields, for bitwise agreement of the vorticity with the vorticity record and of the
slab and driver paths with the one-GPU path.  The worst measured errors are printed, one line per case (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
FB_EINVAL = 1
NU = 6.5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _keff(m, nbins, fields=False):
    out = m.eddy_diffusivity(nbins, fields=fields)
    return tuple(t.cpu().numpy() for t in out) if fields else out.cpu().numpy()


def _table64(q, g, nbins, lx, ly, nu):
    """The definition of include/fftbaro.h evaluated in numpy on the engine's float32 zeta and g."""
    nx, ny = q.shape
    lx, ly, nu = float(np.float32(lx)), float(np.float32(ly)), float(np.float32(nu))
    dx, dy = lx / nx, ly / ny
    q = q.ravel()
    qmin, qmax = float(q.min()), float(q.max())
    if qmax > qmin:
        t = (q.astype(np.float64) - qmin) * (nbins / (qmax - qmin))
        b = np.clip(np.floor(t), 0, nbins - 1).astype(np.int64)
    else:
        b = np.zeros(q.size, dtype=np.int64)
    n = np.bincount(b, minlength=nbins).astype(np.float64)
    s = np.bincount(b, weights=g.ravel().astype(np.float64), minlength=nbins)
    dq = (qmax - qmin) / nbins
    i = np.arange(nbins, dtype=np.float64)
    a = n * dx * dy
    age = np.cumsum(a[::-1])[::-1]
    sb = dx * dy * s
    with np.errstate(divide="ignore", invalid="ignore"):
        le2 = np.where((n > 0) & (dq > 0), sb * a / (dq * dq), 0.0)
        re = np.sqrt((age - a / 2) / np.pi)
        k = np.where((le2 > 0) & (re > 0), nu * le2 / (4 * np.pi * np.pi * re * re), 0.0)
    return np.stack([qmin + i * dq, qmin + (i + 1) * dq, n, a, age, sb, le2, re, k], axis=1)


def _close(a, b, rtol=1e-9):
    """|a - b| <= rtol |b| element by element (exact zeros must be zeros)"""
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


def _check_table(t, want, nx, ny, lx, ly):
    assert t.shape == want.shape and t.dtype == np.float64
    assert np.isfinite(t).all()
    assert np.array_equal(t[:, :5].view(np.uint64), want[:, :5].view(np.uint64))
    for c in range(5, 9):
        assert _close(t[:, c], want[:, c]), c
    assert t[:, 2].sum() == nx * ny
    assert abs(t[0, 4] - float(np.float32(lx)) * float(np.float32(ly))) <= 1e-12 * t[0, 4]


@pytest.mark.parametrize("lx,ly,nx,ny", [(6e5, 3e5, 1024, 1024), (3e5, 6e5, 1024, 1024), (6e5, 3e5, 1024, 512)])
def test_circular_vortex_anisotropic(lx, ly, nx, ny):
    import xlab_fftbarotropic_amd as X
    dx, dy = lx / nx, ly / ny
    x = ((np.arange(nx) - nx / 2) * dx)[:, None]
    y = ((np.arange(ny) - ny / 2) * dy)[None, :]
    r0 = min(lx, ly) / 8
    m = X.Model(nx, ny, Lx=lx, Ly=ly, nu=NU)
    m.set_vort((1e-3 * np.exp(-(x * x + y * y) / (r0 * r0))).astype(np.float32))
    t = _keff(m, 64)
    a, re, k = t[:, 3], t[:, 7], t[:, 8] / np.float32(NU)
    sel = (re > 0.5 * r0) & (re < 2 * r0)
    mean = (k[sel] * a[sel]).sum() / a[sel].sum()
    print("eddy diffusivity gaussian %dx%d Lx=%g Ly=%g: %d bins, area-weighted K/nu %.5f, range %.4f-%.4f"
          % (nx, ny, lx, ly, int(sel.sum()), mean, k[sel].min(), k[sel].max()))
    assert sel.sum() >= 8
    assert abs(mean - 1) <= 0.01
    assert np.all(np.abs(k[sel] - 1) <= 0.25)


def _grad2_64(spec, gx, gy):
    nx, hy = spec.shape
    ny = 2 * (hy - 1)
    s = spec.astype(np.complex128)
    f = lambda z: np.fft.irfft2(z, s=(nx, ny))                             # c2r / GRIDS
    zx = f(1j * gx.astype(np.float64)[:, None] * s)
    zy = f(1j * gy.astype(np.float64)[None, :hy] * s)
    return zx * zx + zy * zy


@pytest.mark.parametrize("nx,ny,kind,steps", [(256, 256, "kuo2004", 5), (768, 768, "elliptic", 3), (256, 512, "elliptic", 3),
                                              (512, 192, "elliptic", 3)])
def test_exact_against_numpy(nx, ny, kind, steps):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, dt=3.0 * 256 / max(nx, ny), nu=NU)
    m.set_vort(X.make_field(kind, nx, ny))
    m.step(steps)
    nbins = 200
    t, zeta, g = _keff(m, nbins, fields=True)
    assert np.array_equal(_bits(zeta), _bits(m.vort().cpu().numpy()))
    gx, gy, _, _, _ = m.fop.tables()
    g64 = _grad2_64(m.spectrum().cpu().numpy(), gx, gy)
    err = np.abs(g - g64).max() / g64.max()
    print("eddy diffusivity %dx%d %s: max|g - g64|/max g64 %.2e" % (nx, ny, kind, err))
    assert err <= 1e-5
    _check_table(t, _table64(zeta, g, nbins, 6e5, 6e5, NU), nx, ny, 6e5, 6e5)
    t2 = _keff(m, nbins)                                                   # without fields: the model's own record buffers
    assert np.array_equal(t2[:, :5].view(np.uint64), t[:, :5].view(np.uint64))


@pytest.mark.parametrize("nbins", [2, 4096])
def test_bin_count_limits(nbins):
    import xlab_fftbarotropic_amd as X
    n = 256
    m = X.Model(n, n, nu=NU)
    m.set_vort(X.make_field("kuo2004", n))
    t, zeta, g = _keff(m, nbins, fields=True)
    _check_table(t, _table64(zeta, g, nbins, 6e5, 6e5, NU), n, n, 6e5, 6e5)


@pytest.mark.parametrize("value", [0.0, 2.0 ** -12])
def test_degenerate_fields(value):
    import xlab_fftbarotropic_amd as X
    n = 256
    m = X.Model(n, n, nu=NU)
    m.set_vort(np.full((n, n), value, dtype=np.float32))
    t, zeta, g = _keff(m, 32, fields=True)
    assert np.isfinite(t).all()
    _check_table(t, _table64(zeta, g, 32, 6e5, 6e5, NU), n, n, 6e5, 6e5)
    exact = bool(np.all(zeta == np.float32(value)))
    print("eddy diffusivity constant %g: the field comes back %s" % (value, "exactly constant" if exact else "with rounding spread"))
    if value == 0.0:
        assert exact
    if not exact:                                                           # (then it is binned as any field is: checked above)
        return
    assert np.all(g == 0)
    assert t[0, 2] == n * n and np.all(t[1:, 2] == 0)
    assert np.all(t[:, 0] == value) and np.all(t[:, 1] == value)
    assert np.all(t[:, 6] == 0) and np.all(t[:, 8] == 0)


def test_record_has_no_side_effects():
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("kuo2004", n)
    ref = X.Model(n, n)
    ref.set_vort(v0)
    ref.step(20)
    want = ref.vort().cpu().numpy()
    m = X.Model(n, n)
    m.set_vort(v0)
    m.step(10)
    vort0 = m.vort().cpu().numpy()
    t0 = _keff(m, 128)
    assert np.array_equal(_bits(m.vort().cpu().numpy()), _bits(vort0))
    t1 = _keff(m, 128)                                                     # repeatable: edges and counts bitwise, sums within rounding
    assert np.array_equal(t1[:, :5].view(np.uint64), t0[:, :5].view(np.uint64))
    for c in range(5, 9):
        assert _close(t1[:, c], t0[:, c]), c
    _keff(m, 4096)                                                         # (grows the reduction buffers)
    assert np.array_equal(_keff(m, 128)[:, :5].view(np.uint64), t0[:, :5].view(np.uint64))
    m.step(10)
    assert np.array_equal(_bits(m.vort().cpu().numpy()), _bits(want))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = X.Model(n, n)
        g.fop.use_current_stream()
        g.use_graph(True)
        g.set_vort(v0)
        g.step(5)
        g.step(5)                                                           # captured and replayed
        tg = g.eddy_diffusivity(128)                                        # between replays, on the model's stream
        g.step(10)
        got = g.vort().cpu().numpy()
        tg = tg.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(tg[:, :5].view(np.uint64), t0[:, :5].view(np.uint64))


def _slab_keff(n, world, steps, v0, env, nbins):
    import threading
    S = _slab()
    hub = S.local_hub(world)
    out, errs = [None] * world, [None] * world

    def work(r):
        try:
            m = S.EngineSlab(n, n, rank=r, world=world, transport=hub)
            try:
                m.set_vort_local(S.local_rows(v0, r, world))
                m.step(steps)
                out[r] = tuple(a.cpu().numpy() for a in m.eddy_diffusivity(nbins, fields=True))
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


@pytest.mark.parametrize("world,n,env", [(2, 256, {}), (4, 768, {}), (8, 512, {"FB_SLAB_COL_GROUPS": "2"}),
                                         (4, 1024, {"FB_SLAB_COL_GROUPS": "2"}), (2, 512, {"FB_SLAB_FIELD_GROUPS": "2"})])
def test_slab_equals_single_gpu(world, n, env):
    import xlab_fftbarotropic_amd as X
    v0 = X.make_field("kuo2004", n)
    ref = X.Model(n, n)
    ref.set_vort(v0)
    ref.step(3)
    want_t, want_z, want_g = _keff(ref, 256, fields=True)
    out = _slab_keff(n, world, 3, v0, env, 256)
    assert np.array_equal(_bits(np.concatenate([o[1] for o in out])), _bits(want_z))
    assert np.array_equal(_bits(np.concatenate([o[2] for o in out])), _bits(want_g))
    for o in out[1:]:
        assert np.array_equal(o[0].view(np.uint64), out[0][0].view(np.uint64))
    t = out[0][0]
    assert np.array_equal(t[:, :3].view(np.uint64), want_t[:, :3].view(np.uint64))
    for c in range(3, 9):
        assert _close(t[:, c], want_t[:, c]), c


def _run_driver(d, n, v0, extra):
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "101"] + extra,
                   cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=300)
    return (d / "log").read_text().split()


def test_driver_dump_eddy_diffusivity(tmp_path):
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, nbins = 256, 128
    v0 = X.make_field("elliptic", n)
    runs = {}
    for tag, extra in (("one", []), ("two", ["--world", "2", "--ranks-as-threads"])):
        log = _run_driver(tmp_path / tag, n, v0, ["--dump-eddy-diffusivity", "--keff-bins", str(nbins)] + extra)
        order = ("vort_src_input", "vort", "psi", "u", "v", "eddy_diffusivity")
        assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in order], tag
        runs[tag] = tmp_path / tag
    m = X.Model(n, n)
    m.set_vort(v0)
    for s in (0, 100):
        want = _keff(m, nbins)
        for tag, d in runs.items():
            f = d / "output" / ("eddy_diffusivity_step_%d.bin" % s)
            assert os.path.getsize(str(f)) == nbins * 9 * 8
            t = np.fromfile(str(f), dtype="<f8").reshape(nbins, 9)
            assert np.array_equal(t[:, :3].view(np.uint64), want[:, :3].view(np.uint64)), (tag, s)
            for c in range(3, 9):
                assert _close(t[:, c], want[:, c]), (tag, s, c)
        m.step(100)
    log = _run_driver(tmp_path / "ow", n, v0, ["--dump-okubo-weiss", "--dump-eddy-diffusivity", "--keff-bins", str(nbins)])
    order = ("vort_src_input", "vort", "psi", "u", "v", "okubo_weiss", "tau_fil", "eddy_diffusivity")
    assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in order]


def test_errors():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    m = X.Model(256, 256)
    m.set_vort(X.make_field("elliptic", 256))
    t = m.torch.empty((4097, 9), dtype=m.torch.float64, device="cuda")
    tp = ctypes.c_void_p(t.data_ptr())
    assert L.fb_model_get_eddy_diffusivity(m._h, 256, None, None, None) == FB_EINVAL
    assert L.fb_model_get_eddy_diffusivity(m._h, 1, tp, None, None) == FB_EINVAL
    assert L.fb_model_get_eddy_diffusivity(m._h, 4097, tp, None, None) == FB_EINVAL
    assert b"nbins" in L.fb_last_error()
    with pytest.raises(X.FftBaroError):
        m.eddy_diffusivity(1)
    s = ctypes.c_void_p()
    assert L.fb_slab_create(ctypes.byref(s), 256, 256, 6e5, 6e5, 6.5, 3.0, 0, 2) == 0
    try:
        assert L.fb_slab_get_eddy_diffusivity(s, 256, tp, None, None) == FB_EINVAL
        assert b"not connected" in L.fb_last_error()
    finally:
        L.fb_slab_destroy(s)
