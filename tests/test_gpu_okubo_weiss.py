"""GPU tests of the Okubo-Weiss record output: fb_model_get_okubo_weiss (Model.okubo_weiss), fb_slab_get_okubo_weiss_local
(EngineSlab.okubo_weiss_local) and the driver's --dump-okubo-weiss.

W = 4 (psi_xy^2 - psi_xx psi_yy) = S1^2 + S2^2 - zeta^2 and tau_fil = 2 / sqrt(W) (+inf where W <= 0) of the flow u = -psi_y,
v = psi_x, psi_c = invertLaplacian(vort_c).  Checked against an analytic field on an anisotropic, non-square domain (both
orientations, so that swapped x and y coefficients fail one of them), against float64 numpy built from the engine's own spectrum,
against the reference's operators composed in float32, and for bitwise agreement between the one-GPU, slab and driver paths.
The worst measured errors are printed, one line per case (pytest -s)."""
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


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _ow(m):
    w, tau = m.okubo_weiss()
    return w.cpu().numpy(), tau.cpu().numpy()


def _second_derivatives64(spec, gx, gy, lap):
    """psi_xx, psi_yy, psi_xy in float64 from a natural half spectrum [nx][ny/2+1] and the engine's coefficient tables."""
    nx, hy = spec.shape
    ny = 2 * (hy - 1)
    lap64 = lap.astype(np.float64).copy()
    lap64[0, 0] = 1.0                                                       # fftwfop.cpp:112-117
    psi = spec.astype(np.complex128) / lap64
    kx = gx.astype(np.float64)[:, None]
    ky = gy.astype(np.float64)[None, :]
    f = lambda s: np.fft.irfft2(s, s=(nx, ny))                             # c2r / GRIDS
    return f(-kx * kx * psi), f(-ky * ky * psi), f(-kx * ky * psi)


@pytest.mark.parametrize("lx,ly", [(6e5, 3e5), (3e5, 6e5)])
def test_analytic_anisotropic_non_square(lx, ly):
    import xlab_fftbarotropic_amd as X
    nx, ny = 256, 128
    kx, ky = 2 * np.pi * 3 / lx, 2 * np.pi * 2 / ly
    A = 1e-4 / (kx * kx + ky * ky)
    x = np.arange(nx)[:, None] * (lx / nx)
    y = np.arange(ny)[None, :] * (ly / ny)
    psi = A * np.sin(kx * x) * np.sin(ky * y)
    m = X.Model(nx, ny, Lx=lx, Ly=ly)
    m.set_vort((-(kx * kx + ky * ky) * psi).astype(np.float32))
    w, tau = _ow(m)
    w_ex = 4 * A * A * kx * kx * ky * ky * (np.cos(kx * x) ** 2 - np.sin(ky * y) ** 2)
    wmax = np.abs(w_ex).max()
    err_w = np.abs(w - w_ex).max() / wmax
    big = w_ex > 1e-2 * w_ex.max()
    tau_ex = 2 / np.sqrt(w_ex[big])
    err_tau = (np.abs(tau[big] - tau_ex) / tau_ex).max()
    print("okubo-weiss analytic %dx%d Lx=%g Ly=%g: max|W-W_exact|/max|W_exact| %.2e, worst tau rel err %.2e" % (nx, ny, lx, ly, err_w, err_tau))
    assert err_w <= 1e-5
    assert err_tau <= 1e-5
    assert not np.isnan(tau).any() and np.array_equal(np.isinf(tau), w <= 0)


@pytest.mark.parametrize("nx,ny,kind", [(256, 256, "elliptic"), (768, 768, "kuo2004"), (1024, 1024, "elliptic"), (4096, 4096, "kuo2004"),
                                        (128, 16384, "elliptic"), (16384, 64, "elliptic")])
def test_against_fp64_from_the_engine_spectrum(nx, ny, kind):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, dt=3.0 * 256 / max(nx, ny))
    m.set_vort(X.make_field(kind, nx, ny))
    m.step(20)
    w, tau = _ow(m)
    spec = m.spectrum().cpu().numpy()
    gx, gy, lap, _, _ = m.fop.tables()
    xx, yy, xy = _second_derivatives64(spec, gx, gy, lap)
    w64 = 4 * (xy * xy - xx * yy)
    smax = ((2 * xy) ** 2 + (xx - yy) ** 2 + (xx + yy) ** 2).max()
    err_w = np.abs(w - w64).max() / smax
    big = w64 >= 1e-2 * smax
    tau64 = 2 / np.sqrt(w64[big])
    err_tau = (np.abs(tau[big] - tau64) / tau64).max() if big.any() else 0.0
    clear = np.abs(w64) >= 1e-4 * smax
    print("okubo-weiss %dx%d %s vs fp64: max|W-W64|/Smax %.2e, worst tau rel err %.2e (%d points with W64 >= 1e-2 Smax)"
          % (nx, ny, kind, err_w, err_tau, int(big.sum())))
    assert not np.isnan(w).any() and not np.isnan(tau).any()
    assert err_w <= 1e-5
    assert err_tau <= 1e-4
    assert np.array_equal(np.isinf(tau)[clear], (w64 <= 0)[clear])
    assert np.array_equal(np.isinf(tau), w <= 0)


def test_against_reference_operators_in_float32():
    import oracle_py as O
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    mo = O.Model(n, n)
    mo.set_vort(O.make_field("elliptic", n))
    mo.step(100)
    vc = mo.spectrum()
    ops = O.Operators(n, n, 6e5, 6e5)
    g = np.float32(n * n)
    psi = ops.invertLaplacian(vc)
    c2r = lambda s: O.c2r(s, n) / g
    s1 = np.float32(-2) * c2r(ops.gradx(ops.grady(psi)))
    xx, yy = ops.gradx(ops.gradx(psi)), ops.grady(ops.grady(psi))
    s2 = c2r(xx - yy)
    zeta = c2r(xx + yy)
    w_ref = s1 * s1 + s2 * s2 - zeta * zeta
    smax = (s1.astype(np.float64) ** 2 + s2.astype(np.float64) ** 2 + zeta.astype(np.float64) ** 2).max()
    m = X.Model(n, n)
    m.set_spectrum(torch.from_numpy(np.ascontiguousarray(vc)).cuda())
    w, _ = _ow(m)
    err = np.abs(w.astype(np.float64) - w_ref).max() / smax
    print("okubo-weiss 256^2 after 100 oracle steps vs the reference's operators in float32: max|W-W_ref|/Smax %.2e" % err)
    assert err <= 1e-5


def test_record_has_no_side_effects():
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("elliptic", n)
    ref = X.Model(n, n)
    ref.set_vort(v0)
    ref.step(20)
    want = ref.vort().cpu().numpy()
    m = X.Model(n, n)
    m.set_vort(v0)
    m.step(10)
    vort0, diag0 = m.vort().cpu().numpy(), [t.cpu().numpy() for t in m.diag()]
    w0, tau0 = _ow(m)
    assert np.array_equal(_bits(m.vort().cpu().numpy()), _bits(vort0))
    assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(m.diag(), diag0))
    w1, tau1 = _ow(m)                                                       # repeatable: the record buffers start from the state every time
    assert np.array_equal(_bits(w1), _bits(w0)) and np.array_equal(_bits(tau1), _bits(tau0))
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
        wg, _ = g.okubo_weiss()                                             # between replays, on the model's stream
        g.step(10)
        got = g.vort().cpu().numpy()
        wg = wg.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(wg), _bits(w0))


def _slab_run(n, world, steps, v0, env, run):
    """`world` EngineSlab ranks as threads over local_hub: set v0, step `steps`, then run(m) -> a tuple of this rank's row tensors;
    the tuple's entries, rows of every rank stacked"""
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
                out[r] = [t.cpu().numpy() for t in run(m)]
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
    return [np.concatenate([o[i] for o in out]) for i in range(len(out[0]))]


@pytest.mark.parametrize("world,n,env", [(2, 256, {}), (4, 768, {}), (8, 512, {"FB_SLAB_COL_GROUPS": "2"}),
                                         (4, 1024, {"FB_SLAB_COL_GROUPS": "2"}), (2, 512, {"FB_SLAB_FIELD_GROUPS": "2"}), (1, 256, {})])
def test_slab_equals_single_gpu_bitwise(world, n, env):
    """The slab's records (ranks as threads) against the one-GPU model's, bit for bit: Okubo-Weiss, vorticity, psi, u, v"""
    import xlab_fftbarotropic_amd as X
    v0 = X.make_field("kuo2004", n)
    ref = X.Model(n, n)
    ref.set_vort(v0)
    ref.step(3)
    want = [t.cpu().numpy() for t in ref.okubo_weiss() + (ref.vort(),) + ref.diag()]
    got = _slab_run(n, world, 3, v0, env, lambda m: m.okubo_weiss_local() + (m.vort_local(),) + m.diag_local())
    for name, a, b in zip(("W", "tau", "vort", "psi", "u", "v"), got, want):
        assert np.array_equal(_bits(a), _bits(b)), name


@pytest.mark.parametrize("n", [4096, 8192])
def test_record_has_no_side_effects_full_pass(n):
    """Records between steps leave the step untouched on the single-pass x transform: k_col_full with k_rowq and its prescale
    (4096^2) and with k_rowh2 (8192^2): step k, every record, step k again == 2k plain steps, bit for bit"""
    import xlab_fftbarotropic_amd as X
    v0 = X.make_field("kuo2004", n)
    ref = X.Model(n, n, dt=3.0 * 1024 / n)
    ref.set_vort(v0)
    ref.step(6)
    want = ref.vort().cpu().numpy()
    ref.close()
    m = X.Model(n, n, dt=3.0 * 1024 / n)
    m.set_vort(v0)
    m.step(3)
    m.vort(), m.diag(), m.okubo_weiss(), m.eddy_diffusivity(fields=True)
    m.step(3)
    assert np.array_equal(_bits(m.vort().cpu().numpy()), _bits(want))


def test_slab_record_has_no_side_effects():
    """The same on a 4-rank slab (ranks as threads): step k, every record, step k again == 2k plain steps, bit for bit"""
    import xlab_fftbarotropic_amd as X
    n, world = 512, 4
    v0 = X.make_field("kuo2004", n)
    want = _slab_run(n, world, 6, v0, {}, lambda m: (m.vort_local(),))[0]

    def records_then_step(m):
        m.vort_local(), m.diag_local(), m.okubo_weiss_local(), m.eddy_diffusivity(fields=True)
        m.step(3)
        return (m.vort_local(),)
    got = _slab_run(n, world, 3, v0, {}, records_then_step)[0]
    assert np.array_equal(_bits(got), _bits(want))


def test_driver_dump_okubo_weiss(tmp_path):
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n = 256
    v0 = X.make_field("elliptic", n)
    runs = {}
    for tag, extra in (("one", []), ("two", ["--world", "2", "--ranks-as-threads"])):
        d = tmp_path / tag
        (d / "input").mkdir(parents=True)
        (d / "output").mkdir()
        v0.tofile(str(d / "input" / "initial_vorticity.bin"))
        subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "101", "--dump-okubo-weiss"] + extra,
                       cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=300)
        runs[tag] = d
    order = ("vort_src_input", "vort", "psi", "u", "v", "okubo_weiss", "tau_fil")
    assert (runs["one"] / "log").read_text().split() == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in order]
    rd = lambda d, name: np.fromfile(str(d / "output" / name), dtype="<f4").reshape(n, n)
    m = X.Model(n, n)
    m.set_vort(v0)
    for s in (0, 100):
        w, tau = _ow(m)
        for name, want in (("okubo_weiss", w), ("tau_fil", tau)):
            f = "%s_step_%d.bin" % (name, s)
            assert np.array_equal(_bits(rd(runs["one"], f)), _bits(want)), f
            assert np.array_equal(_bits(rd(runs["two"], f)), _bits(want)), f
        m.step(100)


def test_errors():
    import xlab_fftbarotropic_amd as X
    L = X.lib()
    m = X.Model(256, 256)
    m.set_vort(X.make_field("elliptic", 256))
    assert L.fb_model_get_okubo_weiss(m._h, None, None) == FB_EINVAL
    w = m.fop.empty_real()
    s = ctypes.c_void_p()
    assert L.fb_slab_create(ctypes.byref(s), 256, 256, 6e5, 6e5, 6.5, 3.0, 0, 2) == 0
    try:
        assert L.fb_slab_get_okubo_weiss_local(s, ctypes.c_void_p(w.data_ptr()), None) == FB_EINVAL
        assert b"not connected" in L.fb_last_error()
    finally:
        L.fb_slab_destroy(s)
