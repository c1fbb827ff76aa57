"""GPU tests of the azimuthal-mean record output: fb_model_get_azimuthal (Model.azimuthal), fb_slab_get_azimuthal
(EngineSlab.azimuthal) and the driver's --dump-azimuthal.

The yardstick is tests/azimuthal_numpy.py, the definition of include/fftbaro.h in float64 numpy on the engine's own records
(m.vort(), m.diag()).  Columns 0-2 (bin edges, counts) and the centre agree bit for bit.  A mean column agrees within
1e-9 <|term|>, the bin mean of the absolute value of the summed term: the float64 summation bound n 2^-53 with n < 2^24 points per
bin is 2e-9 at the very worst and 1e-13 for the bins of these grids (n < 2000), so 1e-9 leaves orders of margin and still scales
with the terms where <v_r> and <v_r zeta> cancel to near zero.  Gamma is held to the same measure against dx dy sum |zeta|.
The worst measured error of every case is printed in units of that bound (pytest -s)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import azimuthal_numpy as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
FB_EINVAL = 1
L = 600000.0
TOL = 1e-9
MODES = {"psi-min": 1, "vort-max": 2}


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _b32(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def _fields(m):
    psi, u, v = (a.cpu().numpy() for a in m.diag())
    return m.vort().cpu().numpy(), psi, u, v


def _az(m, **kw):
    t, c = m.azimuthal(**kw)
    m.torch.cuda.synchronize()
    return t.cpu().numpy(), c.cpu().numpy()


def _want_center(zeta, psi, center):
    if center == "psi-min":
        return A.find_center(psi, L, L, False)
    if center == "vort-max":
        return A.find_center(zeta, L, L, True)
    return np.array([center[0], center[1], -1.0, 0.0])


def _worst(got, want, scale):
    """the largest |got - want| in units of TOL * scale (0 where both the error and the scale are 0)"""
    err = np.abs(got - want)[:, 3:]
    s = TOL * scale[:, 3:]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / s)
    return float(np.max(q))


def _check(tag, got_t, got_c, fields, center, nbins, dr, nmodes):
    zeta, psi, u, v = fields
    want_c = _want_center(zeta, psi, center)
    assert np.array_equal(_b64(got_c), _b64(want_c)), (tag, got_c, want_c)
    want_t, scale = A.table(zeta, u, v, L, L, want_c[0], want_c[1], nbins, dr, nmodes)
    assert got_t.shape == want_t.shape, tag
    assert np.array_equal(_b64(got_t[:, :3]), _b64(want_t[:, :3])), tag
    assert np.all(np.isfinite(got_t)), tag
    w = _worst(got_t, want_t, scale)
    print("azimuthal %-44s worst error %.3g of the bound 1e-9 <|term|>" % (tag, w))
    assert w <= 1.0, (tag, w)
    return want_t, scale


_models = {}


def _model(kind, nx, ny, steps):
    """a stepped model and its records, made once per (field, grid) and left unchanged"""
    import xlab_fftbarotropic_amd as X
    key = (kind, nx, ny, steps)
    if key not in _models:
        m = X.Model(nx, ny)
        m.set_vort(X.make_field(kind, nx, ny))
        m.step(steps)
        _models[key] = (m, _fields(m))
    return _models[key]


# ---- 1. against numpy, on the engine's own fields ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nx,ny,steps", [("kuo2004", 256, 256, 3), ("elliptic", 256, 256, 5), ("kuo2004", 192, 64, 4), ("elliptic", 192, 64, 3),
                                              ("kuo2004", 64, 256, 5), ("elliptic", 64, 256, 4)])
@pytest.mark.parametrize("center", ["psi-min", "vort-max", "fixed"])
def test_against_numpy(kind, nx, ny, steps, center):
    m, fields = _model(kind, nx, ny, steps)
    nb0, dr0 = A.default_bins(nx, ny, L, L)
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    cen = (float(0.37 * L), float(0.81 * L)) if center == "fixed" else center       # a fixed centre off the grid points
    for nmodes, nbins, dr in ((0, 2, dr0), (4, nb0, dr0), (8, nb0, dr0), (4, 2, float(min(dx, dy))), (8, 7, float(2.6 * dr0))):
        t, c = _az(m, center=cen, nbins=nbins, dr=dr, nmodes=nmodes)
        _check("%s %dx%d %s m%d b%d dr%.0f" % (kind, nx, ny, center, nmodes, nbins, dr), t, c, fields, cen, nbins, dr, nmodes)
    t, c = _az(m, center=cen)                                                       # the defaults of the binding
    assert t.shape == (nb0, 20)
    _check("%s %dx%d %s defaults" % (kind, nx, ny, center), t, c, fields, cen, nb0, dr0, 4)


def test_large_tile_grid():
    """1024 x 1024: 1024 tiles of points, more than one wave of workgroups; dr between the grid steps' multiples"""
    m, fields = _model("kuo2004", 1024, 1024, 3)
    nb0, dr0 = A.default_bins(1024, 1024, L, L)
    for center, nmodes, nbins, dr in (("psi-min", 4, nb0, dr0), ("vort-max", 8, 300, 1.7 * dr0)):
        t, c = _az(m, center=center, nbins=nbins, dr=dr, nmodes=nmodes)
        _check("kuo2004 1024x1024 %s m%d b%d" % (center, nmodes, nbins), t, c, fields, center, nbins, dr, nmodes)


def test_4096_bins():
    """nbins = 4096 needs dr <= min(Lx, Ly) / 8192 and dr >= min(dx, dy): a grid side of 8192.  8192 x 64 is the smallest such grid;
    its dy = 128 dx also takes the tiles' radii beyond the window of bins kept on chip."""
    m, fields = _model("elliptic", 8192, 64, 3)
    _, _, dx, dy = A.grid_steps(8192, 64, L, L)
    for center in ("psi-min", (float(4000 * dx), float(31 * dy))):
        t, c = _az(m, center=center, nbins=4096, dr=float(dx), nmodes=8)
        _check("elliptic 8192x64 %s m8 b4096" % (center if isinstance(center, str) else "fixed"), t, c, fields, center, 4096, float(dx), 8)


# ---- 2. the minimum image ----------------------------------------------------------------------------------------------------
def _gaussian(nx, ny, ic, jc):
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    r = A.geometry(nx, ny, L, L, ic * dx, jc * dy, max(dx, dy))[0]
    return (2.0e-3 * np.exp(-(r / 4.0e4) ** 2)).astype(np.float32)


@pytest.mark.parametrize("nx,ny", [(256, 256), (192, 64), (64, 256)])
def test_minimum_image(nx, ny):
    import xlab_fftbarotropic_amd as X
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    nbins, dr = A.default_bins(nx, ny, L, L)
    ic, jc = (9 * nx) // 10, ny // 10
    out = {}
    for tag, (i0, j0) in (("seam", (ic, jc)), ("mid", (nx // 2, ny // 2))):
        m = X.Model(nx, ny)
        m.set_vort(_gaussian(nx, ny, i0, j0))
        fields = _fields(m)
        for center in ("psi-min", "vort-max"):
            t, c = _az(m, center=center, nbins=nbins, dr=dr, nmodes=4)
            assert c[2] == i0 * ny + j0 and c[0] == i0 * dx and c[1] == j0 * dy, (tag, center, c)
            want, scale = _check("gaussian %dx%d %s %s" % (nx, ny, tag, center), t, c, fields, center, nbins, dr, 4)
            out[tag, center] = (t, want, scale)
        m.close()
    for center in ("psi-min", "vort-max"):
        (ts, ws, ss), (tm, wm, sm) = out["seam", center], out["mid", center]
        assert np.array_equal(_b64(ts[:, :3]), _b64(tm[:, :3]))
        # the two records differ by their float32 round-off: numpy's tables of the two say by how much; the engine's tables may differ
        # by that and by the summation bound of each
        allow = np.abs(ws - wm) + TOL * (ss + sm)
        assert np.all(np.abs(ts - tm)[:, 3:] <= allow[:, 3:]), center


# ---- 3. conventions ----------------------------------------------------------------------------------------------------------
def _ellipse(nx, ny, ic, jc, angle):
    """a smooth elliptic cyclone, major axis 2:1 at `angle` from the x axis"""
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    x = (np.arange(nx) - ic)[:, None] * dx
    y = (np.arange(ny) - jc)[None, :] * dy
    a, b = x * np.cos(angle) + y * np.sin(angle), -x * np.sin(angle) + y * np.cos(angle)
    return (2.0e-3 * np.exp(-((a / 8.0e4) ** 2 + (b / 4.0e4) ** 2))).astype(np.float32)


@pytest.mark.parametrize("nx,ny", [(192, 64), (64, 256)])
@pytest.mark.parametrize("angle", [0.0, np.pi / 2, np.pi / 3])
def test_conventions(nx, ny, angle):
    import xlab_fftbarotropic_amd as X
    _, _, dx, dy = A.grid_steps(nx, ny, L, L)
    ic, jc = nx // 2, ny // 2
    nbins, dr = A.default_bins(nx, ny, L, L)
    m = X.Model(nx, ny)
    m.set_vort(_ellipse(nx, ny, ic, jc, angle))
    t, c = _az(m, center=(float(ic * dx), float(jc * dy)), nbins=nbins, dr=dr, nmodes=3)
    assert c[2] == -1.0 and c[3] == 0.0
    edge = (t[:, 3] > 3.0e4) & (t[:, 3] < 9.0e4)                                # the bins around the vortex edge
    assert np.count_nonzero(edge) >= 4
    z1, z2, z3 = (t[:, 12 + 2 * k] + 1j * t[:, 13 + 2 * k] for k in range(3))
    assert np.all(np.abs(z2[edge]) >= 10 * np.abs(z1[edge])) and np.all(np.abs(z2[edge]) >= 10 * np.abs(z3[edge]))
    # zeta = f(r) (1 + e cos 2 (theta - angle)): zeta_2 = <zeta e^{-2 i theta}> has the phase -2 angle.  A ring of these grids holds
    # about a hundred points of a lattice with dy = 3 dx or dx = 4 dy, whose own <e^{-2 i theta}> is several percent; against
    # |zeta_2| / <zeta> = 0.3-0.4 of this vortex that turns the phase by up to asin(0.2): 0.1 rad of the axis.  A swap of x and y
    # (axis pi/2 - angle) or a sign error (-angle) is off by 0.5 rad or more at angle = pi/3.
    axis = -np.angle(z2[edge]) / 2
    assert np.max(np.abs(np.angle(np.exp(2j * (axis - angle))))) <= 2 * 0.1, (axis, angle)
    assert np.all(t[1:, 5][t[1:, 2] > 0] > 0)                                    # a cyclone: v_t > 0
    # seen from a centre shifted by d = (+4 dx, 0) the vortex lies at theta = pi: zeta(x + d) ~ zeta - d . grad zeta, and for this
    # vortex grad zeta = -2 zeta M x with M positive definite (axes 1 / 8e4^2, 1 / 4e4^2), so the wavenumber-1 part points along
    # -M d, within atan(3 / 4) = 37 degrees of -d: zeta_1 = <zeta e^{-i theta}> has a negative real part that exceeds its imaginary part
    ts, _ = _az(m, center=(float((ic + 4) * dx), float(jc * dy)), nbins=nbins, dr=dr, nmodes=3)
    s1 = ts[:, 12] + 1j * ts[:, 13]
    ring = (ts[:, 3] > 4.0e4) & (ts[:, 3] < 8.0e4)
    assert np.all(s1[ring].real < 0) and np.all(np.abs(s1[ring].imag) <= np.abs(s1[ring].real))
    m.close()


# ---- 4. ties and degenerate input --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(256, 256), (192, 64)])
def test_all_zero_field(nx, ny):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny)
    m.set_vort(np.zeros((nx, ny), np.float32))
    nbins, dr = A.default_bins(nx, ny, L, L)
    z = np.zeros((nx, ny), np.float32)
    for center in ("psi-min", "vort-max"):
        t, c = _az(m, center=center, nmodes=8)
        assert np.array_equal(c, np.zeros(4)) and not np.any(np.isnan(t))
        want, _ = A.table(z, z, z, L, L, 0.0, 0.0, nbins, dr, 8)
        assert np.array_equal(_b64(t[:, :3]), _b64(want[:, :3]))
        assert np.all(np.abs(t[:, 3] - want[:, 3]) <= TOL * want[:, 3]) and np.all(t[:, 4:] == 0.0)
    m.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    import xlab_fftbarotropic_amd as X
    Lb = X.lib()
    m, _ = _model("elliptic", 256, 256, 5)
    before = _b32(m.vort())
    tb = m.torch.empty((4097, 28), dtype=m.torch.float64, device="cuda")
    cb = m.torch.empty(4, dtype=m.torch.float64, device="cuda")
    tp, cp = ctypes.c_void_p(tb.data_ptr()), ctypes.c_void_p(cb.data_ptr())
    dx = L / 256
    nan, inf = float("nan"), float("inf")
    ok = dict(m=m._h, mode=1, xc=0.0, yc=0.0, nbins=64, dr=dx, nmodes=4, t=tp, c=cp)
    bad = [("NULL model", dict(m=None)), ("NULL table", dict(t=None)), ("NULL centre", dict(c=None)), ("mode 3", dict(mode=3)), ("mode -1", dict(mode=-1)),
           ("xc = Lx", dict(mode=0, xc=L)), ("yc < 0", dict(mode=0, yc=-1.0)), ("xc NaN", dict(mode=0, xc=nan)), ("yc inf", dict(mode=0, yc=inf)),
           ("nbins 1", dict(nbins=1)), ("nbins 4097", dict(nbins=4097)), ("nmodes -1", dict(nmodes=-1)), ("nmodes 9", dict(nmodes=9)),
           ("dr NaN", dict(dr=nan)), ("dr inf", dict(dr=inf)), ("dr < dx", dict(dr=0.999 * dx)), ("dr < 0", dict(dr=-dx)),
           ("nbins dr > L/2", dict(nbins=129)), ("nbins dr > L/2", dict(nbins=64, dr=2.01 * dx))]
    for what, kw in bad:
        a = dict(ok, **kw)
        Lb.fb_internal_set_error(b"")
        rc = Lb.fb_model_get_azimuthal(a["m"], a["mode"], a["xc"], a["yc"], a["nbins"], a["dr"], a["nmodes"], a["t"], a["c"])
        assert rc == FB_EINVAL, what
        assert Lb.fb_last_error() != b"", what
    assert Lb.fb_model_get_azimuthal(ok["m"], 1, 0.0, 0.0, 128, dx, 4, tp, cp) == 0          # the largest table allowed goes through
    with pytest.raises(X.FftBaroError):
        m.azimuthal(nbins=1)
    with pytest.raises(X.FftBaroError):
        m.azimuthal(center=(L, 0.0))
    with pytest.raises(ValueError):
        m.azimuthal(center="centroid")
    s = ctypes.c_void_p()
    assert Lb.fb_slab_create(ctypes.byref(s), 256, 256, 6e5, 6e5, 6.5, 3.0, 0, 2) == 0
    try:
        assert Lb.fb_slab_get_azimuthal(s, 1, 0.0, 0.0, 1, dx, 4, tp, cp) == FB_EINVAL and b"nbins" in Lb.fb_last_error()
        assert Lb.fb_slab_get_azimuthal(s, 1, 0.0, 0.0, 64, dx, 4, tp, cp) == FB_EINVAL and b"not connected" in Lb.fb_last_error()
        assert Lb.fb_slab_get_azimuthal(None, 1, 0.0, 0.0, 64, dx, 4, tp, cp) == FB_EINVAL
    finally:
        Lb.fb_slab_destroy(s)
    m.torch.cuda.synchronize()
    assert np.array_equal(_b32(m.vort()), before)


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracer", [False, True])
def test_nothing_else_moves(tracer):
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("kuo2004", n)

    def run(with_azimuthal, graph):
        out = []
        stream = torch.cuda.Stream() if graph else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            m = X.Model(n, n)
            m.fop.use_current_stream()
            m.set_vort(v0)
            if tracer:
                m.set_tracer(X.make_field("elliptic", n), 3.0)
            if graph:
                m.use_graph(True)
            m.step(3)
            for center in ("psi-min", "vort-max", (1.0e5, 2.0e5)):
                if with_azimuthal:
                    m.azimuthal(center=center, nmodes=8)
                out += [_b32(m.vort()), _b32(torch.view_as_real(m.spectrum()))]
                if tracer:
                    out.append(_b32(m.tracer()))
                m.step(2)
            out += [_b32(m.vort())] + ([_b32(m.tracer())] if tracer else [])
            if with_azimuthal:                                                   # and the other records after it
                m.azimuthal()
            out += [_b64(m.eddy_diffusivity(64).cpu().numpy()[:, :3]), _b32(m.okubo_weiss()[0]), _b64(m.spectra().cpu().numpy())]
            stream.synchronize()
            m.close()
        return out
    for graph in (False, True):
        a, b = run(False, graph), run(True, graph)
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (graph, k)


# ---- 7. slab -----------------------------------------------------------------------------------------------------------------
def _slab_az(nx, ny, world, steps, v0, calls):
    import threading
    S = _slab()
    hub = S.local_hub(world)
    out, errs = [None] * world, [None] * world

    def work(r):
        try:
            m = S.EngineSlab(nx, ny, rank=r, world=world, transport=hub)
            try:
                m.set_vort_local(S.local_rows(v0, r, world))
                m.step(steps)
                res = []
                for kw in calls:
                    t, c = m.azimuthal(**kw)
                    res.append((t.cpu().numpy(), c.cpu().numpy()))
                out[r] = (res, m.vort_local().cpu().numpy())
            finally:
                m.close()
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
    return out


@pytest.mark.parametrize("world,nx,ny", [(2, 256, 256), (4, 256, 256), (2, 192, 64), (2, 64, 256)])
def test_slab_equals_single_gpu(world, nx, ny):
    import xlab_fftbarotropic_amd as X
    steps = 3
    m, fields = _model("kuo2004", nx, ny, steps)
    nb0, dr0 = A.default_bins(nx, ny, L, L)
    calls = [dict(center="psi-min", nmodes=4), dict(center="vort-max", nmodes=8), dict(center=(0.37 * L, 0.81 * L), nmodes=0),
             dict(center="psi-min", nbins=2, nmodes=2), dict(center="vort-max", nbins=5, dr=3.3 * dr0, nmodes=8)]
    out = _slab_az(nx, ny, world, steps, X.make_field("kuo2004", nx, ny), calls)
    assert np.array_equal(_b32(np.concatenate([o[1] for o in out])), _b32(fields[0]))
    for k, kw in enumerate(calls):
        one_t, one_c = _az(m, **kw)
        for r in range(world):
            t, c = out[r][0][k]
            assert np.array_equal(_b64(c), _b64(one_c)), (k, r)
            assert np.array_equal(_b64(t[:, :3]), _b64(one_t[:, :3])), (k, r)
            assert np.array_equal(_b64(t), _b64(out[0][0][k][0])), (k, r)          # every rank holds the same table
        nbins, dr = kw.get("nbins", nb0), kw.get("dr", dr0)
        _check("slab world %d %dx%d call %d" % (world, nx, ny, k), out[0][0][k][0], out[0][0][k][1], fields, kw["center"], nbins, dr, kw["nmodes"])


# ---- 8. driver ---------------------------------------------------------------------------------------------------------------
def _run_driver(d, n, v0, extra, check=True):
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    p = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "101"] + extra,
                       cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=check, timeout=300)
    return p.returncode, ((d / "log").read_text().split() if (d / "log").exists() else [])


def test_driver_dump_azimuthal(tmp_path):
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, nbins, nmodes = 256, 100, 3
    v0 = X.make_field("kuo2004", n)
    runs = {}
    opts = ["--dump-azimuthal", "--azim-center", "vort-max", "--azim-bins", str(nbins), "--azim-modes", str(nmodes)]
    for tag, extra in (("one", []), ("two", ["--world", "2", "--ranks-as-threads"])):
        _, log = _run_driver(tmp_path / tag, n, v0, ["--dump-eddy-diffusivity"] + opts + extra)
        order = ("vort_src_input", "vort", "psi", "u", "v", "eddy_diffusivity", "azimuthal", "azimuthal_center")
        assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 100) for name in order], tag
        runs[tag] = tmp_path / tag
    m = X.Model(n, n)
    m.set_vort(v0)
    nb0, dr0 = A.default_bins(n, n, L, L)
    for s in (0, 100):
        want_t, want_c = _az(m, center="vort-max", nbins=nbins, nmodes=nmodes)
        _, scale = A.table(*[_fields(m)[k] for k in (0, 2, 3)], L, L, want_c[0], want_c[1], nbins, dr0, nmodes)
        for tag, d in runs.items():
            f, fc = (d / "output" / (name % s) for name in ("azimuthal_step_%d.bin", "azimuthal_center_step_%d.bin"))
            assert os.path.getsize(str(f)) == nbins * (12 + 2 * nmodes) * 8 and os.path.getsize(str(fc)) == 32
            t = np.fromfile(str(f), dtype="<f8").reshape(nbins, 12 + 2 * nmodes)
            assert np.array_equal(_b64(np.fromfile(str(fc), dtype="<f8")), _b64(want_c)), (tag, s)
            assert np.array_equal(_b64(t[:, :3]), _b64(want_t[:, :3])), (tag, s)
            assert _worst(t, want_t, 2 * scale) <= 1.0, (tag, s)                 # two engine tables: the summation bound of each
        m.step(100)
    # with a tracer the two files still come last; the defaults; a fixed centre
    d = tmp_path / "trc"
    (d / "input").mkdir(parents=True)
    X.make_field("elliptic", n).tofile(str(d / "input" / "c.bin"))
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "101", "--tracer", "c.bin", "--dump-eddy-diffusivity",
                    "--dump-azimuthal", "--azim-center", "100000,250000.5"], cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=300)
    log = (d / "log").read_text().split()
    assert [x.split("/")[1].rsplit("_step_", 1)[0] for x in log[-4:]] == ["tracer", "tracer_eddy_diffusivity", "azimuthal", "azimuthal_center"]
    assert os.path.getsize(str(d / "output" / "azimuthal_step_100.bin")) == nb0 * 20 * 8
    assert np.array_equal(np.fromfile(str(d / "output" / "azimuthal_center_step_0.bin"), dtype="<f8"), np.array([100000.0, 250000.5, -1.0, 0.0]))
    # what the ABI would refuse is refused on the command line
    for k, bad in enumerate((["--azim-bins", "1"], ["--azim-bins", "4097"], ["--azim-bins", "200"], ["--azim-modes", "9"], ["--azim-dr", "100"],
                             ["--azim-center", "600000,0"], ["--azim-center", "nowhere"])):
        rc, _ = _run_driver(tmp_path / ("bad%d" % k), n, v0, ["--dump-azimuthal"] + bad, check=False)
        assert rc == 2, bad
