"""GPU tests of the shell spectra and cascade-flux record output: fb_model_get_spectra (Model.spectra), fb_slab_get_spectra
(EngineSlab.spectra) and the driver's --dump-spectra.

The float64 yardstick (tests/spectra_numpy.py) is always built from the engine's own spectrum (Model.spectrum()) and coefficient tables.
Bounds, per shell b with n_b = column 2:
  columns 0-2                bit for bit (no mode of the grids used here lies within 1e-9 shells of a shell edge: asserted)
  E, Z, D_Z                  relative (n_b + 16) 2^-52: reordering a float64 sum of n_b positive terms plus the few roundings per term
  T_Z, T_E                   sum_b |T - T64| <= 1e-5 A, A = sqrt(sum w |a|^2) sqrt(sum w |n64|^2) (T_E: both factors over k): the project's
                             1e-5 relative L2 bar on the tendency carried through Cauchy-Schwarz; at 256^2 also at most 4 times what the
                             float32 CPU oracle's operators give (two float32 FFT factorisations differ by factors of 3 to 6)
  Pi_E, Pi_Z                 the negated running sums of columns 5, 6, bit for bit
  Parseval                   sum Z vs mean(zeta^2)/2, sum E vs mean(u^2 + v^2)/2 of the physical records within 2e-5 (quadratic: twice 1e-5)
Every case prints its measured error on one line (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "xlab-fftbarotropic_amd", "host")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
BAR = 1e-5
EPS = 2.0 ** -52
POS = (3, 4, 9)                                                              # E, Z, D_Z


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _yardstick(m, lx=6e5, ly=6e5, nu=6.5):
    """(table64, sum w|a||n| per shell, the same over k^2, A_Z, A_E, N64) from the engine's spectrum and tables"""
    import spectra_numpy as SN
    spec = m.spectrum().cpu().numpy()
    tables = m.fop.tables()
    n64, _ = SN.nonlinear64(spec, tables)
    tab, scale, scale_e = SN.table64(spec, n64, tables[4], nu, lx, ly)
    k2, _, w, _, edge = SN.geometry(m.nx, m.ny, lx, ly)
    assert edge >= 1e-9
    g = float(m.nx) * m.ny
    a2, n2 = w * np.abs(spec.astype(np.complex128) / g) ** 2, w * np.abs(tables[4] * n64 / g) ** 2
    k2s = np.where(k2 > 0, k2, np.inf)
    return tab, scale, scale_e, np.sqrt(a2.sum() * n2.sum()), np.sqrt((a2 / k2s).sum() * (n2 / k2s).sum()), n64


def _check(tag, got, tab, az, ae):
    """the assertions every table must pass against its float64 yardstick; returns the measured (worst positive-column ratio, T_Z, T_E)"""
    assert got.shape == tab.shape and not np.isnan(got).any()
    assert np.array_equal(_bits(got[:, :3]), _bits(tab[:, :3])), tag
    assert got[:, 2].sum() == tab[:, 2].sum()
    worst = 0.0
    for c in POS:
        bound = (tab[:, 2] + 16.0) * EPS * np.abs(tab[:, c])
        d = np.abs(got[:, c] - tab[:, c])
        worst = max(worst, float((d / np.where(bound > 0, bound, 1.0)).max()))
        assert (d <= bound).all(), (tag, c, int(np.argmax(d - bound)))
    ez, ee = float(np.abs(got[:, 6] - tab[:, 6]).sum() / az), float(np.abs(got[:, 5] - tab[:, 5]).sum() / ae)
    print("spectra %s: E, Z, D_Z worst |diff| / bound %.3f; sum|T_Z - T_Z64| / A %.2e, sum|T_E - T_E64| / A_E %.2e (bar %.0e)" % (tag, worst, ez, ee, BAR))
    assert ez <= BAR and ee <= BAR, tag
    assert np.array_equal(_bits(got[:, 7]), _bits(-np.cumsum(got[:, 5]))), tag
    assert np.array_equal(_bits(got[:, 8]), _bits(-np.cumsum(got[:, 6]))), tag
    return worst, ez, ee


def _oracle32_table(spec, n, mask, nu):
    """the same table through the float32 CPU oracle's operators (as tests/test_gpu_pressure.py::_pres32_reference_operators does for
    the pressure): J in float32 as main.cpp:151-227 forms it, binned in float64"""
    import oracle_py as O
    import spectra_numpy as SN
    ops = O.Operators(n, n, 6e5, 6e5)
    g = np.float32(n * n)
    s = np.ascontiguousarray(spec.astype(np.complex64))
    zx, zy = O.c2r(ops.gradx(s), n) / g, O.c2r(ops.grady(s), n) / g
    psi = ops.invertLaplacian(s)
    u = -(O.c2r(ops.grady(psi), n) / g)
    v = O.c2r(ops.gradx(psi), n) / g
    j = (-u * zx - v * zy).astype(np.float32)
    return SN.table64(spec, O.r2c(j), mask, nu, 6e5, 6e5)[0]


def test_256_against_fp64_and_the_float32_oracle():
    import xlab_fftbarotropic_amd as X
    n = 256
    m = X.Model(n, n)
    m.set_vort(X.make_field("kuo2004", n))
    for step in (0, 100):
        got = m.spectra().cpu().numpy()
        assert got.shape == (182, 10)
        tab, _, _, az, ae, _ = _yardstick(m)
        _, ez, ee = _check("256^2 kuo2004 step %d" % step, got, tab, az, ae)
        o32 = _oracle32_table(m.spectrum().cpu().numpy(), n, m.fop.tables()[4], 6.5)
        oz, oe = float(np.abs(o32[:, 6] - tab[:, 6]).sum() / az), float(np.abs(o32[:, 5] - tab[:, 5]).sum() / ae)
        print("spectra 256^2 kuo2004 step %d: T_Z engine vs fp64 %.3e, float32 oracle vs fp64 %.3e (ratio %.2f); T_E %.3e against %.3e (ratio %.2f); "
              "sum|T_Z64| / A %.2e" % (step, ez, oz, ez / oz, ee, oe, ee / oe, float(np.abs(tab[:, 6]).sum() / az)))
        assert ez <= 4.0 * oz and ee <= 4.0 * oe, step
        # Parseval against the engine's physical records
        z = m.vort().cpu().numpy().astype(np.float64)
        _, u, v = (t.cpu().numpy().astype(np.float64) for t in m.diag())
        pz, pe = 0.5 * np.mean(z * z), 0.5 * np.mean(u * u + v * v)
        rz, re = abs(got[:, 4].sum() - pz) / pz, abs(got[:, 3].sum() - pe) / pe
        print("spectra 256^2 kuo2004 step %d Parseval: sum Z vs mean(zeta^2)/2 %.2e, sum E vs mean(u^2+v^2)/2 %.2e (bar 2e-5)" % (step, rz, re))
        assert rz <= 2e-5 and re <= 2e-5
        m.step(100)


@pytest.mark.parametrize("nx,ny,kind", [(768, 768, "kuo2004"), (1024, 1024, "elliptic"), (4096, 4096, "kuo2004"),
                                        (128, 16384, "elliptic"), (16384, 64, "elliptic")])
def test_against_fp64_from_the_engine_spectrum(nx, ny, kind):
    import xlab_fftbarotropic_amd as X
    m = X.Model(nx, ny, dt=3.0 * 256 / max(nx, ny))
    m.set_vort(X.make_field(kind, nx, ny))
    m.step(20)
    got = m.spectra().cpu().numpy()
    again = m.spectra().cpu().numpy()
    assert np.array_equal(_bits(got), _bits(again))
    tab, _, _, az, ae, _ = _yardstick(m)
    _check("%dx%d %s after 20 steps" % (nx, ny, kind), got, tab, az, ae)
    z = m.vort().cpu().numpy().astype(np.float64)
    pz = 0.5 * np.mean(z * z)
    assert abs(got[:, 4].sum() - pz) / pz <= 2e-5


def test_exact_steady_state():
    """zeta = cos(3 kx0 x) + cos(3 ky0 y): every mode on shell 3, psi = -zeta / k^2, J = 0.  Bound: sum_b |T_Z| <= 1e-5 A with
    A = sqrt(mean zeta^2) sqrt(mean (|u zeta_x| + |v zeta_y|)^2) from the analytic float64 fields: the two products whose float32 rounding
    is all that J holds"""
    import xlab_fftbarotropic_amd as X
    n, L = 256, 6e5
    k = 2 * np.pi * 3 / L
    x = np.arange(n)[:, None] * (L / n)
    y = np.arange(n)[None, :] * (L / n)
    zeta = 1e-4 * (np.cos(k * x) + np.cos(k * y))
    m = X.Model(n, n)
    m.set_vort(zeta.astype(np.float32))
    got = m.spectra().cpu().numpy()
    zx, zy = -1e-4 * k * np.sin(k * x) + 0 * y, -1e-4 * k * np.sin(k * y) + 0 * x
    u, v = zy / (k * k), -zx / (k * k)                                       # u = -psi_y, v = psi_x, psi = -zeta / k^2
    A = np.sqrt(np.mean(zeta * zeta)) * np.sqrt(np.mean((np.abs(u * zx) + np.abs(v * zy)) ** 2))
    tz = float(np.abs(got[:, 6]).sum())
    print("spectra steady state 256^2: sum|T_Z| / A %.2e (bar %.0e); Z on shell 3 %.6e of %.6e" % (tz / A, BAR, got[3, 4], got[:, 4].sum()))
    assert tz <= BAR * A
    assert abs(got[3, 4] - 0.5 * np.mean(zeta * zeta)) <= 2e-5 * got[3, 4]
    assert got[:, 4].sum() - got[3, 4] <= 1e-10 * got[3, 4]


@pytest.mark.parametrize("lx,ly,bx,by", [(6e5, 3e5, 3, 4), (3e5, 6e5, 6, 2)])
def test_analytic_two_shells_anisotropic_non_square(lx, ly, bx, by):
    """zeta = A1 cos(a x) + A2 cos(b y) with wavenumber indices (3, 0) and (0, 2) on a 256 x 128 grid: a lies on shell bx, b on shell by
    (dk = 2 pi / max(Lx, Ly)), Z = A^2 / 4 and E = A^2 / (4 k^2) on each; swapped x / y scales put them on other shells in one of
    the two orientations at least.  2e-5: the field bar on a quadratic quantity"""
    import xlab_fftbarotropic_amd as X
    import spectra_numpy as SN
    nx, ny = 256, 128
    assert SN.geometry(nx, ny, lx, ly)[4] >= 1e-9
    a, b = 2 * np.pi * 3 / lx, 2 * np.pi * 2 / ly
    A1, A2 = 1e-4, 3e-4
    x = np.arange(nx)[:, None] * (lx / nx)
    y = np.arange(ny)[None, :] * (ly / ny)
    m = X.Model(nx, ny, Lx=lx, Ly=ly)
    m.set_vort((A1 * np.cos(a * x) + A2 * np.cos(b * y)).astype(np.float32))
    got = m.spectra().cpu().numpy()
    assert got.shape[0] == X.spectra_shells(nx, ny, lx, ly) == SN.nshells(nx, ny, lx, ly)
    want = {bx: (A1 * A1 / 4, A1 * A1 / (4 * a * a)), by: (A2 * A2 / 4, A2 * A2 / (4 * b * b))}
    worst = 0.0
    for sh, (z, e) in want.items():
        worst = max(worst, abs(got[sh, 4] - z) / z, abs(got[sh, 3] - e) / e)
        assert got[sh, 0] < (a if sh == bx else b) < got[sh, 1]
    rest = got[:, 4].sum() - got[bx, 4] - got[by, 4]
    print("spectra analytic %dx%d Lx=%g Ly=%g: shells %d, %d, worst relative error of E, Z %.2e (bar 2e-5), Z elsewhere %.1e of the total"
          % (nx, ny, lx, ly, bx, by, worst, rest / got[:, 4].sum()))
    assert worst <= 2e-5
    assert rest <= 1e-10 * got[:, 4].sum()
    tab, _, _, az, ae, _ = _yardstick(m, lx, ly)
    assert np.array_equal(_bits(got[:, :3]), _bits(tab[:, :3]))


@pytest.mark.parametrize("graph", [False, True])
def test_record_has_no_side_effects(graph):
    """50 steps with and without a spectra call in between give identical spectra (and state), with the captured step on and off;
    two calls on the same state give identical bits; the other records keep their bits around it (shared record workspace)"""
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("kuo2004", n)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = []
        for call in (False, True):
            m = X.Model(n, n)
            m.fop.use_current_stream()
            m.use_graph(graph)
            m.set_vort(v0)
            m.step(25)
            if call:
                before = [t.cpu().numpy() for t in (m.vort(), m.pressure(), m.okubo_weiss()[0])]
                t0 = m.spectra()
                t1 = m.spectra()
                after = [t.cpu().numpy() for t in (m.vort(), m.pressure(), m.okubo_weiss()[0])]
                assert np.array_equal(_bits(t0.cpu().numpy()), _bits(t1.cpu().numpy()))
                for a, b in zip(before, after):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            m.step(25)
            out.append((m.spectra().cpu().numpy(), m.spectrum().cpu().numpy()))
            m.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


@pytest.mark.parametrize("n", [4096, 8192])
def test_record_has_no_side_effects_single_pass_x(n):
    """the single-pass x transform (4096^2, 8192^2): step, a spectra record, step == plain steps, bit for bit; the record repeats"""
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
    p_before = m.pressure().cpu().numpy()
    t0 = m.spectra().cpu().numpy()
    assert np.array_equal(p_before.view(np.uint32), m.pressure().cpu().numpy().view(np.uint32))
    assert np.array_equal(_bits(t0), _bits(m.spectra().cpu().numpy()))
    assert t0[:, 2].sum() == float(n) * n and not np.isnan(t0).any()
    m.step(3)
    assert np.array_equal(want.view(np.uint32), m.vort().cpu().numpy().view(np.uint32))


def _slab_run(nx, ny, world, steps, v0, env):
    """`world` EngineSlab ranks as threads over local_hub: set v0, step, EngineSlab.spectra() of every rank"""
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
                first = m.spectra().cpu().numpy()
                m.okubo_weiss_local()                                     # another kind in between, on the shared workspace
                out[r] = (first, m.spectra().cpu().numpy())
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


@pytest.mark.parametrize("world,nx,ny,env", [(2, 256, 256, {}), (4, 768, 768, {}), (8, 512, 512, {"FB_SLAB_COL_GROUPS": "2"}),
                                             (8, 8192, 256, {"FB_SLAB_COL_GROUPS": "2"}), (4, 2048, 128, {})])
def test_slab_against_single_gpu(world, nx, ny, env):
    """ranks as threads on one GPU: columns 0-2 bitwise equal to the one-GPU table, E, Z, D_Z within (n_b + 16) 2^-52 of it, T within
    that factor times sum w |a| |n| of the shell (over k^2 for T_E); every rank holds the same bits; the record repeats"""
    import xlab_fftbarotropic_amd as X
    import spectra_numpy as SN
    assert SN.geometry(nx, ny, 6e5, 6e5)[4] >= 1e-9
    v0 = X.make_field("kuo2004", nx, ny)
    one = X.Model(nx, ny)
    one.set_vort(v0)
    one.step(3)
    want = one.spectra().cpu().numpy()
    _, scale, scale_e, _, _, _ = _yardstick(one)
    out = _slab_run(nx, ny, world, 3, v0, env)
    got = out[0][0]
    for r in range(world):
        assert np.array_equal(_bits(out[r][0]), _bits(got)), r
        assert np.array_equal(_bits(out[r][1]), _bits(got)), r
    assert np.array_equal(_bits(got[:, :3]), _bits(want[:, :3]))
    fac = (want[:, 2] + 16.0) * EPS
    worst = 0.0
    for c, sc in ((3, want[:, 3]), (4, want[:, 4]), (9, want[:, 9]), (6, scale), (5, scale_e)):
        d, bound = np.abs(got[:, c] - want[:, c]), fac * np.abs(sc)
        worst = max(worst, float((d / np.where(bound > 0, bound, 1.0)).max()))
        assert (d <= bound).all(), (c, int(np.argmax(d - bound)))
    assert np.array_equal(_bits(got[:, 7]), _bits(-np.cumsum(got[:, 5])))
    assert np.array_equal(_bits(got[:, 8]), _bits(-np.cumsum(got[:, 6])))
    print("spectra slab %d ranks %dx%d %s vs one GPU: worst |diff| / bound %.3f" % (world, nx, ny, env, worst))


def test_driver_dump_spectra(tmp_path):
    """--dump-spectra at 256^2, a record every 10 steps, one GPU and --world 2 --ranks-as-threads: file size nshells * 80 bytes, position
    in ./log, content bitwise equal to Model.spectra() at the same step; without the option the same files with the same bytes"""
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n = 256
    v0 = X.make_field("kuo2004", n)
    runs = {}
    for tag, extra in (("plain", []), ("one", ["--dump-spectra"]), ("two", ["--dump-spectra", "--world", "2", "--ranks-as-threads"]),
                       ("all", ["--dump-spectra", "--dump-pressure", "--dump-eddy-diffusivity", "--record-buffers", "1"])):
        d = tmp_path / tag
        (d / "input").mkdir(parents=True)
        (d / "output").mkdir()
        v0.tofile(str(d / "input" / "initial_vorticity.bin"))
        subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", "21", "--record-step", "10"] + extra,
                       cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=300)
        runs[tag] = d
    base = ("vort_src_input", "vort", "psi", "u", "v")
    steps = (0, 10, 20)
    log = lambda tag: (runs[tag] / "log").read_text().split()
    assert log("plain") == ["output/%s_step_%d.bin" % (name, s) for s in steps for name in base]
    assert log("one") == ["output/%s_step_%d.bin" % (name, s) for s in steps for name in base + ("spectra",)]
    assert log("two") == log("one")
    assert log("all") == ["output/%s_step_%d.bin" % (name, s) for s in steps for name in base + ("pres", "spectra", "eddy_diffusivity")]
    assert sorted(os.listdir(str(runs["plain"] / "output"))) == sorted("%s_step_%d.bin" % (name, s) for s in steps for name in base)
    for f in os.listdir(str(runs["plain"] / "output")):                      # the option changes no other file
        assert (runs["plain"] / "output" / f).read_bytes() == (runs["one"] / "output" / f).read_bytes(), f
    ns = X.spectra_shells(n)
    m = X.Model(n, n)
    m.set_vort(v0)
    for s in steps:
        f = "spectra_step_%d.bin" % s
        assert os.path.getsize(str(runs["one"] / "output" / f)) == ns * 80
        got = np.fromfile(str(runs["one"] / "output" / f), dtype="<f8").reshape(-1, 10)
        assert np.array_equal(_bits(got), _bits(m.spectra().cpu().numpy())), f
        assert (runs["all"] / "output" / f).read_bytes() == (runs["one"] / "output" / f).read_bytes(), f
        two = np.fromfile(str(runs["two"] / "output" / f), dtype="<f8").reshape(-1, 10)
        assert np.array_equal(_bits(two[:, :3]), _bits(got[:, :3])) and two.shape == got.shape
        for c in (3, 4, 9):
            assert (np.abs(two[:, c] - got[:, c]) <= (got[:, 2] + 16.0) * EPS * np.abs(got[:, c])).all(), (f, c)
        m.step(10)
