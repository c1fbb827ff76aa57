"""GPU tests of the vortex census: fb_model_census / fb_slab_census (Model.census, EngineSlab.census) and the driver's --dump-census,
against the float64 numpy restatement of the definition in tests/census_numpy.py (its inputs are checked in tests/test_census_cpu.py).

Asserted for every case: found, both counts, label, n and peak_index exactly; peak bit for bit; the id map cell for cell; every sum
within n 2^-52 sum |term| of numpy's, n the structure's cells -- the float64 bound for two summation orders of bit-equal terms, derived
and not measured, so one-cell structures are exact; two calls give identical integer columns.  Masks are fields of 0 / 1 with the
threshold 0.5 and the weight is a separate white-noise field, so the moment columns are not trivially equal."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "xlab-fftbarotropic_amd", "host")
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import census_numpy as CN  # noqa: E402

GRIDS = [(64, 64), (192, 64), (64, 256)]
INT_COLS = [CN.LABEL, CN.N, CN.PEAK_INDEX]


def _np(t):
    return t.cpu().numpy()


def _same64(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _slab():
    from importlib import import_module
    return import_module("xlab-fftbarotropic_amd.slab")


def _nan_mask(nx, ny):
    f = CN.bernoulli(nx, ny, 8)
    f[3:9, 4:30] = np.nan
    f[nx - 1, :] = np.nan
    return f


MASKS = {
    "empty": lambda nx, ny: np.zeros((nx, ny), np.float32),
    "full": lambda nx, ny: np.ones((nx, ny), np.float32),
    "checkerboard": CN.checkerboard,
    "spiral": CN.spiral,
    "comb": CN.comb,
    "corners": CN.corners,
    "seam": CN.seam_cross,
    "nan": _nan_mask,
    "bernoulli": lambda nx, ny: CN.bernoulli(nx, ny, {(64, 64): 5, (192, 64): 6, (64, 256): 7}[(nx, ny)]),
}


@functools.lru_cache(maxsize=None)
def _case(name, nx, ny):
    """(f, w, the reference), computed once and shared; never modified"""
    f = MASKS[name](nx, ny)
    w = CN.white(nx, ny, 100 + nx + ny)
    if name == "nan":
        w = w.copy()
        w[20:24, :] = np.nan                                    # NaN weights too: they never win the peak
    return f, w, CN.census(f, 0.5, weight=w, max_structures=65536)


def _compare(got, ref, tag, max_structures=65536):
    """got = (table, found, ids, count) from the GPU against a census_numpy result"""
    table, found, ids, count = got
    rows = min(ref["found"], max_structures)
    want, bound = ref["table"][:rows], ref["bound"][:rows]
    assert found == ref["found"] and list(count) == [ref["found"], ref["total"]], (tag, found, count, ref["found"], ref["total"])
    assert table.shape == (rows, CN.COLS), (tag, table.shape)
    for col in INT_COLS:
        assert np.array_equal(table[:, col], want[:, col]), (tag, col)
    assert _same64(table[:, CN.PEAK], want[:, CN.PEAK]), tag
    if ids is not None:
        assert ids.dtype == np.int32 and np.array_equal(ids, ref["ids"]), tag
    worst = 0.0
    for col in CN.SUM_COLS:
        err = np.abs(table[:, col] - want[:, col])
        fin = np.isfinite(want[:, col])
        assert np.array_equal(np.isnan(table[:, col]), np.isnan(want[:, col])), (tag, col)
        over = err[fin] - bound[fin, col]
        if over.size:
            worst = max(worst, float(np.max(err[fin] / np.maximum(bound[fin, col], 1e-300) * (bound[fin, col] > 0))))
            assert np.all(over <= 0.0), (tag, col, float(over.max()))
    print("%s: found %d of %d, largest %d cells, worst sum error %.3f of its bound" % (tag, found, ref["total"], int(want[:, CN.N].max()) if rows else 0, worst))


def _census(m, f, w, **kw):
    """(table, found, ids, count) as numpy; count through the C ABI's own output"""
    t = m.torch
    table, found, ids = m.census(f, 0.5, weight=w, labels=True, **kw)
    count = t.empty(2, dtype=t.int32, device="cuda")
    tab = t.empty((max(int(kw.get("max_structures", 1024)), 1), 12), dtype=t.float64, device="cuda")
    m._hand("census", m._dev(f), m._dev(w), 0, 0.5, int(kw.get("min_cells", 1)), int(kw.get("max_structures", 1024)), tab, count, None)
    tab = _np(tab)
    rows = table.shape[0]
    assert np.all(tab[rows:, 0] == -1.0) and not tab[rows:, 1:].any()                # the unused rows: label -1 and zeros
    for col in INT_COLS:                                                             # two calls: identical integer columns
        assert np.array_equal(tab[:rows, col], _np(table)[:, col])
    assert _same64(tab[:rows, CN.PEAK], _np(table)[:, CN.PEAK])
    return _np(table), found, _np(ids), _np(count)


def _counts(m, f, w, thr, below=False, min_cells=1, max_structures=1024):
    """d_count of one more call through the C ABI, read back: [found, all structures]"""
    t = m.torch
    count = t.empty(2, dtype=t.int32, device="cuda")
    tab = t.empty((max_structures, 12), dtype=t.float64, device="cuda")
    m._hand("census", m._dev(f), None if w is None else m._dev(w), 1 if below else 0, float(thr), int(min_cells), int(max_structures), tab, count, None)
    return list(_np(count))


@pytest.fixture(scope="module")
def models():
    import xlab_fftbarotropic_amd as X
    made = {}

    def get(nx, ny):
        if (nx, ny) not in made:
            made[(nx, ny)] = X.Model(nx, ny)
        return made[(nx, ny)]
    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("name", list(MASKS))
def test_masks(models, name, nx, ny):
    f, w, ref = _case(name, nx, ny)
    _compare(_census(models(nx, ny), f, w, max_structures=65536), ref, "%s %dx%d" % (name, nx, ny))


@pytest.mark.parametrize("n", [256, 1024])
def test_bernoulli_large(models, n):
    f, w = CN.bernoulli(n, n, 5), CN.white(n, n, 3)
    ref = CN.census(f, 0.5, weight=w, max_structures=65536)
    _compare(_census(models(n, n), f, w, max_structures=65536), ref, "bernoulli %d^2" % n)


@pytest.mark.parametrize("nx", [4096, 8192])
def test_lattice(models, nx):
    """Squares of 40 x 40 cells at a pitch of 64 on 4096^2 (64 x 64 of them) and on 8192 x 4096 (128 x 64), a row and a column of them
    across the seams; the expected table in closed form.  4096^2 has exactly 2^24 cells, so only the second grid has flat indices
    beyond 2^24, which a float32 would no longer hold exactly."""
    L = CN.lattice_case(nx=nx)
    assert L["table"][:, CN.LABEL].max() > (2 ** 24 if nx > 4096 else 2 ** 24 - 2 ** 19)
    m = models(nx, 4096)
    t = m.torch
    f, w = t.from_numpy(L["f"]).cuda(), t.from_numpy(L["w"]).cuda()
    table, found, ids = m.census(f, 0.5, weight=w, max_structures=8192, labels=True)
    count = _counts(m, f, w, 0.5, max_structures=8192)
    _compare((_np(table), found, _np(ids), count), {"table": L["table"], "bound": L["bound"], "found": L["found"], "total": L["found"], "ids": L["ids"]}, "lattice %dx4096" % nx)
    table2, found2 = m.census(f, 0.5, weight=w, max_structures=8192)
    for col in INT_COLS:
        assert np.array_equal(_np(table2)[:, col], _np(table)[:, col])


def test_unaligned_weight(models):
    """a weight that is a contiguous view one float into its allocation, so not 16-byte aligned: the scalar path of k_census_sums"""
    f, w, ref = _case("bernoulli", 192, 64)
    m = models(192, 64)
    t = m.torch
    buf = t.empty(192 * 64 + 1, dtype=t.float32, device="cuda")
    wu = buf[1:].view(192, 64)
    wu.copy_(t.from_numpy(w))
    assert wu.data_ptr() % 16 == 4 and wu.is_contiguous()
    table, found, ids = m.census(f, 0.5, weight=wu, max_structures=65536, labels=True)
    _compare((_np(table), found, _np(ids), _counts(m, f, wu, 0.5, max_structures=65536)), ref, "unaligned weight")
    fb = t.empty(192 * 64 + 1, dtype=t.float32, device="cuda")
    fu = fb[1:].view(192, 64)
    fu.copy_(t.from_numpy(f))
    table, found, ids = m.census(fu, 0.5, weight=wu, max_structures=65536, labels=True)       # the mask field too
    _compare((_np(table), found, _np(ids), _counts(m, fu, wu, 0.5, max_structures=65536)), ref, "unaligned field and weight")


def test_below_and_weight_none(models):
    nx, ny = 192, 64
    m = models(nx, ny)
    f = CN.white(nx, ny, 21)
    f[5, 7] = np.nan
    for below, thr in ((True, -0.3), (False, 0.4)):
        ref = CN.census(f, thr, below=below, max_structures=65536)
        assert ref["found"] >= 50
        table, found, ids = m.census(f, thr, below=below, max_structures=65536, labels=True)       # weight=None: w = f
        _compare((_np(table), found, _np(ids), _counts(m, f, None, thr, below=below, max_structures=65536)), ref, "below=%s weight=None" % below)
        assert np.all(_np(table)[:, CN.S_W] < 0.0 if below else _np(table)[:, CN.S_W] > 0.0)


def test_min_cells_and_max_structures(models):
    f, w, full = _case("bernoulli", 64, 256)
    m = models(64, 256)
    ref = CN.census(f, 0.5, weight=w, min_cells=4, max_structures=65536)
    assert 0 < ref["found"] < full["found"] == ref["total"]
    got = _census(m, f, w, min_cells=4, max_structures=65536)
    _compare(got, ref, "min_cells=4")
    small = full["ids"] >= 0
    small &= ref["ids"] < 0
    assert small.any() and np.all(got[2][small] == -1)                      # the dropped structures: -1 in the map, the ids recounted
    cut = 10
    assert full["found"] > cut
    refc = CN.census(f, 0.5, weight=w, max_structures=cut)
    got = _census(m, f, w, max_structures=cut)
    _compare(got, refc, "max_structures=10", max_structures=cut)
    assert got[1] == full["found"] and got[2].max() == full["found"] - 1    # found unchanged, the map's ids go beyond the table
    for col in INT_COLS:
        assert np.array_equal(got[0][:, col], full["table"][:cut, col])


@pytest.mark.parametrize("kind", ["kuo2004", "elliptic"])
def test_physical_fields(kind):
    """zeta of make_field's Kuo2004 and of the elliptic vortex at 256^2 after 20 steps, through census() with field=None, against
    the reference on vort(); then W from okubo_weiss() as the mask, below=True, zeta as the weight; the vorticity after the
    census calls is bit-equal to a run without them"""
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field(kind, n)
    m = X.Model(n, n)
    m.set_vort(v0)
    m.step(20)
    z = _np(m.vort())
    thr = 0.1 * float(z.max())
    ref = CN.census(z, thr, max_structures=1024)
    assert ref["found"] >= 1
    table, found, ids = m.census(threshold=thr, labels=True)
    _compare((_np(table), found, _np(ids), _counts(m, z, None, thr)), ref, "%s zeta" % kind, max_structures=1024)
    shapes = X.census_shapes(_np(table), n, n, m.Lx, m.Ly)
    assert shapes.shape == (found, 10) and np.all(shapes[:, 0] > 0)
    W = m.okubo_weiss()[0]
    wthr = -0.2 * float(_np(W).std())
    ref = CN.census(_np(W), wthr, below=True, weight=z, min_cells=4, max_structures=1024)
    assert ref["found"] >= 1
    table, found, ids = m.census(W, wthr, below=True, weight=m.vort(), min_cells=4, labels=True)
    _compare((_np(table), found, _np(ids), _counts(m, W, z, wthr, below=True, min_cells=4)), ref, "%s W" % kind, max_structures=1024)
    m.step(5)
    after = _np(m.vort())
    m.close()
    m = X.Model(n, n)
    m.set_vort(v0)
    m.step(25)
    assert np.array_equal(_np(m.vort()).view(np.uint32), after.view(np.uint32))
    m.close()


def test_census_between_captured_steps_and_info():
    """a captured step (use_graph) is not disturbed by a census between its replays, and fb_model_info counts the census's buffers"""
    import torch
    import xlab_fftbarotropic_amd as X
    n = 256
    v0 = X.make_field("kuo2004", n)
    out = []
    for with_census in (False, True):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            m = X.Model(n, n)
            m.fop.use_current_stream()
            m.use_graph(True)
            m.set_vort(v0)
            hbm0 = m.info()["hbm_bytes"]
            for _ in range(4):
                m.step(3)
                if with_census:
                    m.census(threshold=1e-4)
            if with_census:
                assert m.info()["hbm_bytes"] == hbm0 + 2 * n * n * 4 + n * n // 128
            out.append(_np(m.vort()))
            m.close()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


def test_slab_of_one_rank_matches_the_model(models):
    S = _slab()
    f, w, ref = _case("bernoulli", 64, 256)
    got = _census(models(64, 256), f, w, max_structures=65536)
    s = S.EngineSlab(64, 256)
    table, found, ids = s.census(f, 0.5, weight=w, max_structures=65536, labels=True)
    s.close()
    assert found == got[1] and np.array_equal(_np(ids), got[2])
    for col in INT_COLS:
        assert np.array_equal(_np(table)[:, col], got[0][:, col])
    assert _same64(_np(table)[:, CN.PEAK], got[0][:, CN.PEAK])


def test_refusals(models):
    import ctypes as C
    import xlab_fftbarotropic_amd as X
    m = models(64, 64)
    t = m.torch
    f = t.zeros((64, 64), dtype=t.float32, device="cuda")
    table = t.empty((4, 12), dtype=t.float64, device="cuda")
    count = t.empty(2, dtype=t.int32, device="cuda")
    L = X.lib()
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())           # noqa: E731
    cases = [
        ((p(None), None, 0, 0.5, 1, 4, p(table), p(count), None), "NULL field, table or count"),
        ((p(f), None, 0, 0.5, 1, 4, p(None), p(count), None), "NULL field, table or count"),
        ((p(f), None, 0, 0.5, 1, 4, p(table), p(None), None), "NULL field, table or count"),
        ((p(f), None, 0, float("nan"), 1, 4, p(table), p(count), None), "threshold is not finite"),
        ((p(f), None, 0, float("inf"), 1, 4, p(table), p(count), None), "threshold is not finite"),
        ((p(f), None, 2, 0.5, 1, 4, p(table), p(count), None), "mode outside {0, 1}"),
        ((p(f), None, -1, 0.5, 1, 4, p(table), p(count), None), "mode outside {0, 1}"),
        ((p(f), None, 0, 0.5, 0, 4, p(table), p(count), None), "min_cells outside [1, 2^30]"),
        ((p(f), None, 0, 0.5, (1 << 30) + 1, 4, p(table), p(count), None), "min_cells outside [1, 2^30]"),
        ((p(f), None, 0, 0.5, 1, 0, p(table), p(count), None), "max_structures outside [1, 65536]"),
        ((p(f), None, 0, 0.5, 1, 65537, p(table), p(count), None), "max_structures outside [1, 65536]"),
    ]
    for args, what in cases:
        assert L.fb_model_census(m._h, *args) == 1, what                     # FB_EINVAL
        msg = L.fb_last_error().decode()
        assert msg.startswith("fb_model_census: ") and what in msg, (what, msg)
    # the handle is checked before the arguments
    assert L.fb_model_census(None, None, None, 7, float("nan"), 0, 0, None, None, None) == 1 and L.fb_last_error().decode() == "fb_model_census: NULL model"
    assert L.fb_slab_census(None, None, None, 7, float("nan"), 0, 0, None, None, None) == 1 and L.fb_last_error().decode() == "fb_slab_census: NULL slab"
    with pytest.raises(X.FftBaroError, match="max_structures outside"):
        m.census(f, 0.5, max_structures=0)
    with pytest.raises(X.FftBaroError, match="min_cells outside"):
        m.census(f, 0.5, min_cells=0)


def test_slab_of_two_ranks_is_refused():
    """world = 2, ranks as threads of this process: the census raises the engine's unsupported error before any buffer is shaped"""
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
                for call in (lambda: s.census(threshold=0.0), lambda: s.census(np.zeros((s.XL, n), np.float32), 0.5, labels=True)):
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
        assert len(msgs[r]) == 2
        for msg in msgs[r]:
            assert msg is not None and msg.startswith("unsupported") and "fb_slab_census" in msg and "not supported" in msg and "world > 1" in msg, msg


def _run_driver(d, n, v0, extra, steps=21):
    import subprocess
    (d / "input").mkdir(parents=True)
    (d / "output").mkdir()
    v0.tofile(str(d / "input" / "initial_vorticity.bin"))
    r = subprocess.run([os.path.join(HOST, "barotropic_main.out"), "--npts", str(n), "--steps", str(steps), "--record-step", "10", "--no-timing"] + extra,
                       cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return r.returncode, r.stderr.decode(), (d / "log").read_text().split() if (d / "log").exists() else []


def test_driver_census(tmp_path):
    """barotropic_main.out --dump-census at 256^2, 20 steps, a record every 10: census_step_N.bin is the last file of each record in
    ./log, holds M x 12 x 8 bytes and equals Model.census at the same steps in the integer columns and the peak; the same with the
    Okubo-Weiss parameter as the mask; a missing threshold, refused arguments and --world 2 end with exit status 2."""
    import subprocess
    import xlab_fftbarotropic_amd as X
    subprocess.check_call(["make", "-s", "-C", HOST])
    n, M = 256, 16
    v0 = X.make_field("kuo2004", n)
    thr, wthr = float(np.float32(0.1 * float(v0.max()))), float(np.float32(-1e-9))     # float32 values: the driver parses them to the same bits
    runs = {"vort": (["--census-threshold", repr(thr)], ("vort_src_input", "vort", "psi", "u", "v", "azimuthal", "azimuthal_center", "census")),
            "ow": (["--census-threshold", repr(wthr), "--census-field", "okubo-weiss", "--census-below", "--census-min-cells", "2"],
                   ("vort_src_input", "vort", "psi", "u", "v", "azimuthal", "azimuthal_center", "census")),
            # with --dump-okubo-weiss the census takes W from the record's own buffer
            "ow-dumped": (["--census-threshold", repr(wthr), "--census-field", "okubo-weiss", "--census-below", "--census-min-cells", "2", "--dump-okubo-weiss"],
                          ("vort_src_input", "vort", "psi", "u", "v", "okubo_weiss", "tau_fil", "azimuthal", "azimuthal_center", "census"))}
    for tag, (extra, names) in runs.items():
        rc, err, log = _run_driver(tmp_path / tag, n, v0, ["--dump-census", "--census-max", str(M), "--dump-azimuthal"] + extra)
        assert rc == 0, err
        assert log == ["output/%s_step_%d.bin" % (name, s) for s in (0, 10, 20) for name in names]
        m = X.Model(n, n)
        m.set_vort(v0)
        for s in (0, 10, 20):
            f = tmp_path / tag / "output" / ("census_step_%d.bin" % s)
            assert f.stat().st_size == M * 12 * 8
            got = np.fromfile(str(f), dtype="<f8").reshape(M, 12)
            if tag == "vort":
                table, found = m.census(threshold=thr, min_cells=4, max_structures=M)
            else:
                table, found = m.census(m.okubo_weiss()[0], wthr, below=True, weight=m.vort(), min_cells=2, max_structures=M)
            table = _np(table)
            rows = table.shape[0]
            assert rows >= 1, (tag, s)
            for col in INT_COLS:
                assert np.array_equal(got[:rows, col], table[:, col]), (tag, s, col)
            assert _same64(got[:rows, CN.PEAK], table[:, CN.PEAK])
            assert np.all(got[rows:, 0] == -1.0) and not got[rows:, 1:].any()
            m.step(10)
        m.close()
    bad = {"no-threshold": ["--dump-census"], "min": ["--dump-census", "--census-threshold", "1", "--census-min-cells", "0"],
           "max": ["--dump-census", "--census-threshold", "1", "--census-max", "65537"], "thr": ["--dump-census", "--census-threshold", "nan"],
           "field": ["--dump-census", "--census-threshold", "1", "--census-field", "psi"],
           "world": ["--dump-census", "--census-threshold", "1", "--world", "2", "--ranks-as-threads"]}
    for tag, extra in bad.items():
        rc, err, _ = _run_driver(tmp_path / tag, n, v0, extra, steps=1)
        assert rc == 2, (tag, rc, err)
        assert len(err.strip().splitlines()) == 1 and "census" in err, (tag, err)
