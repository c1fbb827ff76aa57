"""CPU checks of the vortex census's yardstick (tests/census_numpy.py) and of census_shapes: the conditions on the inputs that make
the cases of tests/test_gpu_census.py meaningful.  No GPU, no scipy needed (the scipy cross-check runs where scipy imports)."""
import numpy as np
import pytest

import census_numpy as CN

GRIDS = [(64, 64), (192, 64), (64, 256)]
# (name, nx, ny, seed): the Bernoulli(0.59) cases of the GPU tests, each with its own seed
# The scipy cross-check and the wrong references leave the 1024^2 case out: each is one or two further labellings of a million cells in
# numpy, tens of seconds for a property that the four smaller cases of the same generator already show at every grid shape.
BERNOULLI = [("b64", 64, 64, 5), ("b192x64", 192, 64, 6), ("b64x256", 64, 256, 7), ("b256", 256, 256, 5), ("b1024", 1024, 1024, 5)]


def _count(f, **kw):
    r = CN.census(f, 0.5, max_structures=65536, **kw)
    return r, r["table"][:min(r["found"], 65536)]


@pytest.mark.parametrize("name,nx,ny,seed", BERNOULLI)
def test_bernoulli_cases_have_many_structures_and_a_large_one(name, nx, ny, seed):
    r, t = _count(CN.bernoulli(nx, ny, seed))
    assert r["found"] >= 50 and t[:, CN.N].max() >= 1000, (r["found"], t[:, CN.N].max())
    assert np.all(np.diff(t[:, CN.LABEL]) > 0)                  # dense ids in label order
    assert t[:, CN.N].sum() == (r["ids"] >= 0).sum()


@pytest.mark.parametrize("name,nx,ny,seed", BERNOULLI[:4])
def test_labelling_agrees_with_scipy(name, nx, ny, seed):
    pytest.importorskip("scipy.ndimage")
    f = CN.bernoulli(nx, ny, seed)
    assert np.array_equal(CN.scipy_labels(f > 0.5), CN.label_roots(f > 0.5)[0])


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_structured_masks_are_what_they_claim(nx, ny):
    r, t = _count(CN.seam_cross(nx, ny))
    on = r["ids"] == 0
    assert on[0].any() and on[-1].any() and on[:, 0].any() and on[:, -1].any()       # ONE structure on all four edges ...
    assert r["found"] == 2 and t[1, CN.N] == 1 and on.sum() == t[0, CN.N] == 2 * 4 * 11 + 10 + 6       # ... and its one-cell satellite
    r, t = _count(CN.corners(nx, ny))
    assert r["found"] == 1 and t[0, CN.N] == 4 * 5 * 7 and t[0, CN.LABEL] == 0
    r, t = _count(CN.checkerboard(nx, ny))
    assert r["found"] == nx * ny // 2 and np.all(t[:, CN.N] == 1)
    r, t = _count(CN.comb(nx, ny))
    assert r["found"] == 1
    r2, _ = _count(CN.comb(nx, ny) * (np.arange(nx)[:, None] != nx - 2))           # without the last row: every tooth on its own
    assert r2["found"] == (ny - 2 + 1) // 2
    sp = CN.spiral(nx, ny)
    r, t = _count(sp)
    assert r["found"] == 1 and t[0, CN.N] >= nx * ny // 3
    nb = sum(np.roll(sp, s, axis=a) for s in (1, -1) for a in (0, 1))
    assert np.all(nb[sp > 0] <= 2)                               # a chain, one cell wide
    r, _ = _count(np.zeros((nx, ny), np.float32))
    assert r["found"] == 0 and r["total"] == 0 and np.all(r["table"][:, CN.LABEL] == -1) and not r["table"][:, 1:].any()
    r, t = _count(np.ones((nx, ny), np.float32))
    assert r["found"] == 1 and t[0, CN.N] == nx * ny


def test_nan_is_never_in_the_mask_and_never_the_peak():
    f = CN.bernoulli(64, 64, 8)
    f[3:9, 4:30] = np.nan
    w = CN.white(64, 64, 9)
    w[20:24, :] = np.nan
    for below in (False, True):
        r = CN.census(f, 0.5, below=below, weight=w)
        assert np.all(r["ids"][3:9, 4:30] == -1)
        t = r["table"][:r["found"]]
        ok = t[:, CN.PEAK_INDEX] >= 0
        assert ok.any() and np.all(np.isfinite(t[ok, CN.PEAK]))
        assert np.array_equal(w.ravel()[t[ok, CN.PEAK_INDEX].astype(int)].astype(np.float64), t[ok, CN.PEAK])


@pytest.mark.parametrize("case", ["seam"] + [b[0] for b in BERNOULLI[:4]])
def test_wrong_references_change_the_table(case):
    """8-connectivity and a grid without the wrap in x must each change the table of the seam case and of the Bernoulli cases: else the
    GPU comparison could not tell them from the definition"""
    if case == "seam":
        f = CN.seam_cross(64, 64)
    else:
        _, nx, ny, seed = [b for b in BERNOULLI if b[0] == case][0]
        f = CN.bernoulli(nx, ny, seed)
    w = CN.white(f.shape[0], f.shape[1], 1)
    good = CN.census(f, 0.5, weight=w, max_structures=4096)
    for kw in ({"connectivity": 8}, {"wrap_x": False}):
        bad = CN.census(f, 0.5, weight=w, max_structures=4096, **kw)
        assert bad["found"] != good["found"] or not np.array_equal(bad["table"][:, :2], good["table"][:, :2]), kw
        assert not np.array_equal(bad["ids"], good["ids"]), kw


def test_min_cells_and_max_structures():
    f = CN.bernoulli(64, 64, 5)
    full = CN.census(f, 0.5, max_structures=4096)
    r = CN.census(f, 0.5, min_cells=4, max_structures=4096)
    big = full["table"][:full["found"]]
    big = big[big[:, CN.N] >= 4]
    assert r["found"] == len(big) < full["found"] == r["total"] and np.array_equal(r["table"][:r["found"]], big)
    cut = CN.census(f, 0.5, max_structures=10)
    assert cut["found"] == full["found"] and np.array_equal(cut["table"], full["table"][:10]) and cut["ids"].max() == full["found"] - 1


def test_lattice_closed_form_agrees_with_the_labelling():
    """the closed form of the 4096^2 case, at a size the labelling does quickly: the same construction, 16 x 16 squares of 10 x 10 on 256^2"""
    L = CN.lattice_case(n=256, per=16, side=10, shift=(-5, -3), seed=3)
    r = CN.census(L["f"], 0.5, weight=L["w"], max_structures=256)
    assert r["found"] == 256 and np.array_equal(r["ids"], L["ids"])
    for col in (CN.LABEL, CN.N, CN.PEAK, CN.PEAK_INDEX):
        assert np.array_equal(r["table"][:, col], L["table"][:, col]), col
    assert np.all(np.abs(r["table"] - L["table"]) <= L["bound"])
    on = L["ids"] >= 0
    assert on[0].any() and on[-1].any() and on[:, 0].any() and on[:, -1].any()      # squares straddle both seams


def test_shapes_recover_an_elliptic_patch_across_both_seams():
    import xlab_fftbarotropic_amd as X
    n, a0, b0, phi0, xc0, yc0 = 128, 24.0, 12.0, np.deg2rad(30.0), 3.3, 125.6
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    ddx, ddy = (i - xc0 + n / 2) % n - n / 2, (j - yc0 + n / 2) % n - n / 2
    u, v = ddx * np.cos(phi0) + ddy * np.sin(phi0), -ddx * np.sin(phi0) + ddy * np.cos(phi0)
    f = ((u / a0) ** 2 + (v / b0) ** 2 <= 1.0).astype(np.float32)
    on = f > 0
    assert on[0].any() and on[-1].any() and on[:, 0].any() and on[:, -1].any()      # it straddles both seams
    r = CN.census(3.0 * f, 0.5, Lx=float(n), Ly=float(n))                             # dx = dy = 1: lengths in cells; weight 3: uniform
    assert r["found"] == 1
    s = dict(zip(X.CENSUS_SHAPE_COLUMNS, X.census_shapes(r["table"][:1], n, n, float(n), float(n))[0]))
    # Computed when this test was written: a = 24.036, b = 11.972, phi = 30.24 deg, n = 904 against pi a b = 904.8.  The margins cover
    # the rasterisation alone: the patch's edge is cut to whole cells, about 116 boundary cells each off by up to half a cell, which moves the
    # second moments by a few parts in a thousand (0.04 of 24 cells) and the angle by a few tenths of a degree.
    assert abs(s["area"] - np.pi * a0 * b0) <= 5.0 and s["area"] == r["table"][0, CN.N]
    assert s["circulation"] == 3.0 * s["area"]
    assert abs(s["a"] - a0) <= 0.1 and abs(s["b"] - b0) <= 0.1 and abs(np.rad2deg(s["phi"]) - 30.0) <= 0.5
    assert abs(s["aspect"] - 2.0) <= 0.02
    for got, want in ((s["xc"], xc0), (s["yc"], yc0), (s["xg"], xc0), (s["yg"], yc0)):
        assert abs((got - want + n / 2) % n - n / 2) <= 0.1
    # an empty row gives NaN, and a structure of zero weight has no weighted centroid
    z = X.census_shapes(np.array([[-1.0] + [0.0] * 11, [5.0, 2.0] + [0.0] * 10]), n, n, float(n), float(n))
    assert np.all(np.isnan(z[0])) and np.isnan(z[1, 2]) and z[1, 0] == 2.0 and z[1, 4] == 0.0 and z[1, 5] == 5.0


def test_columns_and_signature():
    import xlab_fftbarotropic_amd as X
    B = X.package.binding
    assert X.CENSUS_COLUMNS == ("label", "n", "S_w", "S_wx", "S_wy", "S_wxx", "S_wyy", "S_wxy", "S_x", "S_y", "peak", "peak_index")
    assert len(X.CENSUS_COLUMNS) == CN.COLS and len(X.CENSUS_SHAPE_COLUMNS) == 10
    assert "census" in B._CENSUS_PAIRS and "census" not in B._PAIRS
    L = X.lib()
    assert hasattr(L, "fb_model_census") and hasattr(L, "fb_slab_census")
    assert callable(X.Model.census)
