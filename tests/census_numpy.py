"""The vortex census of include/fftbaro.h (fb_model_census) restated in float64 numpy: the yardstick of tests/test_census_cpu.py and
tests/test_gpu_census.py.  Labelling is by min-hooking over the edge list plus pointer jumping until nothing changes; no scipy needed
(scipy_labels is the optional cross-check).  `connectivity` and `wrap_x` exist to build the two deliberately wrong references."""
import numpy as np

COLS = 12
(LABEL, N, S_W, S_WX, S_WY, S_WXX, S_WYY, S_WXY, S_X, S_Y, PEAK, PEAK_INDEX) = range(COLS)
SUM_COLS = (S_W, S_WX, S_WY, S_WXX, S_WYY, S_WXY, S_X, S_Y)


def mask_of(f, threshold, below=False):
    f = np.asarray(f, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return f < np.float32(threshold) if below else f > np.float32(threshold)


def _edges(mask, connectivity, wrap_x, wrap_y):
    """the pairs (a, b) of flat indices of neighbouring mask cells"""
    nx, ny = mask.shape
    idx = np.arange(nx * ny, dtype=np.int64).reshape(nx, ny)
    shifts = [(1, 0), (0, 1)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    out = []
    for di, dj in shifts:
        m2, i2 = np.roll(mask, (-di, -dj), axis=(0, 1)), np.roll(idx, (-di, -dj), axis=(0, 1))
        ok = mask & m2
        if not wrap_x and di:
            ok[nx - di:, :] = False
        if not wrap_y and dj:
            if dj > 0:
                ok[:, ny - dj:] = False
            else:
                ok[:, :-dj] = False
        out.append(np.stack([idx[ok], i2[ok]], axis=1))
    return np.concatenate(out, axis=0)


def label_roots(mask, connectivity=4, wrap_x=True, wrap_y=True):
    """int64 [nx, ny]: the smallest flat index of every mask cell's structure, -1 off the mask; and the number of rounds it took"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    lab = np.where(mask.ravel(), np.arange(n, dtype=np.int64), -1)
    e = _edges(mask, connectivity, wrap_x, wrap_y)
    rounds = 0
    while True:
        rounds += 1
        before = lab.copy()
        if e.size:
            ra, rb = lab[e[:, 0]], lab[e[:, 1]]
            lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
            np.minimum.at(lab, hi, lo)                      # hook the larger root under the smaller
        while True:                                         # pointer jumping
            on = lab >= 0
            nxt = lab.copy()
            nxt[on] = lab[lab[on]]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, before):
            return lab.reshape(mask.shape), rounds


def scipy_labels(mask):
    """the same roots through scipy.ndimage.label plus a merge over both seams (raises ImportError without scipy)"""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    nx, ny = mask.shape
    lab, k = ndimage.label(mask)
    parent = np.arange(k + 1)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    pairs = [(lab[nx - 1, j], lab[0, j]) for j in range(ny)] + [(lab[i, ny - 1], lab[i, 0]) for i in range(nx)]
    for a, b in pairs:
        if a and b:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([find(a) for a in range(k + 1)])[lab]
    flat = np.arange(nx * ny, dtype=np.int64).reshape(nx, ny)
    smallest = np.full(k + 1, nx * ny, dtype=np.int64)
    np.minimum.at(smallest, comp.ravel(), flat.ravel())
    return np.where(mask, smallest[comp], -1)


def terms(roots, w, Lx, Ly):
    """the eight summands of every cell, float64 [8, nx, ny] in the order of SUM_COLS, as the engine forms them: w widened exactly, every
    product one correctly rounded multiply, (w ex) ex, (w ey) ey, (w ex) ey; zeros off the mask"""
    nx, ny = roots.shape
    dx, dy = float(np.float32(Lx)) / nx, float(np.float32(Ly)) / ny
    on = roots >= 0
    r = np.where(on, roots, 0)
    i, j = np.meshgrid(np.arange(nx, dtype=np.int64), np.arange(ny, dtype=np.int64), indexing="ij")
    ex = (np.mod(i - r // ny + nx // 2, nx) - nx // 2).astype(np.float64) * dx
    ey = (np.mod(j - r % ny + ny // 2, ny) - ny // 2).astype(np.float64) * dy
    wd = np.asarray(w, dtype=np.float32).astype(np.float64)
    wx, wy = wd * ex, wd * ey
    t = np.stack([wd, wx, wy, wx * ex, wy * ey, wx * ey, ex, ey])
    return np.where(on[None], t, 0.0)


def census(f, threshold, below=False, weight=None, min_cells=1, max_structures=1024, Lx=600000.0, Ly=600000.0, connectivity=4, wrap_x=True, wrap_y=True):
    """dict: table float64 [max_structures, 12] (rows beyond the structures found: label -1 and zeros), found, total (all structures
    before min_cells), ids int32 [nx, ny] (the dense id of every kept structure's cells, -1 elsewhere), bound float64
    [max_structures, 12]: per sum column n 2^-52 sum |term|, the float64 bound for two summation orders of bit-equal terms (0 elsewhere),
    rounds."""
    f = np.asarray(f, dtype=np.float32)
    w = f if weight is None else np.asarray(weight, dtype=np.float32)
    nx, ny = f.shape
    roots, rounds = label_roots(mask_of(f, threshold, below), connectivity, wrap_x, wrap_y)
    flat = roots.ravel()
    on = flat >= 0
    cells = np.bincount(flat[on], minlength=nx * ny)
    all_roots = np.nonzero(cells > 0)[0]
    kept = all_roots[cells[all_roots] >= min_cells]        # ascending: the label order
    dense = np.full(nx * ny, -1, dtype=np.int64)
    dense[kept] = np.arange(kept.size)
    ids = np.where(on, dense[np.where(on, flat, 0)], -1).astype(np.int32)
    table = np.zeros((max_structures, COLS))
    bound = np.zeros((max_structures, COLS))
    table[:, LABEL] = -1.0
    rows = min(kept.size, max_structures)
    sel = (ids >= 0) & (ids < rows)
    t = terms(roots, w, Lx, Ly).reshape(8, -1)
    table[:rows, LABEL] = kept[:rows]
    table[:rows, N] = cells[kept[:rows]]
    for k, col in enumerate(SUM_COLS):
        table[:rows, col] = np.bincount(ids[sel], weights=t[k][sel], minlength=rows)[:rows]
        bound[:rows, col] = table[:rows, N] * 2.0 ** -52 * np.bincount(ids[sel], weights=np.abs(t[k][sel]), minlength=rows)[:rows]
    # the peak: largest |w|, a NaN never wins, ties to the smallest flat index
    wf = w.ravel()
    a = np.where(np.isnan(wf), -1.0, np.abs(wf).astype(np.float64))
    cand = np.nonzero(sel)[0]
    order = cand[np.lexsort((cand, -a[cand], ids[cand]))]    # by id, then |w| downward, then index
    first = order[np.concatenate([[True], ids[order][1:] != ids[order][:-1]])] if order.size else order
    for c in first:
        r = ids[c]
        table[r, PEAK], table[r, PEAK_INDEX] = (float(wf[c]), float(c)) if a[c] >= 0 else (np.nan, -1.0)
    return {"table": table, "found": int(kept.size), "total": int(all_roots.size), "ids": ids.reshape(nx, ny), "bound": bound, "rounds": rounds, "roots": roots}


# ---- the masks of the tests, as fields of 0 / 1 (threshold 0.5) ----
def spiral(nx, ny):
    """a one-cell-wide spiral walked inwards from (1, 1) with one-cell gaps between its turns: the longest union chains"""
    m = np.zeros((nx, ny), dtype=np.float32)
    i, j, di, dj = 1, 1, 0, 1
    m[i, j] = 1

    def touching(a, b):
        return sum(m[a + p, b + q] for p, q in ((1, 0), (-1, 0), (0, 1), (0, -1)))
    while True:
        for _ in range(2):                                  # straight on while the cell ahead touches the spiral at its head alone, else turn once
            a, b = i + di, j + dj
            if 1 <= a < nx - 1 and 1 <= b < ny - 1 and m[a, b] == 0 and touching(a, b) == 1:
                break
            di, dj = dj, -di
        else:
            return m
        i, j = a, b
        m[i, j] = 1


def comb(nx, ny):
    """teeth along i in every other column that join only in the last row"""
    m = np.zeros((nx, ny), dtype=np.float32)
    m[1:nx - 1, 1:ny - 1:2] = 1
    m[nx - 2, 1:ny - 1] = 1
    return m


def corners(nx, ny, h=5, k=7):
    """four corner blocks: one structure through both seams"""
    m = np.zeros((nx, ny), dtype=np.float32)
    for si in (slice(0, h), slice(nx - h, nx)):
        for sj in (slice(0, k), slice(ny - k, ny)):
            m[si, sj] = 1
    return m


def checkerboard(nx, ny):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return ((i + j) % 2 == 0).astype(np.float32)


def bernoulli(nx, ny, seed, p=0.59):
    return (np.random.default_rng(seed).random((nx, ny)) < p).astype(np.float32)


def seam_cross(nx, ny):
    """ONE structure whose cells touch all four edges and whose parts hang together through the seams alone: a block on the first rows
    joined through the x seam to a block on the last rows, whose arm reaches j = 0 and is joined through the y seam to a piece on the
    last columns.  Beside it one satellite cell that touches the first block by a corner only: a structure of its own in 4-connectivity."""
    m = np.zeros((nx, ny), dtype=np.float32)
    m[0:4, 10:21] = 1
    m[nx - 4:nx, 10:21] = 1
    m[nx - 2, 0:10] = 1
    m[nx - 2, ny - 6:ny] = 1
    m[4, 21] = 1
    return m


def white(nx, ny, seed):
    return np.random.default_rng(seed).standard_normal((nx, ny)).astype(np.float32)


def lattice_case(n=4096, per=64, side=40, shift=(-17, -9), seed=11, nx=None):
    """The lattice of squares of side x side cells at a pitch of n / per cells on an nx x n grid (nx = n unless given, a multiple of the
    pitch), shifted so that a row and a column of squares straddle the seams, with its expected table built in closed form by
    reshaping (no labelling): f (0 / 1), w (float32), table [squares, 12] in label order, bound, ids [nx, n], found."""
    ny, p = n, n // per
    nx = nx or n
    px, py = nx // p, per                                                                                 # squares along i and along j
    rng = np.random.default_rng(seed)
    w0 = rng.standard_normal((nx, ny)).astype(np.float32)
    block = np.zeros((p, p), dtype=bool)
    block[:side, :side] = True
    f0 = np.tile(block, (px, py))
    f, w = np.roll(f0, shift, axis=(0, 1)).astype(np.float32), np.roll(w0, shift, axis=(0, 1))
    # per square (a, b) of the unshifted lattice, its cells [a p + r, b p + s], r, s < side
    cells = w0.reshape(px, p, py, p)[:, :side, :, :side].transpose(0, 2, 1, 3).astype(np.float64)        # [a, b, r, s]
    gi = (np.arange(px)[:, None] * p + np.arange(side)[None, :] + shift[0]) % nx                          # [a, r] shifted row
    gj = (np.arange(py)[:, None] * p + np.arange(side)[None, :] + shift[1]) % ny                          # [b, s] shifted column
    flat = gi[:, None, :, None] * ny + gj[None, :, None, :]                                               # [a, b, r, s]
    nsq = px * py
    label = flat.reshape(px, py, -1).min(axis=2)
    i0, j0 = label // ny, label % ny
    ex = ((gi[:, None, :, None] - i0[:, :, None, None] + nx // 2) % nx - nx // 2).astype(np.float64) * (600000.0 / nx)
    ey = ((gj[None, :, None, :] - j0[:, :, None, None] + ny // 2) % ny - ny // 2).astype(np.float64) * (600000.0 / ny)
    ex, ey = np.broadcast_to(ex, cells.shape), np.broadcast_to(ey, cells.shape)
    wx, wy = cells * ex, cells * ey
    t = [cells, wx, wy, wx * ex, wy * ey, wx * ey, ex, ey]
    table = np.zeros((nsq, COLS))
    bound = np.zeros((nsq, COLS))
    table[:, LABEL] = label.ravel()
    table[:, N] = side * side
    for k, col in enumerate(SUM_COLS):
        table[:, col] = t[k].reshape(nsq, -1).sum(axis=1)
        bound[:, col] = side * side * 2.0 ** -52 * np.abs(t[k]).reshape(nsq, -1).sum(axis=1)
    a = np.abs(cells).reshape(nsq, -1)
    fl = flat.reshape(nsq, -1)
    best = a.max(axis=1, keepdims=True)
    at = np.where(a == best, fl, nx * ny).min(axis=1)
    table[:, PEAK], table[:, PEAK_INDEX] = w.ravel()[at].astype(np.float64), at
    order = np.argsort(table[:, LABEL])
    rank = np.empty(nsq, dtype=np.int64)
    rank[order] = np.arange(nsq)
    ids = np.full((nx, ny), -1, dtype=np.int32)
    ids.ravel()[fl.ravel()] = np.repeat(rank, side * side).astype(np.int32)
    return {"f": f, "w": w, "table": table[order], "bound": bound[order], "ids": ids, "found": nsq}
