"""The azimuthal-mean table of include/fftbaro.h (fb_model_get_azimuthal) evaluated in float64 numpy on given float32 fields: the
yardstick of tests/test_azimuthal_cpu.py (analytic fields) and tests/test_gpu_azimuthal.py (the engine's own records).

Vectorised; the radial bin is floor(r / dr) corrected by comparisons of (b dr)^2 with r^2, so that it depends on correctly rounded
multiplies alone and equals the engine's bin for every point.
"""
import numpy as np

BASE_COLS = 12


def grid_steps(nx, ny, Lx, Ly):
    """Lx, Ly, dx, dy as the engine takes them: the float32 lengths widened, divided by the grid size in float64."""
    lx, ly = np.float64(np.float32(Lx)), np.float64(np.float32(Ly))
    return lx, ly, lx / nx, ly / ny


def default_bins(nx, ny, Lx, Ly):
    """(nbins, dr) of the binding's defaults: dr = max(dx, dy), nbins = floor(min(Lx, Ly) / 2 / dr), at most 4096."""
    lx, ly, dx, dy = grid_steps(nx, ny, Lx, Ly)
    dr = max(dx, dy)
    nbins = min(4096, int(np.floor(min(lx, ly) / 2 / dr)))
    while nbins > 2 and nbins * dr > min(lx, ly) / 2:
        nbins -= 1
    return nbins, float(dr)


def find_center(field, Lx, Ly, largest):
    """center[4] = xc, yc, flat index, value of the smallest (largest) element of the [nx][ny] field, ties to the smallest flat index."""
    nx, ny = field.shape
    _, _, dx, dy = grid_steps(nx, ny, Lx, Ly)
    flat = int(np.argmax(field) if largest else np.argmin(field))
    i, j = divmod(flat, ny)
    return np.array([np.float64(i) * dx, np.float64(j) * dy, np.float64(flat), np.float64(field.reshape(-1)[flat])], np.float64)


def geometry(nx, ny, Lx, Ly, xc, yc, dr):
    """(r, c1, s1, b): distance from the centre by the minimum image, cos and sin of the azimuth (1, 0 at the centre), radial bin."""
    lx, ly, dx, dy = grid_steps(nx, ny, Lx, Ly)
    ddx = np.arange(nx, dtype=np.float64) * dx - np.float64(xc)
    ddx = np.where(ddx > lx / 2, ddx - lx, np.where(ddx < -lx / 2, ddx + lx, ddx))
    ddy = np.arange(ny, dtype=np.float64) * dy - np.float64(yc)
    ddy = np.where(ddy > ly / 2, ddy - ly, np.where(ddy < -ly / 2, ddy + ly, ddy))
    ddx, ddy = ddx[:, None] + 0.0 * ddy[None, :], 0.0 * ddx[:, None] + ddy[None, :]
    r2 = ddx * ddx + ddy * ddy
    r = np.sqrt(r2)
    dr = np.float64(dr)
    b = np.floor(r / dr)
    for _ in range(4):                                          # the division and the root are off by an ulp at the most
        b = np.where((b * dr) * (b * dr) > r2, b - 1.0, b)
    for _ in range(4):
        b = np.where(((b + 1.0) * dr) * ((b + 1.0) * dr) <= r2, b + 1.0, b)
    assert np.all((b * dr) * (b * dr) <= r2) and np.all(((b + 1.0) * dr) * ((b + 1.0) * dr) > r2)
    zero = r2 == 0.0
    rs = np.where(zero, 1.0, r)
    c1 = np.where(zero, 1.0, ddx / rs)
    s1 = np.where(zero, 0.0, ddy / rs)
    return r, c1, s1, b.astype(np.int64)


def table(zeta, u, v, Lx, Ly, xc, yc, nbins, dr, nmodes):
    """(table, scale): the table [nbins][12 + 2 nmodes] and, per entry, the bin mean of the absolute value of the summed term (for
    Gamma: dx dy times the running sum of |zeta|): the measure a float64 summation error is held against.  scale is 0 in the
    columns 0-2, which are exact."""
    nx, ny = zeta.shape
    _, _, dx, dy = grid_steps(nx, ny, Lx, Ly)
    r, c1, s1, b = geometry(nx, ny, Lx, Ly, xc, yc, dr)
    z, uu, vv = (np.asarray(a, np.float32).astype(np.float64) for a in (zeta, u, v))
    vr = uu * c1 + vv * s1
    vt = vv * c1 - uu * s1
    terms = [r, z, vt, vr, z * z, vt * vt, vr * vr, vr * z]
    cm, sm = c1, s1
    for _ in range(nmodes):
        terms += [z * cm, z * sm]
        cm, sm = cm * c1 - sm * s1, sm * c1 + cm * s1
    inside = b < nbins
    bi = b[inside]
    n = np.bincount(bi, minlength=nbins).astype(np.float64)
    nc = BASE_COLS + 2 * nmodes
    out, scale = np.zeros((nbins, nc)), np.zeros((nbins, nc))
    k = np.arange(nbins, dtype=np.float64)
    out[:, 0], out[:, 1], out[:, 2] = k * np.float64(dr), (k + 1.0) * np.float64(dr), n
    div = np.where(n > 0, n, 1.0)
    cols = list(range(3, 11)) + list(range(12, nc))
    for col, t in zip(cols, terms):
        s = np.bincount(bi, weights=t[inside], minlength=nbins)
        a = np.bincount(bi, weights=np.abs(t[inside]), minlength=nbins)
        mean = np.where(n > 0, s / div, 0.0)
        out[:, col] = -mean if (col >= 12 and (col - 12) % 2 == 1) else mean
        scale[:, col] = np.where(n > 0, a / div, 0.0)
    sz = np.bincount(bi, weights=z[inside], minlength=nbins)
    sa = np.bincount(bi, weights=np.abs(z[inside]), minlength=nbins)
    out[:, 11] = (dx * dy) * np.cumsum(sz)
    scale[:, 11] = (dx * dy) * np.cumsum(sa)
    return out, scale
