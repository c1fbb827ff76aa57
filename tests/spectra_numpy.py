"""float64 numpy restatement of the shell spectra table (include/fftbaro.h, fb_model_get_spectra): the yardstick of
tests/test_gpu_spectra.py and tests/test_spectra_cpu.py.  Built from a half spectrum and coefficient tables handed in, never from the
code under test."""
import math

import numpy as np

TWO_PI = 6.283185307179586
COLS = 10


def geometry(nx, ny, lx, ly):
    """(k2 [nx][ny/2+1], shell index b, w, dk, smallest distance of a mode from a shell edge in shells), all float64"""
    lx, ly = float(np.float32(lx)), float(np.float32(ly))
    i = np.arange(nx)
    ip = np.minimum(i, nx - i).astype(np.float64)
    j = np.arange(ny // 2 + 1, dtype=np.float64)
    kx, ky = TWO_PI * ip / lx, TWO_PI * j / ly
    k2 = (kx * kx)[:, None] + (ky * ky)[None, :]
    dk = TWO_PI / max(lx, ly)
    t = np.sqrt(k2) / dk
    b = np.floor(t + 0.5).astype(np.int64)
    w = np.full(ny // 2 + 1, 2.0)
    w[0] = w[ny // 2] = 1.0
    edge = float(np.abs(t - (np.floor(t) + 0.5)).min())
    return k2, b, np.broadcast_to(w[None, :], k2.shape), dk, edge


def nshells(nx, ny, lx, ly):
    lx, ly = float(np.float32(lx)), float(np.float32(ly))
    dk = TWO_PI / max(lx, ly)
    return int(math.floor(math.sqrt((math.pi * nx / lx) ** 2 + (math.pi * ny / ly) ** 2) / dk + 0.5)) + 1


def nonlinear64(spec, tables):
    """the unnormalised r2c of J = -u zeta_x - v zeta_y in float64 from a natural half spectrum and the engine's coefficient tables
    (main.cpp:151-227 without vort_src); also the four physical fields (zeta_x, zeta_y, u, v)"""
    gx, gy, lap, _, _ = tables
    nx, hy = spec.shape
    ny = 2 * (hy - 1)
    s = spec.astype(np.complex128)
    li = lap.astype(np.float64).copy()
    li[0, 0] = 1.0
    psi = s / li
    kx, ky = gx.astype(np.float64)[:, None], gy.astype(np.float64)[None, :]
    i2 = lambda a: np.fft.irfft2(a, s=(nx, ny))
    zx, zy = i2(1j * kx * s), i2(1j * ky * s)
    u, v = -i2(1j * ky * psi), i2(1j * kx * psi)
    return np.fft.rfft2(-u * zx - v * zy), (zx, zy, u, v)


def table64(spec, nhat, mask, nu, lx, ly):
    """the table [nshells][10] in float64 from the state's half spectrum, N (unnormalised, unmasked) and the dealiasing mask; also
    sum w |a| |n| per shell (the scale of the transfer's rounding)"""
    nx, hy = spec.shape
    ny = 2 * (hy - 1)
    k2, b, w, dk, _ = geometry(nx, ny, lx, ly)
    ns = nshells(nx, ny, lx, ly)
    assert int(b.max()) == ns - 1
    g = float(nx) * float(ny)
    m = mask.astype(np.float64)
    a = spec.astype(np.complex128) / g
    n = m * nhat.astype(np.complex128) / g
    p = a.real * a.real + a.imag * a.imag
    k2s = np.where(k2 > 0.0, k2, 1.0)
    nz = (k2 > 0.0).astype(np.float64)
    t = w * (a.real * n.real + a.imag * n.imag)
    s = lambda x: np.bincount(b.ravel(), weights=np.ascontiguousarray(x).ravel(), minlength=ns)
    tab = np.zeros((ns, COLS))
    bb = np.arange(ns, dtype=np.float64)
    tab[:, 0] = np.maximum(bb - 0.5, 0.0) * dk
    tab[:, 1] = (bb + 0.5) * dk
    tab[:, 2] = s(w)
    tab[:, 3] = s(nz * w * p / (2.0 * k2s))
    tab[:, 4] = s(w * p / 2.0)
    tab[:, 5] = s(nz * t / k2s)
    tab[:, 6] = s(t)
    tab[:, 7] = -np.cumsum(tab[:, 5])
    tab[:, 8] = -np.cumsum(tab[:, 6])
    tab[:, 9] = s(m * float(np.float32(nu)) * k2 * w * p)
    return tab, s(w * np.abs(a) * np.abs(n)), s(nz * w * np.abs(a) * np.abs(n) / k2s)
