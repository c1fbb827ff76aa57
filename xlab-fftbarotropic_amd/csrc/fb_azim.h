// fb_azim.h -- the azimuthal-mean record path (fb_model_get_azimuthal, fb_slab_get_azimuthal): a vortex centre found in the resident
// state, then zeta, v_t, v_r, their second moments and the azimuthal Fourier coefficients of zeta binned by distance from it.
//   k_azim_arg(_final)   argmin of psi / argmax of zeta with its flat index: per-workgroup partials, then one workgroup in a fixed order
//   k_azim_center        the ranks' candidates in rank order -> center[4] = xc, yc, flat index, value (or the caller's fixed centre)
//   k_azim_bin           a workgroup takes a 2-D tile of points, sums them in an LDS window of bins and adds the window to this rank's
//                        sums [nbins][9 + 2 nmodes] with global float64 atomics
//   k_azim_table         the ranks' sums added in rank order, the means, the running circulation, the table [nbins][12 + 2 nmodes]
// No reference counterpart: the reference ships find_min, run by hand on a psi record; it never forms a radial profile.
#pragma once

enum { AZIM_BASE_COLS = 12, AZIM_BASE_SUMS = 9, AZIM_MAX_MODES = 8, AZIM_TILE = 1024, AZIM_ARG_W = 4 };
// the sums of one bin: 0 n  1 r  2 zeta  3 v_t  4 v_r  5 zeta^2  6 v_t^2  7 v_r^2  8 v_r zeta  9 + 2 (m - 1) zeta c_m  10 + 2 (m - 1) zeta s_m

struct AzimGeo {
    double dx, dy, lx, ly, dr;  // dx = Lx / nx, dy = Ly / ny from the context's float32 lengths widened
    int nbins, XL, ny, row0;    // this rank's rows [row0, row0 + XL) of the whole domain
    int TX, TY, W;              // a tile is TX rows by TY columns (TX TY = AZIM_TILE, TY a multiple of 4 that divides ny); W bins in LDS
};

// the order of the search: a < b for the minimum, a > b for the maximum (as key = -value); ties go to the smaller index; a NaN never wins
FB_DEV bool azim_better(float ka, long long ia, float kb, long long ib) { return ka < kb || (ka == kb && ia < ib); }

FB_DEV void azim_wave_best(float &k, long long &i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float k2 = __shfl_xor(k, o);
        const long long i2 = __shfl_xor(i, o);
        if (azim_better(k2, i2, k, i)) { k = k2; i = i2; }
    }
}

// the best of a workgroup of 256 in every thread
FB_DEV void azim_block_best(float &k, long long &i, float *sk, long long *si)
{
    azim_wave_best(k, i);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sk[w] = k; si[w] = i; }
    __syncthreads();
    k = sk[0]; i = si[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) if (azim_better(sk[q], si[q], k, i)) { k = sk[q]; i = si[q]; }
}

// per-workgroup best (key, local flat index) of q[0, n): key = q for the minimum, -q for the maximum; index LLONG_MAX where no
// element compared (every one a NaN).  pk[blockIdx.x], pi[blockIdx.x].
template <bool MAX>
__global__ void __launch_bounds__(256) k_azim_arg(const float *__restrict__ q, size_t n, float *__restrict__ pk, long long *__restrict__ pi)
{
    __shared__ float sk[4];
    __shared__ long long si[4];
    float k = __builtin_inff();
    long long i = 0x7fffffffffffffffLL;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const float v = MAX ? -q[e] : q[e];
        if (azim_better(v, (long long)e, k, i)) { k = v; i = (long long)e; }
    }
    azim_block_best(k, i, sk, si);
    if (threadIdx.x == 0) { pk[blockIdx.x] = k; pi[blockIdx.x] = i; }
}

// one workgroup of 256: the nparts partials in a fixed order -> this rank's candidate (key, global flat index or -1, value, 0) as
// four doubles, written `copies` times (multi-GPU: the send buffer of the all-gather, one copy per peer)
__global__ void __launch_bounds__(256) k_azim_arg_final(const float *__restrict__ pk, const long long *__restrict__ pi, int nparts, const float *__restrict__ q,
                                                        long long flat0, double *__restrict__ out, int copies)
{
    __shared__ float sk[4];
    __shared__ long long si[4];
    float k = __builtin_inff();
    long long i = 0x7fffffffffffffffLL;
    for (int p = threadIdx.x; p < nparts; p += blockDim.x) if (azim_better(pk[p], pi[p], k, i)) { k = pk[p]; i = pi[p]; }
    azim_block_best(k, i, sk, si);
    const bool found = i != 0x7fffffffffffffffLL;
    const double val = found ? (double)q[i] : 0.0;
    for (int r = threadIdx.x; r < copies; r += blockDim.x) {
        double *o = out + (size_t)r * AZIM_ARG_W;
        o[0] = (double)k; o[1] = found ? (double)(flat0 + i) : -1.0; o[2] = val; o[3] = 0.0;
    }
}

// one thread: center[4] = xc, yc, flat index, value.  cand == NULL: the caller's (xc, yc), index -1, value 0.  Else the best of the
// ranks' candidates cand[world][4] in rank order (a rank's indices lie above those of the ranks before it); no candidate at all
// (a field of NaNs): grid point 0 with the first rank's value.  xc = i dx, yc = j dy of the flat index ny i + j.
__global__ void k_azim_center(const double *__restrict__ cand, int world, double xc, double yc, int ny, double dx, double dy, double *__restrict__ center)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!cand) { center[0] = xc; center[1] = yc; center[2] = -1.0; center[3] = 0.0; return; }
    double k = 0.0, idx = -1.0, val = cand[2];
    for (int r = 0; r < world; ++r) {
        const double *c = cand + (size_t)r * AZIM_ARG_W;
        if (c[1] >= 0.0 && (idx < 0.0 || c[0] < k)) { k = c[0]; idx = c[1]; val = c[2]; }
    }
    if (idx < 0.0) idx = 0.0;
    const long long flat = (long long)idx, i = flat / ny, j = flat - i * ny;
    center[0] = (double)i * dx; center[1] = (double)j * dy; center[2] = idx; center[3] = val;
}

// the bin of r2 = r^2: the integer b with (b dr)^2 <= r2 < ((b + 1) dr)^2, from floor(r / dr) corrected by comparisons, so that it
// depends on correctly rounded multiplies alone (numpy reproduces it).  Clamped far beyond any table.
FB_DEV int azim_bin_of(double r2, double r, double dr)
{
#pragma clang fp contract(off)
    const double q = r / dr;
    double b = q < 1.0e9 ? (double)(long long)q : 1.0e9;
    while (b > 0.0 && (b * dr) * (b * dr) > r2) b -= 1.0;
    while (b < 1.0e9 && ((b + 1.0) * dr) * ((b + 1.0) * dr) <= r2) b += 1.0;
    return (int)b;
}

// A workgroup of 256 takes one tile of TX rows by TY columns, a thread four neighbouring points of a row (one float4 of each field).
// The radii of a tile span at most hypot((TX - 1) dx, (TY - 1) dy) (the minimum image folds the distance, it never stretches it), so
// its bins lie in a window of W = that / dr + 3 bins above the smallest one, found by a reduction over the tile: the sums of the
// window live in LDS [W][NS] (f64).  The bin changes from point to point, so a lane keeps a run (bin, sums) over its four points in
// registers and adds it to LDS when the bin changes -- along a row near the centre's axis the four share a bin --, with LDS float64
// atomics; the window is then added to part[nbins][NS] with global float64 atomics, consecutive lanes on consecutive addresses,
// rows without a point skipped.  A point beyond the window (W is capped by the LDS there is: a grid with dx and dy far apart) goes
// to part directly.  Tiles wholly beyond nbins dr leave at once.  The sums arrive in whatever order the atomics land; the counts
// are whole numbers far below 2^53 and exact.  center: device xc, yc.  NM: the number of azimuthal modes.
template <int NM>
__global__ void __launch_bounds__(256) k_azim_bin(AzimGeo g, const float *__restrict__ zeta, const float *__restrict__ u, const float *__restrict__ v,
                                                  const double *__restrict__ center, double *__restrict__ part)
{
#pragma clang fp contract(off)
    constexpr int NS = AZIM_BASE_SUMS + 2 * NM;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *win = reinterpret_cast<double *>(smem_raw);
    __shared__ int sbase[4];
    const int tq = g.TY / 4, tiles_y = g.ny / g.TY;
    const int tile_i = blockIdx.x / tiles_y, tile_j = blockIdx.x - tile_i * tiles_y;
    const int li = tile_i * g.TX + (int)threadIdx.x / tq, j0 = tile_j * g.TY + ((int)threadIdx.x % tq) * 4;
    const bool valid = li < g.XL;
    const double xc = center[0], yc = center[1];
    int b[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    double rr[4], c1[4], s1[4];
    float4 fz = make_float4(0.f, 0.f, 0.f, 0.f), fu = fz, fv = fz;
    if (valid) {
        const size_t at = (size_t)li * g.ny + j0;
        fz = *reinterpret_cast<const float4 *>(zeta + at);
        fu = *reinterpret_cast<const float4 *>(u + at);
        fv = *reinterpret_cast<const float4 *>(v + at);
        double ddx = (double)(g.row0 + li) * g.dx - xc;
        if (ddx > g.lx / 2) ddx -= g.lx; else if (ddx < -g.lx / 2) ddx += g.lx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double ddy = (double)(j0 + k) * g.dy - yc;
            if (ddy > g.ly / 2) ddy -= g.ly; else if (ddy < -g.ly / 2) ddy += g.ly;
            const double r2 = ddx * ddx + ddy * ddy, r = sqrt(r2);
            b[k] = azim_bin_of(r2, r, g.dr);
            rr[k] = r;
            c1[k] = r2 == 0.0 ? 1.0 : ddx / r;
            s1[k] = r2 == 0.0 ? 0.0 : ddy / r;
        }
    }
    // the window's first bin: the smallest of the tile
    int lo = min(min(b[0], b[1]), min(b[2], b[3]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o));
    if ((threadIdx.x & 63) == 0) sbase[threadIdx.x >> 6] = lo;
    __syncthreads();
    const int base = min(min(sbase[0], sbase[1]), min(sbase[2], sbase[3]));
    if (base >= g.nbins) return;
    for (int e = threadIdx.x; e < g.W * NS; e += blockDim.x) win[e] = 0.0;
    __syncthreads();

    double acc[NS];
    int cb = -1;
    auto flush = [&]() {
        if (cb < 0 || cb >= g.nbins) return;
        const int w = cb - base;
        if (w < g.W) {
#pragma unroll
            for (int k = 0; k < NS; ++k) __hip_atomic_fetch_add(&win[w * NS + k], acc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) unsafeAtomicAdd(&part[(size_t)cb * NS + k], acc[k]);
        }
    };
    if (valid) {
        const float az[4] = {fz.x, fz.y, fz.z, fz.w}, au[4] = {fu.x, fu.y, fu.z, fu.w}, av[4] = {fv.x, fv.y, fv.z, fv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (b[k] != cb) {
                flush();
                cb = b[k];
#pragma unroll
                for (int q = 0; q < NS; ++q) acc[q] = 0.0;
            }
            const double z = (double)az[k], uu = (double)au[k], vv = (double)av[k];
            const double vr = uu * c1[k] + vv * s1[k], vt = vv * c1[k] - uu * s1[k];
            acc[0] += 1.0; acc[1] += rr[k]; acc[2] += z; acc[3] += vt; acc[4] += vr;
            acc[5] += z * z; acc[6] += vt * vt; acc[7] += vr * vr; acc[8] += vr * z;
            double cm = c1[k], sm = s1[k];
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                acc[AZIM_BASE_SUMS + 2 * m] += z * cm;
                acc[AZIM_BASE_SUMS + 2 * m + 1] += z * sm;
                const double cn = cm * c1[k] - sm * s1[k], sn = sm * c1[k] + cm * s1[k];
                cm = cn; sm = sn;
            }
        }
        flush();
    }
    __syncthreads();
    const int rows = min(g.W, g.nbins - base);
    for (int e = threadIdx.x; e < rows * NS; e += blockDim.x) {
        const int w = e / NS;
        if (win[w * NS] != 0.0) unsafeAtomicAdd(&part[(size_t)base * NS + e], win[e]);
    }
}

// one workgroup of 256: part[world][nbins][ns] summed in rank order -> table[nbins][12 + 2 nmodes] (include/fftbaro.h):
//   0 r_lo = b dr   1 r_hi = (b + 1) dr   2 n   3 <r>   4 <zeta>   5 <v_t>   6 <v_r>   7 <zeta^2>   8 <v_t^2>   9 <v_r^2>   10 <v_r zeta>
//   11 Gamma = dx dy sum_{b' <= b} sum zeta (from bin 0 upwards)   12 + 2 (m - 1), 13 + 2 (m - 1): <zeta c_m>, -<zeta s_m>
// A row with n = 0: zeros in 3-10 and from 12 on.  Dynamic LDS: sum zeta, then its running sum [nbins] (f64).
__global__ void __launch_bounds__(256) k_azim_table(const double *__restrict__ part, int world, int nbins, int nmodes, double dr, double dx, double dy,
                                                    double *__restrict__ table)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *sz = reinterpret_cast<double *>(smem_raw);
    const int ns = AZIM_BASE_SUMS + 2 * nmodes, nc = AZIM_BASE_COLS + 2 * nmodes;
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        double *row = table + (size_t)b * nc;
        double n = 0.0;
        for (int r = 0; r < world; ++r) n += part[((size_t)r * nbins + b) * ns];
        row[0] = (double)b * dr;
        row[1] = (double)(b + 1) * dr;
        row[2] = n;
        for (int k = 1; k < ns; ++k) {
            double s = 0.0;
            for (int r = 0; r < world; ++r) s += part[((size_t)r * nbins + b) * ns + k];
            if (k == 2) sz[b] = s;
            const double mean = n > 0.0 ? s / n : 0.0;
            if (k < AZIM_BASE_SUMS) row[2 + k] = mean;
            else row[AZIM_BASE_COLS + (k - AZIM_BASE_SUMS)] = ((k - AZIM_BASE_SUMS) & 1) && n > 0.0 ? -mean : mean;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int b = 0; b < nbins; ++b) { acc += sz[b]; sz[b] = acc; }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) table[(size_t)b * nc + 11] = (dx * dy) * sz[b];
}
