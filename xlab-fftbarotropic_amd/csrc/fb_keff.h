// fb_keff.h -- the effective eddy diffusivity record path (fb_model_get_eddy_diffusivity, fb_slab_get_eddy_diffusivity):
// vorticity as the tracer (Nakamura 1996, Hendricks and Schubert 2009), its contour areas binned on the GPU.
//   k_keff_spec          zeta, gradx zeta, grady zeta spectra from the exported state (the backward x pass and the ROW_KEFF row
//                        pass follow: zeta and g = |grad zeta|^2 in physical space)
//   k_keff_minmax(_final) min / max of zeta: per-workgroup partials, then one workgroup in a fixed order
//   k_keff_hist          per-workgroup histogram in LDS (u32 count, f64 sum of g per bin), stored plainly
//   k_keff_reduce        the partials of the workgroups summed per bin in a fixed order (one rank's histogram)
//   k_keff_table         the ranks' histograms summed in rank order, the table [nbins][9]
// No reference counterpart: its README names the effective eddy diffusivity as an output; the reference never computes it.
#pragma once

enum { KEFF_COLS = 9 };

// record path of the eddy diffusivity: from one column group's state (3-pass private layout in `zin`, local column j holds
// ky = ky0 + j, as k_ow_spec) into the fields 0, 1, 2 of `z`, fstride apart: zeta, gradx(zeta), grady(zeta); pad columns zero.
// Every column takes part, the frozen ones too.  zin may be field 0 of z: each element is read before it is written, by the same
// thread.  Same float32 forms as k_spec_op (no contraction).
__global__ void __launch_bounds__(256) k_keff_spec(SpecCoef c, const cf *zin, cf *z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / P), col = (int)(idx - (size_t)row * P);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d, j = ky0 + col;
        cf a = cf_make(0.f, 0.f), ax = a, ay = a;
        if (j < c.hy) {
            a = zin[idx];
            const float kx = c.gx[i], ky = c.gy[j];
            ax = cf_make(-a.y * kx, a.x * kx);                                  // fftwfop.cpp:87-94
            ay = cf_make(-a.y * ky, a.x * ky);                                  // fftwfop.cpp:96-103
        }
        z[idx] = a; z[idx + fstride] = ax; z[idx + 2 * fstride] = ay;
    }
}

FB_DEV float keff_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
FB_DEV float keff_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// per-workgroup (min, max) of q[0, n) (n a multiple of 4, q 16-byte aligned when V4) into part[2 * blockIdx.x + 0/1]
template <bool V4>
__global__ void __launch_bounds__(256) k_keff_minmax(const float *__restrict__ q, size_t n, float *__restrict__ part)
{
    __shared__ float sm[2][4];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (V4) {
        const float4 *q4 = reinterpret_cast<const float4 *>(q);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            const float4 v = q4[i];
            lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
            hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { lo = fminf(lo, q[i]); hi = fmaxf(hi, q[i]); }
    }
    lo = keff_wave_min(lo); hi = keff_wave_max(hi);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = lo; sm[1][w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = fminf(fminf(sm[0][0], sm[0][1]), fminf(sm[0][2], sm[0][3]));
        part[2 * blockIdx.x + 1] = fmaxf(fmaxf(sm[1][0], sm[1][1]), fmaxf(sm[1][2], sm[1][3]));
    }
}

// one workgroup of 256: the nparts partials in a fixed order -> this rank's (min, max), written `copies` times, 2 floats apart
// (multi-GPU: the send buffer of the all-gather, one copy per peer)
__global__ void __launch_bounds__(256) k_keff_minmax_final(const float *__restrict__ part, int nparts, float *__restrict__ out, int copies)
{
    __shared__ float sm[2][4];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) { lo = fminf(lo, part[2 * i]); hi = fmaxf(hi, part[2 * i + 1]); }
    lo = keff_wave_min(lo); hi = keff_wave_max(hi);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[0][w] = lo; sm[1][w] = hi; }
    __syncthreads();
    lo = fminf(fminf(sm[0][0], sm[0][1]), fminf(sm[0][2], sm[0][3]));
    hi = fmaxf(fmaxf(sm[1][0], sm[1][1]), fmaxf(sm[1][2], sm[1][3]));
    for (int r = threadIdx.x; r < copies; r += blockDim.x) { out[2 * r] = lo; out[2 * r + 1] = hi; }
}

// the global (qmin, qmax) from the ranks' pairs mm[world][2], in rank order
FB_DEV void keff_range(const float *mm, int world, float &qmin, float &qmax)
{
    qmin = mm[0]; qmax = mm[1];
    for (int r = 1; r < world; ++r) { qmin = fminf(qmin, mm[2 * r]); qmax = fmaxf(qmax, mm[2 * r + 1]); }
}
// nbins / (qmax - qmin) in double (correctly rounded), 0 when qmax == qmin (every point in bin 0)
FB_DEV double keff_inv_width(float qmin, float qmax, int nbins)
{
    return qmax > qmin ? (double)nbins / ((double)qmax - (double)qmin) : 0.0;
}
// bin of one point: floor((q - qmin) * inv) clamped to [0, nbins - 1]; a NaN lands in bin 0, +-inf at either end
FB_DEV int keff_bin(float q, float qmin, double inv, int nbins)
{
#pragma clang fp contract(off)
    const double t = ((double)q - (double)qmin) * inv;
    return t >= (double)(nbins - 1) ? nbins - 1 : (t >= 1.0 ? (int)t : 0);
}

// Per-workgroup histogram of (q, g) over nbins bins, in LDS: f64 sum of g [nbins] then u32 count [nbins] (12 B per bin, dynamic LDS).
// Contention: most points of a vortex field fall in one or two background bins, where per-point LDS atomics of a wave would
// serialise 64 ways on one address.  Each lane instead keeps a run (bin, count, sum) in registers and adds it to LDS only when
// its bin changes (and once at the end): along a smooth field a lane's bin rarely changes.  Partials are stored plainly:
// cnt_part[blockIdx.x][nbins], sum_part[blockIdx.x][nbins].  The f64 sums inside a workgroup are added in whatever order the
// atomics land (the counts are exact).
template <bool V4>
__global__ void __launch_bounds__(256) k_keff_hist(const float *__restrict__ q, const float *__restrict__ g, size_t n, const float *__restrict__ mm,
                                                   int world, int nbins, unsigned *__restrict__ cnt_part, double *__restrict__ sum_part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *ssum = reinterpret_cast<double *>(smem_raw);
    unsigned *scnt = reinterpret_cast<unsigned *>(ssum + nbins);
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) { ssum[b] = 0.0; scnt[b] = 0u; }
    float qmin, qmax;
    keff_range(mm, world, qmin, qmax);
    const double inv = keff_inv_width(qmin, qmax, nbins);
    __syncthreads();
    int cb = 0;
    unsigned cn = 0;
    double cs = 0.0;
    auto flush = [&]() {
        if (cn) {
            __hip_atomic_fetch_add(&scnt[cb], cn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&ssum[cb], cs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    auto put = [&](float qv, float gv) {
        const int b = keff_bin(qv, qmin, inv, nbins);
        if (b != cb) { flush(); cb = b; cn = 0; cs = 0.0; }
        ++cn; cs += (double)gv;
    };
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (V4) {
        const float4 *q4 = reinterpret_cast<const float4 *>(q), *g4 = reinterpret_cast<const float4 *>(g);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += stride) {
            const float4 a = q4[i], s = g4[i];
            put(a.x, s.x); put(a.y, s.y); put(a.z, s.z); put(a.w, s.w);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) put(q[i], g[i]);
    }
    flush();
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        cnt_part[(size_t)blockIdx.x * nbins + b] = scnt[b];
        sum_part[(size_t)blockIdx.x * nbins + b] = ssum[b];
    }
}

// The nparts workgroup partials summed per bin -> this rank's histogram out[bin][2] = (count, sum g), written `copies` times, stride
// apart (multi-GPU: the send buffer of the all-gather, one copy per peer).  A workgroup takes KEFF_RB bins, KEFF_RS slices per bin:
// slice s sums the partials s, s + KEFF_RS, ... in order, then slice 0 adds the slices in order (a fixed order: repeatable bit for bit).
// (One thread per bin walking all partials was latency-bound: 0.14 ms for 512 partials at 256 bins.)
enum { KEFF_RB = 16, KEFF_RS = 16 };
__global__ void __launch_bounds__(256) k_keff_reduce(const unsigned *__restrict__ cnt_part, const double *__restrict__ sum_part, int nparts,
                                                     int nbins, double *__restrict__ out, int copies, size_t stride)
{
    __shared__ unsigned long long sn[KEFF_RS][KEFF_RB];
    __shared__ double ss[KEFF_RS][KEFF_RB];
    const int lb = threadIdx.x % KEFF_RB, sl = threadIdx.x / KEFF_RB, b = blockIdx.x * KEFF_RB + lb;
    unsigned long long n = 0;
    double s = 0.0;
    if (b < nbins) {
#pragma unroll 8
        for (int p = sl; p < nparts; p += KEFF_RS) { n += cnt_part[(size_t)p * nbins + b]; s += sum_part[(size_t)p * nbins + b]; }
    }
    sn[sl][lb] = n; ss[sl][lb] = s;
    __syncthreads();
    if (sl != 0 || b >= nbins) return;
    for (int k = 1; k < KEFF_RS; ++k) { n += sn[k][lb]; s += ss[k][lb]; }
    for (int r = 0; r < copies; ++r) { out[r * stride + 2 * b] = (double)n; out[r * stride + 2 * b + 1] = s; }
}

// one workgroup of 256: hist[world][nbins][2] (count, sum g) summed in rank order, mm[world][2] the ranks' (min, max) -> table[nbins][9]:
//   0 Q_lo = qmin + b dQ   1 Q_hi = qmin + (b + 1) dQ   2 n_b   3 A_b = n_b dx dy   4 A_ge = sum_{b' >= b} A_b' (top bin down)
//   5 S_b = dx dy sum g    6 Le^2 = S_b A_b / dQ^2      7 r_e = sqrt((A_ge - A_b / 2) / pi)   8 K_eff = nu Le^2 / (4 pi^2 r_e^2)
// with dQ = (qmax - qmin) / nbins; Le^2 = 0 where n_b = 0 or dQ is not a positive finite number, K_eff = 0 where Le^2 = 0 or r_e = 0.
// Dynamic LDS: A_b [nbins], A_ge [nbins] (f64).  No contraction: columns 0-4 are reproduced bit for bit by numpy.
__global__ void __launch_bounds__(256) k_keff_table(const double *__restrict__ hist, int world, const float *__restrict__ mm, int nbins,
                                                    double dx, double dy, double nu, double *__restrict__ table)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double *sa = reinterpret_cast<double *>(smem_raw), *sge = sa + nbins;
    float qmin, qmax;
    keff_range(mm, world, qmin, qmax);
    const double dq = ((double)qmax - (double)qmin) / (double)nbins;
    const bool dq_ok = dq > 0.0 && dq < __builtin_inf();
    const double pi = 3.141592653589793;
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        double n = 0.0, s = 0.0;
        for (int r = 0; r < world; ++r) { n += hist[((size_t)r * nbins + b) * 2]; s += hist[((size_t)r * nbins + b) * 2 + 1]; }
        const double a = n * dx * dy;
        double *row = table + (size_t)b * KEFF_COLS;
        row[0] = (double)qmin + (double)b * dq;
        row[1] = (double)qmin + (double)(b + 1) * dq;
        row[2] = n;
        row[3] = a;
        row[5] = dx * dy * s;
        sa[b] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // the suffix sum, top bin down, in eights (loads ahead of the chain)
        double acc = 0.0;
        int b = nbins - 1;
        for (; b >= 7; b -= 8) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = sa[b - k];
#pragma unroll
            for (int k = 0; k < 8; ++k) { acc += v[k]; sge[b - k] = acc; }
        }
        for (; b >= 0; --b) { acc += sa[b]; sge[b] = acc; }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) {
        double *row = table + (size_t)b * KEFF_COLS;
        const double a = sa[b], age = sge[b], n = row[2], s = row[5];
        const double le2 = (n > 0.0 && dq_ok) ? s * a / (dq * dq) : 0.0;
        const double re = sqrt((age - a / 2.0) / pi);
        row[4] = age;
        row[6] = le2;
        row[7] = re;
        row[8] = (le2 > 0.0 && re > 0.0) ? nu * le2 / (4.0 * pi * pi * re * re) : 0.0;
    }
}
