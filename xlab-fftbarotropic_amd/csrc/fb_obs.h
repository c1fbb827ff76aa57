// fb_obs.h -- kernels of the point observations (fb_model_scatter, fb_model_observe, fb_model_obs_misfit, fb_model_adjoint_add_obs and
// their fb_slab_* twins on one rank; host side: fb_beside_adjoint.h, obs_scatter, obs_observe, obs_adjoint_add).
//
// The observation operator H takes a field of the resident state (zeta, u, v or psi, formed as fb_model_get_vort / fb_model_get_diag
// form them: record(), fb_record.h) to n points by k_sample (fb_particles.h).  Its transpose spreads n point values back:
//   k_obs_wmax       max |w| over the points (one integer atomic max on the bits of a non-negative float64)
//   k_scatter        the transpose of k_sample: every point adds w wx[a] wy[b] to its sixteen stencil cells, indices and weights from
//                    pt_axis itself, into a FIXED-POINT accumulator of two 64-bit limbs per cell by integer atomics
//   k_scatter_round  every cell rounded to float32
//   (r2c of that field as beside_in takes a field: beside_r2c, fb_beside.h)
//   k_obs_adjoint    lam += conj(multiplier) r2c(scatter): the transpose of the record's spectral multiplier
// and the misfit of a 4D-Var cost:
//   k_obs_misfit, k_obs_cost_final   r = (h - y) / sigma^2 and J += 1/2 sum (h - y)^2 / sigma^2, float64, in a fixed order
//
// Why fixed point: a sum of floats by atomics depends on the order in which they land, and an optimiser's path must not.  Integer
// addition is associative, so the accumulator, and the rounding after it, are the same bits in any order of the atomics and for any
// permutation of the points.  The scale is a power of two 2^e chosen on the device: with wmax = max |w| < 2^x (frexp) and
// n <= 2^L (L = ceil(log2 n)), e = 62 - x - L, so that n wmax 2^e < 2^62; every |wx wy| is at most 1, so no cell can overflow.  A
// contribution c is split as c 2^e = floor(c 2^e) + fraction: the floor goes to the cell's high limb (a signed sum in two's
// complement), the fraction, rounded to OBS_FRAC = 39 bits, to its low limb (n 2^39 <= 2^63: no overflow either).  So a contribution
// is quantised to a multiple of 2^-(e+39): an absolute error of at most 2^-(e+40) <= n wmax 2^-101 each, far below the float32
// rounding of any cell whose contributions are not themselves 2^-50 of n wmax.
// No reference counterpart: the reference takes no observations.
#pragma once

// the head of the accumulator: the bits of wmax (k_obs_wmax), behind the two limbs of the nx * ny cells
FB_DEV int obs_exponent(const unsigned long long *__restrict__ head, int n)
{
    const double wmax = __longlong_as_double((long long)head[0]);
    int x = 0;
    (void)frexp(wmax, &x);                                  // wmax = f 2^x, f in [0.5, 1): wmax < 2^x (wmax == 0: x = 0)
    const int L = n > 1 ? 64 - __builtin_clzll((unsigned long long)(n - 1)) : 0;
    return 62 - x - L;
}

// max |w| over the finite weights into head[0]: the bits of a non-negative float64 order as unsigned integers do
__global__ void __launch_bounds__(256) k_obs_wmax(const double *__restrict__ w, int n, unsigned long long *__restrict__ head)
{
    __shared__ double sh[256];
    double v = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double a = __builtin_fabs(w[p]);
        if (__builtin_isfinite(a) && a > v) v = a;
    }
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && sh[threadIdx.x + s] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0] > 0.0) atomicMax(head, (unsigned long long)__double_as_longlong(sh[0]));
}

#define OBS_FRAC 39

// The transpose of k_sample: cell [ix[a]][jy[b]] += w_p wx[a] wy[b] 2^e, the floor into acc[cell], the fraction in units of 2^-OBS_FRAC
// into acc[cells + cell]; one thread per point (grid-stride).  A point whose position or weight is not finite deposits nothing
// (pt_axis returns false for such a position and k_sample reads nothing for it).  Every index pt_axis returns lies in [0, n) of its
// axis, so every cell lies in [0, cells), cells = nx * ny.
__global__ void __launch_bounds__(256) k_scatter(PartGeo g, const double *__restrict__ xy, const double *__restrict__ w, int n, unsigned long long *__restrict__ acc,
                                                 size_t cells, const unsigned long long *__restrict__ head)
{
#pragma clang fp contract(off)
    const int e = obs_exponent(head, n);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double qx = xy[2 * p], qy = xy[2 * p + 1], wp = w[p];
        int ix[4], jy[4];
        double wx[4], wy[4];
        const bool okx = pt_axis(qx, g.dx, g.nx, ix, wx), oky = pt_axis(qy, g.dy, g.ny, jy, wy);
        if (!(okx && oky) || !__builtin_isfinite(wp)) continue;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double x = ldexp(wp * (wx[a] * wy[b]), e);                         // |x| < 2^62 / n
                const double fl = __builtin_floor(x);
                const long long hi = (long long)fl;
                const unsigned long long lo = (unsigned long long)__double2ll_rn(ldexp(x - fl, OBS_FRAC));       // x - fl in [0, 1), exact
                const size_t cell = (size_t)ix[a] * g.ny + jy[b];
                if (hi != 0) atomicAdd(acc + cell, (unsigned long long)hi);              // (two's complement: a signed sum)
                if (lo != 0) atomicAdd(acc + cells + cell, lo);
            }
        }
    }
}

// every cell of the accumulator to float32: the low limb's carry into the high one in integers, then (high + fraction) 2^-e through
// float64 (two roundings of 2^-53) into the one float32 rounding
__global__ void __launch_bounds__(256) k_scatter_round(const unsigned long long *__restrict__ acc, const unsigned long long *__restrict__ head, int n,
                                                       float *__restrict__ field, size_t cells)
{
#pragma clang fp contract(off)
    const int e = obs_exponent(head, n);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long lo = acc[cells + i];
        const long long hi = (long long)acc[i] + (long long)(lo >> OBS_FRAC);
        const double fr = ldexp((double)(lo & ((1ull << OBS_FRAC) - 1)), -OBS_FRAC);
        field[i] = (float)ldexp((double)hi + fr, -e);
    }
}

// lam += conj(multiplier) s over one column group in the 3-pass layout (fb_tracer.h), s the r2c of a scattered field: the transpose of
// the spectral multiplier of the observed kind, in the float32 forms of k_psi_private (no contraction; the (0, 0) mode divided by 1):
//   0 zeta: s        3 psi: s / lap        1 u = -grady(psi): +grady(s / lap)        2 v = gradx(psi): -gradx(s / lap)
// (the conjugate of i k is -i k; lap is real).  Pad columns are left as they are: zero.
__global__ void __launch_bounds__(256) k_obs_adjoint(SpecCoef c, const cf *__restrict__ s, cf *__restrict__ lam, int kind, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / P), col = (int)(idx - (size_t)row * P);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d, j = ky0 + col;
        if (j >= c.hy) continue;
        cf a = s[idx];
        if (kind != 0) {
            const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);
            a = cf_make(a.x / li, a.y / li);
            if (kind == 1) { const float k = c.gy[j]; a = cf_make(-a.y * k, a.x * k); }
            if (kind == 2) { const float k = c.gx[i]; a = cf_make(a.y * k, -(a.x * k)); }
        }
        const cf l = lam[idx];
        lam[idx] = cf_make(l.x + a.x, l.y + a.y);
    }
}

// r[p] = (h[p] - y[p]) / sigma[p]^2 (sigma == NULL: 1) and this workgroup's share of sum (h - y)^2 / sigma^2 into part[blockIdx.x]:
// every thread sums its grid-stride points in ascending order, the workgroup by tangent_block_sum
__global__ void __launch_bounds__(256) k_obs_misfit(const double *__restrict__ h, const double *__restrict__ y, const double *__restrict__ sigma, int n,
                                                    double *__restrict__ r, double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double sh[256];
    double acc = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double d = h[p] - y[p], sg = sigma ? sigma[p] : 1.0;
        const double q = d / (sg * sg);
        r[p] = q;
        acc = acc + d * q;
    }
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// *cost += 1/2 sum of the partial sums, in a fixed order
__global__ void __launch_bounds__(256) k_obs_cost_final(const double *__restrict__ part, int nparts, double *__restrict__ cost)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) acc += part[k];
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) *cost = *cost + 0.5 * s;
}
