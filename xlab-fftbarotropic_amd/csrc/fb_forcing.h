// fb_forcing.h -- kernels of the split stage that follows every RK4 step once forcing is set (fb_model_set_forcing; host side:
// fb_beside_forcing.h, forcing_stage): stochastic forcing in a wavenumber ring, linear drag and hyperviscosity,
//   zeta_new = fl32(D zeta) + Delta_n       for every stored mode inside the dealiasing circle (a masked mode keeps its bits),
//   D        = fl32( exp(-(mu + nu_p K^2p) dt) ),  K^2 = -laplacian_coe (the float32 table value, promoted), evaluated in float64,
//   Delta_n  = fl32( GRIDS sqrt(2 eps dt K^2 / N_ring) e^{i theta} ) on the ring | sqrt(K^2) - k_f | <= dk (float64), 0 elsewhere,
//   theta    = 2 pi u / 2^32,  u = word 0 of Philox4x32-10 with counter (i, j, n_lo, n_hi) and key (seed_lo, seed_hi),
// n the forcing clock: the split stages applied since the forcing was set, a 64-bit count in device memory that k_forcing_final
// advances, so that a captured step replays with the clock of its own time.  On the lines j = 0 and j = ny/2 a mode with i > nx/2
// takes the conjugate of mode (nx - i, j): the field stays real.  The four self-conjugate modes are never forced.  The noise is a
// function of (i, j, n, seed) alone: it does not depend on the layout, the kernel path or the launch geometry.
//   k_forcing_stage<true>    the stage on the vorticity in the 3-pass layout, with the budget's partial sums per workgroup
//   k_forcing_final          the partial sums in a fixed order into the running totals; the clock advanced
//   k_forcing_stage<false>   the base of a perturbation of the tangent set times D (the forcing is additive: no increment)
//   k_forcing_increment      Delta_n alone in the public [nx][ny/2+1] layout (fb_model_forcing_increment), from the same device function
// Philox4x32-10: Salmon, Moraes, Dror, Shaw (2011), "Parallel random numbers: as easy as 1, 2, 3".
// No reference counterpart: the reference has no forcing but a fixed real-space source, and no dissipation but nu laplacian.
#pragma once

struct ForcingArgs {
    double mu, nu_p, dt;        // D = fl32(exp(-(mu + nu_p K^2p) dt))
    double kf, dk;              // the ring [rad/m]
    double lo2, hi2;            // K^2 outside [lo2, hi2] is off the ring whatever the rounding of the square root: the cheap test first
    double a2;                  // 2 eps dt / N_ring
    double grids;               // nx ny: the stored spectrum is unnormalised
    unsigned seed_lo, seed_hi;
    int p;                      // hyperviscosity's order, 1..8
    int ny2;                    // ny / 2
    int forced, decays;         // eps > 0; mu > 0 or nu_p > 0
};

// word 0 of Philox4x32-10 of the counter (c0, c1, c2, c3) under the key (k0, k1)
FB_DEV unsigned philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

FB_DEV float forcing_decay(const ForcingArgs &f, double K2)
{
    double kp = K2;
    for (int q = 1; q < f.p; ++q) kp *= K2;
    return (float)exp(-(f.mu + f.nu_p * kp) * f.dt);
}

FB_DEV bool forcing_on_ring(const ForcingArgs &f, int nx, int i, int j, double K2)
{
    if (K2 < f.lo2 || K2 > f.hi2) return false;
    if ((i == 0 || 2 * i == nx) && (j == 0 || j == f.ny2)) return false;       // self-conjugate
    return fabs(sqrt(K2) - f.kf) <= f.dk;
}

// Delta_n of a ring mode.  theta / pi = u / 2^31 is exact in float64, and sincospi reduces it exactly
FB_DEV cf forcing_delta(const ForcingArgs &f, int nx, int i, int j, double K2, unsigned long long n)
{
#pragma clang fp contract(off)
    const bool mirror = (j == 0 || j == f.ny2) && 2 * i > nx;
    const unsigned u = philox4x32_10((unsigned)(mirror ? nx - i : i), (unsigned)j, (unsigned)n, (unsigned)(n >> 32), f.seed_lo, f.seed_hi);
    double s, co;
    sincospi((double)u * 0x1p-31, &s, &co);
    const double amp = f.grids * sqrt(f.a2 * K2);
    const double re = amp * co, im = amp * s;
    return cf_make((float)re, (float)(mirror ? -im : im));
}

// The stage in place on one half spectrum in the 3-pass layout (row N2*c + d holds kx = c + N1*d, column j holds ky = j, pitch P; one
// rank, so one column group).  STATE: the vorticity -- decay, increment with the clock read from *clock, and four float64 partial sums
// per workgroup into part[4 blockIdx.x ..]: with z' = fl32(D z) and Hermitian weights w (1 in the columns j = 0 and ny/2, else 2), the
// sums over the modes of w (|z_new|^2 - |z'|^2) / (2 K^2), w (|z'|^2 - |z|^2) / (2 K^2) (the K = 0 mode left out), w (|z_new|^2 - |z'|^2)
// and w (|z'|^2 - |z|^2); each square is exact in float64.  No atomics: the same grid gives the same bits.  !STATE: decay alone.
// Two modes (16 bytes) per lane and access; the float64 exponential only where something decays, the trigonometry only on the ring.
template <bool STATE>
__global__ void __launch_bounds__(256) k_forcing_stage(SpecCoef c, ForcingArgs f, cf *z, int P, int N1, int N2, const unsigned long long *__restrict__ clock,
                                                       double *__restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double sh[STATE ? 4 * 256 : 1];
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    const unsigned long long n = STATE ? *clock : 0ull;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float4 *q4 = reinterpret_cast<float4 *>(z);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        if (col >= c.hy) continue;
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const float4 v = q4[p];
        float o[4] = {v.x, v.y, v.z, v.w};
        bool changed = false;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = col + e;
            if (coef_mask(c, i, j) == 0.0f) continue;                   // (j >= hy is masked too)
            const double K2 = -(double)coef_lap(c, i, j);
            const float D = f.decays ? forcing_decay(f, K2) : 1.0f;
            const bool ring = STATE && f.forced && forcing_on_ring(f, c.nx, i, j, K2);
            if (D == 1.0f && !ring) continue;
            const float zx = o[2 * e], zy = o[2 * e + 1];
            const float dx = zx * D, dy = zy * D;
            float ux = dx, uy = dy;
            if (ring) { const cf dl = forcing_delta(f, c.nx, i, j, K2, n); ux = dx + dl.x; uy = dy + dl.y; }
            o[2 * e] = ux; o[2 * e + 1] = uy;
            changed = true;
            if (STATE) {
                const double a0 = (double)zx * zx + (double)zy * zy, a1 = (double)dx * dx + (double)dy * dy, a2 = (double)ux * ux + (double)uy * uy;
                const double w = (j == 0 || j == f.ny2) ? 1.0 : 2.0, we = K2 > 0.0 ? w / (2.0 * K2) : 0.0;
                acc[0] += we * (a2 - a1); acc[1] += we * (a1 - a0); acc[2] += w * (a2 - a1); acc[3] += w * (a1 - a0);
            }
        }
        if (changed) q4[p] = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (STATE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[k * 256 + threadIdx.x] = acc[k];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
#pragma unroll
                for (int k = 0; k < 4; ++k) sh[k * 256 + threadIdx.x] += sh[k * 256 + threadIdx.x + w];
            }
            __syncthreads();
        }
        if (threadIdx.x < 4) part[4 * (size_t)blockIdx.x + threadIdx.x] = sh[threadIdx.x * 256];
    }
}

// the partial sums in a fixed order into the running totals tot[0..3] = dE_forc, dE_diss, dZ_forc, dZ_diss (scale = 1 / GRIDS^2; the
// enstrophy's 1/2 here), and the clock advanced: one workgroup of 256, wave k sums column k
__global__ void __launch_bounds__(256) k_forcing_final(const double *__restrict__ part, int nparts, double scale, double *__restrict__ tot,
                                                       unsigned long long *__restrict__ clock)
{
    __shared__ double sh[256];
    const int k = threadIdx.x >> 6, l = threadIdx.x & 63;
    double acc = 0.0;
    for (int b = l; b < nparts; b += 64) acc += part[4 * (size_t)b + k];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (l < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (l == 0) tot[k] += sh[threadIdx.x] * scale * (k < 2 ? 1.0 : 0.5);
    if (threadIdx.x == 0) *clock += 1ull;
}

// Delta_n in the public layout [nx][hy], zeros off the ring
__global__ void __launch_bounds__(256) k_forcing_increment(SpecCoef c, ForcingArgs f, unsigned long long n, cf *__restrict__ out, size_t total)
{
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / c.hy), j = (int)(idx - (size_t)i * c.hy);
        const double K2 = -(double)coef_lap(c, i, j);
        out[idx] = f.forced && forcing_on_ring(f, c.nx, i, j, K2) ? forcing_delta(f, c.nx, i, j, K2, n) : cf_make(0.f, 0.f);
    }
}
