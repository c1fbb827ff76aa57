// fb_particles.h -- kernels of the Lagrangian particles (fb_model_set_particles, fb_model_sample; host side: fb_record.h, particle_stage).
//
// Particles are points (x, y) [m] on the doubly periodic domain, float64 and UNWRAPPED; grid point (i, j) of an [nx][ny] field lies
// at x = i dx, y = j dy.  Every RK4 step of the model advances them by the same scheme, coupled stage by stage:
//   k1 = U_0(X0), k2 = U_1(X0 + dt/2 k1), k3 = U_2(X0 + dt/2 k2), k4 = U_3(X0 + dt k3), X <- X0 + dt/6 (k1 + 2 k2 + 2 k3 + k4)
// with U_s the velocity (u, v) of the vorticity's state of stage s as two float32 [nx][ny] fields, formed as fb_model_get_diag
// forms u and v, and interpolated to the particle by the tensor product of 4-point cubic Lagrange polynomials in float64.  Per stage:
//   k_particle_uv_spec   grady(psi_c), gradx(psi_c) of the stage state into two fields of the record workspace (k_psi_private<1>, <2>)
//   (the backward x pass of the two fields and the ROW_INV row pass of each: fb_record.h, particle_stage)
//   k_particle_stage     interpolation and the RK stage update of every particle
// The state is SoA: six float64 arrays of n (base x, y; stage position x, y; accumulator x, y).
// No reference counterpart: the reference follows no particles.
#pragma once

struct PartGeo { double dx, dy; int nx, ny; };

// The four stencil indices and weights of one axis: s = x / d, i0 = floor(s) (64-bit), t = s - i0, rows (i0 - 1 .. i0 + 2) mod n as a
// non-negative modulus.  false: x is not finite or s lies beyond the 64-bit integers; no index is formed then and the caller reads
// nothing.  Every index returned lies in [0, n).
FB_DEV bool pt_axis(double x, double d, int n, int idx[4], double w[4])
{
#pragma clang fp contract(off)
    if (!__builtin_isfinite(x)) return false;
    const double s = x / d;
    if (!(__builtin_fabs(s) < 4.0e18)) return false;
    const double fl = __builtin_floor(s);
    const long long i0 = (long long)fl;
    const double t = s - fl;                               // (fl == (double)i0 exactly)
    long long r = i0 % (long long)n;
    if (r < 0) r += n;
    const int i = (int)r;
    idx[0] = i == 0 ? n - 1 : i - 1;
    idx[1] = i;
    idx[2] = i + 1 >= n ? i + 1 - n : i + 1;
    idx[3] = i + 2 >= n ? i + 2 - n : i + 2;
    w[0] = -t * (t - 1.0) * (t - 2.0) / 6.0;
    w[1] = (t + 1.0) * (t - 1.0) * (t - 2.0) / 2.0;
    w[2] = -(t + 1.0) * t * (t - 2.0) / 2.0;
    w[3] = (t + 1.0) * t * (t - 1.0) / 6.0;
    return true;
}

// sum_a wx[a] * (sum_b wy[b] * f[ix[a]][jy[b]]): a stencil row is four consecutive floats unless it wraps in y (no alignment assumed)
FB_DEV double pt_gather(const float *__restrict__ f, int ny, const int ix[4], const double wx[4], const int jy[4], const double wy[4])
{
#pragma clang fp contract(off)
    const bool run = jy[3] == jy[0] + 3;
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float *row = f + (size_t)ix[a] * ny;
        float q0, q1, q2, q3;
        if (run) { const float *p = row + jy[0]; q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3]; }
        else { q0 = row[jy[0]]; q1 = row[jy[1]]; q2 = row[jy[2]]; q3 = row[jy[3]]; }
        const double r = ((wy[0] * (double)q0 + wy[1] * (double)q1) + wy[2] * (double)q2) + wy[3] * (double)q3;
        acc = acc + wx[a] * r;
    }
    return acc;
}

// ---- the spectral fields of u and v ----
// za: vort_c0, zb: the stage state, both in the 3-pass layout (a mode outside the dealiasing circle is read from the base, as
// k_advect_deriv reads it; stage 0 and exported states: zb == za).  Field 0 of z: grady(psi_c), field 1 (fstride further):
// gradx(psi_c), psi_c = invertLaplacian(state), in the float32 forms of k_psi_private<1> and <2> (no contraction); pad columns zero.
// za, zb may be field 1 of z: each element is read before it is written, by the same thread.
__global__ void __launch_bounds__(256) k_particle_uv_spec(SpecCoef c, const cf *za, const cf *zb, cf *z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / P), col = (int)(idx - (size_t)row * P);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d, j = ky0 + col;
        cf gy = cf_make(0.f, 0.f), gx = gy;
        if (j < c.hy) {
            cf a = coef_mask(c, i, j) != 0.0f ? zb[idx] : za[idx];
            const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);           // fftwfop.cpp:42-43,112-117
            a = cf_make(a.x / li, a.y / li);
            const float ky = c.gy[j], kx = c.gx[i];
            gy = cf_make(-a.y * ky, a.x * ky);                                        // fftwfop.cpp:96-103
            gx = cf_make(-a.y * kx, a.x * kx);                                        // fftwfop.cpp:87-94
        }
        z[idx] = gy; z[idx + fstride] = gx;
    }
}

// ---- the particles ----
// float64 [n][2] (x, y) -> the base arrays bx, by
__global__ void __launch_bounds__(256) k_particle_unpack(const double *__restrict__ xy, double *__restrict__ bx, double *__restrict__ by, int n)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        bx[p] = xy[2 * p]; by[p] = xy[2 * p + 1];
    }
}
__global__ void __launch_bounds__(256) k_particle_pack(const double *__restrict__ bx, const double *__restrict__ by, double *__restrict__ xy, int n)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        xy[2 * p] = bx[p]; xy[2 * p + 1] = by[p];
    }
}

// One RK stage of every particle, one thread per particle (grid-stride).  pt: the six arrays of n (bx, by, sx, sy, ax, ay).  Stage 0
// reads the base, the later stages the stage position; stages 0..2 write the accumulator k1 + 2 k2 + 2 k3 and the next stage
// position, stage 3 the new base.  A particle whose position is not finite reads nothing and becomes (stays) NaN.
template <int STAGE>
__global__ void __launch_bounds__(256) k_particle_stage(PartGeo g, const float *__restrict__ u, const float *__restrict__ v, double *__restrict__ pt, int n, double dt)
{
#pragma clang fp contract(off)
    double *bx = pt, *by = pt + (size_t)n, *sx = pt + 2 * (size_t)n, *sy = pt + 3 * (size_t)n, *ax = pt + 4 * (size_t)n, *ay = pt + 5 * (size_t)n;
    const double h = STAGE == 2 ? dt : dt / 2.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double x0 = bx[p], y0 = by[p];
        const double x = STAGE == 0 ? x0 : sx[p], y = STAGE == 0 ? y0 : sy[p];
        int ix[4], jy[4];
        double wx[4], wy[4];
        double ku = __builtin_nan(""), kv = ku;
        const bool okx = pt_axis(x, g.dx, g.nx, ix, wx), oky = pt_axis(y, g.dy, g.ny, jy, wy);
        if (okx && oky) { ku = pt_gather(u, g.ny, ix, wx, jy, wy); kv = pt_gather(v, g.ny, ix, wx, jy, wy); }
        if (STAGE == 0) { ax[p] = ku; ay[p] = kv; sx[p] = x0 + h * ku; sy[p] = y0 + h * kv; }
        else if (STAGE < 3) { ax[p] = ax[p] + 2.0 * ku; ay[p] = ay[p] + 2.0 * kv; sx[p] = x0 + h * ku; sy[p] = y0 + h * kv; }
        else { bx[p] = x0 + (dt / 6.0) * (ax[p] + ku); by[p] = y0 + (dt / 6.0) * (ay[p] + kv); }
    }
}

// fb_model_sample: out[p] = the interpolated value of `f` at xy[p] (float64 [n][2]); NaN where a position is not finite
__global__ void __launch_bounds__(256) k_sample(PartGeo g, const float *__restrict__ f, const double *__restrict__ xy, int n, double *__restrict__ out)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double qx = xy[2 * p], qy = xy[2 * p + 1];                              // (8-byte alignment is all the caller owes)
        int ix[4], jy[4];
        double wx[4], wy[4];
        double r = __builtin_nan("");
        const bool okx = pt_axis(qx, g.dx, g.nx, ix, wx), oky = pt_axis(qy, g.dy, g.ny, jy, wy);
        if (okx && oky) r = pt_gather(f, g.ny, ix, wx, jy, wy);
        out[p] = r;
    }
}
