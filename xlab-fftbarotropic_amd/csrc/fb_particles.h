// fb_particles.h -- kernels of the Lagrangian particles (fb_model_set_particles, fb_model_sample; host side: fb_beside_particles.h, particle_stage).
//
// Particles are points (x, y) [m] on the doubly periodic domain, float64 and UNWRAPPED; grid point (i, j) of an [nx][ny] field lies
// at x = i dx, y = j dy.  Every RK4 step of the model advances them by the same scheme, coupled stage by stage:
//   k1 = U_0(X0), k2 = U_1(X0 + dt/2 k1), k3 = U_2(X0 + dt/2 k2), k4 = U_3(X0 + dt k3), X <- X0 + dt/6 (k1 + 2 k2 + 2 k3 + k4)
// with U_s the velocity (u, v) of the vorticity's state of stage s as two float32 [nx][ny] fields, formed as fb_model_get_diag
// forms u and v, and interpolated to the particle by the tensor product of 4-point cubic Lagrange polynomials in float64.  Per stage:
//   k_particle_uv_spec   grady(psi_c), gradx(psi_c) of the stage state into two fields of the record workspace (k_psi_private<1>, <2>)
//   (the backward x pass of the two fields and the ROW_INV row pass of each: fb_record.h, particle_stage)
//   k_particle_stage     interpolation and the RK stage update of every particle
//   k_particle_stage_def  the same with the deformation gradient F carried along (fb_model_set_particle_deformation), in its place
// The state is SoA: six float64 arrays of n (base x, y; stage position x, y; accumulator x, y).
// No reference counterpart: the reference follows no particles.
#pragma once

struct PartGeo { double dx, dy; int nx, ny; };

// The four stencil indices and weights of one axis: s = x / d, i0 = floor(s) (64-bit), t = s - i0, rows (i0 - 1 .. i0 + 2) mod n as a
// non-negative modulus.  false: x is not finite or s lies beyond the 64-bit integers; no index is formed then and the caller reads
// nothing.  Every index returned lies in [0, n).  dw (optional): the weights' derivatives with respect to t; over d they are those
// with respect to x, of the cell [i0, i0 + 1) that t lies in (at t == 0 the cell to the right).
FB_DEV bool pt_axis(double x, double d, int n, int idx[4], double w[4], double *dw = nullptr)
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
    if (dw) {
        const double t3 = 3.0 * t * t;
        dw[0] = -((t3 - 6.0 * t) + 2.0) / 6.0;
        dw[1] = ((t3 - 4.0 * t) - 1.0) / 2.0;
        dw[2] = -((t3 - 2.0 * t) - 2.0) / 2.0;
        dw[3] = (t3 - 1.0) / 6.0;
    }
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

// pt_gather's value (the same expressions in the same order: bit for bit) with both partial derivatives of the interpolant itself, from
// the same sixteen loads: *fx = sum_a dwx[a] r_a / dx, *fy = sum_a wx[a] (sum_b dwy[b] f[ix[a]][jy[b]]) / dy
FB_DEV double pt_gather_grad(const float *__restrict__ f, int ny, const int ix[4], const double wx[4], const double dwx[4], const int jy[4], const double wy[4],
                             const double dwy[4], double dx, double dy, double *fx, double *fy)
{
#pragma clang fp contract(off)
    const bool run = jy[3] == jy[0] + 3;
    double acc = 0.0, gx = 0.0, gy = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float *row = f + (size_t)ix[a] * ny;
        float q0, q1, q2, q3;
        if (run) { const float *p = row + jy[0]; q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3]; }
        else { q0 = row[jy[0]]; q1 = row[jy[1]]; q2 = row[jy[2]]; q3 = row[jy[3]]; }
        const double r = ((wy[0] * (double)q0 + wy[1] * (double)q1) + wy[2] * (double)q2) + wy[3] * (double)q3;
        const double ry = ((dwy[0] * (double)q0 + dwy[1] * (double)q1) + dwy[2] * (double)q2) + dwy[3] * (double)q3;
        acc = acc + wx[a] * r;
        gx = gx + dwx[a] * r;
        gy = gy + wx[a] * ry;
    }
    *fx = gx / dx; *fy = gy / dy;
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

// ---- the deformation gradient along the particles (fb_model_set_particle_deformation) ----
// Every particle carries F = dX(t) / dX(t0), float64 (F11, F12, F21, F22), advanced by the linearisation of the particle's own RK4 step:
//   K1 = A_0(X0) F0, K2 = A_1(X0 + dt/2 k1) (F0 + dt/2 K1), K3 = A_2(X0 + dt/2 k2) (F0 + dt/2 K2), K4 = A_3(X0 + dt k3) (F0 + dt K3),
//   F <- F0 + dt/6 (((K1 + 2 K2) + 2 K3) + K4)
// with A_s(X) = [[du/dx, du/dy], [dv/dx, dv/dy]] the gradient of the INTERPOLANT of the stage's u, v at X (pt_gather_grad): F is the
// exact Jacobian of the discrete map X0 -> X wherever that map is differentiable (the interpolant's derivative jumps at cell faces; on
// a face the cell to the right is taken).  det F is close to 1, not equal: the interpolated velocity is not exactly non-divergent.
// The state is SoA beside pt: twelve float64 arrays of n (base, stage value, accumulator of F11, F12, F21, F22 each).

// F = I into the four base arrays
__global__ void __launch_bounds__(256) k_particle_def_init(double *__restrict__ pd, int n)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        pd[p] = 1.0; pd[(size_t)n + p] = 0.0; pd[2 * (size_t)n + p] = 0.0; pd[3 * (size_t)n + p] = 1.0;
    }
}
// the four base arrays -> float64 [n][4] (F11, F12, F21, F22)
__global__ void __launch_bounds__(256) k_particle_def_pack(const double *__restrict__ pd, double *__restrict__ out, int n)
{
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[4 * p + e] = pd[e * (size_t)n + p];
    }
}

// k_particle_stage with F carried along in the same pass: the position arithmetic is k_particle_stage's, expression for expression
// (positions bit for bit), u, v and the four entries of A come from the same thirty-two loads.  pd: the twelve arrays of n
// (base 0..3, stage value 4..7, accumulator 8..11).  A particle whose position is not finite gets NaN in F.
template <int STAGE>
__global__ void __launch_bounds__(256) k_particle_stage_def(PartGeo g, const float *__restrict__ u, const float *__restrict__ v, double *__restrict__ pt,
                                                            double *__restrict__ pd, int n, double dt)
{
#pragma clang fp contract(off)
    const size_t N = (size_t)n;
    double *bx = pt, *by = pt + N, *sx = pt + 2 * N, *sy = pt + 3 * N, *ax = pt + 4 * N, *ay = pt + 5 * N;
    const double h = STAGE == 2 ? dt : dt / 2.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
        const double x0 = bx[p], y0 = by[p];
        const double x = STAGE == 0 ? x0 : sx[p], y = STAGE == 0 ? y0 : sy[p];
        int ix[4], jy[4];
        double wx[4], wy[4], dwx[4], dwy[4];
        double ku = __builtin_nan(""), kv = ku, a11 = ku, a12 = ku, a21 = ku, a22 = ku;
        const bool okx = pt_axis(x, g.dx, g.nx, ix, wx, dwx), oky = pt_axis(y, g.dy, g.ny, jy, wy, dwy);
        if (okx && oky) {
            ku = pt_gather_grad(u, g.ny, ix, wx, dwx, jy, wy, dwy, g.dx, g.dy, &a11, &a12);
            kv = pt_gather_grad(v, g.ny, ix, wx, dwx, jy, wy, dwy, g.dx, g.dy, &a21, &a22);
        }
        if (STAGE == 0) { ax[p] = ku; ay[p] = kv; sx[p] = x0 + h * ku; sy[p] = y0 + h * kv; }
        else if (STAGE < 3) { ax[p] = ax[p] + 2.0 * ku; ay[p] = ay[p] + 2.0 * kv; sx[p] = x0 + h * ku; sy[p] = y0 + h * kv; }
        else { bx[p] = x0 + (dt / 6.0) * (ax[p] + ku); by[p] = y0 + (dt / 6.0) * (ay[p] + kv); }
        double f0[4], fs[4], k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { f0[e] = pd[e * N + p]; fs[e] = STAGE == 0 ? f0[e] : pd[(4 + e) * N + p]; }
        k[0] = a11 * fs[0] + a12 * fs[2]; k[1] = a11 * fs[1] + a12 * fs[3];
        k[2] = a21 * fs[0] + a22 * fs[2]; k[3] = a21 * fs[1] + a22 * fs[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double *acc = pd + (8 + e) * N;
            if (STAGE == 0) { acc[p] = k[e]; pd[(4 + e) * N + p] = f0[e] + h * k[e]; }
            else if (STAGE < 3) { acc[p] = acc[p] + 2.0 * k[e]; pd[(4 + e) * N + p] = f0[e] + h * k[e]; }
            else pd[e * N + p] = f0[e] + (dt / 6.0) * (acc[p] + k[e]);
        }
    }
}

// fb_model_particle_stretching: the closed-form singular value decomposition of every 2 x 2 matrix of F, float64 [n][4] (F11, F12,
// F21, F22), into out [n][4] = ln sigma1, ln sigma2, theta_in, theta_out with
//   F = Rot(theta_out) diag(sigma1, sign(det F) sigma2) Rot(theta_in)^T up to the overall sign (both angles name an axis, folded into
//   (-pi/2, pi/2]): theta_in the direction of strongest stretching at the initial time, theta_out its image.
// F is divided by its largest |entry| s first (no overflow or underflow in the products); sigma2 = |det| / sigma1, not Q - R, which
// cancels under strong stretching.  s == 0: -inf, -inf, 0, 0; a singular F: ln sigma2 = -inf; an entry that is not finite: four NaN.
// Entry e of particle p is read from F[e * se + p * sp]: se = 1, sp = 4 for [n][4], se = n, sp = 1 for the model's own four base arrays.
__global__ void __launch_bounds__(256) k_particle_stretching(const double *__restrict__ F, size_t se, size_t sp, int n, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const double PI = 3.14159265358979323846, NINF = -__builtin_inf();
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        double a = F[p * sp], b = F[se + p * sp], c = F[2 * se + p * sp], d = F[3 * se + p * sp];
        double l1, l2, ti, to;
        const double s = fmax(fmax(fabs(a), fabs(b)), fmax(fabs(c), fabs(d)));
        if (!(__builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c) && __builtin_isfinite(d))) l1 = l2 = ti = to = __builtin_nan("");
        else if (s == 0.0) { l1 = l2 = NINF; ti = to = 0.0; }
        else {
            a = a / s; b = b / s; c = c / s; d = d / s;
            const double E = (a + d) / 2.0, Fm = (a - d) / 2.0, G = (c + b) / 2.0, H = (c - b) / 2.0;
            const double Q = hypot(E, H), R = hypot(Fm, G);
            const double s1 = Q + R, s2 = fabs(a * d - b * c) / s1, ls = log(s);
            const double a1 = atan2(G, Fm), a2 = atan2(H, E);
            l1 = log(s1) + ls;
            l2 = s2 > 0.0 ? log(s2) + ls : NINF;
            ti = (a1 - a2) / 2.0; to = (a2 + a1) / 2.0;
            if (ti > PI / 2.0) ti -= PI; else if (ti <= -PI / 2.0) ti += PI;
            if (to > PI / 2.0) to -= PI; else if (to <= -PI / 2.0) to += PI;
        }
        out[4 * p] = l1; out[4 * p + 1] = l2; out[4 * p + 2] = ti; out[4 * p + 3] = to;
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
