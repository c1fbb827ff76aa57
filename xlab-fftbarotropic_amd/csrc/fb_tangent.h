// fb_tangent.h -- kernels of the tangent-linear model (fb_model_set_tangent, fb_slab_set_tangent; host side: fb_beside_tangent.h, tangent_stage).
//
// A perturbation dz of the vorticity is carried along the evolving state by the linearisation of the discrete step: at every RK stage
//   tend_dz = dealiase( r2c(-u dz_x - v dz_y  -  du zeta_x - dv zeta_y) + nu laplacian(dz_c) ),
//   u = -psi_y, v = psi_x, du = -dpsi_y, dv = dpsi_x,  psi_c = invertLaplacian(zeta_c), dpsi_c = invertLaplacian(dz_c),
// with zeta the vorticity's state of the same stage and nu the model's own.  A vorticity source does not depend on the state and has
// no term here.  The advective tendency J(a; psi) = -u a_x - v a_y is bilinear, and the tangent is J(dz; psi) + J(zeta; dpsi): two
// passes of record_advect per stage, the first one's result saved before the second overwrites it.  The state (base, stage state,
// accumulator) is kept as the tracer's is (fb_tracer.h): per column group in the 3-pass layout [nx][ncols], pad columns zero, the
// stage arrays written on the active column tiles only; a mode outside the dealiasing circle keeps its bits and is read from the
// base.  Per stage:
//   k_tracer_vstate_*  the vorticity's state of the stage into the 3-pass layout, where the step's layout is private (fb_tracer.h)
//   k_advect_deriv     gradx a, grady a, grady phi, gradx phi with (a, phi) = (dz, psi), then with (a, phi) = (zeta, dpsi) (fb_tracer.h)
//   (record_advect, fb_record.h: the backward x pass, the ROW_FUSED row pass without a source, the forward x pass; twice)
//   k_beside_update    the two tendencies summed, viscous term, mask, RK stage update (fb_tracer.h, NJ == 2)
// The stage's kernels are the tracer's, in fb_tracer.h; this file holds what is the tangent's own, between steps, on the bases of a set
// of perturbations on the one trajectory (fb_model_set_tangents; a single tangent, fb_model_set_tangent, is the set of one):
// k_tangent_scale, the inner product of two bases k_tangent_dot (+ k_tangent_dot_final), whose <a, a> is the norm, and the steps of a
// modified Gram-Schmidt sweep whose coefficients never leave the device, k_tangent_axpy, k_tangent_sqrt, k_tangent_scale_dev (host
// side: tangent_dot, tangent_gram, tangent_qr in fb_beside_tangent.h).
// No reference counterpart: the reference has no tangent-linear model.
#pragma once

// base *= a over a whole column group (n complex, a multiple of 16: pad columns stay zero); 16 bytes per lane and access
__global__ void __launch_bounds__(256) k_tangent_scale(cf *c0, size_t n, float a)
{
    float4 *q = reinterpret_cast<float4 *>(c0);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n / 2; p += (size_t)gridDim.x * blockDim.x) {
        float4 v = q[p];
        v.x *= a; v.y *= a; v.z *= a; v.w *= a;
        q[p] = v;
    }
}

// sum of a float64 per thread over the 256 threads of a workgroup, in a fixed order; the result in thread 0
FB_DEV double tangent_block_sum(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

// ---- inner products and in-place orthonormalisation of the bases ----
// The inner product of two perturbations over the resident half spectrum of one column group (the bases, 3-pass layout), in float64:
// sum over kx and ky <= ny/2 of w q Re(a conj(b)), with the Hermitian weight w = 1 in the columns ky = 0 and ky = ny/2 and 2 elsewhere;
// kind 0 (enstrophy): q = 1; kind 1 (energy): q = |k|^2 / laplacian_coe^2 = |grad dpsi|^2 / |dz|^2 of the mode, the (0, 0) mode left out.
// a == b is allowed and gives the squared norm: each summand, two products of float32 values, is exact in float64 before it is
// rounded once, fused or not.  One partial sum per workgroup into part[blockIdx.x]: no atomics, the same grid gives the same bits.
__global__ void __launch_bounds__(256) k_tangent_dot(SpecCoef c, const cf *a0, const cf *b0, int kind, int P, int N1, int N2, int ky0, double *__restrict__ part)
{
    __shared__ double sh[256];
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    double acc = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        if (ky0 + col >= c.hy) continue;
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const float4 a = reinterpret_cast<const float4 *>(a0)[p], b = reinterpret_cast<const float4 *>(b0)[p];
        const double re[2] = {(double)a.x * b.x + (double)a.y * b.y, (double)a.z * b.z + (double)a.w * b.w};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            if (j >= c.hy) continue;
            double q = (j == 0 || j == c.hy - 1) ? 1.0 : 2.0;
            if (kind == 1) {
                const double lap = (double)coef_lap(c, i, j);
                q = (i == 0 && j == 0) ? 0.0 : q * (c.kx2[i] + c.ky2[j]) / (lap * lap);
            }
            acc += q * re[e];
        }
    }
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the partial sums of every column group, in a fixed order -> *out = scale * sum (scale = 1 / (2 GRIDS^2): half the mean square)
__global__ void __launch_bounds__(256) k_tangent_dot_final(const double *__restrict__ part, int nparts, double scale, double *__restrict__ out)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) acc += part[k];
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) *out = s * scale;
}

// v -= r q over a whole column group (n complex, a multiple of 16), r a float64 on the device (a dot product that the host never
// waits for); every element formed in float64 and rounded once to float32.  Pad columns stay zero: 0 - r 0.
__global__ void __launch_bounds__(256) k_tangent_axpy(cf *__restrict__ v0, const cf *__restrict__ q0, size_t n, const double *__restrict__ rp)
{
#pragma clang fp contract(off)
    const double r = *rp;
    float4 *v4 = reinterpret_cast<float4 *>(v0);
    const float4 *q4 = reinterpret_cast<const float4 *>(q0);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n / 2; p += (size_t)gridDim.x * blockDim.x) {
        float4 v = v4[p];
        const float4 q = q4[p];
        v.x = (float)((double)v.x - r * (double)q.x); v.y = (float)((double)v.y - r * (double)q.y);
        v.z = (float)((double)v.z - r * (double)q.z); v.w = (float)((double)v.w - r * (double)q.w);
        v4[p] = v;
    }
}

// *x = sqrt(*x): <v, v> into r_jj where it stands (one lane)
__global__ void k_tangent_sqrt(double *x)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *x = sqrt(*x);
}

// v /= r over a whole column group, r a float64 on the device; the quotient formed in float64 and rounded once to float32
__global__ void __launch_bounds__(256) k_tangent_scale_dev(cf *__restrict__ v0, size_t n, const double *__restrict__ rp)
{
#pragma clang fp contract(off)
    const double r = *rp;
    float4 *v4 = reinterpret_cast<float4 *>(v0);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n / 2; p += (size_t)gridDim.x * blockDim.x) {
        float4 v = v4[p];
        v.x = (float)((double)v.x / r); v.y = (float)((double)v.y / r); v.z = (float)((double)v.z / r); v.w = (float)((double)v.w / r);
        v4[p] = v;
    }
}

// the lower triangle of a row-major [m][m] matrix from its upper one (one workgroup)
__global__ void __launch_bounds__(256) k_tangent_mirror(double *g, int m)
{
    for (int k = threadIdx.x; k < m * m; k += 256) {
        const int i = k / m, j = k - i * m;
        if (i > j) g[k] = g[j * m + i];
    }
}
