// fb_tangent.h -- kernels of the tangent-linear model (fb_model_set_tangent, fb_slab_set_tangent; host side: fb_record.h, tangent_stage).
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
//   k_tangent_deriv    gradx a, grady a, grady phi, gradx phi with (a, phi) = (dz, psi), then with (a, phi) = (zeta, dpsi)
//   (record_advect, fb_record.h: the backward x pass, the ROW_FUSED row pass without a source, the forward x pass; twice)
//   k_tangent_update   the two tendencies summed, viscous term, mask, RK stage update
// Between steps: k_tangent_norm (+ k_tangent_norm_final) and k_tangent_scale on the base.
// No reference counterpart: the reference has no tangent-linear model.
#pragma once

// The four fields a stage hands to its row pass for J(a; phi), into the fields 0..3 of `z`, fstride apart: gradx(a_c), grady(a_c),
// grady(phi_c), gradx(phi_c) with phi_c = invertLaplacian(b_c) (the (0, 0) mode divided by 1, as k_tracer_deriv has it).  a0 / a1: the
// base / stage state of the advected field, b0 / b1: of the field whose streamfunction advects; all in the 3-pass layout, a mode
// outside the dealiasing circle is read from the base.  Either pair may be field 2 of z (the vorticity's stage state out of
// k_tracer_vstate_*): each element is read before it is written, by the same thread, so no pointer here is __restrict__.  Two modes
// (16 bytes) per lane and access; pad columns zero; the float32 forms of k_tracer_deriv (no contraction).
__global__ void __launch_bounds__(256) k_tangent_deriv(SpecCoef c, const cf *a0, const cf *a1, const cf *b0, const cf *b1, cf *z, long fstride, int P, int N1,
                                                       int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t idx = 2 * p;
        cf o[4][2];
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if (ky0 + col < c.hy) {
            // (uniform but at the circle's edge) both modes of the pair from one array where both are live or both are masked
            const bool l0 = coef_mask(c, i, ky0 + col) != 0.0f, l1 = coef_mask(c, i, ky0 + col + 1) != 0.0f;
            if (l0 == l1) {
                av = *reinterpret_cast<const float4 *>((l0 ? a1 : a0) + idx);
                bv = *reinterpret_cast<const float4 *>((l0 ? b1 : b0) + idx);
            } else {
                const cf ax = (l0 ? a1 : a0)[idx], ay = (l1 ? a1 : a0)[idx + 1], bx = (l0 ? b1 : b0)[idx], by = (l1 ? b1 : b0)[idx + 1];
                av = make_float4(ax.x, ax.y, ay.x, ay.y); bv = make_float4(bx.x, bx.y, by.x, by.y);
            }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            o[0][e] = o[1][e] = o[2][e] = o[3][e] = cf_make(0.f, 0.f);
            if (j < c.hy) {
                const cf a = e ? cf_make(av.z, av.w) : cf_make(av.x, av.y), b = e ? cf_make(bv.z, bv.w) : cf_make(bv.x, bv.y);
                const float kx = c.gx[i], ky = c.gy[j];
                o[0][e] = tr_grad(a, kx);
                o[1][e] = tr_grad(a, ky);
                const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);
                const cf ph = cf_make(b.x / li, b.y / li);
                o[2][e] = tr_grad(ph, ky);
                o[3][e] = tr_grad(ph, kx);
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
            *reinterpret_cast<float4 *>(z + (size_t)f * fstride + idx) = make_float4(o[f][0].x, o[f][0].y, o[f][1].x, o[f][1].y);
    }
}

// RK stage update of the perturbation on the first `ncr` columns of a column group: k_tracer_update (fb_tracer.h) with the two
// tendencies j1 = r2c(J(dz; psi)) and j2 = r2c(J(zeta; dpsi)) summed before the viscous term and the mask,
//   k = ((j1 + j2) + (dz_stage * laplacian_coe) * nu) * mask,
// and its stage forms in its rounding.  A masked mode keeps its bits.  Stages 0..2 write acc and c1, stage 3 the new base into c0.
// Two modes per lane and access (16 bytes), no LDS.
template <int STAGE>
__global__ void __launch_bounds__(256) k_tangent_update(SpecCoef c, const cf *__restrict__ j1, const cf *__restrict__ j2, cf *c0, cf *c1, cf *acc, float nu,
                                                        float dt, int P, int ncr, int N1, int N2, int ky0)
{
    const int hp = ncr >> 1;
    const size_t total = (size_t)c.nx * hp;
    const float hdt = STAGE == 2 ? dt : dt / 2.0f;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t q = ((size_t)row * P + col) >> 1;                                  // float4 index
        const float4 t1 = reinterpret_cast<const float4 *>(j1)[q], t2 = reinterpret_cast<const float4 *>(j2)[q], z0 = reinterpret_cast<const float4 *>(c0)[q];
        float4 zc = z0, ac = make_float4(0.f, 0.f, 0.f, 0.f);
        if (STAGE != 0) { zc = reinterpret_cast<const float4 *>(c1)[q]; ac = reinterpret_cast<const float4 *>(acc)[q]; }
        const float th[4] = {t1.x + t2.x, t1.y + t2.y, t1.z + t2.z, t1.w + t2.w}, b[4] = {z0.x, z0.y, z0.z, z0.w}, s[4] = {zc.x, zc.y, zc.z, zc.w},
                    a[4] = {ac.x, ac.y, ac.z, ac.w};
        float an[4], zn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = ky0 + col + (e >> 1);
            const float msk = coef_mask(c, i, j);
            const float lap = j < c.hy ? coef_lap(c, i, j) : 0.0f;
            const float k = (th[e] + (s[e] * lap) * nu) * msk;
            if (STAGE == 0) { an[e] = k; zn[e] = __builtin_fmaf(k, hdt, b[e]); }
            else if (STAGE < 3) { an[e] = a[e] + 2.0f * k; zn[e] = b[e] + k * hdt; }
            else { an[e] = a[e]; zn[e] = b[e] + (a[e] + k) * dt / 6.0f; }
            if (msk == 0.0f) { an[e] = 0.0f; zn[e] = b[e]; }
        }
        const float4 zo = make_float4(zn[0], zn[1], zn[2], zn[3]);
        if (STAGE < 3) {
            reinterpret_cast<float4 *>(acc)[q] = make_float4(an[0], an[1], an[2], an[3]);
            reinterpret_cast<float4 *>(c1)[q] = zo;
        } else reinterpret_cast<float4 *>(c0)[q] = zo;
    }
}

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

// The squared norm of the perturbation over the resident half spectrum of one column group (the base, 3-pass layout), in float64:
// sum over kx and ky <= ny/2 of w |dz_c|^2 q, with the Hermitian weight w = 1 in the columns ky = 0 and ky = ny/2 and 2 elsewhere;
// kind 0 (enstrophy): q = 1; kind 1 (energy): q = |k|^2 / laplacian_coe^2 = |grad dpsi|^2 / |dz|^2 of the mode, the (0, 0) mode left out.
// One partial sum per workgroup into part[blockIdx.x]: no atomics, the same grid gives the same bits.
__global__ void __launch_bounds__(256) k_tangent_norm(SpecCoef c, const cf *__restrict__ c0, int kind, int P, int N1, int N2, int ky0, double *__restrict__ part)
{
    __shared__ double sh[256];
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    double acc = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        if (ky0 + col >= c.hy) continue;
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const float4 v = reinterpret_cast<const float4 *>(c0)[p];
        const double m2[2] = {(double)v.x * v.x + (double)v.y * v.y, (double)v.z * v.z + (double)v.w * v.w};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            if (j >= c.hy) continue;
            double q = (j == 0 || j == c.hy - 1) ? 1.0 : 2.0;
            if (kind == 1) {
                const double lap = (double)coef_lap(c, i, j);
                q = (i == 0 && j == 0) ? 0.0 : q * (c.kx2[i] + c.ky2[j]) / (lap * lap);
            }
            acc += q * m2[e];
        }
    }
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the partial sums of every column group, in a fixed order -> *out = scale * sum (scale = 1 / (2 GRIDS^2): half the mean square)
__global__ void __launch_bounds__(256) k_tangent_norm_final(const double *__restrict__ part, int nparts, double scale, double *__restrict__ out)
{
    __shared__ double sh[256];
    double acc = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) acc += part[k];
    const double s = tangent_block_sum(acc, sh);
    if (threadIdx.x == 0) *out = s * scale;
}
