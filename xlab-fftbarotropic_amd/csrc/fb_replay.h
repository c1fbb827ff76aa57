// fb_replay.h -- kernels of the tangent replay over the adjoint's tape (fb_model_tangent_replay and its fb_slab_* twin on one rank; host
// side: fb_beside_adjoint.h, replay_stage).
//
// The tangent-linear step of fb_tangent.h applied to a set of perturbations about stage states that are already on the adjoint's tape
// (fb_adjoint.h): nothing nonlinear is stepped.  With zeta the recorded stage state, u = -psi_y, v = psi_x its velocity and dz the
// perturbation's state of the same stage, the stage's tangent tendency is formed as ONE product in physical space,
//   tend_dz = dealiase( r2c( (((-u dz_x) - v dz_y) - du zeta_x) - dv zeta_y ) + nu laplacian(dz_c) ),   du = -dpsi_y, dv = dpsi_x,
// where the live tangent (tangent_stage) sums two spectral tendencies: the same operator, not the same bits.  u, v, zeta_x, zeta_y
// depend on the tape alone and are formed once per stage for the whole set (k_adjoint_base, fb_adjoint.h).  Per stage:
//   k_adjoint_base       grady psi, gradx psi, gradx zeta, grady zeta of the recorded state, once (fb_adjoint.h)
//   k_replay_deriv       grady dpsi, gradx dpsi, gradx dz, grady dz of one perturbation's stage state
//   (the backward x pass of the four fields, four ROW_INV row passes into real fields, for the base and per perturbation)
//   k_replay_prod_set    the product above for a chunk of up to REPLAY_CHUNK perturbations, out of place, the base fields read once
//   (per perturbation: one ROW_FWD row pass, its forward x pass)
//   k_beside_update      viscous term, mask, RK stage update (fb_tracer.h, NJ == 1 with the model's nu: the launch the tracer makes)
// Every pass works on whole fields and the product is one fixed expression per element: perturbation k of a replayed set has the bits
// of the replayed set of one.  No atomics: two runs give the same bits.
// No reference counterpart: the reference has no tangent-linear model.
#pragma once

#define REPLAY_CHUNK 8

// a0 / a1: base and stage state of one perturbation in the 3-pass layout (stage 0: both the base), a mode outside the dealiasing
// circle read from the base: the merge rule of k_advect_deriv.  z: field f at z + f * fstride: 0 grady dpsi, 1 gradx dpsi, 2 gradx dz,
// 3 grady dz, the order k_adjoint_base leaves the base flow's in, in the float32 forms of k_advect_deriv (no contraction).  Two modes
// (16 bytes) per lane and access; pad columns zero.
__global__ void __launch_bounds__(256) k_replay_deriv(SpecCoef c, const cf *a0, const cf *a1, cf *__restrict__ z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t idx = 2 * p;
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ky0 + col < c.hy) {
            // (uniform but at the circle's edge) both modes of the pair from one array where both are live or both are masked
            const bool l0 = coef_mask(c, i, ky0 + col) != 0.0f, l1 = coef_mask(c, i, ky0 + col + 1) != 0.0f;
            if (l0 == l1) av = *reinterpret_cast<const float4 *>((l0 ? a1 : a0) + idx);
            else {
                const cf ax = (l0 ? a1 : a0)[idx], ay = (l1 ? a1 : a0)[idx + 1];
                av = make_float4(ax.x, ax.y, ay.x, ay.y);
            }
        }
        cf o[4][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            o[0][e] = o[1][e] = o[2][e] = o[3][e] = cf_make(0.f, 0.f);
            if (j < c.hy) {
                const cf a = e ? cf_make(av.z, av.w) : cf_make(av.x, av.y);
                const float kx = c.gx[i], ky = c.gy[j];
                const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);
                const cf ph = cf_make(a.x / li, a.y / li);
                o[0][e] = tr_grad(ph, ky);
                o[1][e] = tr_grad(ph, kx);
                o[2][e] = tr_grad(a, kx);
                o[3][e] = tr_grad(a, ky);
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
            *reinterpret_cast<float4 *>(z + (size_t)f * fstride + idx) = make_float4(o[f][0].x, o[f][0].y, o[f][1].x, o[f][1].y);
    }
}

// one element of the tangent tendency's product in physical space, in the order written (a float32 numpy restatement reproduces it)
FB_DEV float replay_prod(float u, float v, float zx, float zy, float du, float dv, float dzx, float dzy)
{
#pragma clang fp contract(off)
    return (((-u * dzx) - v * dzy) - du * zx) - dv * zy;
}

// base: four real fields [4][n], n = nx * ny (a multiple of 4): u, v, zeta_x, zeta_y as the ROW_INV passes left them; pert: [CNT][4][n],
// du, dv, dz_x, dz_y of the chunk's perturbations; out: [CNT][n], one product field each.  The four base values are read once and stay
// in registers while the perturbations stream past, two in flight at a time (8 loads): the whole chunk's 4 CNT loads at once would not
// fit beside them.  16 bytes per lane and access over contiguous rows, no LDS, no atomics.
template <int CNT>
__global__ void __launch_bounds__(256) k_replay_prod_set(const float *__restrict__ base, const float *__restrict__ pert, float *__restrict__ out, size_t n)
{
    const size_t n4 = n / 4;
    const float4 *b = reinterpret_cast<const float4 *>(base), *q = reinterpret_cast<const float4 *>(pert);
    float4 *o = reinterpret_cast<float4 *>(out);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (size_t)gridDim.x * blockDim.x) {
        float4 v[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) v[f] = b[(size_t)f * n4 + p];
#pragma unroll 2
        for (int k = 0; k < CNT; ++k) {
            float4 d[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) d[f] = q[((size_t)k * 4 + f) * n4 + p];
            o[(size_t)k * n4 + p] = make_float4(replay_prod(v[0].x, v[1].x, v[2].x, v[3].x, d[0].x, d[1].x, d[2].x, d[3].x),
                                                replay_prod(v[0].y, v[1].y, v[2].y, v[3].y, d[0].y, d[1].y, d[2].y, d[3].y),
                                                replay_prod(v[0].z, v[1].z, v[2].z, v[3].z, d[0].z, d[1].z, d[2].z, d[3].z),
                                                replay_prod(v[0].w, v[1].w, v[2].w, v[3].w, d[0].w, d[1].w, d[2].w, d[3].w));
        }
    }
}
