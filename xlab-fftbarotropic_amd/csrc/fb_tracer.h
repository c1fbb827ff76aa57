// fb_tracer.h -- kernels of the passive tracer (fb_model_set_tracer, fb_slab_set_tracer_local; host side: fb_beside.h, tracer_stage), shared
// by every field stepped beside the vorticity (the tangent-linear model, fb_tangent.h, launches the same ones).
//
// A tracer c is a second real field advected by the model's velocity, with a diffusivity kappa of its own:
//   tend_c = dealiase( r2c(-u c_x - v c_y) + kappa laplacian(c_c) ),   u = -psi_y, v = psi_x of the vorticity's state of the same RK stage,
// stepped by the RK4 scheme of main.cpp:288-317 stage by stage beside the vorticity.  Its state (base, stage state, accumulator) is
// kept per column group in the record layer's 3-pass layout [nx][ncols] (row N2*c + d holds kx = c + N1*d, local column j holds
// ky = ky0 + j), pad columns zero.  Per stage:
//   k_tracer_vstate    the vorticity's state of the stage out of the step's own layout into a field of the record workspace
//   k_advect_deriv     gradx c, grady c, grady psi, gradx psi: what k_col_mid hands to the row pass, with c in the place of zeta
//   (the backward x pass, the ROW_FUSED row pass without a source and the forward x pass: fb_record.h, record_advect)
//   k_beside_update    viscous term, mask, RK stage update of the tracer
// The step stores its stage state and accumulator only where a mode can change (SURVEY note N1): for a mode outside the dealiasing
// circle the stage state IS the base, and both k_tracer_vstate and k_advect_deriv read it from there.
// No reference counterpart: the reference advects no tracer.
#pragma once

// ---- the vorticity's stage state -> 3-pass layout ----
// za: vort_c0, zb: the stage state (stage 0 and groups of frozen columns: zb == za).  The pad columns next to ny/2 are written as
// zeros (k_advect_deriv loads column pairs); it uses nothing at or beyond ny/2 + 1.
// tile-major state arrays (k_state_relayout; three-kernel path with N2 >= 32)
__global__ void __launch_bounds__(256) k_tracer_vstate_tm(SpecCoef c, const cf *__restrict__ za, const cf *__restrict__ zb, cf *__restrict__ out, int P,
                                                          int N1, int N2, int ky0)
{
    const int R1 = N2 >> 3, NLB = N2 >> 2, ntc = P >> 4;
    const size_t total = (size_t)c.nx * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / P), col = (int)(idx - (size_t)row * P);
        const int cb = row / N2, d = row - cb * N2, ct = col >> 4, cl = col & 15;
        const int q = d / R1, rem = d - q * R1, h = rem & 3, sidx = rem >> 2, e = 8 * sidx + q;
        const size_t tile = (size_t)cb * ntc + ct;
        const size_t tm = ((tile * (NLB / 2) + (e >> 1)) * 64 + (16 * h + cl)) * 2 + (e & 1);
        const int j = ky0 + col;
        if (j >= c.hy) { out[idx] = cf_make(0.f, 0.f); continue; }
        out[idx] = coef_mask(c, cb + N1 * d, j) != 0.0f ? zb[tm] : za[tm];
    }
}
// k_col_full's state arrays (k_full_relayout): [k1][tile 0..ntiles][k3][thread][col]
__global__ void __launch_bounds__(256) k_tracer_vstate_full(SpecCoef c, const cf *__restrict__ za, const cf *__restrict__ zb, cf *__restrict__ out, int P,
                                                            int N1, int N2, int ntiles, int nsub)
{
    const size_t total = (size_t)nsub * (ntiles + 1) * 16 * 1024 * 2;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int col = (int)(idx & 1);
        const int tid = (int)((idx >> 1) & 1023);
        const int k3 = (int)((idx >> 11) & 15);
        const int st = (int)(idx >> 15);                             // k1 * (ntiles + 1) + tile
        const int k1 = st / (ntiles + 1), tile = st - k1 * (ntiles + 1);
        const int w = tid >> 6, l = (tid >> 2) & 15, cq = tid & 3;
        const int kx = nsub * (w + 16 * l + 256 * k3) + k1, ky = tile * 8 + 2 * cq + col;
        const int cc = kx % N1, d = kx / N1;                         // 3-pass layout: row N2*cc + d holds kx = cc + N1*d
        if (ky >= c.hy) { out[(size_t)(N2 * cc + d) * P + ky] = cf_make(0.f, 0.f); continue; }      // (ky <= ny/2 + 7 < P)
        out[(size_t)(N2 * cc + d) * P + ky] = coef_mask(c, kx, ky) != 0.0f ? zb[idx] : za[idx];
    }
}

FB_DEV cf tr_grad(cf a, float k)
{
#pragma clang fp contract(off)
    return cf_make(-a.y * k, a.x * k);                                              // fftwfop.cpp:87-103
}

// The four fields a stage hands to its row pass for the advective tendency J(a; phi) = -u a_x - v a_y, u = -phi_y, v = phi_x, into the
// fields 0..3 of `z`, fstride apart: gradx(a_c), grady(a_c), grady(phi_c), gradx(phi_c) with phi_c = invertLaplacian(b_c) (the (0, 0)
// mode divided by 1): what k_col_mid hands to the row pass, with a in the place of zeta.  a0 / a1: the base / stage state of the
// advected field, b0 / b1: of the field whose streamfunction advects; all in the 3-pass layout, a mode outside the dealiasing circle
// is read from the base.  Either pair may be field 2 of z (the vorticity's stage state out of k_tracer_vstate_*): each element is read
// before it is written, by the same thread, so no pointer here is __restrict__.  Two modes (16 bytes) per lane and access; pad columns
// zero.  Same float32 forms as k_spec_op (no contraction).
__global__ void __launch_bounds__(256) k_advect_deriv(SpecCoef c, const cf *a0, const cf *a1, const cf *b0, const cf *b1, cf *z, long fstride, int P, int N1,
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
                o[0][e] = tr_grad(a, kx);                                           // main.cpp:151 with a_c
                o[1][e] = tr_grad(a, ky);                                           // main.cpp:165 with a_c
                const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);     // fftwfop.cpp:42-43,112-117 (main.cpp:179)
                const cf ph = cf_make(b.x / li, b.y / li);
                o[2][e] = tr_grad(ph, ky);                                          // main.cpp:198
                o[3][e] = tr_grad(ph, kx);                                          // main.cpp:212
            }
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
            *reinterpret_cast<float4 *>(z + (size_t)f * fstride + idx) = make_float4(o[f][0].x, o[f][0].y, o[f][1].x, o[f][1].y);
    }
}

// RK stage update of a field stepped beside the vorticity on the first `ncr` columns of a column group (the tiles that hold a mode
// inside the dealiasing circle; the columns beyond never change), from NJ tendencies as the forward x pass left them: j1 alone (the
// tracer: r2c(-u c_x - v c_y)) or j1 + j2 (the tangent-linear model: r2c(J(dz; psi)) and r2c(J(zeta; dpsi)), summed before the viscous
// term and the mask; NJ == 1 never reads j2).  c0 the base, c1 the stage state, acc the running rk1 + 2 rk2 + 2 rk3, all in the 3-pass
// layout with pitch P; kappa the field's diffusivity (the tangent's is the model's nu).
//   k = (jh + (c_stage * laplacian_coe) * kappa) * mask     main.cpp:240-243 with kappa, main.cpp:148
// and the stage forms of k_col_mid, in its rounding: the explicit fma at stage 0, the accumulator as ac + 2 k, the final combination
// as z0 + (ac + k) * dt / 6 (main.cpp:246-251,296-312).  A masked mode keeps its bits: its stage state is the base, its accumulator
// zero.  Stages 0..2 write acc and c1, stage 3 the new base into c0.  Two modes per lane and access (16 bytes), no LDS.
template <int STAGE, int NJ>
__global__ void __launch_bounds__(256) k_beside_update(SpecCoef c, const cf *__restrict__ j1, const cf *__restrict__ j2, cf *c0, cf *c1, cf *acc, float kappa,
                                                       float dt, int P, int ncr, int N1, int N2, int ky0)
{
    const int hp = ncr >> 1;
    const size_t total = (size_t)c.nx * hp;
    const float hdt = STAGE == 2 ? dt : dt / 2.0f;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t q = ((size_t)row * P + col) >> 1;                                  // float4 index
        float4 t = reinterpret_cast<const float4 *>(j1)[q];
        if (NJ == 2) { const float4 t2 = reinterpret_cast<const float4 *>(j2)[q]; t = make_float4(t.x + t2.x, t.y + t2.y, t.z + t2.z, t.w + t2.w); }
        const float4 z0 = reinterpret_cast<const float4 *>(c0)[q];
        float4 zc = z0, ac = make_float4(0.f, 0.f, 0.f, 0.f);
        if (STAGE != 0) { zc = reinterpret_cast<const float4 *>(c1)[q]; ac = reinterpret_cast<const float4 *>(acc)[q]; }
        const float th[4] = {t.x, t.y, t.z, t.w}, b[4] = {z0.x, z0.y, z0.z, z0.w}, s[4] = {zc.x, zc.y, zc.z, zc.w}, a[4] = {ac.x, ac.y, ac.z, ac.w};
        float an[4], zn[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = ky0 + col + (e >> 1);
            const float msk = coef_mask(c, i, j);
            const float lap = j < c.hy ? coef_lap(c, i, j) : 0.0f;                      // fftwfop.cpp:42,45 (the tables end at ny/2)
            const float k = (th[e] + (s[e] * lap) * kappa) * msk;
            if (STAGE == 0) { an[e] = k; zn[e] = __builtin_fmaf(k, hdt, b[e]); }        // main.cpp:296
            else if (STAGE < 3) { an[e] = a[e] + 2.0f * k; zn[e] = b[e] + k * hdt; }    // main.cpp:299,302
            else { an[e] = a[e]; zn[e] = b[e] + (a[e] + k) * dt / 6.0f; }               // main.cpp:309-312
            if (msk == 0.0f) { an[e] = 0.0f; zn[e] = b[e]; }
        }
        const float4 zo = make_float4(zn[0], zn[1], zn[2], zn[3]);
        if (STAGE < 3) {
            reinterpret_cast<float4 *>(acc)[q] = make_float4(an[0], an[1], an[2], an[3]);
            reinterpret_cast<float4 *>(c1)[q] = zo;
        } else reinterpret_cast<float4 *>(c0)[q] = zo;
    }
}
