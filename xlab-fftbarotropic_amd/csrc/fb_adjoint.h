// fb_adjoint.h -- kernels of the adjoint model (fb_model_adjoint_record, fb_model_set_adjoint, fb_model_adjoint_back and their fb_slab_*
// twins on one rank; host side: fb_beside_adjoint.h, adjoint_stage).
//
// The transpose of the tangent-linear step of fb_tangent.h under the inner product <a, b> = sum over the grid of a b.  With zeta the
// vorticity's state of an RK stage (from the tape: the stage states recorded while the model stepped forward, masked modes merged in
// from the base), mask the dealiasing mask and mu~ = mask mu, the transpose of the stage's tangent tendency is
//   L^T mu = gradx(u mu~) + grady(v mu~) + invertLaplacian( gradx(zeta_y mu~) - grady(zeta_x mu~) ) + nu laplacian(mu~),
//   u = -psi_y, v = psi_x, psi_c = invertLaplacian(zeta_c), the products in physical space, the result NOT masked again,
// and one RK4 step backward, with lam the adjoint variable, takes the stages in the order 3, 2, 1, 0:
//   kb = dt/6 lam, acc = lam;   a = L3^T kb: acc += a, kb = dt/3 lam + dt a;   a = L2^T kb: acc += a, kb = dt/3 lam + dt/2 a;
//   a = L1^T kb: acc += a, kb = dt/6 lam + dt/2 a;   lam = acc + L0^T kb.
// Every array is a half spectrum in the 3-pass layout [nx][P] (fb_tracer.h), pad columns zero.  In the spectral inner product with
// the Hermitian weights the transpose of c2r is r2c and the reverse, and that of a multiplier is its complex conjugate, so the
// sweep stays in half spectra: r2c of lam on the way in (beside_in), c2r on the way out (record).  Per stage:
//   k_adjoint_deriv    mu~, grady psi, gradx psi, gradx zeta, grady zeta into the fields 0..4 of the record workspace
//   (the backward x pass of the five fields, five ROW_INV row passes into real fields)
//   k_adjoint_prod     u mu~, v mu~, zeta_x mu~, zeta_y mu~ in physical space, in place
//   (four ROW_FWD row passes into the fields 0..3 of the record workspace, their forward x pass)
//   k_adjoint_update   the multipliers, the viscous term, acc and the next kb
// and while the model steps forward with recording on, at the top of every stage:
//   k_adjoint_merge    base and stage state merged by the mask into the tape's slot, where the step keeps its state in the 3-pass layout
//                      (elsewhere k_tracer_vstate_* does the same, fb_tracer.h)
// No atomics and a fixed order of arithmetic everywhere: two runs give the same bits.
// No reference counterpart: the reference has no adjoint model.
#pragma once

// ---- the tape: base and stage state of the vorticity in the 3-pass layout -> one array, a masked mode from the base, pad columns zero ----
// Two modes (16 bytes) per lane and access; P is a multiple of 16, so a pair never straddles a row.
__global__ void __launch_bounds__(256) k_adjoint_merge(SpecCoef c, const cf *__restrict__ za, const cf *__restrict__ zb, cf *__restrict__ out, int P, int N1,
                                                       int N2, int ky0)
{
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const int j = ky0 + col;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < c.hy) {
            const float4 a = reinterpret_cast<const float4 *>(za)[p], b = reinterpret_cast<const float4 *>(zb)[p];
            const bool l0 = coef_mask(c, i, j) != 0.0f, l1 = coef_mask(c, i, j + 1) != 0.0f;
            o.x = l0 ? b.x : a.x; o.y = l0 ? b.y : a.y;
            if (j + 1 < c.hy) { o.z = l1 ? b.z : a.z; o.w = l1 ? b.w : a.w; }
        }
        reinterpret_cast<float4 *>(out)[p] = o;
    }
}

// ---- the five spectra a stage hands to its backward x pass ----
// zs: the stage state (a slot of the tape), kb: the k-bar, taken times ks (stage 3: kb = lam, ks = dt/6; else ks = 1); z: the record
// workspace, field f at z + f * fstride: 0 mu~ = mask ks kb, 1 grady psi, 2 gradx psi, 3 gradx zeta, 4 grady zeta, in the float32
// forms of k_advect_deriv (no contraction).  Two modes per lane and access; pad columns zero.
__global__ void __launch_bounds__(256) k_adjoint_deriv(SpecCoef c, const cf *__restrict__ zs, const cf *__restrict__ kb, float ks, cf *__restrict__ z, long fstride,
                                                       int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t idx = 2 * p;
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f), kv = zv;
        if (ky0 + col < c.hy) { zv = reinterpret_cast<const float4 *>(zs)[p]; kv = reinterpret_cast<const float4 *>(kb)[p]; }
        cf o[5][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            o[0][e] = o[1][e] = o[2][e] = o[3][e] = o[4][e] = cf_make(0.f, 0.f);
            if (j < c.hy) {
                const cf a = e ? cf_make(zv.z, zv.w) : cf_make(zv.x, zv.y), k = e ? cf_make(kv.z, kv.w) : cf_make(kv.x, kv.y);
                const float msk = coef_mask(c, i, j), kx = c.gx[i], ky = c.gy[j];
                o[0][e] = cf_make((k.x * ks) * msk, (k.y * ks) * msk);
                const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);
                const cf ph = cf_make(a.x / li, a.y / li);
                o[1][e] = tr_grad(ph, ky);
                o[2][e] = tr_grad(ph, kx);
                o[3][e] = tr_grad(a, kx);
                o[4][e] = tr_grad(a, ky);
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f)
            *reinterpret_cast<float4 *>(z + (size_t)f * fstride + idx) = make_float4(o[f][0].x, o[f][0].y, o[f][1].x, o[f][1].y);
    }
}

// ---- the products in physical space ----
// r: five real fields [5][n], n = nx * ny (a multiple of 4): mu~, u, v, zeta_x, zeta_y as the ROW_INV passes left them; the fields
// 1..4 become u mu~, v mu~, zeta_x mu~, zeta_y mu~ in place.  16 bytes per lane and access over contiguous rows.
__global__ void __launch_bounds__(256) k_adjoint_prod(float *__restrict__ r, size_t n)
{
    const size_t n4 = n / 4;
    float4 *q = reinterpret_cast<float4 *>(r);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (size_t)gridDim.x * blockDim.x) {
        const float4 m = q[p];
#pragma unroll
        for (int f = 1; f < 5; ++f) {
            float4 v = q[(size_t)f * n4 + p];
            v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
            q[(size_t)f * n4 + p] = v;
        }
    }
}

// ---- the stage's transpose tendency and the recurrences ----
// z: the spectra of u mu~, v mu~, zeta_x mu~, zeta_y mu~ in the fields 0..3 as the forward x pass left them; lam: the adjoint variable
// (c0), kb: the k-bar (c1), acc (all [nx][P]):
//   a = gradx(z0) + grady(z1) + (gradx(z3) - grady(z2)) / laplacian_coe + ((mask kb_s) laplacian_coe) nu      ((0, 0): / 1)
// with kb_s the k-bar this stage started from (stage 3: dt/6 lam), then
//   stage 3: acc = lam + a, kb = dt/3 lam + dt a     stage 2: acc += a, kb = dt/3 lam + dt/2 a
//   stage 1: acc += a, kb = dt/6 lam + dt/2 a         stage 0: lam = acc + a
// over every column (the result is not masked); pad columns are written as zeros.  Two modes per lane and access, no LDS; every sum
// in the order written, no contraction.
template <int STAGE>
__global__ void __launch_bounds__(256) k_adjoint_update(SpecCoef c, const cf *__restrict__ z, long fstride, cf *lam, cf *kb, cf *acc, float nu, float dt, int P,
                                                        int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    const float c_l = (STAGE == 3 || STAGE == 2) ? dt / 3.0f : dt / 6.0f;       // the next k-bar's share of lam
    const float c_a = STAGE == 3 ? dt : dt / 2.0f;                              // ... and of a
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        float4 out_l = make_float4(0.f, 0.f, 0.f, 0.f), out_k = out_l, out_a = out_l;
        if (ky0 + col < c.hy) {
            float4 zf[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) zf[f] = *reinterpret_cast<const float4 *>(z + (size_t)f * fstride + 2 * p);
            const float4 lv = reinterpret_cast<const float4 *>(lam)[p];
            float4 kv = lv, av = lv;
            if (STAGE != 3) { kv = reinterpret_cast<const float4 *>(kb)[p]; av = reinterpret_cast<const float4 *>(acc)[p]; }
            float ol[4], ok[4], oa[4];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int j = ky0 + col + e;
                ol[2 * e] = ol[2 * e + 1] = ok[2 * e] = ok[2 * e + 1] = oa[2 * e] = oa[2 * e + 1] = 0.0f;
                if (j >= c.hy) continue;
                const cf p0 = e ? cf_make(zf[0].z, zf[0].w) : cf_make(zf[0].x, zf[0].y), p1 = e ? cf_make(zf[1].z, zf[1].w) : cf_make(zf[1].x, zf[1].y);
                const cf p2 = e ? cf_make(zf[2].z, zf[2].w) : cf_make(zf[2].x, zf[2].y), p3 = e ? cf_make(zf[3].z, zf[3].w) : cf_make(zf[3].x, zf[3].y);
                const cf l = e ? cf_make(lv.z, lv.w) : cf_make(lv.x, lv.y), k = e ? cf_make(kv.z, kv.w) : cf_make(kv.x, kv.y);
                const cf ac = e ? cf_make(av.z, av.w) : cf_make(av.x, av.y);
                const float kx = c.gx[i], ky = c.gy[j], msk = coef_mask(c, i, j), lap = coef_lap(c, i, j);
                const float li = (i == 0 && j == 0) ? 1.0f : lap;
                const cf g0 = tr_grad(p0, kx), g1 = tr_grad(p1, ky), g3 = tr_grad(p3, kx), g2 = tr_grad(p2, ky);
                const float ks = STAGE == 3 ? dt / 6.0f : 1.0f;
                const cf mt = cf_make((k.x * ks) * msk, (k.y * ks) * msk);
                cf a;
                a.x = ((g0.x + g1.x) + (g3.x - g2.x) / li) + (mt.x * lap) * nu;
                a.y = ((g0.y + g1.y) + (g3.y - g2.y) / li) + (mt.y * lap) * nu;
                if (STAGE == 3) { oa[2 * e] = l.x + a.x; oa[2 * e + 1] = l.y + a.y; }
                else if (STAGE != 0) { oa[2 * e] = ac.x + a.x; oa[2 * e + 1] = ac.y + a.y; }
                if (STAGE != 0) { ok[2 * e] = l.x * c_l + a.x * c_a; ok[2 * e + 1] = l.y * c_l + a.y * c_a; }
                else { ol[2 * e] = ac.x + a.x; ol[2 * e + 1] = ac.y + a.y; }
            }
            out_l = make_float4(ol[0], ol[1], ol[2], ol[3]); out_k = make_float4(ok[0], ok[1], ok[2], ok[3]); out_a = make_float4(oa[0], oa[1], oa[2], oa[3]);
        }
        if (STAGE != 0) { reinterpret_cast<float4 *>(kb)[p] = out_k; reinterpret_cast<float4 *>(acc)[p] = out_a; }
        else reinterpret_cast<float4 *>(lam)[p] = out_l;
    }
}

// ---- a set of adjoint variables on the one trajectory (fb_model_set_adjoints; host side: fb_beside_adjoint.h, adjoint_stage_set) ----
// Four of the five fields a stage takes back to physical space are functions of the recorded stage state alone, so a set of M
// variables forms them once per stage and each variable adds its own mu~:
//   k_adjoint_base     grady psi, gradx psi, gradx zeta, grady zeta into the fields 0..3 of the record workspace, once per stage
//   (their backward x pass and four ROW_INV row passes into real fields that the stage does not overwrite)
//   k_adjoint_mu       mu~_k = mask ks kb_k of a chunk of up to ADJOINT_CHUNK variables, one launch, into the set's own spectra
//   (the backward x pass of the chunk, one ROW_INV row pass per variable)
//   k_adjoint_prod_set u mu~_k, v mu~_k, zeta_x mu~_k, zeta_y mu~_k of the chunk out of place, the base fields read once
//   (per variable, as for the one: four ROW_FWD row passes, their forward x pass, k_adjoint_update)
// Every element is formed by the expression k_adjoint_deriv and k_adjoint_prod form it by: variable k of a set has the bits of the
// single variable started from the same field.
#define ADJOINT_CHUNK 8
struct AdjointKbars { const cf *kb[ADJOINT_CHUNK]; };

// zs: the stage state; z: field f at z + f * fstride: 0 grady psi, 1 gradx psi, 2 gradx zeta, 3 grady zeta, the fields 1..4 of
// k_adjoint_deriv in its float32 forms (no contraction).  Two modes per lane and access; pad columns zero.
__global__ void __launch_bounds__(256) k_adjoint_base(SpecCoef c, const cf *__restrict__ zs, cf *__restrict__ z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const size_t idx = 2 * p;
        float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ky0 + col < c.hy) zv = reinterpret_cast<const float4 *>(zs)[p];
        cf o[4][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = ky0 + col + e;
            o[0][e] = o[1][e] = o[2][e] = o[3][e] = cf_make(0.f, 0.f);
            if (j < c.hy) {
                const cf a = e ? cf_make(zv.z, zv.w) : cf_make(zv.x, zv.y);
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

// a.kb[k]: the k-bar of variable k of the chunk, taken times ks; z: mu~_k = mask ks kb_k at z + k * fstride, field 0 of
// k_adjoint_deriv in its float32 form.  The mask of a pair of modes is formed once for the cnt variables.  Pad columns zero.
__global__ void __launch_bounds__(256) k_adjoint_mu(SpecCoef c, AdjointKbars a, int cnt, float ks, cf *__restrict__ z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P / 2;
    const int hp = P >> 1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(p / hp), col = 2 * (int)(p - (size_t)row * hp);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d;
        const int j = ky0 + col;
        const bool in0 = j < c.hy, in1 = j + 1 < c.hy;
        const float m0 = in0 ? coef_mask(c, i, j) : 0.0f, m1 = in1 ? coef_mask(c, i, j + 1) : 0.0f;
        for (int k = 0; k < cnt; ++k) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in0) {
                const float4 kv = reinterpret_cast<const float4 *>(a.kb[k])[p];
                o.x = (kv.x * ks) * m0; o.y = (kv.y * ks) * m0;
                if (in1) { o.z = (kv.z * ks) * m1; o.w = (kv.w * ks) * m1; }
            }
            *reinterpret_cast<float4 *>(z + (size_t)k * fstride + 2 * p) = o;
        }
    }
}

// base: four real fields [4][n], n = nx * ny (a multiple of 4): u, v, zeta_x, zeta_y as the ROW_INV passes left them; mu: [CNT][n], the
// chunk's mu~_k; out: [CNT][4][n], u mu~_k, v mu~_k, zeta_x mu~_k, zeta_y mu~_k.  Each element of the base is read once and kept in
// registers while the CNT mu~ stream past; 16 bytes per lane and access over contiguous rows, no LDS, no atomics.
template <int CNT>
__global__ void __launch_bounds__(256) k_adjoint_prod_set(const float *__restrict__ base, const float *__restrict__ mu, float *__restrict__ out, size_t n)
{
    const size_t n4 = n / 4;
    const float4 *b = reinterpret_cast<const float4 *>(base), *q = reinterpret_cast<const float4 *>(mu);
    float4 *o = reinterpret_cast<float4 *>(out);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (size_t)gridDim.x * blockDim.x) {
        float4 v[4], m[CNT];
#pragma unroll
        for (int f = 0; f < 4; ++f) v[f] = b[(size_t)f * n4 + p];
#pragma unroll
        for (int k = 0; k < CNT; ++k) m[k] = q[(size_t)k * n4 + p];
#pragma unroll
        for (int k = 0; k < CNT; ++k)
#pragma unroll
            for (int f = 0; f < 4; ++f)
                o[((size_t)k * 4 + f) * n4 + p] = make_float4(v[f].x * m[k].x, v[f].y * m[k].y, v[f].z * m[k].z, v[f].w * m[k].w);
    }
}
