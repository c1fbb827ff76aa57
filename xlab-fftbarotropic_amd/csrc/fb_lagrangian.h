// fb_lagrangian.h -- kernels of the adjoint of the particle step (fb_model_particle_tape, fb_model_set_particle_adjoint,
// fb_model_get_particle_adjoint and what fb_model_adjoint_back runs while a particle adjoint is set; their fb_slab_* twins on one rank;
// host side: fb_beside_particles.h, lagrangian_*).
//
// The particles of fb_particles.h are advanced by  x0 = X, x1 = X + dt/2 k1, x2 = X + dt/2 k2, x3 = X + dt k3,  k_{s+1} = U_s(x_s),
// X' = X + dt/6 (k1 + 2 k2 + 2 k3 + k4), U_s the interpolated velocity of the vorticity's state of stage s.  With Xb the gradient of a
// scalar with respect to the particles' positions and A_s = grad U_s(x_s) = [[u_x, u_y], [v_x, v_y]] (pt_gather_grad; on a cell face
// the cell to the right), the transpose of that step takes the stages in the order 3, 2, 1, 0, as the field's sweep does:
//   p = dt/6 Xb;            q = A_3^T p; acc = Xb + q
//   p = dt/3 Xb + dt q;     q = A_2^T p; acc += q
//   p = dt/3 Xb + dt/2 q;   q = A_1^T p; acc += q
//   p = dt/6 Xb + dt/2 q;   q = A_0^T p; Xb <- acc + q            A^T p = (u_x p_x + v_x p_y, u_y p_x + v_y p_y)
// and p, the gradient with respect to the stage's interpolated velocity, forces the adjoint of the stage state: the transpose of the
// interpolation spreads p_x and p_y at x_s onto the grid (S_u, S_v), and the transposes of c2r and of the multipliers of u and v add
//   ( i ky r2c(S_u) - i kx r2c(S_v) ) / lap     ((0, 0): / 1)
// to the stage's `a` of fb_adjoint.h.  k_adjoint_update forms (gradx(z3) - grady(z2)) / lap from the spectra of zeta_y mu~ (z3) and
// zeta_x mu~ (z2) already: S_u is subtracted from the real field zeta_x mu~ and S_v from zeta_y mu~ before their ROW_FWD passes, and
// the forcing rides on the transforms that are run anyway.  The particles do not act on the flow: Xb never depends on lam.  Per stage:
//   k_particle_adjoint  p, q and the recurrences of every particle, after the five ROW_INV passes: u and v are the real fields 1 and
//                       2 of the stage, which k_adjoint_prod then overwrites
//   (k_obs_wmax of p_x and of p_y: fb_obs.h)
//   k_scatter_pair      the transpose of the interpolation for both components at once: the sixteen cells and weights of a particle
//                       are formed once, into two fixed-point accumulators of fb_obs.h's kind (two 64-bit limbs per cell each)
//   k_scatter_fold      every cell of the two product fields minus its accumulator, rounded to float32 once; the limbs are zeroed
// Integer atomics only: the product fields, lam and Xb are the same bits in any order of the particles and of the atomics.
// The state is SoA: eight float64 arrays of n (Xb x, y; p x, y; q x, y; acc x, y).
// No reference counterpart: the reference follows no particles.
#pragma once

// [n][2] float64 (x, y) -> the first two arrays of the adjoint state, the other six zero
__global__ void __launch_bounds__(256) k_particle_adjoint_in(const double *__restrict__ xb, double *__restrict__ pa, int n)
{
    const size_t N = (size_t)n;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
        pa[p] = xb[2 * p]; pa[N + p] = xb[2 * p + 1];
#pragma unroll
        for (int e = 2; e < 8; ++e) pa[e * N + p] = 0.0;
    }
}

// One backward RK stage of every particle, one thread per particle (grid-stride).  xs: the positions the forward stage started from
// (a slot of the particle tape, [n][2]); u, v: the stage's velocity as real fields.  The same thirty-two loads as k_particle_stage_def.
// A particle whose position is not finite reads nothing; its p, as a p that is not finite, becomes NaN in both components, and with
// it q and Xb.
template <int STAGE>
__global__ void __launch_bounds__(256) k_particle_adjoint(PartGeo g, const float *__restrict__ u, const float *__restrict__ v, const double *__restrict__ xs,
                                                          double *__restrict__ pa, int n, double dt)
{
#pragma clang fp contract(off)
    const size_t N = (size_t)n;
    double *bx = pa, *by = pa + N, *px = pa + 2 * N, *py = pa + 3 * N, *qx = pa + 4 * N, *qy = pa + 5 * N, *ax = pa + 6 * N, *ay = pa + 7 * N;
    const double c_b = (STAGE == 3 || STAGE == 0) ? dt / 6.0 : dt / 3.0;       // this stage's p: its share of Xb
    const double c_q = STAGE == 2 ? dt : dt / 2.0;                              // ... and of the q of the stage before (none at stage 3)
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (size_t)gridDim.x * blockDim.x) {
        const double x = xs[2 * p], y = xs[2 * p + 1];
        const double b0 = bx[p], b1 = by[p];
        double p0 = c_b * b0, p1 = c_b * b1;
        if (STAGE != 3) { p0 = p0 + c_q * qx[p]; p1 = p1 + c_q * qy[p]; }
        int ix[4], jy[4];
        double wx[4], wy[4], dwx[4], dwy[4];
        double a11 = __builtin_nan(""), a12 = a11, a21 = a11, a22 = a11;
        const bool okx = pt_axis(x, g.dx, g.nx, ix, wx, dwx), oky = pt_axis(y, g.dy, g.ny, jy, wy, dwy);
        if (okx && oky) {
            (void)pt_gather_grad(u, g.ny, ix, wx, dwx, jy, wy, dwy, g.dx, g.dy, &a11, &a12);
            (void)pt_gather_grad(v, g.ny, ix, wx, dwx, jy, wy, dwy, g.dx, g.dy, &a21, &a22);
        }
        // a particle whose position or p is not finite deposits nothing and counts for nothing in max |p|: both components NaN
        if (!(okx && oky) || !__builtin_isfinite(p0) || !__builtin_isfinite(p1)) p0 = p1 = __builtin_nan("");
        const double q0 = a11 * p0 + a21 * p1, q1 = a12 * p0 + a22 * p1;
        px[p] = p0; py[p] = p1;
        if (STAGE == 3) { ax[p] = b0 + q0; ay[p] = b1 + q1; qx[p] = q0; qy[p] = q1; }
        else if (STAGE != 0) { ax[p] = ax[p] + q0; ay[p] = ay[p] + q1; qx[p] = q0; qy[p] = q1; }
        else { bx[p] = ax[p] + q0; by[p] = ay[p] + q1; }
    }
}

// The transpose of the interpolation for the two components of p at the positions xs [n][2]: cell [ix[a]][jy[b]] of accumulator c
// (c = 0: p_x, c = 1: p_y) += p_c wx[a] wy[b] 2^e, as k_scatter adds it (the floor into the high limb, the fraction in units of
// 2^-OBS_FRAC into the low one).  acc: [2][2][cells] (component, limb, cell); head[0]: the bits of max(|p_x|, |p_y|) over the finite
// ones (k_obs_wmax of both), so that one exponent serves both accumulators and neither can overflow.  A particle whose position is
// not finite deposits nothing, and a component that is not finite deposits nothing.  Every index pt_axis returns lies in [0, n) of
// its axis, so every cell lies in [0, cells), cells = nx * ny.
__global__ void __launch_bounds__(256) k_scatter_pair(PartGeo g, const double *__restrict__ xs, const double *__restrict__ px, const double *__restrict__ py, int n,
                                                      unsigned long long *__restrict__ acc, size_t cells, const unsigned long long *__restrict__ head)
{
#pragma clang fp contract(off)
    const int e = obs_exponent(head, n);
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < (size_t)n; p += (size_t)gridDim.x * blockDim.x) {
        const double qx = xs[2 * p], qy = xs[2 * p + 1];
        const double w[2] = {px[p], py[p]};
        int ix[4], jy[4];
        double wx[4], wy[4];
        const bool okx = pt_axis(qx, g.dx, g.nx, ix, wx), oky = pt_axis(qy, g.dy, g.ny, jy, wy);
        if (!(okx && oky)) continue;
        const bool fin[2] = {(bool)__builtin_isfinite(w[0]), (bool)__builtin_isfinite(w[1])};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double ww = wx[a] * wy[b];
                const size_t cell = (size_t)ix[a] * g.ny + jy[b];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!fin[c]) continue;
                    const double x = ldexp(w[c] * ww, e);                                // |x| < 2^62 / n
                    const double fl = __builtin_floor(x);
                    const long long hi = (long long)fl;
                    const unsigned long long lo = (unsigned long long)__double2ll_rn(ldexp(x - fl, OBS_FRAC));   // x - fl in [0, 1), exact
                    unsigned long long *dst = acc + (size_t)c * 2 * cells + cell;
                    if (hi != 0) atomicAdd(dst, (unsigned long long)hi);                 // (two's complement: a signed sum)
                    if (lo != 0) atomicAdd(dst + cells, lo);
                }
            }
        }
    }
}

// fu[i] -= S_u[i], fv[i] -= S_v[i] over the cells: the accumulator's value as k_scatter_round forms it, in float64, the difference
// rounded to float32 once.  A cell that nothing was added to keeps its bits, and every limb that is not zero is zeroed for the next stage.
__global__ void __launch_bounds__(256) k_scatter_fold(unsigned long long *__restrict__ acc, const unsigned long long *__restrict__ head, int n, float *__restrict__ fu,
                                                      float *__restrict__ fv, size_t cells)
{
#pragma clang fp contract(off)
    const int e = obs_exponent(head, n);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            unsigned long long *a = acc + (size_t)c * 2 * cells;
            const unsigned long long h = a[i], lo = a[cells + i];
            if (h == 0 && lo == 0) continue;
            const long long hi = (long long)h + (long long)(lo >> OBS_FRAC);
            const double fr = ldexp((double)(lo & ((1ull << OBS_FRAC) - 1)), -OBS_FRAC);
            const double s = ldexp((double)hi + fr, -e);
            float *f = c ? fv : fu;
            f[i] = (float)((double)f[i] - s);
            if (h != 0) a[i] = 0;
            if (lo != 0) a[cells + i] = 0;
        }
    }
}
