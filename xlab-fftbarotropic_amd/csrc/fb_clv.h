// fb_clv.h -- the kernel of the covariant Lyapunov vectors (fb_model_tangent_combine, fb_slab_tangent_combine; host side: fb_beside_tangent.h,
// tangent_combine, beside tangent_qr).
//
// Ginelli's algorithm keeps the orthonormal bases Q_n of a window of QR intervals (the basis tape, fb_model::tt: copies of the
// perturbations' bases, device to device, no kernel) and forms V_n = Q_n C_n with a small upper triangular C_n that the host gets from
// the factors R_n by a backward recursion.  The product is M linear combinations of M half spectra; k_tangent_combine forms all M of
// them in one pass, so that every source is read once and every destination written once whatever C holds.
// No reference counterpart: the reference has no tangent-linear model.
#pragma once

// the M sources and the M destinations of one column group, by value in the kernel's arguments: a compile-time index picks a pointer
template <int MB> struct CombineArrays { const cf *src[MB]; cf *dst[MB]; };

// dst_j = sum over i < M of c[i][j] src_i for every j < M at once, over a whole column group (n complex, a multiple of 16: pad columns
// stay zero, a sum of zeros); M <= MB, the loops fully unrolled over the compile-time bound MB with a wave-uniform test of i, j < M, so
// that the inputs live in registers.  Two modes (16 bytes) per lane and array.  A lane loads its M inputs before it stores any output
// and touches no other element: src may be dst (the live set combined in place), so neither is __restrict__.  c: [M][M] float64
// row-major on the device, every element at a wave-uniform address.  Each output element is summed in float64 in ascending i, products
// and sums not contracted, and rounded once to float32, as k_tangent_axpy rounds.
template <int MB> __global__ void __launch_bounds__(256) k_tangent_combine(CombineArrays<MB> a, size_t n, int M, const double *__restrict__ c)
{
#pragma clang fp contract(off)
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n / 2; p += (size_t)gridDim.x * blockDim.x) {
        float4 q[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i)
            if (i < M) q[i] = reinterpret_cast<const float4 *>(a.src[i])[p];
#pragma unroll
        for (int j = 0; j < MB; ++j) {
            if (j < M) {
                double x = c[j] * (double)q[0].x, y = c[j] * (double)q[0].y, z = c[j] * (double)q[0].z, w = c[j] * (double)q[0].w;
#pragma unroll
                for (int i = 1; i < MB; ++i) {
                    if (i < M) {
                        const double cij = c[i * M + j];
                        x += cij * (double)q[i].x; y += cij * (double)q[i].y; z += cij * (double)q[i].z; w += cij * (double)q[i].w;
                    }
                }
                reinterpret_cast<float4 *>(a.dst[j])[p] = make_float4((float)x, (float)y, (float)z, (float)w);
            }
        }
    }
}
