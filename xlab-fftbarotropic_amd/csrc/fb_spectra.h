// fb_spectra.h -- the shell spectra and cascade-flux record path (fb_model_get_spectra, fb_slab_get_spectra): energy and enstrophy
// spectra, the advective transfers and fluxes and the enstrophy dissipation per wavenumber shell, binned on the GPU.
//   k_spectra_deriv   the four derivative spectra of a stage (gradx zeta, grady zeta, grady psi, gradx psi) from the exported state;
//                     the backward x pass, the ROW_FUSED row pass without a source and the forward x pass follow: N = r2c(J)
//   k_spectra_gather  one workgroup per shell: lanes over i' = min(i, nx - i), each lane walks the short run of ky that lies in the
//                     shell's ring for its i' (rows i' and nx - i'), six float64 sums, reduced in a fixed order.  No atomics, no LDS
//                     table: the result repeats bit for bit from call to call.
//   k_spectra_table   the ranks' partial sums added in rank order, the table [nshells][10] (include/fftbaro.h), the two fluxes as
//                     running sums in shell order
// No reference counterpart.  The transfer is advective only: the source term's input is not part of it.
#pragma once

enum { SPEC_COLS = 10, SPEC_SUMS = 6, SPEC_SCAN = 2048 };

// wavenumbers in float64 from the context's float32 lengths: kx = 2 pi i' / Lx, ky = 2 pi j / Ly, dk = 2 pi / max(Lx, Ly)
struct SpecGrid {
    double lx, ly, dk;
    int nx, ny, hy;
};

__host__ __device__ static inline SpecGrid spec_grid(int nx, int ny, float lx, float ly)
{
#pragma clang fp contract(off)
    SpecGrid g;
    g.lx = (double)lx; g.ly = (double)ly; g.nx = nx; g.ny = ny; g.hy = ny / 2 + 1;
    g.dk = 6.283185307179586 / (g.lx > g.ly ? g.lx : g.ly);
    return g;
}
__host__ __device__ static inline double spec_k2(const SpecGrid &g, int ip, int j)
{
#pragma clang fp contract(off)
    const double kx = 6.283185307179586 * (double)ip / g.lx, ky = 6.283185307179586 * (double)j / g.ly;
    return kx * kx + ky * ky;
}
// shell of the mode (i', j): floor(sqrt(k^2) / dk + 0.5)
__host__ __device__ static inline int spec_shell(const SpecGrid &g, int ip, int j)
{
#pragma clang fp contract(off)
    return (int)floor(sqrt(spec_k2(g, ip, j)) / g.dk + 0.5);
}
// the corner mode (nx/2, ny/2) lies in the last shell
__host__ __device__ static inline int spec_nshells(const SpecGrid &g) { return spec_shell(g, g.nx / 2, g.ny / 2) + 1; }

// From one column group's state (3-pass private layout in `zin`, local column j holds ky = ky0 + j) into the fields 0..3 of `z`,
// fstride apart, what a stage of the step hands to its row pass (k_col_mid): gradx(vort_c), grady(vort_c), grady(psi_c), gradx(psi_c)
// with psi_c = invertLaplacian(vort_c); pad columns zero.  Every column takes part, the frozen ones too.  zin may be field 0 of z:
// each element is read before it is written, by the same thread.  Same float32 forms as k_spec_op (no contraction).
__global__ void __launch_bounds__(256) k_spectra_deriv(SpecCoef c, const cf *zin, cf *z, long fstride, int P, int N1, int N2, int ky0)
{
#pragma clang fp contract(off)
    const size_t total = (size_t)c.nx * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(idx / P), col = (int)(idx - (size_t)row * P);
        const int cc = row / N2, d = row - cc * N2, i = cc + N1 * d, j = ky0 + col;
        cf zx = cf_make(0.f, 0.f), zy = zx, py = zx, px = zx;
        if (j < c.hy) {
            const cf a = zin[idx];
            const float kx = c.gx[i], ky = c.gy[j];
            zx = cf_make(-a.y * kx, a.x * kx);                                      // fftwfop.cpp:87-94   (main.cpp:151)
            zy = cf_make(-a.y * ky, a.x * ky);                                      // fftwfop.cpp:96-103  (main.cpp:165)
            const float li = (i == 0 && j == 0) ? 1.0f : coef_lap(c, i, j);         // fftwfop.cpp:42-43,112-117 (main.cpp:179)
            const cf p = cf_make(a.x / li, a.y / li);
            py = cf_make(-p.y * ky, p.x * ky);                                      // main.cpp:198
            px = cf_make(-p.y * kx, p.x * kx);                                      // main.cpp:212
        }
        z[idx] = zx; z[idx + fstride] = zy; z[idx + 2 * fstride] = py; z[idx + 3 * fstride] = px;
    }
}

// a rank's column groups as the gather reads them: the state and N = r2c(J) (NULL for a group of frozen columns: every mode of
// it is masked), both in the 3-pass private layout with pitch ncols, local column 0 = ky0
struct SpecGroups {
    const cf *a[3], *nh[3];
    int ncols[3], ky0[3];
    int ng;
};

// smallest j in [0, hy] with spec_shell(i', j) >= b (the shell index is monotone in j); hy when there is none
FB_DEV int spec_first_j(const SpecGrid &g, int ip, int b)
{
#pragma clang fp contract(off)
    if (b <= 0) return 0;
    const double kx = 6.283185307179586 * (double)ip / g.lx, r = ((double)b - 0.5) * g.dk, t = r * r - kx * kx;
    int j = 0;
    if (t > 0.0) {
        const double e = sqrt(t) * g.ly / 6.283185307179586;
        j = e >= (double)g.hy ? g.hy : (int)e;
    }
    while (j > 0 && spec_shell(g, ip, j - 1) >= b) --j;         // the estimate is off by rounding at most: a step or two
    while (j < g.hy && spec_shell(g, ip, j) < b) ++j;
    return j;
}

// One workgroup of 256 per shell b = blockIdx.x.  Lane t takes i' = t, t + 256, ... <= nx/2; for each, the run [j0, j1) of ky in
// the shell, cut to each column group's columns, on the rows i' and (where it is another row) nx - i'.  Per mode, with G = nx ny,
// a = zeta_c / G, n = mask N / G, w = 1 for j = 0 and j = ny/2 else 2, all in float64 without contraction:
//   0 sum w   1 sum w |a|^2 / (2 k^2)   2 sum w |a|^2 / 2   3 sum w Re(conj(a) n) / k^2   4 sum w Re(conj(a) n)   5 sum mask nu k^2 w |a|^2
// (1 and 3 skip k = 0).  A lane adds its modes in a fixed order, the lanes of a wave are added by a butterfly, the four waves in
// order.  out[r * stride + 6 b + q] for r < copies (multi-GPU: the send buffer of the all-gather, one copy per peer).
__global__ void __launch_bounds__(256) k_spectra_gather(SpecGrid g, SpecGroups G, int N1, int N2, int gws_i, double nu, double *__restrict__ out,
                                                        int copies, size_t stride)
{
#pragma clang fp contract(off)
    __shared__ double sm[4][SPEC_SUMS];
    const int b = blockIdx.x;
    const double grids = (double)g.nx * (double)g.ny;
    double acc[SPEC_SUMS];
#pragma unroll
    for (int q = 0; q < SPEC_SUMS; ++q) acc[q] = 0.0;
    for (int ip = threadIdx.x; ip <= g.nx / 2; ip += blockDim.x) {
        const int j0 = spec_first_j(g, ip, b), j1 = spec_first_j(g, ip, b + 1);
        if (j0 >= j1) continue;
        const int nrows = (ip == 0 || 2 * ip == g.nx) ? 1 : 2;
        for (int q = 0; q < G.ng; ++q) {
            const int c0 = j0 > G.ky0[q] ? j0 : G.ky0[q];
            int c1 = G.ky0[q] + G.ncols[q];
            c1 = c1 < j1 ? c1 : j1;
            for (int r = 0; r < nrows; ++r) {
                const int i = r ? g.nx - ip : ip;
                const int cc = i % N1, d = i / N1;                                  // row N2 cc + d of the private layout holds kx = cc + N1 d
                const size_t base = (size_t)(N2 * cc + d) * G.ncols[q];
                for (int j = c0; j < c1; ++j) {
                    const size_t idx = base + (size_t)(j - G.ky0[q]);
                    const cf z = G.a[q][idx];
                    const double w = (j == 0 || 2 * j == g.ny) ? 1.0 : 2.0;
                    const double k2 = spec_k2(g, ip, j);
                    const double ar = (double)z.x / grids, ai = (double)z.y / grids;
                    const double wp = w * (ar * ar + ai * ai);
                    acc[0] += w;
                    acc[2] += wp / 2.0;
                    if (k2 > 0.0) acc[1] += wp / (2.0 * k2);
                    const bool live = ip * ip + j * j < gws_i;                     // the dealiasing mask (coef_mask)
                    if (live && G.nh[q]) {
                        const cf h = G.nh[q][idx];
                        const double nr = (double)h.x / grids, ni = (double)h.y / grids;
                        const double t = w * (ar * nr + ai * ni);
                        acc[4] += t;
                        if (k2 > 0.0) acc[3] += t / k2;
                        acc[5] += nu * k2 * wp;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SPEC_SUMS; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < SPEC_SUMS; ++q) sm[wv][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < SPEC_SUMS) {
        const int q = threadIdx.x;
        const double s = ((sm[0][q] + sm[1][q]) + sm[2][q]) + sm[3][q];
        for (int r = 0; r < copies; ++r) out[(size_t)r * stride + (size_t)b * SPEC_SUMS + q] = s;
    }
}

// one workgroup of 256: part[world][nshells][6] added in rank order -> table[nshells][10]:
//   0 k_lo = max(b - 0.5, 0) dk   1 k_hi = (b + 0.5) dk   2 n   3 E   4 Z   5 T_E   6 T_Z   7 Pi_E = -sum_{b' <= b} T_E   8 Pi_Z likewise   9 D_Z
// The running sums go from shell 0 upwards one shell at a time (what numpy's cumsum does), SPEC_SCAN shells at a time through LDS:
// lane 0 carries Pi_E, lane 64 Pi_Z.  No contraction.
__global__ void __launch_bounds__(256) k_spectra_table(const double *__restrict__ part, int world, int nshells, double dk, double *__restrict__ table)
{
#pragma clang fp contract(off)
    __shared__ double st[2][SPEC_SCAN];
    for (int b = threadIdx.x; b < nshells; b += blockDim.x) {
        double s[SPEC_SUMS];
#pragma unroll
        for (int q = 0; q < SPEC_SUMS; ++q) s[q] = 0.0;
        for (int r = 0; r < world; ++r) {
#pragma unroll
            for (int q = 0; q < SPEC_SUMS; ++q) s[q] += part[((size_t)r * nshells + b) * SPEC_SUMS + q];
        }
        double *row = table + (size_t)b * SPEC_COLS;
        row[0] = (b > 0 ? (double)b - 0.5 : 0.0) * dk;
        row[1] = ((double)b + 0.5) * dk;
        row[2] = s[0]; row[3] = s[1]; row[4] = s[2]; row[5] = s[3]; row[6] = s[4]; row[9] = s[5];
    }
    __syncthreads();
    double run = 0.0;                                            // (lanes 0 and 64 only)
    for (int b0 = 0; b0 < nshells; b0 += SPEC_SCAN) {
        const int nb = nshells - b0 < SPEC_SCAN ? nshells - b0 : SPEC_SCAN;
        for (int k = threadIdx.x; k < nb; k += blockDim.x) {
            st[0][k] = table[(size_t)(b0 + k) * SPEC_COLS + 5];
            st[1][k] = table[(size_t)(b0 + k) * SPEC_COLS + 6];
        }
        __syncthreads();
        if (threadIdx.x == 0 || threadIdx.x == 64) {
            double *v = st[threadIdx.x >> 6];
            for (int k = 0; k < nb; ++k) { run += v[k]; v[k] = -run; }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < nb; k += blockDim.x) {
            table[(size_t)(b0 + k) * SPEC_COLS + 7] = st[0][k];
            table[(size_t)(b0 + k) * SPEC_COLS + 8] = st[1][k];
        }
        __syncthreads();
    }
}
