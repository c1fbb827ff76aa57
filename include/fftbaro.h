/*
 * fftbaro.h -- C ABI of the MI355X-native pseudospectral barotropic-vorticity engine.
 *
 * Drop-in boundary for the hot path of meteorologytoday/XLab-FFTBarotropic: every entry
 * point below names the reference interface it replaces (paths relative to the reference
 * root).  Plain pointers and sizes only; no C++/torch types.  All `float *` arguments named
 * d_* are DEVICE pointers (HIP); spectra are interleaved (re,im) float32 in the reference's
 * half-spectrum layout HIDX(i,j) = (ny/2+1)*i + j (configuration.hpp:32), real fields are
 * IDX(i,j) = ny*i + j (configuration.hpp:31).
 *
 * Every function returns an int status (FB_OK == 0); the reference's methods are `void` with
 * no error path (fftwfop.hpp:20-24) -- see INTEGRATION.md for the binding a maintainer adds.
 * Work is enqueued on the context's HIP stream (default: the null stream); functions do not
 * synchronise unless stated.
 *
 * There is NO CPU fallback: when no HIP device is usable fb_create fails with FB_EHIP.
 */
#ifndef FFTBARO_H
#define FFTBARO_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK            0
#define FB_EINVAL        1   /* bad argument (null pointer, unsupported size, ...) */
#define FB_ENOMEM        2   /* host or device allocation failed                  */
#define FB_EHIP          3   /* HIP runtime error; see fb_last_error()            */
#define FB_EIO           4   /* file open / short read / short write              */
#define FB_EUNSUPPORTED  5   /* grid size not supported by the kernels            */

const char *fb_strerror(int status);
const char *fb_last_error(void);          /* thread-local detail of the last failure */
int fb_version(void);                      /* 100*major + minor                       */
/* one process per GPU: pick this process's (this thread's) device before creating a context; hipGetDeviceCount / hipSetDevice */
int fb_device_count(int *count);
int fb_set_device(int ordinal);
/* 1 if (nx,ny) is supported: each a power of two in [64, 16384] or 3*2^k in [192, 3072]
 * (the reference's default NPTS = 768, configuration.hpp:18) */
int fb_size_supported(int nx, int ny);

/* ---------------------------------------------------------------------------------------
 * Context = operator tables + FFT plans.
 * Replaces: fftwf_operation<XPTS,YPTS>::fftwf_operation(Lx,Ly) / ~fftwf_operation()
 *           (fftwfop.hpp:18-19, fftwfop.cpp:5-85) and the eight fftwf_plan_dft_{r2c,c2r}_2d
 *           calls of main.cpp:126-135.  Grid size is a run-time argument here
 *           (configuration.hpp:18-21 fixes it at compile time).
 * ------------------------------------------------------------------------------------- */
typedef struct fb_ctx fb_ctx;
int fb_create(fb_ctx **out, int nx, int ny, float lx, float ly);
int fb_destroy(fb_ctx *ctx);
int fb_set_stream(fb_ctx *ctx, void *hip_stream);     /* hipStream_t; NULL = null stream */
int fb_synchronize(fb_ctx *ctx);                       /* hipStreamSynchronize            */
/* copies the five coefficient tables to HOST buffers (any may be NULL): gradx_coe[nx],
 * grady_coe[ny/2+1], laplacian_coe / laplacian_coe_inverse / dealiasing_mask [nx*(ny/2+1)]
 * (fftwfop.cpp:15-68; the debug print of :26-36,70-77) */
int fb_get_tables(fb_ctx *ctx, float *gradx_coe, float *grady_coe, float *laplacian_coe,
                  float *laplacian_coe_inverse, float *dealiasing_mask);

/* ---------------------------------------------------------------------------------------
 * Buffers.  Replaces fftwf_malloc / fftwf_free (main.cpp:103-123) with device memory.
 * ------------------------------------------------------------------------------------- */
int fb_malloc(void **d_ptr, size_t bytes);
int fb_free(void *d_ptr);
int fb_memcpy_h2d(fb_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);  /* synchronous */
int fb_memcpy_d2h(fb_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);  /* synchronous */
int fb_memset0(fb_ctx *ctx, void *d_dst, size_t bytes);

/* Asynchronous record path (no reference counterpart: main.cpp:266-282 writes synchronously from its only
 * thread).  Pinned host buffers, non-blocking streams and events as opaque handles, so that a C/C++ host can
 * overlap the D2H copies and the file writes of a record step with the following RK4 steps:
 *   compute stream: fb_model_get_vort/diag -> fb_event_record(e1, compute)
 *   copy stream   : fb_stream_wait_event(copy, e1) -> fb_memcpy_d2h_async(copy, ...) -> fb_event_record(e2, copy)
 *   writer thread : fb_event_synchronize(e2) -> fb_write_field(...)                (host/barotropic_main.cpp) */
int fb_malloc_host(void **h_ptr, size_t bytes);
int fb_free_host(void *h_ptr);
int fb_stream_create(void **stream);                 /* hipStreamNonBlocking; pass to fb_set_stream */
int fb_stream_destroy(void *stream);
int fb_stream_synchronize(void *stream);
int fb_event_create(void **event);
int fb_event_destroy(void *event);
int fb_event_record(void *event, void *stream);
int fb_stream_wait_event(void *stream, void *event);
int fb_event_synchronize(void *event);
/* events that carry a time stamp, and the GPU time between two of them once both have fired: how the drop-in driver prices its
 * step loop (steps/s without the record steps' stalls) without synchronising it */
int fb_event_create_timing(void **event);
int fb_event_elapsed_ms(void *start, void *stop, float *ms);
int fb_memcpy_d2h_async(void *stream, void *h_dst, const void *d_src, size_t bytes);
/* the other direction, for the FIFO source (main-shallow-water.cpp:304: a reader thread fills a pinned buffer, the copy
 * stream carries it to the device, the compute stream waits for the copy's event before fb_model_set_source) */
int fb_memcpy_h2d_async(void *stream, void *d_dst, const void *h_src, size_t bytes);

/* ---------------------------------------------------------------------------------------
 * Spectral operators on device half spectra (nx*(ny/2+1) complex).  in == out is allowed
 * (main-shallow-water.cpp:327, invert_pres.cpp:148-150).
 * Replaces fftwf_operation::gradx/grady/laplacian/invertLaplacian/dealiase
 * (fftwfop.hpp:20-24, fftwfop.cpp:87-124).  Bit-exact with the reference's float32 forms.
 * ------------------------------------------------------------------------------------- */
int fb_gradx(fb_ctx *ctx, const float *d_in, float *d_out);
int fb_grady(fb_ctx *ctx, const float *d_in, float *d_out);
int fb_laplacian(fb_ctx *ctx, const float *d_in, float *d_out);
int fb_invert_laplacian(fb_ctx *ctx, const float *d_in, float *d_out);
int fb_dealiase(fb_ctx *ctx, const float *d_in, float *d_out);

/* ---------------------------------------------------------------------------------------
 * 2-D FFTs.  Replaces fftwf_execute() on the r2c / c2r plans (main.cpp:154,168,186,200,214,
 * 237,256,275).  Unnormalised, r2c sign -, c2r sign +; c2r accepts non-Hermitian input with
 * FFTW's semantics (SURVEY.md note N2) and -- unlike FFTW -- preserves its input, so the
 * copy_for_c2r dance of main.cpp:273,281 is unnecessary (harmless if kept).
 * fb_c2r with normalize != 0 also applies fftwf_backward_normalize (main.cpp:37-41).
 * ------------------------------------------------------------------------------------- */
int fb_r2c(fb_ctx *ctx, const float *d_in_real, float *d_out_spec);
int fb_c2r(fb_ctx *ctx, const float *d_in_spec, float *d_out_real, int normalize);

/* ---------------------------------------------------------------------------------------
 * Pointwise sweeps the reference driver does in its lambdas.
 * ------------------------------------------------------------------------------------- */
/* data[i] /= GRIDS                                   fftwf_backward_normalize, main.cpp:37-41 */
int fb_backward_normalize(fb_ctx *ctx, float *d_real);
/* data[i] = -data[i]                                 main.cpp:201                            */
int fb_negate(fb_ctx *ctx, float *d_real);
/* out = -u*dzdx - v*dzdy + src (src NULL = 0)        main.cpp:225-227                        */
int fb_jacobian(fb_ctx *ctx, const float *d_u, const float *d_v, const float *d_dzdx,
                const float *d_dzdy, const float *d_src, float *d_out);
/* acc += x * a   on spectra                          main.cpp:240-243 (viscous add)          */
int fb_spec_axpy(fb_ctx *ctx, float *d_acc, const float *d_x, float a);
/* out = base + rk * a  on spectra                    evolve(), main.cpp:246-251              */
int fb_spec_evolve(fb_ctx *ctx, const float *d_base, const float *d_rk, float a, float *d_out);
/* out = base + (k1 + 2 k2 + 2 k3 + k4) * dt / 6      main.cpp:309-312                        */
int fb_spec_rk4_combine(fb_ctx *ctx, const float *d_base, const float *d_k1, const float *d_k2,
                        const float *d_k3, const float *d_k4, float dt, float *d_out);

/* ---------------------------------------------------------------------------------------
 * Fused RK4 model: the hot loop of main.cpp:259-323 / main-shallow-water.cpp:277-338 with
 * the state resident in HBM.  One fb_model_step() == one iteration of the reference's step
 * loop body without the record path (a13-a15 of SURVEY.md section 8 fused into the FFT passes).
 * ------------------------------------------------------------------------------------- */
typedef struct fb_model fb_model;
int fb_model_create(fb_model **out, fb_ctx *ctx, float nu, float dt);      /* NU, dt: configuration.hpp:17,34 */
int fb_model_destroy(fb_model *m);
/* readField + fftwf_execute(p_fwd_vort)              main.cpp:143-144,256 */
int fb_model_set_vort(fb_model *m, const float *d_vort_real);
/* vort_src (device real field, copied; NULL = zeros) main.cpp:110,226; refreshed per step by
 * VortSrcRecipeReader::read in main-shallow-water.cpp:304 */
int fb_model_set_source(fb_model *m, const float *d_src_real);
int fb_model_step(fb_model *m, int nsteps);
/* enable != 0: fb_model_step replays one captured RK4 step as a hipGraph (16 kernel launches per step are
 * launch-bound on small grids).  Needs a non-null context stream (fb_set_stream); otherwise steps run eagerly. */
int fb_model_use_graph(fb_model *m, int enable);
/* record path: c2r of a copy of vort_c + normalise   main.cpp:273-281 */
int fb_model_get_vort(fb_model *m, float *d_vort_real);
/* stage-0 record dumps psi, u, v (any may be NULL)   main.cpp:181-222 */
int fb_model_get_diag(fb_model *m, float *d_psi, float *d_u, float *d_v);
/* Okubo-Weiss record output (no reference counterpart; its README names the filamentation time, Rozoff et al. 2006), device
 * [nx][ny] outputs, either may be NULL (both NULL: FB_EINVAL).  From psi_c = invertLaplacian(vort_c) (fftwfop.cpp:112-117) and the
 * velocity u = -dpsi/dy, v = dpsi/dx of fb_model_get_diag:
 *   W = S1^2 + S2^2 - zeta^2 = 4 (psi_xy^2 - psi_xx psi_yy)  [s^-2],  S1 = u_x - v_y, S2 = v_x + u_y, zeta = v_x - u_y
 *   tau_fil = 2 / sqrt(W) [s] where W > 0, +inf where W <= 0 (never NaN)
 * Each second derivative is gradx/grady applied twice to psi_c, c2r'd and divided by GRIDS; every column takes part, the frozen
 * ones beyond the dealiasing circle too.  zeta here is the vorticity of (u, v): it lacks the domain-mean mode that the vorticity
 * record carries (a periodic psi has no mean, and a mean rotation is no strain).  Enqueued on the context stream, no
 * synchronisation; uses record buffers of its own (allocated on first use) and leaves the state and a captured step untouched. */
int fb_model_get_okubo_weiss(fb_model *m, float *d_w, float *d_tau);
/* Effective eddy diffusivity (Nakamura 1996; Hendricks and Schubert 2009; no reference counterpart, its README names the output)
 * with the vorticity as the tracer and kappa = nu.  zeta is the vorticity record (fb_model_get_vort, bit for bit), g = zeta_x^2 +
 * zeta_y^2 with zeta_x = c2r(gradx(vort_c))/GRIDS, zeta_y = c2r(grady(vort_c))/GRIDS (every column), in float32.  Bins: qmin, qmax =
 * float32 min / max of zeta; point -> b = floor(((double)q - qmin) * ((double)nbins / ((double)qmax - qmin))) clamped to
 * [0, nbins-1] (all in bin 0 when qmax == qmin).  d_table: device float64 [nbins][9], one row per bin, dQ = (qmax - qmin)/nbins,
 * dx = Lx/nx, dy = Ly/ny:
 *   0 Q_lo = qmin + b dQ   1 Q_hi = qmin + (b+1) dQ   2 n_b (points)   3 A_b = n_b dx dy [m^2]
 *   4 A_ge = sum over b' >= b of A_b' (area where zeta >= Q_lo, summed from the top bin down)   5 S_b = dx dy sum_bin g [s^-2]
 *   6 Le^2 = S_b A_b / dQ^2 [m^2] (0 where n_b = 0 or dQ = 0)   7 r_e = sqrt((A_ge - A_b/2)/pi) [m]
 *   8 K_eff = nu Le^2 / (4 pi^2 r_e^2) [m^2 s^-1] (0 where Le^2 = 0 or r_e = 0)
 * Area counts from the top (a cyclone); for other geometries renormalise Le^2 with a minimum length of your own.  d_zeta, d_grad2:
 * optional device [nx][ny] outputs of zeta and g (NULL: record buffers of the model's own).  nbins in [2, 4096], else FB_EINVAL, as
 * for a NULL model or table (checked before any HIP call).  Enqueued on the context stream, no synchronisation; leaves the state
 * and a captured step untouched. */
int fb_model_get_eddy_diffusivity(fb_model *m, int nbins, double *d_table, float *d_zeta, float *d_grad2);
/* Passive tracer (no reference counterpart): a second real [nx][ny] field c with a diffusivity kappa >= 0 of its own, carried along
 * by the model's flow.  fb_model_set_tracer takes the device field d_c_real in as fb_model_set_vort takes the vorticity (readField +
 * r2c, main.cpp:143-144,256) and keeps it as a half spectrum c_c; from then on every step advances c_c by the RK4 step of
 * main.cpp:288-317 beside vort_c, stage by stage: stage k uses psi_c = invertLaplacian(vort_c) of the vorticity's state of stage k,
 * u = -psi_y, v = psi_x as the vorticity's own stage k forms them, and
 *   tend_c = dealiase( r2c(-u c_x - v c_y) + kappa laplacian(c_c) ),  c_x = c2r(gradx c_c)/GRIDS, c_y = c2r(grady c_c)/GRIDS
 * in float32 with the forms of main.cpp:225-227 (no source), :240-243 (kappa for NU), :246-251, :309-312.  Modes outside the
 * dealiasing circle never change after fb_model_set_tracer, the mean mode is kept.  A tracer set to the vorticity with kappa = nu
 * follows the vorticity.  One tracer per model; d_c_real == NULL removes it and frees its state.  The vorticity, its step and every
 * other record are bit for bit what they are without a tracer; fb_model_set_vort leaves the tracer in place.  A captured step
 * (fb_model_use_graph) is dropped and captured again with the tracer's stages.  fb_model_get_tracer: the tracer as fb_model_get_vort
 * returns the vorticity.  fb_model_get_tracer_eddy_diffusivity: fb_model_get_eddy_diffusivity of the tracer, kappa in the place of
 * nu in column 8 (d_c, d_grad2: optional outputs of c and |grad c|^2).  FB_EINVAL before any HIP call: NULL model, kappa negative
 * or not finite, a get without a tracer set, and what fb_model_get_eddy_diffusivity rejects.  Enqueued on the context stream, no
 * synchronisation. */
int fb_model_set_tracer(fb_model *m, const float *d_c_real, float kappa);   /* NULL: remove the tracer */
int fb_model_get_tracer(fb_model *m, float *d_c_real);
int fb_model_get_tracer_eddy_diffusivity(fb_model *m, int nbins, double *d_table, float *d_c, float *d_grad2);
/* Lagrangian particles (no reference counterpart): n points (x, y) [m] on the doubly periodic domain, float64 and UNWRAPPED (a particle
 * that leaves through one side keeps counting; positions are wrapped only where they index a field).  Grid point (i, j) of an
 * [nx][ny] field lies at x = i dx, y = j dy, dx = (double)Lx / nx, dy = (double)Ly / ny (the context's float32 lengths, widened, as
 * fb_model_get_azimuthal takes its centre).  From fb_model_set_particles on every step advances the particles by the RK4 step of
 * main.cpp:288-317 beside vort_c, coupled stage by stage:
 *   k1 = U_0(X0), k2 = U_1(X0 + dt/2 k1), k3 = U_2(X0 + dt/2 k2), k4 = U_3(X0 + dt k3), X <- X0 + dt/6 (k1 + 2 k2 + 2 k3 + k4)
 * with U_s = (u, v) of the vorticity's state of stage s (vort_c0 at stage 0, the stage state afterwards: the state the tracer's
 * stage s uses), two float32 [nx][ny] fields formed as fb_model_get_diag forms u and v, in its kernels and its rounding; everything
 * from the interpolation on is float64.  The interpolation is the tensor product of 4-point cubic Lagrange polynomials: per axis
 * s = x / dx, i0 = floor(s) (a 64-bit integer), t = s - i0, the rows (i0 - 1 .. i0 + 2) mod nx as a non-negative modulus (positions
 * many domain lengths away, on either side, index correctly) with the weights
 *   w(-1) = -t (t-1) (t-2) / 6,  w(0) = (t+1) (t-1) (t-2) / 2,  w(1) = -(t+1) t (t-2) / 2,  w(2) = (t+1) t (t-1) / 6,
 * so that a particle on a grid point gets the grid value.  A position that is not finite reads nothing and stays NaN.
 * fb_model_set_particles: d_xy device float64 [n][2], n in [1, 2^24]; d_xy == NULL (with n == 0) removes the particles and frees
 * their state.  fb_model_get_particles: the unwrapped positions, [n][2].  fb_model_particle_count: n, 0 when none are set.
 * fb_model_sample: the same interpolation of ANY device [nx][ny] float32 field (zeta, the tracer, W, the pressure ...) at any n
 * positions d_xy [n][2] into d_out, float64 [n]; it needs no particles set and does not touch them.  The vorticity, a tracer and
 * every record are bit for bit what they are without particles.  Setting or removing particles drops a captured step
 * (fb_model_use_graph); it is captured again with the particles' stages.  FB_EINVAL before any HIP call: a NULL model, n outside
 * [1, 2^24], NULL positions with n > 0, a NULL field or output, fb_model_get_particles without particles set.  Enqueued on the
 * context stream, no synchronisation, no host round trip. */
int fb_model_set_particles(fb_model *m, const double *d_xy, int n);        /* NULL: remove the particles */
int fb_model_get_particles(fb_model *m, double *d_xy);
int fb_model_particle_count(fb_model *m, int *n);
int fb_model_sample(fb_model *m, const float *d_field, const double *d_xy, int n, double *d_out);
/* The deformation gradient along the particles and the finite-time Lyapunov exponent (no reference counterpart).  Every particle
 * carries F = dX(t) / dX(t0), float64 (F11, F12, F21, F22), advanced in every step by the linearisation of the particle's own RK4 step:
 *   K1 = A_0(X0) F0, K2 = A_1(X0 + dt/2 k1) (F0 + dt/2 K1), K3 = A_2(X0 + dt/2 k2) (F0 + dt/2 K2), K4 = A_3(X0 + dt k3) (F0 + dt K3),
 *   F <- F0 + dt/6 (((K1 + 2 K2) + 2 K3) + K4)
 * with A_s(X) = [[du/dx, du/dy], [dv/dx, dv/dy]] the gradient of the INTERPOLANT of the stage's u, v at X, from the stencils the
 * position update reads: on each axis the value weights w or their derivatives over the spacing,
 *   w'(-1) = -(3t^2 - 6t + 2) / 6,  w'(0) = (3t^2 - 4t - 1) / 2,  w'(1) = -(3t^2 - 2t - 2) / 2,  w'(2) = (3t^2 - 1) / 6.
 * So F is the exact Jacobian of the discrete map X0 -> X in the given flow wherever that map is differentiable: the cubic Lagrange
 * interpolant is continuous, its derivative jumps at cell faces, and at t == 0 the derivative of the cell to the right is taken.  det F
 * is close to 1 and not equal to it (the interpolated velocity is not exactly non-divergent): not a defect.  A particle whose
 * position is not finite gets NaN in F.  The positions, the vorticity, a tracer and the tangent are bit for bit what they are without.
 * fb_model_set_particle_deformation: on == 1 allocates twelve float64 arrays of n where needed, sets F = I and the elapsed time to 0
 * (so it is the reset too: F grows like exp(lambda t)); on == 0 frees; any other value is refused.  Either way a captured step is
 * dropped as fb_model_set_particles drops it.  fb_model_set_particles (a new set or NULL) and fb_model_destroy switch it off.
 * fb_model_get_particle_deformation: F into d_F, device float64 [n][4]; *elapsed (host, may be NULL): (steps since the reset) x dt [s].
 * fb_model_particle_stretching: the closed-form singular value decomposition of every matrix of d_F, device float64 [n][4], n in
 * [1, 2^24] (ANY matrices, as fb_model_sample takes any positions), or with d_F == NULL of the model's own F and n, into d_out,
 * device float64 [n][4] with the columns
 *   ln sigma1, ln sigma2, theta_in, theta_out:  F = Rot(theta_out) diag(sigma1, sign(det F) sigma2) Rot(theta_in)^T up to the overall
 * sign, sigma1 >= sigma2 >= 0, both angles folded into (-pi/2, pi/2] (they name axes): theta_in is the direction of strongest
 * stretching at the initial time, theta_out its image, ln sigma1 / elapsed the forward finite-time Lyapunov exponent.  F is scaled by
 * its largest |entry| first and sigma2 = |det| / sigma1; the zero matrix gives -inf, -inf, 0, 0, a singular one ln sigma2 = -inf, an
 * entry that is not finite four NaN.  FB_EINVAL before any HIP call: a NULL model or output, on outside {0, 1}, n outside [1, 2^24],
 * no particles set, and (get, stretching with d_F == NULL) the deformation not switched on. */
int fb_model_set_particle_deformation(fb_model *m, int on);
int fb_model_get_particle_deformation(fb_model *m, double *d_F, double *elapsed);
int fb_model_particle_stretching(fb_model *m, const double *d_F, int n, double *d_out);
/* Lagrangian observations: the adjoint of the particle step (no reference counterpart).  With Xb the gradient of a scalar with respect
 * to the particles' positions at the time of the newest recorded step, and lam the adjoint variable of fb_model_set_adjoint,
 * fb_model_adjoint_back applies, while a particle adjoint is set, the transpose of the COUPLED discrete step (vorticity and particles):
 * per step, with x_s the position stage s started from and A_s = [[u_x, u_y], [v_x, v_y]] the gradient of the interpolant of the stage's
 * velocity at x_s (as the deformation gradient takes it; on a cell face the cell to the right), the stages in the order 3, 2, 1, 0:
 *   p = dt/6 Xb;           q = A_3^T p; acc = Xb + q        p = dt/3 Xb + dt q;     q = A_2^T p; acc += q
 *   p = dt/3 Xb + dt/2 q;  q = A_1^T p; acc += q            p = dt/6 Xb + dt/2 q;   q = A_0^T p; Xb <- acc + q
 * and the stage's transpose tendency of lam gains ( i ky r2c(S_u) - i kx r2c(S_v) ) / lap ((0, 0): / 1), S_u and S_v the transposes of
 * the interpolation applied to p_x and p_y at x_s (fb_model_scatter's fixed-point scheme: lam and Xb are the same bits in any order
 * of the particles).  The particles do not act on the flow, so Xb never depends on lam.  At the start of the window Xb equals F^T Xb(T)
 * for lam(T) = 0, F the deformation gradient.  A particle whose position or Xb is not finite deposits nothing and ends with NaN in Xb.
 * fb_model_particle_tape: depth >= 1 allocates room for depth steps x 4 stage positions (64 bytes per particle and step) and every
 * step from then on records the positions its stages start from; depth == 0 frees it; either way it starts empty.  The positions, F,
 * the vorticity, a tracer and the tangent are bit for bit what they are without.  While it is on fb_model_step steps eagerly (as
 * while fb_model_adjoint_record's tape is on) and a call that would overrun it is refused before anything is launched.
 * fb_model_set_vort, fb_model_set_spectrum and fb_model_set_particles empty it (another particle count, or NULL, frees it); it
 * needs particles.  FB_ENOMEM leaves nothing allocated.  Under fb_model_adjoint_checkpoint it still holds the whole window: the
 * segments that a sweep runs again move the vorticity alone.  fb_model_particle_tape_count: the steps on it and its depth (0, 0: none).
 * fb_model_set_particle_adjoint: Xb from d_xbar, device float64 [n][2]; NULL removes it; fb_model_set_particles (a new set or NULL)
 * removes it too.  fb_model_get_particle_adjoint: Xb into d_xbar.  While none is set fb_model_adjoint_back launches what it always has.
 * One GPU or a slab of one rank, as the particles.  FB_EINVAL before any HIP call: depth outside [0, 2^20], a NULL output, a NULL
 * model, no particles set, fb_model_get_particle_adjoint with none set; and for fb_model_adjoint_back while one is set: more steps
 * than the particle tape holds, a set of several adjoint variables, a particle tape and an adjoint window that hold different
 * numbers of steps. */
int fb_model_particle_tape(fb_model *m, int depth);
int fb_model_particle_tape_count(fb_model *m, int *count, int *depth);
int fb_model_set_particle_adjoint(fb_model *m, const double *d_xbar);      /* NULL: remove it */
int fb_model_get_particle_adjoint(fb_model *m, double *d_xbar);
/* Tangent-linear model (no reference counterpart): a perturbation dz of the vorticity, a real [nx][ny] field, carried along the
 * evolving state by the linearisation of the DISCRETE step (not of the PDE), so that M(zeta + eps dz) - M(zeta) = eps T(dz) + O(eps^2)
 * for the step M itself.  fb_model_set_tangent takes the device field d_dz_real in as fb_model_set_vort takes the vorticity and keeps
 * it as a half spectrum dz_c; from then on every step advances dz_c by the RK4 step of main.cpp:288-317 beside vort_c, stage by
 * stage: stage k uses the vorticity's state zeta of stage k (the state the tracer's stage k uses), psi_c = invertLaplacian(vort_c),
 * dpsi_c = invertLaplacian(dz_c), u = -psi_y, v = psi_x, du = -dpsi_y, dv = dpsi_x, and
 *   tend_dz = dealiase( r2c(-u dz_x - v dz_y) + r2c(-du zeta_x - dv zeta_y) + nu laplacian(dz_c) )
 * in float32, each r2c(...) formed as the vorticity's own stage forms its advective tendency (no source: a vorticity source does not
 * depend on the state), nu the model's own, the stage forms of main.cpp:246-251, :309-312.  Modes outside the dealiasing circle never
 * change after fb_model_set_tangent.  One perturbation per model; d_dz_real == NULL removes it and frees its state.  The vorticity,
 * its step, a tracer, particles and every record are bit for bit what they are without it; tangent, tracer and particles are
 * independent, any subset may be set.  Setting or removing it drops a captured step (fb_model_use_graph); it is captured again with
 * the tangent's stages.  fb_model_get_tangent: dz as fb_model_get_vort returns the vorticity.  fb_model_tangent_norm: into the device
 * float64 *d_out, kind 0 the enstrophy norm <dz^2> / 2, kind 1 the energy norm <|grad dpsi|^2> / 2 (<.>: the mean over the grid), summed
 * in float64 over the resident half spectrum (Hermitian weights 1 in the columns ky = 0 and ky = ny/2 and 2 elsewhere; the energy norm
 * leaves the (0, 0) mode out) in a fixed order: two calls on one state give the same bits.  fb_model_tangent_scale: dz *= a (the
 * renormalisation of a Lyapunov or bred-vector cycle).  FB_EINVAL before any HIP call: a NULL model, output or field, kind outside
 * {0, 1}, a not finite or zero, get / norm / scale without a tangent set.  Enqueued on the context stream, no synchronisation. */
int fb_model_set_tangent(fb_model *m, const float *d_dz_real);             /* NULL: remove the tangent */
int fb_model_get_tangent(fb_model *m, float *d_dz_real);
int fb_model_tangent_norm(fb_model *m, int kind, double *d_out);           /* 0 enstrophy, 1 energy */
int fb_model_tangent_scale(fb_model *m, float a);                          /* finite, != 0 */
/* Tangent subspace (no reference counterpart): up to FB_TANGENTS_MAX = 32 perturbations carried along the ONE trajectory, for several
 * Lyapunov exponents, the Kaplan-Yorke dimension and the backward Lyapunov vectors.  fb_model_set_tangents takes `count` device fields
 * [count][nx][ny] in, each as fb_model_set_tangent takes its one, and replaces whatever set was there; NULL removes all.  Every step
 * advances them one after the other, each with exactly the launches of the single tangent: perturbation k is bit for bit what
 * fb_model_set_tangent of the same field gives, and the vorticity, a tracer, particles, the adjoint and every record do not depend on
 * the count.  fb_model_set_tangent(dz) is fb_model_set_tangents(dz, 1); fb_model_get_tangent, fb_model_tangent_norm and
 * fb_model_tangent_scale act on perturbation 0.  fb_model_get_tangents: all of them, [count][nx][ny].  fb_model_tangent_count: 0 while
 * none is set (not an error).  Memory per perturbation: 3 half spectra on the active columns, 1 on the frozen ones (at most 203 MB at 4096^2).
 * The inner product of two perturbations is the bilinear form of fb_model_tangent_norm,
 *   <a, b> = 1 / (2 GRIDS^2) sum over kx and ky <= ny/2 of w q Re(a_c conj(b_c)),   GRIDS = nx ny,
 * summed in float64 over the resident half spectra, w = 1 in the columns ky = 0 and ky = ny/2 and 2 elsewhere; kind 0 (enstrophy):
 * q = 1, <a, b> = <a b> / 2 (the mean over the grid); kind 1 (energy): q = |k|^2 / laplacian_coe^2 with the (0, 0) mode left out,
 * <a, b> = <grad psi_a . grad psi_b> / 2.  <a, a> is what fb_model_tangent_norm returns.  The energy kind is a seminorm: a
 * perturbation that is a constant has length 0.  Modes outside the dealiasing circle never evolve but do count in both kinds, so a
 * set meant for exponents should be dealiased before it is set (or it keeps a component that neither grows nor decays).
 * fb_model_tangent_gram: every <v_i, v_j> into the device array d_gram [count][count] float64, row-major, symmetric bit for bit (the
 * upper triangle is computed, the lower copied).  fb_model_tangent_qr: modified Gram-Schmidt in place, in index order: for every j,
 * r_ij = <q_i, v_j> of the current v_j and v_j -= r_ij q_i for i < j, then r_jj = sqrt(<v_j, v_j>) and v_j /= r_jj; every element
 * formed in float64 and rounded once to float32 per update.  d_r [count][count] float64, row-major, is upper triangular with zeros
 * below the diagonal and v_j(before) = sum over i <= j of r_ij q_i; ln r_jj summed over a run and divided by the time is the j-th
 * Lyapunov exponent.  The coefficients stay on the device: nothing waits for the host.  A rank-deficient set shows as a diagonal
 * element that is not finite and positive and as perturbations that are not finite; the engine does not test for it (the caller
 * reads d_r anyway).  Every sum runs in a fixed order: two calls on one state give the same bits.  FB_EINVAL before any HIP call:
 * count outside [1, 32] with a non-NULL field, kind outside {0, 1}, a NULL output, a NULL model, get / gram / qr without a tangent
 * set.  Enqueued on the context stream, no synchronisation. */
#define FB_TANGENTS_MAX 32
int fb_model_set_tangents(fb_model *m, const float *d_dz_real, int count);  /* [count][nx][ny]; NULL: remove all */
int fb_model_get_tangents(fb_model *m, float *d_dz_real);                   /* [count][nx][ny] */
int fb_model_tangent_count(fb_model *m, int *count);                        /* 0 when none is set */
int fb_model_tangent_gram(fb_model *m, int kind, double *d_gram);           /* [count][count] */
int fb_model_tangent_qr(fb_model *m, int kind, double *d_r);                /* [count][count], upper triangular */
/* Covariant Lyapunov vectors (no reference counterpart): what Ginelli's algorithm needs of the engine on top of fb_model_tangent_qr.
 * The basis tape keeps the orthonormal bases Q_n of a window of QR intervals on the device: fb_model_tangent_tape(depth) allocates
 * depth slots, each the bases of all `count` perturbations of the current set (count half spectra; no stage state, no accumulator),
 * and leaves the tape empty; depth 0 frees it.  fb_model_tangent_tape_push copies the live bases into the next slot, device to device
 * on the context stream; it allocates nothing and the captured step stays.  fb_model_tangent_tape_count: slots pushed and slots
 * allocated, 0 and 0 while there is no tape.  The tape is freed with the model, by fb_model_set_tangents with NULL or another count
 * (a set of the same count keeps it); fb_model_set_vort and fb_model_set_spectrum leave it alone.  fb_model_info counts its bytes.
 * fb_model_tangent_combine: the live set becomes V = Q C, v_j = sum over i of c_ij q_i for all j at once, with Q the bases of tape slot
 * `slot` or, slot = -1, the live set itself (in place), and d_c a device array [count][count] float64, row-major.  Each source is
 * read once and each perturbation written once, whatever C holds.  Every element is summed in float64 in ascending i, not contracted,
 * and rounded once to float32: C = I returns the bits of Q, a permutation permutes them, a power of two scales them exactly.  The
 * vorticity, a tracer, particles and the adjoint are not touched by any of the four.  FB_EINVAL before any HIP call: depth outside
 * [0, 2^20], a NULL output, NULL coefficients, a NULL model, a tape of depth >= 1, a push or a combination without a tangent set, a
 * push without a tape or into a full one, slot outside [-1, slots pushed).  FB_ENOMEM: the tape does not fit (none is left).  Enqueued
 * on the context stream, no synchronisation (fb_model_tangent_tape waits for the stream where a tape is freed). */
int fb_model_tangent_tape(fb_model *m, int depth);                          /* 0: free the tape */
int fb_model_tangent_tape_push(fb_model *m);
int fb_model_tangent_tape_count(fb_model *m, int *count, int *depth);       /* 0, 0 while there is none */
int fb_model_tangent_combine(fb_model *m, int slot, const double *d_c);     /* -1: the live set in place; d_c [count][count] */
/* Adjoint model (no reference counterpart): the transpose T^T of the tangent-linear step above under the inner product
 * <a, b> = sum over the grid of a b, so that <T dz, lam> = <dz, T^T lam> for the DISCRETE step: sensitivities of a scalar of the
 * final state to the initial vorticity, singular vectors of T, gradients for fitting an initial state to later data.  It runs
 * backward over steps taken earlier, so the forward steps record a tape.  fb_model_adjoint_record(m, depth): depth >= 1 allocates
 * room for depth steps x 4 stage states of the vorticity (4 half spectra per step: 271 MB per step at 4096^2) and from then on every
 * stage of fb_model_step stores the state it starts from; depth == 0 frees the tape; either way the tape starts empty.  While it is
 * on, fb_model_step steps eagerly (a captured step would bake in a slot; the captured step is dropped and captured again after
 * depth == 0), and a call that would overrun the tape is refused with FB_EINVAL before anything is launched.  fb_model_set_vort and
 * fb_model_set_spectrum empty the tape.  fb_model_adjoint_recorded: the number of steps on the tape.  fb_model_set_adjoint takes the
 * device field d_lambda_real in as fb_model_set_vort takes the vorticity and keeps it as a half spectrum; NULL removes it and frees its
 * state.  fb_model_adjoint_back(m, nsteps) pops the last nsteps recorded steps, newest first, and applies each step's transpose to
 * lam: per stage, about the recorded stage state zeta with u, v its velocity and mu~ = dealiase(mu),
 *   L^T mu = gradx(u mu~) + grady(v mu~) + invertLaplacian( gradx(zeta_y mu~) - grady(zeta_x mu~) ) + nu laplacian(mu~)
 * (products in physical space, the result not dealiased again), combined by the transposed RK4 recurrences (csrc/fb_adjoint.h).  A
 * cost term at an intermediate time is get, add, set between two sweeps.  fb_model_get_adjoint: lam as fb_model_get_vort returns the
 * vorticity.  The vorticity, its step, a tracer, particles and a tangent are bit for bit what they are without the tape; two equal
 * runs give the same bits of lam.  FB_EINVAL before any HIP call: a NULL model, output or count, depth < 0, nsteps < 0 or beyond
 * what is recorded, get / back without an adjoint set.  FB_ENOMEM: the tape does not fit; nothing stays allocated.  Enqueued on the
 * context stream, no synchronisation. */
int fb_model_adjoint_record(fb_model *m, int depth);                       /* 0: stop recording, free the tape */
int fb_model_adjoint_recorded(fb_model *m, int *n);
int fb_model_set_adjoint(fb_model *m, const float *d_lambda_real);         /* NULL: remove the adjoint variable */
int fb_model_get_adjoint(fb_model *m, float *d_real);
int fb_model_adjoint_back(fb_model *m, int nsteps);
/* Adjoint subspace (no reference counterpart): up to FB_ADJOINTS_MAX = 32 adjoint variables swept back over the ONE tape, for the
 * leading singular vectors of T (Model.singular_vectors: block power iteration with a tangent subspace) and for the gradients of
 * several functionals of the final state in one sweep.  fb_model_set_adjoints takes `count` device fields [count][nx][ny] in, each as
 * fb_model_set_adjoint takes its one (never dealiased), and replaces whatever set was there; NULL removes all.
 * fb_model_set_adjoint(lam) is fb_model_set_adjoints(lam, 1): it REPLACES a set of several by the one, and fb_model_get_adjoint
 * returns variable 0 of a set, as fb_model_set_tangent and fb_model_get_tangent do with a tangent set.  fb_model_get_adjoints: all of
 * them, [count][nx][ny].  fb_model_adjoint_count: 0 while none is set (not an error).  fb_model_adjoint_back sweeps every variable of
 * the set: per stage the four fields that depend on the recorded state alone (u, v, zeta_x, zeta_y) go back to physical space ONCE,
 * each variable adds its own mu~, and the products of a chunk of up to 8 variables are formed in one pass that reads the four base
 * fields once: 4 + 5 count transformed fields per stage where count single sweeps take 9 count.  Variable k of a set is bit for bit
 * what fb_model_set_adjoint of the same field and the same sweep give; the set of one runs the single variable's own launches.
 * fb_model_adjoint_add_obs acts on a single variable and is refused (FB_EINVAL) while a set of several is there: forcing one
 * variable of a set at an intermediate time is get, add, set.  The step, the tape, a tracer, particles and a tangent never see the
 * set, and the captured step stays when it comes or goes.  Memory, counted by fb_model_info: per variable 3 half spectra on the
 * active columns and 1 on the frozen ones; shared, with C = min(count, 8), 4 + 5 C real fields and C half spectra (the one: 5 real
 * fields); at 4096^2 and count = 8 that is 1.6 GB + 3.0 GB + 0.5 GB.  FB_EINVAL before any HIP call: count outside [1, 32] with a
 * non-NULL field, a NULL output, a NULL model, a slab of several ranks, get without an adjoint set.  FB_ENOMEM: nothing of the adjoint
 * stays allocated.  Enqueued on the context stream; a set that goes or changes its count waits for the stream first. */
#define FB_ADJOINTS_MAX 32
int fb_model_set_adjoints(fb_model *m, const float *d_lambda_real, int count);  /* [count][nx][ny]; NULL: remove all */
int fb_model_get_adjoints(fb_model *m, float *d_real);                          /* [count][nx][ny] */
int fb_model_adjoint_count(fb_model *m, int *count);                            /* 0 when none is set */
/* Adjoint checkpointing (no reference counterpart): a second way to keep the adjoint's record, for windows whose full tape does not
 * fit.  fb_model_adjoint_checkpoint(m, every, max_steps): every >= 1 allocates a tape SEGMENT of `every` steps (x 4 half spectra),
 * room for ceil(max_steps / every) checkpoints of one state each and one more state for the live one: ceil(T / K) + 4 K + 1 half
 * spectra for a window of T steps where the full tape takes 4 T; K ~ sqrt(T) / 2 (binding.checkpoint_every) makes that
 * about 4 sqrt(T).  every == 0 frees all of it; either way the window starts empty.  This call and fb_model_adjoint_record replace
 * each other: turning one on frees what the other held.  Forward: fb_model_step counts the window's steps and, before every step
 * whose index in the window is a multiple of `every`, copies the state into the next checkpoint (device to device on the context
 * stream); it writes no tape slot, so the captured step is replayed between two checkpoints; a call that would pass max_steps is
 * refused before anything is launched.  Backward: fb_model_adjoint_back works as on the full tape, for one variable or a set, and
 * fills the segment again whenever it is empty: the live state is put aside (once per call), the checkpoint of the segment that
 * holds the newest unswept step is put back, and that segment's steps are taken again with the recording on.  These steps advance
 * the vorticity alone: no tracer, particles, deformation, tangent set, basis tape or step count moves.  Before the call returns the
 * live state is back.  A state that is put back gets its derivative fields from the priming pass and continues bit for bit like the
 * state that was stepped to, so lam is bit for bit what the full tape gives, and the vorticity and everything stepped beside it are
 * what they are with the mode off.  What is left of a segment stays on the tape between two calls: a window swept completely, in
 * whatever pieces, has taken exactly its own length in steps again (replayed).  fb_model_adjoint_recorded: the window's steps not
 * yet swept.  The window: fb_model_set_vort, fb_model_set_spectrum, fb_model_adjoint_checkpoint and fb_model_adjoint_record empty
 * it; once a sweep has popped a step, fb_model_step is refused until then; fb_model_set_source is refused while the window holds
 * unswept steps (they would be run again under another source; the model has no clock, so a source fixed over the window is run
 * again exactly); fb_model_profile_steps is refused while the mode is on.  fb_model_adjoint_checkpoint_info: every, max_steps, the
 * checkpoints the window holds and the steps run again since it began (each output may be NULL; all 0 while the mode is off).
 * fb_model_info counts the segment, the checkpoints and the live copy (and the full tape of fb_model_adjoint_record).  FB_EINVAL
 * before any HIP call: every outside [0, 2^20], max_steps < 1 or more than 2^20 checkpoints with every >= 1, a NULL model, a slab
 * of several ranks.  FB_ENOMEM: nothing of it stays allocated. */
int fb_model_adjoint_checkpoint(fb_model *m, int every, int max_steps);    /* every == 0: off, everything freed */
int fb_model_adjoint_checkpoint_info(fb_model *m, int *every, int *max_steps, int *checkpoints, long long *replayed);
/* Point observations and the forcing of the adjoint by their misfits (no reference counterpart): what a 4D-Var cost
 *   J(zeta_0) = 1/2 sum over times k and points p of (H_k zeta_k - y_k)_p^2 / sigma_p^2
 * and its gradient need of the engine on top of the adjoint sweep.  All four act between two steps only: the step, the tape, a
 * tracer, particles, a tangent and the sweep itself are bit for bit what they are without them.  kind: 0 zeta, 1 u, 2 v, 3 psi.
 * Positions are device float64 [n][2], unwrapped, n in [1, 2^24], on the grid and with the stencil and weights of fb_model_sample.
 * fb_model_observe: h = H zeta of the resident state into d_out, float64 [n]: the field of that kind formed as fb_model_get_vort and
 * fb_model_get_diag form it (their kernels, their rounding) and interpolated as fb_model_sample interpolates, bit for bit
 * fb_model_sample of that record; NaN where a position is not finite.  It changes nothing.
 * fb_model_scatter: the transpose of fb_model_sample, field[i][j] = sum over p of w_p wx_a(p) wy_b(p) over the sixteen stencil cells
 * of every point, into d_field, ANY device [nx][ny] float32 field, so that <sample(f, xy), w> = <f, scatter(xy, w)> (indices and
 * weights come from the one routine both use).  It needs nothing set; it is also how a quantity carried by particles is deposited
 * on the grid.  A point whose position or weight is not finite deposits nothing.  The result is bitwise reproducible, in any order
 * of execution and for any permutation of the points: every contribution is added by integer atomics into a fixed-point
 * accumulator of two 64-bit limbs per cell, in units of 2^-(e+39), e the largest integer with n_2 wmax_2 2^e <= 2^62, n_2 and wmax_2
 * the powers of two at or above n and above max |w| (found on the device), and each cell is then rounded to float32.  Error per
 * cell: half a float32 ulp of the cell's value (times 1 + 2^-28) plus at most 2^-(e+40) <= n max |w| 2^-101 per contribution.
 * fb_model_adjoint_add_obs: lam += H^T w for the adjoint variable set by fb_model_set_adjoint: the scatter of w, its r2c as
 * fb_model_set_adjoint takes a field, times the complex conjugate of the kind's spectral multiplier (1; -i ky / lap for u; i kx / lap
 * for v; 1 / lap for psi, the (0, 0) mode divided by 1 as the record divides it).  A cost term at an intermediate time is this call
 * between two sweeps.  It leaves the tape alone.
 * fb_model_obs_misfit: d_r[p] = (d_h[p] - d_y[p]) / sigma_p^2 and *d_cost += 1/2 sum over p of (d_h[p] - d_y[p])^2 / sigma_p^2, all
 * device float64, summed in a fixed order (two calls give the same bits); *d_cost is a device scalar that the caller zeroes.
 * d_sigma == NULL means sigma = 1; every sigma must be positive and finite, which is the caller's contract (checking it would need
 * a read of device memory).
 * One GPU or a slab of one rank, as the adjoint.  FB_EINVAL before any HIP call: kind outside [0, 3], a NULL pointer (but d_sigma),
 * n outside [1, 2^24], a NULL model, a slab of several ranks, fb_model_adjoint_add_obs without an adjoint set.  Enqueued on the
 * context stream, no synchronisation, no host round trip; each allocates its workspace at its first use (the accumulator, 2 nx ny
 * 64-bit words; one real field) and keeps it until fb_model_destroy. */
int fb_model_scatter(fb_model *m, const double *d_xy, const double *d_w, int n, float *d_field);
int fb_model_observe(fb_model *m, int kind, const double *d_xy, int n, double *d_out);      /* 0 zeta, 1 u, 2 v, 3 psi */
int fb_model_obs_misfit(fb_model *m, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost);
int fb_model_adjoint_add_obs(fb_model *m, int kind, const double *d_xy, const double *d_w, int n);
/* Tangent replay over the adjoint's tape (no reference counterpart): what a Gauss-Newton Hessian-vector product
 *   H_GN v = B^-1 v + sum over times k of T_k^T H_k^T R_k^-1 H_k T_k v
 * needs of the engine beside the sweep, so that no application of T steps the nonlinear model again.
 * fb_model_tangent_replay(m, first, nsteps) applies the tangent step of the taped steps first .. first + nsteps - 1 (0: the oldest slot
 * of fb_model_adjoint_record's tape), oldest first, to every perturbation of the tangent set, from the four recorded stage states of
 * each step: u, v, zeta_x, zeta_y of a stage are formed once for the whole set, and each perturbation's tendency is ONE product in
 * physical space, (((-u dz_x) - v dz_y) - du zeta_x) - dv zeta_y, then the tracer's stage update with the model's nu
 * (csrc/fb_replay.h): 4 + 5 M fields transformed per stage where M perturbations stepped beside the vorticity take 10 M.  It is the
 * operator fb_model_step applies to a tangent, not its bits (that one sums two spectral tendencies); perturbation k of a replayed set
 * has the bits of the replayed set of one, and two equal replays give the same bits.  The vorticity, a tracer, particles, the step
 * count, the tape and what fb_model_adjoint_recorded returns stay as they are.  Steps that a sweep has popped can still be replayed:
 * the range is bounded by the slots that hold recorded steps which no later step has overwritten.  nsteps == 0 does nothing.  Its
 * workspace, 4 + 5 min(M, 8) real fields, is allocated at the first replay of a set, counted by fb_model_info and freed with the set.
 * fb_model_adjoint_rewind(m, n) un-pops the last n steps that fb_model_adjoint_back popped (n == -1: every one still on the tape):
 * the sweep does not erase a slot, so a second sweep over the same steps gives the same bits.  A step recorded after a pop overwrites
 * the slots above it, which can then no longer be rewound to.
 * fb_model_observe_tangent(m, k, kind, d_xy, n, d_out): fb_model_observe of perturbation k of the tangent set in the place of the
 * resident state; for kind 0 bit for bit fb_model_sample of the field fb_model_get_tangents returns for it.
 * One GPU or a slab of one rank.  FB_EINVAL before any HIP call: a NULL model or pointer, first < 0, nsteps < 0, n < -1, kind outside
 * [0, 3], n outside [1, 2^24], k outside the set, no tangent set (replay, observe_tangent), no tape or a range beyond the recorded
 * slots (replay), more steps than were popped (rewind), adjoint checkpointing on (replay, rewind: the segment holds only a part of the
 * window), a particle adjoint set (rewind: the particle tape is popped in step), a slab of several ranks.  Enqueued on the context
 * stream, no synchronisation. */
int fb_model_tangent_replay(fb_model *m, int first, int nsteps);
int fb_model_adjoint_rewind(fb_model *m, int n);                            /* -1: every popped step still on the tape */
int fb_model_observe_tangent(fb_model *m, int k, int kind, const double *d_xy, int n, double *d_out);
/* Nonlinear-balance pressure of the current state into the device [nx][ny] field d_pres: what the reference's second program computes
 * from a psi record (invert_pres.cpp:135-185), here from the resident state with psi_c = invertLaplacian(vort_c) (fftwfop.cpp:112-117)
 * instead of readField + r2c of psi_step_N.bin (:132-135).  In the reference's float32 forms, g = 1/GRIDS:
 *   pxx_c, pyy_c, pxy_c = dealiase(gradx(gradx psi_c)), dealiase(grady(grady psi_c)), dealiase(gradx(grady psi_c))      (:139-150)
 *   curv = (c2r(pxx_c) g) (c2r(pyy_c) g) - (c2r(pxy_c) g)^2, the two products rounded, then the difference               (:153-159)
 *   q_c = rho * (f * (laplacian_coe psi_c) + (L_c + L_c)),  L_c = r2c(curv)                                              (:161-169)
 *   p = c2r(invertLaplacian(q_c)) g                                                                                      (:171-172)
 *   p -= p[ref_x + nx * ref_y]: the reference's flat index into the [nx][ny] field, kept as it is (:182-185; -x, -y of :71-79);
 *   the stored value at that index is exactly 0.  rho, f: configuration.hpp:10-11 (1.0, 1e-5).
 * FB_EINVAL (before any HIP call) for a NULL model or output, a negative ref_x / ref_y or a flat index >= nx * ny.  Enqueued on the
 * context stream, no synchronisation, no host round trip; uses the record buffers and leaves the state and a captured step untouched. */
int fb_model_get_pressure(fb_model *m, float rho, float f, int ref_x, int ref_y, float *d_pres);
/* Shell spectra and cascade fluxes of the current state (no reference counterpart): d_table is a device float64 [nshells][10], one row
 * per wavenumber shell, nshells from fb_spectra_shells.  G = nx ny.  For a mode (i, j) of the half spectrum: i' = min(i, nx - i),
 * kx = 2 pi i' / Lx, ky = 2 pi j / Ly, k^2 = kx^2 + ky^2 in float64 (2 pi = 6.283185307179586, Lx, Ly the context's float32 lengths
 * widened); w = 1 for j = 0 and j = ny/2, else 2; M = the dealiasing mask (fftwfop.cpp:57-68); a = vort_c / G; n = M N / G with N the
 * unnormalised r2c of J = -u zeta_x - v zeta_y, formed in float32 as a stage of the step forms it (main.cpp:151-227) WITHOUT vort_src
 * and without the viscous term: the transfer is advective only, the forcing's input is not in the table.  Shells: dk = 2 pi /
 * max(Lx, Ly), a mode belongs to shell b = floor(sqrt(k^2) / dk + 0.5); shell 0 holds the mean mode only.  Columns, every sum in
 * float64 over all modes of the shell (the frozen ones beyond the mask included unless M appears):
 *   0 k_lo = max(b - 0.5, 0) dk   1 k_hi = (b + 0.5) dk [rad m^-1]   2 n = sum w (modes of the full spectrum; sums to G)
 *   3 E = sum w |a|^2 / (2 k^2) [m^2 s^-2] (0 for k = 0; sums to <u^2 + v^2>/2)   4 Z = sum w |a|^2 / 2 [s^-2] (sums to <zeta^2>/2)
 *   5 T_E = sum w Re(conj(a) n) / k^2 [m^2 s^-3] (0 for k = 0)   6 T_Z = sum w Re(conj(a) n) [s^-3]
 *   7 Pi_E = -sum_{b' <= b} T_E   8 Pi_Z = -sum_{b' <= b} T_Z (added from shell 0 upwards)   9 D_Z = sum M nu k^2 w |a|^2 [s^-3]
 * so that d/dt sum Z = sum_b (T_Z - D_Z) for an unforced run.  The result repeats bit for bit from call to call on the same state.
 * FB_EINVAL (before any HIP call) for a NULL model or table.  Enqueued on the context stream, no synchronisation, no host round trip;
 * uses record buffers of the model's own (allocated on first use) and leaves the state, the step's buffers and a captured step untouched. */
int fb_model_get_spectra(fb_model *m, double *d_table);
/* host logic, no GPU needed: the number of shells, floor(sqrt((pi nx / Lx)^2 + (pi ny / Ly)^2) / dk + 0.5) + 1 (the corner mode lies in
 * the last shell); FB_EINVAL for a NULL pointer, non-positive lengths or an unsupported size */
int fb_spectra_shells(int nx, int ny, float lx, float ly, int *nshells);
/* Azimuthal means about a vortex centre (no reference counterpart: it ships find_min, run by hand on a psi record).  The fields: zeta
 * as fb_model_get_vort returns it, psi, u, v as fb_model_get_diag returns them, bit for bit; psi is formed for FB_CENTER_PSI_MIN only.
 * d_center: four device doubles xc, yc, flat index, value.  FB_CENTER_FIXED: the caller's (xc, yc) with 0 <= xc < Lx, 0 <= yc < Ly,
 * index -1, value 0.  FB_CENTER_PSI_MIN / FB_CENTER_VORT_MAX: the grid point of the smallest psi / largest zeta of the whole domain,
 * ties to the smallest flat index ny i + j (np.argmin / np.argmax of the flattened [nx][ny] field); xc = i dx, yc = j dy, dx =
 * (double)Lx / nx, dy = (double)Ly / ny (the context's float32 lengths widened), the value widened.  Per point (i, j), in float64
 * without contraction: ddx = i dx - xc, minus Lx where ddx > Lx/2, plus Lx where ddx < -Lx/2 (the minimum image), ddy likewise;
 * r2 = ddx^2 + ddy^2, r = sqrt(r2); the bin b is the integer with (b dr)^2 <= r2 < ((b + 1) dr)^2 (points with b >= nbins take no
 * part); c1 = ddx / r, s1 = ddy / r (1, 0 at r2 = 0); v_r = u c1 + v s1, v_t = v c1 - u s1; c_m = c_{m-1} c1 - s_{m-1} s1,
 * s_m = s_{m-1} c1 + c_{m-1} s1.  d_table: device float64 [nbins][12 + 2 nmodes], one row per radial bin, <.> the mean over its points:
 *   0 r_lo = b dr   1 r_hi = (b + 1) dr [m]   2 n (points)   3 <r>   4 <zeta>   5 <v_t>   6 <v_r>   7 <zeta^2>   8 <v_t^2>   9 <v_r^2>
 *   10 <v_r zeta>   11 Gamma = dx dy sum_{b' <= b} sum zeta [m^2 s^-1], the circulation inside r_hi, added from bin 0 upwards
 *   12 + 2 (m - 1), 13 + 2 (m - 1): Re, Im of zeta_m = <zeta e^{-i m theta}> = (<zeta c_m>, -<zeta s_m>), m = 1 .. nmodes
 * A row with n = 0 has zeros in columns 3-10 and from 12 on.  The eddy quantities are the caller's to form: eddy enstrophy
 * <zeta^2> - <zeta>^2, eddy vorticity flux <v_r zeta> - <v_r><zeta>, amplitude of wavenumber m 2 |zeta_m| (the differences cancel;
 * the table keeps the moments).  The counts are exact; the sums are added with float64 atomics and may differ in the last bits from
 * call to call.  FB_EINVAL before any HIP call: a NULL model, table or centre; an unknown mode; a fixed centre outside the domain or
 * not finite; nbins outside [2, 4096]; nmodes outside [0, 8]; dr not finite, dr < min(dx, dy), or nbins dr > min(Lx, Ly) / 2 (every
 * circle lies whole inside the minimum-image cell).  Enqueued on the context stream, no synchronisation, no host round trip; uses
 * record buffers of the model's own (allocated on first use: two real fields and table-sized reduction buffers) and leaves the
 * state, the step's buffers, a tracer and a captured step untouched. */
#define FB_CENTER_FIXED    0   /* the caller's (xc, yc)                                         */
#define FB_CENTER_PSI_MIN  1   /* grid point of the smallest psi (cyclone's circulation centre) */
#define FB_CENTER_VORT_MAX 2   /* grid point of the largest zeta                                */
int fb_model_get_azimuthal(fb_model *m, int center_mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table,
                           double *d_center);
/* host logic, no GPU needed: the columns of the table, 12 + 2 nmodes; FB_EINVAL for nmodes outside [0, 8] or a NULL pointer */
int fb_azimuthal_cols(int nmodes, int *ncols);
/* Vortex census (no reference counterpart; McWilliams 1990): the coherent structures of a thresholded field, labelled and measured.
 * d_field (the mask field f) and d_weight (the weight w; NULL: w = f) are ANY device [nx][ny] float32 fields, as fb_model_sample takes
 * any field: zeta, W, the tracer ...  Cell c is in the mask iff f[c] > threshold (FB_CENSUS_ABOVE) or f[c] < threshold
 * (FB_CENSUS_BELOW); a NaN in f is never in the mask.  A structure is a 4-connected component of the mask on the doubly periodic
 * grid: cell (i, j) neighbours ((i +- 1) mod nx, j) and (i, (j +- 1) mod ny).  Its label is the smallest flat index ny i + j of its
 * cells, and that cell is its anchor (i0, j0).  Structures with fewer than min_cells cells are dropped; the kept ones, in ascending
 * label order, get the dense ids 0, 1, 2, ...  d_table: device float64 [max_structures][FB_CENSUS_COLS], row = dense id:
 *   0 label (a whole number)   1 n (cells)   2 S_w = sum w   3 S_wx = sum (w ex)   4 S_wy = sum (w ey)   5 S_wxx = sum ((w ex) ex)
 *   6 S_wyy = sum ((w ey) ey)   7 S_wxy = sum ((w ex) ey)   8 S_x = sum ex   9 S_y = sum ey
 *   10 peak: the w of largest |w| among the structure's cells (a NaN never wins, ties go to the smallest flat index; NaN where every
 *   w of the structure is a NaN)   11 peak_index: the flat index of that cell (-1 likewise)
 * with ex = (double)((i - i0 + nx/2) mod nx - nx/2) dx, ey = (double)((j - j0 + ny/2) mod ny - ny/2) dy (a non-negative modulus: the
 * minimum-image offset from the anchor [m]), dx = (double)Lx / nx, dy = (double)Ly / ny (the context's float32 lengths widened, as
 * the particles and the azimuthal record take them).  Everything is float64 without contraction, w widened exactly and every product
 * one correctly rounded multiply in the order of the brackets above: every TERM is reproducible bit for bit, and only the order of
 * the sums (float64 atomics) differs, from call to call too; label, n, peak and peak_index are exact.  The table keeps the raw
 * moments and subtracts nothing, as the azimuthal table does (centroid: anchor + (S_wx, S_wy) / S_w; the central second moments
 * follow).  The moments are meaningful for a structure that spans less than half the domain on each axis: beyond that the minimum
 * image misfolds.  label, n, S_w, peak and peak_index stay right for any structure, a percolating one included.  Rows from
 * min(found, max_structures) on hold label = -1 and zeros.  d_count: device int32 [2]: found, the number of kept structures (it may
 * exceed max_structures: the table then holds the first max_structures of them), and the number of all structures before min_cells.
 * d_labels (may be NULL): device int32 [nx][ny], the dense id of every kept structure's cells, ids >= max_structures too, and -1
 * elsewhere.  Memory of the model's own, allocated at the first call and kept: two int32 [nx][ny] arrays and nx ny / 128 bytes; the
 * record workspace, the state, the step's buffers and a captured step are untouched.  FB_EINVAL before any HIP call: a NULL model,
 * then a NULL field, table or count, a threshold that is not finite, a mode outside {0, 1}, min_cells outside [1, 2^30],
 * max_structures outside [1, FB_CENSUS_MAX = 65536].  Enqueued on the context stream, no synchronisation, no host round trip. */
#define FB_CENSUS_ABOVE 0      /* f > threshold */
#define FB_CENSUS_BELOW 1      /* f < threshold */
#define FB_CENSUS_COLS  12
#define FB_CENSUS_MAX   65536
int fb_model_census(fb_model *m, const float *d_field, const float *d_weight, int mode, float threshold, int min_cells, int max_structures,
                    double *d_table, int *d_count, int *d_labels);
/* Stochastic ring forcing, linear drag and hyperviscosity as a split stage after every completed RK4 step (off by default).  For
 * every stored mode (i, j) of the half spectrum inside the dealiasing circle (a masked mode keeps its bits)
 *   zeta_new = fl32(D zeta) + Delta_n,   D = fl32(exp(-(mu + nu_p K^2p) dt)) evaluated in float64, K^2 = -laplacian_coe(i, j),
 * an exact exponential factor, so a nabla^8 hyperviscosity puts no stability limit on dt.  The ring holds the modes with
 * |sqrt(K^2) - k_f| <= dk [rad/m] (float64), the four self-conjugate modes (i in {0, nx/2}, j in {0, ny/2}) left out; N_ring counts
 * them over the FULL spectrum (a stored mode with 0 < j < ny/2 twice).  On the ring
 *   Delta_n = fl32(GRIDS sqrt(2 rate dt K^2 / N_ring) e^{i theta}),  theta = 2 pi u / 2^32,
 * u = output word 0 of Philox4x32-10 with counter (i, j, n_lo, n_hi) and key (seed_lo, seed_hi), n the forcing clock: the split
 * stages applied since this call, a 64-bit count in device memory (a captured step replays correctly).  On the lines j = 0 and
 * j = ny/2 a mode with i > nx/2 takes the conjugate of mode (nx - i, j).  White in time: from rest one stage adds rate dt of energy
 * E = sum over the full spectrum of |zeta / GRIDS|^2 / (2 K^2) exactly; rate [m^2 s^-3] is the mean energy injection rate.  The noise
 * depends on (i, j, n, seed) alone: not on the layout, the kernel path or the launch geometry.
 * rate = mu = nu_p = 0 removes the stage; rate = 0 alone is pure dissipation and needs no ring (k_f, dk ignored).  Every perturbation
 * of the tangent set is multiplied by D inside the circle after each step (the forcing is additive), so the Lyapunov exponents are
 * those of the forced-dissipative system.  The tracer, the particles and their deformation gradient are untouched.  The derivative
 * fields are formed again after the stage, inside the step.  Memory: one half spectrum where the state arrays are not in the
 * 3-pass layout, and a few KiB; allocated here, counted by fb_model_info.
 * FB_EINVAL before any HIP call: rate, mu, nu_p (and with rate > 0 k_f, dk) not finite or negative, p outside [1, 8]; then a
 * NULL model; then k_f - dk <= 0, an empty ring or a ring that holds a masked mode.  FB_EUNSUPPORTED: a slab of several
 * ranks; while the adjoint's tape or a checkpointed window exists (and fb_model_adjoint_record / fb_model_adjoint_checkpoint are
 * refused with FB_EUNSUPPORTED while forcing is set: the transpose through D and the replay of a window's noise are not built). */
int fb_model_set_forcing(fb_model *m, double rate, double k_f, double dk, size_t seed, double mu, double nu_p, int p);
/* out[6] on the HOST: the forcing clock, then the running totals since fb_model_set_forcing of dE_forc = E(zeta_new) - E(zeta'),
 * dE_diss = E(zeta') - E(zeta) with zeta' = fl32(D zeta), dZ_forc and dZ_diss likewise with Z = sum over the full spectrum of
 * |zeta / GRIDS|^2 / 2, then N_ring.  Summed in the stage's own pass in float64 with Hermitian weights, per workgroup and then in a
 * fixed order: no atomics, the bits repeat.  Waits for the model's stream.  FB_EINVAL while no forcing is set. */
int fb_model_forcing_budget(fb_model *m, double *out);
/* Delta_n for the clock value n into d_spec, a device array [nx][ny/2+1] complex in the layout of fb_model_get_spectrum (zeros off
 * the ring), from the device function the stage itself calls.  FB_EINVAL while no forcing is set. */
int fb_model_forcing_increment(fb_model *m, size_t n, float *d_spec);
/* vort_c in the reference layout */
int fb_model_get_spectrum(fb_model *m, float *d_spec);
int fb_model_set_spectrum(fb_model *m, const float *d_spec);
/* bytes of HBM the model holds, and the algorithmic bytes of one step (320*nx*ny) */
int fb_model_info(fb_model *m, size_t *hbm_bytes, size_t *alg_bytes_per_step);
/* times `nsteps` steps with HIP events on the model's stream;
 * total_ms = wall time of the whole batch of steps on the device */
int fb_model_time_steps(fb_model *m, int nsteps, float *total_ms);
/* the same steps with a HIP-event pair around every kernel launch (on the model's stream).
 * Kernel classes: 0 = k_col_strided<+1> (4 fields, backward x sub-pass), 1 = the fused row pass,
 * 2 = k_col_strided<-1> (tendency, forward x sub-pass), 3 = k_col_mid -- or, where the single-pass x
 * transform is in use (nx = 4096 on one GPU), k_col_full, and classes 0 and 2 have no launches.
 * ms_sum[4] receives the summed durations, launches[4] the launch counts. */
int fb_model_profile_steps(fb_model *m, int nsteps, float *ms_sum, int *launches);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU: slab decomposition over the GPUs of one node, one process per GPU, RCCL all-to-all transposes over
 * xGMI between the row and the column passes.  No reference counterpart -- the reference is
 * single-process; one fb_slab_step() computes what one iteration of main.cpp:259-323 computes, on this rank's share.
 *
 * Rank r of `world` (a power of two) owns the x rows [r*XL, (r+1)*XL), XL = nx/world, of every physical field, and of
 * every spectral field KA "active" ky columns [r*KA, (r+1)*KA) -- the columns below world*KA hold every mode inside
 * the dealiasing circle and are exchanged twice per RK stage -- plus KF "frozen" columns [world*KA + r*KF, ...): their
 * modes are masked (fftwfop.cpp:57-61), never change (SURVEY.md note N1), and cross the links once per fb_slab_set_vort_local.
 * The engine owns the exchange buffers, two HIP streams (compute / communication) and the schedule: per stage the four
 * derivative fields leave field group by field group behind their backward x sub-pass, the tendency leaves row chunk
 * by row chunk behind the row pass (fb_slab_plan reports the granularity, which follows the message size).
 *
 * Transports: fb_slab_connect_rccl (the product: grouped ncclSend/ncclRecv; rank 0 obtains the id from
 * fb_slab_unique_id and hands it to the other ranks -- file, environment, torch.distributed, MPI ...),
 * fb_slab_connect_local (all ranks as threads of ONE process on ONE GPU: rehearsal of the schedule),
 * fb_slab_connect_callback (the caller moves the bytes).  world == 1 needs no transport.
 * ------------------------------------------------------------------------------------- */
typedef struct fb_slab fb_slab;
#define FB_UNIQUE_ID_BYTES 128
int fb_slab_unique_id(char *id128);                       /* ncclGetUniqueId */
int fb_slab_create(fb_slab **out, int nx, int ny, float lx, float ly, float nu, float dt, int rank, int world);
int fb_slab_destroy(fb_slab *s);
int fb_slab_connect_rccl(fb_slab *s, const char *id128);  /* ncclCommInitRank: collective over all ranks */
int fb_local_hub_create(void **hub, int world);
int fb_local_hub_destroy(void *hub);
int fb_slab_connect_local(fb_slab *s, void *hub);
/* For every peer p: `count` floats at send + p*stride + offset go to recv + rank*stride + offset of peer p (own block
 * included); must be complete, or ordered on hip_stream, when the callback returns.  Return 0 on success. */
typedef int (*fb_alltoall_fn)(void *user, const float *d_send, float *d_recv, size_t stride, size_t offset, size_t count, void *hip_stream);
int fb_slab_connect_callback(fb_slab *s, fb_alltoall_fn fn, void *user);
/* this rank's rows [XL][ny] (device pointers): readField + r2c (main.cpp:143-144,256), vort_src (main-shallow-water.cpp:304;
 * NULL = zeros), the record path (main.cpp:273-281) */
int fb_slab_set_vort_local(fb_slab *s, const float *d_rows);
int fb_slab_set_source_local(fb_slab *s, const float *d_rows);
int fb_slab_get_vort_local(fb_slab *s, float *d_rows);
/* the stage-0 record dumps psi, u, v (main.cpp:181-222) on this rank's rows; any may be NULL */
int fb_slab_get_diag_local(fb_slab *s, float *d_psi, float *d_u, float *d_v);
/* fb_model_get_okubo_weiss on this rank's rows [XL][ny] (either may be NULL, not both); collective: every rank calls it */
int fb_slab_get_okubo_weiss_local(fb_slab *s, float *d_w_rows, float *d_tau_rows);
/* fb_model_get_eddy_diffusivity of the whole domain: d_zeta_rows, d_grad2_rows are this rank's rows [XL][ny] (optional), d_table
 * the full table, on every rank (the ranks' ranges and histograms are all-gathered through the transport, summed in rank order);
 * collective: every rank calls it */
int fb_slab_get_eddy_diffusivity(fb_slab *s, int nbins, double *d_table, float *d_zeta_rows, float *d_grad2_rows);
/* fb_model_get_pressure on this rank's rows [XL][ny], bit for bit (the reference point is a point of the whole domain: its owner's
 * value reaches every rank through the transport); collective: every rank calls it */
int fb_slab_get_pressure_local(fb_slab *s, float rho, float f, int ref_x, int ref_y, float *d_pres_rows);
/* fb_model_get_spectra of the whole domain: the full table on every rank.  Each rank sums the modes of the ky columns it owns (active
 * and frozen), the ranks' partial sums are all-gathered through the transport and added in rank order, the running sums of columns 7
 * and 8 are taken after that; collective: every rank calls it */
int fb_slab_get_spectra(fb_slab *s, double *d_table);
/* fb_model_get_azimuthal of the whole domain: the full table and the centre on every rank.  The ranks' centre candidates, then their
 * sums over the rows they own, are all-gathered through the transport; the sums are added in rank order; collective: every rank
 * calls it */
int fb_slab_get_azimuthal(fb_slab *s, int center_mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table,
                          double *d_center);
/* the passive tracer (fb_model_set_tracer) of a slab: this rank's rows [XL][ny] in and out, bit for bit what one GPU computes; the
 * table is that of the whole domain, on every rank, as fb_slab_get_eddy_diffusivity gathers it; all three are collective.  The
 * tracer's stages exchange their fields through the transport beside the step's own exchanges. */
int fb_slab_set_tracer_local(fb_slab *s, const float *d_rows, float kappa);  /* NULL: remove the tracer */
int fb_slab_get_tracer_local(fb_slab *s, float *d_rows);
int fb_slab_get_tracer_eddy_diffusivity(fb_slab *s, int nbins, double *d_table, float *d_c_rows, float *d_grad2_rows);
/* the tangent-linear model (fb_model_set_tangent) of a slab of ONE rank: the same code, bit for bit what fb_model_* computes.  On
 * world > 1 they return FB_EINVAL with a message. */
int fb_slab_set_tangent(fb_slab *s, const float *d_dz_real);               /* NULL: remove the tangent */
int fb_slab_get_tangent(fb_slab *s, float *d_dz_real);
int fb_slab_tangent_norm(fb_slab *s, int kind, double *d_out);
int fb_slab_tangent_scale(fb_slab *s, float a);
/* the tangent subspace (fb_model_set_tangents) of a slab of ONE rank, likewise */
int fb_slab_set_tangents(fb_slab *s, const float *d_dz_real, int count);   /* NULL: remove all */
int fb_slab_get_tangents(fb_slab *s, float *d_dz_real);
int fb_slab_tangent_count(fb_slab *s, int *count);
int fb_slab_tangent_gram(fb_slab *s, int kind, double *d_gram);
int fb_slab_tangent_qr(fb_slab *s, int kind, double *d_r);
/* the basis tape and the combination (fb_model_tangent_tape) of a slab of ONE rank, likewise */
int fb_slab_tangent_tape(fb_slab *s, int depth);
int fb_slab_tangent_tape_push(fb_slab *s);
int fb_slab_tangent_tape_count(fb_slab *s, int *count, int *depth);
int fb_slab_tangent_combine(fb_slab *s, int slot, const double *d_c);
/* the adjoint model (fb_model_adjoint_record) of a slab of ONE rank: the same code, bit for bit what fb_model_* computes.  On
 * world > 1 they return FB_EINVAL with a message. */
int fb_slab_adjoint_record(fb_slab *s, int depth);
int fb_slab_adjoint_recorded(fb_slab *s, int *n);
int fb_slab_set_adjoint(fb_slab *s, const float *d_lambda_real);           /* NULL: remove the adjoint variable */
int fb_slab_get_adjoint(fb_slab *s, float *d_real);
int fb_slab_adjoint_back(fb_slab *s, int nsteps);
/* the adjoint subspace (fb_model_set_adjoints) of a slab of ONE rank, likewise */
int fb_slab_set_adjoints(fb_slab *s, const float *d_lambda_real, int count); /* NULL: remove all */
int fb_slab_get_adjoints(fb_slab *s, float *d_real);
int fb_slab_adjoint_count(fb_slab *s, int *count);
/* adjoint checkpointing (fb_model_adjoint_checkpoint) of a slab of ONE rank, likewise */
int fb_slab_adjoint_checkpoint(fb_slab *s, int every, int max_steps);
int fb_slab_adjoint_checkpoint_info(fb_slab *s, int *every, int *max_steps, int *checkpoints, long long *replayed);
/* the point observations (fb_model_scatter) of a slab of ONE rank, likewise */
int fb_slab_scatter(fb_slab *s, const double *d_xy, const double *d_w, int n, float *d_field);
int fb_slab_observe(fb_slab *s, int kind, const double *d_xy, int n, double *d_out);
int fb_slab_obs_misfit(fb_slab *s, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost);
int fb_slab_adjoint_add_obs(fb_slab *s, int kind, const double *d_xy, const double *d_w, int n);
/* the tangent replay, the rewind and the observation of a perturbation (fb_model_tangent_replay) of a slab of ONE rank, likewise */
int fb_slab_tangent_replay(fb_slab *s, int first, int nsteps);
int fb_slab_adjoint_rewind(fb_slab *s, int n);
int fb_slab_observe_tangent(fb_slab *s, int k, int kind, const double *d_xy, int n, double *d_out);
/* the Lagrangian particles (fb_model_set_particles) of a slab of ONE rank: the same code, bit for bit what fb_model_* computes.  On
 * world > 1 they return FB_EUNSUPPORTED: particles distributed over row slabs need neighbour halo rows that the all-to-all transport
 * does not provide. */
int fb_slab_set_particles(fb_slab *s, const double *d_xy, int n);          /* NULL: remove the particles */
int fb_slab_get_particles(fb_slab *s, double *d_xy);
int fb_slab_particle_count(fb_slab *s, int *n);
int fb_slab_sample(fb_slab *s, const float *d_field, const double *d_xy, int n, double *d_out);
/* the particles' deformation gradient (fb_model_set_particle_deformation) on a slab of ONE rank, refused on world > 1 as the particles are */
int fb_slab_set_particle_deformation(fb_slab *s, int on);
int fb_slab_get_particle_deformation(fb_slab *s, double *d_F, double *elapsed);
int fb_slab_particle_stretching(fb_slab *s, const double *d_F, int n, double *d_out);
/* the particle tape and the particle adjoint (fb_model_particle_tape) on a slab of ONE rank, refused on world > 1 as the particles are */
int fb_slab_particle_tape(fb_slab *s, int depth);
int fb_slab_particle_tape_count(fb_slab *s, int *count, int *depth);
int fb_slab_set_particle_adjoint(fb_slab *s, const double *d_xbar);
int fb_slab_get_particle_adjoint(fb_slab *s, double *d_xbar);
/* the vortex census (fb_model_census) on a slab of ONE rank: the same code, bit-equal labels.  On world > 1 it returns
 * FB_EUNSUPPORTED: a structure that crosses the ranks' row slabs needs a border merge over the ranks. */
int fb_slab_census(fb_slab *s, const float *d_field, const float *d_weight, int mode, float threshold, int min_cells, int max_structures,
                   double *d_table, int *d_count, int *d_labels);
/* the split stage (fb_model_set_forcing) on a slab of ONE rank: the same code, the same bits.  On world > 1 they return
 * FB_EUNSUPPORTED: the budget's sums and the re-priming after the stage are built for the one column group of one rank. */
int fb_slab_set_forcing(fb_slab *s, double rate, double k_f, double dk, size_t seed, double mu, double nu_p, int p);
int fb_slab_forcing_budget(fb_slab *s, double *out);
int fb_slab_forcing_increment(fb_slab *s, size_t n, float *d_spec);
int fb_slab_step(fb_slab *s, int nsteps);
int fb_slab_synchronize(fb_slab *s);
/* the rank's compute stream is the engine's own: record an event behind what has been queued on it (fb_slab_get_*_local ->
 * copy stream) or make it wait for one (H2D of a new source -> fb_slab_set_source_local); events from fb_event_create */
int fb_slab_record_event(fb_slab *s, void *event);
int fb_slab_wait_event(fb_slab *s, void *event);
int fb_slab_time_steps(fb_slab *s, int nsteps, float *total_ms);
/* exchanges a known pattern of world*count floats through the connected transport; *wrong_words = 0 when every word arrived */
int fb_slab_transport_selftest(fb_slab *s, size_t count, size_t *wrong_words);
/* what is connected: transport name ("rccl", "local", "callback", "none" for world == 1), the size / rank / device of the transport's
 * own communicator (RCCL: ncclCommCount, ncclCommUserRank, ncclCommCuDevice; -1 where the transport has none) and this rank's HIP
 * device ordinal.  Any pointer may be NULL. */
int fb_slab_transport_info(fb_slab *s, char *name, size_t cap, int *comm_ranks, int *comm_rank, int *comm_device, int *hip_device);
int fb_slab_info(fb_slab *s, int *rows_local, int *cols_active, int *cols_frozen, int *ky0_active, int *ky0_frozen,
                 int *field_groups, int *row_chunks);
/* host logic, no GPU needed: XL, KA, KF of a decomposition */
int fb_slab_geometry(int nx, int ny, int world, int *rows_local, int *cols_active, int *cols_frozen);
/* host logic, no GPU needed: the column groups a rank's active columns are cut into (1, or 2 where a stage is pipelined by
 * column groups: BASELINE configs 4 and 5); cols2[g] = columns per rank of group g (0 for an absent group): a rank's active
 * slab [rank*KA, (rank+1)*KA) is cut locally, its first cols2[0] columns are group 0 */
int fb_slab_col_groups(int nx, int ny, int world, int *ngroups, int *cols2);
/* host logic, no GPU needed: the operations of ONE RK stage in issue order, ops[i] = 16*kind + argument, kind =
 * 1 backward x sub-pass of field group g, 2 all-to-all of the derivative fields (field group g; column group g when
 * pipelined by column groups), 3 row pass of row chunk h, 4 all-to-all of tendency chunk h (every column group), 5 forward x
 * pass + RK update (of column group g), 6 backward x sub-pass of all four fields of column group g.
 * Returns the number of operations (negative never; 0 on error). */
int fb_slab_plan(int nx, int ny, int world, int *field_groups, int *row_chunks, int *ops, int cap);
/* lower level: a context bound to one rank's slabs (the operator / FFT entry points above need world == 1) */
int fb_create_slab(fb_ctx **out, int nx, int ny, float lx, float ly, int rank, int world);

/* ---------------------------------------------------------------------------------------
 * Field I/O on HOST buffers.  Replaces writeField / readField (fieldio.hpp:5-6,
 * fieldio.cpp:7-33): identical bytes on disk and identical stderr lines, plus a status.
 * ------------------------------------------------------------------------------------- */
int fb_write_field(const char *filename, const float *h_data, size_t len);
int fb_read_field(const char *filename, float *h_data, size_t len);

/* ---------------------------------------------------------------------------------------
 * Initial-field synthesis on HOST buffers (nx*ny float32), the inputs of the benchmark configs.
 * kind = "elliptic"  makefield-elliptic-vortex.cpp:14-52
 *        "kuo2004"   makefield-Kuo2004.cpp:30-41 + field_generator.cpp:10-28 (buffer zeroed first)
 *        "gaussian"  makefield-gaussian.cpp:14-31
 *        "const"     makefield-const-vortex.cpp:14-38
 * fb_make_source_kuo2004: the FIFO producer's source cake, vort_src_input.cpp:35-46.
 * ------------------------------------------------------------------------------------- */
int fb_make_field(const char *kind, int nx, int ny, float lx, float ly, float *h_vort);
int fb_make_source_kuo2004(int nx, int ny, float lx, float ly, float duration, float *h_src);

#ifdef __cplusplus
}
#endif
#endif /* FFTBARO_H */
