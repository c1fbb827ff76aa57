// fb_beside_particles.h -- the host side of the Lagrangian particles: the particles and their stage, the deformation gradient and its
// stretching, sample(), the particle tape and the particle adjoint (included by fb_beside.h after the path the fields share; kernels:
// fb_particles.h, fb_lagrangian.h; C ABI: include/fftbaro.h).
#pragma once

// the largest count of particles, and of points of a sample, a scatter or an observation
#define FB_PARTICLES_MAX (1 << 24)

// ---- the Lagrangian particles (kernels: fb_particles.h) ----
static void particle_adjoint_free(fb_model *m)
{
    dev_free(m->pa);
    dev_free(m->pa_acc);
}

static void particle_tape_free(fb_model *m)
{
    dev_free(m->pt_tape);
    m->pt_depth = m->pt_fill = 0;
}

static void particles_free(fb_model *m)
{
    dev_free(m->pd);                                        // F belongs to the particles it was carried by
    particle_tape_free(m);                                  // and so do their tape and their adjoint
    particle_adjoint_free(m);
    dev_free(m->pt);
    dev_free(m->pt_uv);
    m->pt_n = 0;
}

// stage `stage` of step `step` of the particle tape: [pt_n][2] float64
static double *particle_tape_at(const fb_model *m, int step, int stage) { return m->pt_tape + ((size_t)step * 4 + stage) * 2 * (size_t)m->pt_n; }

static PartGeo part_geo(const fb_ctx *c)
{
    PartGeo g;
    g.dx = (double)c->lx / c->nx; g.dy = (double)c->ly / c->ny; g.nx = c->nx; g.ny = c->ny;
    return g;
}

// One RK stage of the particles, at the top of the step's stage `stage`, where tracer_stage runs: before the step's own stage
// overwrites ZB.  The vorticity's state of the stage (tracer_stage: ZA at stage 0, ZB afterwards, a masked mode from ZA) goes into
// the 3-pass layout (k_tracer_vstate_* into field 1 of the record workspace where the state arrays are laid out otherwise; read in
// place where they are not); k_particle_uv_spec leaves the spectra of u and v in the fields 0 and 1; the backward x pass of both and
// one ROW_INV row pass each, with the scales of record(), into the particles' own real fields; k_particle_stage.  One GPU or a slab
// of one rank: one column group, no exchange.
static int particle_stage(fb_model *m, int stage)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    cf *z = m->rec_work[0];
    const cf *v0, *v1;
    int rc;
    if ((rc = stage_vstate(m, 0, stage > 0, z + n, &v0, &v1))) return rc;
    if ((rc = launch_n(c, k_particle_uv_spec, n, coef, v0, v1, z, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
    if ((rc = spectra_to_real(c, z, 2, (long)n, m->pt_uv, 1.0f / (float)nr, 0))) return rc;      // u = -dpsi/dy (record(), REC_U), v = dpsi/dx
    const PartGeo pg = part_geo(c);
    const float *u = m->pt_uv, *v = m->pt_uv + nr;
    const double dt = (double)m->dt;
    if (m->pt_depth) {                                      // the position this stage starts from into the particle tape's next slot
        if (m->pt_fill >= m->pt_depth) return fail(FB_EINVAL, "fb_model_step: the particle tape is full (fb_model_particle_tape)");   // (step_refusals comes first)
        const double *from = m->pt + (stage == 0 ? 0 : 2 * (size_t)m->pt_n);
        if ((rc = launch_n(c, k_particle_pack, (size_t)m->pt_n, from, from + m->pt_n, particle_tape_at(m, m->pt_fill, stage), m->pt_n))) return rc;
    }
    if (m->pd)                                              // positions and the deformation gradient in one pass, in k_particle_stage's place
        return dispatch<4>(stage, [&](auto S) { return launch_n(c, k_particle_stage_def<S()>, (size_t)m->pt_n, pg, u, v, m->pt, m->pd, m->pt_n, dt); });
    return dispatch<4>(stage, [&](auto S) { return launch_n(c, k_particle_stage<S()>, (size_t)m->pt_n, pg, u, v, m->pt, m->pt_n, dt); });
}

// The particles in (d_xy == NULL removes them).  The vorticity, a tracer and `primed` stay as they are.  As tracer_in: the captured
// step is dropped and the next fb_model_step starts with an eager step before the longer step is captured.  The record workspace is
// grown to its largest size first (advect_workspace), so that no later record replaces the buffer a captured step reads.
static int particles_in(fb_model *m, fb_slab *s, const double *d_xy, int n)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_begin(m, m->pt_n != 0))) return rc;
    // a particle tape laid out for the same count stays, emptied: it followed the particles that go.  Another count frees it.
    double *tape = d_xy && n == m->pt_n ? m->pt_tape : nullptr;
    const int depth = m->pt_depth;
    if (tape) m->pt_tape = nullptr;
    particles_free(m);
    if (tape) { m->pt_tape = tape; m->pt_depth = depth; }
    if (!d_xy) return FB_OK;
    if ((rc = advect_workspace(m, s))) return rc;
    if ((rc = dev_alloc((void **)&m->pt, 6 * (size_t)n * sizeof(double), "particle allocation failed")) ||
        (rc = dev_alloc((void **)&m->pt_uv, 2 * (size_t)c->nx * c->ny * sizeof(float), "particle allocation failed"))) {
        particles_free(m);
        return rc;
    }
    HIPCHK(hipMemsetAsync(m->pt, 0, 6 * (size_t)n * sizeof(double), c->stream));
    if ((rc = launch_n(c, k_particle_unpack, (size_t)n, d_xy, m->pt, m->pt + n, n))) return rc;
    m->pt_n = n;
    return FB_OK;
}

static int particles_out(fb_model *m, double *d_xy)
{
    fb_ctx *c = m->c;
    return launch_n(c, k_particle_pack, (size_t)m->pt_n, (const double *)m->pt, (const double *)(m->pt + m->pt_n), d_xy, m->pt_n);
}

static int sample(fb_ctx *c, const float *d_field, const double *d_xy, int n, double *d_out)
{
    return launch_n(c, k_sample, (size_t)n, part_geo(c), d_field, d_xy, n, d_out);
}

// a slab of one rank goes through the same code; on several ranks the particles are refused
constexpr unsigned PARTICLES = NEED_TRANSPORT | ONE_RANK_PARTICLES;
static bool particle_count_ok(int n) { return n >= 1 && n <= FB_PARTICLES_MAX; }

static int set_particles(const Call &k, const double *d_xy, int n)
{
    if (!d_xy && n != 0) return refuse(k, "NULL positions with n > 0");
    if (d_xy && !particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (int rc = enter(k, PARTICLES)) return rc;
    return particles_in(k.m, k.s, d_xy, n);
}
extern "C" int fb_model_set_particles(fb_model *m, const double *d_xy, int n) { return set_particles(on_model("fb_model_set_particles", m), d_xy, n); }
extern "C" int fb_slab_set_particles(fb_slab *s, const double *d_xy, int n) { return set_particles(on_slab("fb_slab_set_particles", s), d_xy, n); }

static int get_particles(const Call &k, double *d_xy)
{
    if (!d_xy) return refuse(k, "NULL output");
    if (int rc = enter(k, PARTICLES | NEED_PARTICLES)) return rc;
    return particles_out(k.m, d_xy);
}
extern "C" int fb_model_get_particles(fb_model *m, double *d_xy) { return get_particles(on_model("fb_model_get_particles", m), d_xy); }
extern "C" int fb_slab_get_particles(fb_slab *s, double *d_xy) { return get_particles(on_slab("fb_slab_get_particles", s), d_xy); }

// (0 on a slab of several ranks, which can have none, and before the slab is connected)
static int particle_count(const Call &k, int *n)
{
    if (!n) return refuse(k, "NULL output");
    if (int rc = enter(k)) return rc;
    *n = k.m->pt_n;
    return FB_OK;
}
extern "C" int fb_model_particle_count(fb_model *m, int *n) { return particle_count(on_model("fb_model_particle_count", m), n); }
extern "C" int fb_slab_particle_count(fb_slab *s, int *n) { return particle_count(on_slab("fb_slab_particle_count", s), n); }

// (the handle's refusals first, for once: EngineSlab.sample asks a slab of several ranks for its refusal before it shapes any buffer)
static int sample(const Call &k, const float *d_field, const double *d_xy, int n, double *d_out)
{
    if (int rc = enter(k, PARTICLES)) return rc;
    if (!d_field || !d_xy || !d_out) return refuse(k, "NULL field, positions or output");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    return sample(k.m->c, d_field, d_xy, n, d_out);
}
extern "C" int fb_model_sample(fb_model *m, const float *d_field, const double *d_xy, int n, double *d_out)
{
    return sample(on_model("fb_model_sample", m), d_field, d_xy, n, d_out);
}
extern "C" int fb_slab_sample(fb_slab *s, const float *d_field, const double *d_xy, int n, double *d_out)
{
    return sample(on_slab("fb_slab_sample", s), d_field, d_xy, n, d_out);
}

// ---- the particles' deformation gradient and its stretching (kernels: fb_particles.h) ----
// on: F = I for every particle and the elapsed time 0, allocating the twelve arrays where they are not there (so it is the reset
// too: F grows like exp(lambda t)); off: freed.  As particles_in, the captured step is dropped: the step's particle kernel changes.
static int deformation_in(fb_model *m, bool on)
{
    fb_ctx *c = m->c;
    const size_t n = (size_t)m->pt_n;
    int rc;
    if ((rc = beside_begin(m, !on && m->pd))) return rc;
    if (!on) { dev_free(m->pd); return FB_OK; }
    if (!m->pd && (rc = dev_alloc((void **)&m->pd, 12 * n * sizeof(double), "particle deformation: allocation failed"))) return rc;
    HIPCHK(hipMemsetAsync(m->pd, 0, 12 * n * sizeof(double), c->stream));
    if ((rc = launch_n(c, k_particle_def_init, n, m->pd, m->pt_n))) return rc;
    m->pd_steps0 = m->steps;
    return FB_OK;
}

constexpr unsigned DEFORMATION = PARTICLES | NEED_PARTICLES | NEED_DEFORMATION;

static int set_particle_deformation(const Call &k, int on)
{
    if (on != 0 && on != 1) return refuse(k, "on must be 0 or 1");
    if (int rc = enter(k, PARTICLES | NEED_PARTICLES)) return rc;
    return deformation_in(k.m, on == 1);
}
extern "C" int fb_model_set_particle_deformation(fb_model *m, int on) { return set_particle_deformation(on_model("fb_model_set_particle_deformation", m), on); }
extern "C" int fb_slab_set_particle_deformation(fb_slab *s, int on) { return set_particle_deformation(on_slab("fb_slab_set_particle_deformation", s), on); }

static int get_particle_deformation(const Call &k, double *d_F, double *elapsed)
{
    if (!d_F) return refuse(k, "NULL output");
    if (int rc = enter(k, DEFORMATION)) return rc;
    fb_model *m = k.m;
    if (elapsed) *elapsed = (double)(m->steps - m->pd_steps0) * (double)m->dt;
    return launch_n(m->c, k_particle_def_pack, (size_t)m->pt_n, (const double *)m->pd, d_F, m->pt_n);
}
extern "C" int fb_model_get_particle_deformation(fb_model *m, double *d_F, double *elapsed)
{
    return get_particle_deformation(on_model("fb_model_get_particle_deformation", m), d_F, elapsed);
}
extern "C" int fb_slab_get_particle_deformation(fb_slab *s, double *d_F, double *elapsed)
{
    return get_particle_deformation(on_slab("fb_slab_get_particle_deformation", s), d_F, elapsed);
}

// d_F == NULL: the model's own F, read where it lies (SoA), and its own n; else any [n][4], as sample takes any positions (and as
// sample the handle's refusals first: ModelSurface.particle_stretching asks a slab of several ranks for its refusal before it shapes
// any buffer)
static int particle_stretching(const Call &k, const double *d_F, int n, double *d_out)
{
    if (int rc = enter(k, d_F ? PARTICLES : DEFORMATION)) return rc;
    if (!d_out) return refuse(k, "NULL output");
    if (d_F && !particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    fb_model *m = k.m;
    if (!d_F) return launch_n(m->c, k_particle_stretching, (size_t)m->pt_n, (const double *)m->pd, (size_t)m->pt_n, (size_t)1, m->pt_n, d_out);
    return launch_n(m->c, k_particle_stretching, (size_t)n, d_F, (size_t)1, (size_t)4, n, d_out);
}
extern "C" int fb_model_particle_stretching(fb_model *m, const double *d_F, int n, double *d_out)
{
    return particle_stretching(on_model("fb_model_particle_stretching", m), d_F, n, d_out);
}
extern "C" int fb_slab_particle_stretching(fb_slab *s, const double *d_F, int n, double *d_out)
{
    return particle_stretching(on_slab("fb_slab_particle_stretching", s), d_F, n, d_out);
}

// ---- the particle tape and the particle adjoint (kernels: fb_lagrangian.h; particle_tape_free, particle_adjoint_free: above) ----
// the tape (64 bytes per particle and step of its depth); the adjoint's eight arrays and its two accumulators with their head
static size_t lagrangian_bytes(const fb_model *m)
{
    const fb_ctx *c = m->c;
    size_t n = (size_t)m->pt_depth * 4 * 2 * (size_t)m->pt_n * sizeof(double);
    if (m->pa) n += 8 * (size_t)m->pt_n * sizeof(double) + (4 * (size_t)c->nx * c->ny + 2) * sizeof(unsigned long long);
    return n;
}

// The tape on (depth >= 1: room for depth steps x 4 stage positions) or off (depth == 0); either way it starts empty.  While it is on
// fb_model_step steps eagerly, as it does while the adjoint's tape is on: particle_stage writes another slot at every stage, which a
// captured step would bake in.  So the captured step is dropped here (beside_begin).  A failure leaves no tape allocated.
static int particle_tape(fb_model *m, int depth)
{
    int rc;
    if ((rc = beside_begin(m, m->pt_tape != nullptr))) return rc;
    particle_tape_free(m);
    if (depth == 0) return FB_OK;
    if ((rc = dev_alloc((void **)&m->pt_tape, (size_t)depth * 4 * 2 * (size_t)m->pt_n * sizeof(double), "the particle tape: allocation failed"))) return rc;
    m->pt_depth = depth;
    return FB_OK;
}

// Xb in (d_xb: [pt_n][2] float64; NULL removes it), with the stage arrays zeroed and the accumulators of the deposit.  A particle
// adjoint that goes may still be read by a queued sweep.  The step's launches do not depend on any of it: the captured step stays.
static int particle_adjoint_in(fb_model *m, const double *d_xb)
{
    fb_ctx *c = m->c;
    const size_t cells = (size_t)c->nx * c->ny;
    if (!d_xb) {
        if (m->pa) HIPCHK(hipStreamSynchronize(c->stream));
        particle_adjoint_free(m);
        return FB_OK;
    }
    int rc;
    if ((rc = rec_alloc((void **)&m->pa, 8 * (size_t)m->pt_n * sizeof(double))) || (rc = rec_alloc((void **)&m->pa_acc, (4 * cells + 2) * sizeof(unsigned long long)))) {
        particle_adjoint_free(m);
        return rc;
    }
    return launch_n(c, k_particle_adjoint_in, (size_t)m->pt_n, d_xb, m->pa, m->pt_n);
}

// The particles' part of a backward stage, between the ROW_INV passes and k_adjoint_prod: p, q and the recurrences from u and v in
// the fields 1 and 2 of ad_real, which k_adjoint_prod overwrites next.  xs: the stage's slot of the particle tape.
static int lagrangian_stage(fb_model *m, int stage, const double *xs)
{
    fb_ctx *c = m->c;
    const size_t nr = (size_t)c->nx * c->ny;
    const float *u = m->ad_real + nr, *v = m->ad_real + 2 * nr;
    const PartGeo pg = part_geo(c);
    const double dt = (double)m->dt;
    return dispatch<4>(stage, [&](auto S) { return launch_n(c, k_particle_adjoint<S()>, (size_t)m->pt_n, pg, u, v, xs, m->pa, m->pt_n, dt); });
}

// ... and after k_adjoint_prod, before the ROW_FWD passes: p_x and p_y spread from xs into the two accumulators (max |p| on the device,
// the integer atomics), and the fold into the real fields zeta_x mu~ (field 3) and zeta_y mu~ (field 4).  The limbs are zero on the way
// in (lagrangian_begin) and zero again on the way out (k_scatter_fold); the head is zeroed here.
static int lagrangian_deposit(fb_model *m, const double *xs)
{
    fb_ctx *c = m->c;
    const size_t cells = (size_t)c->nx * c->ny, N = (size_t)m->pt_n;
    unsigned long long *acc = m->pa_acc, *head = acc + 4 * cells;
    const double *px = m->pa + 2 * N, *py = m->pa + 3 * N;
    int rc;
    HIPCHK(hipMemsetAsync(head, 0, 2 * sizeof(unsigned long long), c->stream));
    if ((rc = launch_n(c, k_obs_wmax, N, px, m->pt_n, head)) || (rc = launch_n(c, k_obs_wmax, N, py, m->pt_n, head))) return rc;
    if ((rc = launch_n(c, k_scatter_pair, N, part_geo(c), xs, px, py, m->pt_n, acc, cells, (const unsigned long long *)head))) return rc;
    return launch_n(c, k_scatter_fold, cells, acc, (const unsigned long long *)head, m->pt_n, m->ad_real + 3 * cells, m->ad_real + 4 * cells, cells);
}

// before the first stage of a sweep: the limbs zeroed, whatever an earlier sweep that failed half way has left in them
static int lagrangian_begin(fb_model *m)
{
    fb_ctx *c = m->c;
    HIPCHK(hipMemsetAsync(m->pa_acc, 0, (4 * (size_t)c->nx * c->ny + 2) * sizeof(unsigned long long), c->stream));
    return FB_OK;
}

// (depth needs no handle; the tape needs particles unless it is only freed)
static int particle_tape(const Call &k, int depth)
{
    if (depth < 0 || depth > (1 << 20)) return refuse(k, "depth outside [0, 2^20]");
    if (int rc = enter(k, depth ? PARTICLES | NEED_PARTICLES : PARTICLES)) return rc;
    return particle_tape(k.m, depth);
}
extern "C" int fb_model_particle_tape(fb_model *m, int depth) { return particle_tape(on_model("fb_model_particle_tape", m), depth); }
extern "C" int fb_slab_particle_tape(fb_slab *s, int depth) { return particle_tape(on_slab("fb_slab_particle_tape", s), depth); }

// (0, 0 while there is none: not a refusal)
static int particle_tape_count(const Call &k, int *count, int *depth)
{
    if (!count || !depth) return refuse(k, "NULL output");
    if (int rc = enter(k, PARTICLES)) return rc;
    *count = k.m->pt_fill;
    *depth = k.m->pt_depth;
    return FB_OK;
}
extern "C" int fb_model_particle_tape_count(fb_model *m, int *count, int *depth) { return particle_tape_count(on_model("fb_model_particle_tape_count", m), count, depth); }
extern "C" int fb_slab_particle_tape_count(fb_slab *s, int *count, int *depth) { return particle_tape_count(on_slab("fb_slab_particle_tape_count", s), count, depth); }

// (NULL removes it; without particles there is none to remove either: the refusal is the particles')
static int set_particle_adjoint(const Call &k, const double *d_xbar)
{
    if (int rc = enter(k, PARTICLES | NEED_PARTICLES)) return rc;
    return particle_adjoint_in(k.m, d_xbar);
}
extern "C" int fb_model_set_particle_adjoint(fb_model *m, const double *d_xbar) { return set_particle_adjoint(on_model("fb_model_set_particle_adjoint", m), d_xbar); }
extern "C" int fb_slab_set_particle_adjoint(fb_slab *s, const double *d_xbar) { return set_particle_adjoint(on_slab("fb_slab_set_particle_adjoint", s), d_xbar); }

static int get_particle_adjoint(const Call &k, double *d_xbar)
{
    if (!d_xbar) return refuse(k, "NULL output");
    if (int rc = enter(k, PARTICLES | NEED_PARTICLES)) return rc;
    fb_model *m = k.m;
    if (!m->pa) return refuse(k, "no particle adjoint is set (fb_model_set_particle_adjoint)");
    return launch_n(m->c, k_particle_pack, (size_t)m->pt_n, (const double *)m->pa, (const double *)(m->pa + m->pt_n), d_xbar, m->pt_n);
}
extern "C" int fb_model_get_particle_adjoint(fb_model *m, double *d_xbar) { return get_particle_adjoint(on_model("fb_model_get_particle_adjoint", m), d_xbar); }
extern "C" int fb_slab_get_particle_adjoint(fb_slab *s, double *d_xbar) { return get_particle_adjoint(on_slab("fb_slab_get_particle_adjoint", s), d_xbar); }

