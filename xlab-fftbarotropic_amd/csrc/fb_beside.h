// fb_beside.h -- the fields stepped beside the vorticity: the passive tracer, the tangent-linear model and the Lagrangian particles
// (included by fftbaro.hip after fb_record.h; kernels: fb_tracer.h, fb_tangent.h, fb_particles.h; C ABI: include/fftbaro.h).
//
// Each is taken in between two steps and advanced at the top of every RK stage of fb_model_step and fb_slab_step, from the state the
// vorticity's stage starts from, through the record workspace (record_advect, fb_record.h): the step's own buffers are only read.  A
// spectral field of this kind (struct Beside, fftbaro.hip: the tracer, the perturbation) has one host path: beside_in, per stage
// beside_advect once per advective tendency and one beside_update, beside_free.  The particles share stage_vstate and beside_begin.
#pragma once

static void beside_free(Beside &f)
{
    for (int g = 0; g < 3; ++g) {
        cf **arr[] = {&f.c0[g], &f.c1[g], &f.acc[g]};
        for (cf **p : arr) if (*p) { hipFree(*p); *p = nullptr; }
    }
}

// What setting or removing any of them starts with: the captured step is dropped and the next fb_model_step starts with an eager
// step, which launches every kernel of the changed step once before it is captured (launch_lds).  going: arrays that a queued step
// may still use are about to be freed.  The vorticity, its derivative fields, `primed` and the other fields stay as they are.
static int beside_begin(fb_model *m, bool going)
{
    model_drop_graph(m);
    m->warmed = false;
    if (going) HIPCHK(hipStreamSynchronize(m->c->stream));
    return FB_OK;
}

// The vorticity's state of an RK stage of column group g in the 3-pass layout: *v0 the base, *v1 the stage state (staged: ZB, else
// the base itself), a masked mode to be read from *v0.  Where the step keeps its state arrays in a layout of its own,
// k_tracer_vstate_* merges the two into `vx` (a field of the record workspace) and both point there.
static int stage_vstate(fb_model *m, int g, bool staged, cf *vx, const cf **v0, const cf **v1)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[g];
    const SpecCoef coef = make_coef(c);
    *v0 = m->gb[g].ZA; *v1 = staged ? m->gb[g].ZB : m->gb[g].ZA;
    if (m->xpass != XP_COLS)
        hipLaunchKernelGGL(k_tracer_vstate_full, dim3(c->max_wg), dim3(256), 0, c->stream, coef, *v0, *v1, vx, c->P, c->N1, c->N2, (c->ny / 2) / 8, (int)m->xpass);
    else if (state_tm(c))
        hipLaunchKernelGGL(k_tracer_vstate_tm, dim3(grid_for(c, grp_elems(c, G))), dim3(256), 0, c->stream, coef, *v0, *v1, vx, G.ncols, c->N1, c->N2, G.ky0);
    else return FB_OK;
    HIPCHK(hipGetLastError());
    *v0 = *v1 = vx;
    return FB_OK;
}

// The advective tendency r2c(J(a; psi of b)) of an RK stage through record_advect, at the top of the step's stage `stage`; a, b: a
// field stepped beside the vorticity, or NULL for the vorticity itself.  The vorticity's state of this stage is vort_c0 (ZA) at stage 0
// and the stage state ZB afterwards (k_col_mid and k_col_full store it at every stage below 3), a Beside's its base and its stage state
// likewise.  Launches per column group: k_tracer_vstate_* (where the state arrays are not in the 3-pass layout) into field 2, which
// k_advect_deriv reads before it writes there, then k_advect_deriv.  On a slab the exchanges are record_advect's, on the streams and
// events the records use.  The result: advect_out(m, s, g).
static int beside_advect(fb_model *m, fb_slab *s, int stage, const Beside *a, const Beside *b)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    auto fill = [&](int g, const ColGroup &G, cf *z, size_t n) -> int {
        const bool staged = stage > 0 && g < c->nact;       // the frozen columns' state is the base at every stage
        const Beside *f[2] = {a, b};
        const cf *p[2][2];
        for (int k = 0; k < 2; ++k) {
            if (f[k]) { p[k][0] = f[k]->c0[g]; p[k][1] = staged ? f[k]->c1[g] : f[k]->c0[g]; }
            else if (int r = stage_vstate(m, g, staged, z + 2 * n, &p[k][0], &p[k][1])) return r;
        }
        hipLaunchKernelGGL(k_advect_deriv, dim3(grid_for(c, n / 2)), dim3(256), 0, c->stream, coef, p[0][0], p[0][1], p[1][0], p[1][1], z, (long)n, G.ncols, c->N1,
                           c->N2, G.ky0);
        HIPCHK(hipGetLastError());
        return FB_OK;
    };
    return record_advect(m, s, fill);
}

// The RK stage update of f per group of active columns (k_beside_update over the column tiles that hold a mode inside the circle),
// from the tendency record_advect has just left (advect_out), with j1 != NULL summed with an earlier one saved in j1[g].
template <int NJ> static int beside_update_nj(fb_model *m, fb_slab *s, int stage, Beside &f, cf *const *j1, float kappa)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    for (int g = 0; g < c->nact; ++g) {
        const ColGroup &G = c->grp[g];
        const int ncr = 16 * G.nct_active;
        if (grp_elems(c, G) == 0 || ncr == 0) continue;
        const dim3 grid(grid_for(c, (size_t)c->nx * ncr / 2)), blk(256);
        const cf *jh = advect_out(m, s, g), *ja = NJ == 2 ? j1[g] : jh, *jb = NJ == 2 ? jh : nullptr;     // NJ == 1: the second is never read
        cf *c0 = f.c0[g], *c1 = f.c1[g], *ac = f.acc[g];
        switch (stage) {
        case 0: hipLaunchKernelGGL((k_beside_update<0, NJ>), grid, blk, 0, c->stream, coef, ja, jb, c0, c1, ac, kappa, m->dt, G.ncols, ncr, c->N1, c->N2, G.ky0); break;
        case 1: hipLaunchKernelGGL((k_beside_update<1, NJ>), grid, blk, 0, c->stream, coef, ja, jb, c0, c1, ac, kappa, m->dt, G.ncols, ncr, c->N1, c->N2, G.ky0); break;
        case 2: hipLaunchKernelGGL((k_beside_update<2, NJ>), grid, blk, 0, c->stream, coef, ja, jb, c0, c1, ac, kappa, m->dt, G.ncols, ncr, c->N1, c->N2, G.ky0); break;
        default: hipLaunchKernelGGL((k_beside_update<3, NJ>), grid, blk, 0, c->stream, coef, ja, jb, c0, c1, ac, kappa, m->dt, G.ncols, ncr, c->N1, c->N2, G.ky0); break;
        }
        HIPCHK(hipGetLastError());
    }
    return FB_OK;
}
static int beside_update(fb_model *m, fb_slab *s, int stage, Beside &f, cf *const *j1, float kappa)
{
    return j1 ? beside_update_nj<2>(m, s, stage, f, j1, kappa) : beside_update_nj<1>(m, s, stage, f, j1, kappa);
}

// readField + r2c of a second real field as state_in takes the vorticity (ROW_FWD, the transpose on a slab, the forward x pass),
// through the record workspace into the field's own arrays in the 3-pass layout: the base c0 of every column group, and for the
// groups of active columns the stage state c1 and the accumulator acc, zeroed.
static int beside_in(fb_model *m, fb_slab *s, const float *d_rows, Beside &f)
{
    fb_ctx *c = m->c;
    const bool xchg = s && c->world > 1;
    int rc;
    if ((rc = advect_workspace(m, s))) return rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const size_t n = grp_elems(c, c->grp[g]);
        if (n == 0) continue;
        void **p[3] = {(void **)&f.c0[g], (void **)&f.c1[g], (void **)&f.acc[g]};
        if ((rc = rec_alloc(p[0], n * sizeof(cf))) || (g < c->nact && ((rc = rec_alloc(p[1], n * sizeof(cf))) || (rc = rec_alloc(p[2], n * sizeof(cf)))))) return rc;
        if (g < c->nact) {                                  // pad columns and the columns beyond the last active tile stay zero
            HIPCHK(hipMemsetAsync(f.c1[g], 0, n * sizeof(cf), c->stream));
            HIPCHK(hipMemsetAsync(f.acc[g], 0, n * sizeof(cf), c->stream));
        }
    }
    RowArgs a = row_args_base(c);
    a.rin = d_rows;
    if (xchg) {
        const cf *ts[3] = {m->rec_send[0], m->rec_send[1], m->rec_send[2]};
        a.T = view_slab(c, ts, 1);
    } else {
        HIPCHK(hipMemsetAsync(m->rec_work[0], 0, priv_elems(c) * sizeof(cf), c->stream));      // pad columns zero
        a.T = view_single(c, m->rec_work[0], 0);
    }
    if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
    if (xchg && (rc = slab_rows_to_cols(s, m->rec_send, m->rec_work, c->ngroups))) return rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        cf *t = m->rec_work[g];
        if ((rc = launch_col_strided<-1>(c, G, t, 1, 0)) || (rc = launch_col_block<-1>(c, G, t, 1, 0))) return rc;
        HIPCHK(hipMemcpyAsync(f.c0[g], t, n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
    }
    return FB_OK;
}

// ---- the passive tracer (kernels: fb_tracer.h) ----
static void tracer_free(fb_model *m)
{
    beside_free(m->tr);
    m->tracer = false;
}

// One RK stage of the tracer: J(c; psi), then the update with the tracer's own diffusivity.
static int tracer_stage(fb_model *m, fb_slab *s, int stage)
{
    int rc;
    if ((rc = beside_advect(m, s, stage, &m->tr, nullptr))) return rc;
    return beside_update(m, s, stage, m->tr, nullptr, m->kappa);
}

// The tracer in (beside_begin, beside_in); d_rows == NULL removes the tracer.
static int tracer_in(fb_model *m, fb_slab *s, const float *d_rows, float kappa)
{
    int rc;
    if ((rc = beside_begin(m, !d_rows && m->tracer))) return rc;
    if (!d_rows) { tracer_free(m); return FB_OK; }
    if ((rc = beside_in(m, s, d_rows, m->tr))) { tracer_free(m); return rc; }
    m->kappa = kappa;
    m->tracer = true;
    return FB_OK;
}

static int kappa_check(const char *fn, float kappa)
{
    if (!(kappa >= 0.0f) || !std::isfinite(kappa)) return fail(FB_EINVAL, std::string(fn) + ": kappa must be finite and >= 0");
    return FB_OK;
}

extern "C" int fb_model_set_tracer(fb_model *m, const float *d_c_real, float kappa)
{
    if (!m) return fail(FB_EINVAL, "fb_model_set_tracer: NULL model");
    int rc;
    if ((rc = kappa_check("fb_model_set_tracer", kappa))) return rc;
    NEED_SINGLE(m->c);
    return tracer_in(m, nullptr, d_c_real, kappa);
}

extern "C" int fb_model_get_tracer(fb_model *m, float *d_c_real)
{
    if (!m || !d_c_real) return fail(FB_EINVAL, "fb_model_get_tracer: NULL");
    if (!m->tracer) return fail(FB_EINVAL, "fb_model_get_tracer: no tracer is set");
    NEED_SINGLE(m->c);
    return record(m, nullptr, REC_VORT, d_c_real, nullptr, m->tr.c0);
}

extern "C" int fb_model_get_tracer_eddy_diffusivity(fb_model *m, int nbins, double *d_table, float *d_c, float *d_grad2)
{
    if (!m) return fail(FB_EINVAL, "fb_model_get_tracer_eddy_diffusivity: NULL model");
    int rc;
    if ((rc = keff_check("fb_model_get_tracer_eddy_diffusivity", d_table, nbins))) return rc;
    if (!m->tracer) return fail(FB_EINVAL, "fb_model_get_tracer_eddy_diffusivity: no tracer is set");
    NEED_SINGLE(m->c);
    return record_keff(m, nullptr, nbins, d_table, d_c, d_grad2, m->tr.c0, m->kappa);
}

// collective on a slab of several ranks, as fb_slab_set_vort_local
extern "C" int fb_slab_set_tracer_local(fb_slab *s, const float *d_rows, float kappa)
{
    if (!s) return fail(FB_EINVAL, "fb_slab_set_tracer_local: NULL slab");
    int rc;
    if ((rc = kappa_check("fb_slab_set_tracer_local", kappa))) return rc;
    SLAB_READY(s);
    return tracer_in(s->m, s, d_rows, kappa);
}

extern "C" int fb_slab_get_tracer_local(fb_slab *s, float *d_rows)
{
    if (!s || !d_rows) return fail(FB_EINVAL, "fb_slab_get_tracer_local: NULL");
    if (!s->m->tracer) return fail(FB_EINVAL, "fb_slab_get_tracer_local: no tracer is set");
    SLAB_READY(s);
    return record(s->m, s, REC_VORT, d_rows, nullptr, s->m->tr.c0);
}

// collective, as fb_slab_get_eddy_diffusivity
extern "C" int fb_slab_get_tracer_eddy_diffusivity(fb_slab *s, int nbins, double *d_table, float *d_c_rows, float *d_grad2_rows)
{
    if (!s) return fail(FB_EINVAL, "fb_slab_get_tracer_eddy_diffusivity: NULL slab");
    int rc;
    if ((rc = keff_check("fb_slab_get_tracer_eddy_diffusivity", d_table, nbins))) return rc;
    if (!s->m->tracer) return fail(FB_EINVAL, "fb_slab_get_tracer_eddy_diffusivity: no tracer is set");
    SLAB_READY(s);
    return record_keff(s->m, s, nbins, d_table, d_c_rows, d_grad2_rows, s->m->tr.c0, s->m->kappa);
}

// ---- the tangent-linear model (kernels: fb_tangent.h) ----
static void tangent_free(fb_model *m)
{
    beside_free(m->tg);
    for (cf *&p : m->tg_j) if (p) { hipFree(p); p = nullptr; }
    if (m->tg_red) { hipFree(m->tg_red); m->tg_red = nullptr; }
    m->tangent = false;
}

// One RK stage of the perturbation, where tracer_stage runs and from the same states.  The tangent of the bilinear J is two advect
// passes, J(dz; psi) + J(zeta; dpsi); the first pass's result is copied to tg_j before the second overwrites the record workspace;
// then the update with both and the model's nu.
static int tangent_stage(fb_model *m, fb_slab *s, int stage)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_advect(m, s, stage, &m->tg, nullptr))) return rc;
    for (int g = 0; g < c->nact; ++g) {
        const size_t n = grp_elems(c, c->grp[g]);
        if (n) HIPCHK(hipMemcpyAsync(m->tg_j[g], advect_out(m, s, g), n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = beside_advect(m, s, stage, nullptr, &m->tg))) return rc;
    return beside_update(m, s, stage, m->tg, m->tg_j, m->nu);
}

// The perturbation in (beside_begin, beside_in) with the scratch of the first advect pass and the partial sums of the norm
// ([ngroups][max_wg] float64); d_rows == NULL removes it.
static int tangent_in(fb_model *m, fb_slab *s, const float *d_rows)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_begin(m, !d_rows && m->tangent))) return rc;
    if (!d_rows) { tangent_free(m); return FB_OK; }
    for (int g = 0; g < c->nact && !rc; ++g)
        if (grp_elems(c, c->grp[g])) rc = rec_alloc((void **)&m->tg_j[g], grp_elems(c, c->grp[g]) * sizeof(cf));
    if (!rc) rc = rec_alloc((void **)&m->tg_red, (size_t)c->ngroups * c->max_wg * sizeof(double));
    if (rc || (rc = beside_in(m, s, d_rows, m->tg))) { tangent_free(m); return rc; }
    m->tangent = true;
    return FB_OK;
}

// kind 0: the enstrophy norm <dz^2> / 2, kind 1: the energy norm <|grad dpsi|^2> / 2 (means over the grid), of the resident spectrum
// (k_tangent_norm per column group, then k_tangent_norm_final over every partial sum) into *d_out on the device
static int tangent_norm(fb_model *m, int kind, double *d_out)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    int np = 0;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        const int nwg = grid_for(c, n / 2);
        hipLaunchKernelGGL(k_tangent_norm, dim3(nwg), dim3(256), 0, c->stream, coef, (const cf *)m->tg.c0[g], kind, G.ncols, c->N1, c->N2, G.ky0, m->tg_red + np);
        HIPCHK(hipGetLastError());
        np += nwg;
    }
    const double grids = (double)c->nx * c->ny;
    hipLaunchKernelGGL(k_tangent_norm_final, dim3(1), dim3(256), 0, c->stream, (const double *)m->tg_red, np, 0.5 / (grids * grids), d_out);
    HIPCHK(hipGetLastError());
    return FB_OK;
}

static int tangent_scale(fb_model *m, float a)
{
    fb_ctx *c = m->c;
    for (int g = 0; g < c->ngroups; ++g) {
        const size_t n = grp_elems(c, c->grp[g]);
        if (n == 0) continue;
        hipLaunchKernelGGL(k_tangent_scale, dim3(grid_for(c, n / 2)), dim3(256), 0, c->stream, m->tg.c0[g], n, a);
        HIPCHK(hipGetLastError());
    }
    return FB_OK;
}

// what the entry points refuse before any HIP call
static int tangent_check(const char *fn, const fb_model *m, bool need_set)
{
    if (!m) return fail(FB_EINVAL, std::string(fn) + ": NULL model");
    if (need_set && !m->tangent) return fail(FB_EINVAL, std::string(fn) + ": no tangent is set");
    return FB_OK;
}
static int tangent_norm_check(const char *fn, int kind, const double *d_out)
{
    if (kind != 0 && kind != 1) return fail(FB_EINVAL, std::string(fn) + ": kind must be 0 (enstrophy) or 1 (energy)");
    if (!d_out) return fail(FB_EINVAL, std::string(fn) + ": NULL output");
    return FB_OK;
}
static int tangent_scale_check(const char *fn, float a)
{
    if (!std::isfinite(a) || a == 0.0f) return fail(FB_EINVAL, std::string(fn) + ": the factor must be finite and not zero");
    return FB_OK;
}

extern "C" int fb_model_set_tangent(fb_model *m, const float *d_dz_real)
{
    int rc;
    if ((rc = tangent_check("fb_model_set_tangent", m, false))) return rc;
    NEED_SINGLE(m->c);
    return tangent_in(m, nullptr, d_dz_real);
}

extern "C" int fb_model_get_tangent(fb_model *m, float *d_dz_real)
{
    int rc;
    if (!d_dz_real) return fail(FB_EINVAL, "fb_model_get_tangent: NULL");
    if ((rc = tangent_check("fb_model_get_tangent", m, true))) return rc;
    NEED_SINGLE(m->c);
    return record(m, nullptr, REC_VORT, d_dz_real, nullptr, m->tg.c0);
}

extern "C" int fb_model_tangent_norm(fb_model *m, int kind, double *d_out)
{
    int rc;
    if ((rc = tangent_norm_check("fb_model_tangent_norm", kind, d_out)) || (rc = tangent_check("fb_model_tangent_norm", m, true))) return rc;
    NEED_SINGLE(m->c);
    return tangent_norm(m, kind, d_out);
}

extern "C" int fb_model_tangent_scale(fb_model *m, float a)
{
    int rc;
    if ((rc = tangent_scale_check("fb_model_tangent_scale", a)) || (rc = tangent_check("fb_model_tangent_scale", m, true))) return rc;
    NEED_SINGLE(m->c);
    return tangent_scale(m, a);
}

// a slab of one rank goes through the same code; on several ranks the tangent-linear model is refused
#define SLAB_TANGENT_ONE_RANK(s, fn) do { if (!(s)) return fail(FB_EINVAL, std::string(fn) + ": NULL slab"); if ((s)->c->world > 1) return fail(FB_EINVAL, std::string(fn) + ": the tangent-linear model is not supported on a slab of several ranks (world > 1)"); } while (0)

extern "C" int fb_slab_set_tangent(fb_slab *s, const float *d_dz_real)
{
    SLAB_TANGENT_ONE_RANK(s, "fb_slab_set_tangent");
    SLAB_READY(s);
    return tangent_in(s->m, s, d_dz_real);
}

extern "C" int fb_slab_get_tangent(fb_slab *s, float *d_dz_real)
{
    SLAB_TANGENT_ONE_RANK(s, "fb_slab_get_tangent");
    int rc;
    if (!d_dz_real) return fail(FB_EINVAL, "fb_slab_get_tangent: NULL");
    if ((rc = tangent_check("fb_slab_get_tangent", s->m, true))) return rc;
    SLAB_READY(s);
    return record(s->m, s, REC_VORT, d_dz_real, nullptr, s->m->tg.c0);
}

extern "C" int fb_slab_tangent_norm(fb_slab *s, int kind, double *d_out)
{
    SLAB_TANGENT_ONE_RANK(s, "fb_slab_tangent_norm");
    int rc;
    if ((rc = tangent_norm_check("fb_slab_tangent_norm", kind, d_out)) || (rc = tangent_check("fb_slab_tangent_norm", s->m, true))) return rc;
    return tangent_norm(s->m, kind, d_out);
}

extern "C" int fb_slab_tangent_scale(fb_slab *s, float a)
{
    SLAB_TANGENT_ONE_RANK(s, "fb_slab_tangent_scale");
    int rc;
    if ((rc = tangent_scale_check("fb_slab_tangent_scale", a)) || (rc = tangent_check("fb_slab_tangent_scale", s->m, true))) return rc;
    return tangent_scale(s->m, a);
}

// ---- the Lagrangian particles (kernels: fb_particles.h) ----
#define FB_PARTICLES_MAX (1 << 24)

static void particles_free(fb_model *m)
{
    if (m->pt) { hipFree(m->pt); m->pt = nullptr; }
    if (m->pt_uv) { hipFree(m->pt_uv); m->pt_uv = nullptr; }
    m->pt_n = 0;
}

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
    hipLaunchKernelGGL(k_particle_uv_spec, dim3(grid_for(c, n)), dim3(256), 0, c->stream, coef, v0, v1, z, (long)n, G.ncols, c->N1, c->N2, G.ky0);
    HIPCHK(hipGetLastError());
    if ((rc = launch_col_block<+1>(c, G, z, 2, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 2, (long)n))) return rc;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    RowArgs a = row_args_base(c);
    a.M = view_single(c, z, (long)n); a.scale = -g; a.rout = m->pt_uv;                // u = -dpsi/dy (record(), REC_U)
    if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    a.M = view_single(c, z + n, (long)n); a.scale = g; a.rout = m->pt_uv + nr;        // v = dpsi/dx
    if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    const dim3 grid(grid_for(c, (size_t)m->pt_n)), blk(256);
    const PartGeo pg = part_geo(c);
    const float *u = m->pt_uv, *v = m->pt_uv + nr;
    const double dt = (double)m->dt;
    switch (stage) {
    case 0: hipLaunchKernelGGL((k_particle_stage<0>), grid, blk, 0, c->stream, pg, u, v, m->pt, m->pt_n, dt); break;
    case 1: hipLaunchKernelGGL((k_particle_stage<1>), grid, blk, 0, c->stream, pg, u, v, m->pt, m->pt_n, dt); break;
    case 2: hipLaunchKernelGGL((k_particle_stage<2>), grid, blk, 0, c->stream, pg, u, v, m->pt, m->pt_n, dt); break;
    default: hipLaunchKernelGGL((k_particle_stage<3>), grid, blk, 0, c->stream, pg, u, v, m->pt, m->pt_n, dt); break;
    }
    HIPCHK(hipGetLastError());
    return FB_OK;
}

static int particles_check(const char *fn, const double *d_xy, int n)
{
    if (!d_xy) return n == 0 ? FB_OK : fail(FB_EINVAL, std::string(fn) + ": NULL positions with n > 0");
    if (n < 1 || n > FB_PARTICLES_MAX) return fail(FB_EINVAL, std::string(fn) + ": n outside [1, 2^24]");
    return FB_OK;
}

// The particles in (d_xy == NULL removes them).  The vorticity, a tracer and `primed` stay as they are.  As tracer_in: the captured
// step is dropped and the next fb_model_step starts with an eager step before the longer step is captured.  The record workspace is
// grown to its largest size first (advect_workspace), so that no later record replaces the buffer a captured step reads.
static int particles_in(fb_model *m, fb_slab *s, const double *d_xy, int n)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_begin(m, m->pt_n != 0))) return rc;
    particles_free(m);
    if (!d_xy) return FB_OK;
    if ((rc = advect_workspace(m, s))) return rc;
    if (hipMalloc((void **)&m->pt, 6 * (size_t)n * sizeof(double)) != hipSuccess) { m->pt = nullptr; return fail(FB_ENOMEM, "particle allocation failed"); }
    if (hipMalloc((void **)&m->pt_uv, 2 * (size_t)c->nx * c->ny * sizeof(float)) != hipSuccess) {
        m->pt_uv = nullptr;
        particles_free(m);
        return fail(FB_ENOMEM, "particle allocation failed");
    }
    HIPCHK(hipMemsetAsync(m->pt, 0, 6 * (size_t)n * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_particle_unpack, dim3(grid_for(c, (size_t)n)), dim3(256), 0, c->stream, d_xy, m->pt, m->pt + n, n);
    HIPCHK(hipGetLastError());
    m->pt_n = n;
    return FB_OK;
}

static int particles_out(fb_model *m, double *d_xy)
{
    fb_ctx *c = m->c;
    hipLaunchKernelGGL(k_particle_pack, dim3(grid_for(c, (size_t)m->pt_n)), dim3(256), 0, c->stream, (const double *)m->pt, (const double *)(m->pt + m->pt_n), d_xy, m->pt_n);
    HIPCHK(hipGetLastError());
    return FB_OK;
}

static int sample_check(const char *fn, const float *d_field, const double *d_xy, int n, const double *d_out)
{
    if (!d_field || !d_xy || !d_out) return fail(FB_EINVAL, std::string(fn) + ": NULL");
    if (n < 1 || n > FB_PARTICLES_MAX) return fail(FB_EINVAL, std::string(fn) + ": n outside [1, 2^24]");
    return FB_OK;
}

static int sample(fb_ctx *c, const float *d_field, const double *d_xy, int n, double *d_out)
{
    hipLaunchKernelGGL(k_sample, dim3(grid_for(c, (size_t)n)), dim3(256), 0, c->stream, part_geo(c), d_field, d_xy, n, d_out);
    HIPCHK(hipGetLastError());
    return FB_OK;
}

extern "C" int fb_model_set_particles(fb_model *m, const double *d_xy, int n)
{
    if (!m) return fail(FB_EINVAL, "fb_model_set_particles: NULL model");
    int rc;
    if ((rc = particles_check("fb_model_set_particles", d_xy, n))) return rc;
    NEED_SINGLE(m->c);
    if (m->phase_flow) return fail(FB_EINVAL, "fb_model_set_particles on a slab model: use fb_slab_set_particles");
    return particles_in(m, nullptr, d_xy, n);
}

extern "C" int fb_model_get_particles(fb_model *m, double *d_xy)
{
    if (!m || !d_xy) return fail(FB_EINVAL, "fb_model_get_particles: NULL");
    if (!m->pt_n) return fail(FB_EINVAL, "fb_model_get_particles: no particles are set");
    return particles_out(m, d_xy);
}

extern "C" int fb_model_particle_count(fb_model *m, int *n)
{
    if (!m || !n) return fail(FB_EINVAL, "fb_model_particle_count: NULL");
    *n = m->pt_n;
    return FB_OK;
}

extern "C" int fb_model_sample(fb_model *m, const float *d_field, const double *d_xy, int n, double *d_out)
{
    if (!m) return fail(FB_EINVAL, "fb_model_sample: NULL model");
    int rc;
    if ((rc = sample_check("fb_model_sample", d_field, d_xy, n, d_out))) return rc;
    NEED_SINGLE(m->c);
    return sample(m->c, d_field, d_xy, n, d_out);
}

// a slab of one rank goes through the same code; particles distributed over row slabs would need neighbour halo rows that the
// all-to-all transport does not provide
#define SLAB_PARTICLES_ONE_RANK(s, fn) do { if ((s)->c->world > 1) return fail(FB_EUNSUPPORTED, std::string(fn) + ": particles are not supported on a slab of several ranks (world > 1)"); } while (0)

extern "C" int fb_slab_set_particles(fb_slab *s, const double *d_xy, int n)
{
    if (!s) return fail(FB_EINVAL, "fb_slab_set_particles: NULL slab");
    SLAB_PARTICLES_ONE_RANK(s, "fb_slab_set_particles");
    int rc;
    if ((rc = particles_check("fb_slab_set_particles", d_xy, n))) return rc;
    SLAB_READY(s);
    return particles_in(s->m, s, d_xy, n);
}

extern "C" int fb_slab_get_particles(fb_slab *s, double *d_xy)
{
    if (!s) return fail(FB_EINVAL, "fb_slab_get_particles: NULL slab");
    SLAB_PARTICLES_ONE_RANK(s, "fb_slab_get_particles");
    if (!d_xy) return fail(FB_EINVAL, "fb_slab_get_particles: NULL");
    if (!s->m->pt_n) return fail(FB_EINVAL, "fb_slab_get_particles: no particles are set");
    return particles_out(s->m, d_xy);
}

extern "C" int fb_slab_particle_count(fb_slab *s, int *n)
{
    if (!s || !n) return fail(FB_EINVAL, "fb_slab_particle_count: NULL");
    *n = s->m->pt_n;
    return FB_OK;
}

extern "C" int fb_slab_sample(fb_slab *s, const float *d_field, const double *d_xy, int n, double *d_out)
{
    if (!s) return fail(FB_EINVAL, "fb_slab_sample: NULL slab");
    SLAB_PARTICLES_ONE_RANK(s, "fb_slab_sample");
    int rc;
    if ((rc = sample_check("fb_slab_sample", d_field, d_xy, n, d_out))) return rc;
    return sample(s->c, d_field, d_xy, n, d_out);
}

// ---- the adjoint model (kernels: fb_adjoint.h) ----
// One GPU or a slab of one rank: one column group, no exchange (as the particles).
static void adjoint_tape_free(fb_model *m)
{
    if (m->ad_tape) { hipFree(m->ad_tape); m->ad_tape = nullptr; }
    m->ad_depth = m->ad_fill = 0;
}

static void adjoint_free(fb_model *m)
{
    beside_free(m->ad);
    if (m->ad_real) { hipFree(m->ad_real); m->ad_real = nullptr; }
    m->adjoint = false;
}

// a step call that would overrun the tape is refused before anything is launched
static int adjoint_room(const fb_model *m, int nsteps, const char *fn)
{
    if (m->ad_depth && nsteps > m->ad_depth - m->ad_fill)
        return fail(FB_EINVAL, std::string(fn) + ": the adjoint's tape has room for " + std::to_string(m->ad_depth - m->ad_fill) + " more steps (fb_model_adjoint_record)");
    return FB_OK;
}

// The tape on (depth >= 1: room for depth steps x 4 stage states) or off (depth == 0); either way it starts empty.  While it is on
// fb_model_step steps eagerly, so the captured step is dropped here (beside_begin) and never holds a slot of the tape.
static int adjoint_record(fb_model *m, int depth)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_begin(m, m->ad_tape != nullptr))) return rc;
    adjoint_tape_free(m);
    if (depth == 0) return FB_OK;
    const size_t n = grp_elems(c, c->grp[0]);
    if (hipMalloc((void **)&m->ad_tape, (size_t)depth * 4 * n * sizeof(cf)) != hipSuccess) {
        m->ad_tape = nullptr;
        (void)hipGetLastError();
        return fail(FB_ENOMEM, "the adjoint's tape: allocation failed");
    }
    m->ad_depth = depth;
    return FB_OK;
}

// The state the step's stage `stage` starts from into the tape's next slot, where tangent_stage runs: stage_vstate merges base and
// stage state into the slot itself where the step keeps its state in a layout of its own; where it hands ZA / ZB back in place,
// k_adjoint_merge does.
static int adjoint_stash(fb_model *m, int stage)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G);
    cf *slot = m->ad_tape + ((size_t)m->ad_fill * 4 + stage) * n;
    const cf *v0, *v1;
    int rc;
    if ((rc = stage_vstate(m, 0, stage > 0 && c->nact > 0, slot, &v0, &v1))) return rc;
    if (v0 == slot) return FB_OK;
    hipLaunchKernelGGL(k_adjoint_merge, dim3(grid_for(c, n / 2)), dim3(256), 0, c->stream, make_coef(c), v0, v1, slot, G.ncols, c->N1, c->N2, G.ky0);
    HIPCHK(hipGetLastError());
    return FB_OK;
}

// The adjoint variable in (beside_in: lam, with the k-bar and the accumulator of a backward step) and the real fields of the product
// pass; d_rows == NULL removes it.  The step's launches do not depend on it: the captured step stays.
static int adjoint_in(fb_model *m, fb_slab *s, const float *d_rows)
{
    fb_ctx *c = m->c;
    int rc;
    if (!d_rows) {
        if (m->adjoint) HIPCHK(hipStreamSynchronize(c->stream));
        adjoint_free(m);
        return FB_OK;
    }
    rc = rec_alloc((void **)&m->ad_real, 5 * (size_t)c->nx * c->ny * sizeof(float));
    if (rc || (rc = beside_in(m, s, d_rows, m->ad))) { adjoint_free(m); return rc; }
    m->adjoint = true;
    return FB_OK;
}

// One RK stage of a backward step: L_stage^T of the k-bar about the recorded stage state zs, then the recurrences (fb_adjoint.h).
// Five fields back to physical space as particle_stage takes u and v, with its scales; four products forward as beside_in takes a
// field; through the record workspace, which the step never reads.
static int adjoint_stage(fb_model *m, int stage, const cf *zs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    cf *z = m->rec_work[0];
    cf *lam = m->ad.c0[0], *kb = m->ad.c1[0], *acc = m->ad.acc[0];
    const dim3 grid(grid_for(c, n / 2)), blk(256);
    int rc;
    hipLaunchKernelGGL(k_adjoint_deriv, grid, blk, 0, c->stream, coef, zs, (const cf *)(stage == 3 ? lam : kb), stage == 3 ? m->dt / 6.0f : 1.0f, z, (long)n, G.ncols,
                       c->N1, c->N2, G.ky0);
    HIPCHK(hipGetLastError());
    if ((rc = launch_col_block<+1>(c, G, z, 5, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 5, (long)n))) return rc;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    for (int f = 0; f < 5; ++f) {
        RowArgs a = row_args_base(c);
        a.M = view_single(c, z + f * n, (long)n); a.scale = f == 1 ? -g : g; a.rout = m->ad_real + f * nr;      // u = -dpsi/dy (record(), REC_U)
        if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    }
    hipLaunchKernelGGL(k_adjoint_prod, dim3(grid_for(c, nr / 4)), blk, 0, c->stream, m->ad_real, nr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(z, 0, 4 * n * sizeof(cf), c->stream));                                                 // pad columns zero
    for (int f = 0; f < 4; ++f) {
        RowArgs a = row_args_base(c);
        a.rin = m->ad_real + (f + 1) * nr; a.T = view_single(c, z + f * n, 0);
        if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
    }
    if ((rc = launch_col_strided<-1>(c, G, z, 4, (long)n)) || (rc = launch_col_block<-1>(c, G, z, 4, (long)n))) return rc;
    switch (stage) {
    case 3: hipLaunchKernelGGL((k_adjoint_update<3>), grid, blk, 0, c->stream, coef, (const cf *)z, (long)n, lam, kb, acc, m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0); break;
    case 2: hipLaunchKernelGGL((k_adjoint_update<2>), grid, blk, 0, c->stream, coef, (const cf *)z, (long)n, lam, kb, acc, m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0); break;
    case 1: hipLaunchKernelGGL((k_adjoint_update<1>), grid, blk, 0, c->stream, coef, (const cf *)z, (long)n, lam, kb, acc, m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0); break;
    default: hipLaunchKernelGGL((k_adjoint_update<0>), grid, blk, 0, c->stream, coef, (const cf *)z, (long)n, lam, kb, acc, m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0); break;
    }
    HIPCHK(hipGetLastError());
    return FB_OK;
}

// The last nsteps recorded steps popped, newest first, each step's transpose applied to lam (its stages in the order 3, 2, 1, 0).
static int adjoint_back(fb_model *m, fb_slab *s, int nsteps)
{
    fb_ctx *c = m->c;
    const size_t n = grp_elems(c, c->grp[0]);
    int rc;
    if ((rc = advect_workspace(m, s))) return rc;
    for (int k = 0; k < nsteps; ++k) {
        const cf *step = m->ad_tape + (size_t)(m->ad_fill - 1) * 4 * n;
        for (int stage = 3; stage >= 0; --stage)
            if ((rc = adjoint_stage(m, stage, step + (size_t)stage * n))) return rc;
        --m->ad_fill;
    }
    return FB_OK;
}

// what the entry points refuse before any HIP call
static int adjoint_check(const char *fn, const fb_model *m, bool need_set)
{
    if (!m) return fail(FB_EINVAL, std::string(fn) + ": NULL model");
    if (need_set && !m->adjoint) return fail(FB_EINVAL, std::string(fn) + ": no adjoint is set");
    return FB_OK;
}
static int adjoint_record_check(const char *fn, int depth)
{
    if (depth < 0 || depth > (1 << 20)) return fail(FB_EINVAL, std::string(fn) + ": depth outside [0, 2^20]");
    return FB_OK;
}
static int adjoint_back_check(const char *fn, const fb_model *m, int nsteps)
{
    if (nsteps < 0) return fail(FB_EINVAL, std::string(fn) + ": nsteps < 0");
    if (int rc = adjoint_check(fn, m, true)) return rc;
    if (nsteps > m->ad_fill) return fail(FB_EINVAL, std::string(fn) + ": " + std::to_string(nsteps) + " steps asked for, " + std::to_string(m->ad_fill) + " recorded");
    return FB_OK;
}

extern "C" int fb_model_adjoint_record(fb_model *m, int depth)
{
    int rc;
    if ((rc = adjoint_record_check("fb_model_adjoint_record", depth)) || (rc = adjoint_check("fb_model_adjoint_record", m, false))) return rc;
    NEED_SINGLE(m->c);
    if (m->phase_flow) return fail(FB_EINVAL, "fb_model_adjoint_record on a slab model: use fb_slab_adjoint_record");
    return adjoint_record(m, depth);
}

extern "C" int fb_model_adjoint_recorded(fb_model *m, int *n)
{
    if (!m || !n) return fail(FB_EINVAL, "fb_model_adjoint_recorded: NULL");
    *n = m->ad_fill;
    return FB_OK;
}

extern "C" int fb_model_set_adjoint(fb_model *m, const float *d_lambda_real)
{
    int rc;
    if ((rc = adjoint_check("fb_model_set_adjoint", m, false))) return rc;
    NEED_SINGLE(m->c);
    return adjoint_in(m, nullptr, d_lambda_real);
}

extern "C" int fb_model_get_adjoint(fb_model *m, float *d_real)
{
    int rc;
    if (!d_real) return fail(FB_EINVAL, "fb_model_get_adjoint: NULL");
    if ((rc = adjoint_check("fb_model_get_adjoint", m, true))) return rc;
    NEED_SINGLE(m->c);
    return record(m, nullptr, REC_VORT, d_real, nullptr, m->ad.c0);
}

extern "C" int fb_model_adjoint_back(fb_model *m, int nsteps)
{
    int rc;
    if ((rc = adjoint_back_check("fb_model_adjoint_back", m, nsteps))) return rc;
    NEED_SINGLE(m->c);
    return adjoint_back(m, nullptr, nsteps);
}

// a slab of one rank goes through the same code; on several ranks the adjoint model is refused
#define SLAB_ADJOINT_ONE_RANK(s, fn) do { if (!(s)) return fail(FB_EINVAL, std::string(fn) + ": NULL slab"); if ((s)->c->world > 1) return fail(FB_EINVAL, std::string(fn) + ": the adjoint model is not supported on a slab of several ranks (world > 1)"); } while (0)

extern "C" int fb_slab_adjoint_record(fb_slab *s, int depth)
{
    SLAB_ADJOINT_ONE_RANK(s, "fb_slab_adjoint_record");
    int rc;
    if ((rc = adjoint_record_check("fb_slab_adjoint_record", depth))) return rc;
    SLAB_READY(s);
    return adjoint_record(s->m, depth);
}

extern "C" int fb_slab_adjoint_recorded(fb_slab *s, int *n)
{
    SLAB_ADJOINT_ONE_RANK(s, "fb_slab_adjoint_recorded");
    if (!n) return fail(FB_EINVAL, "fb_slab_adjoint_recorded: NULL");
    *n = s->m->ad_fill;
    return FB_OK;
}

extern "C" int fb_slab_set_adjoint(fb_slab *s, const float *d_lambda_real)
{
    SLAB_ADJOINT_ONE_RANK(s, "fb_slab_set_adjoint");
    SLAB_READY(s);
    return adjoint_in(s->m, s, d_lambda_real);
}

extern "C" int fb_slab_get_adjoint(fb_slab *s, float *d_real)
{
    SLAB_ADJOINT_ONE_RANK(s, "fb_slab_get_adjoint");
    int rc;
    if (!d_real) return fail(FB_EINVAL, "fb_slab_get_adjoint: NULL");
    if ((rc = adjoint_check("fb_slab_get_adjoint", s->m, true))) return rc;
    SLAB_READY(s);
    return record(s->m, s, REC_VORT, d_real, nullptr, s->m->ad.c0);
}

extern "C" int fb_slab_adjoint_back(fb_slab *s, int nsteps)
{
    SLAB_ADJOINT_ONE_RANK(s, "fb_slab_adjoint_back");
    int rc;
    if ((rc = adjoint_back_check("fb_slab_adjoint_back", s->m, nsteps))) return rc;
    SLAB_READY(s);
    return adjoint_back(s->m, s, nsteps);
}
