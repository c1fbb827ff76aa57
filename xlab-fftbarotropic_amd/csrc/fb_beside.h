// fb_beside.h -- the fields stepped beside the vorticity: the host path they share, the passive tracer, and what the step and the
// model's end know of all of them (included by fftbaro.hip after fb_record.h; C ABI: include/fftbaro.h).  One header per model,
// included below where the shared path ends: fb_beside_tangent.h (the tangent set, its inner products and QR, the basis tape and the
// combination), fb_beside_particles.h (the particles, their deformation gradient, their tape and their adjoint), fb_beside_adjoint.h
// (the adjoint's tape and checkpoints, the adjoint and its set, the sweep, the tangent replay, the observations).  Kernels:
// fb_tracer.h, fb_tangent.h, fb_clv.h, fb_particles.h, fb_lagrangian.h, fb_adjoint.h, fb_replay.h, fb_obs.h.  And the split stage that
// follows a step once forcing, drag or hyperviscosity is set: fb_beside_forcing.h (kernels: fb_forcing.h).
//
// Each is taken in between two steps and advanced at the top of every RK stage of fb_model_step and fb_slab_step, from the state the
// vorticity's stage starts from, through the record workspace (record_advect, fb_record.h): the step's own buffers are only read.  A
// spectral field of this kind (struct Beside, fftbaro.hip: the tracer, each perturbation of the tangent's set, each adjoint variable)
// has one host path: beside_in, per stage beside_advect once per advective tendency and one beside_update, beside_free; a set of
// them (struct BesideSet: the tangent subspace, the adjoint subspace) set_in, set_out, set_count, set_free.  The particles share
// stage_vstate and beside_begin.
#pragma once

static void beside_free(Beside &f)
{
    for (int g = 0; g < 3; ++g) { dev_free(f.c0[g]); dev_free(f.c1[g]); dev_free(f.acc[g]); }
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
    int rc;
    if (m->xpass != XP_COLS) rc = launch(c, k_tracer_vstate_full, dim3(c->max_wg), dim3(256), 0, coef, *v0, *v1, vx, c->P, c->N1, c->N2, (c->ny / 2) / 8, (int)m->xpass);
    else if (state_tm(c)) rc = launch_n(c, k_tracer_vstate_tm, grp_elems(c, G), coef, *v0, *v1, vx, G.ncols, c->N1, c->N2, G.ky0);
    else return FB_OK;
    *v0 = *v1 = vx;
    return rc;
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
        return launch_n(c, k_advect_deriv, n / 2, coef, p[0][0], p[0][1], p[1][0], p[1][1], z, (long)n, G.ncols, c->N1, c->N2, G.ky0);
    };
    return record_advect(m, s, fill);
}

// The RK stage update of f per group of active columns (k_beside_update over the column tiles that hold a mode inside the circle),
// from the tendency record_advect has just left (advect_out), with j1 != NULL summed with an earlier one saved in j1[g].  j0 != NULL
// (one rank, so one group: the tangent replay): the tendency lies there instead.  Where every mode is masked nothing is launched.
template <int NJ> static int beside_update_nj(fb_model *m, fb_slab *s, int stage, Beside &f, const cf *j0, cf *const *j1, float kappa)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    if (j0 && c->nact > 1) return fail(FB_EINVAL, "beside_update: one tendency for several column groups");
    for (int g = 0; g < c->nact; ++g) {
        const ColGroup &G = c->grp[g];
        const int ncr = 16 * G.nct_active;
        if (grp_elems(c, G) == 0 || ncr == 0) continue;
        const cf *jh = j0 ? j0 : advect_out(m, s, g), *ja = NJ == 2 ? j1[g] : jh, *jb = NJ == 2 ? jh : nullptr;     // NJ == 1: the second is never read
        cf *c0 = f.c0[g], *c1 = f.c1[g], *ac = f.acc[g];
        const int rc = dispatch<4>(stage, [&](auto S) {
            return launch_n(c, k_beside_update<S(), NJ>, (size_t)c->nx * ncr / 2, coef, ja, jb, c0, c1, ac, kappa, m->dt, G.ncols, ncr, c->N1, c->N2, G.ky0);
        });
        if (rc) return rc;
    }
    return FB_OK;
}
static int beside_update(fb_model *m, fb_slab *s, int stage, Beside &f, cf *const *j1, float kappa)
{
    return j1 ? beside_update_nj<2>(m, s, stage, f, nullptr, j1, kappa) : beside_update_nj<1>(m, s, stage, f, nullptr, j1, kappa);
}

// f(g, n) for each of the first ngroups column groups that has elements, n (complex) of them; the first status that is not FB_OK ends it
template <class F> static int each_group(const fb_ctx *c, int ngroups, F &&f)
{
    for (int g = 0; g < ngroups; ++g)
        if (const size_t n = grp_elems(c, c->grp[g]))
            if (int rc = f(g, n)) return rc;
    return FB_OK;
}

// readField + r2c of a second real field as state_in takes the vorticity (ROW_FWD, the transpose on a slab, the forward x pass),
// through the record workspace: the half spectrum of column group g is left in rec_work[g], in the 3-pass layout, pad columns zero.
static int beside_r2c(fb_model *m, fb_slab *s, const float *d_rows)
{
    fb_ctx *c = m->c;
    const bool xchg = s && c->world > 1;
    int rc;
    if ((rc = advect_workspace(m, s))) return rc;
    RowArgs a = row_args_base(c);
    a.rin = d_rows;
    if (xchg) {
        const cf *ts[3] = {m->rec_send[0], m->rec_send[1], m->rec_send[2]};
        a.T = view_slab(c, ts, 1);
    } else {                                                // one rank: one column group, the whole of it here
        HIPCHK(hipMemsetAsync(m->rec_work[0], 0, priv_elems(c) * sizeof(cf), c->stream));      // pad columns zero
        return real_to_spectra(c, d_rows, m->rec_work[0], 1, 0);
    }
    if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
    if (xchg && (rc = slab_rows_to_cols(s, m->rec_send, m->rec_work, c->ngroups))) return rc;
    return each_group(c, c->ngroups, [&](int g, size_t) -> int {
        const ColGroup &G = c->grp[g];
        cf *t = m->rec_work[g];
        if (int r = launch_col_strided<-1>(c, G, t, 1, 0)) return r;
        return launch_col_block<-1>(c, G, t, 1, 0);
    });
}

// beside_r2c of a real field into the field's own arrays in the 3-pass layout: the base c0 of every column group, and for the
// groups of active columns the stage state c1 and the accumulator acc, zeroed.
static int beside_in(fb_model *m, fb_slab *s, const float *d_rows, Beside &f)
{
    fb_ctx *c = m->c;
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
    if ((rc = beside_r2c(m, s, d_rows))) return rc;
    return each_group(c, c->ngroups, [&](int g, size_t n) -> int {
        HIPCHK(hipMemcpyAsync(f.c0[g], m->rec_work[g], n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
        return FB_OK;
    });
}

// ---- a set of such fields (struct BesideSet, fftbaro.hip): the tangent subspace and the adjoint subspace ----
static void set_free(BesideSet &S)
{
    for (Beside &f : S.v) beside_free(f);
    S.n = 0;
}

// `count` fields in, d_rows [count] real fields one after the other (beside_in each); whatever set was there is replaced, fields beyond
// `count` freed.  A failure leaves the fields it got to: the caller frees the set.
static int set_in(fb_model *m, fb_slab *s, const float *d_rows, int count, BesideSet &S)
{
    const fb_ctx *c = m->c;
    for (int k = 0; k < count; ++k)
        if (int rc = beside_in(m, s, d_rows + (size_t)k * c->XL * c->ny, S.v[k])) return rc;
    for (int k = count; k < S.n; ++k) beside_free(S.v[k]);
    S.n = count;
    return FB_OK;
}

// ---- the entry points of a field and of a set, behind the guards `needs` ----
// the real field of a field stepped beside the vorticity (f(m): its base arrays, in the 3-pass layout), as the
// vorticity's own record
static int get_beside(const Call &k, unsigned needs, Beside *(*f)(fb_model *), float *d_rows)
{
    if (!d_rows) return refuse(k, "NULL output");
    if (int rc = enter(k, needs)) return rc;
    return record(k.m, k.s, REC_VORT, d_rows, nullptr, f(k.m)->c0);
}

// [count] fields in through the model's `in` (tangent_in, adjoint_in; NULL removes the whole set)
static int set_fields(const Call &k, unsigned needs, int (*in)(fb_model *, fb_slab *, const float *, int), const float *d_rows, int count)
{
    if (d_rows && (count < 1 || count > BesideSet::MAX)) return refuse(k, "count outside [1, 32]");
    if (int rc = enter(k, needs)) return rc;
    return in(k.m, k.s, d_rows, count);
}

// every field of the set out, [n] real fields one after the other, each as get_beside's one
static int set_out(const Call &k, unsigned needs, BesideSet fb_model::*set, float *d_rows)
{
    if (!d_rows) return refuse(k, "NULL output");
    if (int rc = enter(k, needs)) return rc;
    const fb_ctx *c = k.m->c;
    const BesideSet &S = k.m->*set;
    for (int v = 0; v < S.n; ++v)
        if (int rc = record(k.m, k.s, REC_VORT, d_rows + (size_t)v * c->XL * c->ny, nullptr, S.v[v].c0)) return rc;
    return FB_OK;
}

// (0 while none is set: not a refusal)
static int set_count(const Call &k, unsigned needs, BesideSet fb_model::*set, int *count)
{
    if (!count) return refuse(k, "NULL output");
    if (int rc = enter(k, needs)) return rc;
    *count = (k.m->*set).n;
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

// collective on a slab of several ranks, as fb_slab_set_vort_local
static int set_tracer(const Call &k, const float *d_rows, float kappa)
{
    if (!(kappa >= 0.0f) || !std::isfinite(kappa)) return refuse(k, "kappa must be finite and >= 0");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return tracer_in(k.m, k.s, d_rows, kappa);
}
extern "C" int fb_model_set_tracer(fb_model *m, const float *d_c_real, float kappa) { return set_tracer(on_model("fb_model_set_tracer", m), d_c_real, kappa); }
extern "C" int fb_slab_set_tracer_local(fb_slab *s, const float *d_rows, float kappa) { return set_tracer(on_slab("fb_slab_set_tracer_local", s), d_rows, kappa); }

static int get_tracer(const Call &k, float *d_rows) { return get_beside(k, NEED_TRANSPORT | NEED_TRACER, [](fb_model *m) { return &m->tr; }, d_rows); }
extern "C" int fb_model_get_tracer(fb_model *m, float *d_c_real) { return get_tracer(on_model("fb_model_get_tracer", m), d_c_real); }
extern "C" int fb_slab_get_tracer_local(fb_slab *s, float *d_rows) { return get_tracer(on_slab("fb_slab_get_tracer_local", s), d_rows); }

// the pair's body is the vorticity's (get_eddy_diffusivity, fb_record.h) with the tracer in its place
extern "C" int fb_model_get_tracer_eddy_diffusivity(fb_model *m, int nbins, double *d_table, float *d_c, float *d_grad2)
{
    return get_eddy_diffusivity(on_model("fb_model_get_tracer_eddy_diffusivity", m), NEED_TRACER, nbins, d_table, d_c, d_grad2);
}
extern "C" int fb_slab_get_tracer_eddy_diffusivity(fb_slab *s, int nbins, double *d_table, float *d_c_rows, float *d_grad2_rows)
{
    return get_eddy_diffusivity(on_slab("fb_slab_get_tracer_eddy_diffusivity", s), NEED_TRACER, nbins, d_table, d_c_rows, d_grad2_rows);
}

#include "fb_beside_tangent.h"
#include "fb_beside_particles.h"
#include "fb_beside_adjoint.h"
#include "fb_beside_forcing.h"

// ---- what the step and the model's end know of all of them (declared in fftbaro.hip) ----
// At the top of RK stage `stage`, from the state the vorticity's stage starts from: the tracer's stage, the particles', the
// tangent-linear model's, and the state into the adjoint's tape (the last three on one rank only: their set calls refuse more).
static int beside_stage(fb_model *m, fb_slab *s, int stage)
{
    int rc;
    if (m->ck_replay) return adjoint_stash(m, stage);       // a segment of a checkpointed window run again: the vorticity alone moves
    if (m->tracer && (rc = tracer_stage(m, s, stage))) return rc;
    if (m->pt_n && (rc = particle_stage(m, stage))) return rc;
    if (m->tg.n && (rc = tangent_stage(m, s, stage))) return rc;
    if (m->ad_on && (rc = adjoint_stash(m, stage))) return rc;
    return FB_OK;
}

static void beside_step_done(fb_model *m)
{
    if (m->ad_on) m->ad_top = ++m->ad_fill;                 // the four stage states of this step are on the tape, and nothing above them
    if (m->pt_depth && m->pt_n && !m->ck_replay) ++m->pt_fill;      // and its four stage positions on the particles'
}

static void beside_free_all(fb_model *m)
{
    tracer_free(m);
    particles_free(m);
    tangent_free(m);
    adjoint_free(m);
    adjoint_tape_free(m);
    obs_free(m);
    forcing_free(m);
}
