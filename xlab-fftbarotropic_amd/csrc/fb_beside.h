// fb_beside.h -- the fields stepped beside the vorticity: the passive tracer, the tangent-linear model and the Lagrangian particles
// (included by fftbaro.hip after fb_record.h; kernels: fb_tracer.h, fb_tangent.h, fb_clv.h, fb_particles.h, fb_adjoint.h, fb_obs.h,
// fb_lagrangian.h; C ABI: include/fftbaro.h).
//
// Each is taken in between two steps and advanced at the top of every RK stage of fb_model_step and fb_slab_step, from the state the
// vorticity's stage starts from, through the record workspace (record_advect, fb_record.h): the step's own buffers are only read.  A
// spectral field of this kind (struct Beside, fftbaro.hip: the tracer, each perturbation of the tangent's set) has one host path:
// beside_in, per stage beside_advect once per advective tendency and one beside_update, beside_free.  The particles share
// stage_vstate and beside_begin.
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
// from the tendency record_advect has just left (advect_out), with j1 != NULL summed with an earlier one saved in j1[g].
template <int NJ> static int beside_update_nj(fb_model *m, fb_slab *s, int stage, Beside &f, cf *const *j1, float kappa)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    for (int g = 0; g < c->nact; ++g) {
        const ColGroup &G = c->grp[g];
        const int ncr = 16 * G.nct_active;
        if (grp_elems(c, G) == 0 || ncr == 0) continue;
        const cf *jh = advect_out(m, s, g), *ja = NJ == 2 ? j1[g] : jh, *jb = NJ == 2 ? jh : nullptr;     // NJ == 1: the second is never read
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
    return j1 ? beside_update_nj<2>(m, s, stage, f, j1, kappa) : beside_update_nj<1>(m, s, stage, f, j1, kappa);
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
    } else {
        HIPCHK(hipMemsetAsync(m->rec_work[0], 0, priv_elems(c) * sizeof(cf), c->stream));      // pad columns zero
        a.T = view_single(c, m->rec_work[0], 0);
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

// the real field of a field stepped beside the vorticity (f(m): its base arrays, in the 3-pass layout), as the
// vorticity's own record
static int get_beside(const Call &k, unsigned needs, Beside *(*f)(fb_model *), float *d_rows)
{
    if (!d_rows) return refuse(k, "NULL output");
    if (int rc = enter(k, needs)) return rc;
    return record(k.m, k.s, REC_VORT, d_rows, nullptr, f(k.m)->c0);
}
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

// ---- the tangent-linear model (kernels: fb_tangent.h) ----
// A set of tg_n perturbations on the one trajectory; the single tangent of fb_model_set_tangent is the set of one, and its norm the
// inner product of perturbation 0 with itself.
static void tangent_tape_free(fb_model *m)
{
    for (cf *&p : m->tt) if (p) { hipFree(p); p = nullptr; }
    m->tt_depth = m->tt_fill = 0;
}

// the tangent replay's real fields (tangent_replay, below): sized for the set's count, so they go with a set that goes or changes it
static int replay_chunk(int count) { return count < REPLAY_CHUNK ? count : REPLAY_CHUNK; }
static size_t replay_real_fields(int count) { return 4 + 5 * (size_t)replay_chunk(count); }
static void replay_work_free(fb_model *m)
{
    if (m->rp_real) { hipFree(m->rp_real); m->rp_real = nullptr; }
}
static size_t replay_bytes(const fb_model *m) { return m->rp_real ? replay_real_fields(m->tg_n) * m->c->nx * m->c->ny * sizeof(float) : 0; }

// (the basis tape holds copies of this set's bases in this set's count: it goes with the set)
static void tangent_free(fb_model *m)
{
    tangent_tape_free(m);
    replay_work_free(m);
    for (Beside &f : m->tg) beside_free(f);
    for (cf *&p : m->tg_j) if (p) { hipFree(p); p = nullptr; }
    if (m->tg_red) { hipFree(m->tg_red); m->tg_red = nullptr; }
    m->tg_n = 0;
}

// One RK stage of the perturbations, where tracer_stage runs and from the same states, one perturbation after the other in index
// order.  The tangent of the bilinear J is two advect passes, J(dz; psi) + J(zeta; dpsi); the first pass's result is copied to tg_j
// before the second overwrites the record workspace; then the update with both and the model's nu.  Nothing is shared between two
// perturbations but the scratch: perturbation k of a set is bit for bit the set of one started from the same field.
static int tangent_stage(fb_model *m, fb_slab *s, int stage)
{
    fb_ctx *c = m->c;
    int rc;
    for (int k = 0; k < m->tg_n; ++k) {
        Beside &f = m->tg[k];
        if ((rc = beside_advect(m, s, stage, &f, nullptr))) return rc;
        rc = each_group(c, c->nact, [&](int g, size_t n) -> int {
            HIPCHK(hipMemcpyAsync(m->tg_j[g], advect_out(m, s, g), n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
            return FB_OK;
        });
        if (rc || (rc = beside_advect(m, s, stage, nullptr, &f))) return rc;
        if ((rc = beside_update(m, s, stage, f, m->tg_j, m->nu))) return rc;
    }
    return FB_OK;
}

// `count` perturbations in, d_rows [count] real fields one after the other (beside_begin, beside_in each), with the scratch of the
// first advect pass and the partial sums of an inner product ([ngroups][max_wg] float64); whatever set was there is replaced,
// perturbations beyond `count` freed; d_rows == NULL removes all.  The basis tape is freed with a set that goes or changes its count
// (its slots are laid out for that count); a set of the same count keeps it.
static int tangent_in(fb_model *m, fb_slab *s, const float *d_rows, int count)
{
    fb_ctx *c = m->c;
    int rc;
    const bool tape_goes = m->tt_depth && (!d_rows || count != m->tg_n);
    const bool replay_goes = m->rp_real && (!d_rows || count != m->tg_n);     // (a queued replay may still use it)
    if ((rc = beside_begin(m, (m->tg_n && (!d_rows || count < m->tg_n)) || tape_goes || replay_goes))) return rc;
    if (tape_goes) tangent_tape_free(m);
    if (replay_goes) replay_work_free(m);
    if (!d_rows) { tangent_free(m); return FB_OK; }
    rc = each_group(c, c->nact, [&](int g, size_t n) { return rec_alloc((void **)&m->tg_j[g], n * sizeof(cf)); });
    if (!rc) rc = rec_alloc((void **)&m->tg_red, (size_t)c->ngroups * c->max_wg * sizeof(double));
    for (int k = 0; k < count && !rc; ++k) rc = beside_in(m, s, d_rows + (size_t)k * c->XL * c->ny, m->tg[k]);
    if (rc) { tangent_free(m); return rc; }
    for (int k = count; k < m->tg_n; ++k) beside_free(m->tg[k]);
    m->tg_n = count;
    return FB_OK;
}

static int tangent_scale(fb_model *m, float a)
{
    fb_ctx *c = m->c;
    return each_group(c, c->ngroups, [&](int g, size_t n) { return launch_n(c, k_tangent_scale, n / 2, m->tg[0].c0[g], n, a); });
}

// <a, b> of the resident spectra of two perturbations into *d_out on the device (a may be b): kind 0 the enstrophy inner product
// <a b> / 2, kind 1 the energy one <grad psi_a . grad psi_b> / 2, means over the grid (k_tangent_dot per column group, its partial sums
// one group after the other in the one tg_red, then k_tangent_dot_final over all of them: calls follow each other on the one stream)
static int tangent_dot(fb_model *m, int kind, const Beside &a, const Beside &b, double *d_out)
{
    fb_ctx *c = m->c;
    const SpecCoef coef = make_coef(c);
    int np = 0;
    const int rc = each_group(c, c->ngroups, [&](int g, size_t n) {
        const ColGroup &G = c->grp[g];
        const int nwg = grid_for(c, n / 2), at = np;
        np += nwg;
        return launch(c, k_tangent_dot, dim3(nwg), dim3(256), 0, coef, (const cf *)a.c0[g], (const cf *)b.c0[g], kind, G.ncols, c->N1, c->N2, G.ky0, m->tg_red + at);
    });
    if (rc) return rc;
    const double grids = (double)c->nx * c->ny;
    return launch(c, k_tangent_dot_final, dim3(1), dim3(256), 0, (const double *)m->tg_red, np, 0.5 / (grids * grids), d_out);
}

// the norm of perturbation 0 into *d_out on the device: kind 0 <dz^2> / 2, kind 1 <|grad dpsi|^2> / 2
static int tangent_norm0(fb_model *m, int kind, double *d_out) { return tangent_dot(m, kind, m->tg[0], m->tg[0], d_out); }

// every <v_i, v_j> into the device array d_gram, [tg_n][tg_n] float64 row-major: the upper triangle through tangent_dot, mirrored
static int tangent_gram(fb_model *m, int kind, double *d_gram)
{
    const int M = m->tg_n;
    for (int i = 0; i < M; ++i)
        for (int j = i; j < M; ++j)
            if (int rc = tangent_dot(m, kind, m->tg[i], m->tg[j], d_gram + (size_t)i * M + j)) return rc;
    return launch(m->c, k_tangent_mirror, dim3(1), dim3(256), 0, d_gram, M);
}

// Modified Gram-Schmidt in place on the bases, in index order: for every j, r_ij = <q_i, v_j> of the CURRENT v_j and v_j -= r_ij q_i
// for i < j, then r_jj = sqrt(<v_j, v_j>) and v_j /= r_jj.  d_r, a device array [tg_n][tg_n] float64 row-major, ends upper triangular
// with v_j(old) = sum over i <= j of r_ij q_i; every coefficient is written there by one kernel and read from there by the next, so
// the host waits for nothing.  A rank-deficient set leaves a diagonal element that is not finite and positive and vectors that are
// not finite; nothing here tests for it.  The stage arrays hold no live data between two steps: only the bases change.
static int tangent_qr(fb_model *m, int kind, double *d_r)
{
    fb_ctx *c = m->c;
    const int M = m->tg_n;
    int rc;
    HIPCHK(hipMemsetAsync(d_r, 0, (size_t)M * M * sizeof(double), c->stream));
    for (int j = 0; j < M; ++j) {
        Beside &v = m->tg[j];
        for (int i = 0; i < j; ++i) {
            double *r = d_r + (size_t)i * M + j;
            if ((rc = tangent_dot(m, kind, m->tg[i], v, r))) return rc;
            rc = each_group(c, c->ngroups, [&](int g, size_t n) { return launch_n(c, k_tangent_axpy, n / 2, v.c0[g], (const cf *)m->tg[i].c0[g], n, (const double *)r); });
            if (rc) return rc;
        }
        double *r = d_r + (size_t)j * M + j;
        if ((rc = tangent_dot(m, kind, v, v, r)) || (rc = launch(c, k_tangent_sqrt, dim3(1), dim3(64), 0, r))) return rc;
        rc = each_group(c, c->ngroups, [&](int g, size_t n) { return launch_n(c, k_tangent_scale_dev, n / 2, v.c0[g], n, (const double *)r); });
        if (rc) return rc;
    }
    return FB_OK;
}

// ---- the basis tape and the combination of the covariant Lyapunov vectors (kernel: fb_clv.h) ----
// base k of slot `slot` of column group g (n = grp_elems of the group)
static cf *tangent_tape_at(const fb_model *m, int g, size_t n, int slot, int k) { return m->tt[g] + ((size_t)slot * m->tg_n + k) * n; }

// The tape on (depth >= 1 slots for the current set) or off (depth == 0); either way it starts empty.  The step reads no pointer of
// it: the captured step stays.  A tape that goes may still be read or written by queued work.
static int tangent_tape(fb_model *m, int depth)
{
    fb_ctx *c = m->c;
    if (m->tt_depth) HIPCHK(hipStreamSynchronize(c->stream));
    tangent_tape_free(m);
    if (depth == 0) return FB_OK;
    const int rc = each_group(c, c->ngroups, [&](int g, size_t n) -> int {
        if (hipMalloc((void **)&m->tt[g], (size_t)depth * m->tg_n * n * sizeof(cf)) == hipSuccess) return FB_OK;
        m->tt[g] = nullptr;
        (void)hipGetLastError();
        return fail(FB_ENOMEM, "the tangent's basis tape: allocation failed");
    });
    if (rc) { tangent_tape_free(m); return rc; }
    m->tt_depth = depth;
    return FB_OK;
}

// the bases of the live set into the next slot: device to device on the context's stream, nothing allocated
static int tangent_tape_push(fb_model *m)
{
    fb_ctx *c = m->c;
    for (int k = 0; k < m->tg_n; ++k) {
        const int rc = each_group(c, c->ngroups, [&](int g, size_t n) -> int {
            HIPCHK(hipMemcpyAsync(tangent_tape_at(m, g, n, m->tt_fill, k), m->tg[k].c0[g], n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
            return FB_OK;
        });
        if (rc) return rc;
    }
    ++m->tt_fill;
    return FB_OK;
}

// live set <- (slot >= 0: the bases of tape slot `slot`; slot == -1: the live set itself, in place) C, d_c a device array [tg_n][tg_n]
// float64 row-major: v_j = sum over i of c_ij q_i, one k_tangent_combine per column group with the smallest compile-time bound that
// holds the count.  The stage arrays hold no live data between two steps: only the bases change.
template <int MB> static int tangent_combine_mb(fb_model *m, int slot, const double *d_c)
{
    fb_ctx *c = m->c;
    const int M = m->tg_n;
    return each_group(c, c->ngroups, [&](int g, size_t n) {
        CombineArrays<MB> a = {};
        for (int k = 0; k < M; ++k) {
            a.dst[k] = m->tg[k].c0[g];
            a.src[k] = slot < 0 ? a.dst[k] : tangent_tape_at(m, g, n, slot, k);
        }
        return launch_n(c, k_tangent_combine<MB>, n / 2, a, n, M, d_c);
    });
}
static int tangent_combine(fb_model *m, int slot, const double *d_c)
{
    const int M = m->tg_n;
    return M <= 4 ? tangent_combine_mb<4>(m, slot, d_c) : M <= 8 ? tangent_combine_mb<8>(m, slot, d_c)
         : M <= 16 ? tangent_combine_mb<16>(m, slot, d_c) : tangent_combine_mb<32>(m, slot, d_c);
}
static_assert(FB_TANGENTS_MAX <= 32, "k_tangent_combine's largest instance holds 32 perturbations");

// a slab of one rank goes through the same code; on several ranks the tangent-linear model is refused
constexpr unsigned TANGENT =NEED_TRANSPORT | ONE_RANK_TANGENT, TANGENT_SET = TANGENT | NEED_TANGENT;

// [count] fields in; the single tangent's call sets one (and with NULL removes the whole set, as the set's own does)
static int set_tangents(const Call &k, const float *d_dz_real, int count)
{
    if (d_dz_real && (count < 1 || count > FB_TANGENTS_MAX)) return refuse(k, "count outside [1, 32]");
    if (int rc = enter(k, TANGENT)) return rc;
    return tangent_in(k.m, k.s, d_dz_real, count);
}
extern "C" int fb_model_set_tangent(fb_model *m, const float *d_dz_real) { return set_tangents(on_model("fb_model_set_tangent", m), d_dz_real, 1); }
extern "C" int fb_slab_set_tangent(fb_slab *s, const float *d_dz_real) { return set_tangents(on_slab("fb_slab_set_tangent", s), d_dz_real, 1); }
extern "C" int fb_model_set_tangents(fb_model *m, const float *d_dz_real, int count) { return set_tangents(on_model("fb_model_set_tangents", m), d_dz_real, count); }
extern "C" int fb_slab_set_tangents(fb_slab *s, const float *d_dz_real, int count) { return set_tangents(on_slab("fb_slab_set_tangents", s), d_dz_real, count); }

// (perturbation 0 only)
static int get_tangent(const Call &k, float *d_dz_real) { return get_beside(k, TANGENT_SET, [](fb_model *m) { return &m->tg[0]; }, d_dz_real); }
extern "C" int fb_model_get_tangent(fb_model *m, float *d_dz_real) { return get_tangent(on_model("fb_model_get_tangent", m), d_dz_real); }
extern "C" int fb_slab_get_tangent(fb_slab *s, float *d_dz_real) { return get_tangent(on_slab("fb_slab_get_tangent", s), d_dz_real); }

static int get_tangents(const Call &k, float *d_dz_real)
{
    if (!d_dz_real) return refuse(k, "NULL output");
    if (int rc = enter(k, TANGENT_SET)) return rc;
    const fb_ctx *c = k.m->c;
    for (int v = 0; v < k.m->tg_n; ++v)
        if (int rc = record(k.m, k.s, REC_VORT, d_dz_real + (size_t)v * c->XL * c->ny, nullptr, k.m->tg[v].c0)) return rc;
    return FB_OK;
}
extern "C" int fb_model_get_tangents(fb_model *m, float *d_dz_real) { return get_tangents(on_model("fb_model_get_tangents", m), d_dz_real); }
extern "C" int fb_slab_get_tangents(fb_slab *s, float *d_dz_real) { return get_tangents(on_slab("fb_slab_get_tangents", s), d_dz_real); }

// (0 while none is set: not a refusal)
static int tangent_count(const Call &k, int *count)
{
    if (!count) return refuse(k, "NULL output");
    if (int rc = enter(k, TANGENT)) return rc;
    *count = k.m->tg_n;
    return FB_OK;
}
extern "C" int fb_model_tangent_count(fb_model *m, int *count) { return tangent_count(on_model("fb_model_tangent_count", m), count); }
extern "C" int fb_slab_tangent_count(fb_slab *s, int *count) { return tangent_count(on_slab("fb_slab_tangent_count", s), count); }

static int tangent_scale(const Call &k, float a)
{
    if (!std::isfinite(a) || a == 0.0f) return refuse(k, "the factor must be finite and not zero");
    if (int rc = enter(k, TANGENT_SET)) return rc;
    return tangent_scale(k.m, a);
}
extern "C" int fb_model_tangent_scale(fb_model *m, float a) { return tangent_scale(on_model("fb_model_tangent_scale", m), a); }
extern "C" int fb_slab_tangent_scale(fb_slab *s, float a) { return tangent_scale(on_slab("fb_slab_tangent_scale", s), a); }

// tangent_norm0, tangent_gram or tangent_qr behind the guards they share
static int tangent_pairs(const Call &k, int kind, double *d_out, int (*body)(fb_model *, int, double *))
{
    if (kind != 0 && kind != 1) return refuse(k, "kind must be 0 (enstrophy) or 1 (energy)");
    if (!d_out) return refuse(k, "NULL output");
    if (int rc = enter(k, TANGENT_SET)) return rc;
    return body(k.m, kind, d_out);
}
extern "C" int fb_model_tangent_norm(fb_model *m, int kind, double *d_out) { return tangent_pairs(on_model("fb_model_tangent_norm", m), kind, d_out, tangent_norm0); }
extern "C" int fb_slab_tangent_norm(fb_slab *s, int kind, double *d_out) { return tangent_pairs(on_slab("fb_slab_tangent_norm", s), kind, d_out, tangent_norm0); }
extern "C" int fb_model_tangent_gram(fb_model *m, int kind, double *d_gram) { return tangent_pairs(on_model("fb_model_tangent_gram", m), kind, d_gram, tangent_gram); }
extern "C" int fb_slab_tangent_gram(fb_slab *s, int kind, double *d_gram) { return tangent_pairs(on_slab("fb_slab_tangent_gram", s), kind, d_gram, tangent_gram); }
extern "C" int fb_model_tangent_qr(fb_model *m, int kind, double *d_r) { return tangent_pairs(on_model("fb_model_tangent_qr", m), kind, d_r, tangent_qr); }
extern "C" int fb_slab_tangent_qr(fb_slab *s, int kind, double *d_r) { return tangent_pairs(on_slab("fb_slab_tangent_qr", s), kind, d_r, tangent_qr); }

// the basis tape: a set is needed unless the tape is only freed
static int tangent_tape(const Call &k, int depth)
{
    if (depth < 0 || depth > (1 << 20)) return refuse(k, "depth outside [0, 2^20]");
    if (int rc = enter(k, depth ? TANGENT_SET : TANGENT)) return rc;
    return tangent_tape(k.m, depth);
}
extern "C" int fb_model_tangent_tape(fb_model *m, int depth) { return tangent_tape(on_model("fb_model_tangent_tape", m), depth); }
extern "C" int fb_slab_tangent_tape(fb_slab *s, int depth) { return tangent_tape(on_slab("fb_slab_tangent_tape", s), depth); }

// (a full tape, and no tape at all, are refused before anything is launched)
static int tangent_tape_push(const Call &k)
{
    if (int rc = enter(k, TANGENT_SET)) return rc;
    if (!k.m->tt_depth) return refuse(k, "no basis tape (fb_model_tangent_tape)");
    if (k.m->tt_fill >= k.m->tt_depth) return refuse(k, "the basis tape is full: " + std::to_string(k.m->tt_depth) + " slots (fb_model_tangent_tape)");
    return tangent_tape_push(k.m);
}
extern "C" int fb_model_tangent_tape_push(fb_model *m) { return tangent_tape_push(on_model("fb_model_tangent_tape_push", m)); }
extern "C" int fb_slab_tangent_tape_push(fb_slab *s) { return tangent_tape_push(on_slab("fb_slab_tangent_tape_push", s)); }

// (0, 0 while there is none: not a refusal)
static int tangent_tape_count(const Call &k, int *count, int *depth)
{
    if (!count || !depth) return refuse(k, "NULL output");
    if (int rc = enter(k, TANGENT)) return rc;
    *count = k.m->tt_fill;
    *depth = k.m->tt_depth;
    return FB_OK;
}
extern "C" int fb_model_tangent_tape_count(fb_model *m, int *count, int *depth) { return tangent_tape_count(on_model("fb_model_tangent_tape_count", m), count, depth); }
extern "C" int fb_slab_tangent_tape_count(fb_slab *s, int *count, int *depth) { return tangent_tape_count(on_slab("fb_slab_tangent_tape_count", s), count, depth); }

// (the slot's range needs the model's state: after the handle)
static int tangent_combine(const Call &k, int slot, const double *d_c)
{
    if (!d_c) return refuse(k, "NULL coefficients");
    if (int rc = enter(k, TANGENT_SET)) return rc;
    if (slot < -1 || slot >= k.m->tt_fill) return refuse(k, "slot " + std::to_string(slot) + " outside [-1, " + std::to_string(k.m->tt_fill) + "): -1 the live set, else a pushed slot of the basis tape");
    return tangent_combine(k.m, slot, d_c);
}
extern "C" int fb_model_tangent_combine(fb_model *m, int slot, const double *d_c) { return tangent_combine(on_model("fb_model_tangent_combine", m), slot, d_c); }
extern "C" int fb_slab_tangent_combine(fb_slab *s, int slot, const double *d_c) { return tangent_combine(on_slab("fb_slab_tangent_combine", s), slot, d_c); }

// ---- the Lagrangian particles (kernels: fb_particles.h) ----
#define FB_PARTICLES_MAX (1 << 24)

static void deformation_free(fb_model *m)
{
    if (m->pd) { hipFree(m->pd); m->pd = nullptr; }
}

static void lagrangian_free(fb_model *m);

static void particles_free(fb_model *m)
{
    deformation_free(m);                                    // F belongs to the particles it was carried by
    lagrangian_free(m);                                     // and so do their tape and their adjoint
    if (m->pt) { hipFree(m->pt); m->pt = nullptr; }
    if (m->pt_uv) { hipFree(m->pt_uv); m->pt_uv = nullptr; }
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
    if ((rc = launch_col_block<+1>(c, G, z, 2, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 2, (long)n))) return rc;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    RowArgs a = row_args_base(c);
    a.M = view_single(c, z, (long)n); a.scale = -g; a.rout = m->pt_uv;                // u = -dpsi/dy (record(), REC_U)
    if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    a.M = view_single(c, z + n, (long)n); a.scale = g; a.rout = m->pt_uv + nr;        // v = dpsi/dx
    if ((rc = launch_row<ROW_INV>(c, a))) return rc;
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
    if (hipMalloc((void **)&m->pt, 6 * (size_t)n * sizeof(double)) != hipSuccess) { m->pt = nullptr; particles_free(m); return fail(FB_ENOMEM, "particle allocation failed"); }
    if (hipMalloc((void **)&m->pt_uv, 2 * (size_t)c->nx * c->ny * sizeof(float)) != hipSuccess) {
        m->pt_uv = nullptr;
        particles_free(m);
        return fail(FB_ENOMEM, "particle allocation failed");
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
    if (!on) { deformation_free(m); return FB_OK; }
    if (!m->pd && hipMalloc((void **)&m->pd, 12 * n * sizeof(double)) != hipSuccess) {
        m->pd = nullptr;
        (void)hipGetLastError();
        return fail(FB_ENOMEM, "particle deformation: allocation failed");
    }
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

// ---- the particle tape and the particle adjoint (kernels: fb_lagrangian.h) ----
static void particle_adjoint_free(fb_model *m)
{
    if (m->pa) { hipFree(m->pa); m->pa = nullptr; }
    if (m->pa_acc) { hipFree(m->pa_acc); m->pa_acc = nullptr; }
}

static void particle_tape_free(fb_model *m)
{
    if (m->pt_tape) { hipFree(m->pt_tape); m->pt_tape = nullptr; }
    m->pt_depth = m->pt_fill = 0;
}

static void lagrangian_free(fb_model *m)
{
    particle_tape_free(m);
    particle_adjoint_free(m);
}

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
    if (hipMalloc((void **)&m->pt_tape, (size_t)depth * 4 * 2 * (size_t)m->pt_n * sizeof(double)) != hipSuccess) {
        m->pt_tape = nullptr;
        (void)hipGetLastError();
        return fail(FB_ENOMEM, "the particle tape: allocation failed");
    }
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

// ---- the adjoint model (kernels: fb_adjoint.h) ----
// One GPU or a slab of one rank: one column group, no exchange (as the particles).
// (the full tape of fb_model_adjoint_record, or the segment, the checkpoints and the live copy of fb_model_adjoint_checkpoint: one
// mode at a time, and either call frees what the other held)
static void adjoint_tape_free(fb_model *m)
{
    cf **arr[] = {&m->ad_tape, &m->ck_store, &m->ck_live};
    for (cf **p : arr) if (*p) { hipFree(*p); *p = nullptr; }
    m->ad_depth = m->ck_every = m->ck_max = 0;
    m->ad_on = m->ck_replay = false;
    adjoint_window_empty(m);
}

static size_t checkpoint_slots(const fb_model *m) { return m->ck_every ? ((size_t)m->ck_max + m->ck_every - 1) / m->ck_every : 0; }

// the tape (4 half spectra per step of its depth), and under checkpointing the checkpoints and the live copy (one each)
static size_t adjoint_tape_bytes(const fb_model *m)
{
    const size_t n = grp_elems(m->c, m->c->grp[0]);
    return ((size_t)m->ad_depth * 4 + (m->ck_every ? checkpoint_slots(m) + 1 : 0)) * n * sizeof(cf);
}

// the variables of a sweep's chunk, and the real fields of the product pass, for a set of `count`: the one keeps k_adjoint_prod's five
static int adjoint_chunk(int count) { return count < ADJOINT_CHUNK ? count : ADJOINT_CHUNK; }
static size_t adjoint_real_fields(int count) { return count == 1 ? 5 : 4 + 5 * (size_t)adjoint_chunk(count); }

// (the workspace is sized for the count: it goes with a set that changes it)
static void adjoint_work_free(fb_model *m)
{
    if (m->ad_real) { hipFree(m->ad_real); m->ad_real = nullptr; }
    if (m->ad_spec) { hipFree(m->ad_spec); m->ad_spec = nullptr; }
}

static void adjoint_free(fb_model *m)
{
    for (Beside &f : m->ad) beside_free(f);
    adjoint_work_free(m);
    m->ad_n = 0;
}

// per variable 3 half spectra on the active columns and 1 on the frozen ones; the real fields; a set's chunk of mu~ spectra
static size_t adjoint_bytes(const fb_model *m)
{
    const fb_ctx *c = m->c;
    if (!m->ad_n) return 0;
    size_t n = adjoint_real_fields(m->ad_n) * c->nx * c->ny * sizeof(float);
    for (int g = 0; g < c->ngroups; ++g) n += (size_t)m->ad_n * (g < c->nact ? 3 : 1) * grp_elems(c, c->grp[g]) * sizeof(cf);
    if (m->ad_n > 1) n += (size_t)adjoint_chunk(m->ad_n) * grp_elems(c, c->grp[0]) * sizeof(cf);
    return n;
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
    m->ad_on = true;
    return FB_OK;
}

// Checkpointing on (every >= 1: a tape segment of `every` steps, room for ceil(max_steps / every) checkpoints and the live copy) or
// off (every == 0); either way the window starts empty, and a full tape that was on is gone.  A checkpoint is the state arrays of
// column group 0 as they are (ZA: the 3-pass layout, the tile-major one or k_col_full's, pad columns and frozen columns included):
// a state put back by a copy and the priming pass continues bit for bit like the state that was stepped to ("Adjoint
// checkpointing"), so the derivative fields need not be kept.  The forward run stashes nothing, so the captured step stays valid;
// it is dropped all the same, as fb_model_adjoint_record does, so that both modes start from one place.
static int adjoint_checkpoint(fb_model *m, int every, int max_steps)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = beside_begin(m, m->ad_tape != nullptr))) return rc;
    adjoint_tape_free(m);
    if (every == 0) return FB_OK;
    const size_t n = grp_elems(c, c->grp[0]);
    m->ck_every = every; m->ck_max = max_steps;
    if (hipMalloc((void **)&m->ad_tape, (size_t)every * 4 * n * sizeof(cf)) != hipSuccess) m->ad_tape = nullptr;
    else if (hipMalloc((void **)&m->ck_store, checkpoint_slots(m) * n * sizeof(cf)) != hipSuccess) m->ck_store = nullptr;
    else if (hipMalloc((void **)&m->ck_live, n * sizeof(cf)) != hipSuccess) m->ck_live = nullptr;
    if (!m->ck_live) {
        (void)hipGetLastError();
        adjoint_tape_free(m);
        return fail(FB_ENOMEM, "the adjoint's tape segment, checkpoints and live copy: allocation failed");
    }
    m->ad_depth = every;
    return FB_OK;
}

// run_steps, before a piece of at most *nsteps steps of a checkpointed window: where the piece starts on a multiple of ck_every the
// state goes into the next checkpoint (device to device on the context stream; the host waits for nothing), and the piece is cut at
// the next multiple.  step_refusals has seen to it that the window has room.
static int checkpoint_take(fb_model *m, int *nsteps)
{
    fb_ctx *c = m->c;
    const size_t n = grp_elems(c, c->grp[0]);
    const int into = m->ck_done % m->ck_every;
    if (into == 0) {
        HIPCHK(hipMemcpyAsync(m->ck_store + (size_t)(m->ck_done / m->ck_every) * n, m->gb[0].ZA, n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
        m->ck_n = m->ck_done / m->ck_every + 1;
    }
    if (*nsteps > m->ck_every - into) *nsteps = m->ck_every - into;
    return FB_OK;
}

// A kept state (a checkpoint, the live copy) back into the state arrays, as fb_model_set_spectrum puts one back after its relayout:
// the derivative fields come from the priming pass (k_col_full: the PRIME launch here; the three-kernel path: model_prime at the next
// step), and that step is an eager one.  The window stays as it is.
static int checkpoint_restore(fb_model *m, const cf *from)
{
    fb_ctx *c = m->c;
    HIPCHK(hipMemcpyAsync(m->gb[0].ZA, from, grp_elems(c, c->grp[0]) * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
    m->warmed = false;
    m->primed = 0;
    if (m->xpass == XP_COLS) return FB_OK;
    if (int rc = launch_col_full(m, 4)) return rc;
    m->primed = 2;
    return FB_OK;
}

// The tape segment filled again for the sweep: the segment that holds the newest unswept step, from its checkpoint to that step, with
// the recording on.  The steps are the eager ones of either flow and advance the vorticity alone (beside_stage, ck_replay): no
// tracer, particles, tangent; m->steps is run_steps' to count.  *saved: the live state has been put aside (the first refill of a call).
static int checkpoint_refill(fb_model *m, fb_slab *s, bool *saved)
{
    fb_ctx *c = m->c;
    const size_t n = grp_elems(c, c->grp[0]);
    int rc;
    if (!*saved) {
        HIPCHK(hipMemcpyAsync(m->ck_live, m->gb[0].ZA, n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
        *saved = true;
    }
    const int seg = (m->ck_left - 1) / m->ck_every, count = m->ck_left - seg * m->ck_every;
    if ((rc = checkpoint_restore(m, m->ck_store + (size_t)seg * n))) return rc;
    m->ad_fill = m->ad_top = 0;
    m->ad_on = m->ck_replay = true;
    rc = s ? slab_steps(s, count) : model_step_impl(m, count, nullptr);
    m->ad_on = m->ck_replay = false;
    if (rc) { m->ad_fill = m->ad_top = 0; return rc; }
    m->ck_replayed += count;
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
    return launch_n(c, k_adjoint_merge, n / 2, make_coef(c), v0, v1, slot, G.ncols, c->N1, c->N2, G.ky0);
}

// `count` adjoint variables in, d_rows [count] real fields one after the other (beside_in each: lam, with the k-bar and the
// accumulator of a backward step), and the workspace of the product pass for that count; whatever set was there is replaced,
// variables beyond `count` freed; d_rows == NULL removes all.  A set that goes or changes its count may still be read by a queued
// sweep.  The step's launches do not depend on any of it: the captured step stays.  A failure leaves nothing of the adjoint allocated.
static int adjoint_in(fb_model *m, fb_slab *s, const float *d_rows, int count)
{
    fb_ctx *c = m->c;
    if (m->ad_n && (!d_rows || count != m->ad_n)) HIPCHK(hipStreamSynchronize(c->stream));
    if (!d_rows) { adjoint_free(m); return FB_OK; }
    if (count != m->ad_n) adjoint_work_free(m);
    int rc = rec_alloc((void **)&m->ad_real, adjoint_real_fields(count) * c->nx * c->ny * sizeof(float));
    if (!rc && count > 1) rc = rec_alloc((void **)&m->ad_spec, (size_t)adjoint_chunk(count) * grp_elems(c, c->grp[0]) * sizeof(cf));
    for (int k = 0; k < count && !rc; ++k) rc = beside_in(m, s, d_rows + (size_t)k * c->XL * c->ny, m->ad[k]);
    if (rc) { adjoint_free(m); return rc; }
    for (int k = count; k < m->ad_n; ++k) beside_free(m->ad[k]);
    m->ad_n = count;
    return FB_OK;
}

// One RK stage of a backward step: L_stage^T of the k-bar about the recorded stage state zs, then the recurrences (fb_adjoint.h).
// Five fields back to physical space as particle_stage takes u and v, with its scales; four products forward as beside_in takes a
// field; through the record workspace, which the step never reads.  xs != NULL: a particle adjoint is set and xs is the stage's slot
// of the particle tape; its stage runs while u and v are whole, and its forcing is folded into two of the products (fb_lagrangian.h).
// With xs == NULL the launches are the ones a sweep has always made.
static int adjoint_stage(fb_model *m, int stage, const cf *zs, const double *xs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    cf *z = m->rec_work[0];
    cf *lam = m->ad[0].c0[0], *kb = m->ad[0].c1[0], *acc = m->ad[0].acc[0];
    int rc;
    if ((rc = launch_n(c, k_adjoint_deriv, n / 2, coef, zs, (const cf *)(stage == 3 ? lam : kb), stage == 3 ? m->dt / 6.0f : 1.0f, z, (long)n, G.ncols, c->N1, c->N2, G.ky0)))
        return rc;
    if ((rc = launch_col_block<+1>(c, G, z, 5, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 5, (long)n))) return rc;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    for (int f = 0; f < 5; ++f) {
        RowArgs a = row_args_base(c);
        a.M = view_single(c, z + f * n, (long)n); a.scale = f == 1 ? -g : g; a.rout = m->ad_real + f * nr;      // u = -dpsi/dy (record(), REC_U)
        if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    }
    if (xs && (rc = lagrangian_stage(m, stage, xs))) return rc;
    if ((rc = launch_n(c, k_adjoint_prod, nr / 4, m->ad_real, nr))) return rc;
    if (xs && (rc = lagrangian_deposit(m, xs))) return rc;
    HIPCHK(hipMemsetAsync(z, 0, 4 * n * sizeof(cf), c->stream));                                                 // pad columns zero
    for (int f = 0; f < 4; ++f) {
        RowArgs a = row_args_base(c);
        a.rin = m->ad_real + (f + 1) * nr; a.T = view_single(c, z + f * n, 0);
        if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
    }
    if ((rc = launch_col_strided<-1>(c, G, z, 4, (long)n)) || (rc = launch_col_block<-1>(c, G, z, 4, (long)n))) return rc;
    return dispatch<4>(stage, [&](auto S) {
        return launch_n(c, k_adjoint_update<S()>, n / 2, coef, (const cf *)z, (long)n, lam, kb, acc, m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0);
    });
}

// adjoint_stage for a set of ad_n > 1 variables.  u, v, zeta_x, zeta_y depend on zs alone: their four spectra (k_adjoint_base), the
// backward x pass and the four ROW_INV passes run once, into the real fields 0..3 of ad_real, which nothing below writes.  Then in
// chunks of C = min(ad_n, ADJOINT_CHUNK) variables (a chunk re-reads the four base fields once, 16 nx ny bytes): the chunk's mu~ in
// one launch into ad_spec, their backward x pass in one, a ROW_INV pass each into the real fields 4 .. 4 + C; k_adjoint_prod_set
// out of place into the 4 C fields after them; and per variable what adjoint_stage does from its products on, through the fields
// 0..3 of the record workspace.  Launches per stage: 7 + ceil(ad_n / C) * 4 + 9 ad_n.  The passes of distinct fields share no
// arithmetic, so every variable gets the bits adjoint_stage gives it.
static int adjoint_stage_set(fb_model *m, int stage, const cf *zs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    const int M = m->ad_n, C = adjoint_chunk(M);
    cf *z = m->rec_work[0], *zm = m->ad_spec;
    float *base = m->ad_real, *mu = base + 4 * nr, *prod = mu + (size_t)C * nr;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    int rc;
    if ((rc = launch_n(c, k_adjoint_base, n / 2, coef, zs, z, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
    if ((rc = launch_col_block<+1>(c, G, z, 4, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 4, (long)n))) return rc;
    for (int f = 0; f < 4; ++f) {
        RowArgs a = row_args_base(c);
        a.M = view_single(c, z + f * n, (long)n); a.scale = f == 0 ? -g : g; a.rout = base + f * nr;               // u = -dpsi/dy (record(), REC_U)
        if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    }
    for (int k0 = 0; k0 < M; k0 += C) {
        const int cnt = M - k0 < C ? M - k0 : C;
        AdjointKbars kbars = {};
        for (int k = 0; k < cnt; ++k) kbars.kb[k] = stage == 3 ? m->ad[k0 + k].c0[0] : m->ad[k0 + k].c1[0];
        if ((rc = launch_n(c, k_adjoint_mu, n / 2, coef, kbars, cnt, stage == 3 ? m->dt / 6.0f : 1.0f, zm, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
        if ((rc = launch_col_block<+1>(c, G, zm, cnt, (long)n)) || (rc = launch_col_strided<+1>(c, G, zm, cnt, (long)n))) return rc;
        for (int k = 0; k < cnt; ++k) {
            RowArgs a = row_args_base(c);
            a.M = view_single(c, zm + k * n, (long)n); a.scale = g; a.rout = mu + k * nr;
            if ((rc = launch_row<ROW_INV>(c, a))) return rc;
        }
        rc = dispatch<ADJOINT_CHUNK>(cnt - 1, [&](auto K) {
            return launch_n(c, k_adjoint_prod_set<K() + 1>, nr / 4, (const float *)base, (const float *)mu, prod, nr);
        });
        if (rc) return rc;
        for (int k = 0; k < cnt; ++k) {
            Beside &v = m->ad[k0 + k];
            HIPCHK(hipMemsetAsync(z, 0, 4 * n * sizeof(cf), c->stream));                                            // pad columns zero
            for (int f = 0; f < 4; ++f) {
                RowArgs a = row_args_base(c);
                a.rin = prod + ((size_t)k * 4 + f) * nr; a.T = view_single(c, z + f * n, 0);
                if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
            }
            if ((rc = launch_col_strided<-1>(c, G, z, 4, (long)n)) || (rc = launch_col_block<-1>(c, G, z, 4, (long)n))) return rc;
            rc = dispatch<4>(stage, [&](auto S) {
                return launch_n(c, k_adjoint_update<S()>, n / 2, coef, (const cf *)z, (long)n, v.c0[0], v.c1[0], v.acc[0], m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0);
            });
            if (rc) return rc;
        }
    }
    return FB_OK;
}

// The last nsteps recorded steps popped, newest first, each step's transpose applied to every lam (its stages in the order 3, 2, 1, 0).
// The set of one keeps adjoint_stage: its five-field passes are what a single variable has always run.  While a particle adjoint is set
// (the entry point has seen to it that the variable is one and that both tapes hold the same steps) every step pops the particle tape
// too; a segment of a checkpointed window that is run again never writes that tape, which always holds the whole window.
static int adjoint_back(fb_model *m, fb_slab *s, int nsteps)
{
    fb_ctx *c = m->c;
    const size_t n = grp_elems(c, c->grp[0]);
    int rc;
    bool saved = false;
    if ((rc = advect_workspace(m, s))) return rc;
    if (m->pa && nsteps > 0 && (rc = lagrangian_begin(m))) return rc;
    for (int k = 0; k < nsteps && !rc; ++k) {
        // a checkpointed window: an empty tape segment is filled again first; what is left of one stays for the next call
        if (m->ck_every && !m->ad_fill && (rc = checkpoint_refill(m, s, &saved))) break;
        const cf *step = m->ad_tape + (size_t)(m->ad_fill - 1) * 4 * n;
        for (int stage = 3; stage >= 0 && !rc; --stage)
            rc = m->ad_n == 1 ? adjoint_stage(m, stage, step + (size_t)stage * n, m->pa ? particle_tape_at(m, m->pt_fill - 1, stage) : nullptr)
                              : adjoint_stage_set(m, stage, step + (size_t)stage * n);
        if (rc) break;
        --m->ad_fill;
        if (m->pa) --m->pt_fill;
        if (m->ck_every) { --m->ck_left; m->ck_swept = true; }
    }
    if (saved) { const int back = checkpoint_restore(m, m->ck_live); if (!rc) rc = back; }    // the live state is back before the call returns, failed or not
    return rc;
}

// ---- the tangent replay over the adjoint's tape (kernels: fb_replay.h) ----
// One RK stage of the tangent step of every perturbation of the set about the recorded stage state zs, adjoint_stage_set's mirror
// image.  The base flow once: k_adjoint_base, the backward x pass, four ROW_INV passes into the real fields 0..3 of rp_real (u, v,
// zeta_x, zeta_y), which nothing below writes.  Then in chunks of C = min(tg_n, REPLAY_CHUNK) perturbations: per perturbation
// k_replay_deriv from its state of this stage (tangent_stage's: the base at stage 0, the stage state afterwards), the backward x pass
// and four ROW_INV passes into its four real fields (du, dv, dz_x, dz_y); per chunk k_replay_prod_set out of place into one field per
// perturbation; per perturbation its product's r2c as beside_r2c takes a field (field 0 of the record workspace zeroed, ROW_FWD, the
// forward x pass) and the tracer's k_beside_update with the model's nu, on the active column tiles only.  4 + 5 tg_n fields
// transformed and 7 + ceil(tg_n / C) + 12 tg_n launches per stage.  The passes of distinct fields share no arithmetic.
static int replay_stage(fb_model *m, int stage, const cf *zs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    const int M = m->tg_n, C = replay_chunk(M);
    cf *z = m->rec_work[0];
    float *base = m->rp_real, *pert = base + 4 * nr, *prod = pert + (size_t)C * 4 * nr;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    const bool staged = stage > 0 && c->nact > 0;
    const int ncr = 16 * G.nct_active;
    int rc;
    auto to_real = [&](float *out) -> int {                 // the fields 0..3 of the record workspace -> four real fields, the first negated
        int r;
        if ((r = launch_col_block<+1>(c, G, z, 4, (long)n)) || (r = launch_col_strided<+1>(c, G, z, 4, (long)n))) return r;
        for (int f = 0; f < 4; ++f) {
            RowArgs a = row_args_base(c);
            a.M = view_single(c, z + f * n, (long)n); a.scale = f == 0 ? -g : g; a.rout = out + f * nr;           // u = -dpsi/dy (record(), REC_U)
            if ((r = launch_row<ROW_INV>(c, a))) return r;
        }
        return FB_OK;
    };
    if ((rc = launch_n(c, k_adjoint_base, n / 2, coef, zs, z, (long)n, G.ncols, c->N1, c->N2, G.ky0)) || (rc = to_real(base))) return rc;
    for (int k0 = 0; k0 < M; k0 += C) {
        const int cnt = M - k0 < C ? M - k0 : C;
        for (int k = 0; k < cnt; ++k) {
            const Beside &f = m->tg[k0 + k];
            if ((rc = launch_n(c, k_replay_deriv, n / 2, coef, (const cf *)f.c0[0], (const cf *)(staged ? f.c1[0] : f.c0[0]), z, (long)n, G.ncols, c->N1, c->N2, G.ky0)) ||
                (rc = to_real(pert + (size_t)k * 4 * nr)))
                return rc;
        }
        rc = dispatch<REPLAY_CHUNK>(cnt - 1, [&](auto K) {
            return launch_n(c, k_replay_prod_set<K() + 1>, nr / 4, (const float *)base, (const float *)pert, prod, nr);
        });
        if (rc) return rc;
        for (int k = 0; k < cnt; ++k) {
            Beside &f = m->tg[k0 + k];
            HIPCHK(hipMemsetAsync(z, 0, n * sizeof(cf), c->stream));                                                // pad columns zero
            RowArgs a = row_args_base(c);
            a.rin = prod + (size_t)k * nr; a.T = view_single(c, z, 0);
            if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
            if ((rc = launch_col_strided<-1>(c, G, z, 1, 0)) || (rc = launch_col_block<-1>(c, G, z, 1, 0))) return rc;
            if (ncr == 0 || c->nact == 0) continue;         // (every mode masked: nothing evolves)
            rc = dispatch<4>(stage, [&](auto S) {
                return launch_n(c, k_beside_update<S(), 1>, (size_t)c->nx * ncr / 2, coef, (const cf *)z, (const cf *)nullptr, f.c0[0], f.c1[0], f.acc[0], m->nu, m->dt,
                                G.ncols, ncr, c->N1, c->N2, G.ky0);
            });
            if (rc) return rc;
        }
    }
    return FB_OK;
}

// The tangent step of the taped steps first .. first + nsteps - 1 (0: the oldest slot) applied to every perturbation of the set, oldest
// first, each step's stages in the order 0, 1, 2, 3.  The vorticity, a tracer, the particles, m->steps, the tape and the captured step
// are not touched: the launches lie outside the step, as a sweep's do.  The workspace is allocated here at the first replay of a set.
static int tangent_replay(fb_model *m, fb_slab *s, int first, int nsteps)
{
    fb_ctx *c = m->c;
    const size_t n = grp_elems(c, c->grp[0]);
    int rc;
    if ((rc = advect_workspace(m, s))) return rc;
    if ((rc = rec_alloc((void **)&m->rp_real, replay_real_fields(m->tg_n) * c->nx * c->ny * sizeof(float)))) return rc;
    for (int k = 0; k < nsteps; ++k) {
        const cf *step = m->ad_tape + (size_t)(first + k) * 4 * n;
        for (int stage = 0; stage < 4; ++stage)
            if ((rc = replay_stage(m, stage, step + (size_t)stage * n))) return rc;
    }
    return FB_OK;
}

// a slab of one rank goes through the same code; on several ranks the adjoint model is refused
constexpr unsigned ADJOINT = NEED_TRANSPORT | ONE_RANK_ADJOINT, ADJOINT_SET = ADJOINT | NEED_ADJOINT;

static int adjoint_record(const Call &k, int depth)
{
    if (depth < 0 || depth > (1 << 20)) return refuse(k, "depth outside [0, 2^20]");
    if (int rc = enter(k, ADJOINT)) return rc;
    return adjoint_record(k.m, depth);
}
extern "C" int fb_model_adjoint_record(fb_model *m, int depth) { return adjoint_record(on_model("fb_model_adjoint_record", m), depth); }
extern "C" int fb_slab_adjoint_record(fb_slab *s, int depth) { return adjoint_record(on_slab("fb_slab_adjoint_record", s), depth); }

static int adjoint_checkpoint(const Call &k, int every, int max_steps)
{
    if (every < 0 || every > (1 << 20)) return refuse(k, "every outside [0, 2^20]");
    if (every && max_steps < 1) return refuse(k, "max_steps < 1");
    if (every && ((long long)max_steps + every - 1) / every > (1 << 20)) return refuse(k, "more than 2^20 checkpoints (ceil(max_steps / every))");
    if (int rc = enter(k, ADJOINT)) return rc;
    return adjoint_checkpoint(k.m, every, max_steps);
}
extern "C" int fb_model_adjoint_checkpoint(fb_model *m, int every, int max_steps)
{
    return adjoint_checkpoint(on_model("fb_model_adjoint_checkpoint", m), every, max_steps);
}
extern "C" int fb_slab_adjoint_checkpoint(fb_slab *s, int every, int max_steps)
{
    return adjoint_checkpoint(on_slab("fb_slab_adjoint_checkpoint", s), every, max_steps);
}

// (each output may be NULL; all 0 while checkpointing is off: not a refusal)
static int adjoint_checkpoint_info(const Call &k, int *every, int *max_steps, int *checkpoints, long long *replayed)
{
    if (int rc = enter(k, ADJOINT)) return rc;
    if (every) *every = k.m->ck_every;
    if (max_steps) *max_steps = k.m->ck_max;
    if (checkpoints) *checkpoints = k.m->ck_n;
    if (replayed) *replayed = k.m->ck_replayed;
    return FB_OK;
}
extern "C" int fb_model_adjoint_checkpoint_info(fb_model *m, int *every, int *max_steps, int *checkpoints, long long *replayed)
{
    return adjoint_checkpoint_info(on_model("fb_model_adjoint_checkpoint_info", m), every, max_steps, checkpoints, replayed);
}
extern "C" int fb_slab_adjoint_checkpoint_info(fb_slab *s, int *every, int *max_steps, int *checkpoints, long long *replayed)
{
    return adjoint_checkpoint_info(on_slab("fb_slab_adjoint_checkpoint_info", s), every, max_steps, checkpoints, replayed);
}

// the steps that a sweep can still pop: those on the tape, or under checkpointing the window's steps not yet swept
static int adjoint_unswept(const fb_model *m) { return m->ck_every ? m->ck_left : m->ad_fill; }

static int adjoint_recorded(const Call &k, int *n)
{
    if (!n) return refuse(k, "NULL output");
    if (int rc = enter(k, ADJOINT)) return rc;
    *n = adjoint_unswept(k.m);
    return FB_OK;
}
extern "C" int fb_model_adjoint_recorded(fb_model *m, int *n) { return adjoint_recorded(on_model("fb_model_adjoint_recorded", m), n); }
extern "C" int fb_slab_adjoint_recorded(fb_slab *s, int *n) { return adjoint_recorded(on_slab("fb_slab_adjoint_recorded", s), n); }

// [count] fields in; the single variable's call sets one (and with NULL removes the whole set, as the set's own does)
static int set_adjoints(const Call &k, const float *d_lambda_real, int count)
{
    if (d_lambda_real && (count < 1 || count > FB_ADJOINTS_MAX)) return refuse(k, "count outside [1, 32]");
    if (int rc = enter(k, ADJOINT)) return rc;
    return adjoint_in(k.m, k.s, d_lambda_real, count);
}
extern "C" int fb_model_set_adjoint(fb_model *m, const float *d_lambda_real) { return set_adjoints(on_model("fb_model_set_adjoint", m), d_lambda_real, 1); }
extern "C" int fb_slab_set_adjoint(fb_slab *s, const float *d_lambda_real) { return set_adjoints(on_slab("fb_slab_set_adjoint", s), d_lambda_real, 1); }
extern "C" int fb_model_set_adjoints(fb_model *m, const float *d_lambda_real, int count) { return set_adjoints(on_model("fb_model_set_adjoints", m), d_lambda_real, count); }
extern "C" int fb_slab_set_adjoints(fb_slab *s, const float *d_lambda_real, int count) { return set_adjoints(on_slab("fb_slab_set_adjoints", s), d_lambda_real, count); }
static_assert(FB_ADJOINTS_MAX == 32, "the refusal's text names the bound");

// (variable 0 only)
static int get_adjoint(const Call &k, float *d_real) { return get_beside(k, ADJOINT_SET, [](fb_model *m) { return &m->ad[0]; }, d_real); }
extern "C" int fb_model_get_adjoint(fb_model *m, float *d_real) { return get_adjoint(on_model("fb_model_get_adjoint", m), d_real); }
extern "C" int fb_slab_get_adjoint(fb_slab *s, float *d_real) { return get_adjoint(on_slab("fb_slab_get_adjoint", s), d_real); }

static int get_adjoints(const Call &k, float *d_real)
{
    if (!d_real) return refuse(k, "NULL output");
    if (int rc = enter(k, ADJOINT_SET)) return rc;
    const fb_ctx *c = k.m->c;
    for (int v = 0; v < k.m->ad_n; ++v)
        if (int rc = record(k.m, k.s, REC_VORT, d_real + (size_t)v * c->XL * c->ny, nullptr, k.m->ad[v].c0)) return rc;
    return FB_OK;
}
extern "C" int fb_model_get_adjoints(fb_model *m, float *d_real) { return get_adjoints(on_model("fb_model_get_adjoints", m), d_real); }
extern "C" int fb_slab_get_adjoints(fb_slab *s, float *d_real) { return get_adjoints(on_slab("fb_slab_get_adjoints", s), d_real); }

// (0 while none is set: not a refusal)
static int adjoint_count(const Call &k, int *count)
{
    if (!count) return refuse(k, "NULL output");
    if (int rc = enter(k, ADJOINT)) return rc;
    *count = k.m->ad_n;
    return FB_OK;
}
extern "C" int fb_model_adjoint_count(fb_model *m, int *count) { return adjoint_count(on_model("fb_model_adjoint_count", m), count); }
extern "C" int fb_slab_adjoint_count(fb_slab *s, int *count) { return adjoint_count(on_slab("fb_slab_adjoint_count", s), count); }

static int adjoint_back(const Call &k, int nsteps)
{
    if (nsteps < 0) return refuse(k, "nsteps < 0");
    if (int rc = enter(k, ADJOINT_SET)) return rc;
    if (nsteps > adjoint_unswept(k.m)) return refuse(k, std::to_string(nsteps) + " steps asked for, " + std::to_string(adjoint_unswept(k.m)) + " recorded");
    if (k.m->pa) {                                          // a particle adjoint is set: the sweep takes the particle tape along
        const fb_model *m = k.m;
        if (nsteps > m->pt_fill)
            return refuse(k, std::to_string(nsteps) + " steps asked for, " + std::to_string(m->pt_fill) + " on the particle tape (fb_model_particle_tape)");
        if (m->ad_n > 1)
            return refuse(k, "a particle adjoint is set beside a set of " + std::to_string(m->ad_n) + " adjoint variables: it forces a single variable");
        if (m->pt_fill != adjoint_unswept(m))
            return refuse(k, "the particle tape holds " + std::to_string(m->pt_fill) + " steps, the adjoint's window " + std::to_string(adjoint_unswept(m)) +
                          ": both must have recorded the same steps");
    }
    return adjoint_back(k.m, k.s, nsteps);
}
extern "C" int fb_model_adjoint_back(fb_model *m, int nsteps) { return adjoint_back(on_model("fb_model_adjoint_back", m), nsteps); }
extern "C" int fb_slab_adjoint_back(fb_slab *s, int nsteps) { return adjoint_back(on_slab("fb_slab_adjoint_back", s), nsteps); }

// The last n popped steps un-popped (n == -1: every one still on the tape): a sweep pops without erasing, so the slots up to ad_top
// hold what they held.  Not under checkpointing (the segment holds ck_every steps, not the window), not while a particle adjoint is
// set (the particle tape is popped in step with this one).  Nothing is launched.
static int adjoint_rewind(const Call &k, int n)
{
    if (n < -1) return refuse(k, "n < -1 (-1: every step still on the tape)");
    if (int rc = enter(k, ADJOINT)) return rc;
    fb_model *m = k.m;
    if (m->ck_every) return refuse(k, "not under adjoint checkpointing: the tape segment holds " + std::to_string(m->ck_every) + " steps, not the window (fb_model_adjoint_checkpoint)");
    if (m->pa) return refuse(k, "a particle adjoint is set: the particle tape is popped in step with the adjoint's (fb_model_set_particle_adjoint)");
    const int popped = m->ad_top - m->ad_fill;
    if (n > popped) return refuse(k, std::to_string(n) + " steps asked for, " + std::to_string(popped) + " popped and still on the tape");
    m->ad_fill += n < 0 ? popped : n;
    return FB_OK;
}
extern "C" int fb_model_adjoint_rewind(fb_model *m, int n) { return adjoint_rewind(on_model("fb_model_adjoint_rewind", m), n); }
extern "C" int fb_slab_adjoint_rewind(fb_slab *s, int n) { return adjoint_rewind(on_slab("fb_slab_adjoint_rewind", s), n); }

// (the tape's range needs the model's state: after the handle; nsteps == 0 is no refusal and launches nothing)
static int tangent_replay(const Call &k, int first, int nsteps)
{
    if (first < 0 || nsteps < 0) return refuse(k, "first < 0 or nsteps < 0");
    if (int rc = enter(k, TANGENT_SET | ONE_RANK_ADJOINT)) return rc;
    const fb_model *m = k.m;
    if (m->ck_every) return refuse(k, "not under adjoint checkpointing: the tape segment holds " + std::to_string(m->ck_every) + " steps, not the window (fb_model_adjoint_checkpoint)");
    if (!m->ad_tape) return refuse(k, "no tape (fb_model_adjoint_record)");
    if ((long long)first + nsteps > m->ad_top)
        return refuse(k, "steps " + std::to_string(first) + " .. " + std::to_string((long long)first + nsteps) + " asked for, " + std::to_string(m->ad_top) + " on the tape");
    if (nsteps == 0) return FB_OK;
    return tangent_replay(k.m, k.s, first, nsteps);
}
extern "C" int fb_model_tangent_replay(fb_model *m, int first, int nsteps) { return tangent_replay(on_model("fb_model_tangent_replay", m), first, nsteps); }
extern "C" int fb_slab_tangent_replay(fb_slab *s, int first, int nsteps) { return tangent_replay(on_slab("fb_slab_tangent_replay", s), first, nsteps); }

// ---- point observations and the forcing of the adjoint by their misfits (kernels: fb_obs.h) ----
// Between two steps only: the step, the tape, the tangent and the sweep never see any of it.  One GPU or a slab of one rank, as the adjoint.
static void obs_free(fb_model *m)
{
    if (m->ob_acc) { hipFree(m->ob_acc); m->ob_acc = nullptr; }
    if (m->ob_real) { hipFree(m->ob_real); m->ob_real = nullptr; }
    if (m->ob_red) { hipFree(m->ob_red); m->ob_red = nullptr; }
}

// field[i][j] = sum over the points of w wx_a wy_b, the transpose of sample(): the accumulator (two limbs per cell) and its head
// zeroed, max |w|, the integer atomics, the rounding of every cell (fb_obs.h).  d_field: any device [nx][ny] float32 field.
static int obs_scatter(fb_model *m, const double *d_xy, const double *d_w, int n, float *d_field)
{
    fb_ctx *c = m->c;
    const size_t cells = (size_t)c->nx * c->ny;
    int rc;
    if ((rc = rec_alloc((void **)&m->ob_acc, (2 * cells + 2) * sizeof(unsigned long long)))) return rc;
    unsigned long long *acc = m->ob_acc, *head = acc + 2 * cells;
    HIPCHK(hipMemsetAsync(acc, 0, (2 * cells + 2) * sizeof(unsigned long long), c->stream));
    if ((rc = launch_n(c, k_obs_wmax, (size_t)n, d_w, n, head))) return rc;
    if ((rc = launch_n(c, k_scatter, (size_t)n, part_geo(c), d_xy, d_w, n, acc, cells, (const unsigned long long *)head))) return rc;
    return launch_n(c, k_scatter_round, cells, (const unsigned long long *)acc, (const unsigned long long *)head, n, d_field, cells);
}

// kind 0 zeta, 1 u, 2 v, 3 psi of the resident state as the record of that kind forms it (record(): fb_model_get_vort,
// fb_model_get_diag), into the observations' own real field, then sample(): bit for bit sample() of that record
static const RecKind OBS_REC[4] = {REC_VORT, REC_U, REC_V, REC_PSI};
// (of != NULL: of a field stepped beside the vorticity in its place, as get_beside records one: H applied to a perturbation)
static int obs_observe(fb_model *m, fb_slab *s, int kind, const double *d_xy, int n, double *d_out, cf *const *of = nullptr)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = rec_alloc((void **)&m->ob_real, (size_t)c->nx * c->ny * sizeof(float)))) return rc;
    if ((rc = record(m, s, OBS_REC[kind], m->ob_real, nullptr, of))) return rc;
    return sample(c, m->ob_real, d_xy, n, d_out);
}

// lam += H^T w: the scatter into the observations' real field, its r2c as set_adjoint takes lam (beside_r2c: every grid class through
// the row and column dispatch), and the conjugate multiplier of the kind added into lam (k_obs_adjoint).  The k-bar and the
// accumulator hold nothing between two sweeps; the tape is not touched.
static int obs_adjoint_add(fb_model *m, fb_slab *s, int kind, const double *d_xy, const double *d_w, int n)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    int rc;
    if ((rc = rec_alloc((void **)&m->ob_real, (size_t)c->nx * c->ny * sizeof(float)))) return rc;
    if ((rc = obs_scatter(m, d_xy, d_w, n, m->ob_real)) || (rc = beside_r2c(m, s, m->ob_real))) return rc;
    return launch_n(c, k_obs_adjoint, grp_elems(c, G), make_coef(c), (const cf *)m->rec_work[0], m->ad[0].c0[0], kind, G.ncols, c->N1, c->N2, G.ky0);
}

// r = (h - y) / sigma^2 and *d_cost += 1/2 sum (h - y)^2 / sigma^2: the workgroups' partial sums, then one workgroup over them
static int obs_misfit(fb_model *m, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = rec_alloc((void **)&m->ob_red, (size_t)c->max_wg * sizeof(double)))) return rc;
    const int nwg = grid_for(c, (size_t)n);
    if ((rc = launch(c, k_obs_misfit, dim3(nwg), dim3(256), 0, d_h, d_y, d_sigma, n, d_r, m->ob_red))) return rc;
    return launch(c, k_obs_cost_final, dim3(1), dim3(256), 0, (const double *)m->ob_red, nwg, d_cost);
}

static bool obs_kind_ok(int kind) { return kind >= 0 && kind <= 3; }
static const char *const OBS_KIND = "kind must be 0 (zeta), 1 (u), 2 (v) or 3 (psi)";

static int scatter(const Call &k, const double *d_xy, const double *d_w, int n, float *d_field)
{
    if (!d_xy || !d_w || !d_field) return refuse(k, "NULL positions, weights or output");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (int rc = enter(k, ADJOINT)) return rc;
    return obs_scatter(k.m, d_xy, d_w, n, d_field);
}
extern "C" int fb_model_scatter(fb_model *m, const double *d_xy, const double *d_w, int n, float *d_field)
{
    return scatter(on_model("fb_model_scatter", m), d_xy, d_w, n, d_field);
}
extern "C" int fb_slab_scatter(fb_slab *s, const double *d_xy, const double *d_w, int n, float *d_field)
{
    return scatter(on_slab("fb_slab_scatter", s), d_xy, d_w, n, d_field);
}

static int observe(const Call &k, int kind, const double *d_xy, int n, double *d_out)
{
    if (!obs_kind_ok(kind)) return refuse(k, OBS_KIND);
    if (!d_xy || !d_out) return refuse(k, "NULL positions or output");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (int rc = enter(k, ADJOINT)) return rc;
    return obs_observe(k.m, k.s, kind, d_xy, n, d_out);
}
extern "C" int fb_model_observe(fb_model *m, int kind, const double *d_xy, int n, double *d_out) { return observe(on_model("fb_model_observe", m), kind, d_xy, n, d_out); }
extern "C" int fb_slab_observe(fb_slab *s, int kind, const double *d_xy, int n, double *d_out) { return observe(on_slab("fb_slab_observe", s), kind, d_xy, n, d_out); }

// H applied to perturbation `which` of the tangent set: observe with the record's source set to its base (the count needs the
// model's state: after the handle)
static int observe_tangent(const Call &k, int which, int kind, const double *d_xy, int n, double *d_out)
{
    if (!obs_kind_ok(kind)) return refuse(k, OBS_KIND);
    if (!d_xy || !d_out) return refuse(k, "NULL positions or output");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (which < 0) return refuse(k, "perturbation index < 0");
    if (int rc = enter(k, TANGENT_SET | ONE_RANK_ADJOINT)) return rc;
    if (which >= k.m->tg_n) return refuse(k, "perturbation " + std::to_string(which) + " of a set of " + std::to_string(k.m->tg_n));
    return obs_observe(k.m, k.s, kind, d_xy, n, d_out, k.m->tg[which].c0);
}
extern "C" int fb_model_observe_tangent(fb_model *m, int k, int kind, const double *d_xy, int n, double *d_out)
{
    return observe_tangent(on_model("fb_model_observe_tangent", m), k, kind, d_xy, n, d_out);
}
extern "C" int fb_slab_observe_tangent(fb_slab *s, int k, int kind, const double *d_xy, int n, double *d_out)
{
    return observe_tangent(on_slab("fb_slab_observe_tangent", s), k, kind, d_xy, n, d_out);
}

// (d_sigma may be NULL: sigma = 1)
static int obs_misfit(const Call &k, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost)
{
    if (!d_h || !d_y || !d_r || !d_cost) return refuse(k, "NULL values, observations, residual or cost");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (int rc = enter(k, ADJOINT)) return rc;
    return obs_misfit(k.m, d_h, d_y, d_sigma, n, d_r, d_cost);
}
extern "C" int fb_model_obs_misfit(fb_model *m, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost)
{
    return obs_misfit(on_model("fb_model_obs_misfit", m), d_h, d_y, d_sigma, n, d_r, d_cost);
}
extern "C" int fb_slab_obs_misfit(fb_slab *s, const double *d_h, const double *d_y, const double *d_sigma, int n, double *d_r, double *d_cost)
{
    return obs_misfit(on_slab("fb_slab_obs_misfit", s), d_h, d_y, d_sigma, n, d_r, d_cost);
}

static int adjoint_add_obs(const Call &k, int kind, const double *d_xy, const double *d_w, int n)
{
    if (!obs_kind_ok(kind)) return refuse(k, OBS_KIND);
    if (!d_xy || !d_w) return refuse(k, "NULL positions or weights");
    if (!particle_count_ok(n)) return refuse(k, "n outside [1, 2^24]");
    if (int rc = enter(k, ADJOINT_SET)) return rc;
    if (k.m->ad_n > 1)
        return refuse(k, "a set of " + std::to_string(k.m->ad_n) + " adjoint variables is set: the forcing acts on a single variable (get, add, set for one of a set)");
    return obs_adjoint_add(k.m, k.s, kind, d_xy, d_w, n);
}
extern "C" int fb_model_adjoint_add_obs(fb_model *m, int kind, const double *d_xy, const double *d_w, int n)
{
    return adjoint_add_obs(on_model("fb_model_adjoint_add_obs", m), kind, d_xy, d_w, n);
}
extern "C" int fb_slab_adjoint_add_obs(fb_slab *s, int kind, const double *d_xy, const double *d_w, int n)
{
    return adjoint_add_obs(on_slab("fb_slab_adjoint_add_obs", s), kind, d_xy, d_w, n);
}

// ---- what the step and the model's end know of all of them (declared in fftbaro.hip) ----
// At the top of RK stage `stage`, from the state the vorticity's stage starts from: the tracer's stage, the particles', the
// tangent-linear model's, and the state into the adjoint's tape (the last three on one rank only: their set calls refuse more).
static int beside_stage(fb_model *m, fb_slab *s, int stage)
{
    int rc;
    if (m->ck_replay) return adjoint_stash(m, stage);       // a segment of a checkpointed window run again: the vorticity alone moves
    if (m->tracer && (rc = tracer_stage(m, s, stage))) return rc;
    if (m->pt_n && (rc = particle_stage(m, stage))) return rc;
    if (m->tg_n && (rc = tangent_stage(m, s, stage))) return rc;
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
}
