// fb_beside_adjoint.h -- the host side of the adjoint model: the tape and the checkpoints, the adjoint and its set, the sweep, the
// tangent replay over the tape, the point observations (included by fb_beside.h after fb_beside_tangent.h and fb_beside_particles.h,
// whose sets, tapes and sample() it uses; kernels: fb_adjoint.h, fb_replay.h, fb_obs.h; C ABI: include/fftbaro.h).
#pragma once

// ---- the adjoint model (kernels: fb_adjoint.h) ----
// One GPU or a slab of one rank: one column group, no exchange (as the particles).
// (the full tape of fb_model_adjoint_record, or the segment, the checkpoints and the live copy of fb_model_adjoint_checkpoint: one
// mode at a time, and either call frees what the other held)
static void adjoint_tape_free(fb_model *m)
{
    dev_free(m->ad_tape); dev_free(m->ck_store); dev_free(m->ck_live);
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
    dev_free(m->ad_real);
    dev_free(m->ad_spec);
}

static void adjoint_free(fb_model *m)
{
    set_free(m->ad);
    adjoint_work_free(m);
}

// per variable 3 half spectra on the active columns and 1 on the frozen ones; the real fields; a set's chunk of mu~ spectra
static size_t adjoint_bytes(const fb_model *m)
{
    const fb_ctx *c = m->c;
    if (!m->ad.n) return 0;
    size_t n = adjoint_real_fields(m->ad.n) * c->nx * c->ny * sizeof(float);
    for (int g = 0; g < c->ngroups; ++g) n += (size_t)m->ad.n * (g < c->nact ? 3 : 1) * grp_elems(c, c->grp[g]) * sizeof(cf);
    if (m->ad.n > 1) n += (size_t)adjoint_chunk(m->ad.n) * grp_elems(c, c->grp[0]) * sizeof(cf);
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
    if ((rc = dev_alloc((void **)&m->ad_tape, (size_t)depth * 4 * n * sizeof(cf), "the adjoint's tape: allocation failed"))) return rc;
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
    const char *const what = "the adjoint's tape segment, checkpoints and live copy: allocation failed";
    if ((rc = dev_alloc((void **)&m->ad_tape, (size_t)every * 4 * n * sizeof(cf), what)) ||
        (rc = dev_alloc((void **)&m->ck_store, checkpoint_slots(m) * n * sizeof(cf), what)) || (rc = dev_alloc((void **)&m->ck_live, n * sizeof(cf), what))) {
        adjoint_tape_free(m);
        return rc;
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
    if (m->ad.n && (!d_rows || count != m->ad.n)) HIPCHK(hipStreamSynchronize(c->stream));
    if (!d_rows) { adjoint_free(m); return FB_OK; }
    if (count != m->ad.n) adjoint_work_free(m);
    int rc = rec_alloc((void **)&m->ad_real, adjoint_real_fields(count) * c->nx * c->ny * sizeof(float));
    if (!rc && count > 1) rc = rec_alloc((void **)&m->ad_spec, (size_t)adjoint_chunk(count) * grp_elems(c, c->grp[0]) * sizeof(cf));
    if (!rc) rc = set_in(m, s, d_rows, count, m->ad);
    if (rc) adjoint_free(m);
    return rc;
}

// The tail of a backward stage for the variable v: its four product fields at prod forward as beside_in takes a field, into the fields
// 0..3 of the record workspace (zeroed first: pad columns), then the recurrences on its lam, k-bar and accumulator (k_adjoint_update).
static int adjoint_stage_tail(fb_model *m, int stage, const float *prod, Beside &v)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G);
    cf *z = m->rec_work[0];
    HIPCHK(hipMemsetAsync(z, 0, 4 * n * sizeof(cf), c->stream));
    if (int rc = real_to_spectra(c, prod, z, 4, (long)n)) return rc;
    return dispatch<4>(stage, [&](auto S) {
        return launch_n(c, k_adjoint_update<S()>, n / 2, make_coef(c), (const cf *)z, (long)n, v.c0[0], v.c1[0], v.acc[0], m->nu, m->dt, G.ncols, c->N1, c->N2, G.ky0);
    });
}

// One RK stage of a backward step: L_stage^T of the k-bar about the recorded stage state zs, then the recurrences (fb_adjoint.h).
// Five fields back to physical space as particle_stage takes u and v, with its scales; four products forward (adjoint_stage_tail);
// through the record workspace, which the step never reads.  xs != NULL: a particle adjoint is set and xs is the stage's slot
// of the particle tape; its stage runs while u and v are whole, and its forcing is folded into two of the products (fb_lagrangian.h).
// With xs == NULL the launches are the ones a sweep has always made.
static int adjoint_stage(fb_model *m, int stage, const cf *zs, const double *xs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    cf *z = m->rec_work[0];
    Beside &v = m->ad.v[0];
    int rc;
    const cf *kb = stage == 3 ? v.c0[0] : v.c1[0];
    if ((rc = launch_n(c, k_adjoint_deriv, n / 2, make_coef(c), zs, kb, stage == 3 ? m->dt / 6.0f : 1.0f, z, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
    if ((rc = spectra_to_real(c, z, 5, (long)n, m->ad_real, 1.0f / (float)nr, 1))) return rc;     // field 1: u = -dpsi/dy (record(), REC_U)
    if (xs && (rc = lagrangian_stage(m, stage, xs))) return rc;
    if ((rc = launch_n(c, k_adjoint_prod, nr / 4, m->ad_real, nr))) return rc;
    if (xs && (rc = lagrangian_deposit(m, xs))) return rc;
    return adjoint_stage_tail(m, stage, m->ad_real + nr, v);
}

// adjoint_stage for a set of ad.n > 1 variables.  u, v, zeta_x, zeta_y depend on zs alone: their four spectra (k_adjoint_base), the
// backward x pass and the four ROW_INV passes run once, into the real fields 0..3 of ad_real, which nothing below writes.  Then in
// chunks of C = min(ad.n, ADJOINT_CHUNK) variables (a chunk re-reads the four base fields once, 16 nx ny bytes): the chunk's mu~ in
// one launch into ad_spec, their backward x pass in one, a ROW_INV pass each into the real fields 4 .. 4 + C; k_adjoint_prod_set
// out of place into the 4 C fields after them; and per variable adjoint_stage_tail, as adjoint_stage runs it, through the fields
// 0..3 of the record workspace.  Launches per stage: 7 + ceil(ad.n / C) * 4 + 9 ad.n.  The passes of distinct fields share no
// arithmetic, so every variable gets the bits adjoint_stage gives it.
static int adjoint_stage_set(fb_model *m, int stage, const cf *zs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    const int M = m->ad.n, C = adjoint_chunk(M);
    cf *z = m->rec_work[0], *zm = m->ad_spec;
    float *base = m->ad_real, *mu = base + 4 * nr, *prod = mu + (size_t)C * nr;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    int rc;
    if ((rc = launch_n(c, k_adjoint_base, n / 2, coef, zs, z, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
    if ((rc = spectra_to_real(c, z, 4, (long)n, base, g, 0))) return rc;                                           // field 0: u = -dpsi/dy (record(), REC_U)
    for (int k0 = 0; k0 < M; k0 += C) {
        const int cnt = M - k0 < C ? M - k0 : C;
        AdjointKbars kbars = {};
        for (int k = 0; k < cnt; ++k) kbars.kb[k] = stage == 3 ? m->ad.v[k0 + k].c0[0] : m->ad.v[k0 + k].c1[0];
        if ((rc = launch_n(c, k_adjoint_mu, n / 2, coef, kbars, cnt, stage == 3 ? m->dt / 6.0f : 1.0f, zm, (long)n, G.ncols, c->N1, c->N2, G.ky0))) return rc;
        if ((rc = spectra_to_real(c, zm, cnt, (long)n, mu, g, -1))) return rc;
        rc = dispatch<ADJOINT_CHUNK>(cnt - 1, [&](auto K) {
            return launch_n(c, k_adjoint_prod_set<K() + 1>, nr / 4, (const float *)base, (const float *)mu, prod, nr);
        });
        for (int k = 0; k < cnt && !rc; ++k) rc = adjoint_stage_tail(m, stage, prod + (size_t)k * 4 * nr, m->ad.v[k0 + k]);
        if (rc) return rc;
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
            rc = m->ad.n == 1 ? adjoint_stage(m, stage, step + (size_t)stage * n, m->pa ? particle_tape_at(m, m->pt_fill - 1, stage) : nullptr)
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
// its real fields, rp_real: sized for the tangent set's count, so they go with a set that goes or changes it (tangent_in, tangent_free)
static int replay_chunk(int count) { return count < REPLAY_CHUNK ? count : REPLAY_CHUNK; }
static size_t replay_real_fields(int count) { return 4 + 5 * (size_t)replay_chunk(count); }
static size_t replay_bytes(const fb_model *m) { return m->rp_real ? replay_real_fields(m->tg.n) * m->c->nx * m->c->ny * sizeof(float) : 0; }

// One RK stage of the tangent step of every perturbation of the set about the recorded stage state zs, adjoint_stage_set's mirror
// image.  The base flow once: k_adjoint_base, the backward x pass, four ROW_INV passes into the real fields 0..3 of rp_real (u, v,
// zeta_x, zeta_y), which nothing below writes.  Then in chunks of C = min(tg.n, REPLAY_CHUNK) perturbations: per perturbation
// k_replay_deriv from its state of this stage (tangent_stage's: the base at stage 0, the stage state afterwards), the backward x pass
// and four ROW_INV passes into its four real fields (du, dv, dz_x, dz_y); per chunk k_replay_prod_set out of place into one field per
// perturbation; per perturbation its product's r2c as beside_r2c takes a field (field 0 of the record workspace zeroed, ROW_FWD, the
// forward x pass) and the tracer's k_beside_update with the model's nu, on the active column tiles only.  4 + 5 tg.n fields
// transformed and 7 + ceil(tg.n / C) + 12 tg.n launches per stage.  The passes of distinct fields share no arithmetic.
static int replay_stage(fb_model *m, int stage, const cf *zs)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const size_t n = grp_elems(c, G), nr = (size_t)c->nx * c->ny;
    const SpecCoef coef = make_coef(c);
    const int M = m->tg.n, C = replay_chunk(M);
    cf *z = m->rec_work[0];
    float *base = m->rp_real, *pert = base + 4 * nr, *prod = pert + (size_t)C * 4 * nr;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    const bool staged = stage > 0 && c->nact > 0;
    int rc;
    // the fields 0..3 of the record workspace -> four real fields, the first negated: u = -dpsi/dy (record(), REC_U)
    auto to_real = [&](float *out) { return spectra_to_real(c, z, 4, (long)n, out, g, 0); };
    if ((rc = launch_n(c, k_adjoint_base, n / 2, coef, zs, z, (long)n, G.ncols, c->N1, c->N2, G.ky0)) || (rc = to_real(base))) return rc;
    for (int k0 = 0; k0 < M; k0 += C) {
        const int cnt = M - k0 < C ? M - k0 : C;
        for (int k = 0; k < cnt; ++k) {
            const Beside &f = m->tg.v[k0 + k];
            if ((rc = launch_n(c, k_replay_deriv, n / 2, coef, (const cf *)f.c0[0], (const cf *)(staged ? f.c1[0] : f.c0[0]), z, (long)n, G.ncols, c->N1, c->N2, G.ky0)) ||
                (rc = to_real(pert + (size_t)k * 4 * nr)))
                return rc;
        }
        rc = dispatch<REPLAY_CHUNK>(cnt - 1, [&](auto K) {
            return launch_n(c, k_replay_prod_set<K() + 1>, nr / 4, (const float *)base, (const float *)pert, prod, nr);
        });
        if (rc) return rc;
        for (int k = 0; k < cnt; ++k) {
            Beside &f = m->tg.v[k0 + k];
            HIPCHK(hipMemsetAsync(z, 0, n * sizeof(cf), c->stream));                                                // pad columns zero
            if ((rc = real_to_spectra(c, prod + (size_t)k * nr, z, 1, 0))) return rc;
            if ((rc = beside_update_nj<1>(m, nullptr, stage, f, z, nullptr, m->nu))) return rc;
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
    if ((rc = rec_alloc((void **)&m->rp_real, replay_real_fields(m->tg.n) * c->nx * c->ny * sizeof(float)))) return rc;
    for (int k = 0; k < nsteps; ++k) {
        const cf *step = m->ad_tape + (size_t)(first + k) * 4 * n;
        for (int stage = 0; stage < 4; ++stage)
            if ((rc = replay_stage(m, stage, step + (size_t)stage * n))) return rc;
    }
    return FB_OK;
}

// a slab of one rank goes through the same code; on several ranks the adjoint model is refused
constexpr unsigned ADJOINT = NEED_TRANSPORT | ONE_RANK_ADJOINT, ADJOINT_SET = ADJOINT | NEED_ADJOINT;
// the transpose through D and the replay of a window's noise are not built: no tape and no window while forcing is set
static const char *const FORCING_NO_ADJOINT = "not while forcing is set: the adjoint of the split stage is not built (fb_model_set_forcing)";

static int adjoint_record(const Call &k, int depth)
{
    if (depth < 0 || depth > (1 << 20)) return refuse(k, "depth outside [0, 2^20]");
    if (int rc = enter(k, ADJOINT)) return rc;
    if (depth && k.m->fr_on) return refuse(k, FORCING_NO_ADJOINT, FB_EUNSUPPORTED);
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
    if (every && k.m->fr_on) return refuse(k, FORCING_NO_ADJOINT, FB_EUNSUPPORTED);
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
static int set_adjoints(const Call &k, const float *d_lambda_real, int count) { return set_fields(k, ADJOINT, adjoint_in, d_lambda_real, count); }
extern "C" int fb_model_set_adjoint(fb_model *m, const float *d_lambda_real) { return set_adjoints(on_model("fb_model_set_adjoint", m), d_lambda_real, 1); }
extern "C" int fb_slab_set_adjoint(fb_slab *s, const float *d_lambda_real) { return set_adjoints(on_slab("fb_slab_set_adjoint", s), d_lambda_real, 1); }
extern "C" int fb_model_set_adjoints(fb_model *m, const float *d_lambda_real, int count) { return set_adjoints(on_model("fb_model_set_adjoints", m), d_lambda_real, count); }
extern "C" int fb_slab_set_adjoints(fb_slab *s, const float *d_lambda_real, int count) { return set_adjoints(on_slab("fb_slab_set_adjoints", s), d_lambda_real, count); }

// (variable 0 only)
static int get_adjoint(const Call &k, float *d_real) { return get_beside(k, ADJOINT_SET, [](fb_model *m) { return &m->ad.v[0]; }, d_real); }
extern "C" int fb_model_get_adjoint(fb_model *m, float *d_real) { return get_adjoint(on_model("fb_model_get_adjoint", m), d_real); }
extern "C" int fb_slab_get_adjoint(fb_slab *s, float *d_real) { return get_adjoint(on_slab("fb_slab_get_adjoint", s), d_real); }

extern "C" int fb_model_get_adjoints(fb_model *m, float *d_real) { return set_out(on_model("fb_model_get_adjoints", m), ADJOINT_SET, &fb_model::ad, d_real); }
extern "C" int fb_slab_get_adjoints(fb_slab *s, float *d_real) { return set_out(on_slab("fb_slab_get_adjoints", s), ADJOINT_SET, &fb_model::ad, d_real); }
extern "C" int fb_model_adjoint_count(fb_model *m, int *count) { return set_count(on_model("fb_model_adjoint_count", m), ADJOINT, &fb_model::ad, count); }
extern "C" int fb_slab_adjoint_count(fb_slab *s, int *count) { return set_count(on_slab("fb_slab_adjoint_count", s), ADJOINT, &fb_model::ad, count); }

static int adjoint_back(const Call &k, int nsteps)
{
    if (nsteps < 0) return refuse(k, "nsteps < 0");
    if (int rc = enter(k, ADJOINT_SET)) return rc;
    if (nsteps > adjoint_unswept(k.m)) return refuse(k, std::to_string(nsteps) + " steps asked for, " + std::to_string(adjoint_unswept(k.m)) + " recorded");
    if (k.m->pa) {                                          // a particle adjoint is set: the sweep takes the particle tape along
        const fb_model *m = k.m;
        if (nsteps > m->pt_fill)
            return refuse(k, std::to_string(nsteps) + " steps asked for, " + std::to_string(m->pt_fill) + " on the particle tape (fb_model_particle_tape)");
        if (m->ad.n > 1)
            return refuse(k, "a particle adjoint is set beside a set of " + std::to_string(m->ad.n) + " adjoint variables: it forces a single variable");
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
    dev_free(m->ob_acc);
    dev_free(m->ob_real);
    dev_free(m->ob_red);
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
    return launch_n(c, k_obs_adjoint, grp_elems(c, G), make_coef(c), (const cf *)m->rec_work[0], m->ad.v[0].c0[0], kind, G.ncols, c->N1, c->N2, G.ky0);
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
    if (which >= k.m->tg.n) return refuse(k, "perturbation " + std::to_string(which) + " of a set of " + std::to_string(k.m->tg.n));
    return obs_observe(k.m, k.s, kind, d_xy, n, d_out, k.m->tg.v[which].c0);
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
    if (k.m->ad.n > 1)
        return refuse(k, "a set of " + std::to_string(k.m->ad.n) + " adjoint variables is set: the forcing acts on a single variable (get, add, set for one of a set)");
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

