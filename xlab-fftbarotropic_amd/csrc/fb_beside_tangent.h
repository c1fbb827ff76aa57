// fb_beside_tangent.h -- the host side of the tangent-linear model: the tangent set and its stage, the inner products and QR, the basis
// tape and the combination of the covariant Lyapunov vectors (included by fb_beside.h after the path the fields share; kernels:
// fb_tangent.h, fb_clv.h; C ABI: include/fftbaro.h).  The tangent replay over the adjoint's tape is in fb_beside_adjoint.h.
#pragma once

// ---- the tangent-linear model (kernels: fb_tangent.h) ----
// A set of tg.n perturbations on the one trajectory; the single tangent of fb_model_set_tangent is the set of one, and its norm the
// inner product of perturbation 0 with itself.
static void tangent_tape_free(fb_model *m)
{
    for (cf *&p : m->tt) dev_free(p);
    m->tt_depth = m->tt_fill = 0;
}

// (the basis tape holds copies of this set's bases in this set's count: it goes with the set; and so do the tangent replay's real
// fields, rp_real, which tangent_replay sizes for the count: fb_beside_adjoint.h)
static void tangent_free(fb_model *m)
{
    tangent_tape_free(m);
    dev_free(m->rp_real);
    set_free(m->tg);
    for (cf *&p : m->tg_j) dev_free(p);
    dev_free(m->tg_red);
}

// One RK stage of the perturbations, where tracer_stage runs and from the same states, one perturbation after the other in index
// order.  The tangent of the bilinear J is two advect passes, J(dz; psi) + J(zeta; dpsi); the first pass's result is copied to tg_j
// before the second overwrites the record workspace; then the update with both and the model's nu.  Nothing is shared between two
// perturbations but the scratch: perturbation k of a set is bit for bit the set of one started from the same field.
static int tangent_stage(fb_model *m, fb_slab *s, int stage)
{
    fb_ctx *c = m->c;
    int rc;
    for (int k = 0; k < m->tg.n; ++k) {
        Beside &f = m->tg.v[k];
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
    const bool tape_goes = m->tt_depth && (!d_rows || count != m->tg.n);
    const bool replay_goes = m->rp_real && (!d_rows || count != m->tg.n);     // (a queued replay may still use it)
    if ((rc = beside_begin(m, (m->tg.n && (!d_rows || count < m->tg.n)) || tape_goes || replay_goes))) return rc;
    if (tape_goes) tangent_tape_free(m);
    if (replay_goes) dev_free(m->rp_real);
    if (!d_rows) { tangent_free(m); return FB_OK; }
    rc = each_group(c, c->nact, [&](int g, size_t n) { return rec_alloc((void **)&m->tg_j[g], n * sizeof(cf)); });
    if (!rc) rc = rec_alloc((void **)&m->tg_red, (size_t)c->ngroups * c->max_wg * sizeof(double));
    if (!rc) rc = set_in(m, s, d_rows, count, m->tg);
    if (rc) tangent_free(m);
    return rc;
}

static int tangent_scale(fb_model *m, float a)
{
    fb_ctx *c = m->c;
    return each_group(c, c->ngroups, [&](int g, size_t n) { return launch_n(c, k_tangent_scale, n / 2, m->tg.v[0].c0[g], n, a); });
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
static int tangent_norm0(fb_model *m, int kind, double *d_out) { return tangent_dot(m, kind, m->tg.v[0], m->tg.v[0], d_out); }

// every <v_i, v_j> into the device array d_gram, [tg.n][tg.n] float64 row-major: the upper triangle through tangent_dot, mirrored
static int tangent_gram(fb_model *m, int kind, double *d_gram)
{
    const int M = m->tg.n;
    for (int i = 0; i < M; ++i)
        for (int j = i; j < M; ++j)
            if (int rc = tangent_dot(m, kind, m->tg.v[i], m->tg.v[j], d_gram + (size_t)i * M + j)) return rc;
    return launch(m->c, k_tangent_mirror, dim3(1), dim3(256), 0, d_gram, M);
}

// Modified Gram-Schmidt in place on the bases, in index order: for every j, r_ij = <q_i, v_j> of the CURRENT v_j and v_j -= r_ij q_i
// for i < j, then r_jj = sqrt(<v_j, v_j>) and v_j /= r_jj.  d_r, a device array [tg.n][tg.n] float64 row-major, ends upper triangular
// with v_j(old) = sum over i <= j of r_ij q_i; every coefficient is written there by one kernel and read from there by the next, so
// the host waits for nothing.  A rank-deficient set leaves a diagonal element that is not finite and positive and vectors that are
// not finite; nothing here tests for it.  The stage arrays hold no live data between two steps: only the bases change.
static int tangent_qr(fb_model *m, int kind, double *d_r)
{
    fb_ctx *c = m->c;
    const int M = m->tg.n;
    int rc;
    HIPCHK(hipMemsetAsync(d_r, 0, (size_t)M * M * sizeof(double), c->stream));
    for (int j = 0; j < M; ++j) {
        Beside &v = m->tg.v[j];
        for (int i = 0; i < j; ++i) {
            double *r = d_r + (size_t)i * M + j;
            if ((rc = tangent_dot(m, kind, m->tg.v[i], v, r))) return rc;
            rc = each_group(c, c->ngroups, [&](int g, size_t n) { return launch_n(c, k_tangent_axpy, n / 2, v.c0[g], (const cf *)m->tg.v[i].c0[g], n, (const double *)r); });
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
static cf *tangent_tape_at(const fb_model *m, int g, size_t n, int slot, int k) { return m->tt[g] + ((size_t)slot * m->tg.n + k) * n; }

// The tape on (depth >= 1 slots for the current set) or off (depth == 0); either way it starts empty.  The step reads no pointer of
// it: the captured step stays.  A tape that goes may still be read or written by queued work.
static int tangent_tape(fb_model *m, int depth)
{
    fb_ctx *c = m->c;
    if (m->tt_depth) HIPCHK(hipStreamSynchronize(c->stream));
    tangent_tape_free(m);
    if (depth == 0) return FB_OK;
    const int rc = each_group(c, c->ngroups, [&](int g, size_t n) {
        return dev_alloc((void **)&m->tt[g], (size_t)depth * m->tg.n * n * sizeof(cf), "the tangent's basis tape: allocation failed");
    });
    if (rc) { tangent_tape_free(m); return rc; }
    m->tt_depth = depth;
    return FB_OK;
}

// the bases of the live set into the next slot: device to device on the context's stream, nothing allocated
static int tangent_tape_push(fb_model *m)
{
    fb_ctx *c = m->c;
    for (int k = 0; k < m->tg.n; ++k) {
        const int rc = each_group(c, c->ngroups, [&](int g, size_t n) -> int {
            HIPCHK(hipMemcpyAsync(tangent_tape_at(m, g, n, m->tt_fill, k), m->tg.v[k].c0[g], n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
            return FB_OK;
        });
        if (rc) return rc;
    }
    ++m->tt_fill;
    return FB_OK;
}

// live set <- (slot >= 0: the bases of tape slot `slot`; slot == -1: the live set itself, in place) C, d_c a device array [tg.n][tg.n]
// float64 row-major: v_j = sum over i of c_ij q_i, one k_tangent_combine per column group with the smallest compile-time bound that
// holds the count.  The stage arrays hold no live data between two steps: only the bases change.
template <int MB> static int tangent_combine_mb(fb_model *m, int slot, const double *d_c)
{
    fb_ctx *c = m->c;
    const int M = m->tg.n;
    return each_group(c, c->ngroups, [&](int g, size_t n) {
        CombineArrays<MB> a = {};
        for (int k = 0; k < M; ++k) {
            a.dst[k] = m->tg.v[k].c0[g];
            a.src[k] = slot < 0 ? a.dst[k] : tangent_tape_at(m, g, n, slot, k);
        }
        return launch_n(c, k_tangent_combine<MB>, n / 2, a, n, M, d_c);
    });
}
static int tangent_combine(fb_model *m, int slot, const double *d_c)
{
    const int M = m->tg.n;
    return M <= 4 ? tangent_combine_mb<4>(m, slot, d_c) : M <= 8 ? tangent_combine_mb<8>(m, slot, d_c)
         : M <= 16 ? tangent_combine_mb<16>(m, slot, d_c) : tangent_combine_mb<32>(m, slot, d_c);
}
static_assert(FB_TANGENTS_MAX <= 32, "k_tangent_combine's largest instance holds 32 perturbations");

// a slab of one rank goes through the same code; on several ranks the tangent-linear model is refused
constexpr unsigned TANGENT =NEED_TRANSPORT | ONE_RANK_TANGENT, TANGENT_SET = TANGENT | NEED_TANGENT;

// [count] fields in; the single tangent's call sets one (and with NULL removes the whole set, as the set's own does)
static int set_tangents(const Call &k, const float *d_dz_real, int count) { return set_fields(k, TANGENT, tangent_in, d_dz_real, count); }
extern "C" int fb_model_set_tangent(fb_model *m, const float *d_dz_real) { return set_tangents(on_model("fb_model_set_tangent", m), d_dz_real, 1); }
extern "C" int fb_slab_set_tangent(fb_slab *s, const float *d_dz_real) { return set_tangents(on_slab("fb_slab_set_tangent", s), d_dz_real, 1); }
extern "C" int fb_model_set_tangents(fb_model *m, const float *d_dz_real, int count) { return set_tangents(on_model("fb_model_set_tangents", m), d_dz_real, count); }
extern "C" int fb_slab_set_tangents(fb_slab *s, const float *d_dz_real, int count) { return set_tangents(on_slab("fb_slab_set_tangents", s), d_dz_real, count); }

// (perturbation 0 only)
static int get_tangent(const Call &k, float *d_dz_real) { return get_beside(k, TANGENT_SET, [](fb_model *m) { return &m->tg.v[0]; }, d_dz_real); }
extern "C" int fb_model_get_tangent(fb_model *m, float *d_dz_real) { return get_tangent(on_model("fb_model_get_tangent", m), d_dz_real); }
extern "C" int fb_slab_get_tangent(fb_slab *s, float *d_dz_real) { return get_tangent(on_slab("fb_slab_get_tangent", s), d_dz_real); }

extern "C" int fb_model_get_tangents(fb_model *m, float *d_dz_real) { return set_out(on_model("fb_model_get_tangents", m), TANGENT_SET, &fb_model::tg, d_dz_real); }
extern "C" int fb_slab_get_tangents(fb_slab *s, float *d_dz_real) { return set_out(on_slab("fb_slab_get_tangents", s), TANGENT_SET, &fb_model::tg, d_dz_real); }
extern "C" int fb_model_tangent_count(fb_model *m, int *count) { return set_count(on_model("fb_model_tangent_count", m), TANGENT, &fb_model::tg, count); }
extern "C" int fb_slab_tangent_count(fb_slab *s, int *count) { return set_count(on_slab("fb_slab_tangent_count", s), TANGENT, &fb_model::tg, count); }

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

