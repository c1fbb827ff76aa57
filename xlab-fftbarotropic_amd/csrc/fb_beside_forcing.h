// fb_beside_forcing.h -- the host side of the split stage: stochastic ring forcing, linear drag and hyperviscosity after every RK4 step
// (included by fb_beside.h after the other models; kernels and the definition: fb_forcing.h; C ABI: include/fftbaro.h).  One rank only.
//
// The stage works on the vorticity in the 3-pass layout.  Where the state arrays are in that layout (the three-kernel path with
// N2 < 32) it runs in place on ZA; elsewhere the state goes out into fr_work (export_state), the kernel runs there, and it comes back
// in as fb_model_set_spectrum's tail puts a state in (state_convert / k_full_relayout<true>).  fr_work, the partial sums and the
// clock with the four totals are allocated when the forcing is set: a step allocates nothing, and the clock and the totals live in
// device memory, so a captured step replays with the clock of its own time.
#pragma once

static void forcing_free(fb_model *m)
{
    dev_free(m->fr_work);
    dev_free(m->fr_part);
    dev_free(m->fr_dev);
    m->fr_on = false;
    m->fr_nring = 0;
}

// the state arrays are not in the 3-pass layout: the stage needs the workspace
static bool forcing_needs_work(const fb_model *m) { return m->xpass != XP_COLS || state_tm(m->c); }

static size_t forcing_bytes(const fb_model *m)
{
    const fb_ctx *c = m->c;
    if (!m->fr_on) return 0;
    return (m->fr_work ? priv_elems(c) * sizeof(cf) : 0) + 4 * (size_t)c->max_wg * sizeof(double) + 5 * sizeof(double);
}

static unsigned long long *forcing_clock(const fb_model *m) { return m->fr_dev; }
static double *forcing_totals(const fb_model *m) { return reinterpret_cast<double *>(m->fr_dev + 1); }

// The split stage, after the step's fourth stage (fb_model_step and fb_slab_step): the vorticity, then the base of every perturbation
// of the tangent set times D, then the derivative fields again, since those that stage 3 left belong to the state before the
// split stage (as checkpoint_restore re-primes: the PRIME launch of k_col_full; model_prime on the three-kernel path, and for the
// fused flow the backward strided sub-pass on the active tiles, which a slab's stage runs itself).  The tracer, the particles and
// their deformation gradient are not touched.
static int forcing_stage(fb_model *m, fb_slab *s)
{
    if (!m->fr_on) return FB_OK;
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[0];
    const SpecCoef coef = make_coef(c);
    const bool work = forcing_needs_work(m);
    cf *z = work ? m->fr_work : m->gb[0].ZA;
    int rc;
    if (work && (rc = export_state(m, 0, z))) return rc;
    const int nwg = grid_for(c, priv_elems(c) / 2);
    const double grids = (double)c->nx * c->ny;
    if ((rc = launch(c, k_forcing_stage<true>, dim3(nwg), dim3(256), 0, coef, m->fr, z, c->P, c->N1, c->N2, (const unsigned long long *)forcing_clock(m), m->fr_part)) ||
        (rc = launch(c, k_forcing_final, dim3(1), dim3(256), 0, (const double *)m->fr_part, nwg, 1.0 / (grids * grids), forcing_totals(m), forcing_clock(m))))
        return rc;
    if (m->xpass != XP_COLS)
        rc = launch(c, k_full_relayout<true>, dim3(c->max_wg), dim3(256), 0, (const cf *)z, m->gb[0].ZA, c->P, c->N1, c->N2, (c->ny / 2) / 8, (int)m->xpass, c->hy);
    else if (work) rc = state_convert(c, G, z, m->gb[0].ZA, true);
    if (rc) return rc;
    for (int k = 0; k < m->tg.n && m->fr.decays; ++k)
        if ((rc = launch(c, k_forcing_stage<false>, dim3(nwg), dim3(256), 0, coef, m->fr, m->tg.v[k].c0[0], c->P, c->N1, c->N2, (const unsigned long long *)nullptr, (double *)nullptr)))
            return rc;
    if (m->xpass != XP_COLS) {
        if ((rc = launch_col_full(m, 4))) return rc;
        m->primed = 2;
        return FB_OK;
    }
    if ((rc = model_prime(m))) return rc;
    if (s) return FB_OK;                                    // primed == 1: the slab's next stage starts with the backward sub-pass
    if ((rc = model_col_bwd_active(m))) return rc;
    m->primed = 2;
    return FB_OK;
}

// The ring on the host, from the tables the kernels read: N_ring over the full spectrum (a stored mode with 0 < j < ny/2 counts
// twice), and whether it holds a mode outside the dealiasing circle.  The ring test is the kernel's, in float64.
static void forcing_ring(const fb_ctx *c, double kf, double dk, long long *nring, bool *masked)
{
    *nring = 0; *masked = false;
    for (int i = 0; i < c->nx; ++i) {
        const int ii = i < c->nx - i ? i : c->nx - i;
        for (int j = 0; j < c->hy; ++j) {
            if ((i == 0 || 2 * i == c->nx) && (j == 0 || j == c->ny / 2)) continue;
            const double K2 = -(double)(float)(-(c->h_kx2[i] + c->h_ky2[j]));
            if (!(fabs(sqrt(K2) - kf) <= dk)) continue;
            *nring += (j == 0 || j == c->ny / 2) ? 1 : 2;
            if ((double)ii * ii + (double)j * j >= c->gws) *masked = true;
        }
    }
}

// The forcing in (rate = mu = nu_p = 0 removes it); the clock and the totals start at zero.  The captured step is dropped either way.
static int forcing_in(const Call &k, double rate, double kf, double dk, size_t seed, double mu, double nu_p, int p)
{
    fb_model *m = k.m;
    fb_ctx *c = m->c;
    int rc;
    const bool off = rate == 0.0 && mu == 0.0 && nu_p == 0.0;
    long long nring = 0;
    if (rate > 0.0) {
        bool masked = false;
        forcing_ring(c, kf, dk, &nring, &masked);
        if (nring == 0) return refuse(k, "the ring |K - k| <= width holds no mode of this grid");
        if (masked) return refuse(k, "the ring |K - k| <= width holds a mode outside the dealiasing circle");
    }
    if ((rc = beside_begin(m, off && m->fr_on))) return rc;
    if (off) { forcing_free(m); return FB_OK; }
    if ((forcing_needs_work(m) && (rc = rec_alloc((void **)&m->fr_work, priv_elems(c) * sizeof(cf)))) ||
        (rc = rec_alloc((void **)&m->fr_part, 4 * (size_t)c->max_wg * sizeof(double))) || (rc = rec_alloc((void **)&m->fr_dev, 5 * sizeof(double)))) {
        forcing_free(m);
        return rc;
    }
    HIPCHK(hipMemsetAsync(m->fr_dev, 0, 5 * sizeof(double), c->stream));
    ForcingArgs &f = m->fr;
    f.mu = mu; f.nu_p = nu_p; f.dt = (double)m->dt; f.p = p;
    f.kf = rate > 0.0 ? kf : 0.0; f.dk = rate > 0.0 ? dk : 0.0;
    f.lo2 = (f.kf - f.dk) * (f.kf - f.dk) * (1.0 - 1e-12); f.hi2 = (f.kf + f.dk) * (f.kf + f.dk) * (1.0 + 1e-12);
    f.a2 = rate > 0.0 ? 2.0 * rate * f.dt / (double)nring : 0.0;
    f.grids = (double)c->nx * c->ny;
    f.seed_lo = (unsigned)((unsigned long long)seed & 0xffffffffull); f.seed_hi = (unsigned)((unsigned long long)seed >> 32);
    f.ny2 = c->ny / 2;
    f.forced = rate > 0.0; f.decays = mu > 0.0 || nu_p > 0.0;
    m->fr_nring = (int)nring;
    m->fr_on = true;
    return FB_OK;
}

// a slab of one rank goes through the same code; on several ranks the split stage is refused
constexpr unsigned FORCING = NEED_TRANSPORT | ONE_RANK_FORCING, FORCING_SET = FORCING | NEED_FORCING;

static int set_forcing(const Call &k, double rate, double kf, double dk, size_t seed, double mu, double nu_p, int p)
{
    auto bad = [](double v) { return !std::isfinite(v) || v < 0.0; };
    if (bad(rate)) return refuse(k, "rate must be finite and >= 0");
    if (bad(mu)) return refuse(k, "mu must be finite and >= 0");
    if (bad(nu_p)) return refuse(k, "nu_p must be finite and >= 0");
    if (p < 1 || p > 8) return refuse(k, "p outside [1, 8]");
    if (rate > 0.0 && (bad(kf) || bad(dk))) return refuse(k, "k_f and dk must be finite and >= 0");
    if (int rc = enter(k, FORCING)) return rc;
    if (rate > 0.0 && !(kf - dk > 0.0)) return refuse(k, "k_f - dk must be > 0");          // what the ring is refused for: after the handle, before any HIP call
    if (k.m->ad_tape) return refuse(k, "not while the adjoint's tape or a checkpointed window exists: the adjoint of the split stage is not built (fb_model_adjoint_record, fb_model_adjoint_checkpoint)", FB_EUNSUPPORTED);
    return forcing_in(k, rate, kf, dk, seed, mu, nu_p, p);
}
extern "C" int fb_model_set_forcing(fb_model *m, double rate, double k_f, double dk, size_t seed, double mu, double nu_p, int p)
{
    return set_forcing(on_model("fb_model_set_forcing", m), rate, k_f, dk, seed, mu, nu_p, p);
}
extern "C" int fb_slab_set_forcing(fb_slab *s, double rate, double k_f, double dk, size_t seed, double mu, double nu_p, int p)
{
    return set_forcing(on_slab("fb_slab_set_forcing", s), rate, k_f, dk, seed, mu, nu_p, p);
}

// out[6] on the host: the clock, dE_forc, dE_diss, dZ_forc, dZ_diss, N_ring (waits for the stream)
static int forcing_budget(const Call &k, double *out)
{
    if (!out) return refuse(k, "NULL output");
    if (int rc = enter(k, FORCING_SET)) return rc;
    const fb_model *m = k.m;
    unsigned long long h[5];
    HIPCHK(hipMemcpyAsync(h, m->fr_dev, sizeof(h), hipMemcpyDeviceToHost, m->c->stream));
    HIPCHK(hipStreamSynchronize(m->c->stream));
    out[0] = (double)h[0];
    memcpy(out + 1, h + 1, 4 * sizeof(double));
    out[5] = (double)m->fr_nring;
    return FB_OK;
}
extern "C" int fb_model_forcing_budget(fb_model *m, double *out) { return forcing_budget(on_model("fb_model_forcing_budget", m), out); }
extern "C" int fb_slab_forcing_budget(fb_slab *s, double *out) { return forcing_budget(on_slab("fb_slab_forcing_budget", s), out); }

// Delta_n of clock value n into d_spec, a device array [nx][ny/2+1] complex in the public spectrum layout
static int forcing_increment(const Call &k, size_t n, float *d_spec)
{
    if (!d_spec) return refuse(k, "NULL output");
    if (int rc = enter(k, FORCING_SET)) return rc;
    const fb_model *m = k.m;
    const fb_ctx *c = m->c;
    const size_t total = (size_t)c->nx * c->hy;
    return launch_n(c, k_forcing_increment, total, make_coef(c), m->fr, (unsigned long long)n, (cf *)d_spec, total);
}
extern "C" int fb_model_forcing_increment(fb_model *m, size_t n, float *d_spec) { return forcing_increment(on_model("fb_model_forcing_increment", m), n, d_spec); }
extern "C" int fb_slab_forcing_increment(fb_slab *s, size_t n, float *d_spec) { return forcing_increment(on_slab("fb_slab_forcing_increment", s), n, d_spec); }
