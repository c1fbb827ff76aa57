// fb_record.h -- state in and the record outputs of a model (included by fftbaro.hip after fb_slab_driver.h; C ABI: include/fftbaro.h).
//
// One layer serves the one-GPU model (fb_model_*, s == NULL) and a rank of a slab (fb_slab_*, this rank's rows).  A record is, per
// column group: the export of vort_c into the model's record workspace, the spectral kernel of its kind (none for the vorticity;
// k_psi_private for psi, u, v; k_ow_spec; k_keff_spec; k_pres_spec; k_spectra_deriv), the backward x pass; on a slab of several ranks one all-to-all per group in
// the reverse roles; then the row pass with the kind's epilogue (the pressure and the spectra go on from there: record_pres, record_spectra).  The record buffers are the model's own (rec_work, rec_send): a record
// never writes the step's buffers (ZA, ZB, ACC, w4_*, t_*).
#pragma once

// ---- state in (fb_model_set_vort, fb_slab_set_vort_local) ----
// readField + fftwf_execute(p_fwd_vort), main.cpp:143-144,256: y transform of the local rows into t_send -> transpose (slab) -> x
// transform of the local columns in t_recv -> the state's layout.  One GPU: t_send == t_recv.
static int state_in(fb_model *m, fb_slab *s, const float *d_rows)
{
    fb_ctx *c = m->c;
    int rc;
    state_replaced(m);
    if (!s) HIPCHK(hipMemsetAsync(m->gb[0].t_send, 0, priv_elems(c) * sizeof(cf), c->stream));      // pad columns zero
    RowArgs a = row_args_base(c);
    a.rin = d_rows;
    const cf *ts[3] = {m->gb[0].t_send, m->gb[1].t_send, m->gb[2].t_send};
    cf *const tr[3] = {m->gb[0].t_recv, m->gb[1].t_recv, m->gb[2].t_recv};
    a.T = c->world == 1 ? view_single(c, m->gb[0].t_send, 0) : view_slab(c, ts, 1);
    if ((rc = launch_row<ROW_FWD>(c, a)) || (s && (rc = slab_rows_to_cols(s, ts, tr, c->ngroups)))) return rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        cf *t = m->gb[g].t_recv;
        if ((rc = launch_col_strided<-1>(c, G, t, 1, 0)) || (rc = launch_col_block<-1>(c, G, t, 1, 0))) return rc;
        if ((rc = m->xpass != XP_COLS ? full_import_state(m, t) : state_convert(c, G, t, m->gb[g].ZA, true))) return rc;
    }
    return FB_OK;
}

static int set_vort(const Call &k, const float *d_rows)
{
    if (!d_rows) return refuse(k, "NULL input");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return state_in(k.m, k.s, d_rows);
}
extern "C" int fb_model_set_vort(fb_model *m, const float *d_vort) { return set_vort(on_model("fb_model_set_vort", m), d_vort); }
extern "C" int fb_slab_set_vort_local(fb_slab *s, const float *d_rows) { return set_vort(on_slab("fb_slab_set_vort_local", s), d_rows); }

// ---- the record layer ----
enum RecKind { REC_VORT, REC_PSI, REC_U, REC_V, REC_OW, REC_KEFF, REC_PRES };

// a device array: on failure *p == NULL, the runtime's last error is cleared (the next launch's check must not find it) and `what`
// is the message of FB_ENOMEM
static int dev_alloc(void **p, size_t bytes, const char *what)
{
    if (hipMalloc(p, bytes) == hipSuccess) return FB_OK;
    *p = nullptr;
    (void)hipGetLastError();
    return fail(FB_ENOMEM, what);
}
template <class T> static void dev_free(T *&p)
{
    if (p) { hipFree(p); p = nullptr; }
}

// a buffer of the record path: allocated on first use, then kept
static int rec_alloc(void **p, size_t bytes)
{
    return *p ? FB_OK : dev_alloc(p, bytes, "record-path allocation failed");
}
// a scratch buffer of the record path, grown to the largest request (hipFree waits for the device)
static int rec_reserve(void **p, size_t *cap, size_t bytes)
{
    if (*p && *cap >= bytes) return FB_OK;
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; *cap = 0; }
    const int rc = rec_alloc(p, bytes);
    if (!rc) *cap = bytes;
    return rc;
}

// nf fields (one, three, or four for the spectra) of every column group, through the backward x pass in rec_work[g], to the row pass: *M is its view.  One
// GPU: rec_work itself.  A slab of several ranks: one all-to-all per group (columns -> rows).
static int record_to_rows(fb_model *m, fb_slab *s, int nf, RowView *M)
{
    fb_ctx *c = m->c;
    int rc;
    if (!(s && c->world > 1)) { *M = view_single(c, m->rec_work[0], (long)priv_elems(c)); return FB_OK; }
    // [nf][nx][ncols] == [nf][dst][XL][ncols].  Several fields are regrouped into rec_send as [dst][nf][XL][ncols] (each peer's blocks
    // contiguous) and come back into rec_work as [src][nf][XL][ncols]; one field leaves rec_work as it is and arrives in rec_send.
    for (int g = 0; g < c->ngroups && nf > 1; ++g) {
        const size_t blk = (size_t)c->XL * c->grp[g].ncols;
        for (int f = 0; f < nf && blk; ++f)
            HIPCHK(hipMemcpy2DAsync(m->rec_send[g] + f * blk, nf * blk * sizeof(cf), m->rec_work[g] + f * c->world * blk, blk * sizeof(cf),
                                    blk * sizeof(cf), c->world, hipMemcpyDeviceToDevice, c->stream));
    }
    cf *const *send = nf > 1 ? m->rec_send : m->rec_work, *const *recv = nf > 1 ? m->rec_work : m->rec_send;
    if ((rc = slab_after(s->comm, s->comp, s->ev_misc[0]))) return rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const size_t blk = nf * (size_t)c->XL * c->grp[g].ncols;
        if ((rc = slab_xchg(s, send[g], recv[g], blk, 0, blk))) return rc;
    }
    if ((rc = slab_after(s->comp, s->comm, s->ev_misc[1]))) return rc;
    const cf *v[3] = {recv[0], recv[1], recv[2]};
    *M = view_slab(c, v, nf);
    return FB_OK;
}

// The record fields of `kind` (one, or three for REC_OW / REC_KEFF / REC_PRES) of every column group through the backward x pass in
// rec_work[g] ([3][nx][ncols_g], field 0 for one field), and on a slab of several ranks their exchange; *M: the row pass's view.
// of: the record is taken of a field stepped beside the vorticity (the base arrays of the tracer or of the tangent-linear model, in the
// 3-pass layout already) in the place of the vorticity.
static int record_fields(fb_model *m, fb_slab *s, RecKind kind, RowView *M, cf *const *of = nullptr)
{
    fb_ctx *c = m->c;
    const int nf = kind >= REC_OW ? 3 : 1;
    const bool xchg = s && c->world > 1;
    int rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        if ((rc = rec_alloc((void **)&m->rec_work[g], 3 * n * sizeof(cf))) || (xchg && (rc = rec_alloc((void **)&m->rec_send[g], 3 * n * sizeof(cf))))) return rc;
        cf *z = m->rec_work[g];
        // copy of vort_c in the 3-pass layout into field 0 (main.cpp:273), then the kind's fields from it in place
        if (of) HIPCHK(hipMemcpyAsync(z, of[g], n * sizeof(cf), hipMemcpyDeviceToDevice, c->stream));
        else if ((rc = export_state(m, g, z))) return rc;
        const SpecCoef k = make_coef(c);
        rc = FB_OK;                                         // (REC_VORT: the state as it is)
        if (kind >= REC_OW) {
            const auto spec = kind == REC_OW ? k_ow_spec : kind == REC_KEFF ? k_keff_spec : k_pres_spec;
            rc = launch_n(c, spec, n, k, (const cf *)z, z, (long)n, G.ncols, c->N1, c->N2, G.ky0);
        } else if (kind != REC_VORT)
            rc = dispatch<3>(kind - REC_PSI, [&](auto W) { return launch_n(c, k_psi_private<W()>, n, k, z, G.ncols, c->N1, c->N2, G.ky0); });
        if (rc) return rc;
        if ((rc = launch_col_block<+1>(c, G, z, nf, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, nf, (long)n))) return rc;
    }
    return record_to_rows(m, s, nf, M);
}

// One record into the rows of this rank (one GPU: every row), normalised by 1/GRIDS: REC_VORT, REC_PSI, REC_U, REC_V into out0;
// REC_OW: W into out0 and tau_fil into out1 (either may be NULL); REC_KEFF: zeta into out0 and |grad zeta|^2 into out1.
static int record(fb_model *m, fb_slab *s, RecKind kind, float *out0, float *out1 = nullptr, cf *const *of = nullptr)
{
    fb_ctx *c = m->c;
    RowArgs a = row_args_base(c);
    int rc;
    if ((rc = record_fields(m, s, kind, &a.M, of))) return rc;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    a.scale = kind == REC_U ? -g : g;                   // u = -dpsi/dy: normalise, then negate (SURVEY note N3): (x * g) * -1 == x * (-g) exactly
    a.rout = out0; a.rin = out1;                        // (ROW_OW, ROW_KEFF: rin carries the second output, fb_kernels.h row_rout2)
    if (kind == REC_OW) return launch_row<ROW_OW>(c, a);
    if (kind == REC_KEFF) return launch_row<ROW_KEFF>(c, a);
    return launch_row<ROW_INV>(c, a);
}

// the stage-0 record dumps of main.cpp:181-222 (any may be NULL): psi, u = -dpsi/dy, v = dpsi/dx
static int record_diag(fb_model *m, fb_slab *s, float *d_psi, float *d_u, float *d_v)
{
    float *out[3] = {d_psi, d_u, d_v};
    int rc;
    for (int k = 0; k < 3; ++k)
        if (out[k] && (rc = record(m, s, (RecKind)(REC_PSI + k), out[k]))) return rc;
    return FB_OK;
}

// ---- effective eddy diffusivity: zeta and |grad zeta|^2 (REC_KEFF), then the table ----
static int keff_check(const Call &k, const double *d_table, int nbins)
{
    if (!d_table) return refuse(k, "NULL table");
    if (nbins < 2 || nbins > 4096) return refuse(k, "nbins outside [2, 4096]");
    return FB_OK;
}

// zeta and |grad zeta|^2 of this rank's rows -> the table [nbins][9] (fb_keff.h), on every rank.  One reduction buffer, f64 parts first:
//   sum_part [nwg][nbins], hist_send [world][nbins][2], hist_recv [world][nbins][2] (f64); cnt_part [nwg][nbins] (u32);
//   mm_part [nmm][2], mm_send [world][2], mm_recv [world][2] (f32).
// One GPU (s == NULL or world 1): the rank's results are written straight to the receive buffers.  A slab: two small all-gathers
// (slab_gather), behind the compute stream's work.
static int keff_finish(fb_model *m, fb_slab *s, int nbins, const float *zeta, const float *grad2, double *d_table, double kappa)
{
    fb_ctx *c = m->c;
    const int world = c->world;
    const size_t n = (size_t)c->XL * c->ny;
    const bool v4 = (((size_t)zeta | (size_t)grad2) & 15) == 0;          // n is a multiple of 4 (ny >= 64)
    const int nmm = grid_for(c, v4 ? n / 4 : n);
    // histogram workgroups: at least 32 Ki points each; the partials stay within ~12 MiB at 4096 bins
    const int cap = std::min(1024, std::max(256, (1 << 20) / nbins));
    const int nwg = (int)std::max<size_t>(1, std::min<size_t>((size_t)cap, (n + 32767) / 32768));
    const size_t nh = (size_t)nbins * 2;
    const size_t o_hsend = (size_t)nwg * nbins * sizeof(double), o_hrecv = o_hsend + (world > 1 ? world * nh * sizeof(double) : 0);
    const size_t o_cnt = o_hrecv + world * nh * sizeof(double), o_mm = o_cnt + (size_t)nwg * nbins * sizeof(unsigned);
    const size_t o_mmsend = o_mm + 2 * (size_t)nmm * sizeof(float), o_mmrecv = o_mmsend + 2 * (size_t)world * sizeof(float);
    const size_t bytes = o_mmrecv + 2 * (size_t)world * sizeof(float);
    int rc;
    if ((rc = rec_reserve(&m->keff_red, &m->keff_red_cap, bytes))) return rc;
    char *base = (char *)m->keff_red;
    double *sum_part = (double *)base, *hsend = (double *)(base + o_hsend), *hrecv = (double *)(base + o_hrecv);
    unsigned *cnt_part = (unsigned *)(base + o_cnt);
    float *mm_part = (float *)(base + o_mm), *mmsend = (float *)(base + o_mmsend), *mmrecv = (float *)(base + o_mmrecv);
    const bool xchg = s && world > 1;
    const dim3 one(1), blk(256);
    if ((rc = launch(c, v4 ? k_keff_minmax<true> : k_keff_minmax<false>, dim3(nmm), blk, 0, zeta, n, mm_part)) ||
        (rc = launch(c, k_keff_minmax_final, one, blk, 0, (const float *)mm_part, nmm, xchg ? mmsend : mmrecv, xchg ? world : 1)))
        return rc;
    if (xchg && (rc = slab_gather(s, mmsend, mmrecv, 2))) return rc;
    // dynamic LDS: 12 B per bin (histogram), 16 B per bin (table); the attribute once per kernel and device, for 4096 bins
    if ((rc = set_max_lds(c, (const void *)k_keff_hist<true>, 4096 * 12)) || (rc = set_max_lds(c, (const void *)k_keff_hist<false>, 4096 * 12)) ||
        (rc = set_max_lds(c, (const void *)k_keff_table, 4096 * 16)))
        return rc;
    if ((rc = launch(c, v4 ? k_keff_hist<true> : k_keff_hist<false>, dim3(nwg), blk, (size_t)nbins * 12, zeta, grad2, n, (const float *)mmrecv, world, nbins, cnt_part,
                     sum_part)) ||
        (rc = launch(c, k_keff_reduce, dim3((nbins + KEFF_RB - 1) / KEFF_RB), blk, 0, (const unsigned *)cnt_part, (const double *)sum_part, nwg, nbins,
                     xchg ? hsend : hrecv, xchg ? world : 1, nh)))
        return rc;
    if (xchg && (rc = slab_gather(s, hsend, hrecv, 2 * nh))) return rc;
    return launch(c, k_keff_table, one, blk, (size_t)nbins * 16, (const double *)hrecv, world, (const float *)mmrecv, nbins, (double)c->lx / c->nx, (double)c->ly / c->ny,
                  kappa, d_table);
}

// the row pass's outputs: the caller's, or the model's own buffers (keff_fields [2][XL][ny]) for those the caller does not want
// (of, kappa: the table of a field stepped beside the vorticity as record_fields takes it, with its diffusivity; NULL and nu for the vorticity's)
static int record_keff(fb_model *m, fb_slab *s, int nbins, double *d_table, float *zeta, float *grad2, cf *const *of, double kappa)
{
    const size_t n = (size_t)m->c->XL * m->c->ny;
    int rc;
    if ((!zeta || !grad2) && (rc = rec_alloc((void **)&m->keff_fields, 2 * n * sizeof(float)))) return rc;
    if (!zeta) zeta = m->keff_fields;
    if (!grad2) grad2 = m->keff_fields + n;
    if ((rc = record(m, s, REC_KEFF, zeta, grad2, of))) return rc;
    return keff_finish(m, s, nbins, zeta, grad2, d_table, kappa);
}

// ---- azimuthal means about a vortex centre (fb_azim.h): psi or zeta for the centre, then zeta, u, v and the table ----
extern "C" int fb_azimuthal_cols(int nmodes, int *ncols)
{
    if (!ncols) return fail(FB_EINVAL, "fb_azimuthal_cols: NULL");
    *ncols = 0;
    if (nmodes < 0 || nmodes > AZIM_MAX_MODES) return fail(FB_EINVAL, "fb_azimuthal_cols: nmodes outside [0, 8]");
    *ncols = AZIM_BASE_COLS + 2 * nmodes;
    return FB_OK;
}

static int azim_check(const Call &k, const fb_ctx *c, int mode, double xc, double yc, int nbins, double dr, int nmodes)
{
    if (mode != FB_CENTER_FIXED && mode != FB_CENTER_PSI_MIN && mode != FB_CENTER_VORT_MAX) return refuse(k, "unknown centre mode");
    const double lx = (double)c->lx, ly = (double)c->ly, dx = lx / c->nx, dy = ly / c->ny;
    if (mode == FB_CENTER_FIXED && !(std::isfinite(xc) && std::isfinite(yc) && xc >= 0.0 && xc < lx && yc >= 0.0 && yc < ly))
        return refuse(k, "the fixed centre must be finite with 0 <= xc < Lx, 0 <= yc < Ly");
    if (nbins < 2 || nbins > 4096) return refuse(k, "nbins outside [2, 4096]");
    if (nmodes < 0 || nmodes > AZIM_MAX_MODES) return refuse(k, "nmodes outside [0, 8]");
    if (!std::isfinite(dr)) return refuse(k, "dr is not finite");
    if (dr < std::min(dx, dy)) return refuse(k, "dr below min(dx, dy)");
    if ((double)nbins * dr > std::min(lx, ly) / 2) return refuse(k, "nbins * dr beyond min(Lx, Ly) / 2 (the minimum-image cell)");
    return FB_OK;
}

// the tile of k_azim_bin: of the shapes TX x TY = AZIM_TILE with TY = 4 .. 256 a divisor of ny, the one whose radii span the fewest
// bins; W = that span + 3, capped by 64 KiB of LDS (beyond the cap k_azim_bin adds a point to the global sums directly)
static void azim_tile(AzimGeo &g, int ns)
{
    int best = 0x7fffffff;
    for (int ty = 4; ty <= 256 && ty <= g.ny; ty *= 2) {
        if (g.ny % ty) continue;
        const int tx = AZIM_TILE / ty;
        const double span = std::hypot((tx - 1) * g.dx, (ty - 1) * g.dy) / g.dr;
        const int need = span < 1.0e6 ? (int)span + 3 : 1000003;
        if (need < best) { best = need; g.TX = tx; g.TY = ty; }
    }
    g.W = std::min(best, 65536 / (ns * (int)sizeof(double)));
}

template <int NM> static int azim_launch_bin(const fb_ctx *c, const AzimGeo &g, const float *zeta, const float *u, const float *v, const double *center, double *part)
{
    const int ns = AZIM_BASE_SUMS + 2 * NM, tiles = ((g.XL + g.TX - 1) / g.TX) * (g.ny / g.TY);
    int rc;
    if ((rc = set_max_lds(c, (const void *)k_azim_bin<NM>, 65536))) return rc;
    return launch(c, k_azim_bin<NM>, dim3(tiles), dim3(256), (size_t)g.W * ns * sizeof(double), g, zeta, u, v, center, part);
}

// The record's own buffers: azim_fields [2][XL][ny] (f32) and one reduction buffer, grown on demand:
//   part_send [world][nbins][ns], part_recv [world][nbins][ns] (a slab of several ranks; else the one part), cand_send [world][4],
//   cand_recv [world][4] (f64); pi [nparts] (i64); pk [nparts] (f32).
// The fields: psi (FB_CENTER_PSI_MIN only) into field 1 and its argmin, or zeta into field 0 and its argmax; then zeta into field 0,
// u into field 1, and v, the last record taken, into the record workspace where that record's row pass no longer reads or never
// read: field 1 of rec_work on one GPU, the largest group's rec_work on a slab of several ranks (its one field has left for
// rec_send by then).  On a slab two small all-gathers (slab_gather), as keff_finish: the ranks' candidates, then their sums; a
// rank's global row is rank * XL + local row.
static int record_azimuthal(fb_model *m, fb_slab *s, int mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table, double *d_center)
{
    fb_ctx *c = m->c;
    const int world = c->world, ns = AZIM_BASE_SUMS + 2 * nmodes;
    const bool xchg = s && world > 1;
    const size_t n = (size_t)c->XL * c->ny, np = (size_t)nbins * ns;
    const int nparts = grid_for(c, n);
    int rc;
    if ((rc = rec_alloc((void **)&m->azim_fields, 2 * n * sizeof(float)))) return rc;
    const size_t o_precv = (xchg ? world * np : 0) * sizeof(double), o_csend = o_precv + (xchg ? world : 1) * np * sizeof(double);
    const size_t o_crecv = o_csend + (xchg ? world : 0) * AZIM_ARG_W * sizeof(double), o_pi = o_crecv + (size_t)world * AZIM_ARG_W * sizeof(double);
    const size_t o_pk = o_pi + (size_t)nparts * sizeof(long long), bytes = o_pk + (size_t)nparts * sizeof(float);
    if ((rc = rec_reserve(&m->azim_red, &m->azim_red_cap, bytes))) return rc;
    char *base = (char *)m->azim_red;
    double *psend = (double *)base, *precv = (double *)(base + o_precv), *csend = (double *)(base + o_csend), *crecv = (double *)(base + o_crecv);
    long long *pi = (long long *)(base + o_pi);
    float *pk = (float *)(base + o_pk);
    float *f0 = m->azim_fields, *f1 = m->azim_fields + n;
    AzimGeo g;
    g.lx = (double)c->lx; g.ly = (double)c->ly; g.dx = g.lx / c->nx; g.dy = g.ly / c->ny; g.dr = dr;
    g.nbins = nbins; g.XL = c->XL; g.ny = c->ny; g.row0 = c->rank * c->XL;
    azim_tile(g, ns);
    // the centre
    bool have_zeta = false;
    if (mode == FB_CENTER_FIXED) {
        if ((rc = launch(c, k_azim_center, dim3(1), dim3(64), 0, (const double *)nullptr, world, xc, yc, c->ny, g.dx, g.dy, d_center))) return rc;
    } else {
        const bool vmax = mode == FB_CENTER_VORT_MAX;
        float *q = vmax ? f0 : f1;
        if ((rc = record(m, s, vmax ? REC_VORT : REC_PSI, q))) return rc;
        have_zeta = vmax;
        if ((rc = launch(c, vmax ? k_azim_arg<true> : k_azim_arg<false>, dim3(nparts), dim3(256), 0, (const float *)q, n, pk, pi)) ||
            (rc = launch(c, k_azim_arg_final, dim3(1), dim3(256), 0, (const float *)pk, (const long long *)pi, nparts, (const float *)q, (long long)c->rank * (long long)n,
                         xchg ? csend : crecv, xchg ? world : 1)))
            return rc;
        if (xchg && (rc = slab_gather(s, csend, crecv, 2 * AZIM_ARG_W))) return rc;
        if ((rc = launch(c, k_azim_center, dim3(1), dim3(64), 0, (const double *)crecv, world, 0.0, 0.0, c->ny, g.dx, g.dy, d_center))) return rc;
    }
    // the fields
    if (!have_zeta && (rc = record(m, s, REC_VORT, f0))) return rc;
    if ((rc = record(m, s, REC_U, f1))) return rc;
    float *f2 = nullptr;
    if (!xchg) f2 = (float *)(m->rec_work[0] + priv_elems(c));
    else {
        size_t cap = 0;
        for (int k = 0; k < c->ngroups; ++k) {
            const size_t have = (size_t)(m->rec_work_nf[k] ? m->rec_work_nf[k] : 3) * grp_elems(c, c->grp[k]) * sizeof(cf);
            if (m->rec_work[k] && have > cap) { cap = have; f2 = (float *)m->rec_work[k]; }
        }
        if (cap < n * sizeof(float)) return fail(FB_EUNSUPPORTED, "azimuthal record: the record workspace cannot hold a field of rows");
    }
    if ((rc = record(m, s, REC_V, f2))) return rc;
    // the sums and the table
    HIPCHK(hipMemsetAsync(psend, 0, np * sizeof(double), c->stream));
    if ((rc = dispatch<AZIM_MAX_MODES + 1>(nmodes, [&](auto NM) { return azim_launch_bin<NM()>(c, g, f0, f1, f2, d_center, psend); }))) return rc;
    if (xchg) {                                             // one copy of this rank's sums per peer
        for (int r = 1; r < world; ++r) HIPCHK(hipMemcpyAsync(psend + r * np, psend, np * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if ((rc = slab_gather(s, psend, precv, 2 * np))) return rc;
    }
    return launch(c, k_azim_table, dim3(1), dim3(256), (size_t)nbins * sizeof(double), (const double *)precv, xchg ? world : 1, nbins, nmodes, dr, g.dx, g.dy, d_table);
}

// ---- balanced pressure (REC_PRES): there and back ----
// invert_pres.cpp:135-185 on the resident state.  Per column group k_pres_spec and the backward x pass of the three masked second
// derivatives of psi (record_fields); the ROW_PRES row pass takes them to physical space, forms psi_xx psi_yy - psi_xy^2 in registers
// and emits its forward y transform (one GPU: in place over field 0 of rec_work, each row pair reads its rows of all three fields
// before it stores; a slab: into rec_send as [dst][XL][ncols], one all-to-all back into field 0 of rec_work = [nx][ncols]); the
// forward x pass as state_in runs it; the state once more into field 1 (free by now) and k_pres_solve; then one field back as
// every one-field record goes, and the reference point.
static int pres_check(const Call &k, const fb_ctx *c, int ref_x, int ref_y, long *flat)
{
    const long long at = (long long)ref_x + (long long)c->nx * ref_y;    // the reference's flat index (invert_pres.cpp:182), kept as it is
    if (ref_x < 0 || ref_y < 0 || at >= (long long)c->nx * c->ny) return refuse(k, "reference point outside the grid");
    *flat = (long)at;
    return FB_OK;
}

static int record_pres(fb_model *m, fb_slab *s, float rho, float f, long flat, float *out)
{
    fb_ctx *c = m->c;
    const int world = c->world;
    const bool xchg = s && world > 1;
    const float g = 1.0f / (float)((size_t)c->nx * c->ny);
    int rc;
    if ((rc = rec_alloc((void **)&m->pres_ref, 2 * (size_t)world * sizeof(float)))) return rc;
    RowArgs a = row_args_base(c);
    if ((rc = record_fields(m, s, REC_PRES, &a.M))) return rc;
    const cf *ts[3] = {m->rec_send[0], m->rec_send[1], m->rec_send[2]};
    a.T = xchg ? view_slab(c, ts, 1) : view_single(c, m->rec_work[0], 0);
    a.scale = g;
    if ((rc = launch_row<ROW_PRES>(c, a))) return rc;
    if (xchg && (rc = slab_rows_to_cols(s, m->rec_send, m->rec_work, c->ngroups))) return rc;
    const SpecCoef coef = make_coef(c);
    for (int k = 0; k < c->ngroups; ++k) {
        const ColGroup &G = c->grp[k];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        cf *z = m->rec_work[k];
        if ((rc = launch_col_strided<-1>(c, G, z, 1, 0)) || (rc = launch_col_block<-1>(c, G, z, 1, 0))) return rc;
        if ((rc = export_state(m, k, z + n))) return rc;
        if ((rc = launch_n(c, k_pres_solve, n, coef, (const cf *)(z + n), z, rho, f, G.ncols, c->N1, c->N2, G.ky0))) return rc;
        if ((rc = launch_col_block<+1>(c, G, z, 1, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 1, (long)n))) return rc;
    }
    RowArgs b = row_args_base(c);
    if ((rc = record_to_rows(m, s, 1, &b.M))) return rc;
    b.scale = g; b.rout = out;
    if ((rc = launch_row<ROW_INV>(c, b))) return rc;
    // the reference point: its owner's value to every rank (slab_gather of one float), then p -= p_ref over this rank's rows
    const size_t nloc = (size_t)c->XL * c->ny;
    const int owner = (int)((size_t)flat / nloc);
    float *ref_send = m->pres_ref, *ref_recv = m->pres_ref + world;
    const long at = (!xchg || owner == c->rank) ? (long)((size_t)flat - (size_t)owner * nloc) : -1;
    if ((rc = launch(c, k_pres_ref, dim3((world + 63) / 64), dim3(64), 0, (const float *)out, at, xchg ? ref_send : ref_recv, xchg ? world : 1))) return rc;
    if (xchg && (rc = slab_gather(s, ref_send, ref_recv, 1))) return rc;
    const float *ref = ref_recv + (xchg ? owner : 0);
    const bool v4 = ((size_t)out & 15) == 0;                // nloc is a multiple of 4 (ny >= 64)
    return launch_n(c, v4 ? k_pres_sub<true> : k_pres_sub<false>, v4 ? nloc / 4 : nloc, out, nloc, ref);
}

// ---- shell spectra and cascade fluxes: there and back, then the gather (fb_spectra.h) ----
// The record workspace of this kind alone is larger than three fields: one GPU keeps the four derivative fields and N = r2c(J) side by
// side (five fields; the state is exported once more over field 0 for the gather), a slab of several ranks four fields in rec_work
// and in rec_send.  A workspace that another kind allocated first is replaced (hipFree waits for the device); the other kinds go on
// using the larger one.
static int rec_grow(cf **p, unsigned char *have, size_t n, int nf)
{
    if (*p && (*have ? *have : 3) >= nf) return FB_OK;
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; *have = 0; }
    if (int rc = rec_alloc((void **)p, nf * n * sizeof(cf))) return rc;
    *have = (unsigned char)nf;
    return FB_OK;
}

extern "C" int fb_spectra_shells(int nx, int ny, float lx, float ly, int *nshells)
{
    if (!nshells) return fail(FB_EINVAL, "fb_spectra_shells: NULL");
    *nshells = 0;
    if (!(lx > 0.f) || !(ly > 0.f)) return fail(FB_EINVAL, "fb_spectra_shells: Lx, Ly must be positive");
    if (!fb_size_supported(nx, ny)) return fail(FB_EINVAL, "fb_spectra_shells: nx, ny must be powers of two in [64, 16384] or 3*2^k in [192, 3072]");
    *nshells = spec_nshells(spec_grid(nx, ny, lx, ly));
    return FB_OK;
}

// The advective tendency r2c(-u a_x - v a_y) of a scalar exactly as a stage of the step forms it, through the record workspace.  Per
// column group `fill(g, G, z, n)` writes the four derivative spectra a_x, a_y, grady psi, gradx psi into the fields 0..3 of rec_work
// (the workspace is grown to what this path needs first); then the backward x pass of the four fields (on a slab their exchange);
// the step's fused row pass without a source (c2r of the four fields, J = -u a_x - v a_y, its forward y transform) into the record
// workspace (one GPU: field 4 of rec_work; a slab: rec_send as [dst][XL][ncols] of the active groups, one all-to-all back into
// field 0 of rec_work = [nx][ncols]); the forward x pass of the active groups as state_in runs it.  advect_out(m, s, g): where group
// g's result lies, in the 3-pass layout.  The groups of frozen columns get none: every mode of theirs is masked.
static cf *advect_out(fb_model *m, fb_slab *s, int g)
{
    return s && m->c->world > 1 ? m->rec_work[g] : m->rec_work[g] + 4 * grp_elems(m->c, m->c->grp[g]);
}

static int advect_workspace(fb_model *m, fb_slab *s)
{
    fb_ctx *c = m->c;
    const bool xchg = s && c->world > 1;
    int rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const size_t n = grp_elems(c, c->grp[g]);
        if (n == 0) continue;
        if ((rc = rec_grow(&m->rec_work[g], &m->rec_work_nf[g], n, xchg ? 4 : 5)) || (xchg && (rc = rec_grow(&m->rec_send[g], &m->rec_send_nf[g], n, 4)))) return rc;
    }
    return FB_OK;
}

template <class Fill> static int record_advect(fb_model *m, fb_slab *s, Fill fill)
{
    fb_ctx *c = m->c;
    const bool xchg = s && c->world > 1;
    int rc;
    if ((rc = advect_workspace(m, s))) return rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        cf *z = m->rec_work[g];
        if ((rc = fill(g, G, z, n))) return rc;
        if ((rc = launch_col_block<+1>(c, G, z, 4, (long)n)) || (rc = launch_col_strided<+1>(c, G, z, 4, (long)n))) return rc;
    }
    RowArgs a = row_args_base(c);
    if ((rc = record_to_rows(m, s, 4, &a.M))) return rc;
    const size_t n0 = priv_elems(c);
    if (xchg) {
        const cf *ts[3] = {m->rec_send[0], m->rec_send[1], m->rec_send[2]};
        a.T = view_slab(c, ts, 1);
        a.t_frozen = 0;                                     // the frozen columns' transfer is masked: never read
    } else {
        HIPCHK(hipMemsetAsync(m->rec_work[0] + 4 * n0, 0, n0 * sizeof(cf), c->stream));       // pad columns zero
        a.T = view_single(c, m->rec_work[0] + 4 * n0, 0);
    }
    a.scale = 1.0f / (float)((size_t)c->nx * c->ny);
    if ((rc = launch_row<ROW_FUSED>(c, a, c->row))) return rc;             // main.cpp:151-227,237 without vort_src
    if (xchg && (rc = slab_rows_to_cols(s, m->rec_send, m->rec_work, c->nact))) return rc;
    for (int k = 0; k < c->nact; ++k) {
        const ColGroup &G = c->grp[k];
        if (grp_elems(c, G) == 0) continue;
        cf *nh = advect_out(m, s, k);
        if ((rc = launch_col_strided<-1>(c, G, nh, 1, 0)) || (rc = launch_col_block<-1>(c, G, nh, 1, 0))) return rc;
    }
    return FB_OK;
}

// record_advect of the vorticity itself (per column group: the state into field 0 of rec_work, k_spectra_deriv); the state once more
// (one GPU: field 0, a slab: field 1); k_spectra_gather over this rank's columns; on a slab the ranks' partial sums all-gathered as
// keff_finish gathers its histograms; k_spectra_table.  spec_red: [world][nshells][6] to send (a slab of several ranks),
// [world][nshells][6] received.
static int record_spectra(fb_model *m, fb_slab *s, double *d_table)
{
    fb_ctx *c = m->c;
    const int world = c->world;
    const bool xchg = s && world > 1;
    const SpecGrid sg = spec_grid(c->nx, c->ny, c->lx, c->ly);
    const int nshells = spec_nshells(sg);
    const size_t np = (size_t)nshells * SPEC_SUMS;
    int rc;
    if ((rc = rec_alloc(&m->spec_red, (xchg ? 2 : 1) * (size_t)world * np * sizeof(double)))) return rc;
    const SpecCoef coef = make_coef(c);
    auto fill = [&](int g, const ColGroup &G, cf *z, size_t n) -> int {
        int r;
        if ((r = export_state(m, g, z))) return r;
        return launch_n(c, k_spectra_deriv, n, coef, (const cf *)z, z, (long)n, G.ncols, c->N1, c->N2, G.ky0);
    };
    if ((rc = record_advect(m, s, fill))) return rc;
    SpecGroups sgr;
    memset(&sgr, 0, sizeof(sgr));
    for (int k = 0; k < c->ngroups; ++k) {
        const ColGroup &G = c->grp[k];
        const size_t n = grp_elems(c, G);
        if (n == 0) continue;
        const bool active = k < c->nact;
        cf *nh = advect_out(m, s, k), *st = xchg ? m->rec_work[k] + n : m->rec_work[k];
        if ((rc = export_state(m, k, st))) return rc;
        const int q = sgr.ng++;
        sgr.a[q] = st; sgr.nh[q] = active ? nh : nullptr; sgr.ncols[q] = G.ncols; sgr.ky0[q] = G.ky0;
    }
    double *send = (double *)m->spec_red, *recv = send + (xchg ? (size_t)world * np : 0);
    if ((rc = launch(c, k_spectra_gather, dim3(nshells), dim3(256), 0, sg, sgr, c->N1, c->N2, coef.gws_i, (double)m->nu, xchg ? send : recv, xchg ? world : 1, np))) return rc;
    if (xchg && (rc = slab_gather(s, send, recv, 2 * np))) return rc;
    return launch(c, k_spectra_table, dim3(1), dim3(256), 0, (const double *)recv, xchg ? world : 1, nshells, sg.dk, d_table);
}

// ---- the entry points: one body per fb_model_X / fb_slab_X[_local] pair (fb_entry.h) ----
static int get_vort(const Call &k, float *d_rows)
{
    if (!d_rows) return refuse(k, "NULL output");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return record(k.m, k.s, REC_VORT, d_rows);              // main.cpp:273-275
}
extern "C" int fb_model_get_vort(fb_model *m, float *d_vort) { return get_vort(on_model("fb_model_get_vort", m), d_vort); }
extern "C" int fb_slab_get_vort_local(fb_slab *s, float *d_rows) { return get_vort(on_slab("fb_slab_get_vort_local", s), d_rows); }

static int get_diag(const Call &k, float *d_psi, float *d_u, float *d_v)
{
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return record_diag(k.m, k.s, d_psi, d_u, d_v);
}
extern "C" int fb_model_get_diag(fb_model *m, float *d_psi, float *d_u, float *d_v) { return get_diag(on_model("fb_model_get_diag", m), d_psi, d_u, d_v); }
extern "C" int fb_slab_get_diag_local(fb_slab *s, float *d_psi, float *d_u, float *d_v) { return get_diag(on_slab("fb_slab_get_diag_local", s), d_psi, d_u, d_v); }

static int get_okubo_weiss(const Call &k, float *d_w, float *d_tau)
{
    if (!d_w && !d_tau) return refuse(k, "NULL outputs");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return record(k.m, k.s, REC_OW, d_w, d_tau);
}
extern "C" int fb_model_get_okubo_weiss(fb_model *m, float *d_w, float *d_tau) { return get_okubo_weiss(on_model("fb_model_get_okubo_weiss", m), d_w, d_tau); }
extern "C" int fb_slab_get_okubo_weiss_local(fb_slab *s, float *d_w_rows, float *d_tau_rows)
{
    return get_okubo_weiss(on_slab("fb_slab_get_okubo_weiss_local", s), d_w_rows, d_tau_rows);
}

// the table of the vorticity, or with NEED_TRACER of the tracer with its own diffusivity.  Collective on a slab: the ranks' (min, max)
// and histograms are all-gathered through the transport (keff_finish), every rank gets the whole table
static int get_eddy_diffusivity(const Call &k, unsigned of, int nbins, double *d_table, float *d_field, float *d_grad2)
{
    int rc;
    if ((rc = keff_check(k, d_table, nbins)) || (rc = enter(k, NEED_TRANSPORT | of))) return rc;
    fb_model *m = k.m;
    return record_keff(m, k.s, nbins, d_table, d_field, d_grad2, of ? m->tr.c0 : nullptr, of ? m->kappa : m->nu);
}
extern "C" int fb_model_get_eddy_diffusivity(fb_model *m, int nbins, double *d_table, float *d_zeta, float *d_grad2)
{
    return get_eddy_diffusivity(on_model("fb_model_get_eddy_diffusivity", m), 0, nbins, d_table, d_zeta, d_grad2);
}
extern "C" int fb_slab_get_eddy_diffusivity(fb_slab *s, int nbins, double *d_table, float *d_zeta_rows, float *d_grad2_rows)
{
    return get_eddy_diffusivity(on_slab("fb_slab_get_eddy_diffusivity", s), 0, nbins, d_table, d_zeta_rows, d_grad2_rows);
}

// collective on a slab: the reference point's value reaches every rank through the transport (record_pres)
static int get_pressure(const Call &k, float rho, float f, int ref_x, int ref_y, float *d_pres)
{
    if (!d_pres) return refuse(k, "NULL output");
    long flat = 0;
    int rc;
    if ((rc = have_handle(k)) || (rc = pres_check(k, k.m->c, ref_x, ref_y, &flat)) || (rc = enter(k, NEED_TRANSPORT))) return rc;
    return record_pres(k.m, k.s, rho, f, flat, d_pres);     // invert_pres.cpp:135-185
}
extern "C" int fb_model_get_pressure(fb_model *m, float rho, float f, int ref_x, int ref_y, float *d_pres)
{
    return get_pressure(on_model("fb_model_get_pressure", m), rho, f, ref_x, ref_y, d_pres);
}
extern "C" int fb_slab_get_pressure_local(fb_slab *s, float rho, float f, int ref_x, int ref_y, float *d_pres_rows)
{
    return get_pressure(on_slab("fb_slab_get_pressure_local", s), rho, f, ref_x, ref_y, d_pres_rows);
}

// collective on a slab: the ranks' centre candidates and sums are all-gathered through the transport (record_azimuthal), every rank
// gets the whole table and the centre
static int get_azimuthal(const Call &k, int center_mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table, double *d_center)
{
    if (!d_table || !d_center) return refuse(k, "NULL table or centre");
    int rc;
    if ((rc = have_handle(k)) || (rc = azim_check(k, k.m->c, center_mode, xc, yc, nbins, dr, nmodes)) || (rc = enter(k, NEED_TRANSPORT))) return rc;
    return record_azimuthal(k.m, k.s, center_mode, xc, yc, nbins, dr, nmodes, d_table, d_center);
}
extern "C" int fb_model_get_azimuthal(fb_model *m, int center_mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table, double *d_center)
{
    return get_azimuthal(on_model("fb_model_get_azimuthal", m), center_mode, xc, yc, nbins, dr, nmodes, d_table, d_center);
}
extern "C" int fb_slab_get_azimuthal(fb_slab *s, int center_mode, double xc, double yc, int nbins, double dr, int nmodes, double *d_table, double *d_center)
{
    return get_azimuthal(on_slab("fb_slab_get_azimuthal", s), center_mode, xc, yc, nbins, dr, nmodes, d_table, d_center);
}

// collective on a slab: the ranks' partial sums are all-gathered through the transport (record_spectra), every rank gets the whole table
static int get_spectra(const Call &k, double *d_table)
{
    if (!d_table) return refuse(k, "NULL table");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    return record_spectra(k.m, k.s, d_table);
}
extern "C" int fb_model_get_spectra(fb_model *m, double *d_table) { return get_spectra(on_model("fb_model_get_spectra", m), d_table); }
extern "C" int fb_slab_get_spectra(fb_slab *s, double *d_table) { return get_spectra(on_slab("fb_slab_get_spectra", s), d_table); }

// ---- the vortex census (fb_census.h): structures of a thresholded field labelled and measured ----
// The census's own buffers (cs_label, cs_ids [nx][ny] int32; cs_part, the scan's partials per tile of 1024 cells) are allocated at the
// first call and kept: not the record workspace, which a captured step reads.  In stream order: the table and the counts zeroed;
// labels by runs; the unions; the roots and their cell counts; the scan of the kept roots (tile counts, one workgroup over them,
// the ids); the sums; the table's last columns.  The caller's field and weight are read where they lie.
static int record_census(fb_model *m, const float *f, const float *w, int mode, float thr, int min_cells, int max_structures, double *d_table, int *d_count,
                         int *d_labels)
{
    fb_ctx *c = m->c;
    const size_t n = (size_t)c->nx * c->ny;
    const int ntiles = (int)(n / CENSUS_TILE), tile_grid = std::min(ntiles, c->max_wg);
    int rc;
    if ((rc = rec_alloc((void **)&m->cs_label, n * sizeof(int))) || (rc = rec_alloc((void **)&m->cs_ids, n * sizeof(int))) ||
        (rc = rec_alloc((void **)&m->cs_part, (size_t)ntiles * sizeof(int2))))
        return rc;
    if (!w) w = f;
    CensusGeo g;
    g.dx = (double)c->lx / c->nx; g.dy = (double)c->ly / c->ny; g.nx = c->nx; g.ny = c->ny; g.n = n;
    int *label = m->cs_label, *ids = m->cs_ids;
    HIPCHK(hipMemsetAsync(ids, 0, n * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(d_table, 0, (size_t)max_structures * CENSUS_COLS * sizeof(double), c->stream));
    if ((rc = launch_n(c, k_census_init, n, f, thr, mode, n, label)) || (rc = launch_n(c, k_census_merge, n, g, label)) ||
        (rc = launch_n(c, k_census_flatten, n, n, label, ids)))
        return rc;
    if ((rc = launch(c, k_census_tile_counts, dim3(tile_grid), dim3(256), 0, (const int *)label, (const int *)ids, ntiles, min_cells, m->cs_part)) ||
        (rc = launch(c, k_census_scan_tiles, dim3(1), dim3(1024), 0, m->cs_part, ntiles, d_count)) ||
        (rc = launch(c, k_census_ids, dim3(tile_grid), dim3(256), 0, (const int *)label, ids, (const int2 *)m->cs_part, ntiles, min_cells, max_structures, d_table)))
        return rc;
    const bool v4 = (((size_t)w | (size_t)d_labels) & 15) == 0;
    if ((rc = launch_n(c, v4 ? k_census_sums<true> : k_census_sums<false>, n / 4, g, (const int *)label, (const int *)ids, w, max_structures, d_table, d_labels))) return rc;
    return launch(c, k_census_table, dim3((max_structures + 255) / 256), dim3(256), 0, (const int *)d_count, w, max_structures, d_table);
}

// (the handle's refusals first, as sample: EngineSlab.census asks a slab of several ranks for its refusal before it shapes any buffer)
static int census(const Call &k, const float *d_field, const float *d_weight, int mode, float threshold, int min_cells, int max_structures, double *d_table,
                  int *d_count, int *d_labels)
{
    if (int rc = enter(k, NEED_TRANSPORT | ONE_RANK_CENSUS)) return rc;
    if (!d_field || !d_table || !d_count) return refuse(k, "NULL field, table or count");
    if (!std::isfinite(threshold)) return refuse(k, "the threshold is not finite");
    if (mode != FB_CENSUS_ABOVE && mode != FB_CENSUS_BELOW) return refuse(k, "mode outside {0, 1}");
    if (min_cells < 1 || min_cells > (1 << 30)) return refuse(k, "min_cells outside [1, 2^30]");
    if (max_structures < 1 || max_structures > FB_CENSUS_MAX) return refuse(k, "max_structures outside [1, 65536]");
    return record_census(k.m, d_field, d_weight, mode, threshold, min_cells, max_structures, d_table, d_count, d_labels);
}
extern "C" int fb_model_census(fb_model *m, const float *d_field, const float *d_weight, int mode, float threshold, int min_cells, int max_structures,
                               double *d_table, int *d_count, int *d_labels)
{
    return census(on_model("fb_model_census", m), d_field, d_weight, mode, threshold, min_cells, max_structures, d_table, d_count, d_labels);
}
extern "C" int fb_slab_census(fb_slab *s, const float *d_field, const float *d_weight, int mode, float threshold, int min_cells, int max_structures,
                              double *d_table, int *d_count, int *d_labels)
{
    return census(on_slab("fb_slab_census", s), d_field, d_weight, mode, threshold, min_cells, max_structures, d_table, d_count, d_labels);
}
