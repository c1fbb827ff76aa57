// fb_entry.h -- the entry layer of the model's C ABI (included by fb_slab_driver.h once fb_slab is defined; C ABI: include/fftbaro.h).
//
// Every fb_model_X / fb_slab_X[_local] pair is ONE static body that takes a Call -- whom the call acts on, and under which name --
// and the pair's own arguments; the two extern "C" functions forward to it in one line each.  A body refuses in one order, before any
// HIP call, and every message starts with the entry point's own name (refuse):
//   1. arguments that need no handle: NULL outputs, kappa, kind, the factor, nbins, depth, nsteps, n        (the body)
//   2. the NULL handle                                                                                     (have_handle, enter)
//   3. arguments that need the grid: pres_check, azim_check                                                (the body, after have_handle)
//   4. one rank only   5. the feature is not set   6. no transport connected                               (enter)
#pragma once

struct Call { const char *fn; fb_model *m; fb_slab *s; bool slab; };     // m: the model, a slab's own for a slab; s: NULL for a model
static Call on_model(const char *fn, fb_model *m) { return Call{fn, m, nullptr, false}; }
static Call on_slab(const char *fn, fb_slab *s) { return Call{fn, s ? s->m : nullptr, s, true}; }

static int refuse(const Call &k, const std::string &what, int code = FB_EINVAL) { return fail(code, std::string(k.fn) + ": " + what); }
static int have_handle(const Call &k) { return k.m ? FB_OK : refuse(k, k.slab ? "NULL slab" : "NULL model"); }

// what an entry point needs of its handle
enum : unsigned {
    NEED_TRANSPORT = 1,         // a slab: connected (fb_slab_connect_*; a slab of one rank is from creation).  A model: not a slab's own, driven phase by phase
    NEED_TRACER = 2, NEED_TANGENT = 4, NEED_ADJOINT = 8, NEED_PARTICLES = 16,       // the feature is set
    ONE_RANK_TANGENT = 32, ONE_RANK_ADJOINT = 64, ONE_RANK_PARTICLES = 128,         // refused on a slab of several ranks
    NEED_DEFORMATION = 256,     // the particles carry their deformation gradient (after NEED_PARTICLES: no particles is the first refusal)
    ONE_RANK_CENSUS = 512,      // refused on a slab of several ranks
    ONE_RANK_FORCING = 1024,    // likewise
    NEED_FORCING = 2048,        // forcing, drag or hyperviscosity is set (fb_model_set_forcing)
};
static const struct { unsigned need; const char *who; int code; } ONE_RANK[] = {
    {ONE_RANK_TANGENT, "the tangent-linear model is", FB_EINVAL},
    {ONE_RANK_ADJOINT, "the adjoint model is", FB_EINVAL},
    // particles distributed over row slabs would need neighbour halo rows that the all-to-all transport does not provide
    {ONE_RANK_PARTICLES, "particles are", FB_EUNSUPPORTED},
    // a structure that crosses the ranks' row slabs would need a border merge over the ranks
    {ONE_RANK_CENSUS, "the vortex census is", FB_EUNSUPPORTED},
    // the budget's sums and the re-priming after the split stage are built for the one column group of one rank
    {ONE_RANK_FORCING, "the stochastic forcing is", FB_EUNSUPPORTED},
};
static const struct { unsigned need; bool (*set)(const fb_model *); const char *refusal; } FEATURE[] = {
    {NEED_TRACER, [](const fb_model *m) { return m->tracer; }, "no tracer is set"},
    {NEED_TANGENT, [](const fb_model *m) { return m->tg.n != 0; }, "no tangent is set"},
    {NEED_ADJOINT, [](const fb_model *m) { return m->ad.n != 0; }, "no adjoint is set"},
    {NEED_PARTICLES, [](const fb_model *m) { return m->pt_n != 0; }, "no particles are set"},
    {NEED_DEFORMATION, [](const fb_model *m) { return m->pd != nullptr; }, "no particle deformation is set (fb_model_set_particle_deformation)"},
    {NEED_FORCING, [](const fb_model *m) { return m->fr_on; }, "no forcing is set (fb_model_set_forcing)"},
};

// every refusal that depends on the handle alone
static int enter(const Call &k, unsigned needs = 0)
{
    if (int rc = have_handle(k)) return rc;
    const fb_model *m = k.m;
    for (const auto &r : ONE_RANK)
        if ((needs & r.need) && m->c->world > 1) return refuse(k, std::string(r.who) + " not supported on a slab of several ranks (world > 1)", r.code);
    for (const auto &f : FEATURE)
        if ((needs & f.need) && !f.set(m)) return refuse(k, f.refusal);
    if (!(needs & NEED_TRANSPORT)) return FB_OK;
    if (k.slab) return k.s->connected ? FB_OK : refuse(k, "the slab is not connected to a transport (fb_slab_connect_*)");
    return m->c->world == 1 && !m->phase_flow ? FB_OK : refuse(k, "a slab's own model: use the fb_slab_* entry point");
}
