// fftbaro.hip -- C ABI (include/fftbaro.h) of the MI355X-native barotropic-vorticity engine.
// Host side: context/plan/tables, launch logic, model state machine.  Kernels: fb_kernels.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fftbaro.h"
#include "fb_kernels.h"
#include "fb_keff.h"
#include "fb_azim.h"
#include "fb_census.h"
#include "fb_spectra.h"
#include "fb_tracer.h"
#include "fb_particles.h"
#include "fb_tangent.h"
#include "fb_clv.h"
#include "fb_adjoint.h"
#include "fb_obs.h"
#include "fb_lagrangian.h"
#include "fb_replay.h"
#include "fb_forcing.h"
#include "fb_col_full.h"
#include "fb_row3.h"
#include "fb_row8.h"
#include "fb_rowh.h"
#include "fb_rowq.h"

// --------------------------------------------------------------------------------------------
// errors
// --------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) { g_last_error = msg; return code; }

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(FB_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

extern "C" const char *fb_strerror(int s)
{
    switch (s) {
    case FB_OK: return "ok";
    case FB_EINVAL: return "invalid argument";
    case FB_ENOMEM: return "out of memory";
    case FB_EHIP: return "HIP runtime error";
    case FB_EIO: return "I/O error";
    case FB_EUNSUPPORTED: return "unsupported grid size";
    default: return "unknown status";
    }
}
extern "C" const char *fb_last_error(void) { return g_last_error.c_str(); }
extern "C" void fb_internal_set_error(const char *msg) { g_last_error = msg ? msg : ""; }   // fb_fieldio.cpp, fb_slab_comm.cpp
extern "C" int fb_version(void) { return 201; }
extern "C" int fb_device_count(int *count)
{
    if (!count) return fail(FB_EINVAL, "fb_device_count: NULL");
    *count = 0;
    HIPCHK(hipGetDeviceCount(count));
    return FB_OK;
}
extern "C" int fb_set_device(int ordinal) { HIPCHK(hipSetDevice(ordinal)); return FB_OK; }

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
// powers of two 64..16384, or 3*2^k in 192..3072 (the reference's default NPTS = 768)
static bool size_ok(int n) { return (is_pow2(n) && n >= 64 && n <= 16384) || (n % 3 == 0 && is_pow2(n / 3) && n >= 192 && n <= 3072); }
extern "C" int fb_size_supported(int nx, int ny) { return size_ok(nx) && size_ok(ny); }

// --------------------------------------------------------------------------------------------
// context
// --------------------------------------------------------------------------------------------
// A set of local ky columns with a pitch of its own.  One GPU: one group holding every column.  Multi-GPU: groups
// 0 .. nact-1 = this rank's slabs of the ACTIVE columns (ky < world*KA: at least one mode inside the dealiasing circle, exchanged
// every RK stage; two groups where the stage is pipelined by column groups -- fb_slab_driver.h -- else one), the last group =
// its slab of the FROZEN columns beyond them (SURVEY note N1: their state never changes, so their derivative fields cross the
// links once, at priming).  A rank's active slab [rank*KA, (rank+1)*KA) is cut locally: group 0 holds its first columns, group 1
// the rest, so which rank owns which ky column does not depend on the cut.
struct ColGroup {
    int ncols;                  // local columns == pitch of every array of the group (multiple of 16)
    int ky0;                    // global ky of local column 0
    int nct_active;             // 16-column tiles that contain at least one unmasked ky
};

// The kernel of the fused row pass (the FWD / INV passes always run the generic one).  RK_ROWH2 is a model's, not a context's:
// it comes with the x pass XP_FULL2 (launch_fused_row).
enum RowKernel {
    RK_GENERIC,                 // k_row<ny> (Stockham) or k_row3<ny/3>
    RK_ROWQ,                    // ny = 4096: k_rowq, one real row per 4-wave workgroup
    RK_ROW8,                    // ny = 4096: k_row8, two rows per 512-thread workgroup (FB_ROWQ=0)
    RK_ROWH_8192,               // k_rowh<1>
    RK_ROWH_16384,              // k_rowh<2>
    RK_ROWH2,                   // ny = nx = 8192 on one GPU: k_rowh2, the last radix-2 step of the x transform fused in
};
// The x pass of a model's RK stage.  The value is k_col_full's nsub (nx / 4096).
enum XPass {
    XP_COLS = 0,                // the three column kernels: forward strided sub-pass, k_col_mid, backward strided sub-pass
    XP_FULL1 = 1,               // nx = 4096: k_col_full<., 1>
    XP_FULL2 = 2,               // nx = 8192: k_col_full<., 2>, with the row pass through k_rowh2
};

struct fb_ctx {
    int world, rank;            // slab decomposition: this process owns x rows [rank*XL, (rank+1)*XL)
    int XL;
    int ngroups, nact; ColGroup grp[3];   // nact active groups (1 or 2), then the frozen one if KF > 0
    int KA, KF, katot;          // world > 1: columns per rank of the active (all groups together) / frozen slabs, katot = world*KA
    int nx, ny, hy, P;          // P = grp[0].ncols: pitch of the private layouts on one GPU
    int N1, N2;                 // nx = N1*N2
    int jmax;                   // first ky with ky^2 >= gws: that column and all beyond are masked (fftwfop.cpp:57-61)
    float lx, ly;
    hipStream_t stream;
    RowKernel row;              // the fused row pass (choose_row_kernel)
    // device tables
    float *d_gx; double *d_kx2; float *d_gy; double *d_ky2; double gws;
    cf *d_tw_n1, *d_tw_n2, *d_tw_big, *d_tw_row_bwd, *d_tw_row_fwd, *d_tw_256;
    cf *d_tw_row3;              // W_ny^j for k_row3 (ny = 3*M) and the row kernels other than RK_GENERIC, else NULL
    cf *d_tw_4096;              // W_4096^j for k_rowh's sub-transforms
    cf *d_tw_2048;              // k_rowq's per-thread twiddle table (make_rowq_table)
    // the environment switches ("Switches"), read once by read_switches() when the context is created
    bool rowq_off, no_row8, no_rowh;                  // FB_ROWQ=0, FB_NO_ROW8, FB_NO_ROWH
    bool full_pass_off, full_noskip;                  // FB_FULL_PASS=0, FB_FULL_NOSKIP
    bool no_column_skip, no_prescale;                 // FB_NO_COLUMN_SKIP, FB_NO_PRESCALE
    bool full_keep_off;                               // FB_FULL_KEEP=0
    int pitch_extra;                                  // FB_PITCH_EXTRA (0 if unset)
    bool no_pitch_tune, pitch_tune, tune_verbose;     // FB_NO_PITCH_TUNE or FB_PITCH_EXTRA set, FB_PITCH_TUNE, FB_TUNE_VERBOSE
    bool nyq_frozen;            // the ky = ny/2 column lies outside the dealiasing circle (always on square grids)
    cf *d_scratch;              // nx*P complex, lazily allocated (standalone r2c / c2r)
    // host copies of the 1-D tables (fb_get_tables)
    std::vector<float> h_gx, h_gy; std::vector<double> h_kx2, h_ky2;
    int max_wg;                 // grid cap (persistent-style grids)
    int dev;                    // HIP device the context lives on
};

static void split_nx(int nx, int &N1, int &N2)
{
    if (nx % 3 == 0) { N1 = 24; N2 = nx / 24; return; }      // 3*2^k: a 24-row strided sub-pass (radix 3 x 8)
    switch (nx) {
    case 64: N1 = 8; N2 = 8; break;
    case 128: N1 = 16; N2 = 8; break;
    case 256: N1 = 16; N2 = 16; break;
    case 512: N1 = 32; N2 = 16; break;
    case 1024: N1 = 32; N2 = 32; break;
    case 2048: N1 = 64; N2 = 32; break;
    case 4096: N1 = 64; N2 = 64; break;
    case 8192: N1 = 128; N2 = 64; break;
    default: N1 = 128; N2 = 128; break;   // 16384
    }
}

static std::vector<cf> make_root_table(int n)
{
    std::vector<cf> t(n);
    for (int j = 0; j < n; ++j) {
        double a = -2.0 * M_PI * (double)j / (double)n;
        t[j].x = (float)cos(a); t[j].y = (float)sin(a);
    }
    return t;
}

// k_rowq's per-thread twiddles, [9][256] float4 = eighteen complex per thread t (fb_rowq.h): W_2048^{p t} (p = 1..7), W_256^{q (t & 63)}
// (q = 1..3), W_4096^{t}, for t < 64 W_64^{(t >> 3)(t & 7)}, and W_4096^{t + 256 e} for e = 1, 2, 3, 5, 6, 7; the very values of the root tables
static std::vector<cf> make_rowq_table()
{
    const std::vector<cf> r2048 = make_root_table(2048), r4096 = make_root_table(4096);
    std::vector<cf> tab(18 * 256);
    for (int t = 0; t < 256; ++t) {
        cf e[18];
        for (int p = 1; p < 8; ++p) e[p - 1] = r2048[(p * t) % 2048];
        for (int q = 1; q < 4; ++q) e[6 + q] = r2048[(8 * q * (t & 63)) % 2048];
        e[10] = r4096[t];
        e[11] = t < 64 ? r2048[(32 * (t & 7) * (t >> 3)) % 2048] : cf{0.f, 0.f};
        const int es[6] = {1, 2, 3, 5, 6, 7};
        for (int i = 0; i < 6; ++i) e[12 + i] = r4096[t + 256 * es[i]];
        for (int j = 0; j < 9; ++j) { tab[(j * 256 + t) * 2] = e[2 * j]; tab[(j * 256 + t) * 2 + 1] = e[2 * j + 1]; }
    }
    return tab;
}

// Stockham stage tables for a radix list walked in order (forward-sign values); layout must
// match stockham_stage(): offset(s) + (m*(R-1) + (q-1))*T + t
static std::vector<cf> make_row_table(int n, const std::vector<int> &radices)
{
    const int T = n / 16;
    std::vector<cf> t;
    int NS = 1;
    for (size_t s = 0; s < radices.size(); ++s) {
        const int R = radices[s];
        if (s > 0) {
            const int NB = 16 / R;
            for (int m = 0; m < NB; ++m)
                for (int q = 1; q < R; ++q)
                    for (int tt = 0; tt < T; ++tt) {
                        const int j = tt + m * T, k = j % NS;
                        double a = -2.0 * M_PI * (double)k * (double)q / ((double)NS * (double)R);
                        cf w; w.x = (float)cos(a); w.y = (float)sin(a);
                        t.push_back(w);
                    }
        }
        NS *= R;
    }
    return t;
}

template <int N> static std::vector<int> plan_radices(bool fwd)
{
    std::vector<int> r;
    for (int s = 0; s < RowPlan<N>::S; ++s) r.push_back(RowTw<N, false>::radix(s));
    if (fwd) r = std::vector<int>(r.rbegin(), r.rend());
    return r;
}

static std::vector<int> plan_radices_rt(int n, bool fwd)
{
    switch (n) {
    case 64: return plan_radices<64>(fwd);
    case 128: return plan_radices<128>(fwd);
    case 256: return plan_radices<256>(fwd);
    case 512: return plan_radices<512>(fwd);
    case 1024: return plan_radices<1024>(fwd);
    case 2048: return plan_radices<2048>(fwd);
    case 4096: return plan_radices<4096>(fwd);
    case 8192: return plan_radices<8192>(fwd);
    default: return plan_radices<16384>(fwd);
    }
}

template <typename T> static int upload(T **dptr, const std::vector<T> &h)
{
    HIPCHK(hipMalloc((void **)dptr, h.size() * sizeof(T)));
    HIPCHK(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return FB_OK;
}

static int autotune_pitch(fb_ctx *c);

// The engine's environment switches, read here once per context; nothing else in this file but slab_layout (which the
// host-side plan functions also call without a context) reads the environment.
static void read_switches(fb_ctx *c)
{
    auto set = [](const char *name) { return getenv(name) != nullptr; };
    const char *rowq = getenv("FB_ROWQ"), *full = getenv("FB_FULL_PASS"), *extra = getenv("FB_PITCH_EXTRA"), *keep = getenv("FB_FULL_KEEP");
    c->rowq_off = rowq && rowq[0] == '0';
    c->no_row8 = set("FB_NO_ROW8");
    c->no_rowh = set("FB_NO_ROWH");
    c->full_pass_off = full && full[0] == '0';
    c->full_noskip = set("FB_FULL_NOSKIP");
    c->no_column_skip = set("FB_NO_COLUMN_SKIP");
    c->no_prescale = set("FB_NO_PRESCALE");
    c->full_keep_off = keep && keep[0] == '0';
    c->pitch_extra = extra ? atoi(extra) : 0;
    c->no_pitch_tune = extra || set("FB_NO_PITCH_TUNE");          // a fixed pitch (FB_PITCH_EXTRA) disables the autotuner too
    c->pitch_tune = set("FB_PITCH_TUNE");
    c->tune_verbose = set("FB_TUNE_VERBOSE");
}

extern "C" int fb_create(fb_ctx **out, int nx, int ny, float lx, float ly) { return fb_create_slab(out, nx, ny, lx, ly, 0, 1); }

static int round16(int v) { return (v + 15) / 16 * 16; }

// The slab layout of an nx x ny grid on `world` ranks and the schedule of its multi-GPU stage (fb_slab_driver.h).  Also
// defined on one rank, where fb_create_slab replaces the column split by the pitch.  The only reader of the
// FB_SLAB_* switches.
struct SlabLayout {
    double gws;                 // dealiasing radius^2
    int jmax;                   // first ky with ky^2 >= gws: that column and all beyond are masked (fftwfop.cpp:57-61)
    int XL, KA, KF;             // rows per rank; columns per rank of the active and the frozen slabs
    int nact, cols[2];          // active column groups of a rank (1 or 2) and their columns (cols[1] = 0 with one group)
    int nfg, nch;               // field groups of the derivative exchange (1, 2 or 4), row chunks of the tendency exchange (1..8)
    bool two_streams;           // the exchanges go on a communication stream of their own
};

static SlabLayout slab_layout(int nx, int ny, int world)
{
    SlabLayout L;
    const int dxw = (int)ceil(((double)(float)nx) / 3.0), dyw = (int)ceil(((double)(float)ny) / 3.0);   // fftwfop.cpp:11-12
    L.gws = (double)(float)((double)dxw * dxw + (double)dyw * dyw);                                    // :57
    const int hy = ny / 2 + 1;
    L.jmax = 0;
    while (L.jmax < hy && (double)L.jmax * (double)L.jmax < L.gws) ++L.jmax;
    L.XL = nx / world;
    L.KA = round16((L.jmax + world - 1) / world);
    const int nf = hy - world * L.KA;
    L.KF = nf > 0 ? round16((nf + world - 1) / world) : 0;
    // How many column groups the ACTIVE columns of a rank are cut into (fb_slab_driver.h: with two, a stage's forward x pass,
    // update and backward x pass start on the first group while the second group's tendency is still on the links, and the first
    // group's derivative fields leave while the second group is computed).  Worth it where one group's column work hides a
    // collective's latency several times over: ~17.5 passes over nx*KA complex at ~5 TB/s.  FB_SLAB_COL_GROUPS=1|2 overrides.
    L.nact = 1;
    if (world > 1 && L.KA >= 32) {
        const double col_us = 17.5 * (double)nx * L.KA * 8.0 / 5e6;
        if (col_us >= 100.0) L.nact = 2;
        if (const char *e = getenv("FB_SLAB_COL_GROUPS")) { const int v = atoi(e); if (v == 1 || v == 2) L.nact = v; }
    }
    const int tiles = L.KA / 16;                           // whole 16-column tiles, the first group takes the odd one
    for (int g = 0; g < 2; ++g) L.cols[g] = g < L.nact ? 16 * (tiles / L.nact + (g < tiles % L.nact ? 1 : 0)) : 0;
    // Pipelining a transpose against the pass that feeds it hides that pass's time, minus one more collective's latency per
    // extra piece (tens of microseconds for a grouped RCCL send/recv).  So the derivative exchange is cut by fields only where one
    // field's backward sub-pass (2 * nx * KA * 8 bytes at ~5 TB/s) is worth an operation, and the tendency exchange by row chunks
    // only where half the row pass (5 * XL * (ny/2+1) * 8 bytes at ~4 TB/s) is.
    const double bwd_us = 2.0 * nx * L.KA * 8.0 / 5e6, row_us = 5.0 * L.XL * (ny / 2 + 1) * 8.0 / 4e6;
    L.nfg = world == 1 ? 1 : (bwd_us >= 20.0 ? 4 : (bwd_us >= 10.0 ? 2 : 1));
    L.nch = world == 1 ? 1 : (row_us >= 100.0 ? 2 : 1);
    if (const char *e = getenv("FB_SLAB_FIELD_GROUPS")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) L.nfg = v; }
    if (const char *e = getenv("FB_SLAB_ROW_CHUNKS")) { const int v = atoi(e); if (v >= 1 && v <= 8) L.nch = v; }
    while (L.nch > 1 && ((L.XL / L.nch) & 1 || L.XL % L.nch)) L.nch >>= 1;     // chunks are whole row pairs
    if (L.nact > 1) L.nfg = 1;                             // pipelined by column groups instead: a group's four fields leave together
    // Nothing to overlap when a stage has one field group and one row chunk (small slabs): the exchanges then go on the compute
    // stream, in order, and the stage has no cross-stream hand-overs (each costs the GPU ~10-15 us of idling; tools/slab_local_time.py:
    // rank-local 4096^2 step on 8 ranks 0.47 -> 0.3x ms).  FB_SLAB_TWO_STREAMS=1 keeps the separate communication stream.
    L.two_streams = L.nfg > 1 || L.nch > 1 || L.nact > 1 || getenv("FB_SLAB_TWO_STREAMS");
    return L;
}

// the kernel of the context's fused row pass; a model with the x pass XP_FULL2 runs k_rowh2 instead (launch_fused_row)
static RowKernel choose_row_kernel(const fb_ctx *c)
{
    if (c->ny == 4096 && !c->no_row8) return c->rowq_off ? RK_ROW8 : RK_ROWQ;
    if (c->ny == 8192 && !c->no_rowh) return RK_ROWH_8192;
    if (c->ny == 16384 && !c->no_rowh) return RK_ROWH_16384;
    return RK_GENERIC;
}

extern "C" int fb_create_slab(fb_ctx **out, int nx, int ny, float lx, float ly, int rank, int world)
{
    if (!out) return fail(FB_EINVAL, "fb_create: out is NULL");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world || !is_pow2(world) || (nx / world) < 2 || ((nx / world) & 1))
        return fail(FB_EINVAL, "fb_create_slab: world must be a power of two with an even nx/world >= 2, 0 <= rank < world");
    if (!fb_size_supported(nx, ny))
        return fail(FB_EUNSUPPORTED, "fb_create: nx, ny must be powers of two in [64, 16384] or 3*2^k in [192, 3072]");
    if (!(lx > 0.f) || !(ly > 0.f)) return fail(FB_EINVAL, "fb_create: Lx, Ly must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FB_EHIP, "fb_create: no HIP device (this engine has no CPU fallback)");

    fb_ctx *c = new fb_ctx();                              // value-initialised: every pointer NULL, so fb_destroy() is safe on any error path below
    read_switches(c);
    c->nx = nx; c->ny = ny; c->hy = ny / 2 + 1;
    c->world = world; c->rank = rank; c->XL = nx / world;
    split_nx(nx, c->N1, c->N2);
    c->lx = lx; c->ly = ly; c->stream = nullptr; c->d_scratch = nullptr;

    // ---- coefficient tables: fftwfop.cpp:5-79 ----
    const float TWOPI = (float)(acosf(-1.0f) * 2.0f);                  // fftwfop.hpp:7
    const int hx = nx / 2 + 1;
    const SlabLayout L = slab_layout(nx, ny, world);
    c->gws = L.gws; c->jmax = L.jmax;
    int Ptot;                                              // table length: every global ky a local column can map to
    if (world == 1) {
        c->P = round16(c->hy);
        c->P += 16 * c->pitch_extra;                       // tuning hook (disables the autotuner below)
        c->ngroups = c->nact = 1; c->grp[0] = ColGroup{c->P, 0, 0};
        c->KA = c->P; c->KF = 0; c->katot = c->P;
        Ptot = c->P + 96;                                  // room for the pitch candidates of autotune_pitch()
    } else {
        c->KA = L.KA; c->KF = L.KF;
        c->katot = world * c->KA;
        c->nact = L.nact;
        c->ngroups = c->nact + (c->KF > 0 ? 1 : 0);
        for (int g = 0; g < c->nact; ++g) c->grp[g] = ColGroup{L.cols[g], rank * c->KA + (g ? L.cols[0] : 0), 0};
        if (c->KF > 0) c->grp[c->nact] = ColGroup{c->KF, c->katot + rank * c->KF, 0};
        c->P = c->grp[0].ncols;
        Ptot = c->katot + world * c->KF + 16;
    }
    c->h_gx.assign(nx, 0.f); c->h_kx2.assign(nx, 0.0); c->h_gy.assign(Ptot, 0.f); c->h_ky2.assign(Ptot, 0.0);
    for (int i = 0; i < hx; ++i) c->h_gx[i] = TWOPI * ((float)i) / lx;            // :15-17
    for (int i = hx; i < nx; ++i) c->h_gx[i] = -c->h_gx[nx - i];                  // :18-20
    for (int j = 0; j < c->hy; ++j) c->h_gy[j] = TWOPI * ((float)j) / ly;         // :22-24
    for (int i = 0; i < nx; ++i) c->h_kx2[i] = (double)c->h_gx[i] * (double)c->h_gx[i];
    for (int j = 0; j < c->hy; ++j) c->h_ky2[j] = (double)c->h_gy[j] * (double)c->h_gy[j];

    c->nyq_frozen = ((double)(ny / 2) * (double)(ny / 2) >= c->gws);
    int rc;
    if ((rc = upload(&c->d_gx, c->h_gx)) || (rc = upload(&c->d_kx2, c->h_kx2)) ||
        (rc = upload(&c->d_gy, c->h_gy)) || (rc = upload(&c->d_ky2, c->h_ky2)) ||
        (rc = upload(&c->d_tw_n1, make_root_table(c->N1))) || (rc = upload(&c->d_tw_n2, make_root_table(c->N2))) ||
        (rc = upload(&c->d_tw_big, make_root_table(nx))) || (rc = upload(&c->d_tw_256, make_root_table(256))) ||
        (rc = upload(&c->d_tw_row_bwd, make_row_table(ny % 3 ? ny : ny / 3, plan_radices_rt(ny % 3 ? ny : ny / 3, false)))) ||
        (rc = upload(&c->d_tw_row_fwd, make_row_table(ny % 3 ? ny : ny / 3, plan_radices_rt(ny % 3 ? ny : ny / 3, true))))) {
        fb_destroy(c); return rc;
    }
    c->row = choose_row_kernel(c);
    // W_ny^j: k_row3, k_row8 and k_rowh read it.  k_rowq does not, but the table stays, so that the 4096^2 path allocates as it was measured.
    if ((ny % 3 == 0 || c->row != RK_GENERIC) && (rc = upload(&c->d_tw_row3, make_root_table(ny)))) { fb_destroy(c); return rc; }
    if ((c->row == RK_ROWH_8192 || c->row == RK_ROWH_16384) && (rc = upload(&c->d_tw_4096, make_root_table(4096)))) { fb_destroy(c); return rc; }
    if (c->row == RK_ROWQ && (rc = upload(&c->d_tw_2048, make_rowq_table()))) { fb_destroy(c); return rc; }
    hipDeviceProp_t prop;
    if (hipGetDevice(&c->dev) != hipSuccess || hipGetDeviceProperties(&prop, c->dev) != hipSuccess) {
        fb_destroy(c); return fail(FB_EHIP, "fb_create: cannot query the device");
    }
    c->max_wg = prop.multiProcessorCount * 8;
    if ((rc = autotune_pitch(c))) { fb_destroy(c); return rc; }
    *out = c;
    return FB_OK;
}

extern "C" int fb_destroy(fb_ctx *c)
{
    if (!c) return FB_OK;
    void *tabs[] = {c->d_gx, c->d_kx2, c->d_gy, c->d_ky2, c->d_tw_n1, c->d_tw_n2, c->d_tw_big, c->d_tw_row_bwd, c->d_tw_row_fwd, c->d_tw_256, c->d_tw_row3, c->d_tw_4096, c->d_tw_2048};
    for (void *t : tabs) if (t) hipFree(t);
    if (c->d_scratch) hipFree(c->d_scratch);
    delete c;
    return FB_OK;
}

extern "C" int fb_set_stream(fb_ctx *c, void *s) { if (!c) return fail(FB_EINVAL, "ctx NULL"); c->stream = (hipStream_t)s; return FB_OK; }
extern "C" int fb_synchronize(fb_ctx *c) { if (!c) return fail(FB_EINVAL, "ctx NULL"); HIPCHK(hipStreamSynchronize(c->stream)); return FB_OK; }

static SpecCoef make_coef(const fb_ctx *c)
{
    SpecCoef s; s.gx = c->d_gx; s.kx2 = c->d_kx2; s.gy = c->d_gy; s.ky2 = c->d_ky2; s.gws = c->gws; s.nx = c->nx; s.hy = c->hy;
    s.gws_i = c->gws >= 2147483647.0 ? 2147483647 : (int)ceil(c->gws);
    return s;
}

extern "C" int fb_get_tables(fb_ctx *c, float *gx, float *gy, float *lap, float *lapi, float *mask)
{
    if (!c) return fail(FB_EINVAL, "ctx NULL");
    const int nx = c->nx, hy = c->hy;
    if (gx) memcpy(gx, c->h_gx.data(), sizeof(float) * nx);
    if (gy) memcpy(gy, c->h_gy.data(), sizeof(float) * hy);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < hy; ++j) {
            const size_t k = (size_t)i * hy + j;
            const float l = (float)(-(c->h_kx2[i] + c->h_ky2[j]));
            if (lap) lap[k] = l;
            if (lapi) lapi[k] = (i == 0 && j == 0) ? 1.0f : l;
            if (mask) {
                const int ii = i < nx - i ? i : nx - i;
                mask[k] = ((double)ii * ii + (double)j * j >= c->gws) ? 0.0f : 1.0f;
            }
        }
    return FB_OK;
}

// --------------------------------------------------------------------------------------------
// buffers
// --------------------------------------------------------------------------------------------
extern "C" int fb_malloc(void **p, size_t bytes)
{
    if (!p) return fail(FB_EINVAL, "fb_malloc: NULL");
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) return fail(FB_ENOMEM, "hipMalloc: out of memory");
    HIPCHK(e);
    return FB_OK;
}
extern "C" int fb_free(void *p) { if (p) HIPCHK(hipFree(p)); return FB_OK; }
extern "C" int fb_memcpy_h2d(fb_ctx *c, void *d, const void *h, size_t n)
{
    if (!c || !d || !h) return fail(FB_EINVAL, "fb_memcpy_h2d: NULL");
    HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return FB_OK;
}
extern "C" int fb_memcpy_d2h(fb_ctx *c, void *h, const void *d, size_t n)
{
    if (!c || !d || !h) return fail(FB_EINVAL, "fb_memcpy_d2h: NULL");
    HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return FB_OK;
}
extern "C" int fb_memset0(fb_ctx *c, void *d, size_t n)
{
    if (!c || !d) return fail(FB_EINVAL, "fb_memset0: NULL");
    HIPCHK(hipMemsetAsync(d, 0, n, c->stream)); return FB_OK;
}

// ---- asynchronous record path: pinned host memory, streams, events (opaque void* handles) ----
extern "C" int fb_malloc_host(void **p, size_t bytes)
{
    if (!p) return fail(FB_EINVAL, "fb_malloc_host: NULL");
    hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) return fail(FB_ENOMEM, "hipHostMalloc: out of memory");
    HIPCHK(e);
    return FB_OK;
}
extern "C" int fb_free_host(void *p) { if (p) HIPCHK(hipHostFree(p)); return FB_OK; }
extern "C" int fb_stream_create(void **stream)
{
    if (!stream) return fail(FB_EINVAL, "fb_stream_create: NULL");
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void *)s;
    return FB_OK;
}
extern "C" int fb_stream_destroy(void *stream) { if (stream) HIPCHK(hipStreamDestroy((hipStream_t)stream)); return FB_OK; }
extern "C" int fb_stream_synchronize(void *stream) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return FB_OK; }
extern "C" int fb_event_create(void **ev)
{
    if (!ev) return fail(FB_EINVAL, "fb_event_create: NULL");
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *ev = (void *)e;
    return FB_OK;
}
extern "C" int fb_event_create_timing(void **ev)
{
    if (!ev) return fail(FB_EINVAL, "fb_event_create_timing: NULL");
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    *ev = (void *)e;
    return FB_OK;
}
extern "C" int fb_event_elapsed_ms(void *start, void *stop, float *ms)
{
    if (!start || !stop || !ms) return fail(FB_EINVAL, "fb_event_elapsed_ms: NULL");
    HIPCHK(hipEventSynchronize((hipEvent_t)stop));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return FB_OK;
}
extern "C" int fb_event_destroy(void *ev) { if (ev) HIPCHK(hipEventDestroy((hipEvent_t)ev)); return FB_OK; }
extern "C" int fb_event_record(void *ev, void *stream) { if (!ev) return fail(FB_EINVAL, "event NULL"); HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream)); return FB_OK; }
extern "C" int fb_stream_wait_event(void *stream, void *ev) { if (!ev) return fail(FB_EINVAL, "event NULL"); HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0)); return FB_OK; }
extern "C" int fb_event_synchronize(void *ev) { if (!ev) return fail(FB_EINVAL, "event NULL"); HIPCHK(hipEventSynchronize((hipEvent_t)ev)); return FB_OK; }
extern "C" int fb_memcpy_d2h_async(void *stream, void *h_dst, const void *d_src, size_t bytes)
{
    if (!h_dst || !d_src) return fail(FB_EINVAL, "fb_memcpy_d2h_async: NULL");
    HIPCHK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return FB_OK;
}
extern "C" int fb_memcpy_h2d_async(void *stream, void *d_dst, const void *h_src, size_t bytes)
{
    if (!d_dst || !h_src) return fail(FB_EINVAL, "fb_memcpy_h2d_async: NULL");
    HIPCHK(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return FB_OK;
}

// --------------------------------------------------------------------------------------------
// pointwise launches
// --------------------------------------------------------------------------------------------
static int grid_for(const fb_ctx *c, size_t n, int block = 256)
{
    size_t g = (n + block - 1) / block;
    if (g > (size_t)c->max_wg) g = c->max_wg;
    return (int)(g ? g : 1);
}

#define NEED_SINGLE(c) do { if ((c)->world != 1) return fail(FB_EINVAL, "natural-layout entry point on a slab context (world > 1)"); } while (0)

// one kernel launch on the context's stream, checked
template <typename K, typename... A> static int launch(const fb_ctx *c, K kern, dim3 grid, dim3 block, size_t lds, const A &...args)
{
    hipLaunchKernelGGL(kern, grid, block, lds, c->stream, args...);
    HIPCHK(hipGetLastError());
    return FB_OK;
}
// pointwise: n elements over 256-thread workgroups, capped by the context's grid
template <typename K, typename... A> static int launch_n(const fb_ctx *c, K kern, size_t n, const A &...args)
{
    return launch(c, kern, dim3(grid_for(c, n)), dim3(256), 0, args...);
}

// f(std::integral_constant<int, i>) for the run-time i in [0, N) (anything else: 0): a kernel's compile-time stage or mode count
template <int N, class F> static int dispatch(int i, F &&f)
{
    if constexpr (N == 1) return f(std::integral_constant<int, 0>());
    else return i == N - 1 ? f(std::integral_constant<int, N - 1>()) : dispatch<N - 1>(i, f);
}

template <int OP> static int launch_op(fb_ctx *c, const float *in, float *out)
{
    if (!c || !in || !out) return fail(FB_EINVAL, "operator: NULL argument");
    NEED_SINGLE(c);
    const size_t total = (size_t)c->nx * c->hy;
    return launch_n(c, k_spec_op<OP>, total, make_coef(c), (const cf *)in, (cf *)out, c->hy, total);
}
extern "C" int fb_gradx(fb_ctx *c, const float *i, float *o) { return launch_op<OP_GRADX>(c, i, o); }
extern "C" int fb_grady(fb_ctx *c, const float *i, float *o) { return launch_op<OP_GRADY>(c, i, o); }
extern "C" int fb_laplacian(fb_ctx *c, const float *i, float *o) { return launch_op<OP_LAP>(c, i, o); }
extern "C" int fb_invert_laplacian(fb_ctx *c, const float *i, float *o) { return launch_op<OP_INVLAP>(c, i, o); }
extern "C" int fb_dealiase(fb_ctx *c, const float *i, float *o) { return launch_op<OP_DEALIAS>(c, i, o); }

extern "C" int fb_backward_normalize(fb_ctx *c, float *d)
{
    if (!c || !d) return fail(FB_EINVAL, "fb_backward_normalize: NULL");
    const size_t n = (size_t)c->nx * c->ny;
    return launch_n(c, k_scale_real, n, d, (float)(int)n, 1, n);
}
extern "C" int fb_negate(fb_ctx *c, float *d)
{
    if (!c || !d) return fail(FB_EINVAL, "fb_negate: NULL");
    const size_t n = (size_t)c->nx * c->ny;
    return launch_n(c, k_scale_real, n, d, -1.0f, 0, n);
}
extern "C" int fb_jacobian(fb_ctx *c, const float *u, const float *v, const float *dx, const float *dy, const float *src, float *out)
{
    if (!c || !u || !v || !dx || !dy || !out) return fail(FB_EINVAL, "fb_jacobian: NULL");
    const size_t n = (size_t)c->nx * c->ny;
    return launch_n(c, k_jacobian, n, u, v, dx, dy, src, out, n);
}
extern "C" int fb_spec_axpy(fb_ctx *c, float *acc, const float *x, float a)
{
    if (!c || !acc || !x) return fail(FB_EINVAL, "fb_spec_axpy: NULL");
    const size_t n = 2 * (size_t)c->nx * c->hy;
    return launch_n(c, k_spec_axpy, n, (const float *)acc, x, a, acc, n);
}
extern "C" int fb_spec_evolve(fb_ctx *c, const float *base, const float *rk, float a, float *out)
{
    if (!c || !base || !rk || !out) return fail(FB_EINVAL, "fb_spec_evolve: NULL");
    const size_t n = 2 * (size_t)c->nx * c->hy;
    return launch_n(c, k_spec_axpy, n, base, rk, a, out, n);
}
extern "C" int fb_spec_rk4_combine(fb_ctx *c, const float *base, const float *k1, const float *k2, const float *k3,
                                   const float *k4, float dt, float *out)
{
    if (!c || !base || !k1 || !k2 || !k3 || !k4 || !out) return fail(FB_EINVAL, "fb_spec_rk4_combine: NULL");
    const size_t n = 2 * (size_t)c->nx * c->hy;
    return launch_n(c, k_rk4_combine, n, base, k1, k2, k3, k4, dt, out, n);
}

// --------------------------------------------------------------------------------------------
// FFT pass launchers
// --------------------------------------------------------------------------------------------
// hipFuncSetAttribute is per device: remember which (kernel, device) pairs are done
static int set_max_lds(const fb_ctx *c, const void *fn, size_t bytes)
{
    static std::mutex mu; static std::set<std::pair<const void *, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, c->dev})) return FB_OK;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.insert({fn, c->dev});
    return FB_OK;
}

// Launch of a kernel with more dynamic LDS than the default limit.  The attribute is set on the kernel's first launch on a
// device, and hipFuncSetAttribute must not run inside a stream capture: fb_model_step captures a step only after an eager one
// (its warm-up step) has launched every kernel of the step, and the pitch probe and the PRIME launch of k_col_full run eagerly too.
template <typename K, typename... A> static int launch_lds(const fb_ctx *c, K kern, int grid, int block, size_t lds, const A &...args)
{
    if (int rc = set_max_lds(c, (const void *)kern, lds)) return rc;
    return launch(c, kern, dim3(grid), dim3(block), lds, args...);
}

template <int N, int MODE> static int launch_row_t(fb_ctx *c, const RowArgs &a)
{
    using C = RowCfg<N>;
    constexpr int ppw = (C::PAIR2 && MODE == ROW_FUSED) ? C::G / 2 : C::G;      // row pairs per workgroup (fb_kernels.h, RowCfg)
    // persistent-style grid: a few workgroups per CU, each loops over row pairs
    const int grid = std::min((a.nx / 2 + ppw - 1) / ppw, c->max_wg / 2);
    return launch_lds(c, c->world > 1 ? k_row<N, MODE, true> : k_row<N, MODE, false>, grid, C::THREADS, C::LDS_BYTES, a);
}

template <int M, int MODE> static int launch_row3_t(fb_ctx *c, const RowArgs &a)
{
    using C = Row3Cfg<M>;
    constexpr int ppw = (C::TWO && MODE == ROW_FUSED) ? 1 : C::GP;     // row pairs per workgroup (fb_row3.h)
    const int grid = std::min((a.nx / 2 + ppw - 1) / ppw, c->max_wg);
    return launch_lds(c, c->world > 1 ? k_row3<M, MODE, true> : k_row3<M, MODE, false>, grid, C::THREADS, C::LDS_BYTES, a, (const cf *)c->d_tw_row3);
}

// k: the fused row kernel (ROW_FUSED only; the FWD / INV passes run the generic kernel for ny)
template <int MODE> static int launch_row(fb_ctx *c, RowArgs a, RowKernel k = RK_GENERIC)
{
    if (a.nx <= 0) return FB_OK;
    const bool slab = c->world > 1;
    if (MODE == ROW_FUSED) switch (k) {
    case RK_ROWQ:
        // one workgroup per row, four resident per CU: measured 0.076-0.078 ms per launch at 4096^2 against 0.081-0.084 with a persistent
        // grid of 1024 looping over rows (the dispatcher's refill keeps the four contexts of a CU out of step; the prologue is cheap)
        return launch_lds(c, slab ? k_rowq<true, false> : a.prescaled ? k_rowq<false, true> : k_rowq<false, false>, a.nx, 256, RowQ::LDS_BYTES,
                          a, (const float4 *)c->d_tw_2048);
    case RK_ROW8:                                          // two resident workgroups per CU, each loops over row pairs
        if (a.nx < 2) break;
        return launch_lds(c, slab ? k_row8<true> : k_row8<false>, std::min(a.nx / 2, c->max_wg / 4), 512, Row8::LDS_BYTES, a, (const cf *)c->d_tw_row3);
    case RK_ROWH_8192:                                     // resident workgroups: two per CU at ny = 8192, one at 16384; each loops over rows
        return launch_lds(c, slab ? k_rowh<1, true> : k_rowh<1, false>, std::min(a.nx, c->max_wg / 4), 512, RowH<1>::LDS_BYTES,
                          a, (const cf *)c->d_tw_4096, (const cf *)c->d_tw_row3);
    case RK_ROWH_16384:
        return launch_lds(c, slab ? k_rowh<2, true> : k_rowh<2, false>, std::min(a.nx, c->max_wg / 8), 512, RowH<2>::LDS_BYTES,
                          a, (const cf *)c->d_tw_4096, (const cf *)c->d_tw_row3);
    case RK_ROWH2:                                         // one 1024-thread workgroup per CU, each loops over x2 and produces the rows x2, x2 + 4096
        a.nx = 4096; a.sub_rows = 4096; a.tw_x = c->d_tw_big;
        return launch_lds(c, k_rowh2, std::min(a.nx, c->max_wg / 8), 1024, RowH2::LDS_BYTES, a, (const cf *)c->d_tw_4096, (const cf *)c->d_tw_row3);
    case RK_GENERIC: break;
    }
    switch (c->ny) {
    case 192: return launch_row3_t<64, MODE>(c, a);
    case 384: return launch_row3_t<128, MODE>(c, a);
    case 768: return launch_row3_t<256, MODE>(c, a);
    case 1536: return launch_row3_t<512, MODE>(c, a);
    case 3072: return launch_row3_t<1024, MODE>(c, a);
    case 64: return launch_row_t<64, MODE>(c, a);
    case 128: return launch_row_t<128, MODE>(c, a);
    case 256: return launch_row_t<256, MODE>(c, a);
    case 512: return launch_row_t<512, MODE>(c, a);
    case 1024: return launch_row_t<1024, MODE>(c, a);
    case 2048: return launch_row_t<2048, MODE>(c, a);
    case 4096: return launch_row_t<4096, MODE>(c, a);
    case 8192: return launch_row_t<8192, MODE>(c, a);
    case 16384: return launch_row_t<16384, MODE>(c, a);
    }
    return fail(FB_EUNSUPPORTED, "row pass: unsupported ny");
}

static int col_grid(const fb_ctx *c, long ntiles)
{
    long g = (ntiles + 3) / 4;
    if (g > c->max_wg) g = c->max_wg;
    return (int)(g ? g : 1);
}

// natural rows (one block) or, for the 4-field exchange buffer of a slab model, [dst][field][XL][ncols]
static RowMap rowmap_natural() { RowMap r; r.xl_shift = 31; r.xl_mask = 0x7fffffff; r.dstride = 0; r.xl = 0; return r; }
static int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }
static RowMap rowmap_w4(const fb_ctx *c, const ColGroup &G)
{
    if (c->world == 1) return rowmap_natural();
    RowMap r; r.xl_shift = ilog2(c->XL); r.xl_mask = c->XL - 1; r.dstride = 4L * c->XL * G.ncols;
    r.xl = is_pow2(c->XL) ? 0 : c->XL;
    return r;
}
static size_t grp_elems(const fb_ctx *c, const ColGroup &G) { return (size_t)c->nx * G.ncols; }
static long w4_fstride(const fb_ctx *c, const ColGroup &G) { return c->world == 1 ? (long)grp_elems(c, G) : (long)c->XL * G.ncols; }

template <int DIR> static int launch_col_strided(fb_ctx *c, const ColGroup &G, cf *data, int nfields, long fstride, RowMap rm = rowmap_natural(),
                                                 int ct0 = 0, int nct = -1)
{
    if (nct < 0) nct = G.ncols / 16 - ct0;
    if (nct <= 0) return FB_OK;
    ColArgs a; a.data = data; a.fstride = fstride; a.rm = rm; a.ct0 = ct0; a.nct = nct; a.nfields = nfields; a.P = G.ncols; a.N1 = c->N1; a.N2 = c->N2;
    a.tw_n = c->d_tw_n1; a.tw_big = c->d_tw_big;
    const long ntiles = (long)nfields * c->N2 * nct;
    const dim3 g(col_grid(c, ntiles)), b(256);
    switch (c->N1) {
    case 24: hipLaunchKernelGGL((k_col_strided<24, DIR>), g, b, 0, c->stream, a); break;
    case 8: hipLaunchKernelGGL((k_col_strided<8, DIR>), g, b, 0, c->stream, a); break;
    case 16: hipLaunchKernelGGL((k_col_strided<16, DIR>), g, b, 0, c->stream, a); break;
    case 32: hipLaunchKernelGGL((k_col_strided<32, DIR>), g, b, 0, c->stream, a); break;
    case 64: hipLaunchKernelGGL((k_col_strided<64, DIR>), g, b, 0, c->stream, a); break;
    case 128: hipLaunchKernelGGL((k_col_strided<128, DIR>), g, b, 0, c->stream, a); break;
    default: return fail(FB_EUNSUPPORTED, "col strided: N1");
    }
    HIPCHK(hipGetLastError());
    return FB_OK;
}

template <int DIR> static int launch_col_block(fb_ctx *c, const ColGroup &G, cf *data, int nfields, long fstride)
{
    if (G.ncols == 0) return FB_OK;
    ColArgs a; a.data = data; a.fstride = fstride; a.rm = rowmap_natural(); a.ct0 = 0; a.nct = G.ncols / 16; a.nfields = nfields; a.P = G.ncols; a.N1 = c->N1; a.N2 = c->N2;
    a.tw_n = c->d_tw_n2; a.tw_big = c->d_tw_big;
    const long ntiles = (long)nfields * c->N1 * (G.ncols / 16);
    const dim3 g(col_grid(c, ntiles)), b(256);
    switch (c->N2) {
    case 8: hipLaunchKernelGGL((k_col_block<8, DIR>), g, b, 0, c->stream, a); break;
    case 16: hipLaunchKernelGGL((k_col_block<16, DIR>), g, b, 0, c->stream, a); break;
    case 32: hipLaunchKernelGGL((k_col_block<32, DIR>), g, b, 0, c->stream, a); break;
    case 64: hipLaunchKernelGGL((k_col_block<64, DIR>), g, b, 0, c->stream, a); break;
    case 128: hipLaunchKernelGGL((k_col_block<128, DIR>), g, b, 0, c->stream, a); break;
    default: return fail(FB_EUNSUPPORTED, "col block: N2");
    }
    HIPCHK(hipGetLastError());
    return FB_OK;
}

static int launch_col_mid(fb_ctx *c, const MidArgs &a0)
{
    if (a0.nct <= 0) return FB_OK;
    MidArgs a = a0;
    const long ntiles = (long)c->N1 * a.nct;
    // small launches of small tiles (grids up to 1024^2): one tile per workgroup, the derivative fields spread over its four waves
    // (fb_kernels.h, MidArgs::split): 256^2 9072 -> 9808 steps/s, 1024^2 6084 -> 6382.  Not for 64-row tiles (the slabs of a 4096^2
    // multi-GPU rank: 0.336 -> 0.383 ms per step) nor for 2048^2 (0.026 -> 0.038 ms per launch)
    a.split = (ntiles <= 2048 && c->N2 <= 32) ? 1 : 0;
    const dim3 g(a.split ? (unsigned)(ntiles < c->max_wg ? ntiles : c->max_wg) : (unsigned)col_grid(c, ntiles)), b(256);
    switch (c->N2) {
    case 8: hipLaunchKernelGGL((k_col_mid<8>), g, b, 0, c->stream, a); break;
    case 16: hipLaunchKernelGGL((k_col_mid<16>), g, b, 0, c->stream, a); break;
    case 32: hipLaunchKernelGGL((k_col_mid<32>), g, b, 0, c->stream, a); break;
    case 64: hipLaunchKernelGGL((k_col_mid<64>), g, b, 0, c->stream, a); break;
    case 128: hipLaunchKernelGGL((k_col_mid<128>), g, b, 0, c->stream, a); break;
    default: return fail(FB_EUNSUPPORTED, "col mid: N2");
    }
    HIPCHK(hipGetLastError());
    return FB_OK;
}

static size_t priv_elems(const fb_ctx *c) { return grp_elems(c, c->grp[0]); }   // one GPU: the one group

// tiles of every group that hold at least one column inside the dealiasing circle (the rest is frozen forever)
static void finish_groups(fb_ctx *c)
{
    for (int g = 0; g < c->ngroups; ++g) {
        ColGroup &G = c->grp[g];
        const int act = (c->jmax - G.ky0 + 15) / 16;
        G.nct_active = act < 0 ? 0 : (act > G.ncols / 16 ? G.ncols / 16 : act);
        if (c->no_column_skip) G.nct_active = G.ncols / 16;
    }
}

// The x pass of a model on this context that is stepped by fb_model_step (a model driven phase by phase, fb_slab_*, always
// takes XP_COLS).  The single-pass x transform (fb_col_full.h) applies on one GPU with a frozen Nyquist column and whole 8-column
// tiles, at nx = 4096 (0.177 ms per stage against 0.21 ms for the three column kernels) and at nx = ny = 8192 with k_rowh
// (FB_NO_ROWH=1 switches it off there too).  FB_FULL_PASS=0 keeps the three column kernels.
static XPass choose_xpass(const fb_ctx *c)
{
    if (c->world != 1 || !c->nyq_frozen || ((c->ny / 2) % 8) != 0 || c->full_pass_off) return XP_COLS;
    if (c->nx == 4096) return XP_FULL1;
    if (c->nx == 8192 && c->row == RK_ROWH_8192) return XP_FULL2;
    return XP_COLS;
}

// k_col_full<a.stage, a.nsub, KEEP>: stage 0..3 forward x transform of the tendency + RK update + derivatives, 4 PRIME (fb_col_full.h)
static int launch_full(const fb_ctx *c, const FullArgs &a)
{
    using K = void (*)(FullArgs);
#define CF_ROW(N, KP) {k_col_full<0, N, KP>, k_col_full<1, N, KP>, k_col_full<2, N, KP>, k_col_full<3, N, KP>, k_col_full<4, N, KP>}
    static const K ks[2][2][5] = {{CF_ROW(1, 0), CF_ROW(2, 0)},                      // FB_FULL_KEEP=0: no part of the state kept
                                  {CF_ROW(1, CF_KEEP1), CF_ROW(2, CF_KEEP2)}};       // the default
#undef CF_ROW
    return launch_lds(c, ks[c->full_keep_off ? 0 : 1][a.nsub - 1][a.stage], a.nsub * (a.stage == 4 ? a.ntiles + 1 : a.ntiles), CF_THREADS, CF_LDS_BYTES, a);
}

// The strided x sub-pass reads rows N2*P*8 bytes apart; how well that stride spreads over the HBM channels
// depends on the pitch in a way that is specific to the memory controller's address hash (measured on MI355X,
// backward strided pass of four fields: 4096^2: P = 2064 0.0955 ms, 2080 0.084 ms; 8192^2: P = 4112 0.393 ms,
// 4128 0.586 ms).  So on large single-GPU grids the pitch is chosen by timing that pass for a few candidates.
// Results do not depend on the pitch (pad columns are zero and every pass is linear).
static int autotune_pitch(fb_ctx *c)
{
    finish_groups(c);
    if (c->world != 1 || c->no_pitch_tune) return FB_OK;
    if ((size_t)c->nx * c->P * sizeof(cf) < ((size_t)32 << 20)) return FB_OK;      // cache-resident grids: nothing to gain
    const XPass xp = choose_xpass(c);
    const int P0 = c->P, NC = xp != XP_COLS ? 7 : 4;                               // create_impl leaves room for P0 + 96
    constexpr int PITCH_HEADROOM = 96, RULE_EXTRA = 32;                            // the coefficient tables hold P0 + PITCH_HEADROOM columns
    static_assert(RULE_EXTRA <= PITCH_HEADROOM && 16 * (7 - 1) <= PITCH_HEADROOM, "pitch candidates must fit the table head-room of create_impl");
    if ((int)c->h_gy.size() < P0 + PITCH_HEADROOM) return fail(FB_EINVAL, "autotune_pitch: coefficient tables shorter than the pitch candidates");
    // The fixed rule below was measured on MI355X (gfx950): the pitch's effect comes from that part's memory-controller address
    // hash.  On any other device the interleaved probe decides instead.
    hipDeviceProp_t prop;
    int dev = 0;
    const bool is_gfx950 = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    if (xp != XP_COLS && is_gfx950 && !c->pitch_tune) {
        // single-pass x transform: a fixed rule.  tools/pitch_scan.sh on three boxes: round16(ny/2 + 1) is the slowest pitch at
        // 4096^2 (k_col_full 0.1525-0.1556 ms against 0.148-0.152 for every other candidate) and, with + 16, at 8192^2 (0.75 / 0.79 ms
        // against 0.65-0.69 for + 32, + 64, + 96 and 0.69-0.72 for + 48, + 80).  The probe below (FB_PITCH_TUNE=1) sees the same
        // ordering on average but not reliably in one process: its buffers land on other physical pages than the model's, which
        // moves a candidate by up to 5 % at 8192^2, more than what separates the good pitches.
        c->P = c->KA = c->katot = c->grp[0].ncols = P0 + RULE_EXTRA;
        finish_groups(c);
        return FB_OK;
    }
    const size_t maxe = (size_t)c->nx * (P0 + 16 * (NC - 1));
    // the probe is the pitch-sensitive kernel of the path the model will take: the backward strided sub-pass of one field, or
    // a stage-1 launch of k_col_full (tendency in, three state arrays, 64-byte row segments of four derivative fields out, rows
    // P*8 bytes apart) on zeroed buffers.  tools/pitch_scan.sh: the step time follows this probe; PRIME launches with two
    // repetitions per candidate (the first version) did not resolve the 2-4 % between pitches and often kept the worst one.
    const int nbuf = xp != XP_COLS ? 9 : 1;  // k_col_full: Tin, 4 x W4, Z0, Zc, Acc, Zout
    cf *buf = nullptr;
    if (hipMalloc((void **)&buf, maxe * nbuf * sizeof(cf)) != hipSuccess) { hipGetLastError(); return FB_OK; }
    hipMemsetAsync(buf, 0, maxe * nbuf * sizeof(cf), c->stream);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    auto probe = [&](int P) -> int {
        ColGroup G = c->grp[0]; G.ncols = P;
        if (xp == XP_COLS) return launch_col_strided<+1>(c, G, buf, 1, 0);
        FullArgs a; memset(&a, 0, sizeof(a));
        a.Tin = buf; a.W4 = buf + maxe; a.Zbase = buf + 5 * maxe; a.Zcur = buf + 6 * maxe; a.Acc = buf + 7 * maxe; a.Zout = buf + 8 * maxe;
        a.fstride = (long)c->nx * P; a.P = P; a.ntiles = (c->ny / 2) / 8;
        a.ntiles_run = a.ntiles; a.nsub = xp; a.stage = 1; a.nu = 0.f; a.dt = 0.f; a.coef = make_coef(c); a.tw256 = c->d_tw_256;
        a.tw4096 = xp == XP_FULL1 ? c->d_tw_big : c->d_tw_4096; a.sub_rows = 4096;
        return launch_full(c, a);
    };
    const bool verbose = c->tune_verbose;
    // the device needs ~25 ms of this load to reach full speed: run the probe that long before timing it
    hipEventRecord(e0, c->stream);
    for (int it = 0; it < 400; ++it) {
        if (probe(P0) != FB_OK) break;
        if ((it & 7) == 7) {
            hipEventRecord(e1, c->stream); hipEventSynchronize(e1);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms > 30.f) break;
        }
    }
    float tbest[8]; for (int k = 0; k < NC; ++k) tbest[k] = 1e30f;
    for (int rep = 0; rep < 6; ++rep)            // candidates interleaved, so that a drift of the clock hits all of them alike
        for (int k = 0; k < NC; ++k) {
            hipEventRecord(e0, c->stream);
            const int rc = probe(P0 + 16 * k);
            hipEventRecord(e1, c->stream);
            hipEventSynchronize(e1);
            float ms = 0.f;
            if (rc == FB_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < tbest[k]) tbest[k] = ms;
        }
    float best = 1e30f; int bestP = P0;
    for (int k = 0; k < NC; ++k) {
        if (verbose) fprintf(stderr, "fftbaro: pitch probe P=%d %.4f ms\n", P0 + 16 * k, tbest[k]);
        if (tbest[k] < best * 0.99f) { best = tbest[k]; bestP = P0 + 16 * k; }     // a larger pitch must win by 1 % to be taken
    }
    if (verbose) fprintf(stderr, "fftbaro: pitch %d -> %d\n", P0, bestP);
    c->P = c->KA = c->katot = c->grp[0].ncols = bestP;
    finish_groups(c);
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(buf);
    hipGetLastError();
    return FB_OK;
}

static int ensure_scratch(fb_ctx *c)
{
    if (!c->d_scratch) {
        hipError_t e = hipMalloc((void **)&c->d_scratch, priv_elems(c) * sizeof(cf));
        if (e != hipSuccess) return fail(FB_ENOMEM, "scratch allocation failed");
    }
    return FB_OK;
}

// ---- row-pass views (fb_kernels.h: RowView) ----
static unsigned magic_div(int d) { return d > 0 ? (unsigned)((1ull << 32) / (unsigned)d) + 1u : 0u; }
// one GPU: nfields arrays of pitch P, fstride apart
static RowView view_single(const fb_ctx *c, const cf *base, long fstride)
{
    RowView v; memset(&v, 0, sizeof(v));
    v.a = v.b = v.f = base; v.fstrA = v.fstrB = v.fstrF = fstride; v.ka = v.ka0 = c->P; v.kb = 0; v.kf = 16; v.katot = 0x7fffffff;
    return v;
}
// multi-GPU exchange buffers, one per column group: [peer][nfields][XL][ncols_g]; bufs[g] = group g's (fb_ctx::grp order)
static RowView view_slab(const fb_ctx *c, const cf *const *bufs, int nfields)
{
    RowView v; memset(&v, 0, sizeof(v));
    v.a = bufs[0]; v.b = c->nact > 1 ? bufs[1] : bufs[0]; v.f = c->KF > 0 ? bufs[c->nact] : bufs[0];
    v.ka = c->KA; v.ka0 = c->grp[0].ncols; v.kb = c->nact > 1 ? c->grp[1].ncols : 0; v.kf = c->KF > 0 ? c->KF : 16;
    v.katot = c->katot;
    v.fstrA = (long)c->XL * v.ka0; v.fstrB = (long)c->XL * v.kb; v.fstrF = (long)c->XL * v.kf;
    v.sstrA = (long)nfields * v.fstrA; v.sstrB = (long)nfields * v.fstrB; v.sstrF = (long)nfields * v.fstrF;
    v.magA = magic_div(v.ka); v.magF = magic_div(v.kf);
    return v;
}
// the row-side view of one kind of exchange buffer of the model (which: 0 w4_recv, 1 t_send)
static RowArgs row_args_base(const fb_ctx *c)
{
    RowArgs a; memset(&a, 0, sizeof(a));
    a.x0 = 0; a.nx = c->XL; a.tw_bwd = c->d_tw_row_bwd; a.tw_fwd = c->d_tw_row_fwd; a.t_frozen = 1;
    return a;
}

// ---- the two transform passes over several fields (one GPU, or a slab of one rank: column group 0, no exchange) ----
// nf spectra in the private layout at z + f * fstride (destroyed) -> nf real fields [nx][ny] at out + f * nx * ny, each times g, field
// `neg` times -g (-1: none): the backward x pass over all of them in one launch each, then one ROW_INV row pass per field.
// (nf, fstride) go to the column launches as they are: (1, 0) for a single field, (nf, nx * P) for fields one after the other.
static int spectra_to_real(fb_ctx *c, cf *z, int nf, long fstride, float *out, float g, int neg)
{
    const ColGroup &G = c->grp[0];
    const size_t nr = (size_t)c->nx * c->ny;
    int rc;
    if ((rc = launch_col_block<+1>(c, G, z, nf, fstride)) || (rc = launch_col_strided<+1>(c, G, z, nf, fstride))) return rc;
    for (int f = 0; f < nf; ++f) {
        RowArgs a = row_args_base(c);
        a.M = view_single(c, z + f * fstride, fstride); a.scale = f == neg ? -g : g; a.rout = out + f * nr;
        if ((rc = launch_row<ROW_INV>(c, a))) return rc;
    }
    return FB_OK;
}

// nf real fields [nx][ny] at real + f * nx * ny -> nf spectra in the private layout at z + f * fstride: one ROW_FWD row pass per field,
// then the forward x pass over all of them in one launch each.  The row pass writes the live columns only: the caller has zeroed
// the pad columns of z (a memset of the whole destination, wherever it has always stood).
static int real_to_spectra(fb_ctx *c, const float *real, cf *z, int nf, long fstride)
{
    const ColGroup &G = c->grp[0];
    const size_t nr = (size_t)c->nx * c->ny;
    int rc;
    for (int f = 0; f < nf; ++f) {
        RowArgs a = row_args_base(c);
        a.rin = real + f * nr; a.T = view_single(c, z + f * fstride, 0);
        if ((rc = launch_row<ROW_FWD>(c, a))) return rc;
    }
    if ((rc = launch_col_strided<-1>(c, G, z, nf, fstride))) return rc;
    return launch_col_block<-1>(c, G, z, nf, fstride);
}

// real [nx][ny] -> private spectral layout (dst: nx*P complex, pad columns must be zero-initialised)      [one GPU]
static int r2c_private(fb_ctx *c, const float *d_real, cf *dst) { return real_to_spectra(c, d_real, dst, 1, 0); }

// private spectral layout (work: destroyed) -> real [nx][ny] * scale                                       [one GPU]
static int c2r_private(fb_ctx *c, cf *work, float *d_real, float scale) { return spectra_to_real(c, work, 1, 0, d_real, scale, -1); }

// 3-pass row layout <-> the tile-major layout of the state arrays (out-of-place)
static bool state_tm(const fb_ctx *c) { return c->N2 >= 32; }
static int state_convert(fb_ctx *c, const ColGroup &G, const cf *in, cf *out, bool to_tm)
{
    if (G.ncols == 0) return FB_OK;
    if (!state_tm(c)) { HIPCHK(hipMemcpyAsync(out, in, grp_elems(c, G) * sizeof(cf), hipMemcpyDeviceToDevice, c->stream)); return FB_OK; }
    const size_t total = grp_elems(c, G);
    return launch_n(c, to_tm ? k_state_relayout<true> : k_state_relayout<false>, total, in, out, c->nx, G.ncols, c->N2);
}

static int relayout(fb_ctx *c, const cf *in, cf *out, bool to_private)
{
    const size_t total = priv_elems(c);
    return launch_n(c, to_private ? k_spec_relayout<true> : k_spec_relayout<false>, total, in, out, c->nx, c->hy, c->P, c->N1, c->N2);
}

extern "C" int fb_r2c(fb_ctx *c, const float *d_in, float *d_out)
{
    if (!c || !d_in || !d_out) return fail(FB_EINVAL, "fb_r2c: NULL");
    NEED_SINGLE(c);
    int rc;
    if ((rc = ensure_scratch(c))) return rc;
    HIPCHK(hipMemsetAsync(c->d_scratch, 0, priv_elems(c) * sizeof(cf), c->stream));
    if ((rc = r2c_private(c, d_in, c->d_scratch))) return rc;
    return relayout(c, c->d_scratch, (cf *)d_out, false);
}

extern "C" int fb_c2r(fb_ctx *c, const float *d_in, float *d_out, int normalize)
{
    if (!c || !d_in || !d_out) return fail(FB_EINVAL, "fb_c2r: NULL");
    NEED_SINGLE(c);
    int rc;
    if ((rc = ensure_scratch(c))) return rc;
    if ((rc = relayout(c, (const cf *)d_in, c->d_scratch, true))) return rc;
    const float scale = normalize ? 1.0f / (float)((size_t)c->nx * c->ny) : 1.0f;
    return c2r_private(c, c->d_scratch, d_out, scale);
}

// --------------------------------------------------------------------------------------------
// fused RK4 model
// --------------------------------------------------------------------------------------------
// per column group: state arrays in the private layouts (nx*ncols complex each) and the exchange buffers.
// One GPU: w4_recv == w4_send (4 fields) and t_recv == t_send (no exchange).  Multi-GPU (engine-owned):
//   w4_send [dst][4][XL][ncols]  destination-blocked, written by the column kernels     -> all-to-all ->
//   w4_recv [src][4][XL][ncols]  block s = rank s's ky slab of this rank's rows, read by the row pass
//   t_send  [dst][XL][ncols]     written by the row pass                                -> all-to-all ->
//   t_recv  [nx][ncols]          block s = rows of rank s, read by the column kernels
struct GroupBufs { cf *ZA, *ZB, *ACC, *w4_send, *w4_recv, *t_send, *t_recv; };

// a spectral field stepped beside the vorticity (fb_beside.h: the tracer, a perturbation of the tangent set, an adjoint variable): per
// column group in the 3-pass layout [nx][ncols] the base, and for the groups of active columns the stage state and the RK accumulator;
// NULL while the field is not set.  Never in the record workspace: a record taken between two steps overwrites that.
struct Beside { cf *c0[3], *c1[3], *acc[3]; };
// n such fields on the one trajectory, advanced one after the other: what the tangent subspace and the adjoint subspace both are
struct BesideSet { static constexpr int MAX = 32; Beside v[MAX]; int n; };
static_assert(FB_TANGENTS_MAX == BesideSet::MAX && FB_ADJOINTS_MAX == BesideSet::MAX, "BesideSet holds either public bound, and the refusals' text names it");

struct fb_model {
    fb_ctx *c;
    float nu, dt;
    GroupBufs gb[3];
    bool phase_flow;                 // driven phase by phase (fb_slab_*): always the three-kernel column path
    XPass xpass;                     // XP_FULL1/2 (fb_col_full.h): ZA/ZB/ACC then use k_col_full's private layout
    bool prescale;                   // k_col_full writes the derivative fields times 1/GRIDS and k_rowq<false, true> does not normalise (4096^2 on one GPU)
    // hipGraph replay of one RK4 step (launch-bound small grids): captured lazily on a non-null stream,
    // dropped whenever something baked into the kernel arguments changes (source pointer, stream) and by whatever changes the
    // step's launches: a tracer, particles or a tangent that comes or goes (beside_begin, fb_beside.h)
    bool use_graph, warmed;
    hipGraphExec_t graph_exec;
    const float *graph_src; hipStream_t graph_stream;
    float *src;                      // vort_src (this rank's rows) or NULL (== zeros)
    int *src_nz;                     // per row of src: 1 = holds a non-zero value (k_src_row_flags)
    // the record workspace (fb_record.h; lazy, never read by the step): per column group, a record's one or three fields
    // [3][nx][ncols] in rec_work through the x pass; multi-GPU: exchanged into rec_send (one field) or regrouped into rec_send as
    // [dst][3][XL][ncols] and exchanged back into rec_work as [src][3][XL][ncols] (three), the layout of view_slab
    cf *rec_work[3], *rec_send[3];
    // the eddy-diffusivity record adds zeta and |grad zeta|^2 ([2][XL][ny], for a caller who passes no outputs of their own) and
    // the reduction buffers (grown to the largest request)
    float *keff_fields;
    void *keff_red; size_t keff_red_cap;
    // the azimuthal-mean record adds zeta and u (or psi) ([2][XL][ny]; v goes to the record workspace) and its reduction buffer (grown
    // to the largest request)
    float *azim_fields;
    void *azim_red; size_t azim_red_cap;
    // the vortex census (fb_census.h; host side: fb_record.h, record_census): the labels and the cells per root, then the dense ids
    // ([nx][ny] int32 each), and the scan's per-tile partials (nx ny / 1024 int2); allocated at the first census, then kept.  Not the
    // record workspace: a census of the caller's own field between two steps must not move what a captured step reads
    int *cs_label, *cs_ids;
    int2 *cs_part;
    // the pressure record's reference-point value: [world] floats to send, [world] received (fb_record.h, record_pres)
    float *pres_ref;
    // the spectra record: fields the record workspace holds where this kind has grown it (0: the three of the other kinds), and the
    // shells' partial sums [world][nshells][6] to send and received (fb_record.h, record_spectra)
    unsigned char rec_work_nf[3], rec_send_nf[3];
    void *spec_red;
    // 0: derivative fields stale; 1: w4_send holds the derivatives with the backward x pass finished on the frozen
    // tiles only (the backward strided pass on the active tiles comes next); 2: finished on every tile (ready for the row pass)
    int primed;
    // the passive tracer (fb_tracer.h; host side in fb_beside.h) and its diffusivity
    Beside tr;
    float kappa;
    bool tracer;                     // a tracer is set
    // the Lagrangian particles (fb_particles.h; host side in fb_beside_particles.h): six float64 arrays of pt_n (base, stage position, RK
    // accumulator, x then y of each) and the stage velocity u, v as two real fields [2][nx][ny]; NULL and 0 without particles
    double *pt; int pt_n;
    float *pt_uv;
    // the particles' deformation gradient (fb_model_set_particle_deformation): twelve float64 arrays of pt_n (base, stage value, RK
    // accumulator of F11, F12, F21, F22 each), NULL while it is off; steps: the model's steps so far, pd_steps0: at the last reset
    double *pd;
    long long steps, pd_steps0;
    // the tangent-linear model (fb_tangent.h; host side in fb_beside_tangent.h): tg.n perturbations on the one trajectory (a tangent subspace;
    // fb_model_set_tangent sets one), each allocated when it is set, and what they share, since they are advanced one after the other:
    // the first advect pass's tendency of a stage (groups of active columns) and the partial sums of an inner product (the norm is
    // one); NULL and tg.n == 0 without, and tg.n alone says whether a tangent is set
    BesideSet tg;
    cf *tg_j[3];
    double *tg_red;
    // the tangent replay's real fields (fb_replay.h; host side in fb_beside_adjoint.h): [4 + 5 C][nx][ny] for a set replayed in chunks of
    // C = min(tg.n, REPLAY_CHUNK) perturbations (the four base fields, 4 C of the perturbations, C products); allocated at the first
    // replay, sized for the count, freed with the tangent set; NULL before
    float *rp_real;
    // the basis tape of the covariant Lyapunov vectors (fb_clv.h; host side in fb_beside_tangent.h): per column group tt_depth slots of the tg.n
    // bases tg.v[k].c0[g], [tt_depth][tg.n] arrays of grp_elems each in c0's own layout, tt_fill slots of it pushed; NULL and 0 while
    // there is none.  Bases only: stage states and accumulators carry nothing between two steps.  The step never reads it
    cf *tt[3]; int tt_depth, tt_fill;
    // the adjoint model (fb_adjoint.h; host side in fb_beside_adjoint.h).  The tape: ad_depth steps x 4 stage states of the vorticity in the
    // 3-pass layout, masked modes merged in from the base, ad_fill steps of it recorded; NULL and 0 while nothing is recorded.  The
    // ad.n adjoint variables on the one tape (an adjoint subspace; fb_model_set_adjoint sets one), each lam (ad.v[k].c0) with the k-bar
    // (c1) and the accumulator (acc) of a backward step, and what they share: the real fields of the product pass, [5][nx][ny] for
    // the one, [4 + 5 C][nx][ny] for a set swept in chunks of C = min(ad.n, ADJOINT_CHUNK) variables (the four base fields, C mu~,
    // 4 C products), and for a set the C spectra of the chunk's mu~ (ad_spec); NULL and ad.n == 0 without, and ad.n alone says
    // whether an adjoint is set
    cf *ad_tape; int ad_depth, ad_fill;
    // ad_top: the slots from the oldest that hold recorded steps no later step has overwritten (>= ad_fill: a sweep pops without
    // erasing, fb_model_adjoint_rewind un-pops up to here, fb_model_tangent_replay reads up to here); 0 wherever ad_fill is reset
    int ad_top;
    // ad_on: the steps taken now stash their stage states (always while fb_model_adjoint_record's tape is on; under checkpointing only
    // while a segment is run again).  Adjoint checkpointing (fb_model_adjoint_checkpoint; host side in fb_beside_adjoint.h): the tape is one
    // segment of ck_every steps, ck_store holds room for ceil(ck_max / ck_every) states of column group 0 as the state arrays hold them
    // (ZA), ck_n of them taken, ck_live one more for the live state during a sweep.  The window: ck_done steps taken forward, ck_left
    // of them not yet swept (ad_fill of those are on the tape), ck_swept once a sweep has popped one, ck_replayed steps run again
    // since it began; ck_replay: the step under way is such a run, and advances the vorticity alone.  All 0 / NULL while it is off
    bool ad_on, ck_swept, ck_replay;
    int ck_every, ck_max, ck_n, ck_done, ck_left;
    long long ck_replayed;
    cf *ck_store, *ck_live;
    BesideSet ad;
    float *ad_real;
    cf *ad_spec;
    // the point observations (fb_obs.h; host side in fb_beside_adjoint.h): the fixed-point accumulator of a scatter (two 64-bit limbs for
    // each of the nx * ny cells, and its head), the real field that is observed from or scattered into, the partial sums of a misfit ([max_wg]
    // float64); each allocated at its first use, then kept
    unsigned long long *ob_acc;
    float *ob_real;
    double *ob_red;
    // the adjoint of the particle step (fb_lagrangian.h; host side in fb_beside_particles.h).  The particle tape: pt_depth steps x 4 stage
    // positions, float64 [pt_n][2] each, pt_fill steps of it recorded while the model stepped; NULL and 0 while it is off.  The
    // particle adjoint: eight float64 arrays of pt_n (Xb, the stage's p and q, the accumulator; x then y of each), and the two
    // fixed-point accumulators of a stage's deposit (2 x 2 limbs for each of the nx * ny cells, and the head); NULL while none is set.
    // Both go with the particles they belong to
    double *pt_tape; int pt_depth, pt_fill;
    double *pa;
    unsigned long long *pa_acc;
    // the split stage after every step (fb_forcing.h; host side in fb_beside_forcing.h): stochastic ring forcing, linear drag and
    // hyperviscosity.  fr: the kernels' arguments; fr_nring: the ring's modes over the full spectrum; fr_work: the vorticity in the
    // 3-pass layout where the state arrays are in another (NULL where the stage runs in place); fr_part: [max_wg][4] float64 partial
    // sums of the budget; fr_dev: the 64-bit forcing clock, then the four running totals (float64).  All allocated when the forcing is
    // set, so that a step allocates nothing and a captured step reads its clock from the device; NULL and fr_on false without
    bool fr_on;
    ForcingArgs fr;
    int fr_nring;
    cf *fr_work;
    double *fr_part;
    unsigned long long *fr_dev;
};

// one rank of the multi-GPU model (fb_slab_driver.h)
#include "fb_transport.h"
struct fb_slab {
    fb_ctx *c;
    fb_model *m;
    fb_transport tp;
    bool connected, owns_streams;
    hipStream_t comp, comm;
    hipEvent_t ev_f[4], ev_r[8], ev_w4, ev_t, ev_tg[2], ev_rows_done, ev_fwd_done, ev_misc[2];
    int nfg, nch;               // field groups of the derivative exchange (1, 2 or 4), row chunks of the tendency exchange (1..8)
    int ncg;                    // active column groups (fb_ctx::nact): 2 = the stage is pipelined by column groups, and nfg == 1
    int step_ops;               // exchange operations issued per RK stage (diagnostics)
};
#include "fb_entry.h"

static int model_create_impl(fb_model **out, fb_ctx *c, float nu, float dt, bool phase_flow)
{
    if (!out || !c) return fail(FB_EINVAL, "fb_model_create: NULL");
    *out = nullptr;
    fb_model *m = new fb_model();
    memset(m, 0, sizeof(*m));
    m->c = c; m->nu = nu; m->dt = dt; m->phase_flow = phase_flow;
    m->xpass = phase_flow ? XP_COLS : choose_xpass(c);
    m->prescale = m->xpass != XP_COLS && c->world == 1 && c->row == RK_ROWQ && !c->no_prescale;   // k_rowq: ny == 4096, so GRIDS = nx * ny is a power of two
    int rc = FB_OK;
    auto alloc0 = [&](cf **p, size_t elems) {              // zero-initialised device array (pad columns stay zero: every pass is linear)
        if (rc || elems == 0) return;
        if (hipMalloc((void **)p, elems * sizeof(cf)) != hipSuccess) { rc = fail(FB_ENOMEM, "model allocation failed"); return; }
        if (hipMemsetAsync(*p, 0, elems * sizeof(cf), c->stream) != hipSuccess) rc = fail(FB_EHIP, "hipMemsetAsync failed");
    };
    for (int g = 0; g < c->ngroups; ++g) {
        const size_t n = grp_elems(c, c->grp[g]);
        GroupBufs &B = m->gb[g];
        alloc0(&B.ZA, n);
        if (g < c->nact) { alloc0(&B.ZB, n); alloc0(&B.ACC, n); }     // the frozen group's state never changes: vort_c only
        alloc0(&B.w4_send, 4 * n); alloc0(&B.t_send, n);
        if (c->world > 1) { alloc0(&B.w4_recv, 4 * n); alloc0(&B.t_recv, n); }
        else { B.w4_recv = B.w4_send; B.t_recv = B.t_send; }
    }
    if (rc) { fb_model_destroy(m); return rc; }
    *out = m;
    return FB_OK;
}

extern "C" int fb_model_create(fb_model **out, fb_ctx *c, float nu, float dt)
{
    if (c && c->world != 1) return fail(FB_EINVAL, "fb_model_create on a slab context: use fb_slab_create");
    return model_create_impl(out, c, nu, dt, false);
}

// the fields stepped beside the vorticity (fb_beside.h and the headers it includes): what the step and the model's end know of them
static int beside_stage(fb_model *m, fb_slab *s, int stage);            // at the top of RK stage `stage` of fb_model_step and fb_slab_step
static void beside_step_done(fb_model *m);                              // after the step's fourth stage
static int forcing_stage(fb_model *m, fb_slab *s);                      // and after that: the split stage, where forcing is set (fb_beside_forcing.h)
static size_t forcing_bytes(const fb_model *m);                         // what fb_model_info counts for it
static void beside_free_all(fb_model *m);
static size_t adjoint_bytes(const fb_model *m);                         // what fb_model_info counts for the adjoint variables
static size_t adjoint_tape_bytes(const fb_model *m);                    // and for the tape, or the tape segment, the checkpoints and the live copy
static size_t replay_bytes(const fb_model *m);                          // and for the tangent replay's workspace
static int checkpoint_take(fb_model *m, int *nsteps);                   // run_steps under checkpointing, before every piece of a step call
static size_t lagrangian_bytes(const fb_model *m);                      // what fb_model_info counts for the particle tape and the particle adjoint

static void model_drop_graph(fb_model *m)
{
    if (m->graph_exec) { hipGraphExecDestroy(m->graph_exec); m->graph_exec = nullptr; }
}

// nothing recorded, no checkpoint taken, no step of a checkpointed window counted or swept (the arrays stay)
static void adjoint_window_empty(fb_model *m)
{
    m->ad_fill = m->ad_top = 0;
    m->ck_n = m->ck_done = m->ck_left = 0;
    m->ck_swept = false;
    m->ck_replayed = 0;
}

// the vorticity is replaced (state_in, fb_model_set_spectrum): the next fb_model_step starts with an eager (priming) step, and the
// adjoint's tape, or its checkpointed window, belonged to the state that went
static void state_replaced(fb_model *m)
{
    m->warmed = false;
    m->primed = 0;
    adjoint_window_empty(m);
    m->pt_fill = 0;                                         // the particle tape followed the flow that went
}

extern "C" int fb_model_destroy(fb_model *m)
{
    if (!m) return FB_OK;
    for (GroupBufs &B : m->gb) {
        if (B.w4_recv && B.w4_recv != B.w4_send) hipFree(B.w4_recv);
        if (B.t_recv && B.t_recv != B.t_send) hipFree(B.t_recv);
        cf *arr[] = {B.ZA, B.ZB, B.ACC, B.w4_send, B.t_send};
        for (cf *p : arr) if (p) hipFree(p);
    }
    model_drop_graph(m);
    if (m->src) hipFree(m->src);
    if (m->src_nz) hipFree(m->src_nz);
    for (auto p : m->rec_work) if (p) hipFree(p);
    for (auto p : m->rec_send) if (p) hipFree(p);
    if (m->keff_fields) hipFree(m->keff_fields);
    if (m->keff_red) hipFree(m->keff_red);
    if (m->azim_fields) hipFree(m->azim_fields);
    if (m->azim_red) hipFree(m->azim_red);
    if (m->cs_label) hipFree(m->cs_label);
    if (m->cs_ids) hipFree(m->cs_ids);
    if (m->cs_part) hipFree(m->cs_part);
    if (m->pres_ref) hipFree(m->pres_ref);
    if (m->spec_red) hipFree(m->spec_red);
    beside_free_all(m);
    delete m;
    return FB_OK;
}

extern "C" int fb_model_info(fb_model *m, size_t *hbm, size_t *alg)
{
    if (int rc = enter(on_model("fb_model_info", m))) return rc;
    const fb_ctx *c = m->c;
    if (hbm) {
        size_t n = m->src ? (size_t)c->XL * c->ny * 4 : 0;
        for (int g = 0; g < c->ngroups; ++g) n += (c->world > 1 ? (g < c->nact ? 13 : 11) : 8) * grp_elems(c, c->grp[g]) * sizeof(cf);
        for (int g = 0; g < c->ngroups && m->tracer; ++g) n += (g < c->nact ? 3 : 1) * grp_elems(c, c->grp[g]) * sizeof(cf);      // the tracer's state
        if (m->pt_n) n += 6 * (size_t)m->pt_n * sizeof(double) + 2 * (size_t)c->nx * c->ny * sizeof(float);               // the particles' state
        if (m->pd) n += 12 * (size_t)m->pt_n * sizeof(double);                                                             // and their deformation gradient
        n += lagrangian_bytes(m);                                                                                           // their tape and their adjoint
        for (int g = 0; g < c->ngroups && m->tg.n; ++g)       // the tangent-linear model's: per perturbation, and the one shared tg_j
            n += ((size_t)m->tg.n * (g < c->nact ? 3 : 1) + (g < c->nact ? 1 : 0)) * grp_elems(c, c->grp[g]) * sizeof(cf);
        for (int g = 0; g < c->ngroups; ++g) n += (size_t)m->tt_depth * m->tg.n * grp_elems(c, c->grp[g]) * sizeof(cf);            // and its basis tape
        n += replay_bytes(m);                                                                                               // and its replay workspace
        n += adjoint_bytes(m) + adjoint_tape_bytes(m);                                                                      // the adjoint variables and their workspace; the tape
        if (m->cs_label) n += 2 * (size_t)c->nx * c->ny * sizeof(int);                                                      // the census's labels and ids
        if (m->cs_part) n += (size_t)c->nx * c->ny / CENSUS_TILE * sizeof(int2);                                           // and its scan partials
        n += forcing_bytes(m);                                                                                              // the split stage's workspace, sums and clock
        *hbm = n;
    }
    if (alg) *alg = (size_t)320 * c->nx * c->ny;
    return FB_OK;
}

// this rank's [XL][ny] rows of vort_src (main-shallow-water.cpp:304; one GPU: every row), NULL = zeros
static int set_source(const Call &k, const float *d_src)
{
    if (int rc = enter(k)) return rc;
    fb_model *m = k.m;
    fb_ctx *c = m->c;
    // (the model has no clock: a source fixed over the window is run again exactly, another one is not)
    if (m->ck_every && m->ck_left)
        return refuse(k, "the checkpointed window holds " + std::to_string(m->ck_left) + " steps that would be run again under another source: sweep them or start a new window");
    const size_t n = (size_t)c->XL * c->ny * sizeof(float);       // the caller's local rows
    // NULL: no source.  The row kernels test m->src alone, so the row flags (XL ints) are kept for the next source.
    if (!d_src) { if (m->src) { HIPCHK(hipStreamSynchronize(c->stream)); hipFree(m->src); m->src = nullptr; } return FB_OK; }
    if (!m->src_nz && hipMalloc((void **)&m->src_nz, (size_t)c->XL * sizeof(int)) != hipSuccess) { m->src_nz = nullptr; return fail(FB_ENOMEM, "source allocation failed"); }
    // the flags exist before the source is published: a model that goes on stepping after FB_ENOMEM never pairs a source with NULL flags
    if (!m->src && hipMalloc((void **)&m->src, n) != hipSuccess) { m->src = nullptr; return fail(FB_ENOMEM, "source allocation failed"); }
    if (int rc = launch(c, k_src_row_flags, dim3(c->XL), dim3(256), 0, d_src, m->src_nz, c->ny)) return rc;
    // k_rowq and k_rowh read vort_src in their own physical-space order (so does k_rowh2, on an RK_ROWH_8192 context)
    const size_t half = (size_t)c->XL * c->ny / 2;
    switch (c->row) {
    case RK_ROWQ: return launch_n(c, k_rowq_permute_src, half, d_src, m->src, c->XL);
    case RK_ROWH_8192: return launch_n(c, k_rowh_permute_src<1>, half, d_src, m->src, c->XL);
    case RK_ROWH_16384: return launch_n(c, k_rowh_permute_src<2>, half, d_src, m->src, c->XL);
    default: HIPCHK(hipMemcpyAsync(m->src, d_src, n, hipMemcpyDeviceToDevice, c->stream)); return FB_OK;
    }
}
extern "C" int fb_model_set_source(fb_model *m, const float *d_src) { return set_source(on_model("fb_model_set_source", m), d_src); }
extern "C" int fb_slab_set_source_local(fb_slab *s, const float *d_rows) { return set_source(on_slab("fb_slab_set_source_local", s), d_rows); }

static MidArgs mid_args(fb_model *m, int g, int stage)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[g];
    const GroupBufs &B = m->gb[g];
    MidArgs a;
    a.Tin = B.t_recv; a.Zbase = B.ZA; a.Zcur = B.ZB; a.Acc = B.ACC; a.Zout = B.ZA; a.W4 = B.w4_send;
    a.ct0 = 0; a.nct = stage < 0 ? G.ncols / 16 : G.nct_active;     // priming covers every column once
    a.fstride = w4_fstride(c, G); a.rm = rowmap_w4(c, G); a.P = G.ncols; a.N1 = c->N1; a.N2 = c->N2; a.ky0 = G.ky0; a.stage = stage;
    a.nu = m->nu; a.dt = m->dt; a.coef = make_coef(c); a.tw_n = c->d_tw_n2; a.tw_big = c->d_tw_big;
    return a;
}

// stage 0..3: forward x transform of the tendency + RK update + derivatives; stage 4: PRIME (derivatives of vort_c only)
static int launch_col_full(fb_model *m, int stage)
{
    fb_ctx *c = m->c;
    const GroupBufs &B = m->gb[0];
    FullArgs a;
    a.Tin = B.t_recv; a.Zbase = B.ZA; a.Zcur = B.ZB; a.Acc = B.ACC; a.Zout = B.ZA; a.W4 = B.w4_send;
    a.fstride = (long)priv_elems(c); a.P = c->P; a.ntiles = (c->ny / 2) / 8; a.stage = stage; a.nu = m->nu; a.dt = m->dt;
    a.nsub = m->xpass; a.sub_rows = 4096;
    a.wscale = m->prescale ? 1.0f / (float)((size_t)c->nx * c->ny) : 1.0f;
    a.ntiles_run = c->grp[0].nct_active * 2 < a.ntiles ? c->grp[0].nct_active * 2 : a.ntiles;   // 16-column tiles -> 8-column tiles
    if (c->full_noskip) a.ntiles_run = a.ntiles;
    if (stage == 4) a.ntiles_run = a.ntiles + 1;
    a.coef = make_coef(c); a.tw256 = c->d_tw_256; a.tw4096 = m->xpass == XP_FULL1 ? c->d_tw_big : c->d_tw_4096;
    return launch_full(c, a);
}

// full-path model: vort_c arrives in the 3-pass layout in `spec3`: move it into k_col_full's layout (every column, the
// frozen ky = ny/2 one included) and run the PRIME launch, which leaves the four derivative fields of every column in W4
static int full_import_state(fb_model *m, cf *spec3)
{
    fb_ctx *c = m->c;
    const int ntiles = (c->ny / 2) / 8;
    int rc;
    if ((rc = launch(c, k_full_relayout<true>, dim3(c->max_wg), dim3(256), 0, (const cf *)spec3, m->gb[0].ZA, c->P, c->N1, c->N2, ntiles, (int)m->xpass, c->hy)) ||
        (rc = launch_col_full(m, 4)))
        return rc;
    m->primed = 2;
    return FB_OK;
}

// full-path model: vort_c -> 3-pass layout in `dst` (nx*P complex; pad columns zeroed)
static int full_export_state(fb_model *m, cf *dst)
{
    fb_ctx *c = m->c;
    HIPCHK(hipMemsetAsync(dst, 0, priv_elems(c) * sizeof(cf), c->stream));
    const int ntiles = (c->ny / 2) / 8;
    return launch(c, k_full_relayout<false>, dim3(c->max_wg), dim3(256), 0, (const cf *)m->gb[0].ZA, dst, c->P, c->N1, c->N2, ntiles, (int)m->xpass, c->hy);
}

// vort_c of column group g -> 3-pass layout in `dst`, whichever layout the state arrays have
static int export_state(fb_model *m, int g, cf *dst)
{
    return m->xpass != XP_COLS ? full_export_state(m, dst) : state_convert(m->c, m->c->grp[g], m->gb[g].ZA, dst, false);
}

// ---- the local passes of one RK stage, shared by the fused single-GPU flow and the multi-GPU driver ----------------
// priming: derivatives of vort_c for every column of every group; the frozen tiles get their backward strided
// sub-pass here, once -- the per-stage passes only touch the active tiles of group 0
static int model_prime(fb_model *m)
{
    fb_ctx *c = m->c;
    int rc;
    for (int g = 0; g < c->ngroups; ++g) {
        const ColGroup &G = c->grp[g];
        if ((rc = launch_col_mid(c, mid_args(m, g, -1)))) return rc;
        if ((rc = launch_col_strided<+1>(c, G, m->gb[g].w4_send, 4, w4_fstride(c, G), rowmap_w4(c, G), G.nct_active, G.ncols / 16 - G.nct_active))) return rc;
    }
    m->primed = 1;
    return FB_OK;
}
// backward strided sub-pass on the active tiles, fields [f0, f1): the multi-GPU step pipelines it field by field against
// the exchange; the fused flow runs it once right after priming (its stage loop starts with the row pass)
static int model_col_bwd_active(fb_model *m, int f0 = 0, int f1 = 4, int g = 0)
{
    fb_ctx *c = m->c;
    const ColGroup &G = c->grp[g];
    return launch_col_strided<+1>(c, G, m->gb[g].w4_send + (size_t)f0 * w4_fstride(c, G), f1 - f0, w4_fstride(c, G), rowmap_w4(c, G), 0, G.nct_active);
}
// row pass of an RK stage on the local rows [x0, x0 + nrows); the x pass XP_FULL2 comes with the row kernel k_rowh2
static int launch_fused_row(fb_model *m, int x0, int nrows)
{
    fb_ctx *c = m->c;
    RowArgs a = row_args_base(c);
    if (c->world == 1) { a.M = view_single(c, m->gb[0].w4_recv, (long)priv_elems(c)); a.T = view_single(c, m->gb[0].t_send, 0); }
    else {
        const cf *w4[3] = {m->gb[0].w4_recv, m->gb[1].w4_recv, m->gb[2].w4_recv}, *ts[3] = {m->gb[0].t_send, m->gb[1].t_send, m->gb[2].t_send};
        a.M = view_slab(c, w4, 4); a.T = view_slab(c, ts, 1); a.t_frozen = 0;
    }
    a.src = m->src; a.src_nz = m->src_nz; a.scale = 1.0f / (float)((size_t)c->nx * c->ny); a.x0 = x0; a.nx = nrows; a.prescaled = m->prescale ? 1 : 0;
    return launch_row<ROW_FUSED>(c, a, m->xpass == XP_FULL2 ? RK_ROWH2 : c->row);
}
// forward x pass of the tendency + RK stage update + derivatives of the new stage state (three-kernel path)
static int model_col_fwd(fb_model *m, int stage, int g = 0)
{
    fb_ctx *c = m->c;
    int rc;
    if ((rc = launch_col_strided<-1>(c, c->grp[g], m->gb[g].t_recv, 1, 0, rowmap_natural(), 0, c->grp[g].nct_active))) return rc;
    m->primed = 1;
    return launch_col_mid(c, mid_args(m, g, stage));
}

// optional per-launch HIP-event profiler (bench.py's roofline leg)
struct StepProf {
    std::vector<hipEvent_t> ev0[4], ev1[4];
    hipStream_t stream;
    int begin(int cls) { hipEvent_t a, b; if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return 1;
                         ev0[cls].push_back(a); ev1[cls].push_back(b); return hipEventRecord(a, stream) != hipSuccess; }
    int end(int cls) { return hipEventRecord(ev1[cls].back(), stream) != hipSuccess; }
};
#define PROF_BEGIN(cls) do { if (prof && prof->begin(cls)) return fail(FB_EHIP, "event record failed"); } while (0)
#define PROF_END(cls) do { if (prof && prof->end(cls)) return fail(FB_EHIP, "event record failed"); } while (0)

// what a step call refuses before anything is launched: a bad count, the handle (enter), a call that would overrun the adjoint's tape,
// or under checkpointing pass the window's max_steps or follow a sweep of it
static int step_refusals(const Call &k, int nsteps)
{
    if (nsteps < 0) return refuse(k, "bad argument: nsteps < 0");
    if (int rc = enter(k, NEED_TRANSPORT)) return rc;
    const fb_model *m = k.m;
    if (m->ck_every) {
        if (nsteps > 0 && m->ck_swept) return refuse(k, "the window has been swept: start a new one (fb_model_set_vort, fb_model_set_spectrum, fb_model_adjoint_checkpoint)");
        if (nsteps > m->ck_max - m->ck_done)
            return refuse(k, "the checkpointed window has room for " + std::to_string(m->ck_max - m->ck_done) + " more steps (fb_model_adjoint_checkpoint)");
    } else if (m->ad_on && nsteps > m->ad_depth - m->ad_fill)
        return refuse(k, "the adjoint's tape has room for " + std::to_string(m->ad_depth - m->ad_fill) + " more steps (fb_model_adjoint_record)");
    if (m->pt_depth && nsteps > m->pt_depth - m->pt_fill)
        return refuse(k, "the particle tape has room for " + std::to_string(m->pt_depth - m->pt_fill) + " more steps (fb_model_particle_tape)");
    return FB_OK;
}

static int model_step_impl(fb_model *m, int nsteps, StepProf *prof)
{
    fb_ctx *c = m->c;
    int rc;
    if (nsteps == 0) return FB_OK;
    if (m->xpass != XP_COLS && !m->primed) return fail(FB_EINVAL, "fb_model_step: set the state first");
    if (!m->primed && (rc = model_prime(m))) return rc;
    if (m->primed == 1 && m->xpass == XP_COLS) { if ((rc = model_col_bwd_active(m))) return rc; m->primed = 2; }
    const ColGroup &G = c->grp[0];
    GroupBufs &B = m->gb[0];
    for (int s = 0; s < nsteps; ++s) {
        for (int k = 0; k < 4; ++k) {
            if ((rc = beside_stage(m, nullptr, k))) return rc;                    // their stage k, from the state this stage starts from
            // row pass on the derivative fields left by the previous stage (or the priming pass) ...
            PROF_BEGIN(1);
            if ((rc = launch_fused_row(m, 0, c->XL))) return rc;
            PROF_END(1);
            if (m->xpass != XP_COLS) {                        // two launches per stage: row pass, single-pass x transform
                PROF_BEGIN(3);
                if ((rc = launch_col_full(m, k))) return rc;
                PROF_END(3);
                continue;
            }
            // ... then the x pass over the active column tiles: forward strided sub-pass, update + derivatives, backward strided sub-pass
            PROF_BEGIN(2);
            if ((rc = launch_col_strided<-1>(c, G, B.t_recv, 1, 0, rowmap_natural(), 0, G.nct_active))) return rc;
            PROF_END(2);
            PROF_BEGIN(3);
            if ((rc = launch_col_mid(c, mid_args(m, 0, k)))) return rc;
            PROF_END(3);
            PROF_BEGIN(0);
            if ((rc = launch_col_strided<+1>(c, G, B.w4_send, 4, (long)priv_elems(c), rowmap_natural(), 0, G.nct_active))) return rc;
            PROF_END(0);
        }
        beside_step_done(m);
        if ((rc = forcing_stage(m, nullptr))) return rc;
    }
    return FB_OK;
}

extern "C" int fb_model_use_graph(fb_model *m, int enable)
{
    if (int rc = enter(on_model("fb_model_use_graph", m))) return rc;
    m->use_graph = enable != 0;
    if (!m->use_graph) model_drop_graph(m);
    return FB_OK;
}

// nsteps steps of the one-GPU model (the step pair's body: fb_slab_driver.h)
static int model_steps(fb_model *m, int nsteps)
{
    fb_ctx *c = m->c;
    // graph replay needs a capturable (non-null) stream, a primed pipeline and at least one eager step behind
    // us (kernel attributes are set on first launch); anything else runs eagerly.  So does a model that records the adjoint's tape:
    // every step writes another slot, which a captured step would bake in (ad_on: recording now; under checkpointing the forward
    // run writes no slot, so the tape segment that is allocated does not keep it from replaying the captured step); the particle
    // tape, whose slot the particles' stage writes, likewise
    if (!m->use_graph || c->world != 1 || c->stream == nullptr || nsteps < 2 || m->ad_on || m->pt_depth) { if (nsteps > 0) m->warmed = true; return model_step_impl(m, nsteps, nullptr); }
    int rc;
    if (!m->warmed) { if ((rc = model_step_impl(m, 1, nullptr))) return rc; m->warmed = true; --nsteps; }
    if (m->graph_exec && (m->graph_src != m->src || m->graph_stream != c->stream)) model_drop_graph(m);
    if (!m->graph_exec) {
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        rc = model_step_impl(m, 1, nullptr);
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc) { if (g) hipGraphDestroy(g); return rc; }
        HIPCHK(e);
        e = hipGraphInstantiate(&m->graph_exec, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        HIPCHK(e);
        m->graph_src = m->src; m->graph_stream = c->stream;
        // the captured step has NOT executed: replay it below like the others
    }
    for (int s = 0; s < nsteps; ++s) HIPCHK(hipGraphLaunch(m->graph_exec, c->stream));
    return FB_OK;
}

extern "C" int fb_model_profile_steps(fb_model *m, int nsteps, float *ms_sum, int *launches)
{
    const Call k = on_model("fb_model_profile_steps", m);
    if (!ms_sum || !launches) return refuse(k, "NULL output");
    int rc;
    if ((rc = step_refusals(k, nsteps))) return rc;
    if (m->ck_every) return refuse(k, "not while adjoint checkpointing is on: the profiled steps would take no checkpoint (fb_model_adjoint_checkpoint)");
    StepProf prof; prof.stream = m->c->stream;
    rc = model_step_impl(m, nsteps, &prof);
    if (!rc) m->steps += nsteps;
    HIPCHK(hipStreamSynchronize(m->c->stream));
    for (int cls = 0; cls < 4; ++cls) {
        ms_sum[cls] = 0.f; launches[cls] = (int)prof.ev0[cls].size();
        for (size_t i = 0; i < prof.ev0[cls].size(); ++i) {
            float ms = 0.f;
            if (i < prof.ev1[cls].size() && hipEventElapsedTime(&ms, prof.ev0[cls][i], prof.ev1[cls][i]) == hipSuccess) ms_sum[cls] += ms;
            hipEventDestroy(prof.ev0[cls][i]);
            if (i < prof.ev1[cls].size()) hipEventDestroy(prof.ev1[cls][i]);
        }
    }
    return rc;
}

extern "C" int fb_model_get_spectrum(fb_model *m, float *d_spec)
{
    const Call k = on_model("fb_model_get_spectrum", m);
    if (!d_spec) return refuse(k, "NULL output");
    int rc;
    if ((rc = enter(k, NEED_TRANSPORT))) return rc;
    if ((rc = ensure_scratch(m->c))) return rc;
    if ((rc = export_state(m, 0, m->c->d_scratch))) return rc;
    return relayout(m->c, m->c->d_scratch, (cf *)d_spec, false);
}

extern "C" int fb_model_set_spectrum(fb_model *m, const float *d_spec)
{
    const Call k = on_model("fb_model_set_spectrum", m);
    if (!d_spec) return refuse(k, "NULL input");
    int rc;
    if ((rc = enter(k, NEED_TRANSPORT))) return rc;
    state_replaced(m);
    rc = relayout(m->c, (const cf *)d_spec, m->gb[0].ZB, true);
    if (rc) return rc;
    if (m->xpass != XP_COLS) return full_import_state(m, m->gb[0].ZB);
    return state_convert(m->c, m->c->grp[0], m->gb[0].ZB, m->gb[0].ZA, true);
}

#include "fb_slab_driver.h"
#include "fb_record.h"
#include "fb_beside.h"

// field I/O (fb_write_field / fb_read_field, writeField / readField): fb_fieldio.cpp
