// barotropic_main.cpp -- drop-in RK4 driver on the MI355X engine.
//
// Mirrors the surface of the reference drivers main.cpp:65-328 and main-shallow-water.cpp:72-349:
// same option letters (-I -O -i, plus -s -f of the source-forced variant), same output files
// (<O>/vort_src_input_step_N.bin, vort_step_N.bin, psi_step_N.bin, u_step_N.bin, v_step_N.bin),
// same ./log contents, same stdout lines, exit code 0.  The grid and model constants that
// configuration.hpp:10-36 fixes at compile time are run-time long options here.
// Stepping is the fused HIP path (fb_model_step / fb_slab_step); fields only leave HBM at record steps.
//
// Host I/O is off the critical path on every path:
//   record steps : record kernels on the compute stream -> D2H into pinned buffers on a copy stream -> a writer thread
//                  for the files and ./log, while the main thread goes on stepping (main.cpp:266-282 does all of it inline);
//   FIFO source  : a reader thread follows the producer's byte protocol (vorticity_source.cpp:112-133) ahead of the step
//                  loop into pinned buffers; a new source travels H2D on the copy stream and the compute stream waits for
//                  the copy's event only (main-shallow-water.cpp:304 reads and uploads inline).
//
// Multi-GPU (BASELINE configs 4 and 5; no reference counterpart): one process per GPU,
//     barotropic_main.out --world P --rank r --comm-file /shared/path --launch-token T ...   (same other options on every rank)
// rank 0 publishes the RCCL unique id through the comm file (host/comm_bootstrap.hpp: stale files of other launches are
// never taken), every rank reads its x rows of the initial field, steps through fb_slab_step (engine-driven RCCL all-to-all
// transposes) and writes its rows into the shared record files; rank 0 alone prints the step lines and writes ./log.  A
// FIFO source is read per rank from "<fifo>.<rank>" (vort_src_input.out --world P --rank r produces that rank's rows).
// --ranks-as-threads runs all P ranks as threads of ONE process on ONE GPU through the in-process transport: the
// rehearsal of the multi-rank host logic.
// --dump-okubo-weiss (no reference counterpart) adds okubo_weiss_step_N.bin and tau_fil_step_N.bin to every record, after v (and
// dvortdt) in ./log, on one GPU and with --world P.
// --dump-eddy-diffusivity [--keff-bins N] (no reference counterpart, N in [2, 4096], default 256) adds eddy_diffusivity_step_N.bin to
// every record: the effective eddy diffusivity table of fb_model_get_eddy_diffusivity, raw little-endian float64 [N][9], the last
// file of a record in ./log (after v, dvortdt, tau_fil or pres); on one GPU and with --world P, where rank 0 alone writes it.
// --dump-pressure [--pres-rho R] [--pres-f F] [--pres-ref-x X] [--pres-ref-y Y] (defaults 1.0, 1e-5, 0, 0: configuration.hpp:10-11,
// invert_pres.cpp:68-69) adds pres_step_N.bin to every record: the nonlinear-balance pressure that the reference's invert_pres.cpp
// computes from psi_step_N.bin afterwards (:135-185), here from the resident state (fb_model_get_pressure), after tau_fil and before
// eddy_diffusivity in ./log; on one GPU and with --world P.  A reference point outside the grid is refused (exit status 2).
// --dump-spectra (no reference counterpart) adds spectra_step_N.bin to every record: the shell spectra and cascade fluxes of
// fb_model_get_spectra, raw little-endian float64 [nshells][10] (nshells from fb_spectra_shells), after pres and before eddy_diffusivity
// in ./log; on one GPU and with --world P, where rank 0 alone writes it.
// --tracer FILE [--tracer-kappa K] (no reference counterpart, K >= 0, default 0) reads FILE from the input directory as the initial
// field is read and sets it as the model's passive tracer (fb_model_set_tracer) with the diffusivity K; every record gains
// tracer_step_N.bin, the last field file of a record in ./log, and with --dump-eddy-diffusivity tracer_eddy_diffusivity_step_N.bin
// after it (fb_model_get_tracer_eddy_diffusivity, [N][9] float64 as eddy_diffusivity); on one GPU and with --world P, where rank 0
// alone writes the table.
// --dump-azimuthal [--azim-center psi-min|vort-max|X,Y] [--azim-bins N] [--azim-dr D] [--azim-modes M] (no reference counterpart; defaults
// psi-min, D = max(dx, dy), N = floor(min(Lx, Ly) / 2 / D) at most 4096, M = 4) adds azimuthal_step_N.bin to every record: the
// azimuthal-mean table of fb_model_get_azimuthal, raw little-endian float64 [N][12 + 2 M], and azimuthal_center_step_N.bin after it:
// the four doubles xc, yc, flat index, value of the centre, so that the sequence over the records is the vortex track.  The last two
// files of a record in ./log; on one GPU and with --world P, where rank 0 alone writes them.  Arguments that the C ABI would refuse
// are refused here (exit status 2).
// --particles FILE (no reference counterpart) reads FILE from the input directory, raw little-endian float64 [n][2] positions (x, y) [m]
// with n from the file's size, and sets them as the model's Lagrangian particles (fb_model_set_particles); every record gains
// particles_step_N.bin in the same format, the unwrapped positions, the last file of a record in ./log.  One GPU only: --world P > 1,
// a file whose size is no positive multiple of 16 bytes and n above 2^24 are refused (exit status 2).
// --particle-deformation (with --particles; no reference counterpart) lets the particles carry their deformation gradient F
// (fb_model_set_particle_deformation, F = I at the start); every record gains particle_deformation_step_N.bin, raw float64 [n][4]
// (F11, F12, F21, F22), and particle_stretching_step_N.bin, [n][4] (ln sigma1, ln sigma2, theta_in, theta_out:
// fb_model_particle_stretching), right after particles_step_N.bin in ./log.  Without --particles or with --world P > 1: exit status 2.
// --tangent FILE [--tangent-renorm K] (no reference counterpart, K >= 0, default 0) reads FILE from the input directory as the initial
// field is read and sets it as the perturbation of the model's tangent-linear model (fb_model_set_tangent); every record gains
// tangent_step_N.bin and tangent_growth_step_N.bin, three float64: the time, the perturbation's enstrophy norm <dz^2> / 2 and the sum
// of ln(growth) since the start (half the log of the norm's ratios, over every renormalisation), the last two files of a record in
// ./log.  With K > 0 the perturbation is rescaled to its initial norm after every K steps.  One GPU only: --world P > 1 is refused
// (exit status 2).
// --dump-census --census-threshold T [--census-field vort|okubo-weiss] [--census-below] [--census-min-cells K] [--census-max M] (no
// reference counterpart; defaults vort, above, K = 4, M = 256) adds census_step_N.bin to every record: the vortex census table of
// fb_model_census, raw little-endian float64 [M][12] at a fixed size (rows beyond the structures found hold label -1 and zeros), of
// the structures of zeta (or of the Okubo-Weiss parameter W) above (or below) T with at least K cells, always weighted by zeta.  The
// last file of a record in ./log.  One GPU only: --world P > 1, a missing --census-threshold and arguments that the C ABI would
// refuse are refused here (exit status 2).
// --forcing-rate E --forcing-k K --forcing-width W [--forcing-seed S] [--drag MU] [--hyper-nu V --hyper-order P] (no reference
// counterpart; defaults E = 0, S = 0, MU = 0, V = 0, P = 1) set the split stage of fb_model_set_forcing after every step: stochastic
// forcing at the energy rate E [m^2 s^-3] in the ring |K - k| <= W [rad/m], linear drag MU [1/s] and hyperviscosity V K^2P.  Every
// record gains forcing_budget_step_N.bin, six float64 (fb_model_forcing_budget: the forcing clock, dE_forc, dE_diss, dZ_forc,
// dZ_diss, N_ring), the last file of a record in ./log.  One GPU only: --world P > 1, values that are negative or not finite, P
// outside [1, 8] and a rate without a ring are refused here (exit status 2).
#include <fcntl.h>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fftbaro.h"
#include "comm_bootstrap.hpp"

static void must(int status, const char *what)
{
    if (status != FB_OK) { std::fprintf(stderr, "%s: %s (%s)\n", what, fb_strerror(status), fb_last_error()); std::exit(1); }
}

enum RECIPE_TYPE { SCRIPT, FIFO, EMPTY };            // vorticity_source.cpp:48-52

struct Config {
    std::string input = "input", output = "output", init_file = "initial_vorticity.bin", vort_src_filename, comm_file, token;
    int npts = 768, record_step = 100, total_steps = -1, start_step = 0;          // configuration.hpp:18,35,36
    float LX = 600000.0f, LY = 600000.0f, NU = 6.5f, dt = 3.0f;                    // configuration.hpp:15-17,34
    RECIPE_TYPE recipe_type = EMPTY;
    int world = 1, rank = 0; bool threads = false, fanout = false;
    long comm_max_age = 60, comm_timeout = 600;
    bool timing = true;                                                            // the [timing] summary on stderr (--no-timing: off)
    int record_buffers = 0;                                                        // sets of pinned record buffers: 0 = by size (two while a set is <= 1 GiB), 1, 2
    bool dump_grad = false, dump_dvortdt = false;                                  // the OUTPUT_GRAD_VORT / OUTPUT_DVORTDT blocks of main.cpp:156-162,170-176,229-235 as run-time options
    bool dump_ow = false;                                                          // Okubo-Weiss parameter and filamentation time (no reference counterpart)
    bool dump_keff = false; int keff_bins = 256;                                   // effective eddy diffusivity table and its number of bins (no reference counterpart)
    bool dump_pres = false; float pres_rho = 1.0f, pres_f = 1e-5f;                 // balanced pressure (invert_pres.cpp:135-185); rho, f: configuration.hpp:10-11
    int pres_ref_x = 0, pres_ref_y = 0;                                            // its reference point (invert_pres.cpp:67-79)
    bool dump_spectra = false;                                                     // shell spectra and cascade fluxes (no reference counterpart)
    std::string tracer_file; float tracer_kappa = 0.0f;                            // the passive tracer's initial field and diffusivity (no reference counterpart)
    bool dump_azim = false; int azim_mode = FB_CENTER_PSI_MIN; double azim_xc = 0.0, azim_yc = 0.0;   // azimuthal means about a vortex centre (no reference counterpart)
    int azim_bins = 0, azim_modes = 4; double azim_dr = 0.0;                       // 0: the default number of bins / bin width
    std::string tangent_file; int tangent_renorm = 0;                              // the tangent-linear model's initial perturbation; renormalise every K steps (no reference counterpart)
    bool particle_deformation = false;                                             // --particle-deformation: the particles carry F, recorded with its stretching table
    bool dump_census = false, census_have_thr = false, census_ow = false, census_below = false;       // the vortex census (no reference counterpart)
    float census_thr = 0.0f; int census_min = 4, census_max = 256;
    std::string particles_file; int n_particles = 0;                               // the Lagrangian particles' initial positions and their number (no reference counterpart)
    double forcing_rate = 0.0, forcing_k = 0.0, forcing_width = 0.0, drag = 0.0, hyper_nu = 0.0;     // the split stage after every step (no reference counterpart)
    unsigned long long forcing_seed = 0; int hyper_order = 1;
    bool forcing() const { return forcing_rate > 0.0 || drag > 0.0 || hyper_nu > 0.0; }
};

// --fifo-fanout (multi-GPU, SURVEY.md section 8(e) "rank 0 reads, scatters x-slabs"): ONE producer that writes whole fields -- the
// reference's unmodified vort_src_input.out -- feeds every rank.  The lead rank reads `<fifo>` (flag byte per step, GRIDS float32 after
// a flag of 1: vorticity_source.cpp:112-133) and passes the same protocol on to `<fifo>.<r>`, each rank's x rows only; the ranks read
// their `<fifo>.<r>` as they do when per-rank producers feed them.  The launcher creates the FIFOs.
static void fifo_fanout(const Config cfg)
{
    const size_t slab = (size_t)(cfg.npts / cfg.world) * cfg.npts;
    FILE *in = fopen(cfg.vort_src_filename.c_str(), "rb");
    std::vector<FILE *> out(cfg.world, nullptr);
    bool opened = in != nullptr;
    if (!in) printf("ERROR: cannot open file [%s].\n", cfg.vort_src_filename.c_str());
    for (int r = 0; r < cfg.world && opened; ++r) {
        const std::string fn = cfg.vort_src_filename + "." + std::to_string(r);
        if ((out[r] = fopen(fn.c_str(), "wb")) == NULL) { printf("ERROR: cannot open file [%s].\n", fn.c_str()); opened = false; }
    }
    if (!opened) {
        // One FIFO of the fan-out is missing: the readers of those already opened get their EOF, and the launch ends here with a
        // failure instead of leaving ranks inside fopen/fread for ever (the reference has ONE reader, vorticity_source.cpp:121-124,
        // so it knows no such state).  _exit: this is a side thread of a process that is busy on the GPU.
        for (FILE *f : out) if (f) fclose(f);
        if (in) fclose(in);
        fflush(stdout); fflush(stderr);
        _exit(1);
    }
    std::vector<float> buf(slab * (size_t)cfg.world);
    char flag;
    while (fread(&flag, 1, 1, in) == 1) {
        if (((unsigned int)flag) != 1) { for (FILE *f : out) { fwrite(&flag, 1, 1, f); fflush(f); } continue; }
        // a record goes out only when ALL of it has arrived: a short one is passed on to no rank (every rank keeps the source it has,
        // finds EOF and says so), never to some of them -- the ranks must not integrate different forcings
        if (fread(buf.data(), sizeof(float), buf.size(), in) != buf.size()) { fprintf(stderr, "ERROR: Cannot read vorticity source input.\n"); fflush(stderr); break; }
        for (int r = 0; r < cfg.world; ++r) {                                          // the field is x-major: rank r's rows are the r-th piece of the record
            fwrite(&flag, 1, 1, out[r]);
            fwrite(buf.data() + (size_t)r * slab, sizeof(float), slab, out[r]);
            fflush(out[r]);
        }
    }
    for (FILE *f : out) fclose(f);                                                     // EOF for every rank ("No flag was detected")
    fclose(in);
}

// ---- the source: VortSrcRecipeReader<GRIDS> (vorticity_source.cpp:48-135) with the FIFO read ahead of the step loop ------------
// The byte protocol is the reference's: per step one flag byte, followed by `n` float32 when the flag is 1
// (vorticity_source.cpp:112-133).  A reader thread consumes it as fast as the producer writes and parks every new source in
// one of three pinned buffers; the step loop takes one entry per step, so what each step sees -- and what stderr says about
// it -- is what the inline fread of the reference would have seen.
struct SourceFeed {
    struct Entry { int status; int buf; };            // status: 0 flag 0, 1 new source in buf, -1 no flag (EOF), -2 short payload
    RECIPE_TYPE type = EMPTY; std::string filename; size_t n = 0; FILE *fifo = nullptr;
    float *pin[3] = {nullptr, nullptr, nullptr};
    int holds[3] = {0, 0, 0};                         // current source / queued / held by the record writer
    int cur = -1;                                     // buffer of the source in force (-1: zeros)
    std::deque<Entry> q; bool eof = false, quit = false;
    std::mutex mu; std::condition_variable cv; std::thread th;

    void init(RECIPE_TYPE t, const std::string &fn, size_t floats)
    {
        type = t; filename = fn; n = floats;
        if (type == SCRIPT) readScript();
        else if (type == FIFO) {
            if ((fifo = fopen(filename.c_str(), "rb")) == NULL) { printf("ERROR: cannot open file [%s].\n", filename.c_str()); return; }
            for (auto &p : pin) must(fb_malloc_host((void **)&p, n * sizeof(float)), "fb_malloc_host");
            th = std::thread([this] { run(); });
        }
    }
    int readScript()                                  // vorticity_source.cpp:100-110: only opens the file (unimplemented upstream)
    {
        FILE *fd = fopen(filename.c_str(), "r");
        if (fd == NULL) printf("ERROR: cannot open file [%s].\n", filename.c_str()); else fclose(fd);
        return 0;
    }
    void run()
    {
        for (;;) {
            char flag;
            if (fread(&flag, sizeof(char), 1, fifo) != 1) break;                     // EOF: every later step finds no flag either
            Entry e{0, -1};
            if (((unsigned int)flag) == 1) {
                std::unique_lock<std::mutex> lk(mu);
                int b = -1;
                cv.wait(lk, [&] { if (quit) return true; for (int i = 0; i < 3; ++i) if (holds[i] == 0) { b = i; return true; } return false; });
                if (quit) return;
                holds[b] = 1;
                lk.unlock();
                const bool ok = fread(pin[b], sizeof(float), n, fifo) == n;
                e = Entry{ok ? 1 : -2, b};
            }
            { std::lock_guard<std::mutex> lk(mu); q.push_back(e); }
            cv.notify_all();
            if (e.status == -2) break;
        }
        { std::lock_guard<std::mutex> lk(mu); eof = true; }
        cv.notify_all();
    }
    // one step's read (main-shallow-water.cpp:304); returns the entry, with the reference's stderr lines
    Entry read()
    {
        if (type == SCRIPT) { readScript(); return Entry{0, -1}; }
        if (type != FIFO) return Entry{0, -1};
        Entry e{-1, -1};
        if (fifo) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !q.empty() || eof; });
            if (!q.empty()) { e = q.front(); q.pop_front(); }
        }
        if (e.status == -1) { fprintf(stderr, "No flag was detected, assume flag = 0\n"); fflush(stderr); }
        else if (e.status == -2) { fprintf(stderr, "ERROR: Cannot read vorticity source input.\n"); fflush(stderr); release(e.buf); }
        else if (e.status == 1) fprintf(stderr, "New vorticity source was given.\n");
        else { fprintf(stderr, "No new vorticity source input was given.\n"); fflush(stderr); }
        return e;
    }
    void hold(int b) { if (b >= 0) { std::lock_guard<std::mutex> lk(mu); ++holds[b]; } }
    void release(int b) { if (b >= 0) { { std::lock_guard<std::mutex> lk(mu); --holds[b]; } cv.notify_all(); } }
    void make_current(int b) { const int old = cur; cur = b; release(old); }          // the queue's hold on b becomes the "current" hold
    // true: the reader is out of the FIFO and everything is released; false: it still sits in fread on an open FIFO (a producer
    // that outlives the run) -- the object, its stream and its buffers must then be left to process exit
    bool shutdown()
    {
        bool done;
        { std::lock_guard<std::mutex> lk(mu); quit = true; done = eof; }
        cv.notify_all();
        if (!th.joinable()) { if (fifo) fclose(fifo); return true; }
        if (!done) { th.detach(); return false; }
        th.join();
        fclose(fifo);
        for (auto p : pin) fb_free_host(p);
        return true;
    }
};

// ---- the table of record outputs --------------------------------------------------------------------------------------------
// What a record step writes, one entry per file, in the order of ./log: the reference's (main.cpp:266-282, then the stage-0 dumps
// :156-235), followed by the outputs that have no reference counterpart.  run_rank builds the table once from Config; device and pinned
// allocation, the D2H copies of a record, the writer's file loop, the byte count and the frees are loops over it.
//   ROWS   a float32 field of which this rank holds `bytes`: fb_write_field on one GPU, pwrite at the rank's offset on several;
//          pinned on every rank
//   WHOLE  raw bytes, one whole file by fopen/fwrite: written, and pinned, on the lead rank alone; the device buffer exists on every
//          rank, because the record calls are collective.  Without a device buffer the step loop fills the host bytes itself.
//   SOURCE vort_src as of the record step: no buffer of its own, it comes from Job::src
// Adding an output takes its option in Config and main(), one line in run_rank's table at its place in ./log, and the engine call that
// fills its device buffer in the record branch: nothing else.
struct Output {
    enum Kind { ROWS, WHOLE, SOURCE };
    const char *stem; Kind kind; size_t bytes;
    void *dev;                                                                         // NULL: none
    void *host[2];                                                                     // per set of record buffers; NULL: not on this rank
};

// ---- the record path: main.cpp:266-282 and the stage-0 dumps :181-222, written by a thread of its own ---------------------------
struct RecordWriter {
    // Up to TWO sets of pinned buffers, each with the event behind its D2H copies: the step loop hands a record over and goes on; it has
    // to wait only when BOTH sets are still with the writer, i.e. for the record before last.  With one set it waited for the previous
    // record's files at every record step, and one slow record -- measured: 85-96 ms for 336 MB where the average is 50 ms and the stretch
    // between two records 84 ms -- left the compute stream dry (1119-1155 against 1190 steps/s at 4096^2).
    struct Job { int step, set; const float *src; int src_buf; };
    std::thread th; std::mutex mu; std::condition_variable cv;
    std::deque<Job> jobs; bool writing = false, quit = false;
    int nsets = 1; bool set_free[2] = {true, true};
    void *e_copy[2] = {nullptr, nullptr};
    const std::vector<Output> *outs = nullptr;                                         // the table; fixed before start()
    SourceFeed *feed = nullptr;                                                        // vort_src as of the record step is held until written
    std::string output; FILE *log_fd = nullptr;
    bool whole = true, lead = true; off_t off = 0;                                     // whole file (writeField) or this rank's byte range
    double busy_s = 0.0, slowest_s = 0.0; size_t bytes = 0;                            // time spent writing (total, slowest record) and what was written ([timing] summary)
    void start() { th = std::thread([this] { run(); }); }
    void run()
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [this] { return !jobs.empty() || quit; });
            if (jobs.empty() && quit) return;
            const Job job = jobs.front();
            jobs.pop_front();
            writing = true;
            lk.unlock();
            must(fb_event_synchronize(e_copy[job.set]), "record: wait for copies");
            const auto w0 = std::chrono::steady_clock::now();
            char fn[1024];
            for (const Output &o : *outs) {                                            // main.cpp:268-278, :156-235
                snprintf(fn, sizeof fn, "%s/%s_step_%d.bin", output.c_str(), o.stem, job.step);
                if (o.kind == Output::WHOLE) {
                    if (!lead) continue;
                    FILE *f = fopen(fn, "wb");
                    if (!f || fwrite(o.host[job.set], 1, o.bytes, f) != o.bytes) { perror("Write field."); std::exit(1); }
                    fclose(f);
                    if (!whole) fprintf(stderr, "Output %s\n", fn);
                    fprintf(log_fd, "%s\n", fn); fflush(log_fd);
                    bytes += o.bytes;
                    continue;
                }
                const float *data = o.kind == Output::SOURCE ? job.src : (const float *)o.host[job.set];
                if (whole) must(fb_write_field(fn, data, o.bytes / sizeof(float)), "writeField");
                else {
                    const int fd = open(fn, O_WRONLY | O_CREAT, 0644);
                    const char *p = (const char *)data; size_t left = o.bytes; off_t at = off;
                    while (fd >= 0 && left) { const ssize_t k = pwrite(fd, p, left, at); if (k <= 0) break; p += k; left -= (size_t)k; at += k; }
                    if (fd < 0 || left) { perror("Write field."); std::exit(1); }
                    close(fd);
                    if (lead) fprintf(stderr, "Output %s\n", fn);
                }
                if (lead) { fprintf(log_fd, "%s\n", fn); fflush(log_fd); }
                bytes += o.bytes;
            }
            if (feed) feed->release(job.src_buf);
            const double this_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            busy_s += this_s;
            if (this_s > slowest_s) slowest_s = this_s;
            lk.lock();
            writing = false;
            set_free[job.set] = true;
            cv.notify_all();
        }
    }
    // a set of pinned buffers the writer is done with (blocks while every set is still queued or being written)
    int acquire()
    {
        std::unique_lock<std::mutex> lk(mu);
        int got = -1;
        cv.wait(lk, [&] { for (int i = 0; i < nsets; ++i) if (set_free[i]) { got = i; return true; } return false; });
        set_free[got] = false;
        return got;
    }
    void submit(const Job &j) { { std::lock_guard<std::mutex> lk(mu); jobs.push_back(j); } cv.notify_all(); }
    void wait_idle() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return jobs.empty() && !writing; }); }
    void stop() { wait_idle(); { std::lock_guard<std::mutex> lk(mu); quit = true; } cv.notify_all(); if (th.joinable()) th.join(); }
};

// ---- the engine: one GPU (fb_model) or this rank's slab of several (fb_slab) -----------------------------------------------------
// The C ABI pairs fb_model_X with fb_slab_Y (Y = X, or X_local where the slab call takes this rank's rows): same arguments behind the
// handle, one body in the library, and what needs one GPU is refused there on several ranks.  ENGINE_CALL calls the member of the pair
// that applies; must() names it.
#define ENGINE_CALL(eng, X, Y, ...) \
    must((eng).sl ? fb_slab_##Y((eng).sl, __VA_ARGS__) : fb_model_##X((eng).model, __VA_ARGS__), (eng).sl ? "fb_slab_" #Y : "fb_model_" #X)
struct Engine {
    fb_ctx *fop = nullptr; fb_model *model = nullptr; void *compute = nullptr;         // one GPU: the record kernels run on `compute`
    fb_slab *sl = nullptr;                                                             // several: the slab owns its stream
    int npts = 0;
    Engine(const Config &cfg, int rank, void *hub) : npts(cfg.npts)
    {
        if (cfg.world == 1) {
            must(fb_create(&fop, cfg.npts, cfg.npts, cfg.LX, cfg.LY), "fb_create");
            must(fb_stream_create(&compute), "stream");
            must(fb_set_stream(fop, compute), "fb_set_stream");
            must(fb_model_create(&model, fop, cfg.NU, cfg.dt), "fb_model_create");
            return;
        }
        if (!hub && rank == 0) fbcomm::prepare(cfg.comm_file);                         // before anything else: no rank may find a leftover
        must(fb_slab_create(&sl, cfg.npts, cfg.npts, cfg.LX, cfg.LY, cfg.NU, cfg.dt, rank, cfg.world), "fb_slab_create");
        if (hub) { must(fb_slab_connect_local(sl, hub), "fb_slab_connect_local"); return; }
        char id[FB_UNIQUE_ID_BYTES];
        if (rank == 0) {
            must(fb_slab_unique_id(id), "fb_slab_unique_id");
            if (!fbcomm::publish(cfg.comm_file, cfg.token, id, sizeof id)) { perror("comm file"); std::exit(1); }
        } else if (!fbcomm::await(cfg.comm_file, cfg.token, id, sizeof id, cfg.comm_timeout, cfg.comm_max_age)) {
            std::fprintf(stderr, "rank %d: no RCCL id of this launch in %s\n", rank, cfg.comm_file.c_str());
            std::exit(1);
        }
        must(fb_slab_connect_rccl(sl, id), "fb_slab_connect_rccl");
    }
    ~Engine()
    {
        if (sl) { fb_slab_destroy(sl); return; }
        for (float *p : {d_spec, d_tmp, d_gx, d_gy}) if (p) fb_free(p);
        fb_model_destroy(model); fb_destroy(fop); fb_stream_destroy(compute);
    }
    void record(void *e) { must(sl ? fb_slab_record_event(sl, e) : fb_event_record(e, compute), "record"); }      // event behind what the compute stream holds
    void wait(void *e) { must(sl ? fb_slab_wait_event(sl, e) : fb_stream_wait_event(compute, e), "wait"); }       // compute stream waits for it
    void step() { must(sl ? fb_slab_step(sl, 1) : fb_model_step(model, 1), sl ? "fb_slab_step" : "fb_model_step"); }   // main.cpp:286-317
    void sync() { must(sl ? fb_slab_synchronize(sl) : fb_synchronize(fop), "sync"); }
    // the optional stage-0 dumps of getDvortdt(debug) (main.cpp:156-162,170-176,229-235), one GPU only: dvortdx, dvortdy and
    // dvortdt = -u dvortdx - v dvortdy + vort_src of the CURRENT state (u, v as the record branch got them; src NULL = zeros); any output may be NULL
    float *d_spec = nullptr, *d_tmp = nullptr, *d_gx = nullptr, *d_gy = nullptr;
    void get_debug(float *d_dzdx, float *d_dzdy, float *d_dzdt, const float *d_u, const float *d_v, const float *d_src)
    {
        // the reference's own operator sequence on vort_c (main.cpp:151-168,225-227) through the operator entry points of the C ABI
        // (bit-exact standalone kernels): off the hot path, only on record steps and only when asked for
        if (!d_spec) {
            const size_t nreal = (size_t)npts * npts;
            const size_t spec = (size_t)npts * (npts / 2 + 1) * 2 * sizeof(float);
            must(fb_malloc((void **)&d_spec, spec), "fb_malloc"); must(fb_malloc((void **)&d_tmp, spec), "fb_malloc");
            must(fb_malloc((void **)&d_gx, nreal * sizeof(float)), "fb_malloc"); must(fb_malloc((void **)&d_gy, nreal * sizeof(float)), "fb_malloc");
        }
        must(fb_model_get_spectrum(model, d_spec), "fb_model_get_spectrum");
        float *gx = d_dzdx ? d_dzdx : d_gx, *gy = d_dzdy ? d_dzdy : d_gy;
        must(fb_gradx(fop, d_spec, d_tmp), "gradx"); must(fb_c2r(fop, d_tmp, gx, 1), "c2r");          // main.cpp:151,154
        must(fb_grady(fop, d_spec, d_tmp), "grady"); must(fb_c2r(fop, d_tmp, gy, 1), "c2r");          // main.cpp:165,168
        if (d_dzdt) must(fb_jacobian(fop, d_u, d_v, gx, gy, d_src, d_dzdt), "jacobian");               // main.cpp:225-227
    }
    double tangent_norm(double *d_scratch)                                             // the enstrophy norm, on the host, one GPU only: waits for the compute stream
    {
        double v = 0.0;
        must(fb_model_tangent_norm(model, 0, d_scratch), "fb_model_tangent_norm");
        must(fb_memcpy_d2h(fop, &v, d_scratch, sizeof v), "d2h");
        return v;
    }
};

// ---- one rank's run: the whole program when world == 1 --------------------------------------------------------------------------
static void run_rank(const Config &cfg, int rank, void *hub, FILE *log_fd, bool lead)
{
    const int N = cfg.npts, P = cfg.world;
    const size_t floats = (size_t)(N / P) * N;                                         // this rank's share of a field (all of it on one GPU)
    const off_t off = (off_t)rank * floats * sizeof(float);
    Engine *eng = new Engine(cfg, rank, hub);
    void *copy = nullptr, *e_rec = nullptr, *e_h2d = nullptr, *e_src = nullptr;
    must(fb_stream_create(&copy), "stream");
    for (void **e : {&e_rec, &e_h2d, &e_src}) must(fb_event_create(e), "event");
    const bool tracer = !cfg.tracer_file.empty(), tangent = !cfg.tangent_file.empty();
    float *d_in = nullptr;
    must(fb_malloc((void **)&d_in, floats * sizeof(float)), "fb_malloc");

    // the table of outputs, in the order of ./log; a handle is the entry's index, -1 where the option is off
    std::vector<Output> outs;
    auto add = [&](const char *stem, Output::Kind kind, size_t bytes, bool on_device) -> int {
        Output o = {stem, kind, bytes, nullptr, {nullptr, nullptr}};
        if (on_device) must(fb_malloc(&o.dev, bytes), "fb_malloc");
        outs.push_back(o);
        return (int)outs.size() - 1;
    };
    auto rows = [&](bool on, const char *stem) { return on ? add(stem, Output::ROWS, floats * sizeof(float), true) : -1; };
    auto whole = [&](bool on, const char *stem, size_t bytes) { return on ? add(stem, Output::WHOLE, bytes, true) : -1; };
    int nshells = 0;
    if (cfg.dump_spectra) must(fb_spectra_shells(N, N, cfg.LX, cfg.LY, &nshells), "fb_spectra_shells");
    const size_t keff_bytes = (size_t)cfg.keff_bins * 9 * sizeof(double), np = (size_t)cfg.n_particles;
    add("vort_src_input", Output::SOURCE, floats * sizeof(float), false);              // main.cpp:268-278
    const int o_vort = rows(true, "vort");
    const int o_dzdx = rows(cfg.dump_grad, "dvortdx"), o_dzdy = rows(cfg.dump_grad, "dvortdy");                   // main.cpp:156-162,170-176
    const int o_psi = rows(true, "psi"), o_u = rows(true, "u"), o_v = rows(true, "v");                            // main.cpp:181-222
    const int o_dzdt = rows(cfg.dump_dvortdt, "dvortdt");                              // main.cpp:229-235
    const int o_ow = rows(cfg.dump_ow, "okubo_weiss"), o_tau = rows(cfg.dump_ow, "tau_fil");
    const int o_pres = rows(cfg.dump_pres, "pres");                                    // invert_pres.cpp:187
    const int o_spectra = whole(cfg.dump_spectra, "spectra", (size_t)nshells * 10 * sizeof(double));
    const int o_keff = whole(cfg.dump_keff, "eddy_diffusivity", keff_bytes);
    const int o_tracer = rows(tracer, "tracer");
    const int o_tkeff = whole(tracer && cfg.dump_keff, "tracer_eddy_diffusivity", keff_bytes);
    const int o_azim = whole(cfg.dump_azim, "azimuthal", (size_t)cfg.azim_bins * (12 + 2 * cfg.azim_modes) * sizeof(double));
    const int o_center = whole(cfg.dump_azim, "azimuthal_center", 4 * sizeof(double));
    const int o_part = whole(np > 0, "particles", np * 2 * sizeof(double));            // in once, out at every record
    const int o_def = whole(cfg.particle_deformation, "particle_deformation", np * 4 * sizeof(double));
    const int o_stretch = whole(cfg.particle_deformation, "particle_stretching", np * 4 * sizeof(double));
    const int o_tangent = rows(tangent, "tangent");
    const int o_growth = tangent ? add("tangent_growth", Output::WHOLE, 3 * sizeof(double), false) : -1;          // time, norm, sum of ln(growth): filled by the step loop
    const int o_census = whole(cfg.dump_census, "census", (size_t)cfg.census_max * FB_CENSUS_COLS * sizeof(double));
    const int o_budget = cfg.forcing() ? add("forcing_budget", Output::WHOLE, 6 * sizeof(double), false) : -1;     // filled by the step loop
    auto F = [&](int o) { return o < 0 ? (float *)nullptr : (float *)outs[o].dev; };   // an entry's device buffer; NULL where the option is off
    auto D = [&](int o) { return o < 0 ? (double *)nullptr : (double *)outs[o].dev; };

    // device buffers that are no output: the census's two counts, and W where the census is of W and no record buffer holds it
    int *d_census_count = nullptr; float *d_census_w = nullptr;
    if (cfg.dump_census) {
        must(fb_malloc((void **)&d_census_count, 2 * sizeof(int)), "fb_malloc");
        if (cfg.census_ow && !cfg.dump_ow) must(fb_malloc((void **)&d_census_w, floats * sizeof(float)), "fb_malloc");
    }
    // the tangent's norm (--tangent): one float64 on the device; its norm at the start, at the last renormalisation, and the sum of
    // ln(growth) over the renormalisations so far
    double *d_norm = nullptr, tg_norm0 = 0.0, tg_norm_ref = 0.0, tg_sum = 0.0;
    if (tangent) must(fb_malloc((void **)&d_norm, sizeof(double)), "fb_malloc");

    RecordWriter writer;
    size_t set_bytes = 0;                                                              // of the fields: the tables do not count towards the choice
    for (const Output &o : outs) if (o.kind == Output::ROWS) set_bytes += o.bytes;
    writer.nsets = cfg.record_buffers == 1 || cfg.record_buffers == 2 ? cfg.record_buffers : (set_bytes <= ((size_t)1 << 30) ? 2 : 1);
    for (int b = 0; b < writer.nsets; ++b) {
        must(fb_event_create(&writer.e_copy[b]), "event");
        for (Output &o : outs)
            if (o.kind == Output::ROWS || (o.kind == Output::WHOLE && lead)) must(fb_malloc_host(&o.host[b], o.bytes), "fb_malloc_host");
    }
    writer.outs = &outs;
    writer.output = cfg.output; writer.log_fd = log_fd;
    writer.whole = P == 1; writer.lead = lead; writer.off = off;
    writer.start();
    int last_set = -1;                                                                 // the set the previous record's D2H copies went into
    std::vector<float> zeros(floats, 0.0f);                                            // vort_src before the first input (main.cpp:110 leaves it uninitialised)
    char filename[1024];

    // readField (main.cpp:143-144) into a pinned buffer and on into d_in; a rank reads its rows of the file (fieldio.cpp:21-33 reads all of it)
    auto read_rows = [&](float *h0) {
        if (P == 1) must(fb_read_field(filename, h0, floats), "readField");
        else {
            const int fd = open(filename, O_RDONLY);
            char *p = (char *)h0; size_t left = floats * sizeof(float); off_t o = off;
            while (fd >= 0 && left) { const ssize_t k = pread(fd, p, left, o); if (k <= 0) break; p += k; left -= (size_t)k; o += k; }
            if (fd < 0 || left) { perror("Read field."); std::exit(1); }
            close(fd);
            if (lead) fprintf(stderr, "%d bytes read: %s\n", (int)((size_t)N * N), filename);
        }
        must(fb_memcpy_h2d_async(copy, d_in, h0, floats * sizeof(float)), "h2d");
        must(fb_event_record(e_h2d, copy), "record");
        eng->wait(e_h2d);
    };
    snprintf(filename, sizeof filename, "%s/%s", cfg.input.c_str(), cfg.init_file.c_str());
    read_rows((float *)outs[o_vort].host[0]);
    SourceFeed *feedp = new SourceFeed;
    SourceFeed &feed = *feedp;
    const std::string fifo = (P == 1 || cfg.vort_src_filename.empty()) ? cfg.vort_src_filename : cfg.vort_src_filename + "." + std::to_string(rank);
    feed.init(cfg.recipe_type, fifo, floats);                                          // main-shallow-water.cpp:151-152
    writer.feed = &feed;
    if (lead) printf("Initialization complete.\n");
    ENGINE_CALL(*eng, set_vort, set_vort_local, d_in);                                                               // main.cpp:256
    eng->record(e_src);                                                                // d_in is free again behind this
    must(fb_event_synchronize(e_h2d), "sync");                                         // the pinned buffer goes back to the record path
    if (tracer) {                                                                      // the tracer's field, as the initial field was read
        snprintf(filename, sizeof filename, "%s/%s", cfg.input.c_str(), cfg.tracer_file.c_str());
        must(fb_stream_wait_event(copy, e_src), "wait");                               // set_vort has read d_in
        read_rows((float *)outs[o_tracer].host[0]);
        ENGINE_CALL(*eng, set_tracer, set_tracer_local, d_in, cfg.tracer_kappa);
        eng->record(e_src);
        must(fb_event_synchronize(e_h2d), "sync");
    }
    if (o_part >= 0) {                                                                 // the particles' positions, through a pinned record buffer
        const Output &part = outs[o_part];
        snprintf(filename, sizeof filename, "%s/%s", cfg.input.c_str(), cfg.particles_file.c_str());
        FILE *f = fopen(filename, "rb");
        if (!f || fread(part.host[0], 1, part.bytes, f) != part.bytes) { perror("Read particles."); std::exit(1); }
        fclose(f);
        must(fb_memcpy_h2d_async(copy, part.dev, part.host[0], part.bytes), "h2d");
        must(fb_event_record(e_h2d, copy), "record");
        eng->wait(e_h2d);
        ENGINE_CALL(*eng, set_particles, set_particles, D(o_part), cfg.n_particles);
        if (o_def >= 0) ENGINE_CALL(*eng, set_particle_deformation, set_particle_deformation, 1);
        must(fb_event_synchronize(e_h2d), "sync");
    }
    if (tangent) {                                                                     // the perturbation's field, as the initial field was read
        snprintf(filename, sizeof filename, "%s/%s", cfg.input.c_str(), cfg.tangent_file.c_str());
        must(fb_stream_wait_event(copy, e_src), "wait");                               // set_vort / set_tracer has read d_in
        read_rows((float *)outs[o_tangent].host[0]);
        ENGINE_CALL(*eng, set_tangent, set_tangent, d_in);
        eng->record(e_src);
        must(fb_event_synchronize(e_h2d), "sync");
        tg_norm0 = tg_norm_ref = eng->tangent_norm(d_norm);
        if (!(tg_norm0 > 0.0) || !std::isfinite(tg_norm0)) { std::fprintf(stderr, "--tangent: the perturbation's norm is %g\n", tg_norm0); std::exit(1); }
    }

    if (cfg.forcing()) {                                                               // the split stage, after whatever it acts on has been set
        const int st = fb_model_set_forcing(eng->model, cfg.forcing_rate, cfg.forcing_k, cfg.forcing_width, (size_t)cfg.forcing_seed, cfg.drag, cfg.hyper_nu, cfg.hyper_order);
        if (st == FB_EINVAL) { std::fprintf(stderr, "--forcing-rate: %s\n", fb_last_error()); std::exit(2); }     // a ring that is empty on this grid, or that leaves the dealiasing circle
        must(st, "fb_model_set_forcing");
    }

    // [timing] ("add steps/s + GB/s summary"; the reference prints no timing, main.cpp:262-264).  The step loop is
    // never synchronised for it: time-stamped events on the compute stream bracket the stretches BETWEEN record steps -- a stretch ends
    // where the record branch begins, before the host waits for the writer, and the next one begins behind the record kernels -- so
    // their sum is the GPU time of the stepping alone; the host clock around the whole loop, writer included, gives the rate with records.
    const bool timing = cfg.timing && cfg.total_steps > cfg.start_step;
    std::vector<void *> t_beg, t_end;
    auto stamp = [&](std::vector<void *> &v) { if (!timing) return; void *e = nullptr; must(fb_event_create_timing(&e), "event"); eng->record(e); v.push_back(e); };
    eng->sync();
    const auto wall0 = std::chrono::steady_clock::now();
    int n_records = 0;
    double host_wait_s = 0.0, host_get_s = 0.0, host_copy_s = 0.0;                     // host time inside the record branch, by part
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    stamp(t_beg);

    // The reference can be restarted from any vort_step_N.bin via -i, but always renumbers from 0
    // (SURVEY section 5); --start-step N continues the numbering and the source clock instead.
    for (int step = cfg.start_step; step < cfg.total_steps; ++step) {                  // main.cpp:260
        const bool record = (step % cfg.record_step) == 0;
        if (lead) { printf("# Step %d, time = %.2f", step, step * cfg.dt); if (record) printf(", record now!"); printf("\n"); }
        if (record) {                                                                  // main.cpp:266-282 and the stage-0 dumps :181-222
            stamp(t_end);
            ++n_records;
            auto h0 = std::chrono::steady_clock::now();
            const int set = writer.acquire();                                          // a set of pinned buffers the writer is done with
            host_wait_s += since(h0);
            if (last_set >= 0) eng->wait(writer.e_copy[last_set]);                     // device record buffers are free again: the previous record's copies have left them
            feed.hold(feed.cur);                                                       // vort_src as of this step (dumped BEFORE this step's read)
            RecordWriter::Job job{step, set, feed.cur >= 0 ? feed.pin[feed.cur] : zeros.data(), feed.cur};
            h0 = std::chrono::steady_clock::now();
            // the record kernels, on the compute stream, in the order of the data flow (not of ./log)
            ENGINE_CALL(*eng, get_vort, get_vort_local, F(o_vort));
            ENGINE_CALL(*eng, get_diag, get_diag_local, F(o_psi), F(o_u), F(o_v));      // functions of vort_c only: the reference's stage-0 values
            host_get_s += since(h0);
            if (cfg.dump_grad || cfg.dump_dvortdt) {
                // vort_src on the device: d_in holds the source in force once one has been uploaded (before that: zeros = NULL)
                eng->get_debug(F(o_dzdx), F(o_dzdy), F(o_dzdt), F(o_u), F(o_v), feed.cur >= 0 ? d_in : nullptr);
                eng->record(e_src);                                                    // d_in may be overwritten behind this
            }
            if (cfg.dump_ow) ENGINE_CALL(*eng, get_okubo_weiss, get_okubo_weiss_local, F(o_ow), F(o_tau));
            if (cfg.dump_pres) ENGINE_CALL(*eng, get_pressure, get_pressure_local, cfg.pres_rho, cfg.pres_f, cfg.pres_ref_x, cfg.pres_ref_y, F(o_pres));
            if (cfg.dump_spectra) ENGINE_CALL(*eng, get_spectra, get_spectra, D(o_spectra));
            if (cfg.dump_keff) ENGINE_CALL(*eng, get_eddy_diffusivity, get_eddy_diffusivity, cfg.keff_bins, D(o_keff), nullptr, nullptr);
            if (tracer) ENGINE_CALL(*eng, get_tracer, get_tracer_local, F(o_tracer));
            if (o_tkeff >= 0) ENGINE_CALL(*eng, get_tracer_eddy_diffusivity, get_tracer_eddy_diffusivity, cfg.keff_bins, D(o_tkeff), nullptr, nullptr);
            if (cfg.dump_azim)
                ENGINE_CALL(*eng, get_azimuthal, get_azimuthal, cfg.azim_mode, cfg.azim_xc, cfg.azim_yc, cfg.azim_bins, cfg.azim_dr, cfg.azim_modes, D(o_azim), D(o_center));
            if (o_part >= 0) ENGINE_CALL(*eng, get_particles, get_particles, D(o_part));
            if (o_def >= 0) {
                ENGINE_CALL(*eng, get_particle_deformation, get_particle_deformation, D(o_def), nullptr);
                ENGINE_CALL(*eng, particle_stretching, particle_stretching, nullptr, 0, D(o_stretch));
            }
            if (tangent) {
                ENGINE_CALL(*eng, get_tangent, get_tangent, F(o_tangent));
                const double now = eng->tangent_norm(d_norm);                          // (waits for the compute stream: one host round trip per record)
                double *growth = (double *)outs[o_growth].host[set];
                growth[0] = (double)step * cfg.dt; growth[1] = now; growth[2] = tg_sum + 0.5 * std::log(now / tg_norm_ref);
            }
            if (cfg.dump_census) {
                const float *w = !cfg.census_ow ? F(o_vort) : cfg.dump_ow ? F(o_ow) : d_census_w;
                if (d_census_w) ENGINE_CALL(*eng, get_okubo_weiss, get_okubo_weiss_local, d_census_w, nullptr);
                ENGINE_CALL(*eng, census, census, w, F(o_vort), cfg.census_below ? FB_CENSUS_BELOW : FB_CENSUS_ABOVE, cfg.census_thr, cfg.census_min, cfg.census_max,
                            D(o_census), d_census_count, nullptr);
            }
            if (o_budget >= 0 && lead) ENGINE_CALL(*eng, forcing_budget, forcing_budget, (double *)outs[o_budget].host[set]);     // (waits for the compute stream)
            eng->record(e_rec);
            must(fb_stream_wait_event(copy, e_rec), "wait");
            h0 = std::chrono::steady_clock::now();
            for (const Output &o : outs) if (o.dev && o.host[set]) must(fb_memcpy_d2h_async(copy, o.host[set], o.dev, o.bytes), "d2h");
            host_copy_s += since(h0);
            must(fb_event_record(writer.e_copy[set], copy), "record");
            last_set = set;
            writer.submit(job);
            stamp(t_beg);
        }
        if (cfg.recipe_type != EMPTY) {                                                // main-shallow-water.cpp:304
            const SourceFeed::Entry e = feed.read();
            if (e.status == 1) {
                must(fb_event_synchronize(e_h2d), "sync");                             // the buffer about to be given up has been uploaded
                feed.make_current(e.buf);
                must(fb_stream_wait_event(copy, e_src), "wait");                       // the previous set_source has read d_in
                must(fb_memcpy_h2d_async(copy, d_in, feed.pin[e.buf], floats * sizeof(float)), "h2d");
                must(fb_event_record(e_h2d, copy), "record");
                eng->wait(e_h2d);
                ENGINE_CALL(*eng, set_source, set_source_local, d_in);
                eng->record(e_src);
            }
        }
        eng->step();                                                                   // main.cpp:286-317
        if (tangent && cfg.tangent_renorm > 0 && (step + 1 - cfg.start_step) % cfg.tangent_renorm == 0) {       // back to the initial norm
            const double now = eng->tangent_norm(d_norm);
            tg_sum += 0.5 * std::log(now / tg_norm_ref);
            ENGINE_CALL(*eng, tangent_scale, tangent_scale, (float)std::sqrt(tg_norm0 / now));
            tg_norm_ref = eng->tangent_norm(d_norm);
        }
    }
    stamp(t_end);
    eng->sync();                                                                       // the last step has run ...
    const auto compute_done = std::chrono::steady_clock::now();
    writer.stop();                                                                     // ... and now the last record's files are on their way
    const bool feed_done = feed.shutdown();
    must(fb_stream_synchronize(copy), "sync");
    if (timing) {
        const auto wall1 = std::chrono::steady_clock::now();
        const double wall_s = std::chrono::duration<double>(wall1 - wall0).count();
        const double tail_s = std::chrono::duration<double>(wall1 - compute_done).count();
        double gpu_ms = 0.0, rec_ms = 0.0;
        for (size_t k = 0; k < t_beg.size() && k < t_end.size(); ++k) { float ms = 0.0f; must(fb_event_elapsed_ms(t_beg[k], t_end[k], &ms), "elapsed"); gpu_ms += ms; }
        // what lies BETWEEN the stretches on the compute stream: a record branch from its first event to the one behind its record kernels,
        // i.e. those kernels plus whatever time the stream sat idle while the host was inside the branch (waiting for the writer, enqueueing)
        for (size_t k = 0; k + 1 < t_beg.size() && k < t_end.size(); ++k) { float ms = 0.0f; must(fb_event_elapsed_ms(t_end[k], t_beg[k + 1], &ms), "elapsed"); rec_ms += ms; }
        for (void *e : t_beg) fb_event_destroy(e);
        for (void *e : t_end) fb_event_destroy(e);
        if (lead) {
            const int steps = cfg.total_steps - cfg.start_step;
            const double rate = steps / (gpu_ms * 1e-3), gbs = 320.0 * N * (double)N * rate / 1e9, peak = 8000.0 * P;    // B_alg = 320 N^2 per step; HBM3E 8 TB/s per GPU
            fprintf(stderr, "[timing] %d RK4 steps, %d x %d grid, %d GPU%s: step loop without the record steps %.1f steps/s (%.4f ms/step) = %.0f GB/s by 320 N^2 B/step = %.3f of %.0f GB/s\n",
                    steps, N, N, P, P > 1 ? "s" : "", rate, gpu_ms / steps, gbs, gbs / peak, peak);
            fprintf(stderr, "[timing] with %d record steps (%.3f GB written%s): %.1f steps/s over %.3f s of wall time; the writer thread was busy %.3f s = %.2f GB/s to %s\n",
                    n_records, writer.bytes * (double)(P > 1 && !cfg.threads ? P : 1) / 1e9, P > 1 && !cfg.threads ? ", all ranks" : (P > 1 ? ", this rank" : ""), steps / wall_s, wall_s, writer.busy_s,
                    writer.busy_s > 0 ? writer.bytes / writer.busy_s / 1e9 : 0.0, cfg.output.c_str());
            // where the difference between the two rates goes, measured rather than guessed
            fprintf(stderr, "[timing] of those %.3f s: %.3f s stepping, %.3f s with a record step holding the compute stream (record kernels + idle while the host was in the record branch), "
                            "%.3f s between the last step's end and the last file (writer tail), %.3f s unaccounted (loop start-up, event bookkeeping)\n",
                    wall_s, gpu_ms * 1e-3, rec_ms * 1e-3, tail_s, wall_s - gpu_ms * 1e-3 - rec_ms * 1e-3 - tail_s);
            // The host runs a stretch ahead of the GPU and then waits here for the previous record's files; the compute stream only runs dry
            // when ONE record's files take longer than the stretch between two records minus its D2H copies (the slowest record tells).
            fprintf(stderr, "[timing] host time inside the %d record branches: %.3f s waiting for a free set of record buffers (%d set%s), %.3f s enqueueing the record kernels, %.3f s in the D2H copy calls; "
                            "slowest record %.3f s to write, a stretch between records is %.3f s of stepping\n",
                    n_records, host_wait_s, writer.nsets, writer.nsets > 1 ? "s" : "", host_get_s, host_copy_s, writer.slowest_s, n_records > 0 ? gpu_ms * 1e-3 * cfg.record_step / steps : 0.0);
            fflush(stderr);
        }
    }
    if (feed_done) delete feedp;
    for (void *p : {(void *)d_in, (void *)d_census_count, (void *)d_census_w, (void *)d_norm}) if (p) fb_free(p);
    for (const Output &o : outs) {
        if (o.dev) fb_free(o.dev);
        for (int b = 0; b < writer.nsets; ++b) if (o.host[b]) fb_free_host(o.host[b]);
    }
    for (int b = 0; b < writer.nsets; ++b) fb_event_destroy(writer.e_copy[b]);
    delete eng;
    for (void *e : {e_rec, e_h2d, e_src}) fb_event_destroy(e);
    fb_stream_destroy(copy);
}

// the value of the option getopt_long has just returned (optarg): an integer in [lo, hi], or a number between lo (itself allowed where
// lo_ok) and hi, parsed as float where `single`; anything else, trailing characters included, ends the run with `msg` and exit status 2
static int int_option(long lo, long hi, const char *msg)
{
    char *end = nullptr;
    const long v = strtol(optarg, &end, 10);
    if (!*optarg || *end || v < lo || v > hi) { fprintf(stderr, "%s\n", msg); std::exit(2); }
    return (int)v;
}
static double real_option(bool single, double lo, bool lo_ok, double hi, const char *msg)
{
    char *end = nullptr;
    const double v = single ? (double)strtof(optarg, &end) : strtod(optarg, &end);
    if (!*optarg || *end || !(lo_ok ? v >= lo : v > lo) || v > hi) { fprintf(stderr, "%s\n", msg); std::exit(2); }
    return v;
}

int main(int argc, char *args[])
{
    // configuration.hpp:10-41 defaults (NPTS = 768, configuration.hpp:18)
    Config cfg;
    static struct option lopts[] = {{"npts", 1, 0, 1}, {"lx", 1, 0, 2}, {"ly", 1, 0, 3}, {"nu", 1, 0, 4}, {"dt", 1, 0, 5},
                                    {"steps", 1, 0, 6}, {"record-step", 1, 0, 7}, {"start-step", 1, 0, 8},
                                    {"world", 1, 0, 9}, {"rank", 1, 0, 10}, {"comm-file", 1, 0, 11}, {"ranks-as-threads", 0, 0, 12},
                                    {"launch-token", 1, 0, 13}, {"comm-max-age", 1, 0, 14}, {"comm-timeout", 1, 0, 15}, {"fifo-fanout", 0, 0, 16},
                                    {"no-timing", 0, 0, 17}, {"dump-grad-vort", 0, 0, 18}, {"dump-dvortdt", 0, 0, 19}, {"record-buffers", 1, 0, 20},
                                    {"dump-okubo-weiss", 0, 0, 21}, {"dump-eddy-diffusivity", 0, 0, 22}, {"keff-bins", 1, 0, 23},
                                    {"dump-pressure", 0, 0, 24}, {"pres-rho", 1, 0, 25}, {"pres-f", 1, 0, 26}, {"pres-ref-x", 1, 0, 27}, {"pres-ref-y", 1, 0, 28},
                                    {"dump-spectra", 0, 0, 29}, {"tracer", 1, 0, 30}, {"tracer-kappa", 1, 0, 31},
                                    {"dump-azimuthal", 0, 0, 32}, {"azim-center", 1, 0, 33}, {"azim-bins", 1, 0, 34}, {"azim-dr", 1, 0, 35}, {"azim-modes", 1, 0, 36},
                                    {"particles", 1, 0, 37}, {"tangent", 1, 0, 38}, {"tangent-renorm", 1, 0, 39},
                                    {"particle-deformation", 0, 0, 40},
                                    {"dump-census", 0, 0, 41}, {"census-threshold", 1, 0, 42}, {"census-field", 1, 0, 43}, {"census-below", 0, 0, 44},
                                    {"census-min-cells", 1, 0, 45}, {"census-max", 1, 0, 46},
                                    {"forcing-rate", 1, 0, 47}, {"forcing-k", 1, 0, 48}, {"forcing-width", 1, 0, 49}, {"forcing-seed", 1, 0, 50},
                                    {"drag", 1, 0, 51}, {"hyper-nu", 1, 0, 52}, {"hyper-order", 1, 0, 53},
                                    {0, 0, 0, 0}};
    int opt;
    while ((opt = getopt_long(argc, args, "I:O:i:s:f:", lopts, NULL)) != EOF) {      // main.cpp:68-80, main-shallow-water.cpp:75-95
        switch (opt) {
        case 'I': cfg.input = optarg; break;
        case 'O': cfg.output = optarg; break;
        case 'i': cfg.init_file = optarg; break;
        case 's': cfg.vort_src_filename = optarg; cfg.recipe_type = SCRIPT; break;
        case 'f': cfg.vort_src_filename = optarg; cfg.recipe_type = FIFO; break;
        case 1: cfg.npts = atoi(optarg); break;
        case 2: cfg.LX = (float)atof(optarg); break;
        case 3: cfg.LY = (float)atof(optarg); break;
        case 4: cfg.NU = (float)atof(optarg); break;
        case 5: cfg.dt = (float)atof(optarg); break;
        case 6: cfg.total_steps = atoi(optarg); break;
        case 7: cfg.record_step = atoi(optarg); break;
        case 8: cfg.start_step = atoi(optarg); break;    // restart: -i vort_step_N.bin --start-step N keeps file numbering and source timing
        case 9: cfg.world = atoi(optarg); break;
        case 10: cfg.rank = atoi(optarg); break;
        case 11: cfg.comm_file = optarg; break;
        case 12: cfg.threads = true; break;
        case 13: cfg.token = optarg; break;              // the same string on every rank of one launch (job id, start time)
        case 14: cfg.comm_max_age = atol(optarg); break;
        case 15: cfg.comm_timeout = atol(optarg); break;
        case 16: cfg.fanout = true; break;
        case 17: cfg.timing = false; break;
        case 18: cfg.dump_grad = true; break;            // main.cpp:156-162,170-176 (#ifdef OUTPUT_GRAD_VORT; configuration.hpp:4-5 defines only OUTPUT_PSI and OUTPUT_WIND)
        case 19: cfg.dump_dvortdt = true; break;
        case 20: cfg.record_buffers = atoi(optarg); break;         // main.cpp:229-235 (#ifdef OUTPUT_DVORTDT)
        case 21: cfg.dump_ow = true; break;              // okubo_weiss_step_N.bin, tau_fil_step_N.bin (also with --world P)
        case 22: cfg.dump_keff = true; break;            // eddy_diffusivity_step_N.bin (also with --world P)
        case 23: cfg.keff_bins = int_option(2, 4096, "--keff-bins: an integer in [2, 4096]"); break;
        case 24: cfg.dump_pres = true; break;            // pres_step_N.bin (also with --world P)
        case 29: cfg.dump_spectra = true; break;         // spectra_step_N.bin (also with --world P)
        case 30: cfg.tracer_file = optarg; break;       // tracer_step_N.bin (also with --world P)
        case 31: cfg.tracer_kappa = (float)real_option(true, 0.0, true, 3.0e38f, "--tracer-kappa: a finite number >= 0"); break;
        case 32: cfg.dump_azim = true; break;            // azimuthal_step_N.bin, azimuthal_center_step_N.bin (also with --world P)
        case 33: {
            const std::string a = optarg;
            char *e1 = nullptr, *e2 = nullptr;
            if (a == "psi-min") cfg.azim_mode = FB_CENTER_PSI_MIN;
            else if (a == "vort-max") cfg.azim_mode = FB_CENTER_VORT_MAX;
            else {
                cfg.azim_mode = FB_CENTER_FIXED;
                cfg.azim_xc = strtod(optarg, &e1);
                if (e1 != optarg && *e1 == ',') cfg.azim_yc = strtod(e1 + 1, &e2);
                if (!e2 || e2 == e1 + 1 || *e2) { fprintf(stderr, "--azim-center: psi-min, vort-max or X,Y\n"); return 2; }
            }
            break;
        }
        case 34: cfg.azim_bins = int_option(2, 4096, "--azim-bins: an integer in [2, 4096]"); break;
        case 36: cfg.azim_modes = int_option(0, 8, "--azim-modes: an integer in [0, 8]"); break;
        case 35: cfg.azim_dr = real_option(false, 0.0, false, 1.0e300, "--azim-dr: a finite number > 0"); break;
        case 37: cfg.particles_file = optarg; break;    // particles_step_N.bin (one GPU only)
        case 40: cfg.particle_deformation = true; break; // particle_deformation_step_N.bin, particle_stretching_step_N.bin (with --particles)
        case 38: cfg.tangent_file = optarg; break;      // tangent_step_N.bin, tangent_growth_step_N.bin (one GPU only)
        case 39: cfg.tangent_renorm = int_option(0, 0x7fffffffL, "--tangent-renorm: an integer >= 0"); break;
        case 41: cfg.dump_census = true; break;          // census_step_N.bin (one GPU only)
        case 42: cfg.census_thr = (float)real_option(true, -FLT_MAX, true, FLT_MAX, "--census-threshold: a finite number"); cfg.census_have_thr = true; break;
        case 43: {
            const std::string a = optarg;
            if (a != "vort" && a != "okubo-weiss") { fprintf(stderr, "--census-field: vort or okubo-weiss\n"); return 2; }
            cfg.census_ow = a == "okubo-weiss";
            break;
        }
        case 44: cfg.census_below = true; break;
        case 45: cfg.census_min = int_option(1, 1L << 30, "--census-min-cells: an integer in [1, 2^30]"); break;
        case 46: cfg.census_max = int_option(1, FB_CENSUS_MAX, "--census-max: an integer in [1, 65536]"); break;
        case 47: cfg.forcing_rate = real_option(false, 0.0, true, DBL_MAX, "--forcing-rate: a finite number >= 0"); break;     // forcing_budget_step_N.bin (one GPU only)
        case 48: cfg.forcing_k = real_option(false, 0.0, false, DBL_MAX, "--forcing-k: a finite number > 0"); break;
        case 49: cfg.forcing_width = real_option(false, 0.0, true, DBL_MAX, "--forcing-width: a finite number >= 0"); break;
        case 50: {
            char *end = nullptr;
            cfg.forcing_seed = strtoull(optarg, &end, 0);
            if (!*optarg || *end || *optarg == '-') { fprintf(stderr, "--forcing-seed: an integer in [0, 2^64)\n"); return 2; }
            break;
        }
        case 51: cfg.drag = real_option(false, 0.0, true, DBL_MAX, "--drag: a finite number >= 0"); break;
        case 52: cfg.hyper_nu = real_option(false, 0.0, true, DBL_MAX, "--hyper-nu: a finite number >= 0"); break;
        case 53: cfg.hyper_order = int_option(1, 8, "--hyper-order: an integer in [1, 8]"); break;
        case 25: cfg.pres_rho = (float)atof(optarg); break;
        case 26: cfg.pres_f = (float)atof(optarg); break;
        case 27: case 28:                                // invert_pres.cpp:71-79 (-x, -y)
            (opt == 27 ? cfg.pres_ref_x : cfg.pres_ref_y) = int_option(0, 0x7fffffffL, "--pres-ref-x / --pres-ref-y: a non-negative integer");
            break;
        }
    }
    if (cfg.world < 1 || cfg.rank < 0 || cfg.rank >= cfg.world || (cfg.world > 1 && !cfg.threads && cfg.comm_file.empty()) ||
        cfg.token.size() >= fbcomm::TOKEN_BYTES) {
        fprintf(stderr, "usage: ... --world P --rank r --comm-file FILE [--launch-token T]   (or --world P --ranks-as-threads)\n"); return 2;
    }
    // the reference's flat index ref_x + XPTS * ref_y (invert_pres.cpp:182) must name an element of the field
    if ((long long)cfg.pres_ref_x + (long long)cfg.npts * cfg.pres_ref_y >= (long long)cfg.npts * cfg.npts) {
        fprintf(stderr, "--pres-ref-x / --pres-ref-y: the reference point lies outside the %d x %d grid\n", cfg.npts, cfg.npts); return 2;
    }
    if (cfg.dump_azim) {                                                               // what fb_model_get_azimuthal would refuse, and the defaults
        const double lx = (double)cfg.LX, ly = (double)cfg.LY, ddx = lx / cfg.npts, ddy = ly / cfg.npts, half = (lx < ly ? lx : ly) / 2;
        if (!(ddx > 0.0) || !(ddy > 0.0)) { fprintf(stderr, "--dump-azimuthal: needs a positive domain and grid size\n"); return 2; }
        if (cfg.azim_dr == 0.0) cfg.azim_dr = ddx > ddy ? ddx : ddy;
        if (cfg.azim_bins == 0) {
            const double q = half / cfg.azim_dr;
            cfg.azim_bins = q >= 4096.0 ? 4096 : (int)q;
            while (cfg.azim_bins > 2 && cfg.azim_bins * cfg.azim_dr > half) --cfg.azim_bins;
        }
        if (cfg.azim_dr < (ddx < ddy ? ddx : ddy)) { fprintf(stderr, "--azim-dr: below min(dx, dy)\n"); return 2; }
        if (cfg.azim_bins < 2 || cfg.azim_bins * cfg.azim_dr > half) { fprintf(stderr, "--azim-bins / --azim-dr: need 2 <= bins and bins * dr <= min(Lx, Ly) / 2\n"); return 2; }
        if (cfg.azim_mode == FB_CENTER_FIXED && !(cfg.azim_xc >= 0.0 && cfg.azim_xc < lx && cfg.azim_yc >= 0.0 && cfg.azim_yc < ly)) {
            fprintf(stderr, "--azim-center: X,Y must lie inside the domain, 0 <= X < Lx and 0 <= Y < Ly\n"); return 2;
        }
    }
    if (cfg.particle_deformation) {                                                    // what fb_model_set_particle_deformation would refuse
        if (cfg.particles_file.empty()) { fprintf(stderr, "--particle-deformation: needs --particles FILE\n"); return 2; }
        if (cfg.world > 1) { fprintf(stderr, "--particle-deformation: one GPU only (particles are not supported with --world P > 1)\n"); return 2; }
    }
    if (!cfg.particles_file.empty()) {                                                 // what fb_model_set_particles would refuse
        if (cfg.world > 1) { fprintf(stderr, "--particles: one GPU only (particles are not supported with --world P > 1)\n"); return 2; }
        struct stat st;
        const std::string fn = cfg.input + "/" + cfg.particles_file;
        if (stat(fn.c_str(), &st) != 0 || st.st_size <= 0 || st.st_size % 16 != 0) {
            fprintf(stderr, "--particles: %s must hold float64 [n][2], a positive multiple of 16 bytes\n", fn.c_str()); return 2;
        }
        if (st.st_size / 16 > (off_t)(1 << 24)) { fprintf(stderr, "--particles: more than 2^24 particles\n"); return 2; }
        cfg.n_particles = (int)(st.st_size / 16);
    }
    if (cfg.dump_census) {                                                             // what fb_model_census would refuse
        if (!cfg.census_have_thr) { fprintf(stderr, "--dump-census: needs --census-threshold T\n"); return 2; }
        if (cfg.world > 1) { fprintf(stderr, "--dump-census: one GPU only (the vortex census is not supported with --world P > 1)\n"); return 2; }
    }
    if (cfg.forcing() && cfg.world > 1) { fprintf(stderr, "--forcing-rate / --drag / --hyper-nu: one GPU only (the stochastic forcing is not supported with --world P > 1)\n"); return 2; }
    if (cfg.forcing_rate > 0.0 && !(cfg.forcing_k - cfg.forcing_width > 0.0)) { fprintf(stderr, "--forcing-rate: needs --forcing-k K and --forcing-width W with K - W > 0\n"); return 2; }
    if (!cfg.tangent_file.empty() && cfg.world > 1) { fprintf(stderr, "--tangent: one GPU only (the tangent-linear model is not supported with --world P > 1)\n"); return 2; }
    if ((cfg.dump_grad || cfg.dump_dvortdt) && cfg.world > 1) { fprintf(stderr, "--dump-grad-vort / --dump-dvortdt: one GPU only\n"); return 2; }
    if (cfg.total_steps < 0) cfg.total_steps = (int)(60 * 60 / cfg.dt);              // configuration.hpp:36
    float dx = 0, dy = 0;                                                            // printed before being set, main.cpp:89-90

    const bool lead = cfg.world == 1 || cfg.threads || cfg.rank == 0;                  // the rank that owns the banner, stdout's step lines and ./log
    if (cfg.world > 1 && !cfg.threads) {                                              // one process per GPU: rank r on device r mod (visible devices)
        int ndev = 0;
        must(fb_device_count(&ndev), "fb_device_count");
        if (ndev > 0) must(fb_set_device(cfg.rank % ndev), "fb_set_device");
    }
    if (lead) {
    printf("##### Model setting #####\n");
    printf("Initial file          : %s \n", cfg.init_file.c_str());
    printf("Input folder          : %s \n", cfg.input.c_str());
    printf("Output folder         : %s \n", cfg.output.c_str());
    printf("Length X              : %.3f [m]\n", cfg.LX);
    printf("Length Y              : %.3f [m]\n", cfg.LY);
    printf("Spatial Resolution dx : %.3f [m]\n", dx);
    printf("Spatial Resolution dy : %.3f [m]\n", dy);
    printf("Time Resolution dt    : %.3f [s]\n", cfg.dt);
    printf("#########################\n\n\n");
    printf("Start project.\n");
    }

    FILE *log_fd = lead ? fopen("log", "w") : fopen("/dev/null", "w");                // main.cpp:97
    if (log_fd == NULL) { perror("Open log file"); return 1; }
    std::thread fan;
    if (cfg.fanout && cfg.world > 1 && cfg.recipe_type == FIFO && lead) fan = std::thread(fifo_fanout, cfg);
    if (cfg.world > 1 && cfg.threads) {
        void *hub = nullptr;
        must(fb_local_hub_create(&hub, cfg.world), "fb_local_hub_create");
        std::vector<std::thread> ts;
        for (int r = 0; r < cfg.world; ++r) ts.emplace_back([&, r] { run_rank(cfg, r, hub, log_fd, r == 0); });
        for (auto &t : ts) t.join();
        fb_local_hub_destroy(hub);
    } else run_rank(cfg, cfg.rank, nullptr, log_fd, lead);
    if (fan.joinable()) fan.detach();                                                // (a producer that outlives the run keeps it inside fread)
    fclose(log_fd);
    if (lead) printf("Program ends. Congrats!\n");
    return 0;
}
