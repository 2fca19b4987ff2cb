// uf3_hip.hip -- C ABI (include/uf3_hip.h) of the MI355X-native UF3 hot path:
// contexts, device-resident basis tables, per-call frame geometry, kernel launches.
#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <thread>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/uf3_hip.h"
#include "uf3_kernels.h"
#include "uf3_feat3.h"
#include "uf3_virial_rows.h"
#include "uf3_leverage.h"
#include "uf3_md.h"
#include "uf3_ti.h"
#include "uf3_npt.h"
#include "uf3_hessian.h"
#include "uf3_relax.h"
#include "uf3_neb.h"
#include "uf3_idpp.h"
#include "uf3_mc.h"
#include "uf3_phonon.h"
#include "uf3_flux.h"
#include "uf3_site_rows.h"
#include <chrono>
#include <dlfcn.h>

// ------------------------------------------------------------------------------ plumbing
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    bool fine = false;          // fine-grained device memory (ensure_fine): the host may store into it through the BAR
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        fine = false;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    hipError_t ensure_fine(size_t bytes) {
        if (bytes <= cap && fine) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        fine = false;
        size_t want = std::max(bytes, cap) + bytes / 4 + 256;
        hipError_t e = hipExtMallocWithFlags(&p, want, hipDeviceMallocFinegrained);
        if (e == hipSuccess) { cap = want; fine = true; }
        return e;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

struct DevBuf : Buf {                           // a buffer that a driver or a basis owns: freed with its owner
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
};
template <class T>
struct DevTable : DevBuf {                      // ... read as the table of T it holds
    operator T *() const { return as<T>(); }
};

// grow-only pinned host memory: small transfers go through it so that they are true asynchronous copies (a copy
// from / to pageable caller memory is staged by the runtime and waits)
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) hipHostFree(p);
        p = nullptr; cap = 0;
        size_t want = std::max(bytes, (size_t)4096);
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocCoherent);   // (fine-grained: kernels read and write these blocks in flight)
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) hipHostFree(p); p = nullptr; cap = 0; }
};
// workspace of the per-atom image lists (k_flux_lists): frame table, species, the model's copy, counts and entries; the site
// records (u, jp: site terms and heat current only) and the host entries' staging block.  One per user -- the context's
// Hessian entries, its site-term entries, each MD state -- and nothing in it shared.
struct ListWork {
    Buf frames, offsets, spec, cnt, ent, coeff, flags, u, jp, io;
    int cap = 0;                        // list capacity per atom (an MD state keeps it from sample to sample)
    void release() { for (Buf *b : {&frames, &offsets, &spec, &cnt, &ent, &coeff, &flags, &u, &jp, &io}) b->release(); cap = 0; }
};

// One device block of a synchronous host entry (uf3_hessian, uf3_site_terms, uf3_heat_flux, uf3_phonon_mesh / _dos / _thermo,
// uf3_gram, uf3_leverage), cut into sections in the order they are declared.  add() every section (present = false: an optional
// the caller did not pass), alloc(), then at<T>() is a section's device pointer (null when absent), in() queues uploads, and
// out() queues the downloads of the outputs that were asked for and is the call's one hipStreamSynchronize.  Offsets and the
// 16-byte alignment of the sections are computed here and nowhere else.
// Not for upload_frames and the entries built on it (uf3_featurize*, uf3_eval*, uf3_pair_histogram): their BAR / pinned /
// deferred staging is what bench.py measures and has invariants of its own (pin_in_busy, staged_in_dev).  Not for the drivers'
// *_get_state either: those copy out of the state's own buffers.
struct Stage {
    enum { MAX_SECTIONS = 8 };
    Buf &buf;
    hipStream_t st;
    size_t off[MAX_SECTIONS], len[MAX_SECTIONS], total = 0;
    bool here[MAX_SECTIONS];
    int n = 0;
    Stage(Buf &b, hipStream_t s) : buf(b), st(s) {}
    int add(size_t bytes, bool present = true) {
        if (n == MAX_SECTIONS) { fprintf(stderr, "uf3: Stage: more than %d sections\n", (int)MAX_SECTIONS); abort(); }
        off[n] = total; len[n] = present ? bytes : 0; here[n] = present;
        total += (len[n] + 15) / 16 * 16;
        return n++;
    }
    hipError_t alloc() { return buf.ensure(total); }
    template <class T> T *at(int s) const { return here[s] ? (T *)((char *)buf.p + off[s]) : nullptr; }
    struct Copy { int s; const void *host; };
    hipError_t copy(std::initializer_list<Copy> l, bool up) const {
        for (const Copy &k : l) {
            if (!k.host || !len[k.s]) continue;
            void *d = at<char>(k.s), *h = (void *)k.host;
            hipError_t e = up ? hipMemcpyAsync(d, h, len[k.s], hipMemcpyHostToDevice, st) : hipMemcpyAsync(h, d, len[k.s], hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return up ? hipSuccess : hipStreamSynchronize(st);
    }
    hipError_t in(std::initializer_list<Copy> l) const { return copy(l, true); }
    hipError_t out(std::initializer_list<Copy> l) const { return copy(l, false); }
};
#define UF3_PIN_LIMIT (512 * 1024)   // bytes: larger transfers go straight from / to the caller's memory
#define UF3_BAR_LIMIT (128 * 1024)   // bytes: largest block the host stores into device memory itself (beyond it the copy engine is quicker)

struct uf3_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    int lds_max = 65536;
    int n_cu = 256;
    // grow-only workspace
    Buf geoms, offsets, frame_of, atom_bin, atom_wrap, spec, key_in, key_out, val_in, val_out, sort_tmp,
        bin_start, slots, flags,
        n3_cnt, n3_int, n3_dbl, e_atom, nbr_f, coeff, stage_pos, stage_z, stage_out, stage_out2,
        gram_tiles[UF3_MAX_SPECIES + 1], gram_tij, frag, dbg,
        sp_rows, sp_seg,                // force rows by species (uf3_gram_force_rows_dev): row lists | segment starts, counts, cursors
        halo,                           // marks + index list of the halo atoms of a decomposed frame
        n3x_ent, n3x_off,               // extension lists (batches with atoms outside their cell; see N3Lists)
        bin_cnt,                        // atoms per cell-list bin (counting sort)
        part_sums,                      // per-workgroup energy / strain-derivative sums of the MD collection pass (see EvalArgs)
        hist_edges, hist_noise,         // uf3_pair_histogram[_dev]: the caller's bin edges and supercell noise
        hs_part, hs_io,                 // uf3_hessian[_dev]: the row atoms' Born shares | host staging
        ph_ws, ph_part, ph_io;          // uf3_phonon_*: sorted terms and small inputs | smearing partials | host staging
    ListWork hs,                        // uf3_hessian[_dev]: its frame's lists and model copy (a call returns with work queued on them;
                                        // its u, jp and io stay empty: the Hessian has no site records and stages in hs_io)
             fx;                        // uf3_site_terms / uf3_heat_flux / uf3_site_rows / uf3_site_grade: theirs, the site records
                                        // and the host staging
    Buf site_rows_ws, site_off;         // uf3_site_grade: the fall-back's chunk of rows (bounded) | the caller's frame offsets
    std::vector<char> ph_stage;         // host image of ph_ws (kept alive behind the asynchronous copy)
    int n3_cap = 0, cand_cap = 0;
    size_t bin_cnt_clean = 0;        // ints of bin_cnt known to be zero (k_bin_fill leaves the counts it used at zero)
    int n3_last_cap = 0, n3_last_natoms = 0;   // layout of the 3-body lists in the workspace right now (uf3_n3_lists_debug)
    int n3x_cap = 0;                 // capacity of the extension lists (0 until a batch needed them)
    bool img_mode = false;           // a batch with atoms far outside their cell has been seen: 3-body launches with the image-range rule
    int gram_plan_np[UF3_MAX_SPECIES + 1] = {0}, gram_plan_blocks[UF3_MAX_SPECIES + 1] = {0}, gram_plan_next = 0;   // workgroup plans of k_gram_tiled held in
                                                     // gram_tiles[] (each for this many 64-column ranges; 0: none)
    int gram_direct_feat = 0;                        // tile-pair table of k_gram_mfma held in gram_tij (for this n_feat; 0: none)
    hipEvent_t sp_done = nullptr;                    // recorded behind the last launch that read sp_rows / sp_seg (on whichever stream)
    bool sp_done_live = false;
    bool n3_tuned = false;           // capacity re-sized once to the lists actually seen
    bool cand_tuned = false;         // a featurizer call has completed with the current candidate capacity
    // status words of asynchronous featurizer calls: copied to pinned slots behind the launches, looked at later
    struct Pending { hipEvent_t ev = nullptr; int cap = 0, cand = 0, xcap = 0; bool has3 = false, img = true, img_launch = false, live = false;
                     bool virial = false;      // the call wrote virial rows (uf3_featurize_virial_dev): atoms far outside their cell are refused
    };
    enum { N_PENDING = 16 };
    Pending pending_chk[N_PENDING];
    PinBuf pin_flags;                // [N_PENDING][8] ints
    int pending_head = 0;
    // A bad verdict on an asynchronous call belongs to whoever synchronises the context next, not to whichever entry happens to
    // poll first: it is remembered here until uf3_ctx_synchronize has reported it (the entries that meet it on the way still
    // return it once, so an asynchronous loop stops early).
    int async_bad = 0;
    std::string async_msg;
    bool frag_ready = false;
    int32_t *d_stage_z = nullptr;       // species of the staged batch (tail of stage_pos)
    // small MD steps without a fetch kernel: with a large BAR the host stores positions | species straight into a (fine-grained)
    // device block -- no launch that reads the caller's pinned block, no dispatch gap behind a 4 us kernel (eval_impl, MD route)
    bool bar_ok = false;
    bool bar_tested = false;            // bar_self_test has run on this context (it decides bar_ok once, at the first small batch)
    Buf stage_bar;                      // the fine-grained block of small batches (upload_frames)
    char *stage_cur = nullptr;          // the block that holds the current host-entry batch: stage_bar or stage_pos
    size_t staged_in_dev = 0;           // bytes of positions | species the host entry has stored into stage_pos already (0: none)
    // environment switches of the featurizer's asynchronous path, re-read at the top of every featurizer call (read_f3_env)
    bool env_no_feat3 = false, env_debug_lds = false;
    unsigned eval_seq = 0;              // sequence number of the last small evaluator call whose tail kernel signals through the pinned block
    bool tail_signalled = false;        // ... and whether the last eval_impl's k_frame_sum signals
    bool pin_in_busy = false;           // a kernel that reads pin_in directly has been launched and not yet waited for
    size_t pin_in_pending = 0;          // small batch: bytes of positions | species waiting in pin_in; the cell-list
                                        // stage appends the frame geometry and sends everything in ONE copy
    PinBuf pin_in, pin_geo, pin_out;    // positions + species | frame geometry + offsets | results
    PinBuf pin_eval;                    // device-resident evaluator calls: status words [4] | sequence number, written by the last kernel
    hipEvent_t pin_in_done = nullptr, pin_geo_done = nullptr;   // the copies out of pin_in / pin_geo have executed
    std::vector<double> coeff_shadow;   // host copy of the model last uploaded by uf3_eval (c1 | c2 | c3)
    Buf coeff_cw;                       // window table of that model's 3-body coefficients (k_eval<..., CW>), when cw_of is its basis
    const void *cw_of = nullptr;        // the basis the table in coeff_cw was built for (null: none -- coefficients outside the window)
    const void *coeff_dev = nullptr;    // ... and where it lives
    // MD route of the evaluator (uf3_ctx_md_skin): persistent superset lists with a skin, see k_build_sup.  Everything a step
    // needs besides the current positions lives in its own buffers -- the workspace above belongs to whichever call ran last
    struct MdState {
        bool cap_tuned = false;         // the list capacity has held in a build the host looked at
        bool verify_next = false;       // the last step was discarded: the next build waits for its own report
        bool flags_clean = false;       // the status words [1..3] are known to be zero (the last call was an MD step that set none)
        double skin = 0.0;              // 0: off
        bool valid = false;             // the lists describe (basis, offsets, cells, pbc) below
        bool stale = false;             // some atom has passed the early-warning displacement: rebuild before the next step
        const uf3_basis *basis = nullptr;
        int natoms = 0, n_frames = 0, cap = 0;
        std::vector<int64_t> offsets;
        std::vector<double> cells;
        std::vector<uint8_t> pbc;
        Buf ent, cnt, pos_ref, geo, frame_of, spec;       // geo: FrameGeom [n_frames] | atom offsets [n_frames + 1]
        Buf inbox, surv, mark;                            // see EvalArgs::md_inbox / md_surv / md_mark
        size_t inbox_zeroed = 0;                          // bytes of inbox known to hold no stamp of a future launch
        size_t geo_bytes = 0;
        long long builds = 0, steps = 0, redone = 0;
        // "the cells live on the device" (uf3_md_run_npt alone sets it, for its own duration): the integrator keeps the current
        // cells in live_dev [n_frames][9] and in `geo`; the key does not compare cells, and the host copy live_host (what the
        // caller's uf3_frames points at) is refreshed only in front of a list build
        bool live = false;
        const double *live_dev = nullptr;
        double *live_host = nullptr;
        // a wrapping MD object (uf3_md_set_wrap) arms this for each of its evaluations: called with the positions in front of
        // every list build (md_build) and in front of every evaluation on the rebuild-everything route, it folds them into the
        // cell (k_md_wrap) -- never between a build and the steps on its lists.  Empty: nothing wraps
        std::function<int(const double *)> wrap;
    } md;
    // RCCL communicator of this rank (uf3_comm_init): the library is opened at run time (no link dependency), see rccl_api()
    void *comm = nullptr;
    int comm_ranks = 0, comm_rank = -1;
    bool md_step = false;               // the last eval_impl ran on the persistent lists (its status words 2 / 3 are the displacement flags)
    // timing
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double t_feat = 0, t_nbr = 0, t_gram = 0, t_eval = 0;
    long long n_feat_launch = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[4];
};

// What uf3_basis_create decides about a basis besides its tables (basis_plan, below): the facts the launches read.  A BasisPlan is
// these facts plus the host image of every table; a uf3_basis is these facts plus the device copies of the tables, which it owns.
struct BasisFacts {
    BasisDev host;              // host mirror (in a plan: its three device pointers null)
    size_t n_gsrc = 0;
    bool all_grouped7 = false;       // every mode-7 trio stages grouped windows (its force launches do not touch dsrc)
    bool all_banded9 = false;        // every mode-9 trio runs banded (trio_block_banded) with its bands on the column tiles 0, 1, 2
    size_t n_dsrc = 0;
    int sp_ncols[UF3_MAX_SPECIES] = {0};
    std::vector<int> block_bounds;   // column boundaries of interaction blocks (for column windows)
    size_t c2_len = 0, c3_len = 0, n_recs = 0;
    size_t n_pair_recs = 0;
    size_t trio_rec_lo = 0;          // first knot record a trio leg refers to
    size_t wrow_lo = 0;              // where the window rows of the grouped layouts start (they follow the knot records)
    int n_wrows = 0;                 // ... and how many there are
    int dense_stride[16] = {0};      // per featurizer mode: largest staged-record stride (doubles) among its trios
    int dense_stride_f[16] = {0};    // ... when force rows are wanted (grouped 3 x 3 x 9 windows stage 32-double records)
    bool dense_grouped[16] = {false}; // a trio of the mode stages grouped n windows (even-aligned groups: up to two padding records per pass)
    int dense_dump[16] = {0};        // ... smallest stage (doubles) the fold of its widest window needs
    int modes = 1;                   // bit m set: some trio block is handled by featurizer specialisation m
    int vmodes = 0;                  // bit m set (1 .. 5): some trio block is handled by instance m of k_virial_rows
    double r_cut = 0;
    // k_featurize3 (3-body force rows by bond factorisation, uf3_feat3.h): eligibility and tables
    bool feat3_ok = false;
    bool eval_tab_ok = false;        // the evaluator's centre pass may run its TAB instances (see k_eval)
    // k_eval<..., CW>: the coefficients inside the kept-bin window of the centre legs as a table for LDS (EvalArgs::c3w)
    bool eval_cw_ok = false;         // one window on every trio, centre legs alike, table + zero run small enough
    int cw_lo = 0, cw_ext = 0, cw_dim_m = 0, cw_dim_n = 0, cw_zero = 0, cw_bytes = 0;
    std::vector<int> cw_lut_off;     // per trio: where its full grid starts in c3
    std::vector<int> cw_dim_l;
    int n_f3rows = 0;
    int n_f3src = 0;
    Feat3Leg f3_leg_p{}, f3_leg_n{};
    int f3_lo_p = 0, f3_ext_p = 0, f3_lo_n = 0, f3_ext_n = 0;
    int f3_nr = 0;                   // rounds of 32 window positions of the launch that serves the window (1: default trims; 2, 3: wider)
};

struct uf3_basis : BasisFacts {
    uf3_ctx *ctx = nullptr;
    DevTable<BasisDev> dev;
    DevTable<TrioDev> d_trios;
    DevTable<KnotRec> d_recs;
    DevTable<int> d_lut;
    DevTable<int> d_colsrc;
    DevTable<int> d_dsrc;            // colsrc as offsets into the dumped dense window (MFMA specialisation)
    DevTable<unsigned short> d_gsrc; // grouped windows: fold tables (FeatArgs::gsrc)
    DevTable<int> d_sp_cols;         // [S][F]: the columns of the blocks species s takes part in, ascending (uf3_gram_force_rows_dev)
    DevTable<double> d_f3rows;       // k_featurize3: window rows of the centre legs and of leg n
    DevTable<unsigned short> d_f3src; // ... fold tables
    DevTable<int> d_f3off;           // ... [T] a trio's table
};

// ------------------------------------------------------------------------------ environment switches
// The UF3_* switches (A/B measurements, tests) are looked at on every call -- tests flip them between two calls on one context --
// but not through ~25 getenv scans per call: the entries of the hot paths call uf3_env_refresh(), which walks `environ` once when
// its fingerprint (the entries' addresses: setenv / unsetenv change them) has moved and keeps the UF3_* entries; uf3_env() then
// answers from those few (none at all in production).
extern char **environ;
struct Uf3EnvCache { unsigned long long print = ~0ull; std::vector<std::pair<std::string, std::string>> vars; };
static thread_local Uf3EnvCache g_env;
static void uf3_env_refresh() {
    unsigned long long fp = 1469598103934665603ull;
    for (char **e = environ; e && *e; e++) fp = (fp ^ (unsigned long long)(uintptr_t)*e) * 1099511628211ull;
    if (fp == g_env.print) return;
    g_env.print = fp;
    g_env.vars.clear();
    for (char **e = environ; e && *e; e++) {
        if (std::strncmp(*e, "UF3_", 4)) continue;
        const char *eq = std::strchr(*e, '=');
        if (eq) g_env.vars.emplace_back(std::string(*e, eq - *e), std::string(eq + 1));
    }
}
static const char *uf3_env(const char *name) {
    if (g_env.print == ~0ull) uf3_env_refresh();
    for (const auto &kv : g_env.vars)
        if (kv.first == name) return kv.second.c_str();
    return nullptr;
}

// host stores into device memory through the BAR are write-combined: drain them before the launch that reads them is queued
static inline void uf3_store_fence() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_sfence();
#else
    __sync_synchronize();
#endif
}

static thread_local std::string g_err;
static int fail(uf3_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    g_err = msg;
    return code;
}
#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess)                                                                    \
            return fail(ctx, UF3_EHIP, std::string(#call) + ": " + hipGetErrorString(e__));       \
    } while (0)

extern "C" const char *uf3_last_error(const uf3_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }
#ifndef UF3_BUILD_ID
#define UF3_BUILD_ID "unknown"
#endif
extern "C" const char *uf3_build_id(void) { return UF3_BUILD_ID; }

// ------------------------------------------------------------------------------ launch helpers
// More than the default 64 KB of dynamic LDS has to be asked for, and the answer belongs to the kernel instance on a device, not
// to a context or a thread: one process-wide high-water mark per instance and device that only grows -- ADVICE round 5.  Every
// launch whose dynamic LDS can pass 64 KB asks here, nowhere else.  Within the mark no lock is taken; raising it takes a mutex.
template <auto Kernel>
static hipError_t lds_opt_in(int device, size_t lds) {
    static std::mutex mu;
    static std::atomic<size_t> have[64];
    std::atomic<size_t> &hv = have[device & 63];
    if (lds <= hv.load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lk(mu);
    if (lds > hv.load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hv.store(lds, std::memory_order_release);
    }
    return hipSuccess;
}
// ... and the launch behind it, on the context's stream
template <auto Kernel, typename... Args>
static hipError_t launch_lds(const uf3_ctx *c, dim3 grid, dim3 block, size_t lds, const Args &...args) {
    hipError_t e = lds_opt_in<Kernel>(c->device, lds);
    if (e == hipSuccess) hipLaunchKernelGGL(Kernel, grid, block, lds, c->stream, args...);
    return e;
}

// Run-time values as template arguments: f is a generic lambda that takes the value as a std::integral_constant and returns a
// status.  f is instantiated for every value offered, so a caller offers only the values that have a kernel instance (or
// discards the others with `if constexpr`): the library holds the instances the dispatch names and no others.
template <typename F>
static int with_bool(bool v, F &&f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <int... Is, typename F>
static int with_int(int v, std::integer_sequence<int, Is...>, F &&f) {      // (the last value is the default arm, as in a switch)
    constexpr int vals[] = {Is...}, last = vals[sizeof...(Is) - 1];
    int rc = UF3_OK;
    (void)(((v == Is || Is == last) && ((rc = f(std::integral_constant<int, Is>{})), true)) || ...);
    return rc;
}

// The shape the featurizer's three stages (k_featurize, k_featurize3, k_virial_rows) share: workgroups of WPB waves, each walking a
// contiguous run of atoms (keeps the shared energy row on one frame); many more workgroups than resident slots -- 24 per slot
// (measured: 2 per slot 3400 frames/s, 16-48 per slot 3640, finer again slower): the tail of the launch is short and concurrent
// workgroups work on nearby atoms
struct AtomGrid { int atoms_per_block, n_blocks; unsigned grid; };      // grid: n_blocks in whole rounds over the 8 XCDs
static AtomGrid atom_grid(int natoms, size_t lds, int n_cu) {
    const int per_cu = std::max(1, std::min(8, (int)((size_t)(160 * 1024) / lds)));
    int n_blocks = std::min((natoms + WPB - 1) / WPB, n_cu * per_cu * 24);
    const int apb = ((natoms + n_blocks - 1) / n_blocks + WPB - 1) / WPB * WPB;
    n_blocks = (natoms + apb - 1) / apb;
    return {apb, n_blocks, (unsigned)((n_blocks + 7) / 8 * 8)};      // (surplus workgroups find no atoms)
}

// the featurizer's switches, re-read on every call (uf3_env is a look-up in the cached UF3_* entries; tests and A/B runs flip
// them between calls on one shared context -- ADVICE round 5)
static void read_f3_env(uf3_ctx *c) {
    c->env_no_feat3 = uf3_env("UF3_NO_FEAT3") != nullptr;
    c->env_debug_lds = uf3_env("UF3_DEBUG_LDS") != nullptr;
}

extern "C" int uf3_ctx_create(int device, uf3_ctx **out) {
    uf3_env_refresh();
    if (!out) return fail(nullptr, UF3_EINVAL, "uf3_ctx_create: null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, UF3_EHIP, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, UF3_EINVAL, "uf3_ctx_create: bad device index");
    uf3_ctx *c = new uf3_ctx();
    c->device = device;
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIPCHK(c, hipEventCreateWithFlags(&c->pin_in_done, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->pin_geo_done, hipEventDisableTiming));
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, device));
    c->lds_max = (int)prop.sharedMemPerBlock;
    c->n_cu = prop.multiProcessorCount;
    read_f3_env(c);
    { int large = 0; c->bar_ok = hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, device) == hipSuccess && large && !uf3_env("UF3_NO_BAR_STAGE"); }
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        std::string m = std::string("uf3_hip is built for gfx950 only, device is ") + prop.gcnArchName;
        delete c;
        return fail(nullptr, UF3_EHIP, m);
    }
    *out = c;
    return UF3_OK;
}

extern "C" int uf3_comm_destroy(uf3_ctx *c);
extern "C" void uf3_ctx_destroy(uf3_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    Buf *all[] = {&c->geoms, &c->offsets, &c->frame_of, &c->atom_bin, &c->atom_wrap, &c->spec, &c->key_in,
                  &c->key_out, &c->val_in, &c->val_out, &c->sort_tmp, &c->bin_start, &c->slots, &c->flags, &c->n3_cnt, &c->n3_int, &c->n3_dbl, &c->e_atom, &c->nbr_f, &c->coeff,
                  &c->stage_pos, &c->stage_z, &c->stage_out, &c->stage_out2, &c->sp_rows, &c->sp_seg, &c->gram_tij, &c->frag, &c->dbg, &c->halo, &c->n3x_ent, &c->n3x_off,
                  &c->bin_cnt, &c->coeff_cw, &c->part_sums,
                  &c->hs_part, &c->hs_io,
                  &c->ph_ws, &c->ph_part, &c->ph_io};
    for (Buf *b : all) b->release();
    for (Buf &b : c->gram_tiles) b.release();
    c->hs.release(); c->fx.release();
    if (c->comm) uf3_comm_destroy(c);
    { Buf *mdb[] = {&c->md.ent, &c->md.cnt, &c->md.pos_ref, &c->md.geo, &c->md.frame_of, &c->md.spec, &c->md.inbox, &c->md.surv, &c->md.mark}; for (Buf *b : mdb) b->release(); }
    c->stage_bar.release();
    c->pin_in.release(); c->pin_geo.release(); c->pin_out.release(); c->pin_flags.release(); c->pin_eval.release();
    for (auto &pd : c->pending_chk) if (pd.ev) hipEventDestroy(pd.ev);
    if (c->pin_in_done) hipEventDestroy(c->pin_in_done);
    if (c->sp_done) hipEventDestroy(c->sp_done);
    if (c->pin_geo_done) hipEventDestroy(c->pin_geo_done);
    for (auto &v : c->pending) for (auto &p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" int uf3_ctx_set_stream(uf3_ctx *c, void *s) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    c->stream = (hipStream_t)s;     // NULL is HIP's null stream (what torch's default stream is)
    return UF3_OK;
}

extern "C" int uf3_ctx_use_own_stream(uf3_ctx *c) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    c->stream = c->own_stream;
    return UF3_OK;
}

static int check_flags(uf3_ctx *c);
static int poll_pending(uf3_ctx *c, bool wait, bool remember = true);

extern "C" int uf3_ctx_synchronize(uf3_ctx *c) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    poll_pending(c, true);                           // (whatever it finds is remembered in async_bad)
    if (c->async_bad) {
        const int rc = c->async_bad;
        const std::string msg = c->async_msg;
        c->async_bad = 0; c->async_msg.clear();
        return fail(c, rc, msg);
    }
    return check_flags(c);
}

// what the synchronous host entries do at their end: wait for the stream and look at the verdict of THEIR OWN call (verdicts on
// earlier asynchronous calls were drained into async_bad before the call started and stay there for uf3_ctx_synchronize)
static int sync_own_call(uf3_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rc = poll_pending(c, true, false);
    if (rc) return rc;
    return check_flags(c);
}

// ---- timing of kernel classes with HIP events on the launch stream ----------------------
enum { T_FEAT = 0, T_NBR = 1, T_GRAM = 2, T_EVAL = 3 };
struct Timed {
    uf3_ctx *c; int cls; hipEvent_t a = nullptr, b = nullptr;
    Timed(uf3_ctx *c_, int cls_) : c(c_), cls(cls_) {
        if (c->timing) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, c->stream); }
    }
    ~Timed() {
        if (c->timing) { hipEventRecord(b, c->stream); c->pending[cls].push_back({a, b}); if (cls == T_FEAT) c->n_feat_launch++; }
    }
};

extern "C" int uf3_ctx_timing_reset(uf3_ctx *c, int enable) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    hipStreamSynchronize(c->stream);
    for (auto &v : c->pending) { for (auto &p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); } v.clear(); }
    c->t_feat = c->t_nbr = c->t_gram = c->t_eval = 0;
    c->n_feat_launch = 0;
    c->timing = enable != 0;
    return UF3_OK;
}

extern "C" int uf3_ctx_timing_read(uf3_ctx *c, double *feat_ms, int64_t *feat_launches, double *nbr_ms,
                                   double *gram_ms, double *eval_ms) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double *acc[4] = {&c->t_feat, &c->t_nbr, &c->t_gram, &c->t_eval};
    for (int k = 0; k < 4; k++) {
        for (auto &p : c->pending[k]) {
            float ms = 0;
            hipEventElapsedTime(&ms, p.first, p.second);
            *acc[k] += ms;
            hipEventDestroy(p.first); hipEventDestroy(p.second);
        }
        c->pending[k].clear();
    }
    if (feat_ms) *feat_ms = c->t_feat;
    if (feat_launches) *feat_launches = c->n_feat_launch;
    if (nbr_ms) *nbr_ms = c->t_nbr;
    if (gram_ms) *gram_ms = c->t_gram;
    if (eval_ms) *eval_ms = c->t_eval;
    return UF3_OK;
}

// ------------------------------------------------------------------------------ basis
// uf3_basis_create is check, plan, upload, publish.  basis_plan derives every table and every fact on the host alone -- a pure
// function of the spec and of two switches, composed of stages that each decide one thing --; uf3_basis_plan_debug
// returns its tables without a device, and tests/test_basis_plan_host.py pins them.
enum { BASIS_NO_MFMA_FEAT = 1, BASIS_NO_FEAT3 = 2 };      // the switches UF3_NO_MFMA_FEAT / UF3_NO_FEAT3, as bits
struct BasisPlan : BasisFacts {            // + the host image of every table uf3_basis_create uploads
    std::vector<KnotRec> recs;             // knot records of the pairs, then of the trio legs, then the window rows of the grouped layouts
    std::vector<int> lut;                  // raw bin -> global column, or -1
    std::vector<int> colsrc, dsrc;         // per column: the raw bins that feed it (l | m << 8 | n << 16) | their offsets in the dumped dense window
    std::vector<unsigned short> gsrc;      // fold tables of the grouped windows
    std::vector<TrioDev> trios;
    std::vector<double> f3rows;            // k_featurize3: window rows,
    std::vector<unsigned short> f3src;     // ... fold tables
    std::vector<int> f3off;                // ... and [T] where a trio's table starts
    std::vector<int> sp_cols;              // [S][F] the columns of the blocks a species takes part in
};

static bool same_leg(const LegDev &a, const LegDev &b) {
    return a.rec_off == b.rec_off && a.nk == b.nk && a.t0 == b.t0 && a.tlast == b.tlast && a.inv_h == b.inv_h;
}

// Where `run` lies in `table`, appended when no offset that is a multiple of `step` holds an identical run: tables that repeat
// (the same settings on every pair / trio, the same symmetry on the same layout) are stored once and stay small enough for LDS.
// Padding behind a run is the caller's.
template <class T>
static int intern_run(std::vector<T> &table, const std::vector<T> &run, size_t step) {
    for (size_t off = 0; off + run.size() <= table.size(); off += step)
        if (std::equal(run.begin(), run.end(), table.begin() + off, [](const T &a, const T &b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }))
            return (int)off;
    table.insert(table.end(), run.begin(), run.end());
    return (int)(table.size() - run.size());
}

// Interval records of one knot sequence; identical sequences share one run of the table.
static void fill_leg(LegDev &leg, const double *t, int nk, std::vector<KnotRec> &recs) {
    leg.nk = nk;
    leg.t0 = t[0];
    leg.tlast = t[nk - 1];
    leg.inv_h = (leg.tlast > leg.t0) ? (double)(nk - 7) / (leg.tlast - leg.t0) : 0.0;
    std::vector<KnotRec> mine;
    for (int i = 0; i < nk - 1; i++) {
        KnotRec r;
        std::memset(&r, 0, sizeof(r));
        if (i >= 3 && i <= nk - 5) {
            for (int q = 0; q < 6; q++) r.t[q] = t[i - 2 + q];
            auto rc = [](double d) { return d > 0 ? 1.0 / d : 0.0; };
            r.r[0] = rc(t[i + 1] - t[i]);
            r.r[1] = rc(t[i + 1] - t[i - 1]); r.r[2] = rc(t[i + 2] - t[i]);
            r.r[3] = rc(t[i + 1] - t[i - 2]); r.r[4] = rc(t[i + 2] - t[i - 1]); r.r[5] = rc(t[i + 3] - t[i]);
        }
        mine.push_back(r);
    }
    leg.rec_off = intern_run(recs, mine, 1);
}

// Coefficients, in powers of u = x - t[i], of the cubic B-spline basis function j on the knot interval (t[i], t[i+1]]:
// Cox - de Boor with polynomials instead of numbers (long double; 0 / 0 := 0 at repeated knots).  Zero when the interval is
// outside the function's support.
static void bspline_piece(const double *t, int j, int i, double c[4]) {
    long double cur[4][4];
    for (int k = 0; k < 4; k++) for (int e = 0; e < 4; e++) cur[k][e] = (e == 0 && j + k == i) ? 1.0L : 0.0L;
    for (int d = 1; d <= 3; d++)
        for (int k = 0; k + d <= 3; k++) {
            const int q = j + k;
            const long double den1 = (long double)t[q + d] - t[q], den2 = (long double)t[q + d + 1] - t[q + 1];
            long double out[4] = {0, 0, 0, 0};
            if (den1 != 0) {
                const long double a0 = ((long double)t[i] - t[q]) / den1, a1 = 1.0L / den1;
                for (int e = 0; e < 4; e++) { out[e] += a0 * cur[k][e]; if (e < 3) out[e + 1] += a1 * cur[k][e]; }
            }
            if (den2 != 0) {
                const long double b0 = ((long double)t[q + d + 1] - t[i]) / den2, b1 = -1.0L / den2;
                for (int e = 0; e < 4; e++) { out[e] += b0 * cur[k + 1][e]; if (e < 3) out[e + 1] += b1 * cur[k + 1][e]; }
            }
            for (int e = 0; e < 4; e++) cur[k][e] = out[e];
        }
    for (int e = 0; e < 4; e++) c[e] = (double)cur[0][e];
}

// Window rows of one leg, appended to `rows`: for every knot interval i = 3 .. nk - 5 one row of 18 doubles [t_i, t_i+1 |
// 4 functions x (c0 c1 c2 c3)] -- the polynomial pieces, in powers of x - t_i, of four consecutive basis functions of a window of
// the leg's functions.  window(i, w_lo, w_ext, sb) names the window the interval's row serves (first function, extent) and the
// window slot sb of the first of the four: the one thing the users differ in.  Zeros where a function is past the window or
// vanishes on the interval.  A kernel evaluates a record's window slots straight from the row.  Returns the number of rows.
template <class Window>
static int window_rows(const double *tk, int nk, Window window, std::vector<double> &rows) {
    for (int i = 3; i <= nk - 5; i++) {
        double row[18] = {0};
        row[0] = tk[i]; row[1] = tk[i + 1];
        int w_lo, w_ext, sb;
        window(i, w_lo, w_ext, sb);
        for (int fq = 0; fq < 4 && sb + fq < w_ext; fq++) {
            const int j = w_lo + sb + fq;
            if (j >= i - 3 && j <= i && j >= 0 && j <= nk - 5) bspline_piece(tk, j, i, row + 2 + 4 * fq);
        }
        rows.insert(rows.end(), row, row + 18);
    }
    return std::max(0, nk - 7);
}

// Range tests on the squared distance.  The kernels form s = (dx dx + dy dy) + dz dz without fused operations and take the
// correctly rounded root, so that "d < r" agrees with the reference's cdist to the last bit; the root is monotonic in s, so
// the same decisions can be taken on s itself against thresholds found here, and the root is left to the few candidates kept.
static double sq_root_le(double r) {          // the largest double s with sqrt(s) <= r   (r >= 0)
    double s = r * r;
    while (std::sqrt(s) <= r) s = std::nextafter(s, HUGE_VAL);
    while (s > 0 && std::sqrt(s) > r) s = std::nextafter(s, -HUGE_VAL);
    return s;
}
static double sq_root_ge(double r) {          // the smallest double s with sqrt(s) >= r
    double s = r * r;
    while (s > 0 && std::sqrt(s) >= r) s = std::nextafter(s, -HUGE_VAL);
    while (std::sqrt(s) < r) s = std::nextafter(s, HUGE_VAL);
    return s;
}

// Every refusal of a spec but one (more knot intervals than the grouped windows can number: plan_window_rows), before anything is
// derived: the stages below index by what the spec says.  The message, or nothing.
static std::string basis_check(const uf3_basis_spec *s) {
    const int S = s->n_species, T = s->n_trios;
    if (S < 1 || S > UF3_MAX_SPECIES) return "uf3_basis_create: 1..8 species supported";
    if (s->n_pairs != S * (S + 1) / 2) return "uf3_basis_create: n_pairs must be S(S+1)/2";
    int z2s[120];
    for (int &v : z2s) v = -1;
    for (int i = 0; i < S; i++) {
        const int z = s->species_z[i];
        if (z < 1 || z >= 120 || (i && z <= s->species_z[i - 1])) return "species_z must be ascending atomic numbers";
        z2s[z] = i;
    }
    auto species = [&](int z) { return z > 0 && z < 120 ? z2s[z] : -1; };
    int top = S;                                 // where the last column block ends
    for (int p = 0; p < s->n_pairs; p++) {
        const int nk = s->pair_nk[p], col = s->pair_col[p];
        if (species(s->pair_z[2 * p]) < 0 || species(s->pair_z[2 * p + 1]) < 0 || nk < 8 || col < 0) return "bad pair block";
        top = std::max(top, col + nk - 4);
    }
    if (T < 0) return "bad trio block";
    for (int t = 0; t < T; t++) {
        const int sc = species(s->trio_z[3 * t]), sa = species(s->trio_z[3 * t + 1]), sb = species(s->trio_z[3 * t + 2]);
        if (sc < 0 || sa < 0 || sb < 0 || sa > sb || s->trio_col[t] < 0 || s->trio_ncol[t] < 0) return "bad trio block";
        for (int d = 0; d < 3; d++) if (s->trio_nk[3 * t + d] < 8) return "trio knot vector too short";
        top = std::max(top, s->trio_col[t] + s->trio_ncol[t]);
    }
    std::vector<int> most(T, 0);                 // per trio: the most raw bins that feed one of its columns
    const int32_t *lut = s->trio_lut;
    for (int t = 0; t < T; t++) {
        const int *nk = s->trio_nk + 3 * t, ncol = s->trio_ncol[t];
        const size_t n = (size_t)(nk[0] - 4) * (nk[1] - 4) * (nk[2] - 4);
        std::vector<int> fed(ncol, 0);
        for (size_t q = 0; q < n; q++) {
            const int v = lut[q];
            if (v >= ncol) return "trio_lut entry out of range";
            if (v >= 0) most[t] = std::max(most[t], ++fed[v]);
        }
        lut += n;
    }
    for (int t = 0; t < T; t++) {
        for (int d = 0; d < 3; d++) if (s->trio_nk[3 * t + d] - 4 > 255) return "3-body grid dimension > 255";
        if (most[t] > 6) return "a 3-body column is fed by more than 6 raw bins";
    }
    if (top != s->n_feat) return "column blocks do not add up to n_feat";
    return "";
}

static void plan_pairs(const uf3_basis_spec *s, BasisPlan &P) {
    BasisDev &h = P.host;
    const double *kp = s->pair_knots;
    h.rmax2 = 0;
    for (int p = 0; p < h.P; p++) {
        const int a = h.z2s[s->pair_z[2 * p]], bb = h.z2s[s->pair_z[2 * p + 1]], nk = s->pair_nk[p];
        h.pair_of[a * UF3_MAX_SPECIES + bb] = h.pair_of[bb * UF3_MAX_SPECIES + a] = (short)p;
        PairDev &pd = h.pairs[p];
        fill_leg(pd.leg, kp, nk, P.recs);
        pd.col = s->pair_col[p];
        pd.nb = nk - 4;
        pd.sa = std::min(a, bb); pd.sb = std::max(a, bb);
        pd.rmin = s->pair_rmin[p] > 0 ? s->pair_rmin[p] : 0.0;   // max(r_min, 0), distances.py:60
        pd.rmax = s->pair_rmax[p];
        pd.s_lo = sq_root_le(pd.rmin); pd.s_hi = sq_root_ge(pd.rmax);
        h.rmax2 = std::max(h.rmax2, pd.rmax);
        P.block_bounds.push_back(pd.col + pd.nb);
        P.c2_len += (size_t)pd.nb;
        kp += nk;
    }
    P.n_pair_recs = P.recs.size();
}

// The legs, grid and place in the LUT of every trio, and the 3-body list range.  Returns the knots of every leg, [3 t + leg].
static std::vector<const double *> plan_trio_legs(const uf3_basis_spec *s, BasisPlan &P) {
    BasisDev &h = P.host;
    P.trios.resize(h.T);
    std::vector<const double *> knots(3 * (size_t)h.T, nullptr);
    const double *tp = s->trio_knots;
    double lo3 = 1e300, hi3 = -1e300;
    size_t lut_len = 0;
    for (int t = 0; t < h.T; t++) {
        const int sc = h.z2s[s->trio_z[3 * t]], sa = h.z2s[s->trio_z[3 * t + 1]], sb = h.z2s[s->trio_z[3 * t + 2]];
        h.trio_of[(sc * UF3_MAX_SPECIES + sa) * UF3_MAX_SPECIES + sb] = (short)t;
        h.trio_of[(sc * UF3_MAX_SPECIES + sb) * UF3_MAX_SPECIES + sa] = (short)t;
        TrioDev &td = P.trios[t];
        for (int d = 0; d < 3; d++) {
            const int nk = s->trio_nk[3 * t + d];
            fill_leg(td.leg[d], tp, nk, P.recs);
            knots[3 * (size_t)t + d] = tp;
            for (int q = 0; q < nk; q++) {
                lo3 = std::min(lo3, tp[q]);
                if (d < 2) hi3 = std::max(hi3, tp[q]);     // angles.py:322-325: centre legs only
            }
            tp += nk;
        }
        td.dim_l = td.leg[0].nk - 4; td.dim_m = td.leg[1].nk - 4; td.dim_n = td.leg[2].nk - 4;
        td.col = s->trio_col[t];
        td.ncol = s->trio_ncol[t];
        td.sc = sc; td.sa = sa; td.sb = sb;
        td.lut_off = (int)lut_len;
        lut_len += (size_t)td.dim_l * td.dim_m * td.dim_n;
        P.block_bounds.push_back(td.col + td.ncol);
    }
    P.c3_len = lut_len;
    P.lut.assign(lut_len ? lut_len : 1, -1);
    h.rmin3 = h.T ? std::max(lo3, 0.0) : 0.0;
    h.rmax3 = h.T ? hi3 : 0.0;
    h.s3_lo = sq_root_le(h.rmin3); h.s3_hi = sq_root_le(h.rmax3);
    h.rsearch = std::max(h.rmax2, h.rmax3);
    return knots;
}

// One walk of a trio's part of the LUT: its entries as global columns, and per column the distinct raw bins (symmetry images) that
// feed it, l | m << 8 | n << 16, for the output-stationary kernels.  With them nsrc and the window: the bounding box of those bins.
static std::vector<std::vector<int>> trio_sources(const uf3_basis_spec *s, TrioDev &td, std::vector<int> &lut) {
    std::vector<std::vector<int>> per_col(td.ncol);
    const size_t n = (size_t)td.dim_l * td.dim_m * td.dim_n;
    for (size_t q = 0; q < n; q++) {
        const int v = s->trio_lut[td.lut_off + q];
        lut[td.lut_off + q] = v < 0 ? -1 : td.col + v;
        if (v < 0) continue;
        const int l = (int)(q / ((size_t)td.dim_m * td.dim_n)), m = (int)((q / td.dim_n) % td.dim_m), nn = (int)(q % td.dim_n);
        per_col[v].push_back(l | (m << 8) | (nn << 16));
    }
    size_t mx = 1;
    for (auto &v : per_col) mx = std::max(mx, v.size());
    td.nsrc = mx <= 1 ? 1 : (mx <= 2 ? 2 : 6);
    int lo[3] = {1 << 20, 1 << 20, 1 << 20}, hi[3] = {-1, -1, -1};
    for (auto &v : per_col) for (int sp : v) {
        const int idx[3] = {sp & 255, (sp >> 8) & 255, (sp >> 16) & 255};
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], idx[a]); hi[a] = std::max(hi[a], idx[a]); }
    }
    for (int a = 0; a < 3; a++) { td.lo[a] = hi[a] < 0 ? 0 : lo[a]; td.ext[a] = hi[a] < 0 ? 1 : hi[a] - lo[a] + 1; }
    return per_col;
}

// rows (c, l) x columns (m, n) of the window in 16 x 16 tiles: (1,1) (1,2) (1,<=4) (<=2,<=6) have a matrix-core specialisation
// (modes 6-9); wider windows stay on the generic kernels
static void trio_dense_mode(TrioDev &td, const DenseLayout &dl, unsigned switches, BasisPlan &P) {
    td.dense = (switches & BASIS_NO_MFMA_FEAT) ? 0 : dense_mode_for(td.ext[0], td.ext[1], td.ext[2]);
    if (!td.dense) return;
    P.dense_stride[td.dense] = std::max(P.dense_stride[td.dense], dl.stride);
    P.dense_dump[td.dense] = std::max(P.dense_dump[td.dense], td.ext[0] * dl.cw);
}

// 3 x 3 x 6..9 windows of mode 7 stage grouped n windows; tn: the knots of leg n, n_knot_recs: the knot records of all legs
static void trio_grouped(TrioDev &td, const DenseLayout &dl, const double *tn, size_t n_knot_recs, BasisPlan &P) {
    td.grouped = 0; td.gthr0 = -1e300; td.gthr2 = 1e300;
    if (td.dense == 7 && td.ext[1] == 3 && td.ext[0] <= 3 && td.ext[2] >= 6 && td.ext[2] <= 9 && td.nsrc <= 2 && td.ncol <= 128) {
        // first window bin f = interval - 3 - lo_n: f <= 1 -> group 0 (bins 0..4), f >= 4 -> group 2 (bins 4..8)
        const int nk = td.leg[2].nk, i_lo = 3, i_hi = nk - 5;
        const int i0 = td.lo[2] + 4, i2 = td.lo[2] + 7;       // last interval of group 0, first of group 2
        td.grouped = 1;
        if (i0 >= i_lo) td.gthr0 = tn[std::min(i0, i_hi) + 1];
        if (i2 <= i_hi) td.gthr2 = tn[std::max(i2, i_lo)];
    }
    if (td.dense) P.dense_stride_f[td.dense] = std::max(P.dense_stride_f[td.dense], td.grouped ? 34 : dl.stride);
    if (td.grouped && (td.leg[0].nk > 255 || td.leg[1].nk > 255 || td.leg[2].nk > 255 || n_knot_recs > 65535)) td.grouped = 0;   // (GroupedLayout packs them)
    if (td.dense && td.grouped) P.dense_grouped[td.dense] = true;
}

// The column tiles (16 n-major columns each) that the records of knot interval i of leg n touch; false: the interval lies outside
// the window
static bool tiles_of(const TrioDev &td, int i, int &t0, int &t1) {
    const int f = i - 3 - td.lo[2], n0 = std::max(f, 0), n1 = std::min(f + 3, td.ext[2] - 1);
    if (n0 > n1) return false;
    t0 = (n0 * td.ext[1]) / 16; t1 = ((n1 + 1) * td.ext[1] - 1) / 16;
    return true;
}

// wide windows (mode 9, two row tiles): cut the intervals of leg n into at most three bands whose records touch at most three
// neighbouring column tiles (trio_block_banded); windows that do not fit keep the dense loop
static void trio_bands(TrioDev &td, const DenseLayout &dl, const double *tn, BasisPlan &P) {
    td.banded = 0; td.band_tile[0] = td.band_tile[1] = td.band_tile[2] = 0;
    if (!(td.dense == 9 && dl.stride == 64 && (4 * td.ext[0] + 15) / 16 == 2)) return;
    const int i_lo = 3, i_hi = td.leg[2].nk - 5, n_ct = (td.ext[1] * td.ext[2] + 15) / 16;
    int band_first[4] = {i_lo, -1, -1, -1}, band_lo[3] = {-1, -1, -1}, nb = 0;
    for (int i = i_lo; i <= i_hi; i++) {
        int t0, t1;
        if (!tiles_of(td, i, t0, t1)) continue;                   // (an interval outside the window: any band)
        if (band_lo[nb] < 0) band_lo[nb] = t0;
        if (t1 - band_lo[nb] + 1 > 3) {                           // does not fit the open band: start the next one
            if (++nb > 2 || t1 - t0 + 1 > 3) return;
            band_first[nb] = i; band_lo[nb] = t0;
        }
    }
    td.banded = 1;
    td.gthr0 = nb >= 1 ? tn[band_first[1]] : 1e300;               // r_n <= t_i: interval < i
    td.gthr2 = nb >= 2 ? tn[band_first[2]] : 1e300;
    for (int q = 0; q < 3; q++) td.band_tile[q] = std::max(0, std::min(band_lo[q] < 0 ? 0 : band_lo[q], std::max(0, n_ct - 3)));
    P.dense_grouped[9] = true;
}

// two column tiles: the intervals of leg n in order are tile 0 only, ..., tile 1 only (an interval i holds t_i < r <= t_{i+1})
static void trio_tile_thresholds(TrioDev &td, const double *tn) {
    td.thr0 = -1e300; td.thr2 = 1e300;
    if (!(td.dense && dense_ct(td.dense) == 2)) return;
    const int i_lo = 3, i_hi = td.leg[2].nk - 5;
    auto misses = [&](int i, int tile) { int t0, t1; return !tiles_of(td, i, t0, t1) || (tile ? t1 < 1 : t0 > 0); };
    int i0 = i_lo - 1, i2 = i_hi + 1;
    while (i0 + 1 <= i_hi && misses(i0 + 1, 1)) i0++;      // last interval of the leading run without tile 1
    while (i2 - 1 >= i_lo && misses(i2 - 1, 0)) i2--;      // first interval of the trailing run without tile 0
    if (i0 >= i_lo) td.thr0 = tn[i0 + 1];
    if (i2 <= i_hi) td.thr2 = tn[i2];
}

// the output-stationary instance (1 .. 5, of k_featurize and of k_virial_rows alike) that serves a trio
static int generic_mode(const TrioDev &td) { return td.nsrc == 1 ? (td.ncol > WAVE ? 2 : 1) : (td.nsrc == 2 ? (td.ncol > WAVE ? 4 : 3) : 5); }

// Per trio: column sources, window, and the layout its launches use
static void plan_trio_layouts(const uf3_basis_spec *s, unsigned switches, const std::vector<const double *> &knots, BasisPlan &P) {
    const size_t n_knot_recs = P.recs.size();
    for (int t = 0; t < P.host.T; t++) {
        TrioDev &td = P.trios[t];
        const double *tn = knots[3 * (size_t)t + 2];
        const std::vector<std::vector<int>> per_col = trio_sources(s, td, P.lut);
        const DenseLayout dl = dense_layout(td.ext[0], td.ext[1], td.ext[2]);
        trio_dense_mode(td, dl, switches, P);
        trio_grouped(td, dl, tn, n_knot_recs, P);
        trio_bands(td, dl, tn, P);
        trio_tile_thresholds(td, tn);
        P.modes |= 1 << (td.dense ? td.dense : generic_mode(td));
        P.vmodes |= 1 << generic_mode(td);
        td.src_off = (int)P.colsrc.size();
        for (auto &v : per_col) for (int k = 0; k < td.nsrc; k++) {
            const int sp = k < (int)v.size() ? v[k] : -1;
            P.colsrc.push_back(sp);
            // offset inside one component's dumped rows: row l (width cw), columns n-major (n * ext_m + m)
            P.dsrc.push_back(sp < 0 || !td.dense ? -1
                             : ((sp & 255) - td.lo[0]) * dl.cw + (((sp >> 16) & 255) - td.lo[2]) * td.ext[1] + (((sp >> 8) & 255) - td.lo[1]));
        }
    }
}

// Grouped windows: number the distinct window layouts (by first appearance; returns the first trio of every layout) and write the
// fold tables -- per column, for (source 0 | 1) x (group 0 | 1 | 2), the double index of the source bin inside the dumped group
// tiles ([group][row 4 c + l][16 columns], component 0) or 15, an entry no record touches
static std::vector<int> plan_grouped_folds(BasisPlan &P) {
    std::vector<int> layout_rep;
    for (int t = 0; t < P.host.T; t++) {
        TrioDev &td = P.trios[t];
        td.layout = -1; td.gsrc_off = 0;
        if (!td.grouped) continue;
        for (size_t q = 0; q < layout_rep.size() && td.layout < 0; q++) {
            const TrioDev &o = P.trios[layout_rep[q]];
            bool same = o.gthr0 == td.gthr0 && o.gthr2 == td.gthr2;
            for (int a = 0; a < 3; a++) same = same && o.lo[a] == td.lo[a] && o.ext[a] == td.ext[a] && same_leg(o.leg[a], td.leg[a]);
            if (same) td.layout = (int)q;
        }
        if (td.layout < 0) { td.layout = (int)layout_rep.size(); layout_rep.push_back(t); }
        if (td.layout > 254) { td.grouped = 0; td.layout = -1; continue; }     // (never in practice: the ordinary two-tile path)
        std::vector<unsigned short> mine;
        for (int col = 0; col < td.ncol; col++)
            for (int q = 0; q < 2; q++) {
                const int sp = q < td.nsrc ? P.colsrc[td.src_off + col * td.nsrc + q] : -1;
                for (int grp = 0; grp < 3; grp++) {
                    unsigned short a = 15;
                    if (sp >= 0) {
                        const int l_rel = (sp & 255) - td.lo[0], m_rel = ((sp >> 8) & 255) - td.lo[1], n_rel = ((sp >> 16) & 255) - td.lo[2];
                        const int nl = n_rel - 2 * grp;
                        if (nl >= 0 && nl < 5) a = (unsigned short)(grp * 256 + l_rel * 16 + nl * td.ext[1] + m_rel);
                    }
                    mine.push_back(a);
                }
            }
        td.gsrc_off = intern_run(P.gsrc, mine, 2);
        while (P.gsrc.size() & 1) P.gsrc.push_back(15);      // (blocks start on a 4-byte boundary)
    }
    return layout_rep;
}

// Window rows (window_rows) of the grouped layouts, appended to the knot records so that they travel to LDS with them.  The legs l
// and m: three slots from slot 0 (the fourth function is not stored).  Leg n: the window of the GROUP interval i belongs to, five
// slots from slot clamp(i - 3 - window start, 0, 1) -- every function alive on the interval is among the four, the fifth slot is
// zero.  Every slot of every record is written in every staging pass, and nothing has to be cleared (trio_block_grouped).
// TrioDev::wrow: the number of a leg's first row.
static bool plan_window_rows(const std::vector<const double *> &knots, const std::vector<int> &layout_rep, BasisPlan &P, std::string &err) {
    P.wrow_lo = P.recs.size();
    std::vector<double> wrows;
    int n_rows = 0;
    for (const int t : layout_rep) {
        TrioDev &rep = P.trios[t];
        for (int a = 0; a < 3; a++) {
            rep.wrow[a] = n_rows;
            n_rows += window_rows(knots[3 * (size_t)t + a], rep.leg[a].nk, [&](int i, int &w_lo, int &w_ext, int &sb) {
                w_lo = rep.lo[a]; w_ext = a == 0 ? rep.ext[0] : 3; sb = 0;
                if (a == 2) {
                    const int f = i - 3 - rep.lo[2], grp = f <= 1 ? 0 : (f >= 4 ? 2 : 1);
                    w_lo = rep.lo[2] + 2 * grp; w_ext = std::min(5, rep.ext[2] - 2 * grp);
                    sb = std::max(0, std::min(1, f - 2 * grp));
                }
            }, wrows);
        }
    }
    // (rows of nine 16-byte pairs, one behind the other: lanes that read pair k of different rows hit different banks -- 9 is
    // odd, rows 16 apart share one)
    P.n_wrows = n_rows;
    while (wrows.size() % 12) wrows.push_back(0.0);
    for (size_t q = 0; q < wrows.size(); q += 12) {
        KnotRec kr;
        std::memcpy(&kr, &wrows[q], sizeof kr);
        P.recs.push_back(kr);
    }
    for (auto &td : P.trios)
        if (td.grouped && td.layout >= 0) for (int a = 0; a < 3; a++) td.wrow[a] = P.trios[layout_rep[td.layout]].wrow[a];
    if (n_rows > 65535)                                                 // (GroupedLayout packs the row numbers in 16 bits)
        for (auto &td : P.trios) if (td.grouped) { err = "too many knot intervals for the grouped windows"; return false; }
    return true;
}

// What is uniform over the pairs and over the trios, and with it which instances the evaluator may run
static void plan_eval(BasisPlan &P) {
    BasisDev &h = P.host;
    const std::vector<TrioDev> &trios = P.trios;
    h.pairs_uniform = 1;
    for (int a = 0; a < UF3_MAX_SPECIES * UF3_MAX_SPECIES; a++) h.pair_col[a] = h.pair_of[a] >= 0 ? h.pairs[h.pair_of[a]].col : 0;
    for (int p = 1; p < h.P && h.pairs_uniform; p++) {
        const PairDev &a = h.pairs[0], &q = h.pairs[p];
        if (!same_leg(a.leg, q.leg) || a.rmin != q.rmin || a.rmax != q.rmax || a.nb != q.nb) h.pairs_uniform = 0;
    }
    h.trio_legs_uniform = h.T > 0;
    for (int t = 1; t < h.T && h.trio_legs_uniform; t++) {
        for (int d = 0; d < 3; d++) if (!same_leg(trios[0].leg[d], trios[t].leg[d])) h.trio_legs_uniform = 0;
        if (trios[t].dim_l != trios[0].dim_l || trios[t].dim_m != trios[0].dim_m || trios[t].dim_n != trios[0].dim_n) h.trio_legs_uniform = 0;
    }
    // k_eval<TAB>: one set of 3-body legs, the trio tables in one register each, leg n's knot records in the workgroup's LDS
    P.eval_tab_ok = h.trio_legs_uniform && h.T <= WAVE && trios[0].leg[2].nk - 7 <= EVAL_TAB_KN;
    if (!P.eval_tab_ok) return;
    // k_eval<CW>: one window on every trio, centre legs alike, table + zero run small enough
    const TrioDev &t0 = trios[0];
    bool ok = t0.lo[0] == t0.lo[1] && t0.ext[0] == t0.ext[1] && t0.ext[0] >= 1;
    for (int t = 0; t < h.T && ok; t++) {
        const TrioDev &td = trios[t];
        ok = td.lo[0] == t0.lo[0] && td.lo[1] == t0.lo[0] && td.ext[0] == t0.ext[0] && td.ext[1] == t0.ext[0] &&
             td.dim_m == t0.dim_m && td.dim_n == t0.dim_n && td.dim_l == t0.dim_l;
    }
    if (ok) {
        const int ext = t0.ext[0], dn = t0.dim_n;
        const size_t table = (size_t)h.T * ext * ext * dn * 8;
        const size_t zero = ((size_t)(3 * ext + 3) * dn * 8 + 32 + 15) / 16 * 16;        // (any row offset + one row's 32 bytes)
        const size_t total = (table + zero + 1023) / 1024 * 1024;
        ok = total <= 40 * 1024 && ext == EVAL_CW_EXT;        // (UF3_EVAL_NO_CW is looked at per call, where the instance is chosen)
        if (ok) {
            P.cw_lo = t0.lo[0]; P.cw_ext = ext; P.cw_dim_m = t0.dim_m; P.cw_dim_n = dn;
            P.cw_zero = (int)table; P.cw_bytes = (int)total;
            for (int t = 0; t < h.T; t++) { P.cw_lut_off.push_back(trios[t].lut_off); P.cw_dim_l.push_back(trios[t].dim_l); }
        }
    }
    P.eval_cw_ok = ok;
}

// k_featurize3 (uf3_feat3.h) serves a basis with one window layout for all trios, centre legs alike, a window of an instantiated
// shape; trios with two equal neighbour species must fold symmetrically in (l, m).  (f3_nr is set as soon as the legs are uniform,
// whatever the answer: as it always was)
static bool plan_feat3_ok(unsigned switches, BasisPlan &P) {
    const BasisDev &h = P.host;
    if (!(h.T > 0 && h.trio_legs_uniform && !(switches & BASIS_NO_FEAT3))) return false;
    const TrioDev &t0 = P.trios[0];
    // the instantiated shapes (rows of the centre-leg window, rounds of 32 positions): (3, 1) (4, 2) (5, 3) (6, 3)
    const int ep = t0.ext[0], en = t0.ext[2];
    P.f3_nr = ep <= 3 ? 1 : (ep == 4 ? 2 : 3);          // (windows of one or two rows -- the reference's default resolution keeps
                                                         // 2 x 2 x 7 bins -- run in the three-row launch)
    // (a round of 32 positions holds whole rows of the summed leg: 32 / ext_n of them)
    const int prr = en > 0 && en <= 32 ? std::min(ep, 32 / en) : 0;
    const bool shape = prr > 0 && prr * P.f3_nr >= ep &&
                       ((ep >= 1 && ep <= 3 && prr * en <= 31 && en <= 9) || (ep == 4 && en <= 11) || ((ep == 5 || ep == 6) && en <= 13));
    bool ok = t0.lo[0] == t0.lo[1] && t0.ext[0] == t0.ext[1] && same_leg(t0.leg[0], t0.leg[1]) && shape &&
              t0.leg[0].nk >= 8 && t0.leg[2].nk >= 8;
    for (int t = 0; t < h.T && ok; t++) {
        const TrioDev &td = P.trios[t];
        for (int a = 0; a < 3; a++) ok = ok && td.lo[a] == t0.lo[a] && td.ext[a] == t0.ext[a];
        ok = ok && td.nsrc <= 2 && td.ncol >= 1;
        if (!(ok && td.sa == td.sb)) continue;
        const int *src = &P.colsrc[td.src_off];           // (l, m, n) and (m, l, n) feed the same column
        for (int col = 0; col < td.ncol && ok; col++)
            for (int q = 0; q < td.nsrc && ok; q++) {
                const int sp = src[col * td.nsrc + q];
                if (sp < 0) continue;
                const int swapped = ((sp >> 8) & 255) | ((sp & 255) << 8) | (sp & 0xff0000);
                bool found = false;
                for (int q2 = 0; q2 < td.nsrc; q2++) found = found || src[col * td.nsrc + q2] == swapped;
                ok = found;
            }
    }
    return ok;
}

// ... and its tables: the window rows (window_rows) of the centre legs and of leg n -- the first of the four functions at window
// slot clamp(i - 3 - window start, 0, ext - 4) --, and per trio the fold table [orientation 0 | 1][column][source 0 | 1] -> index of
// the source bin in the fold's dump.  False: the fold tables outgrow their 16 KB of LDS.
static bool plan_feat3_tables(const std::vector<const double *> &knots, BasisPlan &P) {
    const BasisDev &h = P.host;
    const TrioDev &t0 = P.trios[0];
    P.f3_lo_p = t0.lo[0]; P.f3_ext_p = t0.ext[0]; P.f3_lo_n = t0.lo[2]; P.f3_ext_n = t0.ext[2];
    for (int kind = 0; kind < 2; kind++) {
        const int a = kind == 0 ? 0 : 2, w_lo_a = t0.lo[a], w_ext_a = t0.ext[a];
        Feat3Leg &lg = kind == 0 ? P.f3_leg_p : P.f3_leg_n;
        lg.t0 = t0.leg[a].t0; lg.tlast = t0.leg[a].tlast; lg.inv_h = t0.leg[a].inv_h; lg.nk = t0.leg[a].nk; lg.row0 = P.n_f3rows;
        P.n_f3rows += window_rows(knots[a], lg.nk, [&](int i, int &w_lo, int &w_ext, int &sb) {
            w_lo = w_lo_a; w_ext = w_ext_a; sb = std::max(0, std::min(std::max(0, w_ext - 4), i - 3 - w_lo));
        }, P.f3rows);
    }
    P.f3off.assign(h.T, 0);
    for (int t = 0; t < h.T; t++) {
        const TrioDev &td = P.trios[t];
        std::vector<unsigned short> mine;
        for (int o = 0; o < 2; o++)
            for (int col = 0; col < td.ncol; col++)
                for (int q = 0; q < 2; q++) {
                    const int sp = q < td.nsrc ? P.colsrc[td.src_off + col * td.nsrc + q] : -1;
                    // (a column's missing second source: position 31 of row 0 -- never a window position in the
                    // one-round launch --, or the zero behind the dumped rows)
                    const int ps = 32 * P.f3_nr;
                    unsigned short e = (unsigned short)(P.f3_nr == 1 ? 31 : td.ext[0] * ps);
                    if (sp >= 0) {
                        const int l = (sp & 255) - td.lo[0], m = ((sp >> 8) & 255) - td.lo[1], n = ((sp >> 16) & 255) - td.lo[2];
                        const int prr = std::min(td.ext[0], 32 / td.ext[2]), j = o == 0 ? m : l;
                        e = (unsigned short)((o == 0 ? l : m) * ps + (j / prr) * 32 + (j % prr) * td.ext[2] + n);
                    }
                    mine.push_back(e);
                }
        P.f3off[t] = intern_run(P.f3src, mine, 2);
    }
    while (P.f3src.size() & 1) P.f3src.push_back(31);
    if (P.f3src.size() * 2 <= 16384) { P.n_f3src = (int)P.f3src.size(); return true; }
    P.f3rows.clear(); P.f3src.clear(); P.f3off.clear();       // (nothing of it is uploaded)
    return false;
}

// the force rows of an atom of species s are zero outside the blocks s takes part in (and in the one-body columns)
static void plan_species_columns(BasisPlan &P) {
    const BasisDev &h = P.host;
    P.sp_cols.assign((size_t)h.S * h.F, 0);
    for (int sp = 0; sp < h.S; sp++) {
        std::vector<char> in(h.F, 0);
        for (int p = 0; p < h.P; p++)
            if (h.pairs[p].sa == sp || h.pairs[p].sb == sp) for (int q = 0; q < h.pairs[p].nb; q++) in[h.pairs[p].col + q] = 1;
        for (auto &td : P.trios)
            if (td.sc == sp || td.sa == sp || td.sb == sp) for (int q = 0; q < td.ncol; q++) in[td.col + q] = 1;
        int n = 0;
        for (int q = 0; q < h.F; q++) if (in[q]) P.sp_cols[(size_t)sp * h.F + n++] = q;
        P.sp_ncols[sp] = n;
    }
}

// P: a fresh plan.  False with the refusal in err.
static bool basis_plan(const uf3_basis_spec *s, unsigned switches, BasisPlan &P, std::string &err) {
    err = basis_check(s);
    if (!err.empty()) return false;
    P.r_cut = s->r_cut;
    BasisDev &h = P.host;
    std::memset(&h, 0, sizeof(h));
    h.S = s->n_species; h.P = s->n_pairs; h.T = s->n_trios; h.F = s->n_feat;
    h.lead2 = s->lead2; h.trail2 = s->trail2;
    std::memset(h.z2s, -1, sizeof(h.z2s));
    for (int i = 0; i < h.S; i++) h.z2s[s->species_z[i]] = (signed char)i;
    for (auto &v : h.pair_of) v = -1;
    for (auto &v : h.trio_of) v = -1;
    for (int i = 0; i <= h.S; i++) P.block_bounds.push_back(i);
    plan_pairs(s, P);
    const std::vector<const double *> knots = plan_trio_legs(s, P);
    plan_trio_layouts(s, switches, knots, P);
    if (!plan_window_rows(knots, plan_grouped_folds(P), P, err)) return false;
    std::sort(P.block_bounds.begin(), P.block_bounds.end());
    P.block_bounds.erase(std::unique(P.block_bounds.begin(), P.block_bounds.end()), P.block_bounds.end());
    P.n_recs = P.recs.size();
    P.trio_rec_lo = P.recs.size();
    for (auto &td : P.trios) for (int d = 0; d < 3; d++) P.trio_rec_lo = std::min(P.trio_rec_lo, (size_t)td.leg[d].rec_off);
    P.n_dsrc = P.dsrc.size();
    P.n_gsrc = P.gsrc.size();
    P.all_grouped7 = P.all_banded9 = true;
    for (auto &td : P.trios) {
        if (td.dense == 7 && !td.grouped) P.all_grouped7 = false;
        // (the banded-only launch names its accumulator tiles at compile time: bands on the tiles 0, 1, 2)
        if (td.dense == 9 && !(td.banded && td.band_tile[0] == 0 && td.band_tile[1] == 1 && td.band_tile[2] == 2)) P.all_banded9 = false;
        td.head = TrioHead{td.dense, td.nsrc, td.ncol, td.sc, td.sa, td.sb, td.col,       // (layouts and bands are final)
                           td.grouped ? ((td.layout + 1) | (td.gsrc_off << 8))
                                      : (td.banded ? (1 | (td.band_tile[0] << 8) | (td.band_tile[1] << 12) | (td.band_tile[2] << 16)) : 0)};
    }
    plan_eval(P);
    P.feat3_ok = plan_feat3_ok(switches, P) && plan_feat3_tables(knots, P);
    if (P.feat3_ok) P.modes |= 1 << 12;
    plan_species_columns(P);
    return true;
}

// One table of a basis on the device: room for `room` >= n elements (kernels may read past the logical end), n of them copied in
template <class T>
static hipError_t upload(DevTable<T> &d, const T *src, size_t n, size_t room) {
    const hipError_t e = hipMalloc(&d.p, sizeof(T) * room);
    if (e != hipSuccess) return e;
    d.cap = sizeof(T) * room;
    return n ? hipMemcpy(d.p, src, sizeof(T) * n, hipMemcpyHostToDevice) : hipSuccess;
}
template <class T>
static hipError_t upload(DevTable<T> &d, const std::vector<T> &v, size_t room = 0) { return upload(d, v.data(), v.size(), std::max(room, v.size())); }

extern "C" int uf3_basis_create(uf3_ctx *c, const uf3_basis_spec *s, uf3_basis **out) {
    uf3_env_refresh();
    if (!c || !s || !out) return fail(c, UF3_EINVAL, "uf3_basis_create: null argument");
    const unsigned switches = (uf3_env("UF3_NO_MFMA_FEAT") ? BASIS_NO_MFMA_FEAT : 0) | (uf3_env("UF3_NO_FEAT3") ? BASIS_NO_FEAT3 : 0);
    BasisPlan P;
    std::string err;
    if (!basis_plan(s, switches, P, err)) return fail(c, UF3_EINVAL, err);
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<uf3_basis> b(new uf3_basis());      // (a failed upload frees what the earlier ones allocated)
    b->ctx = c;
    HIPCHK(c, upload(b->d_recs, P.recs, 1));
    HIPCHK(c, upload(b->d_lut, P.lut));
    HIPCHK(c, upload(b->d_colsrc, P.colsrc, 1));
    HIPCHK(c, upload(b->d_dsrc, P.dsrc, 1));
    HIPCHK(c, upload(b->d_gsrc, P.gsrc, P.gsrc.size() + 8));
    HIPCHK(c, upload(b->d_trios, P.trios, 1));
    if (P.feat3_ok) {
        HIPCHK(c, upload(b->d_f3rows, P.f3rows));
        HIPCHK(c, upload(b->d_f3src, P.f3src));
        HIPCHK(c, upload(b->d_f3off, P.f3off));
    }
    HIPCHK(c, upload(b->d_sp_cols, P.sp_cols));
    P.host.trios = b->d_trios; P.host.recs = b->d_recs; P.host.lut = b->d_lut;
    static_cast<BasisFacts &>(*b) = P;
    HIPCHK(c, upload(b->dev, &b->host, 1, 1));
    *out = b.release();
    return UF3_OK;
}

// table: 0 the summary (uf3_basis_plan_summary), then the host mirror, recs, lut, colsrc, dsrc, gsrc, trios, f3rows, f3src, f3off,
// sp_cols, block_bounds, cw_lut_off, cw_dim_l -- what basis_plan made of the spec, and nothing else
extern "C" int uf3_basis_plan_debug(const uf3_basis_spec *s, int switches, int table, void *out, int64_t cap, int64_t *len) {
    if (!s || !len || cap < 0) return fail(nullptr, UF3_EINVAL, "uf3_basis_plan_debug: bad argument");
    BasisPlan P;
    std::string err;
    if (!basis_plan(s, (unsigned)switches, P, err)) return fail(nullptr, UF3_EINVAL, err);
    uf3_basis_plan_summary o;
    std::memset(&o, 0, sizeof o);
    o.c2_len = (int64_t)P.c2_len; o.c3_len = (int64_t)P.c3_len; o.n_recs = (int64_t)P.n_recs; o.n_pair_recs = (int64_t)P.n_pair_recs;
    o.trio_rec_lo = (int64_t)P.trio_rec_lo; o.wrow_lo = (int64_t)P.wrow_lo; o.n_dsrc = (int64_t)P.n_dsrc; o.n_gsrc = (int64_t)P.n_gsrc;
    o.r_cut = P.r_cut;
    const Feat3Leg *legs[2] = {&P.f3_leg_p, &P.f3_leg_n};
    for (int k = 0; k < 2; k++) {
        o.f3_leg[k][0] = legs[k]->t0; o.f3_leg[k][1] = legs[k]->tlast; o.f3_leg[k][2] = legs[k]->inv_h;
        o.f3_leg_nk[k] = legs[k]->nk; o.f3_leg_row0[k] = legs[k]->row0;
    }
    o.n_wrows = P.n_wrows; o.modes = P.modes; o.vmodes = P.vmodes; o.all_grouped7 = P.all_grouped7; o.all_banded9 = P.all_banded9;
    o.feat3_ok = P.feat3_ok; o.eval_tab_ok = P.eval_tab_ok; o.eval_cw_ok = P.eval_cw_ok;
    o.cw_lo = P.cw_lo; o.cw_ext = P.cw_ext; o.cw_dim_m = P.cw_dim_m; o.cw_dim_n = P.cw_dim_n; o.cw_zero = P.cw_zero; o.cw_bytes = P.cw_bytes;
    o.f3_lo_p = P.f3_lo_p; o.f3_ext_p = P.f3_ext_p; o.f3_lo_n = P.f3_lo_n; o.f3_ext_n = P.f3_ext_n; o.f3_nr = P.f3_nr;
    o.n_f3rows = P.n_f3rows; o.n_f3src = P.n_f3src;
    o.pairs_uniform = P.host.pairs_uniform; o.trio_legs_uniform = P.host.trio_legs_uniform;
    for (int k = 0; k < UF3_MAX_SPECIES; k++) o.sp_ncols[k] = P.sp_ncols[k];
    for (int k = 0; k < 16; k++) {
        o.dense_stride[k] = P.dense_stride[k]; o.dense_stride_f[k] = P.dense_stride_f[k];
        o.dense_grouped[k] = P.dense_grouped[k]; o.dense_dump[k] = P.dense_dump[k];
    }
    auto bytes_of = [](const auto &v) { return std::pair<const void *, size_t>(v.data(), v.size() * sizeof(v[0])); };
    const std::pair<const void *, size_t> tables[] = {
        {&o, sizeof o}, {&P.host, sizeof(BasisDev)}, bytes_of(P.recs), bytes_of(P.lut), bytes_of(P.colsrc), bytes_of(P.dsrc),
        bytes_of(P.gsrc), bytes_of(P.trios), bytes_of(P.f3rows), bytes_of(P.f3src), bytes_of(P.f3off), bytes_of(P.sp_cols),
        bytes_of(P.block_bounds), bytes_of(P.cw_lut_off), bytes_of(P.cw_dim_l)};
    if (table < 0 || table >= (int)(sizeof tables / sizeof tables[0])) return fail(nullptr, UF3_EINVAL, "uf3_basis_plan_debug: no such table");
    *len = (int64_t)tables[table].second;
    if (!out) return UF3_OK;
    if ((size_t)cap < tables[table].second) return fail(nullptr, UF3_EINVAL, "uf3_basis_plan_debug: buffer too small");
    std::memcpy(out, tables[table].first, tables[table].second);
    return UF3_OK;
}

extern "C" int uf3_basis_featurizer_modes(const uf3_basis *b, int32_t *mask) {
    if (!b || !mask) return UF3_EINVAL;
    *mask = b->modes;
    return UF3_OK;
}

extern "C" void uf3_basis_destroy(uf3_basis *handle) {
    const std::unique_ptr<uf3_basis> b(handle);      // (its tables free themselves when it goes, after the two calls below)
    if (!b) return;
    hipSetDevice(b->ctx->device);
    hipStreamSynchronize(b->ctx->stream);
}

// ------------------------------------------------------------------------------ frame geometry
static void cross3(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static double norm3(const double *a) { return std::sqrt(dot3(a, a)); }

// image range of the reference supercell (geometry.py:54-83), on the cell as given
static void reference_factors(const double *cell, double r_cut, int *fac) {
    bool all_zero = true, zero_vec = false;
    for (int i = 0; i < 9; i++) if (cell[i] != 0.0) all_zero = false;
    for (int i = 0; i < 3; i++) if (norm3(cell + 3 * i) == 0.0) zero_vec = true;
    if (all_zero || zero_vec) { fac[0] = fac[1] = fac[2] = 1; return; }
    double n[3][3];
    cross3(cell + 3, cell + 6, n[0]); cross3(cell, cell + 6, n[1]); cross3(cell, cell + 3, n[2]);
    for (int i = 0; i < 3; i++) {
        double s = dot3(cell + 3 * i, n[i]) / dot3(n[i], n[i]);
        double p[3] = {n[i][0] * s, n[i][1] * s, n[i][2] * s};
        fac[i] = (int)std::ceil(r_cut / norm3(p));
    }
}

static bool invert3(const double *m, double *inv) {
    double c0[3], c1[3], c2[3];
    cross3(m + 3, m + 6, c0); cross3(m + 6, m, c1); cross3(m, m + 3, c2);
    double det = dot3(m, c0);
    if (!(std::fabs(det) > 1e-300)) return false;
    for (int k = 0; k < 3; k++) { inv[3 * k] = c0[k] / det; inv[3 * k + 1] = c1[k] / det; inv[3 * k + 2] = c2[k] / det; }
    return true;
}

// (extra: added to the search radius of the cell list -- the skin of the MD route's superset lists; the reference's image range
// `fac` and the window stay those of r_cut)
static int make_geom(uf3_ctx *c, const uf3_basis *b, const uf3_frames *fr, int f, FrameGeom &g, int &bin_cursor, double extra = 0.0) {
    const double *cell = fr->cells + 9 * (size_t)f;
    const uint8_t *pbc = fr->pbc + 3 * (size_t)f;
    int64_t lo = fr->atom_offsets[f], hi = fr->atom_offsets[f + 1];
    std::memset(&g, 0, sizeof(g));
    g.atom_lo = (int)lo; g.atom_hi = (int)hi;
    int n = (int)(hi - lo), n_per = 0;
    for (int k = 0; k < 3; k++) { g.per[k] = pbc[k] ? 1 : 0; n_per += g.per[k]; }
    std::memcpy(g.cell, cell, sizeof(double) * 9);
    // effective cell: non-periodic axes become unit vectors orthogonal to the periodic ones
    double eff[9];
    std::memcpy(eff, cell, sizeof(eff));
    if (n_per == 0) {
        double id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(eff, id, sizeof(eff));
    } else if (n_per < 3) {
        int pa[3], np = 0, na[3], nn = 0;
        for (int k = 0; k < 3; k++) { if (g.per[k]) pa[np++] = k; else na[nn++] = k; }
        if (np == 2) {
            double w[3];
            cross3(eff + 3 * pa[0], eff + 3 * pa[1], w);
            double l = norm3(w);
            if (l == 0) return fail(c, UF3_EINVAL, "periodic lattice vectors are parallel");
            for (int q = 0; q < 3; q++) eff[3 * na[0] + q] = w[q] / l;
        } else {
            const double *u = eff + 3 * pa[0];
            double l = norm3(u);
            if (l == 0) return fail(c, UF3_EINVAL, "periodic lattice vector has zero length");
            double t[3] = {0, 0, 0};
            int mn = 0;
            for (int q = 1; q < 3; q++) if (std::fabs(u[q]) < std::fabs(u[mn])) mn = q;
            t[mn] = 1.0;
            double v[3], w[3];
            cross3(u, t, v);
            double lv = norm3(v);
            for (int q = 0; q < 3; q++) v[q] /= lv;
            cross3(u, v, w);
            double lw = norm3(w);
            for (int q = 0; q < 3; q++) { eff[3 * na[0] + q] = v[q]; eff[3 * na[1] + q] = w[q] / lw; }
        }
    }
    if (!invert3(eff, g.inv)) return fail(c, UF3_EINVAL, "cell is singular along a periodic direction");
    double rs = b->host.rsearch + extra;
    // bins of half the search radius (scan radius 2): 125 bins cover 15.6 r^3 instead of 27 r^3 for 27 full-size bins
    const double bin_frac = 0.5;
    if (n_per) {
        reference_factors(cell, b->r_cut, g.fac);
        for (int k = 0; k < 3; k++) if (!g.per[k]) g.fac[k] = 0;
    }
    // perpendicular heights of the effective cell
    double nrm[3][3];
    cross3(eff + 3, eff + 6, nrm[0]); cross3(eff + 6, eff, nrm[1]); cross3(eff, eff + 3, nrm[2]);
    double vol = std::fabs(dot3(eff, nrm[0]));
    int nb_np = std::max(1, std::min(32, (int)std::cbrt((double)std::max(1, n) / 4.0)));
    long long nbins = 1;
    for (int k = 0; k < 3; k++) {
        double h = vol / norm3(nrm[k]);
        g.cnt[k] = g.per[k] ? 2 * g.fac[k] + 1 : 1;
        if (g.per[k]) {
            int nb = (int)std::floor(h / (rs * bin_frac));
            nb = std::max(1, std::min(nb, 256));
            g.nb[k] = nb;
            g.rad[k] = (int)std::ceil(rs / (h / nb) - 1e-12);
            if (g.rad[k] < 1) g.rad[k] = 1;
            g.binw[k] = 1.0 / nb;
            if (g.fac[k] > 400) return fail(c, UF3_EINVAL, "cell is too small relative to the cutoff");
            // atoms inside a window of fractional width fac + 1 - r_cut / h around the cell (>= 1: the cell itself always
            // is) are at most fac images apart whenever they are within r_cut of each other
            const double w = g.fac[k] + 1.0 - b->r_cut / h - 1e-9;
            g.win_lo[k] = 0.5 - 0.5 * w; g.win_hi[k] = 0.5 + 0.5 * w;
        } else {
            g.win_lo[k] = -1e300; g.win_hi[k] = 1e300;
            g.nb[k] = nb_np;
            g.rad[k] = 1;
            g.binw[k] = rs / h;      // fractional width of a bin of real width rs
        }
        nbins *= g.nb[k];
    }
    long long m = (long long)g.cnt[0] * g.cnt[1] * g.cnt[2] * n;
    if (m >= (1LL << 31)) return fail(c, UF3_EINVAL, "reference supercell index exceeds int32");
    g.bin_base = bin_cursor;
    if (nbins + bin_cursor >= (1LL << 30)) return fail(c, UF3_EINVAL, "too many cell-list bins");
    bin_cursor += (int)nbins;
    return UF3_OK;
}

// ------------------------------------------------------------------------------ shared pipeline
struct Prepared {
    int natoms = 0, n_frames = 0, nbins = 0;
    double max_density = 0;
    CellList cl;
    N3Lists n3;
    const FrameGeom *geoms = nullptr;
    const int *frame_of = nullptr;
    const signed char *spec = nullptr;
    const int64_t *d_offsets = nullptr;
    size_t geo_bytes = 0;       // FrameGeom [n_frames] | atom offsets [n_frames + 1] behind `geoms`, one block
    bool deferred = false;      // the list-capacity / error flags of this build have not been read yet
    bool flags_zeroed = false;  // the cell-list stage has already zeroed the n3 / candidate status words
    bool small_prepared = false; // ... by the one-workgroup kernel, which also zeroes md_build's list-length report
};

#define UF3_VIRIAL_OUTSIDE_MSG "uf3_featurize_virial: an atom lies far outside its cell; wrap the atoms into the cell first (virial rows follow the energy row, the image-range rule of the force rows has no strain analogue)"
static int check_flags(uf3_ctx *c) {
    if (!c->flags.p) return UF3_OK;
    int fl[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpy(fl, c->flags.p, sizeof(fl), hipMemcpyDeviceToHost));
    if (fl[ST_ERROR] == 2) { hipMemset(c->flags.p, 0, sizeof(fl)); return fail(c, UF3_ESPECIES, "frame contains an element outside the basis"); }
    if (fl[ST_ERROR] == 1) { hipMemset(c->flags.p, 0, sizeof(fl)); return fail(c, UF3_EINVAL, "atom too far outside the periodic cell (|wrap| > 250)"); }
    return UF3_OK;
}

// Status words of earlier asynchronous featurizer calls (error flag | 3-body list length needed | candidates needed).
// wait = false: only the slots whose copy has completed are looked at.  Returns the first problem found, once.
static int poll_pending(uf3_ctx *c, bool wait, bool remember) {
    int rc = UF3_OK;
    for (int q = 0; q < uf3_ctx::N_PENDING; q++) {
        uf3_ctx::Pending &p = c->pending_chk[(c->pending_head + q) % uf3_ctx::N_PENDING];
        if (!p.live) continue;
        if (wait) { HIPCHK(c, hipEventSynchronize(p.ev)); }
        else if (hipEventQuery(p.ev) != hipSuccess) continue;
        p.live = false;
        const int *fl = (const int *)c->pin_flags.p + 8 * ((c->pending_head + q) % uf3_ctx::N_PENDING);
        if (fl[0] == 2 && !rc) rc = fail(c, UF3_ESPECIES, "frame contains an element outside the basis (earlier asynchronous call)");
        else if (fl[0] == 1 && !rc) rc = fail(c, UF3_EINVAL, "atom too far outside the periodic cell (|wrap| > 250) (earlier asynchronous call)");
        bool grown = false;
        // (with headroom: a data set ordered by increasing density would otherwise overflow chunk after chunk)
        if (p.has3 && fl[1] > p.cap) { c->n3_cap = std::max(c->n3_cap, (std::max(fl[1] + 8, p.cap + p.cap / 4) + 7) / 8 * 8); grown = true; }
        if (fl[2] > p.cand) { c->cand_cap = std::max(c->cand_cap, (std::max(fl[2] + 16, p.cand + p.cand / 4) + 7) / 8 * 8); grown = true; }
        if (fl[3] > p.xcap) { c->n3x_cap = std::max(c->n3x_cap, std::min(248, (fl[3] + 8 + 7) / 8 * 8)); grown = true; }
        if (fl[4] && p.virial && !rc) rc = fail(c, UF3_EINVAL, UF3_VIRIAL_OUTSIDE_MSG " (earlier asynchronous call)");
        if (fl[4] && !p.img) { c->img_mode = true; grown = true; }      // (its 3-body launches left without writing rows)
        else if (!fl[4] && p.img_launch) c->img_mode = false;            // back to the ordinary launches
        if (grown && !rc)
            rc = fail(c, UF3_ERETRY, "an earlier asynchronous featurizer call overflowed its neighbour capacities: its outputs are "
                                     "invalid; the capacities have been raised, repeat the work since the last synchronisation");
    }
    if (rc && c->flags.p) hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream);
    if (rc && remember && !c->async_bad) { c->async_bad = rc; c->async_msg = c->err; }
    return rc;
}

static int n3_alloc(uf3_ctx *c, int natoms, int cap, N3Lists &n3) {
    HIPCHK(c, c->n3_cnt.ensure(sizeof(int) * (size_t)natoms * (UF3_MAX_SPECIES + 2)));
    HIPCHK(c, c->n3_dbl.ensure(sizeof(N3Entry) * (size_t)natoms * cap));
    n3.cap = cap;
    c->n3_last_cap = cap; c->n3_last_natoms = natoms;
    n3.cnt = c->n3_cnt.as<int>();
    n3.spoff = n3.cnt + natoms;
    n3.ent = c->n3_dbl.as<N3Entry>();
    return UF3_OK;
}

// The capacity a list gets after one of `need` entries outgrew it: 8 entries of headroom, a multiple of 8 (the evaluator's 3-body
// lists and the MD route's superset lists alike)
static int cap_for(int need) { return (need + 8 + 7) / 8 * 8; }

static int n3_cap_estimate(const uf3_basis *b, double dens) {
    double r = b->host.rmax3;
    double est = dens > 0 ? 4.18879 * r * r * r * dens : 24.0;
    return std::max(16, ((int)(est * 1.8) + 8 + 7) / 8 * 8);
}

// The density estimate is generous: after the first successful build later calls pad to what that batch really
// needed (a batch that needs more trips the overflow path and grows the capacity again).
static int n3_tune(uf3_ctx *c, const N3Lists &n3, int natoms) {
    hipStream_t st = c->stream;
    int *flags = c->flags.as<int>();
    c->n3_tuned = true;
    HIPCHK(c, hipMemsetAsync(flags + ST_N3_SEEN, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_max_count, dim3(64), dim3(256), 0, st, n3.cnt, natoms, flags + ST_N3_SEEN);
    int seen = 0;
    HIPCHK(c, hipMemcpyAsync(&seen, flags + ST_N3_SEEN, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    c->n3_cap = std::max(8, (seen + 7) / 8 * 8);
    return UF3_OK;
}

// 3-body lists of the HALO of the block of atoms [lo, hi), whose own lists exist: the atoms outside the block that those
// lists mention are marked and collected on the device (c->halo: marks [natoms] | indices [natoms] | count), then built
static int build_halo_lists(uf3_basis *b, const Prepared &P, const N3Lists &n3, const double *d_pos, int lo, int hi,
                            bool marks_zeroed = false) {
    uf3_ctx *c = b->ctx;
    hipStream_t st = c->stream;
    const int natoms = P.natoms, nb_ = hi - lo;
    HIPCHK(c, c->halo.ensure(sizeof(int) * ((size_t)natoms + 4)));
    int *mark = c->halo.as<int>(), *range = mark + natoms;
    if (!marks_zeroed) HIPCHK(c, hipMemsetAsync(mark, 0, sizeof(int) * (size_t)natoms, st));
    if (nb_ <= 0 || natoms - nb_ <= 0) return UF3_OK;
    const size_t lds = (size_t)n3.cap * (8 + 32 + 16);
    hipLaunchKernelGGL(k_mark_halo, dim3((nb_ + 3) / 4), dim3(256), 0, st, n3, lo, hi, mark, range);
    // (one workgroup per atom outside the block; the unmarked ones leave at once)
    hipLaunchKernelGGL(k_build_n3, dim3(natoms - nb_), dim3(64), lds, st, b->dev, P.geoms, P.frame_of, P.cl, n3, d_pos,
                       natoms, c->flags.as<int>() + 1, 0, (const int *)mark, (const int *)range);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

// cell list + 3-body neighbour lists for a batch (positions / species already in HBM)
// defer_check: once the list capacity is tuned, do not wait for the build's flags; the caller reads them together
// with its results and repeats the call if the lists overflowed (all kernels are safe on clipped lists)
// n3_lo / n3_hi: build the 3-body lists only for the atoms [n3_lo, n3_hi) and for their halo (the atoms in their
// lists): what a rank of a decomposed frame needs (n3_hi < 0: every atom)
static int prepare(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, bool need_n3,
                   Prepared &P, bool defer_check = false, int64_t n3_lo = 0, int64_t n3_hi = -1, double extra_radius = 0.0) {
    uf3_ctx *c = b->ctx;
    c->md.flags_clean = false;          // (the cell-list stage and what follows it use the status words)
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || !fr->cells || !fr->pbc)
        return fail(c, UF3_EINVAL, "bad uf3_frames");
    if (fr->atom_offsets[0] != 0) return fail(c, UF3_EINVAL, "atom_offsets[0] must be 0");
    int nf = fr->n_frames;
    int64_t total = fr->atom_offsets[nf];
    if (total < 1 || total >= (1LL << 31) / 8) return fail(c, UF3_EINVAL, "batch must hold 1 .. 2^28 atoms");
    for (int f = 0; f < nf; f++)
        if (fr->atom_offsets[f + 1] < fr->atom_offsets[f]) return fail(c, UF3_EINVAL, "atom_offsets must be non-decreasing");
    int natoms = (int)total;
    std::vector<FrameGeom> geoms(nf);
    int bin_cursor = 0;
    double dens = 0;
    for (int f = 0; f < nf; f++) {
        int rc = make_geom(c, b, fr, f, geoms[f], bin_cursor, extra_radius);
        if (rc) return rc;
        int n = geoms[f].atom_hi - geoms[f].atom_lo;
        double vol = 0;
        if (geoms[f].per[0] && geoms[f].per[1] && geoms[f].per[2]) {
            double cr[3];
            cross3(geoms[f].cell + 3, geoms[f].cell + 6, cr);
            vol = std::fabs(dot3(geoms[f].cell, cr));
        }
        if (vol > 0) dens = std::max(dens, n / vol);
    }
    int nbins = bin_cursor;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    // frame geometry | atom offsets: one block, staged in pinned memory (the copy is asynchronous; the event tells
    // the next call when the staging block may be overwritten)
    const size_t geo_bytes = (sizeof(FrameGeom) * nf + 15) / 16 * 16, off_bytes = sizeof(int64_t) * (nf + 1);
    const FrameGeom *d_geoms;
    const int64_t *d_offsets;
    const int4 *host_block = nullptr;           // != null: k_prepare_small fetches the staged block itself
    size_t host_block_bytes = 0;
    if (c->staged_in_dev && d_pos == (const double *)c->stage_cur) {
        // positions | species are in the device block already (upload_frames, through the BAR): geometry | offsets behind them
        const size_t at = c->staged_in_dev;
        c->staged_in_dev = 0;
        std::memcpy(c->stage_cur + at, geoms.data(), sizeof(FrameGeom) * nf);
        std::memcpy(c->stage_cur + at + geo_bytes, fr->atom_offsets, off_bytes);
        uf3_store_fence();
        d_geoms = (const FrameGeom *)((const char *)c->stage_cur + at);
        d_offsets = (const int64_t *)((const char *)c->stage_cur + at + geo_bytes);
    } else if (c->pin_in_pending && d_pos == (const double *)c->stage_cur) {
        // small batch staged by upload_frames: positions | species | geometry | offsets leave pin_in in one piece -- fetched by
        // the cell-list kernel itself when that is the one-workgroup kernel, by one copy otherwise
        const size_t at = c->pin_in_pending;
        std::memcpy((char *)c->pin_in.p + at, geoms.data(), sizeof(FrameGeom) * nf);
        std::memcpy((char *)c->pin_in.p + at + geo_bytes, fr->atom_offsets, off_bytes);
        if (natoms <= UF3_SMALL_ATOMS && !uf3_env("UF3_NO_SMALL_PREPARE") && !uf3_env("UF3_NO_ZERO_COPY")) {
            host_block = (const int4 *)c->pin_in.p;
            host_block_bytes = (at + geo_bytes + off_bytes + 15) / 16 * 16;
        } else {
            HIPCHK(c, hipMemcpyAsync(c->stage_cur, c->pin_in.p, at + geo_bytes + off_bytes, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipEventRecord(c->pin_in_done, st));
        }
        c->pin_in_pending = 0;
        d_geoms = (const FrameGeom *)((const char *)c->stage_cur + at);
        d_offsets = (const int64_t *)((const char *)c->stage_cur + at + geo_bytes);
    } else {
        HIPCHK(c, c->geoms.ensure(geo_bytes + off_bytes));
        HIPCHK(c, hipEventSynchronize(c->pin_geo_done));
        HIPCHK(c, c->pin_geo.ensure(geo_bytes + off_bytes));
        std::memcpy(c->pin_geo.p, geoms.data(), sizeof(FrameGeom) * nf);
        std::memcpy((char *)c->pin_geo.p + geo_bytes, fr->atom_offsets, off_bytes);
        HIPCHK(c, hipMemcpyAsync(c->geoms.p, c->pin_geo.p, geo_bytes + off_bytes, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipEventRecord(c->pin_geo_done, st));
        d_geoms = c->geoms.as<FrameGeom>();
        d_offsets = (const int64_t *)((const char *)c->geoms.p + geo_bytes);
    }
    size_t na = (size_t)natoms;
    HIPCHK(c, c->frame_of.ensure(4 * na)); HIPCHK(c, c->atom_bin.ensure(4 * na)); HIPCHK(c, c->atom_wrap.ensure(4 * na));
    HIPCHK(c, c->spec.ensure(na)); HIPCHK(c, c->key_in.ensure(4 * na)); HIPCHK(c, c->val_out.ensure(4 * na));
    HIPCHK(c, c->bin_start.ensure(4 * ((size_t)nbins + 2)));
    HIPCHK(c, c->slots.ensure(sizeof(SlotRec) * na));
    if (!c->flags.p) { HIPCHK(c, c->flags.ensure(64)); HIPCHK(c, hipMemsetAsync(c->flags.p, 0, 64, st)); }
    int *flags = c->flags.as<int>();

    Timed tm(c, T_NBR);
    int tb = 256, gb = (natoms + tb - 1) / tb;
    if (natoms <= UF3_SMALL_ATOMS && !uf3_env("UF3_NO_SMALL_PREPARE")) {
        // an MD step: the whole cell-list stage in one workgroup (and the status words of the launches that follow zeroed)
        hipLaunchKernelGGL(k_prepare_small, dim3(1), dim3(natoms <= 256 ? 256 : 1024), 0, st, b->dev, d_geoms, d_offsets, nf,
                           natoms, nbins, d_pos, d_z, c->frame_of.as<int>(), c->atom_bin.as<int>(), c->atom_wrap.as<int>(),
                           c->spec.as<signed char>(), c->bin_start.as<int>(), c->slots.as<SlotRec>(), flags, 2,
                           host_block, (int4 *)c->stage_cur, (int)(host_block_bytes / 16));
        P.small_prepared = true;
        if (host_block) c->pin_in_busy = true;     // (until the caller's wait for the stream: upload_frames checks)
        // (host_block: no event behind the kernel -- a record between two launches costs the next kernel ~5 us of dispatch
        // latency, and the only caller on this path, the synchronous evaluator entry, waits for the stream before it returns)
        P.flags_zeroed = true;
    } else {
    // n3 need | candidate need | extension-list need | "some atom outside its cell" (k_frame_bins): one fill for all four (the
    // launches behind this stage then need none of their own; every fill is a small kernel on the stream)
    HIPCHK(c, hipMemsetAsync(flags + 1, 0, 4 * sizeof(int), st));
    P.flags_zeroed = true;
    // counting sort by global bin: counts (k_frame_bins) -> exclusive scan = bin starts -> fill -> per-bin order + slot records
    // (k_bin_fill takes every count back to zero: the buffer is cleared only where it has not been through a fill yet)
    {
        const void *before = c->bin_cnt.p;
        HIPCHK(c, c->bin_cnt.ensure(4 * ((size_t)nbins + 8)));
        if (c->bin_cnt.p != before) c->bin_cnt_clean = 0;
        if ((size_t)nbins + 1 > c->bin_cnt_clean) {
            HIPCHK(c, hipMemsetAsync(c->bin_cnt.p, 0, (4 * ((size_t)nbins + 1) + 15) / 16 * 16, st));      // (whole 16-byte pieces: one fill kernel)
            c->bin_cnt_clean = (size_t)nbins + 1;
        }
    }
    hipLaunchKernelGGL(k_frame_bins, dim3(gb), dim3(tb), 0, st, b->dev, d_geoms,
                       d_offsets, nf, natoms, d_pos, d_z, c->frame_of.as<int>(), c->atom_bin.as<int>(),
                       c->atom_wrap.as<int>(), c->spec.as<signed char>(), c->key_in.as<int>(), c->bin_cnt.as<int>(), flags);
    // (up to 16 384 bins -- frames of about 20 k atoms: one workgroup walking 36 k counts of the 50 k-atom frame took 40 us longer than the
    // library scan's two launches)
    if ((size_t)nbins + 1 <= 16384)
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, st, (const int *)c->bin_cnt.as<int>(), c->bin_start.as<int>(), nbins + 1);
    else {
        size_t tmp_bytes = 0;
        HIPCHK(c, rocprim::exclusive_scan(nullptr, tmp_bytes, c->bin_cnt.as<int>(), c->bin_start.as<int>(), 0, (size_t)nbins + 1,
                                           rocprim::plus<int>(), st));
        HIPCHK(c, c->sort_tmp.ensure(tmp_bytes));
        HIPCHK(c, rocprim::exclusive_scan(c->sort_tmp.p, tmp_bytes, c->bin_cnt.as<int>(), c->bin_start.as<int>(), 0, (size_t)nbins + 1,
                                           rocprim::plus<int>(), st));
    }
    hipLaunchKernelGGL(k_bin_fill, dim3(gb), dim3(tb), 0, st, c->key_in.as<int>(), natoms, c->bin_start.as<int>(),
                       c->bin_cnt.as<int>(), c->val_out.as<int>());
    hipLaunchKernelGGL(k_bin_finish, dim3((nbins + tb - 1) / tb), dim3(tb), 0, st, nbins, c->bin_start.as<int>(),
                       c->val_out.as<int>(), d_pos, c->atom_wrap.as<int>(), c->spec.as<signed char>(), c->slots.as<SlotRec>());
    }
    HIPCHK(c, hipGetLastError());

    P.natoms = natoms; P.n_frames = nf; P.nbins = nbins; P.max_density = dens;
    P.geo_bytes = geo_bytes + off_bytes;
    P.geoms = d_geoms;
    P.frame_of = c->frame_of.as<int>();
    P.spec = c->spec.as<signed char>();
    P.d_offsets = d_offsets;
    P.cl.bin_start = c->bin_start.as<int>(); P.cl.slots = c->slots.as<SlotRec>();
    P.cl.atom_bin = c->atom_bin.as<int>(); P.cl.atom_wrap = c->atom_wrap.as<int>();
    std::memset(&P.n3, 0, sizeof(P.n3));
    if (need_n3 && b->host.T > 0) {
        // capacity: remembered from earlier calls, else a density estimate; overflow -> grow and redo
        if (c->n3_cap == 0) c->n3_cap = n3_cap_estimate(b, dens);
        for (int attempt = 0; attempt < 6; attempt++) {
            int cap = c->n3_cap;
            int rc = n3_alloc(c, natoms, cap, P.n3);
            if (rc) return rc;
            HIPCHK(c, hipMemsetAsync(flags + 1, 0, sizeof(int), st));
            size_t lds = (size_t)cap * (8 + 32 + 16);
            if ((int)lds > c->lds_max) return fail(c, UF3_EOVERFLOW, "3-body neighbour list does not fit in LDS");
            const bool block_only = n3_hi >= 0 && !(n3_lo == 0 && n3_hi == natoms) && !uf3_env("UF3_NO_HALO");
            if (!block_only)
                hipLaunchKernelGGL(k_build_n3, dim3(natoms), dim3(64), lds, st, b->dev, P.geoms, P.frame_of, P.cl, P.n3,
                                   d_pos, natoms, flags + 1, 0, (const int *)nullptr, (const int *)nullptr);
            else if (n3_hi > n3_lo) {
                // the block, then the atoms its lists mention (marked and collected on the device), nothing else
                const int nb_ = (int)(n3_hi - n3_lo);
                HIPCHK(c, hipMemsetAsync(P.n3.cnt, 0, sizeof(int) * (size_t)natoms, st));      // lists not built: empty
                hipLaunchKernelGGL(k_build_n3, dim3(nb_), dim3(64), lds, st, b->dev, P.geoms, P.frame_of, P.cl, P.n3,
                                   d_pos, natoms, flags + 1, (int)n3_lo, (const int *)nullptr, (const int *)nullptr);
                int rh = build_halo_lists(b, P, P.n3, d_pos, (int)n3_lo, (int)n3_hi);
                if (rh) return rh;
            }
            HIPCHK(c, hipGetLastError());
            if (defer_check && c->n3_tuned) { P.deferred = true; return UF3_OK; }
            int fl[4] = {0, 0, 0, 0};                                   // error flag | list length needed | .. | ..
            HIPCHK(c, hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (fl[0]) return check_flags(c);
            const int need = fl[1];
            if (need <= cap) {
                if (!c->n3_tuned) { int rt = n3_tune(c, P.n3, natoms); if (rt) return rt; }
                return UF3_OK;
            }
            c->n3_tuned = true;
            c->n3_cap = (need + 8 + 7) / 8 * 8;
        }
        return fail(c, UF3_EOVERFLOW, "3-body neighbour capacity did not converge");
    }
    return UF3_OK;
}

// ------------------------------------------------------------------------------ featurize
static int ensure_frag(uf3_ctx *c);

// LDS bytes of one featurizer workgroup; must mirror the carve at the top of k_featurize
// (FeatShape: what a call's launches have in common -- features, species, list and candidate capacities, the energy row in LDS,
// pair columns; the knot records in LDS, the mode and its staging area differ from launch to launch)
struct FeatShape { int F, S, cap, cand_cap; bool e_lds; int n_pair_cols; };
static size_t feat_lds_bytes(const FeatShape &sh, size_t n_recs, int mode, int dense_stage) {
    const bool dense = mode >= 6;
    const int S = sh.S, cap = sh.cap, n_pair_cols = sh.n_pair_cols;
    const int F = mode == 0 ? S + n_pair_cols : sh.F;            // (the pair launch's energy row: one-body + pair columns)
    size_t e_d = sh.e_lds ? (size_t)F + (F & 1) : 0;
    size_t cand_d = (size_t)sh.cand_cap * CAND_STRIDE;
    size_t pair_buf_d = std::max(4 * (size_t)n_pair_cols, (3 * (size_t)cap + 1) / 2 + 2);
    size_t stage_d = mode == 0 ? cand_d + pair_buf_d
                     : (dense ? (size_t)dense_stage : (size_t)NSTAGE * ITEM_STRIDE);
    size_t list_d = mode == 0 ? 0 : 5 * (size_t)cap + ((5 * cap) & 1);
    size_t geo_d = dense ? (size_t)7 * GEO_N : 0;
    size_t per_wave_d = list_d + stage_d + (stage_d & 1) + geo_d;
    size_t per_wave_i = mode == 0 ? 0 : 3 * (size_t)cap + 2 * ((size_t)cap + 1) + (UF3_MAX_SPECIES + 2) +
                                        (size_t)cap * (S + 1);
    size_t ints = ((size_t)WPB * per_wave_i + 3) & ~(size_t)3;
    return (e_d + WPB * per_wave_d) * 8 + ints * 4 + n_recs * sizeof(KnotRec) + 32;
}

// LDS footprint of k_featurize3 at list capacity cap (uf3_feat3.h): grows by ~168 B (3-row windows) to ~264 B (6-row windows)
// per list entry and wave -- faster than the launches it replaces, so uf3_featurize_dev asks BEFORE it chooses the launch
static void feat3_shape(const uf3_basis *b, int &ep, int &stage) {      // (the records' headers travel in registers: uf3_feat3.h)
    ep = std::max(3, b->f3_ext_p);
    switch (ep) {
        case 3: stage = F3Cfg<3, 1>::STAGE; break;
        case 4: stage = F3Cfg<4, 2>::STAGE; break;
        case 5: stage = F3Cfg<5, 3>::STAGE; break;
        default: stage = F3Cfg<6, 3>::STAGE; break;
    }
}
static size_t feat3_lds_bytes(const uf3_basis *b, int cap, bool e_lds) {
    int ep, stage;
    feat3_shape(b, ep, stage);
    const int F = b->host.F, S = b->host.S;
    const size_t e_d = e_lds ? (size_t)F + (F & 1) : 0, rows_d = (size_t)b->n_f3rows * 18;
    const size_t list_d = 5 * (size_t)cap + ((5 * cap) & 1), tq_d = (size_t)cap * ep * 4, stage_d = (size_t)stage;
    const size_t per_wave_i = 2 * (size_t)cap + 2 * ((size_t)cap + 1) + (UF3_MAX_SPECIES + 2) + (size_t)cap * (S + 1) + (size_t)cap;
    const size_t ints = ((size_t)WPB * per_wave_i + 3) & ~(size_t)3;
    return (e_d + rows_d + WPB * (list_d + tq_d + stage_d)) * 8 + ints * 4 + (size_t)b->n_f3src * 2 + 32;
}
#define UF3_LDS_LIMIT ((size_t)160 * 1024 - 512)

static int featurize_dev_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                              double *d_xe, double *d_xf, int64_t ld, double *d_xv = nullptr);

extern "C" int uf3_featurize_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                 double *d_xe, double *d_xf) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return featurize_dev_impl(b, fr, d_pos, d_z, d_xe, d_xf, b->host.F);
}

// force rows `ld` doubles apart (ld >= F; the columns F .. ld of a row are not touched): with ld a multiple of 16 every row
// starts on a 128-byte line -- rows of F = 434 or 1798 doubles do not, and the partial lines at their ends are written twice
extern "C" int uf3_featurize_ld_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                    double *d_xe, double *d_xf, int64_t ld) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (ld < b->host.F || ld > (1 << 24)) return fail(b->ctx, UF3_EINVAL, "uf3_featurize_ld_dev: ld must be >= the number of features");
    return featurize_dev_impl(b, fr, d_pos, d_z, d_xe, d_xf, ld);
}

// virial rows (uf3_virial_rows.h): x_v [n_frames][6][F] = the strain derivative of the energy row, by launches of their own
// behind the featurizer's (whose instances, registers and LDS carve they leave alone)
extern "C" int uf3_featurize_virial_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                        double *d_xe, double *d_xf, double *d_xv) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (!d_xv) return fail(b->ctx, UF3_EINVAL, "uf3_featurize_virial_dev: null x_v");
    return featurize_dev_impl(b, fr, d_pos, d_z, d_xe, d_xf, b->host.F, d_xv);
}

// LDS bytes of one k_virial_rows workgroup WITHOUT its row set; must mirror the carve at the top of the kernel
static size_t virial_lds_bytes(int cap, int n_pair_cols, int mode) {
    const size_t list_d = mode == 0 ? 0 : 4 * (size_t)cap;
    const size_t stage_d = mode == 0 ? 6 * (size_t)n_pair_cols : (size_t)VSTAGE * VREC_STRIDE;
    const size_t per_wave_d = list_d + stage_d + ((list_d + stage_d) & 1);
    const size_t per_wave_i = mode == 0 ? 0 : UF3_MAX_SPECIES + 2;
    return WPB * per_wave_d * 8 + WPB * per_wave_i * 4 + 32;
}
// The six rows live in LDS while the whole carve leaves room for a second workgroup on the CU (half of the 160 KB less the
// allocation granule, the target the featurizer's 3-body launches use): four waves alone would leave the walk's latency
// uncovered.  Past that every add goes straight to HBM -- the e_direct rule (48 KB for the one energy row) with its threshold
// moved to (this limit - the launch's other LDS) / 6 per row.
#define UF3_VROWS_LDS (((size_t)160 * 1024 - 1024) / 2)

// Which instances of the featurizer's kernels the library holds -- the dispatch below (launch_featurize, feat3_stage,
// virial_rows_stage) names exactly these (the evaluator's k_eval: above launch_eval):
//   k_featurize<WANT_E, WANT_F, RECS_LDS, MODE, IMG>  WANT_E or WANT_F, modes 0 .. 9; modes 10 and 11 (mode 7 with grouped windows
//       only, mode 9 banded only) for force launches only.  IMG launches (the image-range rule) are force launches of modes
//       1 .. 9 and carry the knot records in HBM only
//   k_featurize3<WANT_E, EF, NR, CAP>  (EF, NR) = (3, 1), (4, 2), (5, 3), (6, 3); the list capacity at run time (CAP 0) or 16 as a
//       constant, 24 and 32 for EF = 3 only
//   k_virial_rows<MODE>  modes 0 .. 5
static int launch_featurize(uf3_ctx *c, bool want_e, bool want_f, bool recs_lds, int launch_mode, bool img, unsigned grid,
                            size_t lds, const FeatArgs &A) {
    auto go = [&](auto E, auto Fo, auto R, auto M, auto I) {
        HIPCHK(c, (launch_lds<k_featurize<E, Fo, R, M, I>>(c, dim3(grid), dim3(WPB * WAVE), lds, A)));
        return (int)UF3_OK;
    };
    constexpr std::true_type yes{}; constexpr std::false_type no{};
    if (img && launch_mode != 0)         // (the pair launch has no image-range variant)
        return with_int(launch_mode, std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9>{}, [&](auto M) {
            return with_bool(want_e, [&](auto E) { return go(E, yes, no, M, yes); }); });
    if (launch_mode >= 10)
        return with_int(launch_mode, std::integer_sequence<int, 10, 11>{}, [&](auto M) {
            return with_bool(want_e, [&](auto E) { return with_bool(recs_lds, [&](auto R) { return go(E, yes, R, M, no); }); }); });
    return with_int(launch_mode, std::make_integer_sequence<int, 10>{}, [&](auto M) {
        return with_bool(recs_lds, [&](auto R) {
            if (!want_f) return go(yes, no, R, M, no);
            return with_bool(want_e, [&](auto E) { return go(E, yes, R, M, no); }); }); });
}

// The plan of one k_featurize launch: the instance, what of the tables goes to LDS, the bytes.  Modes that are not dense leave
// the dense fields and dsrc_lds as the launch before left them in A (their kernels do not read them).
struct FeatPlan {
    int launch_mode;                    // the instance's MODE
    int trio_rec_lo;                    // first knot record (window row) the launch reads ...
    size_t n_rec_mode;                  // ... and how many of them
    bool recs_lds;                      // those in LDS
    size_t lds, lds_plain, lds_recs;    // dynamic LDS of the launch | without and with the records, where both were looked at
    size_t lds_extra;                   // the source tables' part of it
    int dense_nrec, dense_stage, dsrc_lds, gsrc_lds;      // FeatArgs' fields of these names
};
static FeatPlan feat_plan(const uf3_basis *b, const FeatShape &sh, const FeatArgs &A, int mode, bool want_f, bool img_launch,
                          bool dsrc_ok) {
    FeatPlan p = {};
    const bool dense_mode = mode >= 6;
    // knot records go to LDS when the block then still reaches the occupancy its registers allow
    // (10: mode 7 with grouped windows only -- the force launches of a basis whose mode-7 blocks are all grouped)
    p.launch_mode = (mode == 7 && want_f && b->all_grouped7 && !img_launch) ? 10
                    : ((mode == 9 && want_f && b->all_banded9 && !img_launch) ? 11 : mode);
    // (a grouped-only launch reads the window rows, not the knot records of the legs)
    p.trio_rec_lo = (int)(p.launch_mode == 10 ? b->wrow_lo : b->trio_rec_lo);
    p.n_rec_mode = mode == 0 ? b->n_pair_recs : b->n_recs - (size_t)p.trio_rec_lo;
    p.dense_nrec = A.dense_nrec; p.dense_stage = A.dense_stage;
    p.dsrc_lds = dense_mode ? (dsrc_ok && !(mode == 7 && want_f && b->all_grouped7)) : A.dsrc_lds;
    const bool gsrc_wanted = mode == 7 && want_f && b->dense_grouped[7] && b->n_gsrc > 0 && b->n_gsrc * 2 <= 4096;
    const size_t gsrc_bytes = gsrc_wanted ? b->n_gsrc * 2 : 0;
    p.gsrc_lds = gsrc_wanted;
    p.lds_extra = ((dense_mode && p.dsrc_lds) ? sizeof(int) * b->n_dsrc : 0) + gsrc_bytes;
    const bool recs_allowed = !(img_launch && mode != 0);
    bool found = false;
    if (dense_mode) {
        const int stride = want_f ? b->dense_stride_f[mode] : b->dense_stride[mode];
        // (grouped windows fold from three 16 x 16 tiles side by side: 768 doubles)
        const int dump = want_f && b->dense_grouped[mode] ? std::max(768, b->dense_dump[mode]) : b->dense_dump[mode];
        const bool grouped = want_f && b->dense_grouped[mode];
        const int nrec_max = std::max(4, std::min(DENSE_NREC, 1200 / stride));
        // (+ the padding record of an odd pass; grouped windows: one per odd group, at most 2 + (nr odd))
        auto stage_for = [&](int nr) { return std::max(dump, (nr + (nr & 1) + (grouped ? 2 : 0)) * stride); };
        // (21 records = 63 staging lanes = one walk step: a block of <= 63 items is one step and three passes)
        p.dense_nrec = nrec_max; p.dense_stage = stage_for(nrec_max);
        if (mode <= 7) {
            // records per staging pass: as many as the stage allows; fewer (smaller stage) if that lets a third
            // workgroup onto the CU -- the kernel is latency-bound.  Three workgroups per CU need <= 52 KB each
            // (LDS is granted in coarse granules: 53 KB did not fit).  Candidates in order of preference: the
            // knot records / window rows in LDS first, then more records per pass
            const int tries[3] = {nrec_max, std::min(nrec_max, 20), std::min(nrec_max, 15)};
            const size_t budget = (WPB == 4 ? 52 : 13 * WPB) * 1024;      // (12 waves per CU: 3 x 4 or 2 x 6)
            const bool dsrc_allowed = p.dsrc_lds;
            for (int q = 0; q < 12 && !found; q++) {
                // (the records / window rows in LDS first: a staging lane reads eleven 16-byte pieces of them per pass)
                const int nr = tries[(q % 6) / 2];
                const bool with_recs = q < 6, with_dsrc = (q & 1) == 0;
                if ((with_recs && !recs_allowed) || (with_dsrc && !dsrc_allowed)) continue;
                size_t need = feat_lds_bytes(sh, with_recs ? p.n_rec_mode : 0, mode, stage_for(nr)) +
                              (with_dsrc ? sizeof(int) * b->n_dsrc : 0) + gsrc_bytes;
                if (need <= budget) {
                    found = true; p.recs_lds = with_recs; p.lds = p.lds_recs = need;
                    p.dense_nrec = nr; p.dense_stage = stage_for(nr); p.dsrc_lds = with_dsrc;
                }
            }
        }
    }
    if (!found) {
        p.lds_plain = feat_lds_bytes(sh, 0, mode, p.dense_stage) + p.lds_extra;
        p.lds_recs = feat_lds_bytes(sh, p.n_rec_mode, mode, p.dense_stage) + p.lds_extra;
        const size_t lds_target = (160 * 1024 - 1024) / (mode == 0 ? 4 : 2);
        p.recs_lds = p.lds_recs <= lds_target && recs_allowed;
        p.lds = p.recs_lds ? p.lds_recs : p.lds_plain;
    }
    return p;
}

// Stage 2, 3-body force rows by bond factorisation: one k_featurize3 launch (or two, of which one leaves at once) for all trio
// blocks, behind the pair launch that built the lists of A at capacity `cap`
static int feat3_stage(uf3_basis *b, const FeatArgs &A, int cap) {
    uf3_ctx *c = b->ctx;
    const bool e_lds = A.x_e && !A.e_direct;
    Feat3Args G;
    G.B = b->dev; G.trios = b->d_trios; G.rows = b->d_f3rows; G.n_rows = b->n_f3rows;
    G.fsrc = b->d_f3src; G.trio_fsrc = b->d_f3off; G.n_fsrc = b->n_f3src;
    G.leg_p = b->f3_leg_p; G.leg_n = b->f3_leg_n;
    G.lo_p = b->f3_lo_p; G.ext_p = b->f3_ext_p; G.lo_n = b->f3_lo_n; G.ext_n = b->f3_ext_n;
    G.pr_rows = std::min(b->f3_ext_p, 32 / b->f3_ext_n);
    G.geoms = A.geoms; G.frame_of = A.frame_of; G.n3 = A.n3; G.pos = A.pos; G.spec = A.spec;
    G.x_e = A.x_e; G.x_f = A.x_f; G.ld = A.ld; G.natoms = A.natoms; G.e_direct = A.e_direct; G.skip = A.skip;
    G.sel = A.n3_seen; G.sel_mode = 0; G.sel_cap = 16;
    const int ep = std::max(3, b->f3_ext_p);                    // (the window's rows, as feat3_shape has them)
    // one launch laid out for lists of up to `lcap` entries (the batch's list array keeps the context's capacity as
    // its stride); sel_mode: see Feat3Args
    auto launch_f3 = [&](int lcap, int sel_mode) -> int {
        G.sel_mode = sel_mode;
        const size_t lds = feat3_lds_bytes(b, lcap, e_lds);      // (<= UF3_LDS_LIMIT: checked where feat3 was decided)
        const AtomGrid g = atom_grid(G.natoms, lds, c->n_cu);
        G.atoms_per_block = g.atoms_per_block;
        if (c->env_debug_lds)
            fprintf(stderr, "uf3 featurize3: lds %zu B, cap %d (lists %d apart), selection %d, blocks %u x %d atoms, window %d x %d, %d round(s)\n",
                    lds, lcap, cap, sel_mode, g.grid, G.atoms_per_block, G.ext_p, G.ext_n, b->f3_nr);
        return with_bool(A.x_e != nullptr, [&](auto E) {
        return with_int(ep, std::integer_sequence<int, 3, 4, 5, 6>{}, [&](auto EF) {
        return with_int(lcap, std::integer_sequence<int, 16, 24, 32, 0>{}, [&](auto LC) {
            // the list capacity as a constant where an instance has it: 16, and (the default trims) 24 and 32 -- fcc and denser
            // cells; at run time (0) otherwise
            constexpr int NR = EF == 3 ? 1 : (EF == 4 ? 2 : 3), CAP = (LC == 16 || EF == 3) ? LC : 0;
            HIPCHK(c, (launch_lds<k_featurize3<E, EF, NR, CAP>>(c, dim3(g.grid), dim3(WPB * WAVE), lds, G)));
            return (int)UF3_OK;
        }); }); });
    };
    // The lists of this batch were built just now at the context's capacity -- an estimate on a context's first call,
    // what the densest batch so far needed later on -- but the instance that serves most cells is the one laid out for 16
    // entries (4 workgroups per CU, LDS offsets as immediates).  Which one applies is known on the device only: the list
    // build leaves the batch's longest list in flags[7], and two launches follow of which one leaves at once.
    if (A.n3_seen && cap > 16) {
        const int r1 = launch_f3(16, 1);
        return r1 ? r1 : launch_f3(cap, 2);
    }
    return launch_f3(cap, 0);
}

// Stage 3, virial rows: a k_virial_rows launch per mode of the basis (3-body modes: where lists exist) into d_xv
static int virial_rows_stage(uf3_basis *b, FeatArgs &A, double *d_xv, bool lists) {
    uf3_ctx *c = b->ctx;
    const int F = b->host.F, S = b->host.S;
    for (int vm = 0; vm <= 5; vm++) {
        if (vm && !((b->vmodes & (1 << vm)) && lists && b->host.T > 0)) continue;
        const int fe = vm == 0 ? A.n_pair_cols : F - S - A.n_pair_cols;
        const size_t other = virial_lds_bytes(vm == 0 ? 1 : A.n3.cap, A.n_pair_cols, vm);
        const size_t rows = 6 * ((size_t)fe + (fe & 1)) * 8;
        const int v_direct = rows + other > UF3_VROWS_LDS ? 1 : 0;
        const size_t lds = other + (v_direct ? 0 : rows);
        if (lds > UF3_LDS_LIMIT) return fail(c, UF3_EOVERFLOW, "virial rows: LDS footprint exceeds 160 KB (neighbour count too large)");
        const AtomGrid g = atom_grid(A.natoms, lds, c->n_cu);
        A.atoms_per_block = g.atoms_per_block;
        if (c->env_debug_lds)
            fprintf(stderr, "uf3 virial rows mode %d: lds %zu B, rows in %s (6 x %d columns = %zu B + %zu B other, limit %zu B), "
                    "cap %d, blocks %d x %d atoms\n", vm, lds, v_direct ? "hbm" : "lds", fe, rows, other, (size_t)UF3_VROWS_LDS,
                    A.n3.cap, g.n_blocks, g.atoms_per_block);
        int rc = with_int(vm, std::make_integer_sequence<int, 6>{}, [&](auto M) {
            HIPCHK(c, (launch_lds<k_virial_rows<M>>(c, dim3(g.grid), dim3(WPB * WAVE), lds, A, d_xv, v_direct)));
            return (int)UF3_OK;
        });
        if (rc) return rc;
    }
    return UF3_OK;
}

// The verdict deferred (capacities known from earlier calls: do not wait): the status words follow the launches into a pinned
// slot beside `what`, the call's capacities and routes; the context's next call / uf3_ctx_synchronize looks (UF3_ERETRY on overflow)
static int featurize_defer(uf3_ctx *c, uf3_ctx::Pending what) {
    int slot = -1;
    for (int q = 0; q < uf3_ctx::N_PENDING && slot < 0; q++)
        if (!c->pending_chk[(c->pending_head + q) % uf3_ctx::N_PENDING].live) slot = (c->pending_head + q) % uf3_ctx::N_PENDING;
    if (slot < 0) {        // all slots in flight: wait for the oldest
        int rcw = poll_pending(c, true);
        if (rcw) return rcw;
        slot = c->pending_head;
    }
    HIPCHK(c, c->pin_flags.ensure(sizeof(int) * 8 * uf3_ctx::N_PENDING));
    uf3_ctx::Pending &pd = c->pending_chk[slot];
    if (!pd.ev) HIPCHK(c, hipEventCreateWithFlags(&pd.ev, hipEventDisableTiming));
    HIPCHK(c, hipMemcpyAsync((int *)c->pin_flags.p + 8 * slot, c->flags.p, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(pd.ev, c->stream));
    what.ev = pd.ev; what.live = true;
    pd = what;
    c->pending_head = (slot + 1) % uf3_ctx::N_PENDING;
    return UF3_OK;
}

// The verdict at once: wait for the status words and adapt the context's capacities and routes to them.  redo (false on entry)
// becomes true where the call's launches have to be repeated with what the context has learnt
static int featurize_adapt(uf3_ctx *c, const FeatArgs &A, bool has3, bool want_v, bool img_launch, int cap, bool &redo) {
    const bool want_e = A.x_e != nullptr, want_f = A.x_f != nullptr;
    int fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // error flag, n3 need, candidate need, extension need, atoms far outside
    HIPCHK(c, hipMemcpyAsync(fl, c->flags.p, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (fl[0]) return check_flags(c);
    if (want_v && fl[4]) return fail(c, UF3_EINVAL, UF3_VIRIAL_OUTSIDE_MSG);
    if (has3 && want_f && A.outside && fl[4] && !c->img_mode) { c->img_mode = true; redo = true; }
    else if (img_launch && !fl[4]) c->img_mode = false;                 // (valid all the same) back to the ordinary launches
    if (img_launch && fl[3] > c->n3x_cap) {              // (the extension lists of the image-range launches)
        if (fl[3] > 248) return fail(c, UF3_EOVERFLOW, "extension neighbour lists of atoms far outside their cell exceed 248 entries");
        c->n3x_cap = (fl[3] + 8 + 7) / 8 * 8; redo = true;
    }
    if (has3 && fl[1] > cap) { c->n3_cap = (fl[1] + 8 + 7) / 8 * 8; c->n3_tuned = true; redo = true; }
    if (fl[2] > c->cand_cap) { c->cand_cap = (fl[2] + 16 + 7) / 8 * 8; redo = true; }
    if (redo) return UF3_OK;
    if (has3 && !c->n3_tuned) { int rc = n3_tune(c, A.n3, A.natoms); if (rc) return rc; }
    if (want_e || want_f) c->cand_tuned = true;
    return UF3_OK;
}

static int featurize_dev_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                              double *d_xe, double *d_xf, int64_t ld, double *d_xv) {
    uf3_ctx *c = b->ctx;
    uf3_env_refresh();
    read_f3_env(c);
    if (!d_pos || !d_z) return fail(c, UF3_EINVAL, "null positions / species");
    if (!d_xe && !d_xf && !d_xv) return UF3_OK;
    const bool want_v = d_xv != nullptr;
    // verdicts on earlier asynchronous calls that have arrived: returned to the asynchronous caller (their owner) HERE, so not
    // kept for uf3_ctx_synchronize as well -- a caller that redoes the work would meet the same verdict again after a clean redo
    { int rc0 = poll_pending(c, false, false); if (rc0) return rc0; }
    Prepared P;
    // (lists from k_build_n3 instead: debugging, and virial rows alone -- no pair launch of the featurizer to build them)
    const bool old_n3 = uf3_env("UF3_SEPARATE_N3") != nullptr || (want_v && !d_xe && !d_xf);
    int rc = prepare(b, fr, d_pos, d_z, old_n3, P);       // cell list only: MODE 0 builds the 3-body lists itself
    if (rc) return rc;
    hipStream_t st = c->stream;
    const int F = b->host.F;
    const bool want_e = d_xe != nullptr, want_f = d_xf != nullptr;
    const bool has3 = b->host.T > 0 && !old_n3;
    if (has3 && c->n3_cap == 0) c->n3_cap = n3_cap_estimate(b, P.max_density);
    int cap = 1;
    auto cand_estimate = [&]() {
        double r = b->host.rsearch;
        double est = P.max_density > 0 ? 4.18879 * r * r * r * P.max_density : 64.0;
        return std::max(32, ((int)(est * 1.6) + 16 + 7) / 8 * 8);
    };
    if (c->cand_cap == 0) c->cand_cap = cand_estimate();
    bool caps_reset = false;
    FeatArgs A;
    A.B = b->dev; A.trios = b->d_trios; A.recs = b->d_recs; A.colsrc = b->d_colsrc;
    A.frag = nullptr;
    A.dense_stage = 0; A.dense_nrec = DENSE_NREC;
    A.dsrc = b->d_dsrc; A.n_dsrc = (int)b->n_dsrc;
    A.gsrc = b->d_gsrc; A.n_gsrc = (int)b->n_gsrc; A.gsrc_lds = 0;
    const int dense_modes = (1 << 6) | (1 << 7) | (1 << 8) | (1 << 9);
    const bool dsrc_ok = (b->modes & dense_modes) && b->n_dsrc * sizeof(int) <= 8192;
    A.dsrc_lds = dsrc_ok;
    if (b->modes & dense_modes) { rc = ensure_frag(c); if (rc) return rc; A.frag = c->frag.as<int>(); }
    A.geoms = P.geoms; A.frame_of = P.frame_of; A.cl = P.cl;
    std::memset(&A.n3, 0, sizeof(A.n3));
    A.n3.cap = 1;
    if (old_n3 && P.n3.cap) A.n3 = P.n3;
    A.build_n3 = has3 ? 1 : 0;
    // the block-shared energy row costs 8 F bytes of LDS: past 48 KB the contributions go straight to HBM instead
    A.e_direct = (want_e && (size_t)F * 8 > 48 * 1024) ? 1 : 0;
    A.n3_need = c->flags.as<int>() + 1;
    A.n3_seen = nullptr;
    A.pos = d_pos; A.spec = P.spec; A.x_e = d_xe; A.x_f = d_xf; A.ld = (int)ld; A.natoms = P.natoms;
    A.cand_need = c->flags.as<int>() + 2;
    // (UF3_KEEP_GHOST_TERMS: keep the force terms of ghost-centred triplets whose third atom the reference's image range
    // does not reach -- rows of unwrapped atoms are then the exact gradient of the energy row instead of the reference's)
    A.outside = uf3_env("UF3_KEEP_GHOST_TERMS") ? nullptr : c->flags.as<int>() + 4;
    { const char *e = uf3_env("UF3_DEBUG_SKIP"); A.skip = e ? atoi(e) : 0; }
    for (int attempt = 0; attempt < 6; attempt++) {
        A.cand_cap = c->cand_cap;
        A.n_recs = (int)b->n_recs;
        A.n_pair_recs = (int)b->n_pair_recs;
        A.trio_rec_lo = (int)b->trio_rec_lo;
        A.wrow_base = (int)(b->wrow_lo * 6); A.n_wrows = b->n_wrows;
        A.n_pair_cols = 0;
        for (int p = 0; p < b->host.P; p++) A.n_pair_cols += b->host.pairs[p].nb;
        if (old_n3) cap = A.n3.cap;
        if (has3) {
            cap = c->n3_cap;
            rc = n3_alloc(c, P.natoms, cap, A.n3);
            if (rc) return rc;
        }
        if (want_e) HIPCHK(c, hipMemsetAsync(d_xe, 0, sizeof(double) * (size_t)P.n_frames * F, st));
        if (want_v) HIPCHK(c, hipMemsetAsync(d_xv, 0, sizeof(double) * (size_t)P.n_frames * 6 * F, st));
        if (!P.flags_zeroed || attempt) HIPCHK(c, hipMemsetAsync(A.n3_need, 0, 2 * sizeof(int), st));       // n3_need, cand_need
        const bool img_launch = c->img_mode && has3 && want_f && A.outside;
        if (img_launch) {
            // extension lists for batches with atoms outside their cell (the kernel leaves at once otherwise); storage only
            // once a batch has asked for it (flags[3], through the same retry path as the other capacities)
            const int xcap = c->n3x_cap;
            A.n3.xcap = xcap; A.n3.xent = nullptr; A.n3.xoff = nullptr;
            if (xcap > 0) {
                HIPCHK(c, c->n3x_ent.ensure(sizeof(N3Entry) * (size_t)P.natoms * xcap));
                HIPCHK(c, c->n3x_off.ensure(sizeof(int) * (size_t)P.natoms * (UF3_MAX_SPECIES + 1)));
                A.n3.xent = c->n3x_ent.as<N3Entry>(); A.n3.xoff = c->n3x_off.as<int>();
            }
            hipLaunchKernelGGL(k_build_n3_ext, dim3(std::min(P.natoms, 2048)), dim3(64), (size_t)xcap * (8 + 32 + 12) + 16, st,
                               b->dev, P.geoms, P.frame_of, P.cl, A.n3, d_pos, P.natoms, c->flags.as<int>());
        }
        // 3-body force rows by bond factorisation (k_featurize3) where the basis allows it: one launch for all trio blocks,
        // behind the pair launch that builds the lists
        // (dense or long-range lists, past ~200 entries at the default trims and ~100 on the 6 x 12 windows, do not fit its
        // LDS layout: those calls keep the matrix-core / generic launches, which handled them before k_featurize3 existed)
        FeatShape sh = {F, b->host.S, cap, A.cand_cap, want_e && !A.e_direct, A.n_pair_cols};
        const bool feat3 = b->feat3_ok && want_f && (has3 || old_n3) && !img_launch && cap <= 255 && !c->env_no_feat3 &&
                           feat3_lds_bytes(b, cap, sh.e_lds) <= UF3_LDS_LIMIT;
        // (the pair launch below leaves the batch's longest 3-body list in flags[7] when k_featurize3 can use it: see there)
        A.n3_seen = nullptr;
        if (feat3 && has3 && cap > 16) {
            A.n3_seen = c->flags.as<int>() + 7;
            HIPCHK(c, hipMemsetAsync(A.n3_seen, 0, sizeof(int), st));
        }
        bool restart = false;
        {
            Timed tm(c, T_FEAT);
            for (int mode = 0; mode <= 9; mode++) {
                if (!(b->modes & (1 << mode)) || !(want_e || want_f)) continue;
                if (feat3 && mode >= 1) continue;
                FeatPlan pl = feat_plan(b, sh, A, mode, want_f, img_launch, dsrc_ok);
                A.trio_rec_lo = pl.trio_rec_lo;
                A.dense_nrec = pl.dense_nrec; A.dense_stage = pl.dense_stage; A.dsrc_lds = pl.dsrc_lds; A.gsrc_lds = pl.gsrc_lds;
                if (pl.lds > UF3_LDS_LIMIT && mode == 0 && !c->cand_tuned && c->cand_cap > 64) {
                    // the candidate capacity is still the density ESTIMATE (60 % headroom): a dense frame must not fail on the
                    // guess -- take what fits, the overflow flag reports the true need and the call is repeated with it
                    while (c->cand_cap > 64 && pl.lds > UF3_LDS_LIMIT) {
                        sh.cand_cap = c->cand_cap = (c->cand_cap * 7 / 8 + 7) / 8 * 8;
                        pl.lds = feat_lds_bytes(sh, pl.recs_lds ? pl.n_rec_mode : 0, 0, pl.dense_stage) + pl.lds_extra;
                    }
                    A.cand_cap = c->cand_cap;
                }
                if (pl.lds > UF3_LDS_LIMIT && !caps_reset) {
                    // the capacities are grow-only memories of the densest batch this context has seen: a sparser batch on a wider
                    // basis must not fail on them -- back to this batch's own estimates, once, and the call starts over
                    const int est3 = has3 ? n3_cap_estimate(b, P.max_density) : 0, estc = cand_estimate();
                    if ((has3 && c->n3_cap > est3) || c->cand_cap > estc) {
                        if (has3 && c->n3_cap > est3) { c->n3_cap = est3; c->n3_tuned = false; }
                        if (c->cand_cap > estc) { c->cand_cap = estc; c->cand_tuned = false; }
                        caps_reset = restart = true;
                        break;
                    }
                }
                if (pl.lds > UF3_LDS_LIMIT) return fail(c, UF3_EOVERFLOW, "featurizer LDS footprint exceeds 160 KB (F or neighbour count too large)");
                const AtomGrid g = atom_grid(P.natoms, pl.lds, c->n_cu);
                A.atoms_per_block = g.atoms_per_block;
                if (uf3_env("UF3_DEBUG_LDS"))
                    fprintf(stderr, "uf3 featurize mode %d: lds %zu B (plain %zu, with recs %zu), recs_lds %d, cap %d, cand_cap %d, "
                            "blocks %d x %d atoms, n_recs %zu, dense nrec %d stage %d\n", pl.launch_mode, pl.lds, pl.lds_plain, pl.lds_recs,
                            (int)pl.recs_lds, cap, A.cand_cap, g.n_blocks, g.atoms_per_block, pl.n_rec_mode, A.dense_nrec, A.dense_stage);
                rc = launch_featurize(c, want_e, want_f, pl.recs_lds, pl.launch_mode, img_launch, g.grid, pl.lds, A);
                if (rc) return rc;
            }
            if (feat3 && !restart) { rc = feat3_stage(b, A, cap); if (rc) return rc; }
            if (want_v && !restart) { rc = virial_rows_stage(b, A, d_xv, has3 || old_n3); if (rc) return rc; }
        }
        HIPCHK(c, hipGetLastError());
        if (restart) continue;
        if ((!has3 || c->n3_tuned) && c->cand_tuned && !old_n3) {
            uf3_ctx::Pending pd;
            pd.virial = want_v; pd.cap = cap; pd.cand = c->cand_cap; pd.has3 = has3; pd.xcap = img_launch ? c->n3x_cap : (1 << 30);
            pd.img = img_launch || !(has3 && want_f && A.outside); pd.img_launch = img_launch;
            return featurize_defer(c, pd);
        }
        bool redo = false;
        rc = featurize_adapt(c, A, has3, want_v, img_launch, cap, redo);
        if (rc || !redo) return rc;
    }
    return fail(c, UF3_EOVERFLOW, "neighbour capacities did not converge");
}

// host-buffer helpers
// BAR staging rests on two things the HIP API does not promise: that host stores into a fine-grained device
// allocation, followed by a store fence, are visible to the NEXT kernel launched -- no stale line of the block left in the GPU's
// L2 or scalar cache from the previous launch -- and that this holds with no stream synchronisation in between (the MD steps wait on
// a polled status word).  So the path is gated on a start-up self-test of exactly that sequence, on this device, with this driver:
// 48 rounds of (host writes a new pattern into the block | fence | k_bar_probe reads it with vector AND scalar loads | host polls the
// pinned word the kernel leaves last), patterns compared at the end.  One mismatch, a time-out or any HIP error: bar_ok = false and
// the small batches take the pinned-block route (k_md_fetch / k_prepare_small fetch them) as before round 5.  Costs < 1 ms, once.
static bool bar_self_test(uf3_ctx *c) {
    const int n_words = 2048, rounds = 48;          // (8 KB: what a 128-atom MD step stages is 3.6 KB)
    Buf blk, out;
    PinBuf word;
    bool ok = blk.ensure_fine(4 * (size_t)n_words) == hipSuccess && out.ensure(4 * (size_t)rounds * (n_words + 16)) == hipSuccess &&
              word.ensure(64) == hipSuccess;
    std::vector<unsigned> got;
    if (ok) {
        volatile unsigned *w = (volatile unsigned *)word.p;
        *w = 0;
        std::vector<unsigned> pat(n_words);
        for (int r = 1; r <= rounds && ok; r++) {
            for (int q = 0; q < n_words; q++) pat[q] = 0x9e3779b9u * (unsigned)(r * 4099 + q) + (unsigned)r;
            std::memcpy(blk.p, pat.data(), 4 * (size_t)n_words);
            uf3_store_fence();
            hipLaunchKernelGGL(k_bar_probe, dim3(1), dim3(256), 0, c->stream, (const unsigned *)blk.p, n_words,
                               out.as<unsigned>() + (size_t)(r - 1) * (n_words + 16), (unsigned *)word.p, (unsigned)r);
            ok = hipGetLastError() == hipSuccess;
            const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
            while (ok && __atomic_load_n((const unsigned *)word.p, __ATOMIC_ACQUIRE) != (unsigned)r)
                if (std::chrono::steady_clock::now() > t_end) ok = false;
        }
        ok = hipStreamSynchronize(c->stream) == hipSuccess && ok;
        if (ok) {
            got.resize((size_t)rounds * (n_words + 16));
            ok = hipMemcpy(got.data(), out.p, 4 * got.size(), hipMemcpyDeviceToHost) == hipSuccess;
        }
        for (int r = 1; r <= rounds && ok; r++)
            for (int q = 0; q < n_words + 16 && ok; q++) {
                const int src = q < n_words ? q : q - n_words;
                ok = got[(size_t)(r - 1) * (n_words + 16) + q] == 0x9e3779b9u * (unsigned)(r * 4099 + src) + (unsigned)r;
            }
    }
    (void)hipGetLastError();
    blk.release(); out.release(); word.release();
    if (!ok && uf3_env("UF3_DEBUG_LDS")) fprintf(stderr, "uf3: BAR staging self-test failed on device %d: small batches go through the pinned block\n", c->device);
    return ok;
}

static int upload_frames(uf3_ctx *c, const uf3_frames *fr, const double *pos, const int32_t *z, int &natoms,
                         bool defer_small = false) {
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets) return fail(c, UF3_EINVAL, "bad uf3_frames");
    int64_t total = fr->atom_offsets[fr->n_frames];
    if (total < 1 || total >= (1LL << 28)) return fail(c, UF3_EINVAL, "batch must hold 1 .. 2^28 atoms");
    if (!pos || !z) return fail(c, UF3_EINVAL, "null positions / species");
    natoms = (int)total;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bp = 24 * (size_t)natoms, bz = 4 * (size_t)natoms;
    // (room behind positions | species for the frame geometry: see pin_in_pending)
    const size_t geo_room = 96 + sizeof(FrameGeom) * (size_t)fr->n_frames + 8 * ((size_t)fr->n_frames + 1);
    // small batches of the synchronous evaluator entry: with a large BAR the block is a fine-grained device allocation and the
    // host stores into it directly (write-combined, posted; a store fence; the launches' doorbell follows over the same link) --
    // no kernel or copy that reads the caller's memory.  The entry's previous call has been waited for (pin_in_busy says when an
    // error return skipped that wait): nothing reads the block.  Gated on bar_self_test.
    bool bar = defer_small && c->bar_ok && bp + bz + geo_room <= UF3_BAR_LIMIT;
    if (bar && !c->bar_tested) {
        c->bar_tested = true;
        c->bar_ok = bar = bar_self_test(c);
        if (uf3_env("UF3_BAR_FORCE_FAIL")) c->bar_ok = bar = false;       // (tests: the fall-back route on a box where the test passes)
    }
    // (a block of its own: the big batches' staging block stays ordinary device memory)
    if (bar && c->stage_bar.ensure_fine(bp + bz + geo_room) != hipSuccess) { (void)hipGetLastError(); c->bar_ok = false; bar = false; }
    if (!bar) HIPCHK(c, c->stage_pos.ensure(bp + bz + geo_room));  // positions | species, one block
    c->stage_cur = (char *)(bar ? c->stage_bar.p : c->stage_pos.p);
    c->d_stage_z = (int32_t *)(c->stage_cur + bp);
    c->pin_in_pending = 0;
    c->staged_in_dev = 0;
    if (bar) {
        if (c->pin_in_busy) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->pin_in_busy = false; }
        std::memcpy(c->stage_cur, pos, bp);
        std::memcpy(c->stage_cur + bp, z, bz);
        uf3_store_fence();
        c->staged_in_dev = (bp + bz + 15) / 16 * 16;
        // (kernels that read this block follow; an entry that returns an error behind them never waits for them: the flag stays up
        // until a successful wait clears it, and the next upload waits for the stream before it stores into the block -- above)
        c->pin_in_busy = true;
        return UF3_OK;
    }
    if (bp + bz <= UF3_PIN_LIMIT) {
        // (an entry that returned an error behind a launch reading the staging block directly never waited for it)
        if (c->pin_in_busy) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->pin_in_busy = false; }
        HIPCHK(c, hipEventSynchronize(c->pin_in_done));
        HIPCHK(c, c->pin_in.ensure(bp + bz + geo_room));
        std::memcpy(c->pin_in.p, pos, bp);
        std::memcpy((char *)c->pin_in.p + bp, z, bz);
        if (defer_small && bp + bz + geo_room <= UF3_PIN_LIMIT) { c->pin_in_pending = (bp + bz + 15) / 16 * 16; return UF3_OK; }
        HIPCHK(c, hipMemcpyAsync(c->stage_pos.p, c->pin_in.p, bp + bz, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->pin_in_done, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->stage_pos.p, pos, bp, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_stage_z, z, bz, hipMemcpyHostToDevice, c->stream));
    }
    return UF3_OK;
}

extern "C" int uf3_featurize(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, double *xe,
                             double *xf) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    int natoms = 0;
    poll_pending(c, true);                   // verdicts on earlier asynchronous calls: remembered for uf3_ctx_synchronize, not ours
    int rc = upload_frames(c, fr, pos, z, natoms);
    if (rc) return rc;
    size_t F = (size_t)b->host.F;
    size_t be = xe ? 8 * F * fr->n_frames : 0, bf = xf ? 8 * F * 3 * (size_t)natoms : 0;
    if (be) HIPCHK(c, c->stage_out.ensure(be));
    if (bf) HIPCHK(c, c->stage_out2.ensure(bf));
    for (int attempt = 0; attempt < 6; attempt++) {
        rc = uf3_featurize_dev(b, fr, (const double *)c->stage_cur, c->d_stage_z,
                               be ? c->stage_out.as<double>() : nullptr, bf ? c->stage_out2.as<double>() : nullptr);
        if (rc) return rc;
        if (be) HIPCHK(c, hipMemcpyAsync(xe, c->stage_out.p, be, hipMemcpyDeviceToHost, c->stream));
        if (bf) HIPCHK(c, hipMemcpyAsync(xf, c->stage_out2.p, bf, hipMemcpyDeviceToHost, c->stream));
        rc = sync_own_call(c);
        if (rc != UF3_ERETRY) return rc;     // the lists of this very call overflowed: repeat it with the raised capacities
    }
    return fail(c, UF3_EOVERFLOW, "neighbour capacities did not converge");
}

extern "C" int uf3_featurize_virial(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, double *xe,
                                    double *xf, double *xv) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!xv) return fail(c, UF3_EINVAL, "uf3_featurize_virial: null x_v");
    int natoms = 0;
    poll_pending(c, true);
    int rc = upload_frames(c, fr, pos, z, natoms);
    if (rc) return rc;
    const size_t F = (size_t)b->host.F;
    const size_t be = xe ? 8 * F * fr->n_frames : 0, bf = xf ? 8 * F * 3 * (size_t)natoms : 0, bv = 8 * F * 6 * (size_t)fr->n_frames;
    // (x_e and x_v share one block: stage_out2 belongs to the force rows)
    HIPCHK(c, c->stage_out.ensure(be + bv));
    if (bf) HIPCHK(c, c->stage_out2.ensure(bf));
    double *d_xv = (double *)((char *)c->stage_out.p + be);
    for (int attempt = 0; attempt < 6; attempt++) {
        rc = uf3_featurize_virial_dev(b, fr, (const double *)c->stage_cur, c->d_stage_z,
                                      be ? c->stage_out.as<double>() : nullptr, bf ? c->stage_out2.as<double>() : nullptr, d_xv);
        if (rc) return rc;
        if (be) HIPCHK(c, hipMemcpyAsync(xe, c->stage_out.p, be, hipMemcpyDeviceToHost, c->stream));
        if (bf) HIPCHK(c, hipMemcpyAsync(xf, c->stage_out2.p, bf, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(xv, d_xv, bv, hipMemcpyDeviceToHost, c->stream));
        rc = sync_own_call(c);
        if (rc != UF3_ERETRY) return rc;     // the lists of this very call overflowed: repeat it with the raised capacities
    }
    return fail(c, UF3_EOVERFLOW, "neighbour capacities did not converge");
}

// ------------------------------------------------------------------------------ eval
// ---- MD route: persistent superset lists with a skin (uf3_ctx_md_skin) ----------------------
// The reference's calculator rebuilds supercell, distances and neighbour pairs on every call (calculator.py:124-153,
// 183-343).  An MD loop repeats that work on almost the same positions: with a skin s the context keeps, per atom, every
// neighbour image within r_cut + s of it (k_build_sup: who, which image, reference supercell index, species -- sorted by
// (species, supercell index), no geometry) and a step filters that list by the TRUE distances of the current positions.  The
// survivors come out in the order the rebuild-every-step route sorts its lists into, so a step's result does not depend on
// when the lists were built.  Valid while no atom has moved more than s / 2 from where the lists were built, the cells, the
// offsets and the species are the same: the kernel checks displacement and species, the host the rest.
static bool md_key_matches(const uf3_ctx::MdState &md, const uf3_basis *b, const uf3_frames *fr) {
    if (!md.valid || md.basis != b || !fr || !fr->atom_offsets || !fr->cells || !fr->pbc || fr->n_frames != md.n_frames) return false;
    const size_t nf = (size_t)fr->n_frames;
    return fr->atom_offsets[nf] == md.natoms && !memcmp(fr->atom_offsets, md.offsets.data(), 8 * (nf + 1)) &&
           (md.live || !memcmp(fr->cells, md.cells.data(), 72 * nf)) && !memcmp(fr->pbc, md.pbc.data(), 3 * nf);
}

// cells that live on the device: the host's copy brought up to date (in front of anything that reads the cells on the host)
static int md_live_fetch(uf3_ctx *c, const uf3_frames *fr) {
    HIPCHK(c, hipMemcpyAsync(c->md.live_host, c->md.live_dev, 72 * (size_t)fr->n_frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

// may_defer: the caller's step has a verdict of its own (status words read behind its last kernel) and nothing zeroes them between
// this build and that step -- then a build at a capacity that has held before does not wait for its own report: an overflow
// raises the step's "lists outrun" word (k_sup_reverse), the step is discarded and the repeat builds with the host looking
static int md_build(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, Prepared &P, bool may_defer = false) {
    uf3_ctx *c = b->ctx;
    uf3_ctx::MdState &md = c->md;
    md.valid = false; md.stale = false;
    const bool defer = may_defer && md.cap_tuned && !md.verify_next && md.basis == b && md.cap > 0;
    int rc = md.wrap ? md.wrap(d_pos) : (int)UF3_OK;       // (k_md_snapshot below then sees the wrapped positions)
    if (rc) return rc;
    rc = prepare(b, fr, d_pos, d_z, false, P, false, 0, -1, md.skin);      // cell list at r_cut + skin
    if (rc) return rc;
    hipStream_t st = c->stream;
    const int natoms = P.natoms, nf = P.n_frames;
    const double r_sup = b->host.rsearch + md.skin;
    if (md.cap == 0 || md.basis != b) {
        const double est = P.max_density > 0 ? 4.18879 * r_sup * r_sup * r_sup * P.max_density : 64.0;
        md.cap = std::max(32, ((int)(est * 1.3) + 16 + 7) / 8 * 8);
    }
    int *flags = c->flags.as<int>();
    const double r_sup2 = r_sup * r_sup * (1.0 + 1e-12);
    for (int attempt = 0; ; attempt++) {
        const int cap = md.cap;
        HIPCHK(c, md.ent.ensure(sizeof(SupEntry) * (size_t)natoms * cap));
        HIPCHK(c, md.cnt.ensure(sizeof(int) * (size_t)natoms));
        if (!(P.small_prepared && attempt == 0)) HIPCHK(c, hipMemsetAsync(flags + ST_SUP_NEED, 0, sizeof(int), st));    // (the one-workgroup cell-list kernel has zeroed it)
        const size_t lds = (size_t)cap * 16;
        if ((int)lds > c->lds_max) return fail(c, UF3_EOVERFLOW, "MD neighbour list does not fit in LDS");
        hipLaunchKernelGGL(k_build_sup, dim3((unsigned)((natoms + 7) / 8 * 8)), dim3(64), lds, st, b->dev, P.geoms, P.frame_of, P.cl,
                           d_pos, natoms, r_sup2, md.ent.as<SupEntry>(), md.cnt.as<int>(), cap, flags + ST_SUP_NEED);
        HIPCHK(c, hipGetLastError());
        if (defer) break;
        int fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(c, hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->pin_in_busy = false;
        if (fl[ST_ERROR]) return check_flags(c);
        if (fl[ST_SUP_NEED] <= cap) { md.cap_tuned = true; md.verify_next = false; break; }
        if (attempt >= 5) return fail(c, UF3_EOVERFLOW, "MD neighbour capacity did not converge");
        md.cap = cap_for(fl[ST_SUP_NEED]);
    }
    hipLaunchKernelGGL(k_sup_reverse, dim3((unsigned)(((natoms + 15) / 16 + 7) / 8 * 8)), dim3(256), 0, st, md.ent.as<SupEntry>(),
                       (const int *)md.cnt.as<int>(), md.cap, natoms, P.geoms, P.frame_of, P.spec, (const int *)(flags + ST_SUP_NEED),
                       defer ? flags + ST_MD_OUTRUN : (int *)nullptr);
    HIPCHK(c, hipGetLastError());
    // inbox of every (atom, list position): zeroed when (re)allocated -- stamps start at 1
    {
        const size_t need = 32 * (size_t)natoms * md.cap;
        const void *before = md.inbox.p;
        HIPCHK(c, md.inbox.ensure(need));
        if (md.inbox.p != before || md.inbox_zeroed < need) {
            HIPCHK(c, hipMemsetAsync(md.inbox.p, 0, md.inbox.cap, st));
            md.inbox_zeroed = md.inbox.cap;
        }
    }
    // what a step reads besides the lists: frame geometry | offsets, frame and species of every atom, the positions of the build
    const size_t geo_bytes = (sizeof(FrameGeom) * (size_t)nf + 15) / 16 * 16;
    HIPCHK(c, md.geo.ensure(P.geo_bytes));
    HIPCHK(c, md.frame_of.ensure(4 * (size_t)natoms));
    HIPCHK(c, md.spec.ensure((size_t)natoms));
    HIPCHK(c, md.pos_ref.ensure(24 * (size_t)natoms));
    hipLaunchKernelGGL(k_md_snapshot, dim3((unsigned)std::min<size_t>((6 * (size_t)natoms + 255) / 256, 2048)), dim3(256), 0, st,
                       (const unsigned *)P.geoms, md.geo.as<unsigned>(), P.geo_bytes / 4, (const unsigned *)P.frame_of, md.frame_of.as<unsigned>(),
                       (size_t)natoms, P.spec, md.spec.as<signed char>(), (const unsigned *)d_pos, md.pos_ref.as<unsigned>());
    HIPCHK(c, hipGetLastError());
    md.geo_bytes = geo_bytes;
    md.basis = b; md.natoms = natoms; md.n_frames = nf;
    md.offsets.assign(fr->atom_offsets, fr->atom_offsets + nf + 1);
    md.cells.assign(fr->cells, fr->cells + 9 * (size_t)nf);
    md.pbc.assign(fr->pbc, fr->pbc + 3 * (size_t)nf);
    md.valid = true;
    md.builds++;
    return UF3_OK;
}

// a step on the lists: `P` as the kernels behind it expect it, from the context's persistent copies
static void md_prepared(const uf3_ctx *c, Prepared &P) {
    const uf3_ctx::MdState &md = c->md;
    P = Prepared();
    P.natoms = md.natoms; P.n_frames = md.n_frames;
    P.geoms = md.geo.as<FrameGeom>();
    P.d_offsets = (const int64_t *)((const char *)md.geo.p + md.geo_bytes);
    P.frame_of = md.frame_of.as<int>();
    P.spec = md.spec.as<signed char>();
    P.flags_zeroed = true;
    std::memset(&P.n3, 0, sizeof(P.n3));
    std::memset(&P.cl, 0, sizeof(P.cl));
}

extern "C" int uf3_ctx_md_skin(uf3_ctx *c, double skin) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (!(skin >= 0.0) || skin > 4.0) return fail(c, UF3_EINVAL, "uf3_ctx_md_skin: skin must lie in [0, 4] Angstrom");
    if (skin != c->md.skin) { c->md.valid = false; c->md.cap = 0; c->md.cap_tuned = false; }
    c->md.skin = skin;
    return UF3_OK;
}

extern "C" int uf3_ctx_md_stats(uf3_ctx *c, int64_t *builds, int64_t *steps, int64_t *redone) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (builds) *builds = c->md.builds;
    if (steps) *steps = c->md.steps;
    if (redone) *redone = c->md.redone;
    return UF3_OK;
}

// ---- one evaluator call, in stages ---------------------------------------------
// eval_impl is a retry loop around: eval_route (which route), md_stage or prepare (the lists and inputs in place), eval_model
// (the model on the device), eval_plan (which k_eval instance, how much LDS), launch_eval / launch_collect / the frame sum (the
// launches), wait_seq and eval_verdict (does the result stand).  eval_host is the second loop around it, for host arrays.

// What a caller asks of eval_impl besides frames, model and outputs.  The defaults are a whole batch whose status words
// eval_impl looks at itself; a call site names what it sets.
struct EvalCall {
    int64_t atom_begin = 0, atom_end = -1;  // the atoms whose terms are wanted (-1: to the end of the batch)
    bool centre_share = false;              // uf3_eval_centres: a block of centres, not of atoms (see EvalRoute::centres)
    // eval_host's calls: the status words travel with the results and eval_host gives the verdict
    int *deferred_cap = nullptr;            // out: the list capacity nobody has checked yet (0: none); eval_impl does not wait
    int *flags_tail = nullptr;              // device block behind the results: the last kernel copies the status words there
    double *mirror = nullptr;               // pinned block the last kernel writes results, forces and its sequence number into
};

// The route of a call, decided once.
struct EvalRoute {
    int64_t atom_lo, atom_hi;   // the range, its end resolved
    bool whole;                 // ... and whether it is the batch
    // a block of CENTRES (uf3_eval_centres): the two-pass route on the block -- every triplet once, at its centre inside the
    // block; the collection pass then serves the block and its halo (the atoms the block's lists mention), whose lists are
    // built for that purpose.  Rows of all other atoms stay zero; the shares of disjoint blocks add up to the frame.
    bool centres;
    // whole batch (or block of centres) with forces and 3-body terms: every triplet once, at its centre, + a collection pass;
    // otherwise the gather instances -- a block of atoms (its neighbours' centres may lie outside the block): every atom walks
    // the triplets it belongs to
    bool two_pass;
    // two-pass route, list capacity known: the centre pass builds each atom's 3-body list from the candidates of its own pair
    // walk (no k_build_n3 launch, one neighbourhood scan less)
    bool fuse;
    // MD route: the candidates of every atom from the context's persistent lists instead of a cell-list walk (see md_build)
    bool md_step;
    // a block of centres with the fused list build zeroes rows, list counts and halo marks in ONE launch (k_zero3)
    bool zero3;
};
static int eval_route(const uf3_basis *b, const uf3_frames *fr, const EvalCall &call, bool forces, EvalRoute &R) {
    uf3_ctx *c = b->ctx;
    const int64_t total = (fr && fr->atom_offsets && fr->n_frames >= 1) ? fr->atom_offsets[fr->n_frames] : -1;
    // (the one range check: prepare refuses a batch without a total, and a batch that passes it -- or matches the key of the
    // MD lists, whose offsets are compared -- holds exactly `total` atoms.  An open end with a begin past the total, which only
    // the check behind the staging used to catch, is caught here: no entry can ask for it today, they refuse an open end)
    if (total >= 0 && (call.atom_begin < 0 || call.atom_begin > total ||
                       (call.atom_end >= 0 && (call.atom_begin > call.atom_end || call.atom_end > total))))
        return fail(c, UF3_EINVAL, "uf3_eval_atoms: atom range outside the batch");
    const bool three = forces && b->host.T > 0;
    R.atom_lo = call.atom_begin;
    R.atom_hi = call.atom_end < 0 ? total : call.atom_end;
    R.whole = call.atom_begin == 0 && (call.atom_end < 0 || call.atom_end == total);
    R.centres = call.centre_share && !R.whole && three && call.atom_end > call.atom_begin;
    R.two_pass = (R.whole || R.centres) && three && !uf3_env("UF3_EVAL_GATHER");
    R.fuse = R.two_pass && c->n3_tuned && c->n3_cap > 0 && !uf3_env("UF3_SEPARATE_N3");
    R.md_step = c->md.skin > 0.0 && R.fuse && !uf3_env("UF3_NO_MD");      // (a block of centres too: round 5)
    R.zero3 = R.centres && R.fuse && !R.md_step && !uf3_env("UF3_NO_HALO");
    return UF3_OK;
}

// MD route: everything a step reads is put in place, in exactly one of five ways -- new lists (which bring their own inputs), or
// the lists stand and only positions | species and zeroed status words are due -- and `P` describes it (md_prepared).
// was_clean: the words are known to be zero (the previous call was an MD step of the host entry that set none).
static int md_stage(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, bool was_clean, Prepared &P) {
    uf3_ctx *c = b->ctx;
    hipStream_t st = c->stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->md.stale || !md_key_matches(c->md, b, fr)) {
        int rc = md_build(b, fr, d_pos, d_z, P, true);
        if (rc) return rc;
    } else if (c->md.live) {
        // (the integrator's frame kernel has zeroed the step's status words and its move kernel has raised those of the list test)
    } else if (c->staged_in_dev && d_pos == (const double *)c->stage_cur) {
        // positions | species are in the device block already (upload_frames, through the BAR).  k_md_fetch also zeroed the
        // step's status words: needed only when they are not known to be zero (was_clean: the host has just read them)
        c->staged_in_dev = 0;
        if (!was_clean)
            hipLaunchKernelGGL(k_md_fetch, dim3(1), dim3(64), 0, st, (const int4 *)nullptr, (int4 *)nullptr, 0, c->flags.as<int>());
    } else if (c->pin_in_pending && d_pos == (const double *)c->stage_cur) {
        // a small batch staged by upload_frames: positions | species are still in the caller's pinned block
        const size_t at = c->pin_in_pending;
        c->pin_in_pending = 0;
        if (c->md.natoms <= UF3_SMALL_ATOMS && !uf3_env("UF3_NO_ZERO_COPY")) {
            hipLaunchKernelGGL(k_md_fetch, dim3(1), dim3(256), 0, st, (const int4 *)c->pin_in.p, (int4 *)c->stage_cur, (int)(at / 16),
                               c->flags.as<int>());
            c->pin_in_busy = true;
        } else {
            HIPCHK(c, hipMemcpyAsync(c->stage_cur, c->pin_in.p, at, hipMemcpyHostToDevice, st));
            HIPCHK(c, hipEventRecord(c->pin_in_done, st));
            HIPCHK(c, hipMemsetAsync(c->flags.as<int>() + ST_N3_NEED, 0, 4 * sizeof(int), st));
        }
    } else
        HIPCHK(c, hipMemsetAsync(c->flags.as<int>() + ST_N3_NEED, 0, 4 * sizeof(int), st));
    md_prepared(c, P);
    return UF3_OK;
}

// The model on the device: c1 | c2 | c3 in c->coeff, and the window table of the CW / WIN instances where the model allows one
// (c->cw_of).  An MD loop passes the same model every step: it is uploaded -- and the caller's buffers waited for, the one
// hipStreamSynchronize -- only when it differs from the host shadow; the unchanged path is three memcmps.
static int eval_model(uf3_basis *b, const double *c1, const double *c2, const double *c3, const double *&model) {
    uf3_ctx *c = b->ctx;
    hipStream_t st = c->stream;
    const size_t n1 = (size_t)b->host.S, n2 = b->c2_len, n3 = b->c3_len;
    HIPCHK(c, c->coeff.ensure(8 * (n1 + n2 + n3 + 1)));
    double *dc = c->coeff.as<double>();
    model = dc;
    std::vector<double> &sh = c->coeff_shadow;
    const bool same = c->coeff_dev == (const void *)dc && sh.size() == n1 + n2 + n3 && !memcmp(sh.data(), c1, 8 * n1) &&
                      (!n2 || !memcmp(sh.data() + n1, c2, 8 * n2)) && (!n3 || !memcmp(sh.data() + n1 + n2, c3, 8 * n3));
    if (same) return UF3_OK;
    sh.resize(n1 + n2 + n3);
    memcpy(sh.data(), c1, 8 * n1);
    if (n2) memcpy(sh.data() + n1, c2, 8 * n2);
    if (n3) memcpy(sh.data() + n1 + n2, c3, 8 * n3);
    c->coeff_dev = nullptr;
    HIPCHK(c, hipMemcpyAsync(dc, sh.data(), 8 * sh.size(), hipMemcpyHostToDevice, st));
    // the window table of the CW instances: only when every coefficient outside the kept-bin window of the centre legs is
    // exactly zero (bins without a column decompress to zero: any fitted or loaded model; arbitrary grids keep the global rows)
    c->cw_of = nullptr;
    std::vector<double> tab;
    if (b->eval_cw_ok && n3) {
        const double *g3 = sh.data() + n1 + n2;
        const int lo = b->cw_lo, ext = b->cw_ext, dm = b->cw_dim_m, dn = b->cw_dim_n;
        tab.assign((size_t)b->cw_bytes / 8, 0.0);
        bool zero_outside = true;
        for (size_t t = 0; t < b->cw_lut_off.size() && zero_outside; t++) {
            const double *g = g3 + b->cw_lut_off[t];
            for (int l = 0; l < b->cw_dim_l[t] && zero_outside; l++)
                for (int mm = 0; mm < dm && zero_outside; mm++) {
                    const bool in = l >= lo && l < lo + ext && mm >= lo && mm < lo + ext;
                    const double *row = g + ((size_t)l * dm + mm) * dn;
                    if (in) std::memcpy(tab.data() + ((t * ext + (l - lo)) * ext + (mm - lo)) * dn, row, 8 * (size_t)dn);
                    else for (int q = 0; q < dn; q++) zero_outside = zero_outside && row[q] == 0.0;
                }
        }
        if (zero_outside) {
            HIPCHK(c, c->coeff_cw.ensure((size_t)b->cw_bytes));
            HIPCHK(c, hipMemcpyAsync(c->coeff_cw.p, tab.data(), (size_t)b->cw_bytes, hipMemcpyHostToDevice, st));
            c->cw_of = b;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    c->coeff_dev = dc;
    return UF3_OK;
}

// The plan of one k_eval launch: which instance, how much dynamic LDS.  A pure function of numbers -- no context, no basis, no
// HIP call (uf3_eval_plan_debug is its test surface) -- and the only place that states the bytes of the three LDS layouts.
enum { EVAL_NO_TAB = 1, EVAL_NO_CW = 2, EVAL_NO_CAP16 = 4 };      // the switches UF3_EVAL_NO_TAB / _NO_CW / _NO_CAP16, as bits
struct EvalPlan {
    bool gather, md;            // the route's part of the instance: !two_pass | candidates from the persistent lists
    bool cw, win, tab, cap16;   // centre legs from a window table in LDS | in global memory | from per-bond tables; capacity 16 as a constant
    size_t lds;                 // dynamic LDS of the workgroup
    size_t lds_per_wave;        // CW: bytes of the per-wave arrays of its multi-wave workgroup (else 0)
    bool fits;                  // false: a one-wave layout larger than the device grants
};
static EvalPlan eval_plan(size_t cap, bool two_pass, bool md_step, size_t n2, size_t n_recs, size_t cw_bytes, bool tab_ok,
                          bool has_window, int lds_max, int switches) {
    EvalPlan p = {};
    p.gather = !two_pass; p.md = md_step;
    // own list (32 + 20 B per entry), queue of bonds, force on the entries (24), walk-order entries + keys (48)
    const size_t lds_plain = cap * 32 + (5 * cap + 2) * 4 + 16 + 2 * WAVE * EVAL_Q * sizeof(double) + cap * 24 + cap * 48;
    // TAB instances (centre legs from per-bond tables, k_eval): + leg n's knot records, + the tables when they do not fit
    // over the queue.  Chosen by the basis alone -- not by the capacity -- unless the longer layout does not fit at all
    const size_t lds_tab = lds_plain + 16 + EVAL_TAB_KN * sizeof(KnotRec) + (cap > EVAL_TAB_CAP ? 136 * cap + 16 : 0);
    p.tab = two_pass && tab_ok && (int)lds_tab <= lds_max && !(switches & EVAL_NO_TAB);
    // CW instances (MD route only: measured 197 against 190 M atom-steps/s there, a loss on the plain route): EVAL_CW_WAVES
    // one-atom waves per workgroup around one copy of the window table, every knot record and the pair coefficients
    const size_t cw_per_wave = ((md_step ? lds_plain - cap * 48 : lds_plain) + 15) / 16 * 16;      // (the walk-order arrays: fused builds only)
    const size_t lds_cw = cw_bytes + n_recs * sizeof(KnotRec) + (n2 * 8 + 15) / 16 * 16 + EVAL_CW_WAVES * cw_per_wave;
    p.cw = p.tab && md_step && has_window && cap <= 16 &&      /* (lists of <= 16 entries: the force gather's stage, k_eval) */
           lds_cw <= UF3_LDS_LIMIT / (EVAL_CW_WAVES > 8 ? 1 : 2) && !(switches & EVAL_NO_CW);
    // WIN instances: the same window table read through global memory by the one-wave TAB instances CW does not serve
    p.win = p.tab && !p.cw && has_window && !(switches & EVAL_NO_CW);
    p.cap16 = two_pass && cap == 16 && !(switches & EVAL_NO_CAP16);
    p.lds = p.cw ? lds_cw : (p.tab ? lds_tab : lds_plain);
    p.lds_per_wave = p.cw ? cw_per_wave : 0;
    p.fits = p.cw || (int)p.lds <= lds_max;      // (CW asks for more than the default grant itself: launch_lds)
    return p;
}

extern "C" int uf3_eval_plan_debug(int32_t cap, int two_pass, int md_step, int64_t n2, int64_t n_recs, int64_t cw_bytes, int tab_ok,
                                   int has_window, int32_t lds_max, int switches, int32_t *instance, int64_t *lds,
                                   int64_t *lds_per_wave, int32_t *fits) {
    if (cap < 1 || n2 < 0 || n_recs < 0 || cw_bytes < 0 || lds_max < 0 || !instance || !lds || !lds_per_wave || !fits)
        return fail(nullptr, UF3_EINVAL, "uf3_eval_plan_debug: bad argument");
    const EvalPlan p = eval_plan((size_t)cap, two_pass != 0, md_step != 0, (size_t)n2, (size_t)n_recs, (size_t)cw_bytes, tab_ok != 0,
                                 has_window != 0, lds_max, switches);
    *instance = (p.cw ? 1 : 0) | (p.win ? 2 : 0) | (p.tab ? 4 : 0) | (p.cap16 ? 8 : 0);
    *lds = (int64_t)p.lds; *lds_per_wave = (int64_t)p.lds_per_wave; *fits = p.fits;
    return UF3_OK;
}

// Which instances of k_eval the library holds -- this dispatch names exactly these:
//   k_eval<false, VIR, CAP, MD, TAB, CW, WIN>  CAP 0 or 16; CW and WIN are TAB instances, and CW exists on the MD route only
//   k_eval<true, VIR>  the gather instances
// instance: strain derivative | list capacity 16 as a constant | candidates from the persistent lists | centre legs from per-bond
// tables (one set of 3-body legs, T <= 64, short lists: the usual case).  One wave per centre, CW: EVAL_CW_WAVES of them
static int launch_eval(uf3_ctx *c, const EvalPlan &p, const EvalArgs &A, int64_t n_centres) {
    hipStream_t st = c->stream;
    const size_t lds = p.lds;
    const dim3 eg((unsigned)((n_centres + 7) / 8 * 8));
    const dim3 eg_cw((unsigned)(((n_centres + EVAL_CW_WAVES - 1) / EVAL_CW_WAVES + 7) / 8 * 8));
    if (!p.gather)
        return with_bool(A.virial != 0, [&](auto VIR) {
        return with_bool(p.cap16, [&](auto C16) {
        return with_bool(p.md, [&](auto MD) {
            constexpr int CAP = C16 ? 16 : 0;
            if (p.cw) {
                // (MD route only: with the walk-order arrays of the fused list build the waves' own LDS is 7.1 KB each, and two
                // 8-wave workgroups + two copies of the tables do not fit a CU -- 168 of 160 KB; not instantiated)
                if constexpr (MD)
                    HIPCHK(c, (launch_lds<k_eval<false, VIR, CAP, true, true, true>>(c, eg_cw, dim3(64 * EVAL_CW_WAVES), lds, A)));
                else
                    return fail(c, UF3_EINVAL, "k_eval<CW> outside the MD route");
            }
            else if (p.win) hipLaunchKernelGGL((k_eval<false, VIR, CAP, MD, true, false, true>), eg, dim3(64), lds, st, A);
            else if (p.tab) hipLaunchKernelGGL((k_eval<false, VIR, CAP, MD, true>), eg, dim3(64), lds, st, A);
            else hipLaunchKernelGGL((k_eval<false, VIR, CAP, MD, false>), eg, dim3(64), lds, st, A);
            return (int)UF3_OK;
        }); }); });
    if (n_centres <= 0) return UF3_OK;
    if (A.virial) hipLaunchKernelGGL((k_eval<true, true>), eg, dim3(64), lds, st, A);
    else hipLaunchKernelGGL((k_eval<true, false>), eg, dim3(64), lds, st, A);
    return UF3_OK;
}

// The collection pass behind the centre pass of the two-pass route: every atom gathers what the centres put on it -- one of three
// kernels, by who has lists and where the shares wait.  A block of centres off the MD route first gets its halo's lists.
// part_sums: the whole-batch pass of the MD route also leaves per-workgroup sums for the frame sum to add.
static int launch_collect(uf3_basis *b, const Prepared &P, const EvalRoute &R, const double *d_pos, bool part_sums, EvalArgs &A) {
    uf3_ctx *c = b->ctx;
    hipStream_t st = c->stream;
    const dim3 grid((unsigned)(((P.natoms + 15) / 16 + 7) / 8 * 8));
    if (R.centres && !R.md_step) {
        // the block's lists exist now (the centre pass built them, or prepare did): the halo's, then the collection pass over
        // block + halo
        if (R.fuse || uf3_env("UF3_NO_HALO")) {
            int rh = build_halo_lists(b, P, A.n3, d_pos, (int)R.atom_lo, (int)R.atom_hi, R.zero3);
            if (rh) return rh;
        }
        A.halo_mark = c->halo.as<int>();
    }
    if (R.md_step && R.centres)      // every atom checks itself; the block and the atoms its centres wrote to collect
        hipLaunchKernelGGL(k_eval_collect_md_halo, dim3((unsigned)((P.natoms + 15) / 16)), dim3(256), 0, st, A);
    else if (R.md_step) {
        if (part_sums) {
            const size_t n_wg = ((size_t)P.natoms + 15) / 16;
            HIPCHK(c, c->part_sums.ensure(8 * (7 * n_wg + 2)));
            A.part_e = c->part_sums.as<double>(); A.part_v = A.part_e + n_wg; A.part_off = (long long *)(A.part_v + 6 * n_wg);
        }
        hipLaunchKernelGGL(k_eval_collect_md, grid, dim3(256), 0, st, A);
    }
    else hipLaunchKernelGGL(k_eval_collect, grid, dim3(256), 0, st, A);
    return UF3_OK;
}

// The polled wait of a call whose last kernel stores the call's sequence number, behind system-scope fences, into a pinned word:
// a few us sooner than the stream's completion signal reaches the host.  Bounded (2 ms); false: not seen -- the caller falls
// back on hipStreamSynchronize.
static bool wait_seq(const unsigned *word, unsigned seq) {
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
    for (int spin = 0; ; spin++) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return true;
        if ((spin & 255) == 255 && std::chrono::steady_clock::now() > t_end) return false;
    }
}

// What the status words `fl` of a finished evaluation say, and the consequences every caller shares: an error word is turned into
// its error (rc), the early warning marks the MD lists stale, a 3-body list longer than the capacity used raises n3_cap.
// EVAL_OUTRUN and EVAL_REGROWN void the results; how the call is repeated -- and how often -- is the caller's.
enum EvalVerdict { EVAL_DONE, EVAL_OUTRUN, EVAL_REGROWN, EVAL_ERROR };
static EvalVerdict eval_verdict(uf3_ctx *c, const int *fl, int cap_used, bool md_step, int &rc) {
    if (fl[ST_ERROR]) { rc = check_flags(c); return EVAL_ERROR; }
    // an atom beyond skin / 2 of where the lists were built (or of another species), or lists clipped by a build nobody waited for
    if (md_step && fl[ST_MD_OUTRUN]) return EVAL_OUTRUN;
    if (md_step && fl[ST_MD_WARN]) c->md.stale = true;       // (early warning: rebuild in front of the next step)
    if (cap_used && fl[ST_N3_NEED] > cap_used) { c->n3_cap = cap_for(fl[ST_N3_NEED]); return EVAL_REGROWN; }
    return EVAL_DONE;
}

static int eval_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *c1,
                     const double *c2, const double *c3, double *d_energies, double *d_forces, double *d_virials,
                     const EvalCall &call = EvalCall()) {
    uf3_ctx *c = b->ctx;
    uf3_env_refresh();
    if (!d_pos || !d_z || !c1 || !d_energies) return fail(c, UF3_EINVAL, "uf3_eval: null argument");
    if ((b->c2_len && !c2) || (b->c3_len && !c3)) return fail(c, UF3_EINVAL, "uf3_eval: missing coefficients");
    EvalRoute R;
    int rc = eval_route(b, fr, call, d_forces != nullptr, R);
    if (rc) return rc;
    Prepared P;
    hipStream_t st = c->stream;
    c->md_step = R.md_step;
    const bool was_clean = c->md.flags_clean;      // (true only straight after an MD step of eval_host that set no status word)
    c->md.flags_clean = false;
    if (c->md.live && (!R.md_step || c->md.stale || !md_key_matches(c->md, b, fr))) {
        rc = md_live_fetch(c, fr);                  // (a list build or the rebuild route is due: both read the cells on the host)
        if (rc) return rc;
    }
    if (R.md_step) {
        rc = md_stage(b, fr, d_pos, d_z, was_clean, P);
        if (rc) return rc;
    } else {
        if (c->md.wrap) {                           // (the rebuild-everything route: every evaluation builds its lists)
            rc = c->md.wrap(d_pos);
            if (rc) return rc;
        }
        rc = prepare(b, fr, d_pos, d_z, !R.fuse, P, call.deferred_cap != nullptr, call.atom_begin, R.whole ? -1 : call.atom_end);
        if (rc) return rc;
    }
    if (call.deferred_cap) *call.deferred_cap = P.deferred ? P.n3.cap : 0;
    const double *dc;
    rc = eval_model(b, c1, c2, c3, dc);
    if (rc) return rc;
    const size_t n1 = (size_t)b->host.S, n2 = b->c2_len;
    HIPCHK(c, c->e_atom.ensure(8 * (size_t)P.natoms * (d_virials ? 7 : 1)));
    // (atoms outside the range: the per-frame sums run over the range only)
    EvalArgs A = {};
    A.B = b->dev; A.geoms = P.geoms; A.frame_of = P.frame_of; A.cl = P.cl; A.n3 = P.n3;
    if (!A.n3.cap) A.n3.cap = 1;
    A.pos = d_pos; A.spec = P.spec; A.c1 = dc; A.c2 = dc + n1; A.c3 = dc + n1 + n2;
    A.e_atom = c->e_atom.as<double>(); A.forces = d_forces; A.natoms = P.natoms;
    A.atom_lo = (int)R.atom_lo; A.atom_hi = (int)R.atom_hi;
    A.virial = d_virials ? A.e_atom + P.natoms : nullptr;
    // (rows of atoms that no centre of the block touches: zero -- here, or by k_zero3 inside the loop below, or, on the MD route,
    // on every attempt)
    if (call.centre_share && !R.whole && d_forces && !R.zero3 && !R.md_step)
        HIPCHK(c, hipMemsetAsync(d_forces, 0, 24 * (size_t)P.natoms, st));
    const int switches = (uf3_env("UF3_EVAL_NO_TAB") ? EVAL_NO_TAB : 0) | (uf3_env("UF3_EVAL_NO_CW") ? EVAL_NO_CW : 0) |
                         (uf3_env("UF3_EVAL_NO_CAP16") ? EVAL_NO_CAP16 : 0);
    const bool no_spin = c->timing || uf3_env("UF3_NO_TAIL_SPIN");        // (event timing queues a record behind the chain)
    // one whole frame on the MD route, large: the collection pass also leaves per-workgroup sums of the atoms' energies (and strain
    // derivatives), and the frame sum adds those -- natoms / 16 values instead of natoms (12 -> 4 us at 50 k atoms)
    const bool part_sums = R.md_step && R.whole && P.n_frames == 1 && P.natoms >= 8192 && !call.mirror && !uf3_env("UF3_NO_PART_SUMS");
    {
        Timed tm(c, T_EVAL);
        for (int attempt = 0; ; attempt++) {
            c->tail_signalled = false;
            if (R.fuse) {
                rc = n3_alloc(c, P.natoms, c->n3_cap, A.n3);
                if (rc) return rc;
                A.fuse_n3 = 1;
                A.n3_need = c->flags.as<int>() + ST_N3_NEED;
                if (!P.flags_zeroed || attempt) HIPCHK(c, hipMemsetAsync(A.n3_need, 0, (R.md_step ? 3 : 1) * sizeof(int), st));
            }
            if (R.md_step) {
                const uf3_ctx::MdState &md = c->md;
                A.fuse_n3 = 0;
                A.geoms = P.geoms; A.frame_of = P.frame_of; A.spec = P.spec;
                A.sup_ent = md.ent.as<SupEntry>(); A.sup_cnt = md.cnt.as<int>(); A.sup_cap = md.cap;
                A.pos_ref = md.pos_ref.as<double>(); A.z_now = d_z;
                const double hard = 0.5 * md.skin * (1.0 - 1e-9), soft = 0.7 * hard;
                A.md_hard2 = hard * hard; A.md_soft2 = soft * soft;
                A.md_flags = c->flags.as<int>() + ST_MD_OUTRUN;
                c->md.steps++;
                HIPCHK(c, c->md.surv.ensure(sizeof(int) * (size_t)P.natoms * A.n3.cap));
                A.md_inbox = c->md.inbox.as<double>(); A.md_surv = c->md.surv.as<int>();
                A.md_stamp = (double)c->md.steps;
                if (R.centres) {
                    // marks of the atoms the block's centres write to: zeroed when (re)allocated, launch numbers only grow
                    const void *before = c->md.mark.p;
                    HIPCHK(c, c->md.mark.ensure(sizeof(int) * (size_t)P.natoms));
                    if (c->md.mark.p != before) HIPCHK(c, hipMemsetAsync(c->md.mark.p, 0, c->md.mark.cap, st));
                    A.md_mark = c->md.mark.as<int>();
                    A.md_mark_now = (int)(c->md.steps & 0x7fffffff);
                }
            }
            const size_t cap = (size_t)A.n3.cap;
            const EvalPlan plan = eval_plan(cap, R.two_pass, R.md_step, n2, b->n_recs, (size_t)b->cw_bytes, b->eval_tab_ok,
                                            c->cw_of == (const void *)b, c->lds_max, switches);
            if (!plan.fits) return fail(c, UF3_EOVERFLOW, "3-body neighbour list does not fit in LDS");
            if (plan.win) { A.c3w = c->coeff_cw.as<double>(); A.cw_lo = b->cw_lo; A.cw_ext = b->cw_ext; }
            if (plan.cw) {
                A.c3w = c->coeff_cw.as<double>(); A.cw_bytes = b->cw_bytes; A.cw_zero = b->cw_zero; A.cw_lo = b->cw_lo; A.cw_ext = b->cw_ext;
                A.lds_per_wave = (int)plan.lds_per_wave; A.cw_recs_bytes = (int)(b->n_recs * sizeof(KnotRec)); A.cw_c2 = (int)n2;
            }
            if (R.two_pass) {
                if (!R.md_step) {
                    HIPCHK(c, c->nbr_f.ensure(24 * (size_t)P.natoms * cap));
                    A.nbr_f = c->nbr_f.as<double>();
                }
                // (a block of centres on the MD route: its halo's rows are sums into zeros -- again on every attempt)
                if (R.md_step && R.centres) HIPCHK(c, hipMemsetAsync(d_forces, 0, 24 * (size_t)P.natoms, st));
                if (R.zero3) {
                    HIPCHK(c, c->halo.ensure(sizeof(int) * ((size_t)P.natoms + 4)));
                    const size_t words = 8 * (size_t)P.natoms;
                    hipLaunchKernelGGL(k_zero3, dim3((unsigned)std::min<size_t>((words + 255) / 256, 4096)), dim3(256), 0, st,
                                       (unsigned *)d_forces, 6 * (size_t)P.natoms, (unsigned *)A.n3.cnt, (size_t)P.natoms,
                                       (unsigned *)c->halo.p, (size_t)P.natoms);
                }
                else if (R.centres && R.fuse && !R.md_step) HIPCHK(c, hipMemsetAsync(A.n3.cnt, 0, sizeof(int) * (size_t)P.natoms, st));   // (lists not built: empty)
            }
            rc = launch_eval(c, plan, A, R.atom_hi - R.atom_lo);
            if (rc) return rc;
            if (R.two_pass) {
                if (R.fuse && call.deferred_cap) *call.deferred_cap = (int)cap;
                rc = launch_collect(b, P, R, d_pos, part_sums, A);
                if (rc) return rc;
            }
            // (UF3_DEBUG_LDS: which k_eval instance ran -- tests assert the route they mean to reach; atom range, centre range
            // and whole batch alike)
            if (c->env_debug_lds && R.atom_hi > R.atom_lo)
                fprintf(stderr, "uf3: k_eval cw=%d win=%d tab=%d gather=%d md=%d cap16=%d vir=%d centres=%d part_sums=%d cap=%d atoms=%lld\n",
                        (int)plan.cw, (int)plan.win, (int)plan.tab, (int)plan.gather, (int)plan.md, (int)plan.cap16, (int)(A.virial != nullptr),
                        (int)R.centres, (int)part_sums, (int)cap, (long long)(R.atom_hi - R.atom_lo));
            // How the call's end reaches the host.  Into the caller's pinned block (mirror): the launch's last workgroup signals the
            // host itself; the tail-count word counts workgroups.
            // INVARIANT of the polled completion (eval_host returns without hipStreamSynchronize once the sequence number shows):
            // k_frame_sum is the LAST launch of the call's chain, and its sequence store, behind system-scope fences, the last
            // access of that chain to pin_in / pin_out -- the next call's memcpy into those blocks relies on it.  Anything queued
            // behind this launch (a timing event, a second mirror write) must clear `tail_signalled` so that the host waits
            // for the stream instead.
            // A device-resident call that looks at its status words before it returns (the fused list build, the MD route): the
            // last kernel puts them, and the call's sequence number behind them, into a pinned block the host polls -- no copy
            // of 16 bytes through the runtime's staging and no wait for the stream's completion signal (~10 us of an MD step)
            const bool own_verdict = R.fuse && !call.deferred_cap;
            int *flags_host = nullptr;
            unsigned *seq_host = nullptr;
            unsigned seq = 0;
            if (!no_spin && (call.mirror || (own_verdict && !call.flags_tail))) {
                if (++c->eval_seq == 0) c->eval_seq = 1;
                seq = c->eval_seq;
                if (call.mirror) c->tail_signalled = true;
                else {
                    HIPCHK(c, c->pin_eval.ensure(64));
                    flags_host = (int *)c->pin_eval.p; seq_host = (unsigned *)c->pin_eval.p + 4;
                }
            }
            {
                // the per-atom values of every frame over the range -- or, behind a collection pass that left them, its per-workgroup
                // sums as ONE frame of (natoms + 15) / 16 values (one workgroup per frame and component: wide for big frames, the loop
                // is a latency chain)
                const int n_wg = (P.natoms + 15) / 16;
                const int sum_threads = P.natoms / P.n_frames >= 2048 ? 1024 : 256;        // (part sums: a frame of >= 8192 atoms)
                hipLaunchKernelGGL(k_frame_sum, dim3(part_sums ? 1 : P.n_frames, d_virials ? 7 : 1), dim3(sum_threads), 0, st,
                                   part_sums ? (const double *)A.part_e : A.e_atom, part_sums ? (const double *)A.part_v : A.virial,
                                   part_sums ? (const int64_t *)A.part_off : P.d_offsets, d_energies, d_virials,
                                   (const int *)c->flags.as<int>(), flags_host ? flags_host : call.flags_tail, call.mirror,
                                   (const double *)d_forces, d_forces ? 3 * P.natoms : 0, part_sums ? 0 : (int)R.atom_lo,
                                   part_sums ? n_wg : (int)R.atom_hi, seq, c->flags.as<int>() + ST_TAIL_COUNT, seq_host);
            }
            if (!own_verdict) break;
            // the lists were part of this launch: did they fit?  (Asked after everything is queued -- all kernels
            // are safe on clipped lists -- so that the GPU does not idle while the host looks.)
            int fl[4] = {0, 0, 0, 0};
            if (seq_host) {
                if (!wait_seq(seq_host, seq)) HIPCHK(c, hipStreamSynchronize(st));
                std::memcpy(fl, flags_host, sizeof(fl));
            } else {
                HIPCHK(c, hipMemcpyAsync(fl, c->flags.p, sizeof(fl), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
            }
            const EvalVerdict v = eval_verdict(c, fl, (int)cap, R.md_step, rc);
            if (v == EVAL_ERROR) return rc;
            if (v == EVAL_DONE) break;
            if (v == EVAL_OUTRUN) {
                // the results are void -- new lists from these positions, and again
                if (attempt >= 5) return fail(c, UF3_EOVERFLOW, "MD neighbour lists did not settle");
                c->md.redone++;
                if (c->md.live) { rc = md_live_fetch(c, fr); if (rc) return rc; }
                rc = md_build(b, fr, d_pos, d_z, P);
                if (rc) return rc;
                md_prepared(c, P);
            } else if (attempt >= 5) return fail(c, UF3_EOVERFLOW, "3-body neighbour capacity did not converge");
        }
    }
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_eval_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                            const double *c1, const double *c2, const double *c3, double *d_energies, double *d_forces) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return eval_impl(b, fr, d_pos, d_z, c1, c2, c3, d_energies, d_forces, nullptr);
}

extern "C" int uf3_eval_virial_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                   const double *c1, const double *c2, const double *c3, double *d_energies,
                                   double *d_forces, double *d_virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return eval_impl(b, fr, d_pos, d_z, c1, c2, c3, d_energies, d_forces, d_virials);
}

// host arrays in and out: the batch staged on the device, eval_impl on it, the results back.  `call`: range and centre_share; the
// three fields of a host call are set here
static int eval_host(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                     const double *c2, const double *c3, double *energies, double *forces, double *virials,
                     EvalCall call = EvalCall()) {
    uf3_ctx *c = b->ctx;
    uf3_env_refresh();
    if (!energies) return fail(c, UF3_EINVAL, "uf3_eval: null energies");
    int natoms = 0;
    poll_pending(c, false);                  // (arrived verdicts on asynchronous featurizer calls: for uf3_ctx_synchronize, not for us)
    int rc = upload_frames(c, fr, pos, z, natoms, true);
    if (rc) return rc;
    // results in one block: energies [nf] | virials [nf][6] | forces [natoms][3]
    const size_t nf = (size_t)fr->n_frames, bf = forces ? 24 * (size_t)natoms : 0, total = 8 * nf * 7 + bf;
    HIPCHK(c, c->stage_out.ensure(total + 16));
    double *d_e = c->stage_out.as<double>(), *d_v = d_e + nf, *d_f = d_e + 7 * nf;
    if (forces && (call.atom_begin != 0 || (call.atom_end >= 0 && call.atom_end != natoms)))   // rows of other ranks' atoms: zero
        HIPCHK(c, hipMemsetAsync(d_f, 0, bf, c->stream));
    if (total + 16 <= UF3_PIN_LIMIT) {
        // small batch (an MD step): results and the neighbour stage's status words come back in ONE download and ONE
        // wait -- the lists are built at the remembered capacity and the evaluation runs on them right away; if they
        // overflowed (or a species / wrap error was flagged) the results are discarded and the call repeated / failed
        HIPCHK(c, c->pin_out.ensure(total + 32));
        const int *fl = (const int *)((const char *)c->pin_out.p + total);
        unsigned *seq_word = (unsigned *)((char *)c->pin_out.p + total + 16);
        int cap_used = 0;
        call.deferred_cap = &cap_used;
        call.flags_tail = (int *)((char *)c->stage_out.p + total);
        for (int attempt = 0; attempt < 6; attempt++) {
            // (up to the one-workgroup cell-list limit the last kernel writes the results into the pinned block itself; the
            // mirror's layout has the forces right behind the 7 nf sums, as d_e does)
            const bool zero_copy = natoms <= UF3_SMALL_ATOMS && !uf3_env("UF3_NO_ZERO_COPY");
            call.mirror = zero_copy ? (double *)c->pin_out.p : nullptr;
            cap_used = 0;
            *(volatile unsigned *)seq_word = 0;
            rc = eval_impl(b, fr, (const double *)c->stage_cur, c->d_stage_z, c1, c2, c3, d_e, forces ? d_f : nullptr,
                           virials ? d_v : nullptr, call);
            if (rc) return rc;
            if (!zero_copy) HIPCHK(c, hipMemcpyAsync(c->pin_out.p, d_e, total + 16, hipMemcpyDeviceToHost, c->stream));
            if (!(zero_copy && c->tail_signalled && wait_seq(seq_word, c->eval_seq))) HIPCHK(c, hipStreamSynchronize(c->stream));
            c->pin_in_busy = false;
            poll_pending(c, true);           // (remembered, see above)
            const EvalVerdict v = eval_verdict(c, fl, cap_used, c->md_step, rc);
            if (v == EVAL_ERROR) return rc;
            if (v == EVAL_OUTRUN) { c->md.valid = false; c->md.verify_next = true; c->md.redone++; }      // (rebuilt by the repeat, with the host looking)
            if (v != EVAL_DONE) continue;
            c->md.flags_clean = c->md_step && !fl[ST_N3_NEED] && !fl[ST_MD_OUTRUN] && !fl[ST_MD_WARN];
            const double *h = (const double *)c->pin_out.p;
            std::memcpy(energies, h, 8 * nf);
            if (virials) std::memcpy(virials, h + nf, 48 * nf);
            if (forces) std::memcpy(forces, h + 7 * nf, bf);
            return UF3_OK;
        }
        return fail(c, UF3_EOVERFLOW, "3-body neighbour capacity did not converge");
    }
    rc = eval_impl(b, fr, (const double *)c->stage_cur, c->d_stage_z, c1, c2, c3, d_e, forces ? d_f : nullptr,
                   virials ? d_v : nullptr, call);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(energies, d_e, 8 * nf, hipMemcpyDeviceToHost, c->stream));
    if (virials) HIPCHK(c, hipMemcpyAsync(virials, d_v, 48 * nf, hipMemcpyDeviceToHost, c->stream));
    if (forces) HIPCHK(c, hipMemcpyAsync(forces, d_f, bf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    poll_pending(c, true);
    return check_flags(c);
}

extern "C" int uf3_eval(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                        const double *c2, const double *c3, double *energies, double *forces) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return eval_host(b, fr, pos, z, c1, c2, c3, energies, forces, nullptr);
}

extern "C" int uf3_eval_virial(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                               const double *c2, const double *c3, double *energies, double *forces, double *virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return eval_host(b, fr, pos, z, c1, c2, c3, energies, forces, virials);
}

extern "C" int uf3_eval_atoms_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                  const double *c1, const double *c2, const double *c3, int64_t atom_begin,
                                  int64_t atom_end, double *d_energies, double *d_forces, double *d_virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (atom_end < 0) return fail(b->ctx, UF3_EINVAL, "uf3_eval_atoms: atom range outside the batch");
    EvalCall call;
    call.atom_begin = atom_begin; call.atom_end = atom_end;
    return eval_impl(b, fr, d_pos, d_z, c1, c2, c3, d_energies, d_forces, d_virials, call);
}

extern "C" int uf3_eval_atoms(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                              const double *c2, const double *c3, int64_t atom_begin, int64_t atom_end,
                              double *energies, double *forces, double *virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (atom_end < 0) return fail(b->ctx, UF3_EINVAL, "uf3_eval_atoms: atom range outside the batch");
    EvalCall call;
    call.atom_begin = atom_begin; call.atom_end = atom_end;
    return eval_host(b, fr, pos, z, c1, c2, c3, energies, forces, virials, call);
}

extern "C" int uf3_eval_centres_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z,
                                    const double *c1, const double *c2, const double *c3, int64_t atom_begin,
                                    int64_t atom_end, double *d_energies, double *d_forces, double *d_virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (atom_end < 0) return fail(b->ctx, UF3_EINVAL, "uf3_eval_centres: atom range outside the batch");
    EvalCall call;
    call.atom_begin = atom_begin; call.atom_end = atom_end; call.centre_share = true;
    return eval_impl(b, fr, d_pos, d_z, c1, c2, c3, d_energies, d_forces, d_virials, call);
}

extern "C" int uf3_eval_centres(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                                const double *c2, const double *c3, int64_t atom_begin, int64_t atom_end,
                                double *energies, double *forces, double *virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (atom_end < 0) return fail(b->ctx, UF3_EINVAL, "uf3_eval_centres: atom range outside the batch");
    EvalCall call;
    call.atom_begin = atom_begin; call.atom_end = atom_end; call.centre_share = true;
    return eval_host(b, fr, pos, z, c1, c2, c3, energies, forces, virials, call);
}

extern "C" int uf3_allreduce_sum_f64(uf3_ctx *c, double *d_buf, int64_t n);
// ------------------------------------------------------------------------------ the fit's accumulation, host arrays in (round 5)
// What pipeline.DeviceFitAccumulator.add_frames does with torch's buffers and streams, inside the library: frames (one pointer
// per frame: positions, atomic numbers, force targets -- no concatenation on the caller's side) are packed chunk by chunk into
// one of two pinned blocks, ONE transfer per chunk runs on a copy stream beside the previous chunk's kernels, the rows of a
// chunk live in HBM between the featurizer and the Gram kernels, and everything additive sits in one flat device buffer
// [G_e | G_f | o_e | o_f | m_e | m_f].  Reference: BasisFeaturizer.evaluate -> HDF5 -> WeightedLinearModel.fit_from_file
// (uf3/representation/process.py:121-291, uf3/regression/least_squares.py:355-483).
struct uf3_fit {
    uf3_basis *b = nullptr;
    uf3_ctx *c = nullptr;
    bool with_forces = true;
    int F = 0;
    int64_t max_atoms = 320000;
    double first_fraction = 0.125;
    int pack_threads = 4;
    Buf flat, xe, xf, frozen_idx, frozen_c;
    double *flat_ext = nullptr;      // the caller's device buffer for the pieces instead of `flat` (uf3_fit_use_flat)
    int n_frozen = 0;
    struct Set { PinBuf host; Buf dev; hipEvent_t copied = nullptr, consumed = nullptr; bool copied_live = false, consumed_live = false; } set[2];
    hipStream_t copy_stream = nullptr;
    double n_e = 0, n_f = 0;
    long long n_chunks = 0;
};

extern "C" void uf3_fit_destroy(uf3_fit *f) {
    if (!f) return;
    hipSetDevice(f->c->device);
    hipStreamSynchronize(f->c->stream);
    if (f->copy_stream) { hipStreamSynchronize(f->copy_stream); hipStreamDestroy(f->copy_stream); }
    for (auto &st : f->set) {
        st.host.release(); st.dev.release();
        if (st.copied) hipEventDestroy(st.copied);
        if (st.consumed) hipEventDestroy(st.consumed);
    }
    f->flat.release(); f->xe.release(); f->xf.release(); f->frozen_idx.release(); f->frozen_c.release();
    delete f;
}

extern "C" int uf3_fit_reset(uf3_fit *f) {
    if (!f) return fail(nullptr, UF3_EINVAL, "null fit");
    uf3_ctx *c = f->c;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(f->flat_ext ? (void *)f->flat_ext : f->flat.p, 0, 8 * (2 * (size_t)f->F * f->F + 2 * (size_t)f->F + 6), c->stream));
    f->n_e = f->n_f = 0; f->n_chunks = 0;
    return UF3_OK;
}

// the pieces into a device buffer of the caller's (2 F^2 + 2 F + 6 doubles, [G_e | G_f | o_e | o_f | m_e | m_f]; not zeroed here:
// uf3_fit_reset does that) -- so that frames given as host arrays and batches already resident in HBM (uf3_featurize_dev +
// uf3_gram*_dev by the caller) add up in one place.  NULL: back to the accumulator's own buffer.
// a call's first chunk holds this fraction of max_atoms_per_chunk and the following ones double it up to the limit (default 0.125:
// the GPU starts sooner; 1: chunks of equal size)
extern "C" int uf3_fit_first_chunk(uf3_fit *f, double fraction) {
    if (!f || !(fraction > 0.0) || fraction > 1.0) return fail(f ? f->c : nullptr, UF3_EINVAL, "uf3_fit_first_chunk: fraction in (0, 1]");
    f->first_fraction = fraction;
    return UF3_OK;
}

extern "C" int uf3_fit_use_flat(uf3_fit *f, double *d_flat) {
    if (!f) return fail(nullptr, UF3_EINVAL, "null fit");
    f->flat_ext = d_flat;
    return UF3_OK;
}

extern "C" int uf3_fit_create(uf3_basis *b, int with_forces, int64_t max_atoms_per_chunk, const int64_t *frozen_idx,
                              const double *frozen_c, int32_t n_frozen, uf3_fit **out) {
    if (!b || !out || n_frozen < 0 || (n_frozen && (!frozen_idx || !frozen_c))) return fail(b ? b->ctx : nullptr, UF3_EINVAL, "uf3_fit_create: bad argument");
    uf3_ctx *c = b->ctx;
    uf3_env_refresh();                      // (UF3_FIT_PACK_THREADS below: not a stale cache)
    HIPCHK(c, hipSetDevice(c->device));
    uf3_fit *f = new uf3_fit();
    f->b = b; f->c = c; f->with_forces = with_forces != 0; f->F = b->host.F;
    if (max_atoms_per_chunk > 0) f->max_atoms = max_atoms_per_chunk;
    f->n_frozen = n_frozen;
    if (const char *e = uf3_env("UF3_FIT_PACK_THREADS")) f->pack_threads = std::max(1, std::min(16, atoi(e)));
    auto bail = [&](int rc) { uf3_fit_destroy(f); return rc; };
    if (f->flat.ensure(8 * (2 * (size_t)f->F * f->F + 2 * (size_t)f->F + 6)) != hipSuccess) return bail(fail(c, UF3_ENOMEM, "uf3_fit_create: out of device memory"));
    if (n_frozen) {
        if (f->frozen_idx.ensure(8 * (size_t)n_frozen) != hipSuccess || f->frozen_c.ensure(8 * (size_t)n_frozen) != hipSuccess)
            return bail(fail(c, UF3_ENOMEM, "uf3_fit_create: out of device memory"));
        if (hipMemcpy(f->frozen_idx.p, frozen_idx, 8 * (size_t)n_frozen, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(f->frozen_c.p, frozen_c, 8 * (size_t)n_frozen, hipMemcpyHostToDevice) != hipSuccess)
            return bail(fail(c, UF3_EHIP, "uf3_fit_create: upload of the frozen columns failed"));
    }
    if (hipStreamCreateWithFlags(&f->copy_stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(c, UF3_EHIP, "uf3_fit_create: no copy stream"));
    for (auto &st : f->set)
        if (hipEventCreateWithFlags(&st.copied, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&st.consumed, hipEventDisableTiming) != hipSuccess)
            return bail(fail(c, UF3_EHIP, "uf3_fit_create: no events"));
    int rc = uf3_fit_reset(f);
    if (rc) return bail(rc);
    *out = f;
    return UF3_OK;
}

// The chunks of one uf3_fit_add call, [first, second) frame ranges (round 6: the plan, not the loop, decides).  The ramp:
// first_fraction of the limit, then doubling -- the GPU starts after a short pack, and the pack of chunk k + 1 (host, about half
// the GPU's time per frame on a one-species basis) hides behind the kernels of chunk k.  Behind the ramp the remaining frames are
// spread EVENLY over the fewest chunks of at most the limit (128 frames of 10 k atoms used to end on a 4-frame chunk --
// 4 + 8 + 16 + 3 x 32 + 4 -- whose launches fill the GPU for a fraction of their tails).  When no even spread keeps every chunk
// of two or more frames within the limit (uneven frames: [73, 109, 103] at a limit of 120 .. 200), the tail is packed greedily,
// which always does.  A chunk exceeds max_atoms only when it is a single frame.  Host only (uf3_fit_plan_debug).
static void fit_plan(int n_frames, const int64_t *atom_counts, int64_t max_atoms, double first_fraction,
                     std::vector<std::pair<int, int>> &plan) {
    plan.clear();
    double fr_ = first_fraction;
    int s0 = 0;
    while (s0 < n_frames && fr_ < 1.0) {
        const int64_t limit = std::max<int64_t>(1, (int64_t)(max_atoms * fr_));
        fr_ = std::min(1.0, 2.0 * fr_);
        int s1 = s0;
        int64_t atoms = 0;
        while (s1 < n_frames && (s1 == s0 || atoms + atom_counts[s1] <= limit)) atoms += atom_counts[s1++];
        plan.emplace_back(s0, s1);
        s0 = s1;
    }
    if (s0 >= n_frames) return;
    int64_t rest = 0;
    for (int i = s0; i < n_frames; i++) rest += atom_counts[i];
    for (int64_t n_chunks = (rest + max_atoms - 1) / max_atoms;; n_chunks++) {
        // chunk k ends behind the first frame at which the running atom count reaches (k + 1) / n_chunks of the rest
        std::vector<std::pair<int, int>> tail;
        int q0 = s0;
        int64_t run = 0;
        bool fits = true;
        for (int64_t k = 0; k < n_chunks && q0 < n_frames; k++) {
            const int64_t target = (rest * (k + 1) + n_chunks - 1) / n_chunks;
            int q1 = q0;
            int64_t atoms = 0;
            while (q1 < n_frames && (q1 == q0 || run + atoms < target)) atoms += atom_counts[q1++];
            if (k == n_chunks - 1) while (q1 < n_frames) atoms += atom_counts[q1++];
            fits = fits && (atoms <= max_atoms || q1 == q0 + 1);
            run += atoms;
            tail.emplace_back(q0, q1);
            q0 = q1;
        }
        if (fits) { plan.insert(plan.end(), tail.begin(), tail.end()); return; }
        if (n_chunks >= n_frames - s0) break;
    }
    // no even spread fits: greedy, each chunk as many frames as stay within the limit
    while (s0 < n_frames) {
        int s1 = s0;
        int64_t atoms = 0;
        while (s1 < n_frames && (s1 == s0 || atoms + atom_counts[s1] <= max_atoms)) atoms += atom_counts[s1++];
        plan.emplace_back(s0, s1);
        s0 = s1;
    }
}

extern "C" int uf3_fit_plan_debug(int32_t n_frames, const int64_t *atom_counts, int64_t max_atoms, double first_fraction,
                                  int32_t *chunk_ends, int32_t *n_chunks) {
    if (n_frames < 0 || (n_frames && !atom_counts) || !n_chunks || !(first_fraction > 0.0) || first_fraction > 1.0)
        return fail(nullptr, UF3_EINVAL, "uf3_fit_plan_debug: bad argument");
    for (int i = 0; i < n_frames; i++)
        if (atom_counts[i] <= 0) return fail(nullptr, UF3_EINVAL, "uf3_fit_plan_debug: a frame without atoms");
    std::vector<std::pair<int, int>> plan;
    fit_plan(n_frames, atom_counts, max_atoms > 0 ? max_atoms : 320000, first_fraction, plan);
    *n_chunks = (int32_t)plan.size();
    if (chunk_ends)
        for (size_t k = 0; k < plan.size(); k++) chunk_ends[k] = plan[k].second;
    return UF3_OK;
}

// frames: n_frames entries each of atom_counts / pos[f] ([N_f][3]) / z[f] ([N_f], int64 when z_is_int64 else int32) / cells
// ([n_frames][9]) / pbc ([n_frames][3]) / energies (total energy of the frame) / forces[f] ([N_f][3]; null array: no forces)
extern "C" int uf3_fit_add(uf3_fit *f, int32_t n_frames, const int64_t *atom_counts, const double *const *pos, const void *const *z,
                           int z_is_int64, const double *cells, const uint8_t *pbc, const double *energies, const double *const *forces) {
    if (!f) return fail(nullptr, UF3_EINVAL, "null fit");
    uf3_ctx *c = f->c;
    if (n_frames < 0 || (n_frames && (!atom_counts || !pos || !z || !cells || !pbc || !energies))) return fail(c, UF3_EINVAL, "uf3_fit_add: bad argument");
    if (f->with_forces && n_frames && !forces) return fail(c, UF3_EINVAL, "uf3_fit_add: this accumulator was set up with forces: pass them");
    HIPCHK(c, hipSetDevice(c->device));
    const int F = f->F;
    const size_t F2 = (size_t)F * F;
    double *flat = f->flat_ext ? f->flat_ext : f->flat.as<double>(), *gram_e = flat, *gram_f = flat + F2, *ord_e = flat + 2 * F2, *ord_f = ord_e + F, *mom = ord_f + F;
    int start = 0;
    for (int i = 0; i < n_frames; i++)
        if (atom_counts[i] <= 0) return fail(c, UF3_EINVAL, "uf3_fit_add: a frame without atoms (its per-atom energy target is undefined)");
    // the chunks of this call, planned ahead (fit_plan).  Every buffer is sized ONCE for the largest chunk (a Buf that grows chunk by
    // chunk frees and allocates -- an implicit device synchronisation -- in the middle of the copy / compute overlap).
    std::vector<std::pair<int, int>> plan;
    {
        fit_plan(n_frames, atom_counts, f->max_atoms, f->first_fraction, plan);
        int64_t big_atoms = 0, big_block = 0;
        int big_nf = 0;
        for (const auto &ch : plan) {
            int64_t atoms = 0;
            for (int i = ch.first; i < ch.second; i++) atoms += atom_counts[i];
            big_atoms = std::max(big_atoms, atoms); big_nf = std::max(big_nf, ch.second - ch.first);
            big_block = std::max<int64_t>(big_block, 6 * atoms + 2 * (int64_t)(ch.second - ch.first) + (atoms + 1) / 2);
        }
        if (big_atoms >= (1LL << 28)) return fail(c, UF3_EINVAL, "uf3_fit_add: a chunk must hold 1 .. 2^28 atoms");
        for (int q = 0; q < 2 && n_frames; q++) {
            uf3_fit::Set &st = f->set[q];
            if (8 * (size_t)big_block > st.host.cap && st.copied_live) { HIPCHK(c, hipEventSynchronize(st.copied)); st.copied_live = false; }
            HIPCHK(c, st.host.ensure(8 * (size_t)big_block));
            if (8 * (size_t)big_block > st.dev.cap && st.consumed_live) { HIPCHK(c, hipEventSynchronize(st.consumed)); st.consumed_live = false; }
            HIPCHK(c, st.dev.ensure(8 * (size_t)big_block));
        }
        if (n_frames) {
            if (8 * (size_t)big_nf * F > f->xe.cap || (f->with_forces && 24 * (size_t)big_atoms * F > f->xf.cap)) HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, f->xe.ensure(8 * (size_t)big_nf * F));
            if (f->with_forces) HIPCHK(c, f->xf.ensure(24 * (size_t)big_atoms * F));
        }
    }
    for (const auto &chunk : plan) {
        start = chunk.first;
        const int stop = chunk.second;
        int64_t atoms = 0;
        for (int i = start; i < stop; i++) atoms += atom_counts[i];
        const int nf = stop - start;
        if (atoms < 1 || atoms >= (1LL << 28)) return fail(c, UF3_EINVAL, "uf3_fit_add: a chunk must hold 1 .. 2^28 atoms");
        // block layout, host and device alike: positions [3 A] | force targets [3 A] | per-atom energies [nf] | atom counts [nf] | species [A] (int32)
        const size_t A3 = 3 * (size_t)atoms, n_block = 2 * A3 + 2 * (size_t)nf + ((size_t)atoms + 1) / 2;
        uf3_fit::Set &st = f->set[f->n_chunks & 1];
        if (st.copied_live) { HIPCHK(c, hipEventSynchronize(st.copied)); st.copied_live = false; }      // (the pinned block is free again)
        HIPCHK(c, st.host.ensure(8 * n_block));
        if (8 * n_block > st.dev.cap && st.consumed_live) { HIPCHK(c, hipEventSynchronize(st.consumed)); st.consumed_live = false; }
        HIPCHK(c, st.dev.ensure(8 * n_block));
        double *h = (double *)st.host.p, *h_pos = h, *h_yf = h + A3, *h_ye = h + 2 * A3, *h_cnt = h_ye + nf;
        int32_t *h_z = (int32_t *)(h_cnt + nf);
        std::vector<int64_t> offsets(nf + 1, 0);
        for (int i = 0; i < nf; i++) {
            const int64_t n = atom_counts[start + i];
            if (n && (!pos[start + i] || !z[start + i] || (f->with_forces && !forces[start + i]))) return fail(c, UF3_EINVAL, "uf3_fit_add: null frame array");
            offsets[i + 1] = offsets[i] + n;
        }
        auto pack = [&](int i0, int i1) {
            for (int i = i0; i < i1; i++) {
                const int64_t n = atom_counts[start + i], k = offsets[i];
                std::memcpy(h_pos + 3 * k, pos[start + i], 24 * (size_t)n);
                if (z_is_int64) { const int64_t *zz = (const int64_t *)z[start + i]; for (int64_t q = 0; q < n; q++) h_z[k + q] = (int32_t)zz[q]; }
                else std::memcpy(h_z + k, z[start + i], 4 * (size_t)n);
                if (f->with_forces) std::memcpy(h_yf + 3 * k, forces[start + i], 24 * (size_t)n);
                h_cnt[i] = (double)n;
                h_ye[i] = energies[start + i] / (double)n;      // per-atom normalisation of the targets (least_squares.py:697-700)
            }
        };
        // big chunks are packed by a few threads (a single core copies ~8 GB/s into pinned memory: 2 ms per 32 frames of 10 k atoms)
        // (from two frames of 10 k atoms on: one core packs 0.18 ms per such frame, the GPU takes 0.145 on a one-species basis)
        const int n_thr = (atoms >= 20000 && nf >= 2) ? std::min(f->pack_threads, nf) : 1;
        if (n_thr > 1) {
            std::vector<std::thread> thr;
            int done_to = nf / n_thr;                   // frames [0, done_to) are this thread's; a thread that cannot be started leaves its share to it too
            std::vector<std::pair<int, int>> mine;
            for (int t = 1; t < n_thr; t++) {
                const int i0 = (int)((int64_t)nf * t / n_thr), i1 = (int)((int64_t)nf * (t + 1) / n_thr);
                try { thr.emplace_back(pack, i0, i1); } catch (...) { mine.emplace_back(i0, i1); }
            }
            pack(0, done_to);
            for (auto &r : mine) pack(r.first, r.second);
            for (auto &t : thr) t.join();
        } else pack(0, nf);
        if (st.consumed_live) HIPCHK(c, hipStreamWaitEvent(f->copy_stream, st.consumed, 0));            // (the device block is free again)
        HIPCHK(c, hipMemcpyAsync(st.dev.p, st.host.p, 8 * n_block, hipMemcpyHostToDevice, f->copy_stream));
        HIPCHK(c, hipEventRecord(st.copied, f->copy_stream));
        st.copied_live = true;
        HIPCHK(c, hipStreamWaitEvent(c->stream, st.copied, 0));
        double *d = st.dev.as<double>(), *d_pos = d, *d_yf = d + A3, *d_ye = d + 2 * A3, *d_cnt = d_ye + nf;
        const int32_t *d_z = (const int32_t *)(d_cnt + nf);
        // the rows of this chunk (the previous chunk's kernels are ahead of these launches on the same stream)
        HIPCHK(c, f->xe.ensure(8 * (size_t)nf * F));
        if (f->with_forces) HIPCHK(c, f->xf.ensure(8 * A3 * F));
        uf3_frames fr;
        fr.n_frames = nf; fr.atom_offsets = offsets.data(); fr.cells = cells + 9 * (size_t)start; fr.pbc = pbc + 3 * (size_t)start;
        int rc = uf3_featurize_dev(f->b, &fr, d_pos, d_z, f->xe.as<double>(), f->with_forces ? f->xf.as<double>() : nullptr);
        if (rc) return rc;
        rc = uf3_fit_rows_dev(c, nf, F, f->xe.as<double>(), d_cnt, d_ye, f->with_forces ? d_yf : nullptr, f->with_forces ? (int64_t)A3 : 0,
                              f->n_frozen ? f->frozen_idx.as<int64_t>() : nullptr, f->n_frozen ? f->frozen_c.as<double>() : nullptr, f->n_frozen, mom);
        if (rc) return rc;
        rc = uf3_gram_dev(c, f->xe.as<double>(), d_ye, nf, F, F, 1, gram_e, ord_e);
        if (rc) return rc;
        if (f->with_forces) {
            rc = uf3_gram_force_rows_dev(f->b, f->xf.as<double>(), d_yf, d_z, atoms, F, 1, gram_f, ord_f);
            if (rc) return rc;
        }
        HIPCHK(c, hipEventRecord(st.consumed, c->stream));
        st.consumed_live = true;
        f->n_e += nf;
        if (f->with_forces) f->n_f += (double)A3;
        f->n_chunks++;
    }
    return UF3_OK;
}

// the additive pieces of this rank over the n_keep unfrozen columns, frozen columns folded out: [G_e | G_f | o_e | o_f | m_e | m_f]
// (2 n_keep^2 + 2 n_keep + 6 doubles) into host memory; allreduce != 0: summed over the ranks of the context's communicator first
extern "C" int uf3_fit_pack(uf3_fit *f, const int64_t *keep, int32_t n_keep, int allreduce, double *out_host) {
    if (!f || !out_host || n_keep < 0 || n_keep > f->F || (n_keep && !keep)) return fail(f ? f->c : nullptr, UF3_EINVAL, "uf3_fit_pack: bad argument");
    uf3_ctx *c = f->c;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = uf3_ctx_synchronize(c);                  // (verdicts on the asynchronous featurizer calls: UF3_ERETRY = start over)
    if (rc) return rc;
    const size_t n = 2 * (size_t)n_keep * n_keep + 2 * (size_t)n_keep + 6;
    Buf d_keep, d_out;
    HIPCHK(c, d_keep.ensure(8 * (size_t)std::max(n_keep, 1)));
    HIPCHK(c, d_out.ensure(8 * n));
    auto done = [&](int r) { hipStreamSynchronize(c->stream); d_keep.release(); d_out.release(); return r; };
    if (n_keep && hipMemcpyAsync(d_keep.p, keep, 8 * (size_t)n_keep, hipMemcpyHostToDevice, c->stream) != hipSuccess) return done(fail(c, UF3_EHIP, "uf3_fit_pack: upload failed"));
    rc = uf3_fit_pack_dev(c, f->F, f->flat_ext ? f->flat_ext : f->flat.as<double>(), d_keep.as<int64_t>(), n_keep, f->n_frozen ? f->frozen_idx.as<int64_t>() : nullptr,
                          f->n_frozen ? f->frozen_c.as<double>() : nullptr, f->n_frozen, f->n_e, f->n_f, d_out.as<double>());
    if (rc) return done(rc);
    if (allreduce && c->comm) { rc = uf3_allreduce_sum_f64(c, d_out.as<double>(), (int64_t)n); if (rc) return done(rc); }
    if (hipMemcpyAsync(out_host, d_out.p, 8 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return done(fail(c, UF3_EHIP, "uf3_fit_pack: download failed"));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return done(fail(c, UF3_EHIP, "uf3_fit_pack: stream"));
    return done(UF3_OK);
}

extern "C" int uf3_fit_info(const uf3_fit *f, int64_t *n_chunks, double *n_energy_rows, double *n_force_rows) {
    if (!f) return fail(nullptr, UF3_EINVAL, "null fit");
    if (n_chunks) *n_chunks = f->n_chunks;
    if (n_energy_rows) *n_energy_rows = f->n_e;
    if (n_force_rows) *n_force_rows = f->n_f;
    return UF3_OK;
}

// ------------------------------------------------------------------------------ RCCL behind the C ABI
// One process per GPU; the ONE exchange of the path is the sum of the packed normal-equation pieces (and, for a decomposed
// frame, of [forces | energy | strain derivative]) over the ranks -- what the reference does by returning per-chunk results
// to the parent process and adding them there (uf3/representation/process.py:196-254, uf3/regression/least_squares.py:
// 391-412); SURVEY 8b's `uf3_gram_allreduce`.  librccl is opened at run time: the copy already in the process (a PyTorch-ROCm
// wheel brings its own, next to its own HIP runtime, and two HIP runtimes in one process do not mix), else UF3_RCCL_PATH,
// else the system's.
struct RcclId { char b[128]; };            // ncclUniqueId, passed by value
struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, RcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why;
};
static RcclApi &rccl_api() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api;
    tried = true;
    const char *names[] = {uf3_env("UF3_RCCL_PATH"), "librccl.so.1", "librccl.so"};
    for (int pass = 0; pass < 2 && !api.lib; pass++)                 // first: whatever is loaded already
        for (const char *nm : names) {
            if (!nm || api.lib) continue;
            api.lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
        }
    if (!api.lib) { api.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return api; }
    api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
    api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce) { api.why = "librccl lacks the nccl* entry points"; api.lib = nullptr; }
    return api;
}
static int rccl_fail(uf3_ctx *c, const char *what, int rc) {
    RcclApi &r = rccl_api();
    return fail(c, UF3_EHIP, std::string(what) + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}

extern "C" int uf3_comm_unique_id(uf3_ctx *c, void *id128) {
    uf3_env_refresh();
    if (!c || !id128) return fail(c, UF3_EINVAL, "uf3_comm_unique_id: null argument");
    RcclApi &r = rccl_api();
    if (!r.lib) return fail(c, UF3_EHIP, r.why);
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = r.GetUniqueId(id128);
    return rc ? rccl_fail(c, "ncclGetUniqueId", rc) : UF3_OK;
}

extern "C" int uf3_comm_init(uf3_ctx *c, int n_ranks, int rank, const void *id128) {
    uf3_env_refresh();
    if (!c || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, UF3_EINVAL, "uf3_comm_init: bad argument");
    RcclApi &r = rccl_api();
    if (!r.lib) return fail(c, UF3_EHIP, r.why);
    if (c->comm) { int rc0 = uf3_comm_destroy(c); if (rc0) return rc0; }
    HIPCHK(c, hipSetDevice(c->device));
    RcclId id;
    std::memcpy(id.b, id128, sizeof(id.b));
    const int rc = r.CommInitRank(&c->comm, n_ranks, id, rank);
    if (rc) { c->comm = nullptr; return rccl_fail(c, "ncclCommInitRank", rc); }
    c->comm_ranks = n_ranks; c->comm_rank = rank;
    return UF3_OK;
}

extern "C" int uf3_comm_destroy(uf3_ctx *c) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (!c->comm) return UF3_OK;
    RcclApi &r = rccl_api();
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    const int rc = r.CommDestroy ? r.CommDestroy(c->comm) : 0;
    c->comm = nullptr; c->comm_ranks = 0; c->comm_rank = -1;
    return rc ? rccl_fail(c, "ncclCommDestroy", rc) : UF3_OK;
}

extern "C" int uf3_comm_info(const uf3_ctx *c, int32_t *n_ranks, int32_t *rank) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_ranks) *n_ranks = c->comm ? c->comm_ranks : 0;
    if (rank) *rank = c->comm ? c->comm_rank : -1;
    return UF3_OK;
}

// in place, on the context's stream, asynchronous like every *_dev entry
extern "C" int uf3_allreduce_sum_f64(uf3_ctx *c, double *d_buf, int64_t n) {
    if (!c || (n > 0 && !d_buf) || n < 0) return fail(c, UF3_EINVAL, "uf3_allreduce_sum_f64: bad argument");
    if (!c->comm) return fail(c, UF3_EINVAL, "uf3_allreduce_sum_f64: no communicator (uf3_comm_init)");
    if (n == 0) return UF3_OK;
    RcclApi &r = rccl_api();
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = r.AllReduce(d_buf, d_buf, (size_t)n, /* ncclFloat64 */ 8, /* ncclSum */ 0, c->comm, c->stream);
    return rc ? rccl_fail(c, "ncclAllReduce", rc) : UF3_OK;
}

extern "C" int uf3_gram_allreduce(uf3_ctx *c, double *d_packed, int64_t n) { return uf3_allreduce_sum_f64(c, d_packed, n); }

// ------------------------------------------------------------------------------ gram
static int ensure_frag(uf3_ctx *c) {
    if (c->frag_ready) return UF3_OK;
    HIPCHK(c, c->frag.ensure(sizeof(int) * 64 * 4 * 2));
    hipLaunchKernelGGL(k_mfma_probe, dim3(1), dim3(64), 0, c->stream, c->frag.as<int>());
    int tab[512];
    HIPCHK(c, hipMemcpyAsync(tab, c->frag.p, sizeof(tab), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool seen[256] = {false};
    for (int q = 0; q < 256; q++) {
        int r = tab[2 * q], cc = tab[2 * q + 1];
        if (r < 0 || r > 15 || cc < 0 || cc > 15 || seen[r * 16 + cc])
            return fail(c, UF3_EHIP, "unexpected v_mfma_f64_16x16x4 fragment layout");
        seen[r * 16 + cc] = true;
    }
    c->frag_ready = true;
    return UF3_OK;
}

// k_gram_tiled over all rows and columns (rowmap == nullptr), or over the rows rowmap[seg[0] .. seg[0] + seg[1]) -- seg on the
// device -- and the n_cols columns of colmap: n_rows is then the bound the grid covers, n_rows_plan what a segment is expected
// to hold (the chunks are cut for it; workgroups past the segment leave at once).  Accumulates the upper triangle.
static int launch_gram_tiled(uf3_ctx *c, const double *dx, const double *dy, int64_t n_rows, int64_t n_rows_plan, int n_feat,
                             int64_t ld, double *d_gram, double *d_ord, const int *rowmap, const int *seg, const int *colmap,
                             int n_cols, int accumulate) {
    hipStream_t st = c->stream;
    const int np = (n_cols + 63) / 64;
    // LDS-tiled kernel: patches of 64 x 64 packed into workgroups (at most four patches on at most four column ranges)
    int ps = -1;
    // (one slot per species' column subset + the full matrix: a basis of UF3_MAX_SPECIES species never evicts)
    const int n_slots = UF3_MAX_SPECIES + 1;
    for (int q = 0; q < n_slots; q++) if (c->gram_plan_np[q] == np) ps = q;
    const bool plan_new = ps < 0;
    if (ps < 0) {
        ps = c->gram_plan_next;
        c->gram_plan_next = (ps + 1) % n_slots;
        std::vector<GramBlock> plan;
        auto fresh = [&]() { GramBlock g; memset(&g, 0, sizeof g); for (int q = 0; q < 4; q++) g.range[q] = -1; return g; };
        auto slot_of = [&](GramBlock &g, int r, bool add) {
            for (int q = 0; q < 4; q++) if (g.range[q] == r) return q;
            if (add) for (int q = 0; q < 4; q++) if (g.range[q] < 0) { g.range[q] = r; return q; }
            return -1;
        };
        auto n_waves = [&](const GramBlock &g) { int n = 0; for (int w = 0; w < 4; w++) n += g.kind[w] != 0; return n; };
        auto fits = [&](const GramBlock &g, int pa, int pb) {
            if (n_waves(g) >= 4) return false;
            int free_slots = 0, need = 0;
            bool has_a = false, has_b = false;
            for (int q = 0; q < 4; q++) { free_slots += g.range[q] < 0; has_a |= g.range[q] == pa; has_b |= g.range[q] == pb; }
            need = (has_a ? 0 : 1) + ((has_b || pb == pa) ? 0 : 1);
            return need <= free_slots;
        };
        auto add_patch = [&](GramBlock &g, int pa, int pb) {
            const int w = n_waves(g);
            g.wa[w] = slot_of(g, pa, true); g.wb[w] = slot_of(g, pb, true);
            g.kind[w] = pa == pb ? 2 : 1;
            if (pa == pb) g.ord_mask |= 1 << g.wa[w];
        };
        // diagonal patches four at a time (equal work per wave)
        for (int p0 = 0; p0 < np; p0 += 4) {
            GramBlock g = fresh();
            for (int p = p0; p < std::min(np, p0 + 4); p++) add_patch(g, p, p);
            plan.push_back(g);
        }
        // off-diagonal patches four to a workgroup on at most four ranges: greedy (to the patch that opened the workgroup add
        // the ones that need no new range, then one, then two), over the natural order and a few shuffles of it; the fewest
        // workgroups win (every workgroup costs the time of a full patch, however many of its waves have one)
        std::vector<std::pair<int, int>> pairs;
        for (int pa = 0; pa < np; pa++) for (int pb = pa + 1; pb < np; pb++) pairs.push_back({pa, pb});
        std::vector<GramBlock> best;
        unsigned lcg = 12345u;
        for (int attempt = 0; attempt < 64; attempt++) {
            std::vector<std::pair<int, int>> left = pairs;
            if (attempt)
                for (size_t q = left.size(); q > 1; q--) { lcg = lcg * 1664525u + 1013904223u; std::swap(left[q - 1], left[(lcg >> 8) % q]); }
            std::vector<GramBlock> blocks;
            while (!left.empty()) {
                GramBlock g = fresh();
                add_patch(g, left[0].first, left[0].second);
                left.erase(left.begin());
                while (n_waves(g) < 4 && !left.empty()) {
                    int pick = -1;
                    for (int need = 0; need <= 2 && pick < 0; need++)
                        for (size_t q = 0; q < left.size() && pick < 0; q++) {
                            const int n_new = (slot_of(g, left[q].first, false) < 0) + (slot_of(g, left[q].second, false) < 0);
                            if (n_new == need && fits(g, left[q].first, left[q].second)) pick = (int)q;
                        }
                    if (pick < 0) break;
                    add_patch(g, left[pick].first, left[pick].second);
                    left.erase(left.begin() + pick);
                }
                blocks.push_back(g);
            }
            if (best.empty() || blocks.size() < best.size()) best = blocks;
            if (best.size() * 4 < pairs.size() + 4) break;                  // (cannot get better)
        }
        for (auto &g : best) plan.push_back(g);
        for (auto &g : plan)
            for (int q = 0; q < 4; q++) if (g.range[q] < 0) g.range[q] = g.range[0];
        c->gram_plan_np[ps] = 0;
        HIPCHK(c, hipDeviceSynchronize());                             // (a launch -- on this or an earlier stream of the context -- may still be reading the plan this one replaces)
        HIPCHK(c, c->gram_tiles[ps].ensure(sizeof(GramBlock) * plan.size()));
        HIPCHK(c, hipMemcpyAsync(c->gram_tiles[ps].p, plan.data(), sizeof(GramBlock) * plan.size(), hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        c->gram_plan_np[ps] = np; c->gram_plan_blocks[ps] = (int)plan.size();
    }
    // row chunks: about two rounds of workgroups over the chip's resident slots (two per CU)
    const int bpc = c->gram_plan_blocks[ps];
    // (measured flat between two and twelve workgroups per CU)
    const int want_chunks = std::max(8, (c->n_cu * 4 + bpc - 1) / bpc / 8 * 8);
    int64_t rpc = (n_rows_plan + want_chunks - 1) / want_chunks;
    rpc = std::max<int64_t>(256, (rpc + GT_KS - 1) / GT_KS * GT_KS);
    const int chunks = (int)((n_rows + rpc - 1) / rpc), chunks8 = (chunks + 7) / 8 * 8;
    if (rowmap)
        hipLaunchKernelGGL(k_gram_tiled<true>, dim3(bpc * chunks8), dim3(256), 0, st, dx, (d_ord && dy) ? dy : nullptr, n_rows, n_feat,
                           ld, (int)rpc, bpc, (const GramBlock *)c->gram_tiles[ps].p, c->frag.as<int>(), d_gram, d_ord, rowmap, seg, colmap,
                           n_cols);
    else
        hipLaunchKernelGGL(k_gram_tiled<false>, dim3(bpc * chunks8), dim3(256), 0, st, dx, (d_ord && dy) ? dy : nullptr, n_rows, n_feat,
                           ld, (int)rpc, bpc, (const GramBlock *)c->gram_tiles[ps].p, c->frag.as<int>(), d_gram, d_ord,
                           (const int *)nullptr, (const int *)nullptr, (const int *)nullptr, n_feat);
    HIPCHK(c, hipGetLastError());
    // (UF3_DEBUG_LDS: which Gram kernel ran, as the k_eval lines -- tests assert the route they mean to reach)
    if (c->env_debug_lds)
        fprintf(stderr, "uf3: gram kernel=%s rows=%lld feat=%d ld=%lld acc=%d ord=%d cols=%d plan_slot=%d plan_new=%d\n",
                rowmap ? "tiled_sub" : "tiled", (long long)n_rows, n_feat, (long long)ld, accumulate ? 1 : 0, (d_ord && dy) ? 1 : 0,
                n_cols, ps, (int)plan_new);
    return UF3_OK;
}

extern "C" int uf3_gram_dev(uf3_ctx *c, const double *dx, const double *dy, int64_t n_rows, int32_t n_feat, int64_t ld,
                            int accumulate, double *d_gram, double *d_ord) {
    uf3_env_refresh();
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (!dx || !d_gram || n_feat < 1 || ld < n_feat || n_rows < 0) return fail(c, UF3_EINVAL, "uf3_gram: bad argument");
    read_f3_env(c);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_frag(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if (!accumulate) {
        HIPCHK(c, hipMemsetAsync(d_gram, 0, 8 * (size_t)n_feat * n_feat, st));
        if (d_ord) HIPCHK(c, hipMemsetAsync(d_ord, 0, 8 * (size_t)n_feat, st));
    }
    if (n_rows == 0) return UF3_OK;
    // (up to two column ranges the patches are mostly padding: one wave per 32 x 32 tile with direct loads is faster there --
    // measured 0.62 against 0.81 ms at F = 73, 960 k rows)
    // (and below ~64 k rows the row chunks get too short for the slab pipeline: 0.24 against 0.21 ms at 30 001 x 425)
    if (n_feat > 128 && n_rows >= 65536) {
        // LDS-tiled kernel: patches of 64 x 64 packed into workgroups (at most four patches on at most four column ranges)
        Timed tm(c, T_GRAM);
        rc = launch_gram_tiled(c, dx, dy, n_rows, n_rows, n_feat, ld, d_gram, d_ord, nullptr, nullptr, nullptr, n_feat, accumulate);
        if (rc) return rc;
        hipLaunchKernelGGL(k_gram_mirror, dim3((n_feat + 255) / 256, n_feat), dim3(256), 0, st, d_gram, n_feat);
        HIPCHK(c, hipGetLastError());
        return UF3_OK;
    }
    if (n_feat <= GS_LDW && n_rows >= 16384) {
        // narrow matrices: slabs of 32 rows through LDS, every row read once (k_gram_small); about eight workgroups per CU
        const int64_t want_blocks = (int64_t)c->n_cu * 8;
        int64_t rpb = (n_rows + want_blocks - 1) / want_blocks;
        rpb = std::max<int64_t>(4 * GS_ROWS, (rpb + GS_ROWS - 1) / GS_ROWS * GS_ROWS);
        const int64_t blocks = (n_rows + rpb - 1) / rpb;
        Timed tm(c, T_GRAM);
        hipLaunchKernelGGL(k_gram_small, dim3((unsigned)blocks), dim3(256), 0, st, dx, (d_ord && dy) ? dy : nullptr, n_rows, n_feat, ld,
                           rpb, c->frag.as<int>(), d_gram, d_ord);
        hipLaunchKernelGGL(k_gram_mirror, dim3((n_feat + 255) / 256, n_feat), dim3(256), 0, st, d_gram, n_feat);
        HIPCHK(c, hipGetLastError());
        if (c->env_debug_lds)
            fprintf(stderr, "uf3: gram kernel=small rows=%lld feat=%d ld=%lld acc=%d ord=%d\n", (long long)n_rows, n_feat, (long long)ld,
                    accumulate ? 1 : 0, (d_ord && dy) ? 1 : 0);
        return UF3_OK;
    }
    // tile-pair table of the direct kernel: built and uploaded when n_feat changes (its own buffer and key: a fit that sends
    // its energy rows here and its force rows to the tiled kernel keeps both plans)
    const int nt = (n_feat + 31) / 32;
    size_t np = (size_t)nt * (nt + 1) / 2;
    np = (np + 3) / 4 * 4;
    const bool table_new = c->gram_direct_feat != n_feat;
    if (table_new) {
        std::vector<int> tij;
        for (int i = 0; i < nt; i++) for (int j = i; j < nt; j++) tij.push_back(i);
        while (tij.size() < np) tij.push_back(-1);
        for (int i = 0; i < nt; i++) for (int j = i; j < nt; j++) tij.push_back(j);
        while (tij.size() < 2 * np) tij.push_back(-1);
        c->gram_direct_feat = 0;
        // (a k_gram_mfma on this or an earlier stream of the context may still be reading the table this one overwrites in place
        // when it fits the buffer: the same order as the tiled plan's)
        if (c->gram_tij.p) HIPCHK(c, hipDeviceSynchronize());
        HIPCHK(c, c->gram_tij.ensure(8 * np));
        HIPCHK(c, hipMemcpyAsync(c->gram_tij.p, tij.data(), 8 * np, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));                           // (tij is a local)
        c->gram_direct_feat = n_feat;
    }
    int *d_ti = c->gram_tij.as<int>(), *d_tj = d_ti + np;
    // enough row chunks to fill the chip, each a multiple of 4 rows
    int blocks_xy = (int)(np / 4);
    int want_chunks = std::max(1, (c->n_cu * 8 + blocks_xy - 1) / blocks_xy);
    int64_t rpc = (n_rows + want_chunks - 1) / want_chunks;
    rpc = std::max<int64_t>(64, (rpc + 3) / 4 * 4);
    int chunks = (int)((n_rows + rpc - 1) / rpc);
    {
        Timed tm(c, T_GRAM);
        const int chunks8 = (chunks + 7) / 8 * 8;                  // whole rounds over the 8 XCDs
        hipLaunchKernelGGL(k_gram_mfma, dim3(blocks_xy * chunks8), dim3(256), 0, st, dx, (d_ord && dy) ? dy : nullptr, n_rows, n_feat, ld,
                           (int)rpc, blocks_xy, d_ti, d_tj, c->frag.as<int>(), d_gram, d_ord);
        hipLaunchKernelGGL(k_gram_mirror, dim3((n_feat + 255) / 256, n_feat), dim3(256), 0, st, d_gram, n_feat);
    }
    HIPCHK(c, hipGetLastError());
    if (c->env_debug_lds)
        fprintf(stderr, "uf3: gram kernel=mfma rows=%lld feat=%d ld=%lld acc=%d ord=%d table_new=%d\n", (long long)n_rows, n_feat,
                (long long)ld, accumulate ? 1 : 0, (d_ord && dy) ? 1 : 0, (int)table_new);
    return UF3_OK;
}

extern "C" int uf3_gram_force_rows_dev(uf3_basis *b, const double *d_x_f, const double *d_y_f, const int32_t *d_z, int64_t n_atoms,
                                       int64_t ld, int accumulate, double *d_gram, double *d_ord) {
    uf3_env_refresh();
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    const int F = b->host.F, S = b->host.S;
    if (!d_x_f || !d_gram || !d_z || n_atoms < 0 || ld < F || 3 * n_atoms > INT32_MAX)
        return fail(c, UF3_EINVAL, "uf3_gram_force_rows_dev: bad argument");
    read_f3_env(c);
    int widest = 0;
    for (int sp = 0; sp < S; sp++) widest = std::max(widest, b->sp_ncols[sp]);
    // One species, a narrow matrix or short segments: the plain product (same result; the zero columns are multiplied).  Also
    // when no species leaves out at least one 64-column range's worth of columns.
    if (S < 2 || F <= 128 || 3 * n_atoms / S < 65536 || (widest + 63) / 64 >= (F + 63) / 64)
        return uf3_gram_dev(c, d_x_f, d_y_f, 3 * n_atoms, F, ld, accumulate, d_gram, d_ord);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_frag(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if (!accumulate) {
        HIPCHK(c, hipMemsetAsync(d_gram, 0, 8 * (size_t)F * F, st));
        if (d_ord) HIPCHK(c, hipMemsetAsync(d_ord, 0, 8 * (size_t)F, st));
    }
    if (n_atoms == 0) return UF3_OK;
    // row lists by species (readable two slabs past the end: the kernel fetches row indices a slab ahead)
    const size_t n_list = 3 * (size_t)n_atoms + 2 * GT_KS + 8;
    HIPCHK(c, c->sp_rows.ensure(sizeof(int) * n_list));
    HIPCHK(c, c->sp_seg.ensure(sizeof(int) * 3 * UF3_MAX_SPECIES));
    int *seg = c->sp_seg.as<int>(), *cursor = seg + 2 * UF3_MAX_SPECIES, *rows = c->sp_rows.as<int>();
    Timed tm(c, T_GRAM);
    // the lists are refilled in place: after the previous call's launches that read them, whichever stream they ran on
    if (!c->sp_done) HIPCHK(c, hipEventCreateWithFlags(&c->sp_done, hipEventDisableTiming));
    if (c->sp_done_live) HIPCHK(c, hipStreamWaitEvent(st, c->sp_done, 0));
    HIPCHK(c, hipMemsetAsync(seg, 0, sizeof(int) * 3 * UF3_MAX_SPECIES, st));
    // (the whole list: k_species_rows skips atoms whose species is outside the basis, so entries between the end of the segments
    // and 3 n_atoms would otherwise be uninitialised row indices for the kernel's one-slab-ahead prefetch; 12 bytes per atom)
    HIPCHK(c, hipMemsetAsync(rows, 0, sizeof(int) * n_list, st));
    const unsigned nblk = (unsigned)((n_atoms + SR_ATOMS - 1) / SR_ATOMS);
    hipLaunchKernelGGL(k_species_rows, dim3(nblk), dim3(256), 0, st, (const BasisDev *)b->dev, d_z, n_atoms, 0, seg, cursor, rows);
    hipLaunchKernelGGL(k_species_rows, dim3(nblk), dim3(256), 0, st, (const BasisDev *)b->dev, d_z, n_atoms, 1, seg, cursor, rows);
    for (int sp = 0; sp < S; sp++) {
        if (b->sp_ncols[sp] == 0) continue;
        rc = launch_gram_tiled(c, d_x_f, d_y_f, 3 * n_atoms, 3 * n_atoms / S, F, ld, d_gram, d_ord, rows, seg + 2 * sp,
                               b->d_sp_cols + (size_t)sp * F, b->sp_ncols[sp], accumulate);
        if (rc) return rc;
    }
    HIPCHK(c, hipEventRecord(c->sp_done, st));
    c->sp_done_live = true;
    hipLaunchKernelGGL(k_gram_mirror, dim3((F + 255) / 256, F), dim3(256), 0, st, d_gram, F);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_gram(uf3_ctx *c, const double *x, const double *y, int64_t n_rows, int32_t n_feat, int64_t ld,
                        int accumulate, double *gram, double *ord) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (!x || !gram || n_feat < 1 || ld < n_feat || n_rows < 0) return fail(c, UF3_EINVAL, "uf3_gram: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    // the rows in stage_out2 (with the 64 bytes of slack behind them that the block has always had), the sums in stage_out
    Stage I(c->stage_out2, c->stream), O(c->stage_out, c->stream);
    const int s_x = I.add(8 * (size_t)n_rows * ld), s_y = I.add(8 * (size_t)n_rows, y != nullptr);
    I.add(64);
    const int s_g = O.add(8 * (size_t)n_feat * n_feat), s_o = O.add(8 * (size_t)n_feat, ord != nullptr);
    HIPCHK(c, I.alloc());
    HIPCHK(c, O.alloc());
    HIPCHK(c, I.in({{s_x, x}, {s_y, y}}));
    if (accumulate) HIPCHK(c, O.in({{s_g, gram}, {s_o, ord}}));
    int rc = uf3_gram_dev(c, I.at<double>(s_x), I.at<double>(s_y), n_rows, n_feat, ld, accumulate, O.at<double>(s_g),
                          y ? O.at<double>(s_o) : nullptr);
    if (rc) return rc;
    HIPCHK(c, O.out({{s_g, gram}, {s_o, y ? ord : nullptr}}));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ leverage (uf3_leverage.h)
extern "C" int uf3_leverage_dev(uf3_ctx *c, const double *d_x, int64_t n_rows, int32_t n_feat, int64_t ld, const double *d_w,
                                int32_t group, double *d_q) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_rows < 0 || n_feat < 1 || ld < n_feat || (group != 1 && group != 3) || n_rows % group != 0 ||
        n_rows / LV_ROWS >= INT32_MAX || (n_rows && (!d_x || !d_w || !d_q)))
        return fail(c, UF3_EINVAL, "uf3_leverage: bad argument (group is 1 or 3 and divides n_rows, ld >= n_feat >= 1)");
    if (n_rows == 0) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_frag(c);
    if (rc) return rc;
    const unsigned blocks = (unsigned)((n_rows + LV_ROWS - 1) / LV_ROWS);
    hipLaunchKernelGGL(k_leverage, dim3(blocks), dim3(256), 0, c->stream, d_x, n_rows, n_feat, ld, d_w, group, c->frag.as<int>(), d_q);
    HIPCHK(c, hipGetLastError());
    if (c->env_debug_lds) {
        const int nt = (n_feat + 15) / 16;
        fprintf(stderr, "uf3: leverage kernel=k_leverage rows=%lld feat=%d ld=%lld group=%d blocks=%u rows_per_block=%d lds=%zu B "
                "slab=%d passes=%d\n", (long long)n_rows, n_feat, (long long)ld, group, blocks, LV_ROWS,
                sizeof(double) * (LV_ROWS * LV_LDW + 128), LV_SLAB, (nt + 4 * LV_KT - 1) / (4 * LV_KT));
    }
    return UF3_OK;
}

extern "C" int uf3_leverage(uf3_ctx *c, const double *x, int64_t n_rows, int32_t n_feat, int64_t ld, const double *w, int32_t group,
                            double *q) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_rows < 0 || n_feat < 1 || ld < n_feat || (group != 1 && group != 3) || n_rows % group != 0 || (n_rows && (!x || !w || !q)))
        return fail(c, UF3_EINVAL, "uf3_leverage: bad argument (group is 1 or 3 and divides n_rows, ld >= n_feat >= 1)");
    if (n_rows == 0) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the rows in stage_out2, [w | q] in stage_out, each with the 64 bytes of slack behind it that the block has always had
    Stage I(c->stage_out2, c->stream), O(c->stage_out, c->stream);
    const int s_x = I.add(8 * (size_t)n_rows * ld);
    I.add(64);
    const int s_w = O.add(8 * (size_t)n_feat * n_feat), s_q = O.add(8 * (size_t)(n_rows / group));
    O.add(64);
    HIPCHK(c, I.alloc());
    HIPCHK(c, O.alloc());
    HIPCHK(c, I.in({{s_x, x}}));
    HIPCHK(c, O.in({{s_w, w}}));
    int rc = uf3_leverage_dev(c, I.at<double>(s_x), n_rows, n_feat, ld, O.at<double>(s_w), group, O.at<double>(s_q));
    if (rc) return rc;
    HIPCHK(c, O.out({{s_q, q}}));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ fit bookkeeping
extern "C" int uf3_fit_rows_dev(uf3_ctx *c, int32_t n_frames, int32_t n_feat, double *d_x_e, const double *d_counts,
                                const double *d_y_e, const double *d_y_f, int64_t n_y_f, const int64_t *d_frozen,
                                const double *d_c_frozen, int32_t n_frozen, double *d_moments) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_frames < 0 || n_feat < 1 || !d_x_e || !d_counts || !d_y_e || !d_moments || n_y_f < 0 || n_frozen < 0 ||
        (n_frozen && (!d_frozen || !d_c_frozen)))
        return fail(c, UF3_EINVAL, "uf3_fit_rows_dev: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t f_blocks = d_y_f ? (n_y_f + 4095) / 4096 : 0;
    if (n_frames + f_blocks == 0) return UF3_OK;
    hipLaunchKernelGGL(k_fit_rows, dim3((unsigned)(n_frames + f_blocks)), dim3(256), 0, c->stream, n_frames, n_feat, d_x_e, d_counts,
                       d_y_e, d_y_f, n_y_f, d_frozen, d_c_frozen, n_frozen, d_moments);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_fit_pack_dev(uf3_ctx *c, int32_t n_feat, const double *d_flat, const int64_t *d_keep, int32_t n_keep,
                                const int64_t *d_frozen, const double *d_c_frozen, int32_t n_frozen, double n_energy_rows,
                                double n_force_rows, double *d_packed) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_feat < 1 || n_keep < 0 || n_keep > n_feat || !d_flat || (n_keep && !d_keep) || !d_packed || n_frozen < 0 ||
        (n_frozen && (!d_frozen || !d_c_frozen)))
        return fail(c, UF3_EINVAL, "uf3_fit_pack_dev: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    // (n_keep == 0, every column frozen: the six moments are the whole packed buffer)
    hipLaunchKernelGGL(k_fit_pack, dim3((unsigned)std::max(n_keep, 1), 2), dim3(256), 0, c->stream, n_feat, d_flat, d_keep, n_keep, d_frozen,
                       d_c_frozen, n_frozen, n_energy_rows, n_force_rows, d_packed);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

// ------------------------------------------------------------------------------ pair-distance histograms
// The reference's DataAnalyzer.get_distances + update_histograms (uf3/data/analyze.py) and summarize_distances
// (uf3/representation/distances.py:367-442): cdist of the frame against its explicit supercell, masked, np.histogram per pair.
// Here the cell list of prepare() enumerates the same (centre, image) pairs and k_pair_hist counts them into the bins.
#define UF3_HIST_LDS_BYTES 65536     // LDS counters of one workgroup: [P][n_bins] int32 up to this size, global atomics beyond

static int pair_hist_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, int32_t n_bins,
                          const double *edges, int upper_incl, const double *noise, int64_t n_noise, int per_frame,
                          int64_t *d_out) {
    uf3_ctx *c = b->ctx;
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || !fr->cells || !fr->pbc) return fail(c, UF3_EINVAL, "bad uf3_frames");
    if (n_bins < 1) return fail(c, UF3_EINVAL, "uf3_pair_histogram: n_bins must be >= 1");
    if (!edges) return fail(c, UF3_EINVAL, "uf3_pair_histogram: null edges");
    if (!(edges[0] >= 0.0)) return fail(c, UF3_EINVAL, "uf3_pair_histogram: edges must start at >= 0");
    for (int k = 0; k < n_bins; k++)
        if (!(edges[k + 1] > edges[k])) return fail(c, UF3_EINVAL, "uf3_pair_histogram: edges must be strictly increasing");
    if (n_noise < 0 || (n_noise > 0 && !noise)) return fail(c, UF3_EINVAL, "uf3_pair_histogram: bad noise array");
    const int nf = fr->n_frames, P = b->host.P;
    // rows of the noise table the frames reach: the reference supercell of every frame (geometry.py:14-51)
    int64_t need = 0;
    for (int f = 0; f < nf; f++) {
        const int64_t n = fr->atom_offsets[f + 1] - fr->atom_offsets[f];
        int fac[3] = {0, 0, 0};
        const uint8_t *pbc = fr->pbc + 3 * (size_t)f;
        if (pbc[0] || pbc[1] || pbc[2]) reference_factors(fr->cells + 9 * (size_t)f, b->r_cut, fac);
        int64_t cnt = 1;
        for (int k = 0; k < 3; k++) cnt *= pbc[k] ? 2 * (int64_t)fac[k] + 1 : 1;
        need = std::max(need, cnt * n);
    }
    double extra = 1e-9 * b->host.rsearch;          // (pairs at exactly r_max with the upper bound inclusive)
    if (noise) {
        if (n_noise < need) return fail(c, UF3_EINVAL, "uf3_pair_histogram: noise array shorter than a frame's supercell");
        double m2 = 0;
        for (int64_t q = 0; q < need; q++) m2 = std::max(m2, dot3(noise + 3 * q, noise + 3 * q));
        extra += std::sqrt(m2) * (1.0 + 1e-12);     // a rattled image moves at most this far towards a centre
    }
    Prepared P_;
    int rc = prepare(b, fr, d_pos, d_z, false, P_, false, 0, -1, extra);
    if (rc) return rc;
    hipStream_t st = c->stream;
    HIPCHK(c, c->hist_edges.ensure(8 * ((size_t)n_bins + 1)));
    HIPCHK(c, hipMemcpyAsync(c->hist_edges.p, edges, 8 * ((size_t)n_bins + 1), hipMemcpyHostToDevice, st));
    if (noise) {
        HIPCHK(c, c->hist_noise.ensure(24 * (size_t)need));
        HIPCHK(c, hipMemcpyAsync(c->hist_noise.p, noise, 24 * (size_t)need, hipMemcpyHostToDevice, st));
    }
    const size_t nh = (size_t)P * n_bins, n_out = (per_frame ? (size_t)nf : 1) * nh;
    HIPCHK(c, hipMemsetAsync(d_out, 0, 8 * n_out, st));
    double rmax = 0;
    for (int p = 0; p < P; p++) rmax = std::max(rmax, b->host.pairs[p].rmax);
    HistArgs a;
    a.edges = c->hist_edges.as<double>();
    a.noise = noise ? c->hist_noise.as<double>() : nullptr;
    a.out = (unsigned long long *)d_out;
    a.offsets = P_.d_offsets;
    a.natoms = P_.natoms; a.n_bins = n_bins; a.per_frame = per_frame ? 1 : 0; a.upper_incl = upper_incl ? 1 : 0;
    a.s_cut = rmax * rmax * (1.0 + 1e-12);
    // runs of consecutive atoms per workgroup: about four workgroups per CU, 4 .. 256 atoms
    int chunk = (int)((P_.natoms + 4LL * c->n_cu - 1) / (4LL * c->n_cu));
    chunk = std::max(4, std::min(256, (chunk + 3) / 4 * 4));
    a.chunk = chunk;
    const unsigned grid = (unsigned)((P_.natoms + chunk - 1) / chunk);
    const size_t lds = 4 * nh;
    Timed tm(c, T_NBR);
    if (lds <= (size_t)std::min(c->lds_max, UF3_HIST_LDS_BYTES))
        hipLaunchKernelGGL(k_pair_hist<true>, dim3(grid), dim3(256), lds, st, b->dev, P_.geoms, P_.frame_of, P_.cl, d_pos, P_.spec, a);
    else
        hipLaunchKernelGGL(k_pair_hist<false>, dim3(grid), dim3(256), 0, st, b->dev, P_.geoms, P_.frame_of, P_.cl, d_pos, P_.spec, a);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_pair_histogram_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, int32_t n_bins,
                                      const double *edges, int upper_inclusive, const double *noise, int64_t n_noise,
                                      int per_frame, int64_t *d_out) {
    uf3_env_refresh();
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!d_pos || !d_z || !d_out) return fail(c, UF3_EINVAL, "uf3_pair_histogram_dev: null device array");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = pair_hist_impl(b, fr, d_pos, d_z, n_bins, edges, upper_inclusive, noise, n_noise, per_frame, d_out);
    if (rc) return rc;
    // (species outside the basis are not reported here -- nothing waits --: the status word is cleared for the calls that follow)
    if (c->flags.p) HIPCHK(c, hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream));
    return UF3_OK;
}

extern "C" int uf3_pair_histogram(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, int32_t n_bins,
                                  const double *edges, int upper_inclusive, const double *noise, int64_t n_noise, int per_frame,
                                  int64_t *out) {
    uf3_env_refresh();
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!out) return fail(c, UF3_EINVAL, "uf3_pair_histogram: null out");
    if (!fr || fr->n_frames < 1) return fail(c, UF3_EINVAL, "bad uf3_frames");
    if (n_bins < 1) return fail(c, UF3_EINVAL, "uf3_pair_histogram: n_bins must be >= 1");
    int natoms = 0;
    int rc = upload_frames(c, fr, pos, z, natoms);
    if (rc) return rc;
    const size_t n_out = (per_frame ? (size_t)fr->n_frames : 1) * (size_t)b->host.P * (size_t)n_bins;
    // (the output behind positions | species would move with the staging block: a buffer of its own)
    HIPCHK(c, c->dbg.ensure(8 * n_out));
    rc = pair_hist_impl(b, fr, (const double *)c->stage_cur, c->d_stage_z, n_bins, edges, upper_inclusive, noise, n_noise,
                        per_frame, c->dbg.as<int64_t>());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->dbg.p, 8 * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pin_in_busy = false;
    return check_flags(c);
}

// ------------------------------------------------------------------------------ cut-off / regulariser scans
// k_scan_assemble (one wave per system row, every system of the batch in one grid) then k_scan_solve (one workgroup per
// system): systems of different sizes share both launches, each paying for its own rows only.
extern "C" int uf3_scan_solve_dev(uf3_ctx *c, int32_t n_cols, int32_t n_folds, const double *d_slots, const int32_t *d_cols,
                                  const int64_t *d_col_off, const int32_t *d_reg_rc, const double *d_reg_v,
                                  const int64_t *d_reg_off, int32_t n_sys, int64_t total_rows, const int64_t *d_sys,
                                  const double *d_sys_w, double *d_ws, int64_t ws_len, double *d_x, int64_t x_len,
                                  double *d_sse, int32_t *d_status) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_cols < 1 || n_folds < 1 || n_folds > UF3_SCAN_MAX_FOLDS || n_sys < 0 || total_rows < 0 || ws_len < 0 || x_len < 0)
        return fail(c, UF3_EINVAL, "uf3_scan_solve_dev: bad sizes (1 <= n_folds <= 32)");
    if (n_sys == 0) return UF3_OK;
    if (!d_slots || !d_cols || !d_col_off || !d_reg_off || !d_sys || !d_sys_w || !d_ws || !d_x || !d_sse || !d_status)
        return fail(c, UF3_EINVAL, "uf3_scan_solve_dev: null device array");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_frag(c);
    if (rc) return rc;
    ScanArgs a;
    a.n = n_cols; a.n_folds = n_folds; a.n_sys = n_sys;
    a.total_rows = total_rows; a.ws_len = ws_len; a.x_len = x_len;
    a.slots = d_slots; a.cols = d_cols; a.col_off = d_col_off; a.reg_rc = d_reg_rc; a.reg_v = d_reg_v; a.reg_off = d_reg_off;
    a.sys = d_sys; a.w = d_sys_w; a.frag = c->frag.as<int>();
    a.ws = d_ws; a.x = d_x; a.sse = d_sse; a.status = d_status;
    HIPCHK(c, hipMemsetAsync(d_status, 0, sizeof(int32_t) * (size_t)n_sys, c->stream));
    if (total_rows > 0) {
        hipLaunchKernelGGL(k_scan_assemble, dim3((unsigned)((total_rows + 3) / 4)), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(k_scan_solve, dim3((unsigned)n_sys), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

// ------------------------------------------------------------------------------ neighbour debug
static int neighbors_impl(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z,
                          int64_t *pair_count, int64_t *pair_ij, double *pair_geo, int64_t pair_cap, int64_t *n3_count,
                          int64_t *n3_ij, int64_t n3_cap) {
    uf3_env_refresh();
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!fr || fr->n_frames != 1) return fail(c, UF3_EINVAL, "the neighbour queries take exactly one frame");
    int natoms = 0;
    int rc = upload_frames(c, fr, pos, z, natoms);
    if (rc) return rc;
    Prepared P;
    rc = prepare(b, fr, (const double *)c->stage_cur, c->d_stage_z, false, P);
    if (rc) return rc;
    int np = b->host.P;
    std::vector<long long> counts(np + 2, 0);
    std::vector<long long> tuples;
    std::vector<double> geo;
    long long cap = 0;
    for (int pass = 0; pass < 2; pass++) {
        const size_t head = 8 * (size_t)(np + 2), ncap = (size_t)std::max<long long>(1, cap);
        HIPCHK(c, c->dbg.ensure(head + 24 * ncap + (pair_geo ? 32 * ncap : 0)));
        long long *d_counts = c->dbg.as<long long>(), *d_tuples = d_counts + np + 2;
        double *d_geo = pair_geo ? (double *)(d_tuples + 3 * ncap) : nullptr;
        HIPCHK(c, hipMemsetAsync(d_counts, 0, head, c->stream));
        hipLaunchKernelGGL(k_debug_pairs, dim3(natoms), dim3(64), 0, c->stream, b->dev, P.geoms, P.frame_of, P.cl,
                           (const double *)c->stage_cur, P.spec, natoms, d_counts, d_tuples, cap, d_geo);
        HIPCHK(c, hipMemcpyAsync(counts.data(), d_counts, head, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (pass == 0) { cap = counts[np + 1]; if (cap == 0) break; continue; }
        tuples.resize(3 * (size_t)cap);
        HIPCHK(c, hipMemcpy(tuples.data(), d_tuples, 24 * (size_t)cap, hipMemcpyDeviceToHost));
        if (pair_geo) {
            geo.resize(4 * (size_t)cap);
            HIPCHK(c, hipMemcpy(geo.data(), d_geo, 32 * (size_t)cap, hipMemcpyDeviceToHost));
        }
    }
    rc = check_flags(c);
    if (rc) return rc;
    if (pair_count) for (int p = 0; p < np; p++) pair_count[p] = counts[p];
    if (n3_count) *n3_count = counts[np];
    struct T3 { long long p, i, j, at; };
    std::vector<T3> v((size_t)cap);
    for (long long q = 0; q < cap; q++) v[q] = {tuples[3 * q], tuples[3 * q + 1], tuples[3 * q + 2], q};
    std::sort(v.begin(), v.end(), [](const T3 &a, const T3 &bb) {
        return a.p != bb.p ? a.p < bb.p : (a.i != bb.i ? a.i < bb.i : a.j < bb.j);
    });
    std::vector<long long> cur(np + 1, 0);
    for (const T3 &t : v) {
        if (t.p < np) {
            if (cur[t.p] < pair_cap) {
                const long long o = t.p * pair_cap + cur[t.p];
                if (pair_ij) { pair_ij[2 * o] = t.i; pair_ij[2 * o + 1] = t.j; }
                if (pair_geo) for (int k = 0; k < 4; k++) pair_geo[4 * o + k] = geo[4 * (size_t)t.at + k];
            }
        } else if (n3_ij && cur[np] < n3_cap) { n3_ij[2 * cur[np]] = t.i; n3_ij[2 * cur[np] + 1] = t.j; }
        cur[t.p]++;
    }
    return UF3_OK;
}

// The 3-body neighbour lists the LAST featurizer / evaluator call on this context built and consumed (MODE 0's build_n3_list or
// k_build_n3 -- not the separate walk of k_debug_pairs): per atom the entry count and, per entry, the neighbour's reference
// supercell index (image_rank * N + atom) in list order (species, then supercell index).  Test infrastructure: valid only straight
// after a synchronised call, before anything else runs on the context.
extern "C" int uf3_n3_lists_debug(uf3_basis *b, int64_t natoms, int64_t *cap_out, int32_t *counts, int32_t *sidx, int64_t sidx_cap) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->n3_last_cap <= 0 || natoms != c->n3_last_natoms || !c->n3_cnt.p || !c->n3_dbl.p)
        return fail(c, UF3_EINVAL, "uf3_n3_lists_debug: no 3-body lists of a batch of this size in the workspace");
    const int cap = c->n3_last_cap;
    if (cap_out) *cap_out = cap;
    if (counts) HIPCHK(c, hipMemcpy(counts, c->n3_cnt.p, sizeof(int) * (size_t)natoms, hipMemcpyDeviceToHost));
    if (sidx) {
        if (sidx_cap < cap) return fail(c, UF3_EINVAL, "uf3_n3_lists_debug: sidx_cap below the list capacity");
        std::vector<N3Entry> ent((size_t)natoms * cap);
        HIPCHK(c, hipMemcpy(ent.data(), c->n3_dbl.p, sizeof(N3Entry) * ent.size(), hipMemcpyDeviceToHost));
        for (int64_t a = 0; a < natoms; a++)
            for (int q = 0; q < cap; q++) sidx[a * sidx_cap + q] = ent[(size_t)a * cap + q].sidx;
    }
    return UF3_OK;
}

extern "C" int uf3_neighbors_debug(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z,
                                   int64_t *pair_count, int64_t *pair_ij, int64_t pair_cap, int64_t *n3_count,
                                   int64_t *n3_ij, int64_t n3_cap) {
    return neighbors_impl(b, fr, pos, z, pair_count, pair_ij, nullptr, pair_cap, n3_count, n3_ij, n3_cap);
}

extern "C" int uf3_pair_geometry(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z,
                                 int64_t *pair_count, int64_t *pair_ij, double *pair_geo, int64_t pair_cap) {
    if (pair_cap > 0 && !pair_geo) return fail(b ? b->ctx : nullptr, UF3_EINVAL, "uf3_pair_geometry: null pair_geo");
    return neighbors_impl(b, fr, pos, z, pair_count, pair_ij, pair_cap > 0 ? pair_geo : nullptr, pair_cap, nullptr, nullptr, 0);
}

// ------------------------------------------------------------------------------ dense helpers (small frames)
extern "C" int uf3_distance_matrix(uf3_ctx *c, const double *a, int64_t na, const double *bb, int64_t nb, double *out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (na < 0 || nb < 0 || (na && !a) || (nb && !bb)) return fail(c, UF3_EINVAL, "uf3_distance_matrix: bad argument");
    const size_t n = (size_t)na * (size_t)nb;
    if (!n) return UF3_OK;
    if (!out) return fail(c, UF3_EINVAL, "uf3_distance_matrix: null out");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->dbg.ensure(24 * (size_t)(na + nb) + 8 * n));
    double *d_a = c->dbg.as<double>(), *d_b = d_a + 3 * na, *d_out = d_b + 3 * nb;
    HIPCHK(c, hipMemcpyAsync(d_a, a, 24 * (size_t)na, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_b, bb, 24 * (size_t)nb, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_distance_matrix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_a, (long long)na, d_b,
                       (long long)nb, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

extern "C" int uf3_direction_cosines(uf3_ctx *c, const double *sup_pos, int64_t n_sup, const int64_t *i_where,
                                     const int64_t *j_where, const double *rij, int64_t n_d, int64_t n_atoms, double *out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n_sup < 0 || n_d < 0 || n_atoms < 0) return fail(c, UF3_EINVAL, "uf3_direction_cosines: bad argument");
    const size_t n = (size_t)n_atoms * 3 * (size_t)n_d;
    if (!n) return UF3_OK;
    if (!sup_pos || !i_where || !j_where || !rij || !out) return fail(c, UF3_EINVAL, "uf3_direction_cosines: null argument");
    for (int64_t q = 0; q < n_d; q++)
        if (i_where[q] < 0 || i_where[q] >= n_sup || j_where[q] < 0 || j_where[q] >= n_sup)
            return fail(c, UF3_EINVAL, "uf3_direction_cosines: index outside the supercell");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->dbg.ensure(24 * (size_t)n_sup + 24 * (size_t)n_d + 8 * n));
    double *d_pos = c->dbg.as<double>();
    long long *d_i = (long long *)(d_pos + 3 * n_sup), *d_j = d_i + n_d;
    double *d_r = (double *)(d_j + n_d), *d_out = d_r + n_d;
    HIPCHK(c, hipMemcpyAsync(d_pos, sup_pos, 24 * (size_t)n_sup, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_i, i_where, 8 * (size_t)n_d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_j, j_where, 8 * (size_t)n_d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_r, rij, 8 * (size_t)n_d, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_direction_cosines, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_pos, d_i, d_j, d_r,
                       (long long)n_d, (long long)n_atoms, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ what the library-owned drivers share
// (uf3_md, uf3_relax, uf3_neb and uf3_mc below: a batch with its model and its buffers, stepped between calls of eval_impl)
struct Batch {
    uf3_basis *b = nullptr;
    uf3_ctx *c = nullptr;
    int32_t n_frames = 0;
    int64_t natoms = 0;
    std::vector<int64_t> offsets;
    std::vector<double> cells;                  // the current cells (host: what eval_impl reads)
    std::vector<uint8_t> pbc;
    uf3_frames fr{};
    std::vector<double> c1, c2, c3;             // the model (host copies: eval_impl takes host coefficients)
    DevBuf pos, z, energies, offsets_dev;
};

static bool md_finite(const double *a, size_t n) {
    for (size_t i = 0; i < n; i++) if (!std::isfinite(a[i])) return false;
    return true;
}

// what every *_create checks of its batch; *n: the atoms of the batch
// (b null: a batch without a model -- uf3_idpp_create -- on context c)
static int batch_check(uf3_ctx *c, uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                       const double *c2, const double *c3, const void *out, const std::string &who, int64_t *n) {
    if (!out) return fail(c, UF3_EINVAL, who + ": out is NULL");
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || !fr->cells || !fr->pbc) return fail(c, UF3_EINVAL, who + ": bad uf3_frames");
    if (!pos) return fail(c, UF3_EINVAL, who + ": pos is NULL");
    if (!z) return fail(c, UF3_EINVAL, who + ": z is NULL");
    if (b && (!c1 || (b->c2_len && !c2) || (b->c3_len && !c3))) return fail(c, UF3_EINVAL, who + ": missing coefficients (c1 / c2 / c3)");
    const int nf = fr->n_frames;
    if (fr->atom_offsets[0] != 0) return fail(c, UF3_EINVAL, who + ": atom_offsets[0] must be 0");
    for (int f = 0; f < nf; f++)
        if (fr->atom_offsets[f + 1] <= fr->atom_offsets[f]) return fail(c, UF3_EINVAL, who + ": every frame needs an atom");
    *n = fr->atom_offsets[nf];
    if (*n >= (1LL << 28)) return fail(c, UF3_EINVAL, who + ": batch must hold 1 .. 2^28 atoms");
    if (!md_finite(pos, 3 * (size_t)*n)) return fail(c, UF3_EINVAL, who + ": pos must be finite");
    if (!md_finite(fr->cells, 9 * (size_t)nf)) return fail(c, UF3_EINVAL, who + ": cells must be finite");
    return UF3_OK;
}

static int batch_check(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1, const double *c2,
                       const double *c3, const void *out, const std::string &who, int64_t *n) {
    if (!b) return fail(nullptr, UF3_EINVAL, who + ": basis is NULL");
    return batch_check(b->ctx, b, fr, pos, z, c1, c2, c3, out, who, n);
}

// the host copies of a checked batch (c2 / c3 followed by coeff_pad zeros), the four common buffers and their uploads, queued on
// the stream: the caller's own uploads follow, then one wait.  pos == nullptr: the caller uploads the positions itself
// (b null: no model is kept, c is the context)
static int batch_init(Batch &B, uf3_ctx *c, uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                      const double *c2, const double *c3, size_t coeff_pad, const std::string &who) {
    const int nf = fr->n_frames;
    const size_t n = (size_t)fr->atom_offsets[nf];
    B.b = b; B.c = c; B.n_frames = nf; B.natoms = (int64_t)n;
    B.offsets.assign(fr->atom_offsets, fr->atom_offsets + nf + 1);
    B.cells.assign(fr->cells, fr->cells + 9 * (size_t)nf);
    B.pbc.assign(fr->pbc, fr->pbc + 3 * (size_t)nf);
    B.fr.n_frames = nf; B.fr.atom_offsets = B.offsets.data(); B.fr.cells = B.cells.data(); B.fr.pbc = B.pbc.data();
    if (b) {
        B.c1.assign(c1, c1 + b->host.S);
        B.c2.assign(c2 ? c2 : c1, (c2 ? c2 : c1) + b->c2_len); B.c2.resize(b->c2_len + coeff_pad, 0.0);
        B.c3.assign(c3 ? c3 : c1, (c3 ? c3 : c1) + b->c3_len); B.c3.resize(b->c3_len + coeff_pad, 0.0);
    }
    if (B.pos.ensure(24 * n) || B.z.ensure(4 * n) || B.energies.ensure(8 * (size_t)nf) || B.offsets_dev.ensure(8 * (size_t)(nf + 1)))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    hipStream_t s = c->stream;
    if ((pos && hipMemcpyAsync(B.pos.p, pos, 24 * n, hipMemcpyHostToDevice, s)) || hipMemcpyAsync(B.z.p, z, 4 * n, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(B.offsets_dev.p, B.offsets.data(), 8 * (size_t)(nf + 1), hipMemcpyHostToDevice, s))
        return fail(c, UF3_EHIP, who + ": upload failed");
    return UF3_OK;
}

static int batch_init(Batch &B, uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                      const double *c2, const double *c3, size_t coeff_pad, const std::string &who) {
    return batch_init(B, b->ctx, b, fr, pos, z, c1, c2, c3, coeff_pad, who);
}

// the evaluator on the batch's positions: energies, and forces / strain derivatives where asked for
static int batch_eval(Batch &B, double *forces, double *virials) {
    return eval_impl(B.b, &B.fr, B.pos.as<double>(), B.z.as<int32_t>(), B.c1.data(), B.c2.data(), B.c3.data(), B.energies.as<double>(),
                     forces, virials);
}

// chunks of <= width atoms from each frame's first atom (a chunk never straddles frames): the workgroups of the drivers'
// partial kernels, and each frame's chunks for the kernel that sums them
struct ChunkTable {
    DevBuf blk_frame, blk_lo, blk_n;            // [n_blocks]: the chunk's frame, its first atom, its atoms
    DevBuf frame_blk, frame_of;                 // [n_frames + 1]: the frame's chunks; [N]: the atom's frame
    int n_blocks = 0;
};

static int chunk_table_build(uf3_ctx *c, const std::vector<int64_t> &offsets, int n_frames, int width, ChunkTable &T,
                             const std::string &who) {
    const size_t n = (size_t)offsets[n_frames];
    std::vector<int> blk_frame, blk_n, frame_blk(1, 0), frame_of(n);
    std::vector<long long> blk_lo;
    for (int f = 0; f < n_frames; f++) {
        for (int64_t lo = offsets[f]; lo < offsets[f + 1]; lo += width) {
            blk_frame.push_back(f);
            blk_lo.push_back(lo);
            blk_n.push_back((int)std::min<int64_t>(width, offsets[f + 1] - lo));
        }
        frame_blk.push_back((int)blk_frame.size());
        for (int64_t i = offsets[f]; i < offsets[f + 1]; i++) frame_of[i] = f;
    }
    const size_t nb = blk_frame.size();
    if (T.blk_frame.ensure(4 * nb) || T.blk_lo.ensure(8 * nb) || T.blk_n.ensure(4 * nb) || T.frame_blk.ensure(4 * (size_t)(n_frames + 1)) ||
        T.frame_of.ensure(4 * n))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(T.blk_frame.p, blk_frame.data(), 4 * nb, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(T.blk_lo.p, blk_lo.data(), 8 * nb, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(T.blk_n.p, blk_n.data(), 4 * nb, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(T.frame_blk.p, frame_blk.data(), 4 * (size_t)(n_frames + 1), hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(T.frame_of.p, frame_of.data(), 4 * n, hipMemcpyHostToDevice, s) || hipStreamSynchronize(s))
        return fail(c, UF3_EHIP, who + ": upload failed");      // (waited for: the host vectors go out of scope)
    T.n_blocks = (int)nb;
    return UF3_OK;
}

// uf3_*_destroy: waits for the driver's queued work, then frees it (its DevBufs with it)
template <class Driver> static void driver_destroy(Driver *d) {
    if (!d) return;
    hipSetDevice(d->c->device);
    hipStreamSynchronize(d->c->stream);
    delete d;
}

// the run's skin for its own duration, the caller's back on every way out (a change of skin drops the lists: each run starts
// with one list build); the run's error message outlives the restore
template <class Run> static int with_run_skin(uf3_ctx *c, double skin, Run run) {
    const double caller_skin = c->md.skin;
    int rc = uf3_ctx_md_skin(c, skin);
    if (rc) return rc;
    rc = run();
    const std::string msg = c->err;
    const int rs = uf3_ctx_md_skin(c, caller_skin);
    return rc ? fail(c, rc, msg) : rs;
}

// ------------------------------------------------------------------------------ molecular dynamics (uf3_md_*, uf3_md.h)
// A library-owned state: positions (unwrapped), velocities, forces, inverse masses and species in HBM, stepped by k_md_step
// between calls of the evaluator (eval_impl, unchanged).  Between two launches the velocities are at integer time t and the
// forces are F(t): a launch closes step t with a half-kick and opens step t + 1 (half-kick, drift; BAOAB's A-O-A with friction).
struct uf3_md : Batch {
    DevBuf vel, frc, inv_m, virials, kin, ring;
    int64_t step = 0;                           // absolute step counter (feeds the random numbers)
    bool forces_valid = false;                  // frc / energies describe pos
    // constant-pressure runs (uf3_md_run_npt, uf3_npt.h): chunk table, pistons, the current cells on the device
    ChunkTable chunks;
    DevBuf npt_st, npt_coef, npt_partial, cells_dev;
    bool npt_ready = false;
    bool virials_valid = false;                 // virials describe pos and cells (with forces_valid)
    bool g_valid = false;                       // the pistons' g_close belongs to the current state
    // heat-current samples (uf3_md_run_flux, uf3_flux.h): the masses as given, the lists' workspace, the records of a run
    DevBuf mass, flux_ring;
    // grade samples (uf3_md_run_grade, uf3_site_rows.h): the atoms' grades of one sample, the records of a run
    DevBuf grade, grade_ring;
    // periodic wrapping (uf3_md_set_wrap, k_md_wrap): off, img is zero and no run reads it.  On, the object's position is
    // pos + img . cell with the current cell; cells_now() is that cell on the device
    bool wrap = false;
    bool chunks_ready = false;                  // `chunks` is built (npt_init, md_wrap_buffers, the MSD sampler)
    DevBuf img, wrap_cells, wrap_pbc, wrap_flag, unwrapped;
    // mean-squared-displacement samples (uf3_md_run_msd): species of every atom (host: from uf3_md_create), the origin
    std::vector<signed char> spec;
    DevBuf msd_spec, msd_origin, msd_partial, msd_ring;
    bool msd_origin_set = false;
    // switching runs (uf3_md_set_reference, uf3_md_run_switch, uf3_ti.h): reference sites and springs, the chunks' partial sums,
    // the frames' scratch (lambda, U_E, D, W, the projections' vectors), the run's per-frame parameters and its schedule
    DevBuf ti_x0, ti_spring, ti_partial, ti_frame, ti_par, ti_sched;
    bool ti_ready = false;
    ListWork fx;
    ~uf3_md() { fx.release(); }
    const double *cells_now() const { return npt_ready ? cells_dev.as<double>() : wrap_cells.as<double>(); }
};

extern "C" void uf3_md_destroy(uf3_md *md) { driver_destroy(md); }

static int md_chunks(uf3_md *md, const std::string &who) {
    if (md->chunks_ready) return UF3_OK;
    int rc = chunk_table_build(md->c, md->offsets, md->n_frames, UF3_NPT_THREADS, md->chunks, who);
    md->chunks_ready = rc == UF3_OK;
    return rc;
}

// what the wrap kernels read besides pos: image counts (zero when first made), the frames' cells and boundary flags, the chunk
// table's frame of every atom.  Outside a constant-pressure object the cells never change: one upload
static int md_wrap_buffers(uf3_md *md, const std::string &who) {
    uf3_ctx *c = md->c;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = md_chunks(md, who);
    if (rc) return rc;
    if (md->img.p) return UF3_OK;
    const size_t nf = (size_t)md->n_frames;
    if (md->wrap_cells.ensure(72 * nf) || md->wrap_pbc.ensure(3 * nf) || md->wrap_flag.ensure(4) || md->img.ensure(12 * (size_t)md->natoms))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(md->wrap_cells.p, md->cells.data(), 72 * nf, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(md->wrap_pbc.p, md->pbc.data(), 3 * nf, hipMemcpyHostToDevice, s) ||
        hipMemsetAsync(md->img.p, 0, 12 * (size_t)md->natoms, s) || hipStreamSynchronize(s)) {
        md->img.release();
        return fail(c, UF3_EHIP, who + ": upload failed");
    }
    return UF3_OK;
}

static MdWrapArgs md_wrap_args(uf3_md *md, int *changed) {
    MdWrapArgs A;
    A.pos = md->pos.as<double>(); A.img = md->img.as<int>(); A.cells = md->cells_now();
    A.pbc = md->wrap_pbc.as<unsigned char>(); A.frame_of = md->chunks.frame_of.as<int>(); A.n = md->natoms; A.changed = changed;
    return A;
}

// the hook of uf3_ctx::MdState::wrap: queued in front of the list build (or the evaluation) that called it
static int md_wrap_launch(uf3_md *md, const double *d_pos, int *changed = nullptr) {
    uf3_ctx *c = md->c;
    if (d_pos != md->pos.as<double>()) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_md_wrap, dim3((unsigned)((md->natoms + 255) / 256)), dim3(256), 0, c->stream, md_wrap_args(md, changed));
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

// pos + img . cell into `out` (fold: into pos itself, img zeroed); *moved: some atom had a nonzero image count
static int md_unwrap(uf3_md *md, double *out, bool fold, bool *moved) {
    uf3_ctx *c = md->c;
    int *flag = moved ? md->wrap_flag.as<int>() : nullptr;
    if (flag) HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));
    hipLaunchKernelGGL(k_md_unwrap, dim3((unsigned)((md->natoms + 255) / 256)), dim3(256), 0, c->stream, md_wrap_args(md, flag), out,
                       fold ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    if (flag) {
        int h = 0;
        HIPCHK(c, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *moved = h != 0;
    }
    return UF3_OK;
}

// positions changed under the evaluator's feet: its lists and everything evaluated go
static void md_positions_changed(uf3_md *md) {
    md->c->md.valid = false;
    md->forces_valid = false; md->virials_valid = false; md->g_valid = false;
}

extern "C" int uf3_md_set_wrap(uf3_md *md, int on) {
    if (!md) return fail(nullptr, UF3_EINVAL, "uf3_md_set_wrap: null md");
    uf3_ctx *c = md->c;
    if ((on != 0) == md->wrap) return UF3_OK;
    if (on) {
        int rc = md_wrap_buffers(md, "uf3_md_set_wrap");
        if (rc) return rc;
        int *flag = md->wrap_flag.as<int>(), h = 0;
        HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));
        rc = md_wrap_launch(md, md->pos.as<double>(), flag);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        md->wrap = true;
        if (h) md_positions_changed(md);
        return UF3_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    bool moved = false;
    int rc = md_unwrap(md, md->pos.as<double>(), true, &moved);
    if (rc) return rc;
    md->wrap = false;
    if (moved) md_positions_changed(md);
    return UF3_OK;
}

extern "C" int uf3_md_get_wrapped(uf3_md *md, double *pos, int32_t *images) {
    if (!md) return fail(nullptr, UF3_EINVAL, "uf3_md_get_wrapped: null md");
    uf3_ctx *c = md->c;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = 3 * (size_t)md->natoms;
    if (pos) HIPCHK(c, hipMemcpyAsync(pos, md->pos.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (images) {
        if (md->img.p) HIPCHK(c, hipMemcpyAsync(images, md->img.p, 4 * n3, hipMemcpyDeviceToHost, c->stream));
        else memset(images, 0, 4 * n3);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

static int md_upload(uf3_md *md, const double *pos, const double *vel) {
    uf3_ctx *c = md->c;
    const size_t n3 = 3 * (size_t)md->natoms;
    if (pos && !md_finite(pos, n3)) return fail(c, UF3_EINVAL, "uf3_md: positions must be finite");
    if (vel && !md_finite(vel, n3)) return fail(c, UF3_EINVAL, "uf3_md: velocities must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    if (pos) HIPCHK(c, hipMemcpyAsync(md->pos.p, pos, 8 * n3, hipMemcpyHostToDevice, c->stream));
    if (pos && md->img.p) HIPCHK(c, hipMemsetAsync(md->img.p, 0, 4 * n3, c->stream));      // (positions are taken as given)
    if (vel) HIPCHK(c, hipMemcpyAsync(md->vel.p, vel, 8 * n3, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (pos) md->forces_valid = false;
    md->g_valid = false;
    return UF3_OK;
}

extern "C" int uf3_md_create(uf3_basis *b, const uf3_frames *fr, const double *pos, const double *vel, const int32_t *z,
                             const double *masses, const double *c1, const double *c2, const double *c3, uf3_md **out) {
    const char *who = "uf3_md_create";
    int64_t n = 0;
    int rc = batch_check(b, fr, pos, z, c1, c2, c3, out, who, &n);
    if (rc) return rc;
    uf3_ctx *c = b->ctx;
    if (!masses) return fail(c, UF3_EINVAL, "uf3_md_create: null argument");
    std::vector<double> inv(n);
    for (int64_t i = 0; i < n; i++) {
        if (!(masses[i] > 0.0) || !std::isfinite(masses[i])) return fail(c, UF3_EINVAL, "uf3_md_create: masses must be positive and finite");
        inv[i] = 1.0 / masses[i];
    }
    HIPCHK(c, hipSetDevice(c->device));
    uf3_md *md = new uf3_md();
    md->spec.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) md->spec[i] = z[i] >= 0 && z[i] < 120 ? b->host.z2s[z[i]] : (signed char)-1;
    auto bail = [&](int rc) { uf3_md_destroy(md); return rc; };
    rc = batch_init(*md, b, fr, pos, z, c1, c2, c3, 1, who);
    if (rc) return bail(rc);
    const size_t n3 = 3 * (size_t)n;
    if (md->vel.ensure(8 * n3) || md->frc.ensure(8 * n3) || md->inv_m.ensure(8 * (size_t)n) || md->virials.ensure(48 * (size_t)md->n_frames) ||
        md->mass.ensure(8 * (size_t)n))
        return bail(fail(c, UF3_ENOMEM, "uf3_md_create: out of device memory"));
    if (hipMemcpyAsync(md->inv_m.p, inv.data(), 8 * (size_t)n, hipMemcpyHostToDevice, c->stream) ||
        hipMemcpyAsync(md->mass.p, masses, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream) ||
        hipMemsetAsync(md->vel.p, 0, 8 * n3, c->stream))
        return bail(fail(c, UF3_EHIP, "uf3_md_create: upload failed"));
    rc = md_upload(md, nullptr, vel);           // (waits for the uploads above)
    if (rc) return bail(rc);
    *out = md;
    return UF3_OK;
}

extern "C" int uf3_md_set_state(uf3_md *md, const double *pos, const double *vel) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    if (pos && md->wrap) md->c->md.valid = false;           // (as given, possibly outside the cell: the next evaluation builds, and wraps)
    return md_upload(md, pos, vel);
}

// F(t) and the per-frame energies (and strain derivatives) of the current positions
static int md_forces(uf3_md *md, bool virial) {
    if (md->wrap) md->c->md.wrap = [md](const double *d_pos) { return md_wrap_launch(md, d_pos); };
    int rc = batch_eval(*md, md->frc.as<double>(), virial ? md->virials.as<double>() : nullptr);
    if (md->wrap) md->c->md.wrap = nullptr;
    md->forces_valid = rc == UF3_OK;
    md->virials_valid = md->forces_valid && virial;
    return rc;
}

extern "C" int uf3_md_get_state(uf3_md *md, double *pos, double *vel, double *forces, double *energies) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    HIPCHK(c, hipSetDevice(c->device));
    if ((forces || energies) && !md->forces_valid) {        // (positions set since the last evaluation: evaluate them now)
        int rc = md_forces(md, false);
        if (rc) return rc;
    }
    const size_t n3 = 3 * (size_t)md->natoms;
    const void *d_pos = md->pos.p;
    if (pos && md->wrap) {                                  // (unwrapped, as always: pos + img . cell, formed on the device)
        HIPCHK(c, md->unwrapped.ensure(8 * n3));
        int rc = md_unwrap(md, md->unwrapped.as<double>(), false, nullptr);
        if (rc) return rc;
        d_pos = md->unwrapped.p;
    }
    if (pos) HIPCHK(c, hipMemcpyAsync(pos, d_pos, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (vel) HIPCHK(c, hipMemcpyAsync(vel, md->vel.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (forces) HIPCHK(c, hipMemcpyAsync(forces, md->frc.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (energies) HIPCHK(c, hipMemcpyAsync(energies, md->energies.p, 8 * (size_t)md->n_frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

extern "C" int uf3_md_init_velocities(uf3_md *md, double temperature_K, uint64_t seed, int exact_temperature) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    if (!(temperature_K >= 0.0) || !std::isfinite(temperature_K)) return fail(c, UF3_EINVAL, "uf3_md_init_velocities: temperature must be finite and >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_md_init_velocities, dim3((unsigned)((md->natoms + 255) / 256)), dim3(256), 0, c->stream, md->vel.as<double>(),
                       (const double *)md->inv_m.as<double>(), (long long)md->natoms, UF3_MD_KB * temperature_K, (unsigned long long)seed,
                       (unsigned long long)md->step);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_md_init_com, dim3((unsigned)md->n_frames), dim3(UF3_MD_THREADS), 0, c->stream, md->vel.as<double>(),
                       (const double *)md->inv_m.as<double>(), (const int64_t *)md->offsets_dev.as<int64_t>(), UF3_MD_KB * temperature_K,
                       exact_temperature ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    md->g_valid = false;
    return UF3_OK;
}

// ---- the run loop of uf3_md_run, uf3_md_run_flux, uf3_md_run_grade and uf3_md_run_npt ----------------------
// what a run asks of each of its record buffers (thermo, flux, grade): given exactly when records are due
static int md_records_check(uf3_ctx *c, const std::string &who, const char *what, const char *buffer, int64_t due, const void *given) {
    if ((due > 0) == (given != nullptr)) return UF3_OK;
    return fail(c, UF3_EINVAL, due > 0 ? who + ": " + what + " records are due but the " + buffer + " buffer is NULL"
                                       : who + ": a " + buffer + " buffer was given but no record is due");
}

struct NptBaro { double p0, tau, gamma_p, Tp; };        // pressure, barostat time and friction, piston temperature

// what the four entries (who) ask of a run's arguments, in the order of uf3_md_run_npt's parameter list: the barostat's four sit
// in the middle of it, so their tests do too (baro null: a constant-volume run has none)
static int md_run_check(uf3_ctx *c, const std::string &who, int64_t n_steps, double dt, double T, double gamma, const NptBaro *baro,
                        int64_t every, double skin, const double *thermo) {
    if (n_steps < 0) return fail(c, UF3_EINVAL, who + ": n_steps must be >= 0");
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail(c, UF3_EINVAL, who + ": dt must be positive and finite");
    if (!(T >= 0.0) || !std::isfinite(T)) return fail(c, UF3_EINVAL, who + ": temperature must be finite and >= 0");
    if (!(gamma >= 0.0) || !std::isfinite(gamma)) return fail(c, UF3_EINVAL, who + ": friction must be finite and >= 0");
    if (baro) {
        if (!std::isfinite(baro->p0)) return fail(c, UF3_EINVAL, who + ": pressure must be finite");
        if (!(baro->tau > 0.0) || !std::isfinite(baro->tau)) return fail(c, UF3_EINVAL, who + ": barostat time must be positive and finite");
        if (!(baro->gamma_p >= 0.0) || !std::isfinite(baro->gamma_p)) return fail(c, UF3_EINVAL, who + ": barostat friction must be finite and >= 0");
        if (!(baro->Tp > 0.0) || !std::isfinite(baro->Tp)) return fail(c, UF3_EINVAL, who + ": piston temperature must be positive and finite");
    }
    if (every < 0) return fail(c, UF3_EINVAL, who + ": thermo_every must be >= 0");
    if (!(skin >= 0.0) || skin > 4.0) return fail(c, UF3_EINVAL, who + ": skin must lie in [0, 4] Angstrom");
    return md_records_check(c, who, "thermo", "thermo", every ? n_steps / every : 0, thermo);
}

// A run without samples (uf3_md_run, uf3_md_run_npt), and what a sampler is: a period, and what the loop calls
struct MdSampler {
    int64_t every = 0;                          // a sample of the closed state after every every-th step (0: none)
    int64_t *steps_done = nullptr;              // where the number of completed steps goes (uf3_md_run_grade)
    int prepare() { return UF3_OK; }            // the ring of the run's records, the lists' workspace
    int sample(int64_t, bool &) { return UF3_OK; }      // record s (0-based); true in `stop` when it ends the run
    int copy_out() { return UF3_OK; }           // queues the records' way to the caller
};

// The loop every run is.  E, the ensemble: prepare(n_rec) (its buffers, and F(t) of the state the run starts from), launch(close,
// open, step, record) (what lies between two force calls, + the frame sums of thermo record `record` >= 0), forces(k) (the
// evaluator for step k), moved() (the validity flags an opening launch drops) and copy_out() (what else the caller gets back).
// S, the sampler (above): the launch that closes a sampled step does not open the next one, and the sample sits between the
// two launches.  That is the split a run boundary makes anyway: the trajectory's bits do not change.  A sample that stops the run
// ends it there: the state is the closed one the sample saw, the thermo records due so far are copied out.
template <class Ensemble, class Sampler>
static int md_steps(uf3_md *md, int64_t n_steps, int64_t every, int width, double *thermo, Ensemble &E, Sampler &S) {
    uf3_ctx *c = md->c;
    const int64_t n_rec = every ? n_steps / every : 0, t0 = md->step;
    int rc = S.prepare();
    if (rc) return rc;
    if (n_rec) HIPCHK(c, md->ring.ensure(8 * (size_t)n_rec * md->n_frames * width));
    rc = E.prepare(n_rec);
    if (rc) return rc;
    // after `done` steps of the run: the thermo record its close fills (-1: none), whether a sample is due, and the run's end
    auto record = [&](int64_t done) { return done && every && done % every == 0 ? done / every - 1 : -1; };
    auto sampled = [&](int64_t done) { return done && S.every && done % S.every == 0; };
    auto finish = [&](int64_t done) {
        const int64_t due = every ? done / every : 0;
        int rc = S.copy_out();
        if (rc) return rc;
        if (due) HIPCHK(c, hipMemcpyAsync(thermo, md->ring.p, 8 * (size_t)due * md->n_frames * width, hipMemcpyDeviceToHost, c->stream));
        rc = E.copy_out();
        if (rc) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return (int)UF3_OK;
    };
    for (int64_t k = 1; k <= n_steps; k++) {
        // closes step k - 1 of the run (its record, if due) and opens step k
        const int64_t step = t0 + k - 1;
        if (sampled(k - 1)) {
            rc = E.launch(1, 0, step, record(k - 1));
            // step k - 1 is closed and nothing has moved since its forces: a closed state, whatever happens below -- an error
            // leaves the state of a run that ended here, which a later run goes on from
            md->step = step;
            if (rc) return rc;
            if (S.steps_done) *S.steps_done = k - 1;
            bool stop = false;
            rc = S.sample((k - 1) / S.every - 1, stop);
            if (rc) return rc;
            if (stop) return finish(k - 1);
            rc = E.launch(0, 1, step, -1);
        } else
            rc = E.launch(k > 1, 1, step, record(k - 1));
        E.moved();
        md->step = step;
        if (rc) return rc;
        rc = E.forces(k);
        if (rc) return rc;
    }
    // the closing half of the last step
    rc = E.launch(1, 0, t0 + n_steps - 1, record(n_steps));
    if (rc) return rc;
    md->step = t0 + n_steps;
    if (S.steps_done) *S.steps_done = n_steps;
    if (sampled(n_steps)) {
        bool stop;
        rc = S.sample(n_steps / S.every - 1, stop);
        if (rc) return rc;
    }
    return finish(n_steps);
}

// NVE / Langevin: one k_md_step launch between two force calls
struct MdVerlet {
    uf3_md *md; MdStepArgs A; bool langevin, stress; int64_t every; int width;
    MdVerlet(uf3_md *md, double dt, double T, double gamma, uint64_t seed, int64_t every, bool stress)
        : md(md), langevin(gamma > 0.0), stress(stress), every(every), width(stress ? 14 : 2) {
        A.pos = md->pos.as<double>(); A.vel = md->vel.as<double>(); A.frc = md->frc.as<double>(); A.inv_m = md->inv_m.as<double>();
        A.n = md->natoms; A.dt = dt;
        A.c = std::exp(-gamma * dt); A.kT = UF3_MD_KB * T; A.seed = (unsigned long long)seed;
    }
    int prepare(int64_t n_rec) {
        if (n_rec) HIPCHK(md->c, md->kin.ensure(56 * (size_t)md->natoms));
        A.kin = md->kin.as<double>();
        return md->forces_valid ? (int)UF3_OK : md_forces(md, false);
    }
    int launch(int close, int open, int64_t step, int64_t record) {
        uf3_ctx *c = md->c;
        A.step = (unsigned long long)step; A.close = close; A.open = open;
        const dim3 g((unsigned)((md->natoms + 255) / 256)), blk(256);
        with_bool(langevin, [&](auto L) { return with_bool(record >= 0, [&](auto T) {
            hipLaunchKernelGGL((k_md_step<L, T>), g, blk, 0, c->stream, A);
            return (int)UF3_OK; }); });
        HIPCHK(c, hipGetLastError());
        if (record >= 0) {
            hipLaunchKernelGGL(k_md_thermo, dim3((unsigned)md->n_frames), dim3(UF3_MD_THREADS), 0, c->stream, (const double *)md->kin.as<double>(),
                               (long long)md->natoms, (const int64_t *)md->offsets_dev.as<int64_t>(), (const double *)md->energies.as<double>(),
                               (const double *)md->virials.as<double>(), md->ring.as<double>() + (size_t)record * md->n_frames * width, width);
            HIPCHK(c, hipGetLastError());
        }
        return UF3_OK;
    }
    int forces(int64_t k) { return md_forces(md, stress && every && k % every == 0); }
    void moved() { md->forces_valid = false; }
    int copy_out() { return UF3_OK; }
};

static int lists_prepare(uf3_basis *b, const uf3_frames *fr, ListWork &W, const int32_t *d_z, const double *c1, const double *c2,
                         const double *c3, const char *who, const char *what, FluxArgs &F, bool model = true);
static int flux_sample(uf3_ctx *c, ListWork &W, FluxArgs &F, bool headroom, const char *who);
static int site_grade_sample(uf3_basis *b, ListWork &W, FluxArgs &F, bool headroom, const char *who, const double *d_w,
                             double *d_grade, const int64_t *d_offsets, int n_out, double *d_fmax, int32_t *d_fargmax,
                             double *d_pair, const std::function<int()> &after);

// uf3_md_run_flux: one heat-current record [n_frames][6] per sample (velocities at integer time, the positions the forces belong
// to), copied out at the end of the run
struct MdFluxSampler : MdSampler {
    uf3_md *md; int64_t n_flux; double *out; FluxArgs F;
    MdFluxSampler(uf3_md *md, int64_t n_steps, int64_t flux_every, double *flux)
        : md(md), n_flux(flux_every ? n_steps / flux_every : 0), out(flux) { every = flux_every; }
    int prepare() {
        if (!n_flux) return UF3_OK;
        HIPCHK(md->c, md->flux_ring.ensure(48 * (size_t)n_flux * md->n_frames));
        int rc = lists_prepare(md->b, &md->fr, md->fx, md->z.as<int32_t>(), md->c1.data(), md->c2.data(), md->c3.data(), "uf3_md_run_flux", "batch", F);
        F.pos = md->pos.as<double>(); F.vel = md->vel.as<double>(); F.mass = md->mass.as<double>(); F.w = nullptr;
        return rc;
    }
    int sample(int64_t s, bool &) {
        F.flux = md->flux_ring.as<double>() + (size_t)s * md->n_frames * 6;
        return flux_sample(md->c, md->fx, F, true, "uf3_md_run_flux");
    }
    int copy_out() {
        uf3_ctx *c = md->c;
        if (n_flux) HIPCHK(c, hipMemcpyAsync(out, md->flux_ring.p, 48 * (size_t)n_flux * md->n_frames, hipMemcpyDeviceToHost, c->stream));
        return UF3_OK;
    }
};

// uf3_md_run_grade: W on the device, the stop threshold (<= 0: none) and the caller's records [n_samples][n_frames][2].  A
// sample's record is in the caller's array when sample() returns (the copy is queued in front of the sample's own synchronisation)
struct MdGradeSampler : MdSampler {
    uf3_md *md; int64_t n_grade; const double *d_w; double stop_above, *out; FluxArgs F;
    MdGradeSampler(uf3_md *md, int64_t n_steps, const double *d_w, int64_t grade_every, double grade_stop, double *grades, int64_t *done)
        : md(md), n_grade(grade_every ? n_steps / grade_every : 0), d_w(d_w), stop_above(grade_stop), out(grades) {
        every = grade_every; steps_done = done;
    }
    int prepare() {
        if (!n_grade) return UF3_OK;
        HIPCHK(md->c, md->grade.ensure(8 * (size_t)md->natoms));
        HIPCHK(md->c, md->grade_ring.ensure(16 * (size_t)n_grade * md->n_frames));
        int rc = lists_prepare(md->b, &md->fr, md->fx, md->z.as<int32_t>(), nullptr, nullptr, nullptr, "uf3_md_run_grade", "batch", F, false);
        F.pos = md->pos.as<double>();
        return rc;
    }
    int sample(int64_t s, bool &stop) {
        uf3_ctx *c = md->c;
        const size_t rec = 2 * (size_t)md->n_frames;
        double *d_rec = md->grade_ring.as<double>() + (size_t)s * rec, *h_rec = out + (size_t)s * rec;
        int rc = site_grade_sample(md->b, md->fx, F, true, "uf3_md_run_grade", d_w, md->grade.as<double>(),
                                   md->offsets_dev.as<int64_t>(), md->n_frames, nullptr, nullptr, d_rec, [&] {
            HIPCHK(c, hipMemcpyAsync(h_rec, d_rec, 8 * rec, hipMemcpyDeviceToHost, c->stream));
            return (int)UF3_OK;
        });
        if (rc) return rc;
        stop = false;
        if (stop_above > 0.0)
            for (int f = 0; f < md->n_frames; f++) stop = stop || h_rec[2 * (size_t)f] > stop_above;
        return UF3_OK;
    }
};

// what the three constant-volume entries share, behind the checks of their own sampler
template <class Sampler>
static int md_run_entry(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                        double skin, int64_t thermo_every, int with_stress, double *thermo, Sampler &&S, const char *who = "uf3_md_run") {
    uf3_ctx *c = md->c;
    int rc = md_run_check(c, who, n_steps, dt_fs, temperature_K, friction_per_fs, nullptr, thermo_every, skin, thermo);
    if (rc) return rc;
    if (n_steps == 0) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return with_run_skin(c, skin, [&] {
        MdVerlet E(md, dt_fs, temperature_K, friction_per_fs, seed, thermo_every, with_stress != 0);
        return md_steps(md, n_steps, thermo_every, E.width, thermo, E, S);
    });
}

extern "C" int uf3_md_run(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                          double skin, int64_t thermo_every, int with_stress, double *thermo) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    return md_run_entry(md, n_steps, dt_fs, temperature_K, friction_per_fs, seed, skin, thermo_every, with_stress, thermo, MdSampler());
}

extern "C" int uf3_md_run_flux(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                               double skin, int64_t thermo_every, int with_stress, double *thermo, int64_t flux_every, double *flux) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    if (flux_every < 0) return fail(c, UF3_EINVAL, "uf3_md_run_flux: flux_every must be >= 0");
    int rc = md_records_check(c, "uf3_md_run_flux", "flux", "flux", flux_every ? n_steps / flux_every : 0, flux);
    if (rc) return rc;
    return md_run_entry(md, n_steps, dt_fs, temperature_K, friction_per_fs, seed, skin, thermo_every, with_stress, thermo,
                        MdFluxSampler(md, n_steps, flux_every, flux));
}

extern "C" int uf3_md_run_grade(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                                double skin, int64_t thermo_every, int with_stress, double *thermo, const double *d_w,
                                int64_t grade_every, double grade_stop, double *grades, int64_t *steps_done) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    if (!steps_done) return fail(c, UF3_EINVAL, "uf3_md_run_grade: null argument (steps_done)");
    *steps_done = 0;
    if (grade_every < 0) return fail(c, UF3_EINVAL, "uf3_md_run_grade: grade_every must be >= 0");
    if (std::isnan(grade_stop)) return fail(c, UF3_EINVAL, "uf3_md_run_grade: grade_stop is not a number");
    const int64_t n_grade = grade_every && n_steps > 0 ? n_steps / grade_every : 0;
    int rc = md_records_check(c, "uf3_md_run_grade", "grade", "grades", n_grade, grades);
    if (rc) return rc;
    if (n_grade && !d_w) return fail(c, UF3_EINVAL, "uf3_md_run_grade: null argument (w)");
    return md_run_entry(md, n_steps, dt_fs, temperature_K, friction_per_fs, seed, skin, thermo_every, with_stress, thermo,
                        MdGradeSampler(md, n_steps, d_w, grade_every, grade_stop, grades, steps_done));
}

// uf3_md_run_msd: one record [n_frames][4 S + 4] per sample (k_md_msd_partial, k_md_msd_frame: uf3_md.h) of the closed state,
// copied out at the end of the run.  The sample only reads: the trajectory and the thermo records do not depend on it
static int md_msd_origin(uf3_md *md, const double *origin, const std::string &who) {
    uf3_ctx *c = md->c;
    const size_t n3 = 3 * (size_t)md->natoms;
    HIPCHK(c, hipSetDevice(c->device));
    if (origin && !md_finite(origin, n3)) return fail(c, UF3_EINVAL, who + ": origin must be finite");
    if (md->msd_origin.ensure(8 * n3)) return fail(c, UF3_ENOMEM, who + ": out of device memory");
    if (origin) HIPCHK(c, hipMemcpyAsync(md->msd_origin.p, origin, 8 * n3, hipMemcpyHostToDevice, c->stream));
    else if (md->wrap) {
        int rc = md_unwrap(md, md->msd_origin.as<double>(), false, nullptr);
        if (rc) return rc;
    } else
        HIPCHK(c, hipMemcpyAsync(md->msd_origin.p, md->pos.p, 8 * n3, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    md->msd_origin_set = true;
    return UF3_OK;
}

extern "C" int uf3_md_msd_origin(uf3_md *md, const double *origin) {
    if (!md) return fail(nullptr, UF3_EINVAL, "uf3_md_msd_origin: null md");
    return md_msd_origin(md, origin, "uf3_md_msd_origin");
}

struct MdMsdSampler : MdSampler {
    uf3_md *md; int64_t n_msd; double *out; MdMsdArgs A; int width;
    MdMsdSampler(uf3_md *md, int64_t n_steps, int64_t msd_every, double *msd)
        : md(md), n_msd(msd_every ? n_steps / msd_every : 0), out(msd), width(4 * md->b->host.S + 4) { every = msd_every; }
    int prepare() {
        if (!n_msd) return UF3_OK;
        uf3_ctx *c = md->c;
        const char *who = "uf3_md_run_msd";
        int rc = md_chunks(md, who);
        if (rc) return rc;
        if (!md->msd_origin_set) { rc = md_msd_origin(md, nullptr, who); if (rc) return rc; }    // (no origin yet: where the run starts)
        if (!md->msd_spec.p) {
            if (md->msd_spec.ensure((size_t)md->natoms)) return fail(c, UF3_ENOMEM, "uf3_md_run_msd: out of device memory");
            HIPCHK(c, hipMemcpyAsync(md->msd_spec.p, md->spec.data(), (size_t)md->natoms, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        if (md->msd_partial.ensure(8 * (size_t)md->chunks.n_blocks * width) || md->msd_ring.ensure(8 * (size_t)n_msd * md->n_frames * width))
            return fail(c, UF3_ENOMEM, "uf3_md_run_msd: out of device memory");
        const ChunkTable &ct = md->chunks;
        A.pos = md->pos.as<double>(); A.origin = md->msd_origin.as<double>(); A.mass = md->mass.as<double>();
        A.img = md->wrap ? md->img.as<int>() : nullptr; A.cells = md->wrap ? md->cells_now() : nullptr;
        A.spec = md->msd_spec.as<signed char>(); A.frame_of = ct.frame_of.as<int>(); A.blk_n = ct.blk_n.as<int>();
        A.frame_blk = ct.frame_blk.as<int>(); A.blk_lo = ct.blk_lo.as<long long>();
        A.partial = md->msd_partial.as<double>(); A.rec = nullptr; A.S = md->b->host.S;
        return UF3_OK;
    }
    int sample(int64_t s, bool &) {
        uf3_ctx *c = md->c;
        A.rec = md->msd_ring.as<double>() + (size_t)s * md->n_frames * width;
        hipLaunchKernelGGL(k_md_msd_partial, dim3((unsigned)md->chunks.n_blocks), dim3(UF3_MD_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_md_msd_frame, dim3((unsigned)md->n_frames), dim3(64), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        return UF3_OK;
    }
    int copy_out() {
        uf3_ctx *c = md->c;
        if (n_msd) HIPCHK(c, hipMemcpyAsync(out, md->msd_ring.p, 8 * (size_t)n_msd * md->n_frames * width, hipMemcpyDeviceToHost, c->stream));
        return UF3_OK;
    }
};

extern "C" int uf3_md_run_msd(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                              double skin, int64_t thermo_every, int with_stress, double *thermo, int64_t msd_every, double *msd) {
    if (!md) return fail(nullptr, UF3_EINVAL, "uf3_md_run_msd: null md");
    uf3_ctx *c = md->c;
    if (msd_every < 0) return fail(c, UF3_EINVAL, "uf3_md_run_msd: msd_every must be >= 0");
    int rc = md_records_check(c, "uf3_md_run_msd", "msd", "msd", msd_every && n_steps > 0 ? n_steps / msd_every : 0, msd);
    if (rc) return rc;
    return md_run_entry(md, n_steps, dt_fs, temperature_K, friction_per_fs, seed, skin, thermo_every, with_stress, thermo,
                        MdMsdSampler(md, n_steps, msd_every, msd), "uf3_md_run_msd");
}

// ------------------------------------------------------------------------------ switching runs (uf3_md_run_switch, uf3_ti.h)
// The same state and the same loop (md_steps); the ensemble's force is the model's mixed with an Einstein crystal's, and after
// every force call k_ti_partial / k_ti_frame close the state: lambda, U_E, the work, the projections of the step opened next.
static int ti_refused(uf3_md *md, const std::string &who) {
    uf3_ctx *c = md->c;
    if (md->wrap)
        return fail(c, UF3_EINVAL, who + ": the object wraps its positions (a spring needs the unwrapped displacement from its site, and "
                                         "a solid does not diffuse): turn wrap off");
    if (md->npt_ready) return fail(c, UF3_EINVAL, who + ": the object runs at a pressure: a switch is made at constant volume");
    return UF3_OK;
}

extern "C" int uf3_md_set_reference(uf3_md *md, const double *ref_pos, const double *spring) {
    const std::string who = "uf3_md_set_reference";
    if (!md) return fail(nullptr, UF3_EINVAL, who + ": null md");
    uf3_ctx *c = md->c;
    int rc = ti_refused(md, who);
    if (rc) return rc;
    const size_t n = (size_t)md->natoms;
    if (ref_pos && !md_finite(ref_pos, 3 * n)) return fail(c, UF3_EINVAL, who + ": ref_pos must be finite");
    if (spring)
        for (size_t i = 0; i < n; i++)
            if (!(spring[i] >= 0.0) || !std::isfinite(spring[i])) return fail(c, UF3_EINVAL, who + ": spring must be finite and >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    rc = md_chunks(md, who);
    if (rc) return rc;
    const size_t nf = (size_t)md->n_frames;
    md->ti_ready = false;
    if (md->ti_x0.ensure(24 * n) || md->ti_spring.ensure(8 * n) || md->ti_partial.ensure(8 * (size_t)md->chunks.n_blocks * UF3_TI_PART) ||
        md->ti_frame.ensure(8 * 10 * nf) || md->ti_par.ensure(8 * 3 * nf))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(md->ti_x0.p, ref_pos ? (const void *)ref_pos : md->pos.p, 24 * n, ref_pos ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    if (spring) HIPCHK(c, hipMemcpyAsync(md->ti_spring.p, spring, 8 * n, hipMemcpyHostToDevice, s));
    else HIPCHK(c, hipMemsetAsync(md->ti_spring.p, 0, 8 * n, s));
    HIPCHK(c, hipStreamSynchronize(s));
    md->ti_ready = true;
    return UF3_OK;
}

// the switching ensemble: MdVerlet's five members with k_ti_step in k_md_step's place and the frame kernels behind every force call
struct MdSwitch {
    uf3_md *md; TiArgs A; bool langevin; int64_t n_steps, t0; double *work;
    MdSwitch(uf3_md *md, int64_t n_steps, double dt, double gamma, uint64_t seed, int fix_com, double *work)
        : md(md), langevin(gamma > 0.0), n_steps(n_steps), t0(md->step), work(work) {
        const ChunkTable &ct = md->chunks;
        const size_t nf = (size_t)md->n_frames;
        A.pos = md->pos.as<double>(); A.vel = md->vel.as<double>(); A.frc = md->frc.as<double>(); A.inv_m = md->inv_m.as<double>();
        A.mass = md->mass.as<double>(); A.kin = nullptr; A.x0 = md->ti_x0.as<double>(); A.spring = md->ti_spring.as<double>();
        A.frame_of = ct.frame_of.as<int>(); A.blk_n = ct.blk_n.as<int>(); A.frame_blk = ct.frame_blk.as<int>();
        A.blk_lo = ct.blk_lo.as<long long>(); A.energies = md->energies.as<double>();
        A.kT = md->ti_par.as<double>(); A.lam_a = A.kT + nf; A.lam_b = A.kT + 2 * nf; A.sched = md->ti_sched.as<double>();
        A.partial = md->ti_partial.as<double>();
        A.lam = md->ti_frame.as<double>(); A.ue = A.lam + nf; A.d = A.lam + 2 * nf; A.w = A.lam + 3 * nf; A.cf = A.lam + 4 * nf; A.cn = A.lam + 7 * nf;
        A.n = md->natoms; A.dt = dt; A.c = std::exp(-gamma * dt); A.seed = (unsigned long long)seed; A.step = 0; A.j = 0;
        A.fix_com = fix_com ? 1 : 0; A.noise = 0; A.close = A.open = 0;
    }
    // closes state j of the run (the positions the forces belong to)
    int frame(int64_t j) {
        uf3_ctx *c = md->c;
        A.j = j; A.step = (unsigned long long)(t0 + j); A.noise = langevin && A.fix_com && j < n_steps;
        hipLaunchKernelGGL(k_ti_partial, dim3((unsigned)md->chunks.n_blocks), dim3(UF3_MD_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_ti_frame, dim3((unsigned)md->n_frames), dim3(64), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        return UF3_OK;
    }
    int prepare(int64_t n_rec) {
        if (n_rec) HIPCHK(md->c, md->kin.ensure(56 * (size_t)md->natoms));
        A.kin = md->kin.as<double>();
        if (!md->forces_valid) { int rc = md_forces(md, false); if (rc) return rc; }
        return frame(0);
    }
    int launch(int close, int open, int64_t step, int64_t record) {
        uf3_ctx *c = md->c;
        A.step = (unsigned long long)step; A.close = close; A.open = open;
        const dim3 g((unsigned)((md->natoms + 255) / 256)), blk(256);
        with_bool(langevin, [&](auto L) { return with_bool(record >= 0, [&](auto T) {
            hipLaunchKernelGGL((k_ti_step<L, T>), g, blk, 0, c->stream, A);
            return (int)UF3_OK; }); });
        HIPCHK(c, hipGetLastError());
        if (record >= 0) {
            hipLaunchKernelGGL(k_ti_record, dim3((unsigned)md->n_frames), dim3(UF3_MD_THREADS), 0, c->stream, A,
                               (const int64_t *)md->offsets_dev.as<int64_t>(), md->ring.as<double>() + (size_t)record * md->n_frames * UF3_TI_REC);
            HIPCHK(c, hipGetLastError());
        }
        return UF3_OK;
    }
    int forces(int64_t k) {
        int rc = md_forces(md, false);
        return rc ? rc : frame(k);
    }
    void moved() { md->forces_valid = false; }
    int copy_out() {
        HIPCHK(md->c, hipMemcpyAsync(work, A.w, 8 * (size_t)md->n_frames, hipMemcpyDeviceToHost, md->c->stream));
        return UF3_OK;
    }
};

extern "C" int uf3_md_run_switch(uf3_md *md, int64_t n_steps, double dt_fs, const double *temperatures_K, double friction_per_fs,
                                 uint64_t seed, double skin, const double *lambda_a, const double *lambda_b, const double *schedule,
                                 int fix_com, int64_t every, double *records, double *work) {
    const std::string who = "uf3_md_run_switch";
    if (!md) return fail(nullptr, UF3_EINVAL, who + ": null md");
    uf3_ctx *c = md->c;
    int rc = ti_refused(md, who);
    if (rc) return rc;
    if (!md->ti_ready) return fail(c, UF3_EINVAL, who + ": no reference: call uf3_md_set_reference first");
    const size_t nf = (size_t)md->n_frames;
    if (n_steps < 0) return fail(c, UF3_EINVAL, who + ": n_steps must be >= 0");
    if (!(dt_fs > 0.0) || !std::isfinite(dt_fs)) return fail(c, UF3_EINVAL, who + ": dt must be positive and finite");
    if (!temperatures_K) return fail(c, UF3_EINVAL, who + ": null argument (temperatures_K)");
    for (size_t f = 0; f < nf; f++)
        if (!(temperatures_K[f] >= 0.0) || !std::isfinite(temperatures_K[f])) return fail(c, UF3_EINVAL, who + ": temperatures must be finite and >= 0");
    if (!(friction_per_fs >= 0.0) || !std::isfinite(friction_per_fs)) return fail(c, UF3_EINVAL, who + ": friction must be finite and >= 0");
    if (!(skin >= 0.0) || skin > 4.0) return fail(c, UF3_EINVAL, who + ": skin must lie in [0, 4] Angstrom");
    if (!lambda_a || !lambda_b) return fail(c, UF3_EINVAL, who + ": null argument (lambda_a / lambda_b)");
    for (const double *lam : {lambda_a, lambda_b})
        for (size_t f = 0; f < nf; f++)
            if (!(lam[f] >= 0.0 && lam[f] <= 1.0)) return fail(c, UF3_EINVAL, who + ": lambda must be finite and lie in [0, 1]");
    if (!schedule) return fail(c, UF3_EINVAL, who + ": null argument (schedule)");
    for (int64_t j = 0; j <= n_steps; j++)
        if (!(schedule[j] >= 0.0 && schedule[j] <= 1.0)) return fail(c, UF3_EINVAL, who + ": schedule entries must be finite and lie in [0, 1]");
    if (every < 0) return fail(c, UF3_EINVAL, who + ": every must be >= 0");
    rc = md_records_check(c, who, "switch", "records", every ? n_steps / every : 0, records);
    if (rc) return rc;
    if (!work) return fail(c, UF3_EINVAL, who + ": null argument (work)");
    for (size_t f = 0; f < nf; f++) work[f] = 0.0;
    if (n_steps == 0) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> par(3 * nf);
    for (size_t f = 0; f < nf; f++) { par[f] = UF3_MD_KB * temperatures_K[f]; par[nf + f] = lambda_a[f]; par[2 * nf + f] = lambda_b[f]; }
    if (md->ti_sched.ensure(8 * (size_t)(n_steps + 1))) return fail(c, UF3_ENOMEM, who + ": out of device memory");
    HIPCHK(c, hipMemcpyAsync(md->ti_par.p, par.data(), 8 * 3 * nf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(md->ti_sched.p, schedule, 8 * (size_t)(n_steps + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (par goes out of scope)
    return with_run_skin(c, skin, [&] {
        MdSwitch E(md, n_steps, dt_fs, friction_per_fs, seed, fix_com, work);
        MdSampler none;
        return md_steps(md, n_steps, every, UF3_TI_REC, records, E, none);
    });
}

// ------------------------------------------------------------------------------ constant pressure (uf3_md_run_npt, uf3_npt.h)
// The same state as above plus one piston per frame.  Between two force calls: k_npt_partial, k_npt_frame, k_npt_move.  The
// cells change on every step and stay on the device: the evaluator runs on its persistent lists in the "cells live" mode of
// its MD state (eval_impl), and the host's copy is refreshed in front of a list build and at the end of the run.
static int npt_init(uf3_md *md) {
    if (md->npt_ready) return UF3_OK;
    uf3_ctx *c = md->c;
    const int nf = md->n_frames;
    std::vector<NptFrame> st(nf);
    for (int f = 0; f < nf; f++) {
        if (!(md->pbc[3 * f] && md->pbc[3 * f + 1] && md->pbc[3 * f + 2]))
            return fail(c, UF3_EINVAL, "uf3_md_run_npt: every frame must be periodic along all three axes");
        NptFrame &S = st[f];
        memset(&S, 0, sizeof(S));
        const double *cl = md->cells.data() + 9 * (size_t)f;
        double nrm[3][3];
        cross3(cl + 3, cl + 6, nrm[0]); cross3(cl + 6, cl, nrm[1]); cross3(cl, cl + 3, nrm[2]);
        const double vol = std::fabs(dot3(cl, nrm[0]));
        if (!(vol > 0.0) || !std::isfinite(vol)) return fail(c, UF3_EINVAL, "uf3_md_run_npt: a frame's cell is singular");
        S.s = S.s_closed = S.s_build = 1.0;
        for (int k = 0; k < 9; k++) S.cell0[k] = cl[k];
        S.vol0 = vol;
        for (int k = 0; k < 3; k++) S.hgt0[k] = vol / norm3(nrm[k]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = md_chunks(md, "uf3_md_run_npt");
    if (rc) return rc;
    if (md->npt_st.ensure(sizeof(NptFrame) * (size_t)nf) || md->npt_coef.ensure(sizeof(NptCoef) * (size_t)nf) ||
        md->npt_partial.ensure(24 * (size_t)md->chunks.n_blocks) || md->cells_dev.ensure(72 * (size_t)nf))
        return fail(c, UF3_ENOMEM, "uf3_md_run_npt: out of device memory");
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(md->npt_st.p, st.data(), sizeof(NptFrame) * (size_t)nf, hipMemcpyHostToDevice, s) ||
        hipMemsetAsync(md->npt_coef.p, 0, sizeof(NptCoef) * (size_t)nf, s) ||
        hipMemcpyAsync(md->cells_dev.p, md->cells.data(), 72 * (size_t)nf, hipMemcpyHostToDevice, s) || hipStreamSynchronize(s))
        return fail(c, UF3_EHIP, "uf3_md_run_npt: upload failed");
    md->npt_ready = true;
    return UF3_OK;
}

// NPH / NPT: three launches between two force calls, the cells on the device
struct MdPiston {
    uf3_md *md; NptArgs A;
    MdPiston(uf3_md *md, double dt, double T, double gamma, const NptBaro &B, uint64_t seed, double skin) : md(md) {
        memset(&A, 0, sizeof(A));
        A.pos = md->pos.as<double>(); A.vel = md->vel.as<double>(); A.frc = md->frc.as<double>(); A.inv_m = md->inv_m.as<double>();
        const ChunkTable &ct = md->chunks;
        A.frame_of = ct.frame_of.as<int>(); A.n = md->natoms;
        A.blk_frame = ct.blk_frame.as<int>(); A.blk_n = ct.blk_n.as<int>(); A.frame_blk = ct.frame_blk.as<int>();
        A.blk_lo = ct.blk_lo.as<long long>(); A.partial = md->npt_partial.as<double>();
        A.offsets = md->offsets_dev.as<long long>(); A.virials = md->virials.as<double>();
        A.st = md->npt_st.as<NptFrame>(); A.coef = md->npt_coef.as<NptCoef>(); A.cells = md->cells_dev.as<double>();
        A.dt = dt; A.p0 = B.p0; A.tau2_kTp = B.tau * B.tau * UF3_MD_KB * B.Tp; A.kT = UF3_MD_KB * T;
        A.c = std::exp(-gamma * dt); A.cp = std::exp(-B.gamma_p * dt);
        A.r_cut = md->b->host.rsearch; A.skin = skin;
        A.seed = (unsigned long long)seed;
        A.langevin = gamma > 0.0 || B.gamma_p > 0.0;
    }
    int prepare(int64_t) {
        uf3_ctx *c = md->c;
        HIPCHK(c, md->kin.ensure(56 * (size_t)md->natoms));
        if (!c->flags.p) { HIPCHK(c, c->flags.ensure(64)); HIPCHK(c, hipMemsetAsync(c->flags.p, 0, 64, c->stream)); }
        A.kin = md->kin.as<double>(); A.flags = c->flags.as<int>();
        if (md->forces_valid && md->virials_valid) return UF3_OK;
        md->g_valid = false;
        return forces(0);
    }
    // use_g: the opening half takes G from the last closing half (nothing changed since)
    int launch(int close, int open, int64_t step, int64_t record) {
        uf3_ctx *c = md->c;
        hipStream_t s = c->stream;
        A.step = (unsigned long long)step; A.close = close; A.open = open; A.use_g = open && md->g_valid;
        // the evaluator's persistent copies, while its lists are this run's
        const bool lists = c->md.live && c->md.valid && c->md.natoms == md->natoms && c->md.n_frames == md->n_frames;
        A.geo = lists ? c->md.geo.as<FrameGeom>() : nullptr;
        A.pos_ref = lists ? c->md.pos_ref.as<double>() : nullptr;
        A.thermo = record >= 0;
        hipLaunchKernelGGL(k_npt_partial, dim3((unsigned)md->chunks.n_blocks), dim3(UF3_NPT_THREADS), 0, s, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_npt_frame, dim3((unsigned)md->n_frames), dim3(UF3_NPT_THREADS), 0, s, A);
        HIPCHK(c, hipGetLastError());
        const dim3 g((unsigned)((md->natoms + UF3_NPT_THREADS - 1) / UF3_NPT_THREADS)), blk(UF3_NPT_THREADS);
        with_bool(A.langevin, [&](auto L) { return with_bool(A.thermo, [&](auto T) {
            hipLaunchKernelGGL((k_npt_move<L, T>), g, blk, 0, s, A);
            return (int)UF3_OK; }); });
        HIPCHK(c, hipGetLastError());
        if (A.thermo) {
            hipLaunchKernelGGL(k_npt_thermo, dim3((unsigned)md->n_frames), dim3(UF3_MD_THREADS), 0, s, A, (const double *)md->energies.as<double>(),
                               md->ring.as<double>() + (size_t)record * md->n_frames * UF3_NPT_REC);
            HIPCHK(c, hipGetLastError());
        }
        A.rebuilt = 0;
        if (!open) md->g_valid = true;           // (the pistons' g_close belongs to the closed state)
        return UF3_OK;
    }
    // forces, energies and strain derivatives of the current positions and cells; rebuilt: the evaluator built its lists on the way
    int forces(int64_t) {
        const long long before = md->c->md.builds;
        int rc = md_forces(md, true);
        if (md->c->md.builds != before) A.rebuilt = 1;
        return rc;
    }
    void moved() { md->forces_valid = false; md->virials_valid = false; md->g_valid = false; }
    int copy_out() {
        uf3_ctx *c = md->c;
        HIPCHK(c, hipMemcpyAsync(md->cells.data(), md->cells_dev.p, 72 * (size_t)md->n_frames, hipMemcpyDeviceToHost, c->stream));
        return UF3_OK;
    }
};

extern "C" int uf3_md_run_npt(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs,
                              double pressure_eV_A3, double barostat_time_fs, double barostat_friction_per_fs,
                              double piston_temperature_K, uint64_t seed, double skin, int64_t thermo_every, double *thermo) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    const NptBaro B = {pressure_eV_A3, barostat_time_fs, barostat_friction_per_fs, piston_temperature_K};
    int rc = md_run_check(c, "uf3_md_run_npt", n_steps, dt_fs, temperature_K, friction_per_fs, &B, thermo_every, skin, thermo);
    if (rc) return rc;
    rc = npt_init(md);
    if (rc) return rc;
    if (n_steps == 0) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // the run's skin and the "cells live" mode for its own duration; the caller's mode, then the caller's skin, back on every
    // way out.  Lists from before the run are dropped on the way in (their cells are not compared any more), the run's own on
    // the way out
    return with_run_skin(c, skin, [&] {
        const bool caller_live = c->md.live;
        const double *caller_dev = c->md.live_dev;
        double *caller_host = c->md.live_host;
        c->md.valid = false;
        c->md.live = true; c->md.live_dev = md->cells_dev.as<double>(); c->md.live_host = md->cells.data();
        MdPiston E(md, dt_fs, temperature_K, friction_per_fs, B, seed, skin);
        MdSampler none;
        const int rc = md_steps(md, n_steps, thermo_every, UF3_NPT_REC, thermo, E, none);
        if (rc) {
            // (the device's cells are the state: the host's copy follows them, whatever stopped the run)
            hipMemcpyAsync(md->cells.data(), md->cells_dev.p, 72 * (size_t)md->n_frames, hipMemcpyDeviceToHost, c->stream);
            hipStreamSynchronize(c->stream);
            md->forces_valid = false; md->virials_valid = false; md->g_valid = false;
        }
        c->md.valid = false;
        c->md.live = caller_live; c->md.live_dev = caller_dev; c->md.live_host = caller_host;
        return rc;
    });
}

extern "C" int uf3_md_get_cells(uf3_md *md, double *cells, double *scales, double *strain_rates) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    uf3_ctx *c = md->c;
    const int nf = md->n_frames;
    if (cells) memcpy(cells, md->cells.data(), 72 * (size_t)nf);
    if (scales || strain_rates) {
        std::vector<NptFrame> st(nf);
        if (md->npt_ready) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipMemcpyAsync(st.data(), md->npt_st.p, sizeof(NptFrame) * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        for (int f = 0; f < nf; f++) {
            if (scales) scales[f] = md->npt_ready ? st[f].s : 1.0;
            if (strain_rates) strain_rates[f] = md->npt_ready ? st[f].veps : 0.0;
        }
    }
    return UF3_OK;
}

extern "C" int uf3_ctx_md_live(uf3_ctx *c, int32_t *live) {
    if (!c || !live) return fail(c, UF3_EINVAL, "uf3_ctx_md_live: null argument");
    *live = c->md.live ? 1 : 0;
    return UF3_OK;
}

extern "C" int uf3_md_info(const uf3_md *md, int64_t *step, int64_t *n_atoms, int32_t *n_frames) {
    if (!md) return fail(nullptr, UF3_EINVAL, "null md");
    if (step) *step = md->step;
    if (n_atoms) *n_atoms = md->natoms;
    if (n_frames) *n_frames = md->n_frames;
    return UF3_OK;
}

extern "C" int uf3_philox_debug(uf3_ctx *c, int64_t n, const uint32_t *counters, const uint32_t *keys, uint32_t *out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "null ctx");
    if (n < 0 || n > (1LL << 26) || (n && (!counters || !keys || !out))) return fail(c, UF3_EINVAL, "uf3_philox_debug: bad argument");
    if (!n) return UF3_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->dbg.ensure(40 * (size_t)n));
    uint4 *d_ctr = c->dbg.as<uint4>(), *d_out = d_ctr + n;
    uint2 *d_key = (uint2 *)(d_out + n);
    HIPCHK(c, hipMemcpyAsync(d_ctr, counters, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_key, keys, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_philox_debug, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (long long)n, (const uint4 *)d_ctr,
                       (const uint2 *)d_key, d_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, d_out, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ structure relaxation (uf3_relax_*, uf3_relax.h)
// A library-owned FIRE state for a batch of frames: positions (unwrapped), velocities, forces, the per-frame optimiser state and,
// in cell runs, the scaled coordinates q (x = q D) in HBM.  Every step is one evaluator call (eval_impl, unchanged) and three
// launches; positions-only runs wait for the device only every check_every steps.  Cell runs copy the new cells back every step
// (the evaluator reads them from the host uf3_frames) and run on the rebuild route (skin 0: the MD route's key holds the cells).
struct uf3_relax : Batch {
    bool cell_run = false;                      // some frame has the cell as a degree of freedom
    bool has_fixed = false;
    std::vector<RelaxFrame> st_host;
    ChunkTable chunks;
    DevBuf q, vel, frc, fixed, virials, st, coef, partial, cells_dev, ring;
    bool forces_valid = false;                  // frc / energies (/ virials in a cell run) describe pos
};

extern "C" void uf3_relax_destroy(uf3_relax *r) { driver_destroy(r); }

static double det3(const double *m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// what uf3_relax_run and uf3_neb_run (who) ask of their arguments, in the order of the parameter list (climb sits in the middle
// of it, so its test does too: uf3_relax_run has none and passes 0)
static int fire_run_check(uf3_ctx *c, const std::string &who, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep,
                          double skin, int climb, int64_t check_every, int64_t record_every, const double *records) {
    if (max_steps < 0) return fail(c, UF3_EINVAL, who + ": max_steps must be >= 0");
    if (!(fmax > 0.0) || !std::isfinite(fmax)) return fail(c, UF3_EINVAL, who + ": fmax must be positive and finite");
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail(c, UF3_EINVAL, who + ": dt must be positive and finite");
    if (!(dt_max > 0.0) || !std::isfinite(dt_max)) return fail(c, UF3_EINVAL, who + ": dt_max must be positive and finite");
    if (!(maxstep > 0.0) || !std::isfinite(maxstep)) return fail(c, UF3_EINVAL, who + ": maxstep must be positive and finite");
    if (!(skin >= 0.0) || skin > 4.0) return fail(c, UF3_EINVAL, who + ": skin must lie in [0, 4] Angstrom");
    if (climb != 0 && climb != 1) return fail(c, UF3_EINVAL, who + ": climb must be 0 or 1");
    if (check_every < 1) return fail(c, UF3_EINVAL, who + ": check_every must be >= 1");
    if (record_every < 0) return fail(c, UF3_EINVAL, who + ": record_every must be >= 0");
    if ((record_every > 0) != (records != nullptr))
        return fail(c, UF3_EINVAL, who + (record_every ? ": records are due but the records buffer is NULL"
                                                       : ": a records buffer was given but no record is due"));
    return UF3_OK;
}

extern "C" int uf3_relax_create(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const uint8_t *fixed,
                                const double *c1, const double *c2, const double *c3, int relax_cell, uf3_relax **out) {
    const char *who = "uf3_relax_create";
    int64_t n = 0;
    int rc = batch_check(b, fr, pos, z, c1, c2, c3, out, who, &n);
    if (rc) return rc;
    uf3_ctx *c = b->ctx;
    if (relax_cell != 0 && relax_cell != 1) return fail(c, UF3_EINVAL, "uf3_relax_create: relax_cell must be 0 or 1");
    if (relax_cell && fixed) return fail(c, UF3_EINVAL, "uf3_relax_create: fixed atoms together with relax_cell are not supported");
    const int nf = fr->n_frames;
    if (fixed)
        for (int64_t i = 0; i < n; i++)
            if (fixed[i] > 1) return fail(c, UF3_EINVAL, "uf3_relax_create: fixed must hold 0 or 1 per atom");
    std::vector<RelaxFrame> st(nf);
    bool cell_run = false;
    for (int f = 0; f < nf; f++) {
        RelaxFrame &S = st[f];
        memset(&S, 0, sizeof(S));
        const double *cl = fr->cells + 9 * (size_t)f;
        const bool periodic = fr->pbc[3 * f] && fr->pbc[3 * f + 1] && fr->pbc[3 * f + 2];
        if (relax_cell && periodic && det3(cl) == 0.0) return fail(c, UF3_EINVAL, "uf3_relax_create: a periodic frame's cell is singular");
        S.cellf = relax_cell && periodic;
        cell_run = cell_run || S.cellf;
        S.fire.alpha = UF3_FIRE_ASTART; S.fire.first = 1;
        S.e_last = S.fmax_last = std::numeric_limits<double>::quiet_NaN();
        for (int k = 0; k < 9; k++) { S.D[k] = (k % 4 == 0) ? 1.0 : 0.0; S.cell0[k] = cl[k]; }
        S.status = UF3_RELAX_RUNNING;
    }
    HIPCHK(c, hipSetDevice(c->device));
    uf3_relax *r = new uf3_relax();
    r->cell_run = cell_run; r->has_fixed = fixed != nullptr;
    r->st_host = st;
    auto bail = [&](int rc) { uf3_relax_destroy(r); return rc; };
    rc = batch_init(*r, b, fr, pos, z, c1, c2, c3, 1, who);
    if (!rc) rc = chunk_table_build(c, r->offsets, nf, UF3_RELAX_THREADS, r->chunks, who);
    if (rc) return bail(rc);
    const size_t n3 = 3 * (size_t)n, nb = (size_t)r->chunks.n_blocks;
    if ((cell_run && r->q.ensure(8 * n3)) || r->vel.ensure(8 * n3) || r->frc.ensure(8 * n3) || (fixed && r->fixed.ensure((size_t)n)) ||
        r->virials.ensure(48 * (size_t)nf) || r->st.ensure(sizeof(RelaxFrame) * (size_t)nf) ||
        r->coef.ensure(sizeof(RelaxCoef) * (size_t)nf) || r->partial.ensure(32 * nb) || r->cells_dev.ensure(72 * (size_t)nf))
        return bail(fail(c, UF3_ENOMEM, "uf3_relax_create: out of device memory"));
    hipStream_t s = c->stream;
    if ((cell_run && hipMemcpyAsync(r->q.p, pos, 8 * n3, hipMemcpyHostToDevice, s)) || hipMemsetAsync(r->vel.p, 0, 8 * n3, s) ||
        (fixed && hipMemcpyAsync(r->fixed.p, fixed, (size_t)n, hipMemcpyHostToDevice, s)) ||
        hipMemcpyAsync(r->st.p, st.data(), sizeof(RelaxFrame) * (size_t)nf, hipMemcpyHostToDevice, s) ||
        hipMemsetAsync(r->coef.p, 0, sizeof(RelaxCoef) * (size_t)nf, s) ||
        hipMemcpyAsync(r->cells_dev.p, r->cells.data(), 72 * (size_t)nf, hipMemcpyHostToDevice, s) || hipStreamSynchronize(s))
        return bail(fail(c, UF3_EHIP, "uf3_relax_create: upload failed"));
    *out = r;
    return UF3_OK;
}

static int relax_forces(uf3_relax *r) {
    int rc = batch_eval(*r, r->frc.as<double>(), r->cell_run ? r->virials.as<double>() : nullptr);
    r->forces_valid = rc == UF3_OK;
    return rc;
}

static int relax_fetch_state(uf3_relax *r) {
    uf3_ctx *c = r->c;
    HIPCHK(c, hipMemcpyAsync(r->st_host.data(), r->st.p, sizeof(RelaxFrame) * (size_t)r->n_frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

// evaluations k = 0 .. max_steps; each but the last may move the frames still running
static int relax_run(uf3_relax *r, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, int64_t every,
                     int64_t rec_every, double *records) {
    uf3_ctx *c = r->c;
    hipStream_t s = c->stream;
    const int nf = r->n_frames;
    const int64_t n_rec = rec_every ? max_steps / rec_every + 1 : 0;
    if (n_rec) HIPCHK(c, r->ring.ensure(16 * (size_t)n_rec * nf));
    RelaxPartialArgs P;
    P.frc = r->frc.as<double>(); P.vel = r->vel.as<double>(); P.fixed = r->has_fixed ? r->fixed.as<uint8_t>() : nullptr;
    const ChunkTable &T = r->chunks;
    P.blk_frame = T.blk_frame.as<int>(); P.blk_lo = T.blk_lo.as<long long>(); P.blk_n = T.blk_n.as<int>();
    P.st = r->st.as<RelaxFrame>(); P.partial = r->partial.as<double>();
    RelaxFrameArgs F;
    F.partial = r->partial.as<double>(); F.frame_blk = T.frame_blk.as<int>(); F.offsets = r->offsets_dev.as<long long>();
    F.energies = r->energies.as<double>(); F.virials = r->cell_run ? r->virials.as<double>() : nullptr;
    F.st = r->st.as<RelaxFrame>(); F.coef = r->coef.as<RelaxCoef>(); F.cells = r->cells_dev.as<double>();
    F.fmax = fmax; F.dt0 = dt; F.dt_max = dt_max; F.maxstep = maxstep;
    RelaxMoveArgs M;
    M.pos = r->pos.as<double>(); M.vel = r->vel.as<double>(); M.q = r->cell_run ? r->q.as<double>() : nullptr;
    M.frc = r->frc.as<double>(); M.fixed = P.fixed; M.frame_of = T.frame_of.as<int>(); M.coef = r->coef.as<RelaxCoef>();
    M.n = r->natoms;
    int64_t last = max_steps;                   // the last evaluation made
    for (int64_t k = 0; k <= max_steps; k++) {
        if (!(k == 0 && r->forces_valid)) {     // (a run continues from the previous run's last evaluation)
            int rc = relax_forces(r);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_relax_partial, dim3((unsigned)T.n_blocks), dim3(UF3_RELAX_THREADS), 0, s, P);
        HIPCHK(c, hipGetLastError());
        F.rec = (n_rec && k % rec_every == 0) ? r->ring.as<double>() + 2 * (size_t)nf * (size_t)(k / rec_every) : nullptr;
        F.can_move = k < max_steps;
        hipLaunchKernelGGL(k_relax_frame, dim3((unsigned)nf), dim3(UF3_RELAX_THREADS), 0, s, F);
        HIPCHK(c, hipGetLastError());
        if (k == max_steps) break;
        hipLaunchKernelGGL(k_relax_move, dim3((unsigned)((r->natoms + UF3_RELAX_THREADS - 1) / UF3_RELAX_THREADS)),
                           dim3(UF3_RELAX_THREADS), 0, s, M);
        HIPCHK(c, hipGetLastError());
        r->forces_valid = false;
        if (r->cell_run) {                      // (the evaluator and its list build read the cells on the host)
            HIPCHK(c, hipMemcpyAsync(r->cells.data(), r->cells_dev.p, 72 * (size_t)nf, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        if ((k + 1) % every == 0) {             // poll: stop once no frame runs (nothing moved in this step then)
            int rc = relax_fetch_state(r);
            if (rc) return rc;
            bool running = false;
            for (int f = 0; f < nf; f++) running = running || r->st_host[f].status == UF3_RELAX_RUNNING;
            if (!running) { last = k; r->forces_valid = true; break; }
        }
    }
    int rc = relax_fetch_state(r);
    if (rc) return rc;
    if (n_rec) {
        // rows after the last evaluation repeat each frame's final values (no frame ran any more)
        const int64_t written = last / rec_every + 1;
        HIPCHK(c, hipMemcpyAsync(records, r->ring.p, 16 * (size_t)written * nf, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int64_t j = written; j < n_rec; j++)
            for (int f = 0; f < nf; f++) {
                records[2 * (j * nf + f)] = r->st_host[f].e_last;
                records[2 * (j * nf + f) + 1] = r->st_host[f].fmax_last;
            }
    }
    return UF3_OK;
}

extern "C" int uf3_relax_run(uf3_relax *r, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, double skin,
                             int64_t check_every, int64_t record_every, double *records) {
    if (!r) return fail(nullptr, UF3_EINVAL, "uf3_relax_run: relax is NULL");
    uf3_ctx *c = r->c;
    int rc = fire_run_check(c, "uf3_relax_run", max_steps, fmax, dt, dt_max, maxstep, skin, 0, check_every, record_every, records);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // (skin 0 in a cell run: the MD route's list key holds the cells)
    return with_run_skin(c, r->cell_run ? 0.0 : skin,
                         [&] { return relax_run(r, max_steps, fmax, dt, dt_max, maxstep, check_every, record_every, records); });
}

extern "C" int uf3_relax_get_state(uf3_relax *r, double *pos, double *cells, double *forces, double *energies, int32_t *status,
                                   int64_t *steps, double *fmax) {
    if (!r) return fail(nullptr, UF3_EINVAL, "uf3_relax_get_state: relax is NULL");
    uf3_ctx *c = r->c;
    HIPCHK(c, hipSetDevice(c->device));
    if ((forces || energies) && !r->forces_valid) {
        int rc = relax_forces(r);
        if (rc) return rc;
    }
    const size_t n3 = 3 * (size_t)r->natoms;
    if (pos) HIPCHK(c, hipMemcpyAsync(pos, r->pos.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (forces) HIPCHK(c, hipMemcpyAsync(forces, r->frc.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (energies) HIPCHK(c, hipMemcpyAsync(energies, r->energies.p, 8 * (size_t)r->n_frames, hipMemcpyDeviceToHost, c->stream));
    int rc = relax_fetch_state(r);
    if (rc) return rc;
    if (cells) memcpy(cells, r->cells.data(), 72 * (size_t)r->n_frames);
    for (int f = 0; f < r->n_frames; f++) {
        if (status) status[f] = r->st_host[f].status;
        if (steps) steps[f] = r->st_host[f].fire.steps;
        if (fmax) fmax[f] = r->st_host[f].fmax_last;
    }
    return UF3_OK;
}

// ------------------------------------------------------------------------------ nudged elastic bands (uf3_neb_*, uf3_neb.h)
// A library-owned set of bands: positions (unwrapped), velocities, true forces, NEB forces, the per-band optimiser state in HBM.
// Every step is one evaluator call over all frames (eval_impl, unchanged; the end points are evaluated with the rest because
// their energies are needed) and four launches; the host waits for the device only every check_every steps.
struct uf3_neb : Batch {
    int32_t n_bands = 0;
    bool has_fixed = false;
    std::vector<NebBand> st_host;
    std::vector<double> e_last_host;
    ChunkTable chunks;
    DevBuf vel, frc, g, fixed, e_last, frame_band, st, coef, img, partial, cmax, ring;
    bool forces_valid = false;                  // frc / energies describe pos
    bool g_valid = false;                       // g describes pos (and the climb flag of the last run)
    int last_climb = 0;
    bool idpp = false;                          // made by uf3_idpp_create: energies and forces are k_idpp's, not the evaluator's
    DevBuf idpp_cells, idpp_partial;
    // made by uf3_ssneb_create (k_neb_*<true>): the cell is part of every image's vector
    bool cellb = false;
    DevBuf q, fq, D, vc, G, gc, D_ev, vc_ev, kappa, virials, cells_dev;
};

extern "C" void uf3_neb_destroy(uf3_neb *r) { driver_destroy(r); }

static int idpp_setup(uf3_neb *r, const std::string &who);
static int ssneb_setup(uf3_neb *r, const double *pos, const int32_t *band_first_frame, const double *cell_factor, const std::string &who);

// uf3_neb_create (b: the basis of the model c1 / c2 / c3) and uf3_idpp_create (b null: no model, the handle evaluates k_idpp)
static int neb_create(uf3_ctx *c, uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const uint8_t *fixed,
                      const double *c1, const double *c2, const double *c3, int32_t n_bands, const int32_t *band_first_frame,
                      const double *spring, uf3_neb **out, const std::string &me, bool cellb = false,
                      const double *cell_factor = nullptr) {
    int64_t n = 0;
    int rc = batch_check(c, b, fr, pos, z, c1, c2, c3, out, me, &n);
    if (rc) return rc;
    if (n_bands < 1 || !band_first_frame || !spring) return fail(c, UF3_EINVAL, me + ": needs a band, band_first_frame and spring");
    const int nf = fr->n_frames;
    if (fixed)
        for (int64_t i = 0; i < n; i++)
            if (fixed[i] > 1) return fail(c, UF3_EINVAL, me + ": fixed must hold 0 or 1 per atom");
    if (band_first_frame[0] != 0 || band_first_frame[n_bands] != nf)
        return fail(c, UF3_EINVAL, me + ": band_first_frame must run from 0 to n_frames");
    std::vector<NebBand> st(n_bands);
    std::vector<int> frame_band(nf);
    for (int bd = 0; bd < n_bands; bd++) {
        const int f0 = band_first_frame[bd], M = band_first_frame[bd + 1] - f0;
        const std::string who = me + ": band " + std::to_string(bd);
        if (M < 3) return fail(c, UF3_EINVAL, who + " has " + std::to_string(M) + " images; a band needs at least 3");
        if (!(spring[bd] > 0.0) || !std::isfinite(spring[bd])) return fail(c, UF3_EINVAL, who + ": spring must be positive and finite");
        const int64_t lo0 = fr->atom_offsets[f0], na = fr->atom_offsets[f0 + 1] - lo0;
        for (int j = 1; j < M; j++) {
            const int f = f0 + j;
            const int64_t lo = fr->atom_offsets[f];
            const std::string img = who + ", image " + std::to_string(j);
            if (fr->atom_offsets[f + 1] - lo != na) return fail(c, UF3_EINVAL, img + ": atom count differs from image 0");
            if (memcmp(z + lo, z + lo0, 4 * (size_t)na)) return fail(c, UF3_EINVAL, img + ": species differ from image 0");
            if (!cellb && memcmp(fr->cells + 9 * (size_t)f, fr->cells + 9 * (size_t)f0, 72))
                return fail(c, UF3_EINVAL, img + ": cell differs from image 0");
            for (int k = 0; k < 3; k++)
                if ((fr->pbc[3 * f + k] != 0) != (fr->pbc[3 * f0 + k] != 0)) return fail(c, UF3_EINVAL, img + ": pbc differs from image 0");
            if (fixed && memcmp(fixed + lo, fixed + lo0, (size_t)na)) return fail(c, UF3_EINVAL, img + ": fixed mask differs from image 0");
            bool same = true;
            for (int64_t q = 0; q < 3 * na && same; q++) same = pos[3 * lo + q] == pos[3 * (lo - na) + q];
            if (same) return fail(c, UF3_EINVAL, img + ": positions identical to image " + std::to_string(j - 1));
        }
        if (cellb) {
            if (cell_factor && (!(cell_factor[bd] > 0.0) || !std::isfinite(cell_factor[bd])))
                return fail(c, UF3_EINVAL, who + ": cell_factor must be positive and finite");
            for (int j = 0; j < M; j++) {
                const int f = f0 + j;
                const std::string img = who + ", image " + std::to_string(j);
                if (!(fr->pbc[3 * f] && fr->pbc[3 * f + 1] && fr->pbc[3 * f + 2]))
                    return fail(c, UF3_EINVAL, img + ": a cell band needs frames periodic along all three axes");
                const double *cl = fr->cells + 9 * (size_t)f;
                // (singular to rounding: the volume against the product of the row lengths)
                if (!(std::fabs(det3(cl)) > 1e-12 * norm3(cl) * norm3(cl + 3) * norm3(cl + 6)))
                    return fail(c, UF3_EINVAL, img + ": the cell is singular");
            }
        }
        NebBand &S = st[bd];
        memset(&S, 0, sizeof(S));
        S.fire.alpha = UF3_FIRE_ASTART; S.fire.first = 1; S.spring = spring[bd];
        S.crit_last = std::numeric_limits<double>::quiet_NaN();
        S.status = UF3_RELAX_RUNNING; S.climbing = -1; S.frame0 = f0; S.n_img = M;
        for (int j = 0; j < M; j++) frame_band[f0 + j] = bd;
    }
    HIPCHK(c, hipSetDevice(c->device));
    uf3_neb *r = new uf3_neb();
    r->n_bands = n_bands; r->has_fixed = fixed != nullptr;
    r->st_host = st;
    r->e_last_host.assign(nf, std::numeric_limits<double>::quiet_NaN());
    auto bail = [&](int rc) { uf3_neb_destroy(r); return rc; };
    rc = batch_init(*r, c, b, fr, pos, z, c1, c2, c3, 1, me);
    if (!rc) rc = chunk_table_build(c, r->offsets, nf, UF3_RELAX_THREADS, r->chunks, me);
    if (rc) return bail(rc);
    const size_t n3 = 3 * (size_t)n, nb = (size_t)r->chunks.n_blocks;
    if (r->vel.ensure(8 * n3) || r->frc.ensure(8 * n3) || r->g.ensure(8 * n3) || (fixed && r->fixed.ensure((size_t)n)) ||
        r->e_last.ensure(8 * (size_t)nf) || r->frame_band.ensure(4 * (size_t)nf) || r->st.ensure(sizeof(NebBand) * (size_t)n_bands) ||
        r->coef.ensure(sizeof(NebCoef) * (size_t)n_bands) || r->img.ensure(sizeof(NebImage) * (size_t)nf) ||
        r->partial.ensure(8 * UF3_NEB_NSUM * nb) || r->cmax.ensure(8 * nb))
        return bail(fail(c, UF3_ENOMEM, me + ": out of device memory"));
    hipStream_t s = c->stream;
    if (hipMemsetAsync(r->vel.p, 0, 8 * n3, s) || hipMemsetAsync(r->g.p, 0, 8 * n3, s) ||
        (fixed && hipMemcpyAsync(r->fixed.p, fixed, (size_t)n, hipMemcpyHostToDevice, s)) ||
        hipMemcpyAsync(r->e_last.p, r->e_last_host.data(), 8 * (size_t)nf, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(r->frame_band.p, frame_band.data(), 4 * (size_t)nf, hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(r->st.p, st.data(), sizeof(NebBand) * (size_t)n_bands, hipMemcpyHostToDevice, s) ||
        hipMemsetAsync(r->coef.p, 0, sizeof(NebCoef) * (size_t)n_bands, s) ||
        hipMemsetAsync(r->img.p, 0, sizeof(NebImage) * (size_t)nf, s) ||
        hipMemsetAsync(r->partial.p, 0, 8 * UF3_NEB_NSUM * nb, s) || hipMemsetAsync(r->cmax.p, 0, 8 * nb, s) ||
        hipStreamSynchronize(s))
        return bail(fail(c, UF3_EHIP, me + ": upload failed"));
    if (!b) {
        rc = idpp_setup(r, me);
        if (rc) return bail(rc);
    }
    if (cellb) {
        rc = ssneb_setup(r, pos, band_first_frame, cell_factor, me);
        if (rc) return bail(rc);
    }
    *out = r;
    return UF3_OK;
}

extern "C" int uf3_neb_create(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const uint8_t *fixed,
                              const double *c1, const double *c2, const double *c3, int32_t n_bands, const int32_t *band_first_frame,
                              const double *spring, uf3_neb **out) {
    if (!b) return fail(nullptr, UF3_EINVAL, "uf3_neb_create: basis is NULL");
    return neb_create(b->ctx, b, fr, pos, z, fixed, c1, c2, c3, n_bands, band_first_frame, spring, out, "uf3_neb_create");
}

// the cell band's own state: D_i = C0^-1 C_i and q_i = x_i D_i^-1 per image (host, once), zero cell velocities, kappa per band
// (cell_factor null: the band's atom count per image, uf3_relax.h's convention)
static int ssneb_setup(uf3_neb *r, const double *pos, const int32_t *band_first_frame, const double *cell_factor, const std::string &who) {
    uf3_ctx *c = r->c;
    r->cellb = true;
    const int nf = r->n_frames, nbd = r->n_bands;
    const size_t n3 = 3 * (size_t)r->natoms;
    std::vector<double> D(9 * (size_t)nf), q(n3), kappa(nbd);
    for (int bd = 0; bd < nbd; bd++) {
        const int f0 = band_first_frame[bd], M = band_first_frame[bd + 1] - f0;
        kappa[bd] = cell_factor ? cell_factor[bd] : (double)(r->offsets[f0 + 1] - r->offsets[f0]);
        double C0i[9];
        relax_inv3(r->cells.data() + 9 * (size_t)f0, C0i);
        for (int j = 0; j < M; j++) {
            const int f = f0 + j;
            const double *C = r->cells.data() + 9 * (size_t)f;
            double *Df = D.data() + 9 * (size_t)f, Di[9];
            for (int a = 0; a < 3; a++)
                for (int k = 0; k < 3; k++)
                    Df[3 * a + k] = j == 0 ? (a == k ? 1.0 : 0.0) : C0i[3 * a] * C[k] + C0i[3 * a + 1] * C[3 + k] + C0i[3 * a + 2] * C[6 + k];
            relax_inv3(Df, Di);
            for (int64_t i = r->offsets[f]; i < r->offsets[f + 1]; i++)
                for (int k = 0; k < 3; k++)
                    q[3 * i + k] = pos[3 * i] * Di[k] + pos[3 * i + 1] * Di[3 + k] + pos[3 * i + 2] * Di[6 + k];
        }
    }
    if (!md_finite(D.data(), D.size()) || !md_finite(q.data(), q.size()))
        return fail(c, UF3_EINVAL, who + ": the images' cells do not give finite deformations of image 0's cell");
    const size_t f9 = 72 * (size_t)nf;
    if (r->q.ensure(8 * n3) || r->fq.ensure(8 * n3) || r->D.ensure(f9) || r->vc.ensure(f9) || r->G.ensure(f9) || r->gc.ensure(f9) ||
        r->D_ev.ensure(f9) || r->vc_ev.ensure(f9) || r->kappa.ensure(8 * (size_t)nbd) || r->virials.ensure(48 * (size_t)nf) ||
        r->cells_dev.ensure(f9))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    hipStream_t s = c->stream;
    if (hipMemcpyAsync(r->q.p, q.data(), 8 * n3, hipMemcpyHostToDevice, s) || hipMemsetAsync(r->fq.p, 0, 8 * n3, s) ||
        hipMemcpyAsync(r->D.p, D.data(), f9, hipMemcpyHostToDevice, s) || hipMemsetAsync(r->vc.p, 0, f9, s) ||
        hipMemsetAsync(r->G.p, 0, f9, s) || hipMemsetAsync(r->gc.p, 0, f9, s) ||
        hipMemcpyAsync(r->D_ev.p, D.data(), f9, hipMemcpyHostToDevice, s) || hipMemsetAsync(r->vc_ev.p, 0, f9, s) ||
        hipMemcpyAsync(r->kappa.p, kappa.data(), 8 * (size_t)nbd, hipMemcpyHostToDevice, s) ||
        hipMemsetAsync(r->virials.p, 0, 48 * (size_t)nf, s) ||
        hipMemcpyAsync(r->cells_dev.p, r->cells.data(), f9, hipMemcpyHostToDevice, s) || hipStreamSynchronize(s))
        return fail(c, UF3_EHIP, who + ": upload failed");      // (waited for: the host vectors go out of scope)
    return UF3_OK;
}

extern "C" int uf3_ssneb_create(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                                const double *c2, const double *c3, int32_t n_bands, const int32_t *band_first_frame,
                                const double *spring, const double *cell_factor, uf3_neb **out) {
    if (!b) return fail(nullptr, UF3_EINVAL, "uf3_ssneb_create: basis is NULL");
    return neb_create(b->ctx, b, fr, pos, z, nullptr, c1, c2, c3, n_bands, band_first_frame, spring, out, "uf3_ssneb_create", true,
                      cell_factor);
}

// one frame's cell for k_idpp: the inverse of the cell completed as neb._axes does (the rows of non-periodic axes replaced by unit
// vectors orthogonal to the rows there) and the flags.  False: the periodic rows span nothing
static bool idpp_cell(const double *cell, const uint8_t *pbc, IdppCell &C) {
    double h[3][3];
    int np = 0;
    for (int k = 0; k < 3; k++) {
        C.per[k] = pbc[k] != 0;
        np += C.per[k];
        for (int q = 0; q < 3; q++) h[k][q] = C.per[k] ? cell[3 * k + q] : 0.0;
    }
    auto cross = [](const double *u, const double *v, double *w) {
        w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
    };
    auto unit = [](double *w) {
        const double l = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        if (!(l > 0.0) || !std::isfinite(l)) return false;
        for (int q = 0; q < 3; q++) w[q] /= l;
        return true;
    };
    if (np == 2) {
        const int k = !C.per[0] ? 0 : (!C.per[1] ? 1 : 2);
        cross(h[(k + 1) % 3], h[(k + 2) % 3], h[k]);
        if (!unit(h[k])) return false;
    } else if (np == 1) {
        const int k = C.per[0] ? 0 : (C.per[1] ? 1 : 2);
        int m = 0;                                  // the Cartesian axis least along the row
        for (int q = 1; q < 3; q++) if (std::fabs(h[k][q]) < std::fabs(h[k][m])) m = q;
        double e[3] = {0.0, 0.0, 0.0};
        e[m] = 1.0;
        cross(h[k], e, h[(k + 1) % 3]);
        if (!unit(h[(k + 1) % 3])) return false;
        cross(h[k], h[(k + 1) % 3], h[(k + 2) % 3]);
        if (!unit(h[(k + 2) % 3])) return false;
    } else if (np == 0) {
        for (int k = 0; k < 3; k++) h[k][k] = 1.0;
    }
    double co[3][3];
    cross(h[1], h[2], co[0]); cross(h[2], h[0], co[1]); cross(h[0], h[1], co[2]);
    const double det = h[0][0] * co[0][0] + h[0][1] * co[0][1] + h[0][2] * co[0][2];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
    bool ortho = true;
    for (int k = 0; k < 3; k++) {
        for (int q = 0; q < 3; q++) {
            C.h[3 * k + q] = C.per[k] ? cell[3 * k + q] : 0.0;
            C.g[3 * k + q] = co[k][q] / det;        // the fraction along axis k of D: D . (h_l x h_m) / det
        }
        for (int l = k + 1; l < 3; l++)
            if (C.per[k] && C.per[l] && h[k][0] * h[l][0] + h[k][1] * h[l][1] + h[k][2] * h[l][2] != 0.0) ortho = false;
    }
    C.search = (np > 0 && !ortho) ? 1 : 0;          // mutually orthogonal periodic rows (exact zeros): rounding alone is exact
    return true;
}

static int idpp_setup(uf3_neb *r, const std::string &who) {
    uf3_ctx *c = r->c;
    r->idpp = true;
    std::vector<IdppCell> cells(r->n_frames);
    for (int f = 0; f < r->n_frames; f++)
        if (!idpp_cell(r->cells.data() + 9 * (size_t)f, r->pbc.data() + 3 * (size_t)f, cells[f]))
            return fail(c, UF3_EINVAL, who + ": frame " + std::to_string(f) + ": the periodic cell rows span no volume");
    if (r->idpp_cells.ensure(sizeof(IdppCell) * cells.size()) || r->idpp_partial.ensure(8 * (size_t)r->chunks.n_blocks))
        return fail(c, UF3_ENOMEM, who + ": out of device memory");
    if (hipMemcpyAsync(r->idpp_cells.p, cells.data(), sizeof(IdppCell) * cells.size(), hipMemcpyHostToDevice, c->stream) ||
        hipStreamSynchronize(c->stream))
        return fail(c, UF3_EHIP, who + ": upload failed");
    return UF3_OK;
}

extern "C" int uf3_idpp_create(uf3_ctx *c, const uf3_frames *fr, const double *pos, const int32_t *z, const uint8_t *fixed,
                               int32_t n_bands, const int32_t *band_first_frame, const double *spring, uf3_neb **out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_idpp_create: ctx is NULL");
    return neb_create(c, nullptr, fr, pos, z, fixed, nullptr, nullptr, nullptr, n_bands, band_first_frame, spring, out, "uf3_idpp_create");
}

// S and F of every image of a handle of uf3_idpp_create (k_idpp, k_idpp_sum): no lists, no model, nothing of the context's MD state
static int idpp_evaluate(uf3_neb *r) {
    uf3_ctx *c = r->c;
    const ChunkTable &T = r->chunks;
    IdppArgs P;
    P.pos = r->pos.as<double>(); P.blk_frame = T.blk_frame.as<int>(); P.blk_lo = T.blk_lo.as<long long>(); P.blk_n = T.blk_n.as<int>();
    P.frame_blk = T.frame_blk.as<int>(); P.frame_band = r->frame_band.as<int>(); P.offsets = r->offsets_dev.as<long long>();
    P.bands = r->st.as<NebBand>(); P.cells = r->idpp_cells.as<IdppCell>(); P.frc = r->frc.as<double>();
    P.partial = r->idpp_partial.as<double>(); P.energies = r->energies.as<double>(); P.n_frames = r->n_frames;
    hipLaunchKernelGGL(k_idpp, dim3((unsigned)T.n_blocks), dim3(UF3_RELAX_THREADS), 0, c->stream, P);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_idpp_sum, dim3((unsigned)((r->n_frames + UF3_RELAX_THREADS - 1) / UF3_RELAX_THREADS)), dim3(UF3_RELAX_THREADS), 0,
                       c->stream, P);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

static int neb_evaluate(uf3_neb *r) {
    int rc = r->idpp ? idpp_evaluate(r) : batch_eval(*r, r->frc.as<double>(), r->cellb ? r->virials.as<double>() : nullptr);
    r->forces_valid = rc == UF3_OK;
    r->g_valid = false;
    return rc;
}

static int neb_fetch_state(uf3_neb *r) {
    uf3_ctx *c = r->c;
    HIPCHK(c, hipMemcpyAsync(r->st_host.data(), r->st.p, sizeof(NebBand) * (size_t)r->n_bands, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return UF3_OK;
}

static NebChunkArgs neb_chunk_args(uf3_neb *r, int climb, int all) {
    NebChunkArgs P;
    P.pos = r->cellb ? r->q.as<double>() : r->pos.as<double>(); P.frc = r->frc.as<double>(); P.vel = r->vel.as<double>();
    P.fixed = r->has_fixed ? r->fixed.as<uint8_t>() : nullptr;
    const ChunkTable &T = r->chunks;
    P.blk_frame = T.blk_frame.as<int>(); P.blk_lo = T.blk_lo.as<long long>(); P.blk_n = T.blk_n.as<int>();
    P.frame_blk = T.frame_blk.as<int>(); P.frame_band = r->frame_band.as<int>(); P.offsets = r->offsets_dev.as<long long>();
    P.energies = r->energies.as<double>(); P.bands = r->st.as<NebBand>(); P.partial = r->partial.as<double>();
    P.g = r->g.as<double>(); P.cmax = r->cmax.as<double>(); P.img = r->img.as<NebImage>();
    P.climb = climb; P.all = all;
    // (null pointers on a handle without cells)
    P.virials = r->virials.as<double>(); P.D = r->D.as<double>(); P.vc = r->vc.as<double>(); P.kappa = r->kappa.as<double>();
    P.fq = r->fq.as<double>(); P.G = r->G.as<double>(); P.D_ev = r->D_ev.as<double>(); P.vc_ev = r->vc_ev.as<double>();
    P.gc = r->gc.as<double>();
    return P;
}

// the partial and the force launch of an evaluation (the <true> instances on a handle of uf3_ssneb_create)
static int neb_launch_forces(uf3_neb *r, const NebChunkArgs &P) {
    uf3_ctx *c = r->c;
    const dim3 grid((unsigned)r->chunks.n_blocks), blk(UF3_RELAX_THREADS);
    return with_bool(r->cellb, [&](auto CELL) {
        hipLaunchKernelGGL(k_neb_partial<CELL>, grid, blk, 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_neb_force<CELL>, grid, blk, 0, c->stream, P);
        HIPCHK(c, hipGetLastError());
        return (int)UF3_OK;
    });
}

// evaluations k = 0 .. max_steps; each but the last may move the bands still running
static int neb_run(uf3_neb *r, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, int climb, int64_t every,
                   int64_t rec_every, double *records) {
    uf3_ctx *c = r->c;
    hipStream_t s = c->stream;
    const int nf = r->n_frames, nbd = r->n_bands;
    const size_t row = (size_t)nf + 2 * (size_t)nbd;
    const int64_t n_rec = rec_every ? max_steps / rec_every + 1 : 0;
    if (n_rec) HIPCHK(c, r->ring.ensure(8 * (size_t)n_rec * row));
    const NebChunkArgs P = neb_chunk_args(r, climb, 0);
    NebBandArgs F;
    F.cmax = r->cmax.as<double>(); F.frame_blk = r->chunks.frame_blk.as<int>(); F.energies = r->energies.as<double>();
    F.img = r->img.as<NebImage>(); F.bands = r->st.as<NebBand>(); F.coef = r->coef.as<NebCoef>(); F.e_last = r->e_last.as<double>();
    F.fmax = fmax; F.dt0 = dt; F.dt_max = dt_max; F.maxstep = maxstep; F.n_frames = nf; F.climb = climb;
    NebMoveArgs M;
    M.pos = r->pos.as<double>(); M.vel = r->vel.as<double>(); M.g = r->g.as<double>(); M.fixed = P.fixed;
    M.frame_of = r->chunks.frame_of.as<int>(); M.frame_band = r->frame_band.as<int>(); M.bands = r->st.as<NebBand>();
    M.coef = r->coef.as<NebCoef>(); M.n = r->natoms;
    // (null pointers on a handle without cells)
    M.q = r->q.as<double>(); M.D = r->D.as<double>(); M.vc = r->vc.as<double>(); M.cells = r->cells_dev.as<double>();
    M.gc = r->gc.as<double>(); M.D_ev = r->D_ev.as<double>(); M.vc_ev = r->vc_ev.as<double>(); M.kappa = r->kappa.as<double>();
    M.offsets = r->offsets_dev.as<long long>();
    r->last_climb = climb;
    hipLaunchKernelGGL(k_neb_rearm, dim3((unsigned)((nbd + UF3_RELAX_THREADS - 1) / UF3_RELAX_THREADS)), dim3(UF3_RELAX_THREADS), 0, s,
                       r->st.as<NebBand>(), nbd);
    HIPCHK(c, hipGetLastError());
    int64_t last = max_steps;                   // the last evaluation made
    for (int64_t k = 0; k <= max_steps; k++) {
        if (!(k == 0 && r->forces_valid)) {     // (a run continues from the previous run's last evaluation)
            int rc = neb_evaluate(r);
            if (rc) return rc;
        }
        int rl = neb_launch_forces(r, P);
        if (rl) return rl;
        F.rec = (n_rec && k % rec_every == 0) ? r->ring.as<double>() + row * (size_t)(k / rec_every) : nullptr;
        F.can_move = k < max_steps;
        hipLaunchKernelGGL(k_neb_band, dim3((unsigned)nbd), dim3(UF3_RELAX_THREADS), 0, s, F);
        HIPCHK(c, hipGetLastError());
        r->g_valid = false;                     // (frozen bands' rows are older than this evaluation: get_state forms them all)
        if (k == max_steps) break;
        const dim3 mgrid((unsigned)((r->natoms + UF3_RELAX_THREADS - 1) / UF3_RELAX_THREADS));
        rl = with_bool(r->cellb, [&](auto CELL) {
            hipLaunchKernelGGL(k_neb_move<CELL>, mgrid, dim3(UF3_RELAX_THREADS), 0, s, M);
            HIPCHK(c, hipGetLastError());
            return (int)UF3_OK;
        });
        if (rl) return rl;
        r->forces_valid = false;
        if (r->cellb) {                         // (the evaluator and its list build read the cells on the host)
            HIPCHK(c, hipMemcpyAsync(r->cells.data(), r->cells_dev.p, 72 * (size_t)nf, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        if ((k + 1) % every == 0) {             // poll: stop once no band runs (nothing moved in this step then)
            int rc = neb_fetch_state(r);
            if (rc) return rc;
            bool running = false;
            for (int bd = 0; bd < nbd; bd++) running = running || r->st_host[bd].status == UF3_RELAX_RUNNING;
            if (!running) { last = k; r->forces_valid = true; break; }
        }
    }
    int rc = neb_fetch_state(r);
    if (rc) return rc;
    if (n_rec) {
        // rows after the last evaluation repeat the final values (no band ran any more)
        const int64_t written = last / rec_every + 1;
        HIPCHK(c, hipMemcpyAsync(records, r->ring.p, 8 * (size_t)written * row, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(r->e_last_host.data(), r->e_last.p, 8 * (size_t)nf, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int64_t j = written; j < n_rec; j++) {
            double *out = records + (size_t)j * row;
            for (int f = 0; f < nf; f++) out[f] = r->e_last_host[f];
            for (int bd = 0; bd < nbd; bd++) {
                out[nf + 2 * bd] = r->st_host[bd].crit_last;
                out[nf + 2 * bd + 1] = (double)r->st_host[bd].climbing;
            }
        }
    }
    return UF3_OK;
}

extern "C" int uf3_neb_run(uf3_neb *r, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, double skin,
                           int climb, int64_t check_every, int64_t record_every, double *records) {
    if (!r) return fail(nullptr, UF3_EINVAL, "uf3_neb_run: neb is NULL");
    uf3_ctx *c = r->c;
    int rc = fire_run_check(c, "uf3_neb_run", max_steps, fmax, dt, dt_max, maxstep, skin, climb, check_every, record_every, records);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (r->idpp) {                              // no lists are built: the context's MD skin is not touched
        if (climb) return fail(c, UF3_EINVAL, "uf3_neb_run: a handle of uf3_idpp_create takes no climbing image");
        return neb_run(r, max_steps, fmax, dt, dt_max, maxstep, 0, check_every, record_every, records);
    }
    // (skin 0 on a handle of uf3_ssneb_create: the MD route's list key holds the cells)
    return with_run_skin(c, r->cellb ? 0.0 : skin,
                         [&] { return neb_run(r, max_steps, fmax, dt, dt_max, maxstep, climb, check_every, record_every, records); });
}

static int neb_all_forces(uf3_neb *r) {
    int rc = neb_launch_forces(r, neb_chunk_args(r, r->last_climb, 1));
    r->g_valid = rc == UF3_OK;
    return rc;
}

extern "C" int uf3_neb_get_state(uf3_neb *r, double *pos, double *forces, double *neb_forces, double *energies, int32_t *status,
                                 int64_t *steps, double *criterion, int32_t *climbing) {
    if (!r) return fail(nullptr, UF3_EINVAL, "uf3_neb_get_state: neb is NULL");
    uf3_ctx *c = r->c;
    HIPCHK(c, hipSetDevice(c->device));
    if ((forces || energies || neb_forces) && !r->forces_valid) {
        int rc = neb_evaluate(r);
        if (rc) return rc;
    }
    // g of every band at these positions, frozen bands included; no state changes (a cell band's forces are F D^T: k_neb_partial's)
    if ((neb_forces || (forces && r->cellb)) && !r->g_valid) {
        int rc = neb_all_forces(r);
        if (rc) return rc;
    }
    const size_t n3 = 3 * (size_t)r->natoms;
    if (pos) HIPCHK(c, hipMemcpyAsync(pos, r->pos.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (forces) HIPCHK(c, hipMemcpyAsync(forces, r->cellb ? r->fq.p : r->frc.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (neb_forces) HIPCHK(c, hipMemcpyAsync(neb_forces, r->g.p, 8 * n3, hipMemcpyDeviceToHost, c->stream));
    if (energies) HIPCHK(c, hipMemcpyAsync(energies, r->energies.p, 8 * (size_t)r->n_frames, hipMemcpyDeviceToHost, c->stream));
    int rc = neb_fetch_state(r);
    if (rc) return rc;
    for (int bd = 0; bd < r->n_bands; bd++) {
        if (status) status[bd] = r->st_host[bd].status;
        if (steps) steps[bd] = r->st_host[bd].fire.steps;
        if (criterion) criterion[bd] = r->st_host[bd].crit_last;
        if (climbing) climbing[bd] = r->st_host[bd].climbing;
    }
    return UF3_OK;
}

extern "C" int uf3_neb_get_cell_state(uf3_neb *r, double *cells, double *virials, double *cell_forces, double *neb_cell_forces) {
    if (!r) return fail(nullptr, UF3_EINVAL, "uf3_neb_get_cell_state: neb is NULL");
    uf3_ctx *c = r->c;
    if (!r->cellb) return fail(c, UF3_EINVAL, "uf3_neb_get_cell_state: the handle is not a cell band (uf3_ssneb_create)");
    HIPCHK(c, hipSetDevice(c->device));
    if ((virials || cell_forces || neb_cell_forces) && !r->forces_valid) {
        int rc = neb_evaluate(r);
        if (rc) return rc;
    }
    if ((cell_forces || neb_cell_forces) && !r->g_valid) {
        int rc = neb_all_forces(r);
        if (rc) return rc;
    }
    const size_t nf = (size_t)r->n_frames;
    if (virials) HIPCHK(c, hipMemcpyAsync(virials, r->virials.p, 48 * nf, hipMemcpyDeviceToHost, c->stream));
    if (cell_forces) HIPCHK(c, hipMemcpyAsync(cell_forces, r->G.p, 72 * nf, hipMemcpyDeviceToHost, c->stream));
    if (neb_cell_forces) HIPCHK(c, hipMemcpyAsync(neb_cell_forces, r->gc.p, 72 * nf, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cells) memcpy(cells, r->cells.data(), 72 * nf);
    return UF3_OK;
}

// ------------------------------------------------------------------------------ species-swap Monte Carlo (uf3_mc_*, uf3_mc.h)
// A library-owned batch of lattice Monte Carlo chains on fixed positions: the species (atomic numbers) live in HBM and change there,
// the neighbour table depends on the positions alone (built on the host at creation and by uf3_mc_set_positions, O(N^2 images)
// per frame: once per geometry, not per trial), the running energies start from the evaluator's (eval_impl, energies only: the
// context's MD lists and skin are not touched) and follow the accepted differences.
struct uf3_mc : Batch {
    int max_frame = 0;                          // atoms of the largest frame
    bool has_mask = false, energy_valid = false;
    uint64_t trial = 0;                         // absolute index of the next trial (Philox counter)
    std::vector<double> pos_host;
    int s2z[UF3_MAX_SPECIES] = {0};
    DevBuf swappable, accepted, trials, status, kT, off2, off3, ent2, ent3, c1d, c2d, c3d, ring, prop, dE;
};

extern "C" void uf3_mc_destroy(uf3_mc *m) { driver_destroy(m); }

// the geometry-only neighbour table of the object's positions: the evaluator's candidate set (images -fac .. fac of every atom of
// the frame, image_delta's arithmetic) cut at the largest pair range and at the 3-body range, entries in supercell index order
static int mc_build_table(uf3_mc *m, const char *who) {
    uf3_ctx *c = m->c;
    const uf3_basis *b = m->b;
    const BasisDev &H = b->host;
    double s2_hi = 0.0;
    for (int p = 0; p < H.P; p++) s2_hi = std::max(s2_hi, H.pairs[p].s_hi);
    const bool has3 = H.T > 0;
    std::vector<long long> off2(m->natoms + 1, 0), off3(m->natoms + 1, 0);
    std::vector<McEnt2> ent2;
    std::vector<McEnt3> ent3;
    auto image_pos_h = [](int s) { return s == 0 ? 0 : (s > 0 ? 2 * s - 1 : -2 * s); };
    for (int f = 0; f < m->n_frames; f++) {
        const double *cell = m->cells.data() + 9 * (size_t)f;
        const uint8_t *pbc = m->pbc.data() + 3 * (size_t)f;
        const int64_t lo = m->offsets[f], n = m->offsets[f + 1] - lo;
        int fac[3] = {0, 0, 0};
        if (pbc[0] || pbc[1] || pbc[2]) {
            reference_factors(cell, b->r_cut, fac);
            for (int k = 0; k < 3; k++) if (!pbc[k]) fac[k] = 0;
        }
        for (int k = 0; k < 3; k++)
            if (fac[k] > 400) return fail(c, UF3_EINVAL, std::string(who) + ": cell is too small relative to the cutoff");
        const int cnt[3] = {2 * fac[0] + 1, 2 * fac[1] + 1, 2 * fac[2] + 1};
        // the image shifts in the order of their rank in the reference supercell
        struct Shift { int rank, s[3]; double off[3]; };
        std::vector<Shift> shifts;
        for (int s0 = -fac[0]; s0 <= fac[0]; s0++)
            for (int s1 = -fac[1]; s1 <= fac[1]; s1++)
                for (int s2 = -fac[2]; s2 <= fac[2]; s2++) {
                    Shift sh;
                    sh.rank = (image_pos_h(s1) * cnt[0] + image_pos_h(s0)) * cnt[2] + image_pos_h(s2);
                    sh.s[0] = s0; sh.s[1] = s1; sh.s[2] = s2;
                    for (int k = 0; k < 3; k++) sh.off[k] = s0 * cell[k] + s1 * cell[3 + k] + s2 * cell[6 + k];
                    shifts.push_back(sh);
                }
        std::sort(shifts.begin(), shifts.end(), [](const Shift &a, const Shift &b2) { return a.rank < b2.rank; });
        const double *P = m->pos_host.data() + 3 * (size_t)lo;
        for (int64_t i = 0; i < n; i++) {
            int n3_here = 0;
            for (const Shift &sh : shifts)
                for (int64_t j = 0; j < n; j++) {
                    if (i == j && sh.rank == 0) continue;
                    const double dx = (P[3 * j] + sh.off[0]) - P[3 * i], dy = (P[3 * j + 1] + sh.off[1]) - P[3 * i + 1],
                                 dz = (P[3 * j + 2] + sh.off[2]) - P[3 * i + 2];
                    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                    const double s = (xx + yy) + zz;
                    if (s < s2_hi) { McEnt2 e; e.s = s; e.atom = (int)j; e.pad = 0; ent2.push_back(e); }
                    if (has3 && s > H.s3_lo && s <= H.s3_hi) {
                        McEnt3 e;
                        e.dx = dx; e.dy = dy; e.dz = dz; e.r = std::sqrt(s); e.atom = (int)j; e.pad[0] = e.pad[1] = e.pad[2] = 0;
                        ent3.push_back(e);
                        n3_here++;
                    }
                }
            if (n3_here > UF3_MC_MAX_N3)
                return fail(c, UF3_EINVAL, std::string(who) + ": an atom has " + std::to_string(n3_here) + " neighbours in the 3-body range, "
                            "more than the " + std::to_string(UF3_MC_MAX_N3) + " the trial kernel's LDS list holds");
            off2[lo + i + 1] = (long long)ent2.size();
            off3[lo + i + 1] = (long long)ent3.size();
        }
    }
    const size_t nn = (size_t)m->natoms + 1;
    HIPCHK(c, m->off2.ensure(8 * nn));
    HIPCHK(c, m->off3.ensure(8 * nn));
    HIPCHK(c, m->ent2.ensure(sizeof(McEnt2) * std::max<size_t>(ent2.size(), 1)));
    HIPCHK(c, m->ent3.ensure(sizeof(McEnt3) * std::max<size_t>(ent3.size(), 1)));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(m->off2.p, off2.data(), 8 * nn, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(m->off3.p, off3.data(), 8 * nn, hipMemcpyHostToDevice, s));
    if (!ent2.empty()) HIPCHK(c, hipMemcpyAsync(m->ent2.p, ent2.data(), sizeof(McEnt2) * ent2.size(), hipMemcpyHostToDevice, s));
    if (!ent3.empty()) HIPCHK(c, hipMemcpyAsync(m->ent3.p, ent3.data(), sizeof(McEnt3) * ent3.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(m->pos.p, m->pos_host.data(), 24 * (size_t)m->natoms, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));           // (the host vectors go out of scope)
    m->energy_valid = false;
    return UF3_OK;
}

extern "C" int uf3_mc_create(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const uint8_t *swappable,
                             const double *c1, const double *c2, const double *c3, uf3_mc **out) {
    const char *who = "uf3_mc_create";
    int64_t n = 0;
    int rc = batch_check(b, fr, pos, z, c1, c2, c3, out, who, &n);
    if (rc) return rc;
    uf3_ctx *c = b->ctx;
    const int nf = fr->n_frames;
    int max_frame = 0;
    for (int f = 0; f < nf; f++) {
        const int64_t nfr = fr->atom_offsets[f + 1] - fr->atom_offsets[f];
        if (nfr > UF3_MC_MAX_ATOMS)
            return fail(c, UF3_EINVAL, "uf3_mc_create: a frame holds more than " + std::to_string(UF3_MC_MAX_ATOMS) + " atoms (its species sit in LDS)");
        max_frame = std::max(max_frame, (int)nfr);
    }
    for (int64_t i = 0; i < n; i++) {
        if (z[i] < 0 || z[i] >= 120 || b->host.z2s[z[i]] < 0) return fail(c, UF3_ESPECIES, "uf3_mc_create: element outside the basis");
        if (swappable && swappable[i] > 1) return fail(c, UF3_EINVAL, "uf3_mc_create: swappable must hold 0 or 1 per atom");
    }
    HIPCHK(c, hipSetDevice(c->device));
    uf3_mc *m = new uf3_mc();
    m->max_frame = max_frame; m->has_mask = swappable != nullptr;
    m->pos_host.assign(pos, pos + 3 * (size_t)n);
    for (int zz = 0; zz < 120; zz++)
        if (b->host.z2s[zz] >= 0 && b->host.z2s[zz] < UF3_MAX_SPECIES) m->s2z[b->host.z2s[zz]] = zz;
    auto bail = [&](int rc) { uf3_mc_destroy(m); return rc; };
    rc = batch_init(*m, b, fr, nullptr, z, c1, c2, c3, 8, who);     // (mc_build_table uploads the positions)
    if (rc) return bail(rc);
    if ((swappable && m->swappable.ensure((size_t)n)) || m->accepted.ensure(8 * (size_t)nf) || m->trials.ensure(8 * (size_t)nf) ||
        m->status.ensure(4 * (size_t)nf) || m->kT.ensure(8 * (size_t)nf) || m->c1d.ensure(8 * m->c1.size()) ||
        m->c2d.ensure(8 * m->c2.size()) || m->c3d.ensure(8 * m->c3.size()))
        return bail(fail(c, UF3_ENOMEM, "uf3_mc_create: out of device memory"));
    hipStream_t s = c->stream;
    if ((swappable && hipMemcpyAsync(m->swappable.p, swappable, (size_t)n, hipMemcpyHostToDevice, s)) ||
        hipMemsetAsync(m->energies.p, 0, 8 * (size_t)nf, s) || hipMemsetAsync(m->accepted.p, 0, 8 * (size_t)nf, s) ||
        hipMemsetAsync(m->trials.p, 0, 8 * (size_t)nf, s) || hipMemsetAsync(m->status.p, 0, 4 * (size_t)nf, s) ||
        hipMemcpyAsync(m->c1d.p, m->c1.data(), 8 * m->c1.size(), hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(m->c2d.p, m->c2.data(), 8 * m->c2.size(), hipMemcpyHostToDevice, s) ||
        hipMemcpyAsync(m->c3d.p, m->c3.data(), 8 * m->c3.size(), hipMemcpyHostToDevice, s) || hipStreamSynchronize(s))
        return bail(fail(c, UF3_EHIP, "uf3_mc_create: upload failed"));
    rc = mc_build_table(m, who);
    if (rc) return bail(rc);
    *out = m;
    return UF3_OK;
}

// the evaluator's energies of the current species at the current positions, when the running energies do not describe them
static int mc_energies(uf3_mc *m) {
    if (m->energy_valid) return UF3_OK;
    const int rc = batch_eval(*m, nullptr, nullptr);
    if (rc) return rc;
    m->energy_valid = true;
    return UF3_OK;
}

static McModel mc_model(const uf3_mc *m) {
    McModel M;
    M.B = m->b->dev; M.c1 = m->c1d.as<double>(); M.c2 = m->c2d.as<double>(); M.c3 = m->c3d.as<double>();
    M.S = m->b->host.S; M.T = m->b->host.T;
    return M;
}

static McTable mc_table(const uf3_mc *m) {
    McTable t;
    t.off2 = m->off2.as<long long>(); t.off3 = m->off3.as<long long>(); t.ent2 = m->ent2.as<McEnt2>(); t.ent3 = m->ent3.as<McEnt3>();
    return t;
}

extern "C" int uf3_mc_set_positions(uf3_mc *m, const double *pos) {
    if (!m) return fail(nullptr, UF3_EINVAL, "uf3_mc_set_positions: mc is NULL");
    uf3_ctx *c = m->c;
    if (!pos) return fail(c, UF3_EINVAL, "uf3_mc_set_positions: pos is NULL");
    if (!md_finite(pos, 3 * (size_t)m->natoms)) return fail(c, UF3_EINVAL, "uf3_mc_set_positions: pos must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const std::vector<double> before = m->pos_host;
    m->pos_host.assign(pos, pos + 3 * (size_t)m->natoms);
    const int rc = mc_build_table(m, "uf3_mc_set_positions");
    if (rc) {                                    // (refused: the object keeps its positions and its table)
        const std::string msg = c->err;
        m->pos_host = before;
        mc_build_table(m, "uf3_mc_set_positions");
        return fail(c, rc, msg);
    }
    return UF3_OK;
}

extern "C" int uf3_mc_run(uf3_mc *m, int64_t n_trials, int mode, const double *temperatures_K, const double *mu, uint64_t seed,
                          int64_t record_every, double *records) {
    if (!m) return fail(nullptr, UF3_EINVAL, "uf3_mc_run: mc is NULL");
    uf3_ctx *c = m->c;
    const int nf = m->n_frames, S = m->b->host.S;
    if (n_trials < 0) return fail(c, UF3_EINVAL, "uf3_mc_run: n_trials must be >= 0");
    if (mode != 0 && mode != 1) return fail(c, UF3_EINVAL, "uf3_mc_run: mode must be 0 (swap) or 1 (transmute)");
    if (!temperatures_K) return fail(c, UF3_EINVAL, "uf3_mc_run: temperatures_K is NULL");
    for (int f = 0; f < nf; f++)
        if (!(temperatures_K[f] >= 0.0) || !std::isfinite(temperatures_K[f]))
            return fail(c, UF3_EINVAL, "uf3_mc_run: temperatures must be finite and >= 0");
    if ((mode == 1) != (mu != nullptr)) return fail(c, UF3_EINVAL, "uf3_mc_run: mu goes with mode 1 (transmute), and only with it");
    if (mu)
        for (int s = 0; s < S; s++)
            if (std::isnan(mu[s]) || mu[s] == std::numeric_limits<double>::infinity())
                return fail(c, UF3_EINVAL, "uf3_mc_run: a chemical potential must be finite or -inf (species not allowed)");
    if (record_every < 0) return fail(c, UF3_EINVAL, "uf3_mc_run: record_every must be >= 0");
    if ((record_every > 0) != (records != nullptr))
        return fail(c, UF3_EINVAL, record_every ? "uf3_mc_run: records are due but the records buffer is NULL"
                                                : "uf3_mc_run: a records buffer was given but no record is due");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = mc_energies(m);
    if (rc) return rc;
    hipStream_t s = c->stream;
    std::vector<double> kT(nf);
    for (int f = 0; f < nf; f++) kT[f] = UF3_MD_KB * temperatures_K[f];
    HIPCHK(c, hipMemcpyAsync(m->kT.p, kT.data(), 8 * (size_t)nf, hipMemcpyHostToDevice, s));
    const int width = 3 + S;
    const int64_t n_rec = record_every ? n_trials / record_every : 0;
    if (n_rec) {
        HIPCHK(c, m->ring.ensure(8 * (size_t)n_rec * nf * width));
        HIPCHK(c, hipMemsetAsync(m->ring.p, 0, 8 * (size_t)n_rec * nf * width, s));
    }
    McTrialArgs A;
    A.M = mc_model(m); A.tb = mc_table(m);
    A.offsets = m->offsets_dev.as<long long>(); A.z = m->z.as<int32_t>();
    A.swappable = m->has_mask ? m->swappable.as<uint8_t>() : nullptr;
    A.energy = m->energies.as<double>(); A.accepted = m->accepted.as<long long>(); A.trials = m->trials.as<long long>();
    A.status = m->status.as<int>(); A.kT = m->kT.as<double>();
    for (int q = 0; q < UF3_MAX_SPECIES; q++) { A.mu[q] = (mu && q < S) ? mu[q] : 0.0; A.s2z[q] = m->s2z[q]; }
    A.mode = mode; A.seed = seed; A.rec_every = record_every; A.records = n_rec ? m->ring.as<double>() : nullptr; A.n_frames = nf;
    const size_t lds = ((size_t)m->max_frame + 15) & ~(size_t)15;
    // a launch is a bounded block of trials; the blocks of a run queue up on the stream
    for (int64_t done = 0; done < n_trials; done += UF3_MC_BLOCK_TRIALS) {
        A.t0 = m->trial + (uint64_t)done; A.run_done = done;
        A.n_trials = (int)std::min<int64_t>(UF3_MC_BLOCK_TRIALS, n_trials - done);
        hipLaunchKernelGGL(k_mc_trials, dim3((unsigned)nf), dim3(UF3_MC_THREADS), lds, s, A);
        HIPCHK(c, hipGetLastError());
    }
    if (n_rec) HIPCHK(c, hipMemcpyAsync(records, m->ring.p, 8 * (size_t)n_rec * nf * width, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    m->trial += (uint64_t)n_trials;
    if (n_rec) {
        // a frame frozen inside the run wrote no later record: its rows repeat the last one written (trials > 0 marks a written row)
        for (int f = 0; f < nf; f++)
            for (int64_t k = 1; k < n_rec; k++) {
                double *row = records + ((size_t)k * nf + f) * width;
                if (row[2] == 0.0) memcpy(row, row - (size_t)nf * width, 8 * (size_t)width);
            }
    }
    return UF3_OK;
}

extern "C" int uf3_mc_delta(uf3_mc *m, int64_t n, const int32_t *frame, const int32_t *i, const int32_t *j_or_species, int mode,
                            double *dE) {
    if (!m) return fail(nullptr, UF3_EINVAL, "uf3_mc_delta: mc is NULL");
    uf3_ctx *c = m->c;
    if (n < 0 || n >= (1LL << 30)) return fail(c, UF3_EINVAL, "uf3_mc_delta: n must lie in 0 .. 2^30");
    if (mode != 0 && mode != 1) return fail(c, UF3_EINVAL, "uf3_mc_delta: mode must be 0 (swap) or 1 (transmute)");
    if (n == 0) return UF3_OK;
    if (!frame || !i || !j_or_species || !dE) return fail(c, UF3_EINVAL, "uf3_mc_delta: null argument");
    std::vector<int32_t> prop(3 * (size_t)n);
    for (int64_t q = 0; q < n; q++) {
        if (frame[q] < 0 || frame[q] >= m->n_frames) return fail(c, UF3_EINVAL, "uf3_mc_delta: frame outside the batch");
        const int64_t nfr = m->offsets[frame[q] + 1] - m->offsets[frame[q]];
        if (i[q] < 0 || i[q] >= nfr) return fail(c, UF3_EINVAL, "uf3_mc_delta: atom i outside its frame");
        int32_t second = j_or_species[q];
        if (mode == 0) {
            if (second < 0 || second >= nfr) return fail(c, UF3_EINVAL, "uf3_mc_delta: atom j outside its frame");
        } else {
            if (second < 0 || second >= 120 || m->b->host.z2s[second] < 0) return fail(c, UF3_ESPECIES, "uf3_mc_delta: element outside the basis");
            second = m->b->host.z2s[second];
        }
        prop[q] = frame[q]; prop[n + q] = i[q]; prop[2 * n + q] = second;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, m->prop.ensure(12 * (size_t)n));
    HIPCHK(c, m->dE.ensure(8 * (size_t)n));
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(m->prop.p, prop.data(), 12 * (size_t)n, hipMemcpyHostToDevice, s));
    McDeltaArgs A;
    A.M = mc_model(m); A.tb = mc_table(m);
    A.offsets = m->offsets_dev.as<long long>(); A.z = m->z.as<int32_t>();
    A.frame = m->prop.as<int32_t>(); A.i = A.frame + n; A.j = A.frame + 2 * n;
    A.mode = mode; A.dE = m->dE.as<double>();
    const size_t lds = ((size_t)m->max_frame + 15) & ~(size_t)15;
    hipLaunchKernelGGL(k_mc_delta, dim3((unsigned)n), dim3(UF3_MC_THREADS), lds, s, A);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dE, m->dE.p, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return UF3_OK;
}

extern "C" int uf3_mc_get_state(uf3_mc *m, int32_t *z, double *energies, int64_t *accepted, int64_t *trials, int32_t *status) {
    if (!m) return fail(nullptr, UF3_EINVAL, "uf3_mc_get_state: mc is NULL");
    uf3_ctx *c = m->c;
    HIPCHK(c, hipSetDevice(c->device));
    if (energies) {
        const int rc = mc_energies(m);
        if (rc) return rc;
    }
    hipStream_t s = c->stream;
    const size_t nf = (size_t)m->n_frames;
    if (z) HIPCHK(c, hipMemcpyAsync(z, m->z.p, 4 * (size_t)m->natoms, hipMemcpyDeviceToHost, s));
    if (energies) HIPCHK(c, hipMemcpyAsync(energies, m->energies.p, 8 * nf, hipMemcpyDeviceToHost, s));
    if (accepted) HIPCHK(c, hipMemcpyAsync(accepted, m->accepted.p, 8 * nf, hipMemcpyDeviceToHost, s));
    if (trials) HIPCHK(c, hipMemcpyAsync(trials, m->trials.p, 8 * nf, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(c, hipMemcpyAsync(status, m->status.p, 4 * nf, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ per-atom image lists (hess_lists_atom, k_flux_lists)
// What the Hessian, the site terms / heat current and an MD state's flux samples are computed from.  lists_prepare: what does
// not change while the atoms move (frame table, species, the model's copy); lists_longest: the count pass; lists_fill: the
// entries at the workspace's capacity, which the caller derives from the longest list.
// the list geometry of one frame: lattice rows (zero on a non-periodic axis), the inverse of the completed cell, and the
// images tried per side around the nearest one
static int hess_geometry(uf3_ctx *c, const uf3_basis *b, const double *cells, const uint8_t *pbc, const char *who, double *cell_out,
                         double *inv_out, int *per_out, int *nimg_out) {
    // cell: the periodic rows as given; a non-periodic axis gets a unit vector orthogonal to what is there already, so that the
    // fractional coordinates along the periodic axes bound the image distance whatever the other rows hold
    double cell[9], comp[9];
    for (int k = 0; k < 9; k++) cell[k] = cells[k];
    int per[3];
    for (int k = 0; k < 3; k++) per[k] = pbc[k] ? 1 : 0;
    {
        std::vector<std::array<double, 3>> basis_v;
        for (int k = 0; k < 3; k++) if (per[k]) basis_v.push_back({cell[3 * k], cell[3 * k + 1], cell[3 * k + 2]});
        for (int k = 0; k < 3; k++) {
            if (per[k]) { for (int q = 0; q < 3; q++) comp[3 * k + q] = cell[3 * k + q]; continue; }
            // orthonormal complement: the unit axis with the largest remainder after removing the span so far
            std::array<double, 3> best = {0, 0, 0};
            double best_n = -1;
            for (int e = 0; e < 3; e++) {
                std::array<double, 3> v = {0, 0, 0};
                v[e] = 1.0;
                std::vector<std::array<double, 3>> ortho;
                for (auto w : basis_v) {
                    for (auto &o : ortho) { double t = w[0] * o[0] + w[1] * o[1] + w[2] * o[2]; for (int q = 0; q < 3; q++) w[q] -= t * o[q]; }
                    double nn = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
                    if (nn > 0) { for (int q = 0; q < 3; q++) w[q] /= nn; ortho.push_back(w); }
                }
                for (auto &o : ortho) { double t = v[0] * o[0] + v[1] * o[1] + v[2] * o[2]; for (int q = 0; q < 3; q++) v[q] -= t * o[q]; }
                double nn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                if (nn > best_n) { best_n = nn; for (int q = 0; q < 3; q++) best[q] = v[q] / nn; }
            }
            basis_v.push_back(best);
            for (int q = 0; q < 3; q++) comp[3 * k + q] = best[q];
        }
    }
    double inv[9];
    if (!invert3(comp, inv)) return fail(c, UF3_EINVAL, std::string(who) + ": singular cell");
    const double reach = std::max(b->host.rmax2, b->host.T > 0 ? b->host.rmax3 : 0.0);
    for (int k = 0; k < 9; k++) { cell_out[k] = per[k / 3] ? cell[k] : 0.0; inv_out[k] = inv[k]; }
    for (int k = 0; k < 3; k++) {
        per_out[k] = per[k];
        // |image distance| >= h_k |f_k + s_k| with h_k = 1 / |column k of inv|: |s_k| <= reach / h_k + 1/2 around the nearest image
        const double h = 1.0 / std::sqrt(inv[k] * inv[k] + inv[3 + k] * inv[3 + k] + inv[6 + k] * inv[6 + k]);
        nimg_out[k] = per[k] ? (int)std::floor(reach / h + 0.5 + 1e-6) : 0;
        if (nimg_out[k] > 64) return fail(c, UF3_EINVAL, std::string(who) + ": cell far thinner than the cut-off");
    }
    return UF3_OK;
}

// Fills F with everything but the positions and the outputs.  what: "frame" or "batch", for the species message.  model = false
// (site rows and grades: they take no coefficients): c1 / c2 / c3 are not looked at and F's stay null.
static int lists_prepare(uf3_basis *b, const uf3_frames *fr, ListWork &W, const int32_t *d_z, const double *c1, const double *c2,
                         const double *c3, const char *who, const char *what, FluxArgs &F, bool model) {
    uf3_ctx *c = b->ctx;
    const std::string me(who);
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || !fr->cells || !fr->pbc) return fail(c, UF3_EINVAL, me + ": bad uf3_frames");
    if (!d_z || (model && !c1)) return fail(c, UF3_EINVAL, me + ": null argument");
    if (model && ((b->c2_len && !c2) || (b->c3_len && !c3))) return fail(c, UF3_EINVAL, me + ": missing coefficients");
    const int nf = fr->n_frames;
    if (fr->atom_offsets[0] != 0) return fail(c, UF3_EINVAL, me + ": atom_offsets[0] must be 0");
    for (int f = 0; f < nf; f++)
        if (fr->atom_offsets[f + 1] <= fr->atom_offsets[f]) return fail(c, UF3_EINVAL, me + ": every frame needs an atom");
    const int64_t n = fr->atom_offsets[nf];
    if (n > (int64_t)1 << 30) return fail(c, UF3_EINVAL, me + ": bad atom count");
    std::vector<FluxFrame> tab((size_t)nf);
    for (int f = 0; f < nf; f++) {
        FluxFrame &g = tab[f];
        int rc = hess_geometry(c, b, fr->cells + 9 * (size_t)f, fr->pbc + 3 * (size_t)f, who, g.cell, g.inv, g.per, g.nimg);
        if (rc) return rc;
        g.lo = fr->atom_offsets[f];
        g.natoms = (int)(fr->atom_offsets[f + 1] - fr->atom_offsets[f]);
        g.pad = 0;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, W.frames.ensure(sizeof(FluxFrame) * (size_t)nf));
    HIPCHK(c, W.offsets.ensure(8 * (size_t)(nf + 1)));
    HIPCHK(c, W.spec.ensure(sizeof(int) * (size_t)n));
    HIPCHK(c, W.cnt.ensure(sizeof(int) * (size_t)n));
    HIPCHK(c, W.flags.ensure(sizeof(int) * 4));
    // the model: the library's own copy (the evaluator's model cache is left alone)
    const size_t n1 = model ? (size_t)b->host.S : 0, n2 = model ? b->c2_len : 0, n3 = model ? b->c3_len : 0;
    HIPCHK(c, W.coeff.ensure(8 * (n1 + n2 + n3 + 1)));
    double *dc = W.coeff.as<double>();
    // (pageable sources: each copy has left the host buffer when the call returns)
    HIPCHK(c, hipMemcpyAsync(W.frames.p, tab.data(), sizeof(FluxFrame) * (size_t)nf, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(W.offsets.p, fr->atom_offsets, 8 * (size_t)(nf + 1), hipMemcpyHostToDevice, st));
    if (n1) HIPCHK(c, hipMemcpyAsync(dc, c1, 8 * n1, hipMemcpyHostToDevice, st));
    if (n2) HIPCHK(c, hipMemcpyAsync(dc + n1, c2, 8 * n2, hipMemcpyHostToDevice, st));
    if (n3) HIPCHK(c, hipMemcpyAsync(dc + n1 + n2, c3, 8 * n3, hipMemcpyHostToDevice, st));
    int *d_flags = W.flags.as<int>();
    HIPCHK(c, hipMemsetAsync(d_flags, 0, sizeof(int) * 4, st));
    hipLaunchKernelGGL(k_hess_species, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const BasisDev *)b->dev, d_z, (int)n,
                       W.spec.as<int>(), d_flags + 2);
    int bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, d_flags + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (bad) return fail(c, UF3_ESPECIES, me + ": the " + what + " contains an element outside the basis");
    F = FluxArgs();
    F.B = b->dev; F.frames = W.frames.as<FluxFrame>(); F.offsets = W.offsets.as<int64_t>(); F.n_frames = nf; F.n = n;
    F.spec = W.spec.as<int>(); F.cnt = W.cnt.as<int>(); F.flags = d_flags;
    if (model) { F.c1 = dc; F.c2 = dc + n1; F.c3 = dc + n1 + n2; }
    return UF3_OK;
}

// the count pass on F.pos: the longest list of the batch (at least 1)
static int lists_longest(uf3_ctx *c, FluxArgs &F, const char *who, int &longest) {
    hipStream_t st = c->stream;
    const size_t n = (size_t)F.n;
    F.cap = 0; F.ent = nullptr;
    hipLaunchKernelGGL(k_flux_lists<false>, dim3((unsigned)n), dim3(64), 0, st, F);
    std::vector<int> cnt(n);
    int flags[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt.data(), F.cnt, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (flags[0]) return fail(c, UF3_EINVAL, std::string(who) + ": atoms lie more than 500 cells apart along a periodic axis: wrap the positions");
    longest = std::max(1, *std::max_element(cnt.begin(), cnt.end()));
    return UF3_OK;
}

// the fill pass on F.pos at capacity W.cap (every atom: the centres of a row's triplets may lie anywhere in its frame)
static int lists_fill(uf3_ctx *c, ListWork &W, FluxArgs &F) {
    HIPCHK(c, W.ent.ensure(sizeof(HessNbr) * (size_t)F.n * (size_t)W.cap));
    F.cap = W.cap; F.ent = W.ent.as<HessNbr>();
    hipLaunchKernelGGL(k_flux_lists<true>, dim3((unsigned)F.n), dim3(64), 0, c->stream, F);
    return UF3_OK;
}

// ------------------------------------------------------------------------------ analytic Hessian (uf3_hessian.h)
// The one-frame case of the batched lists, sized exactly; the lists live in the context's own workspace (hs), which no other
// entry touches: uf3_hessian_dev returns with k_hessian queued on them.
static int hessian_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *c1,
                        const double *c2, const double *c3, int64_t row_begin, int64_t row_end, double *d_hess, double *d_mixed,
                        double *d_born) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!fr || fr->n_frames != 1 || !fr->atom_offsets || !fr->cells || !fr->pbc)
        return fail(c, UF3_EINVAL, "uf3_hessian: exactly one frame");
    if (!d_pos || !d_z || !c1 || !d_hess) return fail(c, UF3_EINVAL, "uf3_hessian: null argument");
    if ((b->c2_len && !c2) || (b->c3_len && !c3)) return fail(c, UF3_EINVAL, "uf3_hessian: missing coefficients");
    const int64_t N = fr->atom_offsets[1] - fr->atom_offsets[0];
    if (fr->atom_offsets[0] != 0 || N < 1 || N > (int64_t)1 << 30) return fail(c, UF3_EINVAL, "uf3_hessian: bad atom count");
    if (row_begin < 0 || row_end > N || row_begin >= row_end)
        return fail(c, UF3_EINVAL, "uf3_hessian: row span [" + std::to_string(row_begin) + ", " + std::to_string(row_end) +
                                       ") empty or outside the frame's " + std::to_string(N) + " atoms");
    if (d_born && (row_begin != 0 || row_end != N))
        return fail(c, UF3_EINVAL, "uf3_hessian: born needs the whole frame's rows");
    ListWork &W = c->hs;
    FluxArgs F;
    // (the argument checks of lists_prepare cannot fire here: every case was refused above, in the Hessian's own words)
    int rc = lists_prepare(b, fr, W, d_z, c1, c2, c3, "uf3_hessian", "frame", F);
    if (rc) return rc;
    F.pos = d_pos;
    rc = lists_longest(c, F, "uf3_hessian", W.cap);
    if (rc) return rc;
    rc = lists_fill(c, W, F);
    if (rc) return rc;
    hipStream_t st = c->stream;
    HessArgs A = {};      // (geometry and bad stay zero: the list build's, filled per frame by k_flux_lists; k_hessian reads none)
    A.B = b->dev; A.pos = d_pos; A.spec = F.spec; A.natoms = (int)N;
    A.cap = F.cap; A.cnt = F.cnt; A.ent = F.ent; A.c2 = F.c2; A.c3 = F.c3;
    const int64_t R = row_end - row_begin;
    A.row_begin = row_begin; A.row_end = row_end; A.ld = 3 * N;
    A.hess = d_hess; A.mixed = d_mixed;
    HIPCHK(c, hipMemsetAsync(d_hess, 0, sizeof(double) * 9 * (size_t)R * (size_t)N, st));
    if (d_mixed) HIPCHK(c, hipMemsetAsync(d_mixed, 0, sizeof(double) * 18 * (size_t)R, st));
    if (d_born) {
        HIPCHK(c, c->hs_part.ensure(sizeof(double) * 36 * (size_t)R));
        A.born_part = c->hs_part.as<double>();
        HIPCHK(c, hipMemsetAsync(A.born_part, 0, sizeof(double) * 36 * (size_t)R, st));
    }
    hipLaunchKernelGGL(k_hessian, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, st, A);
    if (d_born) hipLaunchKernelGGL(k_hess_born_sum, dim3(36), dim3(256), 0, st, (const double *)A.born_part, (long long)R, d_born);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_hessian_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *c1,
                               const double *c2, const double *c3, int64_t row_begin, int64_t row_end, double *d_hess,
                               double *d_mixed, double *d_born) {
    return hessian_impl(b, fr, d_pos, d_z, c1, c2, c3, row_begin, row_end, d_hess, d_mixed, d_born);
}

extern "C" int uf3_hessian(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                           const double *c2, const double *c3, int64_t row_begin, int64_t row_end, double *hess, double *mixed,
                           double *born) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!fr || fr->n_frames != 1 || !fr->atom_offsets) return fail(c, UF3_EINVAL, "uf3_hessian: exactly one frame");
    if (!pos || !z || !hess) return fail(c, UF3_EINVAL, "uf3_hessian: null argument");
    const int64_t N = fr->atom_offsets[1] - fr->atom_offsets[0];
    if (N < 1 || row_begin < 0 || row_end > N || row_begin >= row_end) return hessian_impl(b, fr, pos, z, c1, c2, c3, row_begin, row_end, hess, mixed, born);
    const size_t R = (size_t)(row_end - row_begin), n = (size_t)N;
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->hs_io, c->stream);
    const int s_pos = S.add(24 * n), s_z = S.add(4 * n), s_h = S.add(72 * R * n), s_m = S.add(144 * R, mixed != nullptr),
              s_b = S.add(36 * 8, born != nullptr);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_pos, pos}, {s_z, z}}));
    int rc = hessian_impl(b, fr, S.at<double>(s_pos), S.at<int32_t>(s_z), c1, c2, c3, row_begin, row_end, S.at<double>(s_h),
                          S.at<double>(s_m), S.at<double>(s_b));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_h, hess}, {s_m, mixed}, {s_b, born}}));
    if (c->hs_io.cap > ((size_t)1 << 30)) c->hs_io.release();      // (a large slab's staging is not kept for the context's lifetime)
    return UF3_OK;
}

// ------------------------------------------------------------------------------ site terms and the heat current (uf3_flux.h)
// lists, k_flux_site_terms, k_flux_frame on device positions (and velocities).  F from lists_prepare, and F.pos, F.vel
// (null: no current), F.mass, F.u (null: the workspace's), F.w (null: no virials), F.flux set by the caller.  headroom: keep
// the capacity between calls (an MD run: sized at the first sample with room to move, grown when a list overflows); without
// it the lists are sized exactly for these positions.
// The lists of F.pos at the workspace's capacity, then launch() (the kernels that walk them; a walk that meets a cut list sets
// flags[1]).  headroom: see flux_sample.  cap_limit / what: the walk's own limit on the capacity and its words for it.
template <class Launch>
static int lists_sample(uf3_ctx *c, ListWork &W, FluxArgs &F, bool headroom, const char *who, int cap_limit, const char *what,
                        Launch launch) {
    hipStream_t st = c->stream;
    const std::string me(who);
    for (int attempt = 0; attempt < 3; attempt++) {
        if (!headroom || W.cap == 0) {
            int longest;
            int rc = lists_longest(c, F, who, longest);
            if (rc) return rc;
            W.cap = headroom ? longest + longest / 4 + 8 : longest;
            if (W.cap > cap_limit) { W.cap = 0; return fail(c, UF3_EINVAL, me + what); }
        }
        int rc = lists_fill(c, W, F);
        if (rc) return rc;
        rc = launch();
        if (rc) return rc;
        HIPCHK(c, hipGetLastError());
        if (!headroom) return UF3_OK;           // (sized for these very positions: nothing can overflow)
        int flags[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(flags, F.flags, sizeof(flags), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (flags[0]) return fail(c, UF3_EINVAL, me + ": atoms lie more than 500 cells apart along a periodic axis: wrap the positions");
        if (!flags[1]) return UF3_OK;
        HIPCHK(c, hipMemsetAsync(F.flags, 0, sizeof(int) * 2, st));
        W.cap = 0;                              // a list was cut: size again from these positions and redo the sample
    }
    return fail(c, UF3_EINVAL, me + ": the neighbour lists keep overflowing");
}

static int flux_sample(uf3_ctx *c, ListWork &W, FluxArgs &F, bool headroom, const char *who) {
    hipStream_t st = c->stream;
    const unsigned n = (unsigned)F.n;
    HIPCHK(c, W.u.ensure(8 * (size_t)n));
    HIPCHK(c, W.jp.ensure(24 * (size_t)n));
    if (!F.u) F.u = W.u.as<double>();
    F.jp = W.jp.as<double>();
    // (k_flux_site_terms' index array, [cap] ints of LDS: its limit, not the lists')
    return lists_sample(c, W, F, headroom, who, 12288, ": more than 12288 neighbours of one atom", [&] {
        const size_t lds = sizeof(int) * (size_t)F.cap;
        const bool want_w = F.w != nullptr, want_j = F.vel != nullptr;
        with_bool(want_w, [&](auto WANT_W) { return with_bool(want_j, [&](auto WANT_J) {
            hipLaunchKernelGGL((k_flux_site_terms<WANT_W, WANT_J>), dim3(n), dim3(64), lds, st, F);
            return (int)UF3_OK; }); });
        if (want_j) hipLaunchKernelGGL(k_flux_frame, dim3((unsigned)F.n_frames), dim3(UF3_MD_THREADS), 0, st, F);
        return (int)UF3_OK;
    });
}

static int site_terms_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const double *d_vel, const int32_t *d_z,
                           const double *d_mass, const double *c1, const double *c2, const double *c3, double *d_u, double *d_w,
                           double *d_flux, const char *who) {
    uf3_ctx *c = b->ctx;
    if (!d_pos) return fail(c, UF3_EINVAL, std::string(who) + ": null argument");
    FluxArgs F;
    int rc = lists_prepare(b, fr, c->fx, d_z, c1, c2, c3, who, "batch", F);
    if (rc) return rc;
    F.pos = d_pos; F.vel = d_vel; F.mass = d_mass; F.u = d_u; F.w = d_w; F.flux = d_flux;
    return flux_sample(c, c->fx, F, false, who);
}

static bool flux_frames_ok(const uf3_frames *fr) {
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets) return false;
    return fr->atom_offsets[fr->n_frames] >= 1 && fr->atom_offsets[fr->n_frames] <= (int64_t)1 << 30;
}

extern "C" int uf3_site_terms_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *c1,
                                  const double *c2, const double *c3, double *d_site_energies, double *d_site_virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (!d_site_energies && !d_site_virials) return fail(b->ctx, UF3_EINVAL, "uf3_site_terms: nothing asked for");
    return site_terms_impl(b, fr, d_pos, nullptr, d_z, nullptr, c1, c2, c3, d_site_energies, d_site_virials, nullptr, "uf3_site_terms");
}

extern "C" int uf3_site_terms(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *c1,
                              const double *c2, const double *c3, double *site_energies, double *site_virials) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!flux_frames_ok(fr)) return fail(c, UF3_EINVAL, "uf3_site_terms: bad uf3_frames");
    if (!pos || !z) return fail(c, UF3_EINVAL, "uf3_site_terms: null argument");
    if (!site_energies && !site_virials) return fail(c, UF3_EINVAL, "uf3_site_terms: nothing asked for");
    const size_t n = (size_t)fr->atom_offsets[fr->n_frames];
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->fx.io, c->stream);
    // (the energies' section is there whether or not they are asked for: the kernel writes them either way)
    const int s_pos = S.add(24 * n), s_z = S.add(4 * n), s_u = S.add(8 * n), s_w = S.add(72 * n, site_virials != nullptr);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_pos, pos}, {s_z, z}}));
    int rc = site_terms_impl(b, fr, S.at<double>(s_pos), nullptr, S.at<int32_t>(s_z), nullptr, c1, c2, c3, S.at<double>(s_u),
                             S.at<double>(s_w), nullptr, "uf3_site_terms");
    if (rc) return rc;
    HIPCHK(c, S.out({{s_u, site_energies}, {s_w, site_virials}}));
    return UF3_OK;
}

extern "C" int uf3_heat_flux_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const double *d_vel, const int32_t *d_z,
                                 const double *d_masses, const double *c1, const double *c2, const double *c3, double *d_flux,
                                 double *d_site_energies) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    if (!d_vel || !d_masses || !d_flux) return fail(b->ctx, UF3_EINVAL, "uf3_heat_flux: null argument");
    return site_terms_impl(b, fr, d_pos, d_vel, d_z, d_masses, c1, c2, c3, d_site_energies, nullptr, d_flux, "uf3_heat_flux");
}

extern "C" int uf3_heat_flux(uf3_basis *b, const uf3_frames *fr, const double *pos, const double *vel, const int32_t *z,
                             const double *masses, const double *c1, const double *c2, const double *c3, double *flux,
                             double *site_energies) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!flux_frames_ok(fr)) return fail(c, UF3_EINVAL, "uf3_heat_flux: bad uf3_frames");
    if (!pos || !vel || !z || !masses || !flux) return fail(c, UF3_EINVAL, "uf3_heat_flux: null argument");
    const size_t n = (size_t)fr->atom_offsets[fr->n_frames], nf = (size_t)fr->n_frames;
    for (size_t i = 0; i < n; i++)
        if (!(masses[i] > 0.0) || !std::isfinite(masses[i])) return fail(c, UF3_EINVAL, "uf3_heat_flux: masses must be positive and finite");
    if (!md_finite(vel, 3 * n)) return fail(c, UF3_EINVAL, "uf3_heat_flux: velocities must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->fx.io, c->stream);
    const int s_pos = S.add(24 * n), s_vel = S.add(24 * n), s_z = S.add(4 * n), s_m = S.add(8 * n), s_u = S.add(8 * n),
              s_f = S.add(48 * nf);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_pos, pos}, {s_vel, vel}, {s_z, z}, {s_m, masses}}));
    int rc = site_terms_impl(b, fr, S.at<double>(s_pos), S.at<double>(s_vel), S.at<int32_t>(s_z), S.at<double>(s_m), c1, c2, c3,
                             S.at<double>(s_u), nullptr, S.at<double>(s_f), "uf3_heat_flux");
    if (rc) return rc;
    HIPCHK(c, S.out({{s_f, flux}, {s_u, site_energies}}));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ site rows and grades (uf3_site_rows.h)
#define SITE_ROWS_LDS SG_LDS_BUDGET                // k_site_rows: row + index array; as k_site_grade, two workgroups per CU (a row of
                                                   // eight species' notebook basis, F = 8164, takes 65 552 bytes)
#define SITE_CHUNK_BYTES ((size_t)64 << 20)        // the fall-back's chunk of rows

// k_site_rows on centres [m0, m1) of the lists in F
static void site_rows_launch(uf3_ctx *c, const FluxArgs &F, int n_feat, long long m0, long long m1, double *d_rows, int64_t ld) {
    SiteArgs A = {};
    A.F = F; A.m0 = m0; A.m1 = m1; A.n_feat = n_feat; A.rows = d_rows; A.ld = ld;
    const size_t lds = 8 * (size_t)site_row_stride(n_feat) + 4 * (size_t)F.cap;
    hipLaunchKernelGGL(k_site_rows, dim3((unsigned)(m1 - m0)), dim3(64), lds, c->stream, A);
}
static int site_rows_cap_limit(int n_feat) { return (SITE_ROWS_LDS - 8 * site_row_stride(n_feat)) / 4; }

static int site_rows_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, double *d_rows, int64_t ld) {
    uf3_ctx *c = b->ctx;
    const int n_feat = b->host.F;
    if (!d_pos || !d_rows) return fail(c, UF3_EINVAL, "uf3_site_rows: null argument");
    if (ld < n_feat) return fail(c, UF3_EINVAL, "uf3_site_rows: ld must be >= n_feat");
    if (site_rows_cap_limit(n_feat) < 1) return fail(c, UF3_EINVAL, "uf3_site_rows: a row of this basis does not fit in LDS");
    HIPCHK(c, lds_opt_in<k_site_rows>(c->device, SITE_ROWS_LDS));       // (its whole budget, before the first launch)
    FluxArgs F;
    int rc = lists_prepare(b, fr, c->fx, d_z, nullptr, nullptr, nullptr, "uf3_site_rows", "batch", F, false);
    if (rc) return rc;
    F.pos = d_pos;
    return lists_sample(c, c->fx, F, false, "uf3_site_rows", site_rows_cap_limit(n_feat),
                        ": an atom has more neighbours than fit in LDS beside its row", [&] {
        site_rows_launch(c, F, n_feat, 0, F.n, d_rows, ld);
        return (int)UF3_OK;
    });
}

extern "C" int uf3_site_rows_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, double *d_rows, int64_t ld) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return site_rows_impl(b, fr, d_pos, d_z, d_rows, ld);
}

extern "C" int uf3_site_rows(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, double *rows, int64_t ld) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!flux_frames_ok(fr)) return fail(c, UF3_EINVAL, "uf3_site_rows: bad uf3_frames");
    if (!pos || !z || !rows) return fail(c, UF3_EINVAL, "uf3_site_rows: null argument");
    if (ld < b->host.F) return fail(c, UF3_EINVAL, "uf3_site_rows: ld must be >= n_feat");
    const size_t n = (size_t)fr->atom_offsets[fr->n_frames], F = (size_t)b->host.F;
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->fx.io, c->stream);
    const int s_pos = S.add(24 * n), s_z = S.add(4 * n), s_r = S.add(8 * n * F);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_pos, pos}, {s_z, z}}));
    int rc = site_rows_impl(b, fr, S.at<double>(s_pos), S.at<int32_t>(s_z), S.at<double>(s_r), (int64_t)F);
    if (rc) return rc;
    // (the caller's padding columns F .. ld are not written: a strided copy of the F used ones)
    HIPCHK(c, hipMemcpy2DAsync(rows, 8 * (size_t)ld, S.at<double>(s_r), 8 * F, 8 * F, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->fx.io.cap > ((size_t)1 << 30)) c->fx.io.release();
    return UF3_OK;
}

// The grades of the lists' batch: F from lists_prepare with F.pos set.  d_offsets: the frames the maxima are taken over
// ([n_out + 1] on the device); the other outputs as k_site_frame_max's.  Fused (k_site_grade) where the tile and the four index
// arrays fit SG_LDS_BUDGET at the lists' capacity; otherwise chunks of k_site_rows into the context's scratch + k_leverage.
// after(): queued behind the sample's kernels and in front of the sample's one synchronisation (headroom), or nullptr.
static int site_grade_sample(uf3_basis *b, ListWork &W, FluxArgs &F, bool headroom, const char *who, const double *d_w,
                             double *d_grade, const int64_t *d_offsets, int n_out, double *d_fmax, int32_t *d_fargmax,
                             double *d_pair, const std::function<int()> &after) {
    uf3_ctx *c = b->ctx;
    const int n_feat = b->host.F;
    int rc = ensure_frag(c);
    if (rc) return rc;
    HIPCHK(c, lds_opt_in<k_site_grade>(c->device, SG_LDS_BUDGET));      // (the kernels' whole budgets, before their first launches)
    HIPCHK(c, lds_opt_in<k_site_rows>(c->device, SITE_ROWS_LDS));
    if (site_rows_cap_limit(n_feat) < 1) return fail(c, UF3_EINVAL, std::string(who) + ": a row of this basis does not fit in LDS");
    hipStream_t st = c->stream;
    return lists_sample(c, W, F, headroom, who, site_rows_cap_limit(n_feat), ": an atom has more neighbours than fit in LDS beside its row", [&] {
        const size_t lds = site_grade_lds(n_feat, F.cap);
        const bool fused = lds <= SG_LDS_BUDGET;
        if (fused) {
            SiteArgs A = {};
            A.F = F; A.m0 = 0; A.m1 = F.n; A.n_feat = n_feat; A.w = d_w; A.frag = c->frag.as<int>(); A.grade = d_grade;
            hipLaunchKernelGGL(k_site_grade, dim3((unsigned)((F.n + SG_TILE - 1) / SG_TILE)), dim3(256), lds, st, A);
        } else {
            // whole leverage tiles per chunk; the scratch does not grow with the batch
            long long chunk = (long long)(SITE_CHUNK_BYTES / (8 * (size_t)n_feat)) / LV_ROWS * LV_ROWS;
            chunk = std::max<long long>(LV_ROWS, std::min<long long>(chunk, (F.n + LV_ROWS - 1) / LV_ROWS * LV_ROWS));
            HIPCHK(c, c->site_rows_ws.ensure(8 * (size_t)chunk * n_feat));
            for (long long m0 = 0; m0 < F.n; m0 += chunk) {
                const long long m1 = std::min<long long>(F.n, m0 + chunk);
                site_rows_launch(c, F, n_feat, m0, m1, c->site_rows_ws.as<double>(), n_feat);
                int rl = uf3_leverage_dev(c, c->site_rows_ws.as<double>(), m1 - m0, n_feat, n_feat, d_w, 1, d_grade + m0);
                if (rl) return rl;
            }
        }
        if (c->env_debug_lds)
            fprintf(stderr, "uf3: site grade kernel=%s atoms=%lld feat=%d cap=%d tile=%d lds=%zu B budget=%d B\n",
                    fused ? "k_site_grade" : "k_site_rows+k_leverage", (long long)F.n, n_feat, F.cap, SG_TILE, lds, (int)SG_LDS_BUDGET);
        if (d_fmax || d_fargmax || d_pair)
            hipLaunchKernelGGL(k_site_frame_max, dim3((unsigned)n_out), dim3(256), 0, st, (const double *)d_grade, d_offsets, d_fmax,
                               d_fargmax, d_pair);
        return after ? after() : (int)UF3_OK;
    });
}

// The caller's frames may hold empty ones (0 and -1 for them): the lists are built for the others.
static int site_grade_impl(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *d_w,
                           double *d_grade, double *d_fmax, int32_t *d_fargmax) {
    uf3_ctx *c = b->ctx;
    const char *who = "uf3_site_grade";
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || !fr->cells || !fr->pbc) return fail(c, UF3_EINVAL, "uf3_site_grade: bad uf3_frames");
    if (!d_w) return fail(c, UF3_EINVAL, "uf3_site_grade: null argument (w)");
    const int nf = fr->n_frames;
    if (fr->atom_offsets[0] != 0) return fail(c, UF3_EINVAL, "uf3_site_grade: atom_offsets[0] must be 0");
    for (int f = 0; f < nf; f++)
        if (fr->atom_offsets[f + 1] < fr->atom_offsets[f]) return fail(c, UF3_EINVAL, "uf3_site_grade: atom_offsets must not decrease");
    const int64_t n = fr->atom_offsets[nf];
    if (n && (!d_pos || !d_z || !d_grade)) return fail(c, UF3_EINVAL, "uf3_site_grade: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->site_off.ensure(8 * (size_t)(nf + 1)));
    HIPCHK(c, hipMemcpyAsync(c->site_off.p, fr->atom_offsets, 8 * (size_t)(nf + 1), hipMemcpyHostToDevice, c->stream));
    if (n == 0) {
        if (d_fmax || d_fargmax)
            hipLaunchKernelGGL(k_site_frame_max, dim3((unsigned)nf), dim3(256), 0, c->stream, (const double *)nullptr,
                               (const int64_t *)c->site_off.as<int64_t>(), d_fmax, d_fargmax, (double *)nullptr);
        HIPCHK(c, hipStreamSynchronize(c->stream));        // (the offsets' pageable source)
        return UF3_OK;
    }
    std::vector<int64_t> off(1, 0);
    std::vector<double> cells;
    std::vector<uint8_t> pbc;
    for (int f = 0; f < nf; f++) {
        if (fr->atom_offsets[f + 1] == fr->atom_offsets[f]) continue;
        off.push_back(fr->atom_offsets[f + 1]);
        cells.insert(cells.end(), fr->cells + 9 * (size_t)f, fr->cells + 9 * (size_t)f + 9);
        pbc.insert(pbc.end(), fr->pbc + 3 * (size_t)f, fr->pbc + 3 * (size_t)f + 3);
    }
    uf3_frames live = *fr;
    live.n_frames = (int)off.size() - 1; live.atom_offsets = off.data(); live.cells = cells.data(); live.pbc = pbc.data();
    FluxArgs F;
    int rc = lists_prepare(b, &live, c->fx, d_z, nullptr, nullptr, nullptr, who, "batch", F, false);   // (synchronises: the offsets have left)
    if (rc) return rc;
    F.pos = d_pos;
    return site_grade_sample(b, c->fx, F, false, who, d_w, d_grade, c->site_off.as<int64_t>(), nf, d_fmax, d_fargmax, nullptr, nullptr);
}

extern "C" int uf3_site_grade_dev(uf3_basis *b, const uf3_frames *fr, const double *d_pos, const int32_t *d_z, const double *d_w,
                                  double *d_grade, double *d_frame_max, int32_t *d_frame_argmax) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    return site_grade_impl(b, fr, d_pos, d_z, d_w, d_grade, d_frame_max, d_frame_argmax);
}

extern "C" int uf3_site_grade(uf3_basis *b, const uf3_frames *fr, const double *pos, const int32_t *z, const double *w, double *grade,
                              double *frame_max, int32_t *frame_argmax) {
    if (!b) return fail(nullptr, UF3_EINVAL, "null basis");
    uf3_ctx *c = b->ctx;
    if (!fr || fr->n_frames < 1 || !fr->atom_offsets || fr->atom_offsets[fr->n_frames] < 0 || fr->atom_offsets[fr->n_frames] > (int64_t)1 << 30)
        return fail(c, UF3_EINVAL, "uf3_site_grade: bad uf3_frames");
    if (!w) return fail(c, UF3_EINVAL, "uf3_site_grade: null argument (w)");
    const size_t n = (size_t)fr->atom_offsets[fr->n_frames], nf = (size_t)fr->n_frames, F = (size_t)b->host.F;
    if (n && (!pos || !z || !grade)) return fail(c, UF3_EINVAL, "uf3_site_grade: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->fx.io, c->stream);
    const int s_pos = S.add(24 * n), s_z = S.add(4 * n), s_w = S.add(8 * F * F), s_g = S.add(8 * n), s_m = S.add(8 * nf, frame_max != nullptr),
              s_a = S.add(4 * nf, frame_argmax != nullptr);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_pos, pos}, {s_z, z}, {s_w, w}}));
    int rc = site_grade_impl(b, fr, S.at<double>(s_pos), S.at<int32_t>(s_z), S.at<double>(s_w), S.at<double>(s_g), S.at<double>(s_m),
                             S.at<int32_t>(s_a));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_g, grade}, {s_m, frame_max}, {s_a, frame_argmax}}));
    return UF3_OK;
}

// ------------------------------------------------------------------------------ phonons on a q-mesh (uf3_phonon.h)
// the eigenvector entry's extras: the cell (host, [3][3], only looked at with d_gvel), the velocity cut-off, the two outputs
struct PhVecOut { const double *cell; double cutoff; double *d_evec, *d_gvel; };

static int phonon_mesh_impl(uf3_ctx *c, int32_t n_atoms, int64_t n_sc, const double *d_fc, const double *d_ism, int64_t n_terms,
                            const int32_t *terms, const double *term_w, int64_t nq, const double *d_q, double *d_lam,
                            int32_t *d_status, const PhVecOut *vec = nullptr) {
    const std::string who = vec ? "uf3_phonon_mesh_vec: " : "uf3_phonon_mesh: ";
    if (!c) return fail(nullptr, UF3_EINVAL, who + "ctx is NULL");
    if (n_atoms < 1) return fail(c, UF3_EINVAL, who + "no atoms");
    if (n_atoms > PH_MAX_ATOMS)
        return fail(c, UF3_EINVAL, who + "" + std::to_string(n_atoms) + " atoms in the cell, the limit is " +
                                       std::to_string(PH_MAX_ATOMS) + " (D(q), 16 (3N)^2 bytes, is held in LDS)");
    if (vec && n_atoms > PH_VEC_MAX_ATOMS)
        return fail(c, UF3_EINVAL, who + std::to_string(n_atoms) + " atoms in the cell, the limit with eigenvectors is " +
                                       std::to_string(PH_VEC_MAX_ATOMS) + " (V is held beside D(q) in LDS, 32 (3N)^2 bytes)");
    if (nq < 1 || nq > (int64_t)1 << 30) return fail(c, UF3_EINVAL, who + "nq must be in [1, 2^30]");
    if (n_sc < n_atoms || n_sc % n_atoms || n_sc > (int64_t)1 << 24)
        return fail(c, UF3_EINVAL, who + "the supercell's atom count must be a multiple of the cell's");
    if (n_terms < 1 || n_terms > (int64_t)1 << 28) return fail(c, UF3_EINVAL, who + "n_terms must be in [1, 2^28]");
    if (!d_fc || !d_ism || !terms || !term_w || !d_q || !d_lam || !d_status)
        return fail(c, UF3_EINVAL, who + "null argument");
    if (vec) {
        if (!vec->d_evec && !vec->d_gvel) return fail(c, UF3_EINVAL, who + "neither output asked for (evec and gvel both NULL)");
        if (vec->d_gvel) {
            if (!vec->cell) return fail(c, UF3_EINVAL, who + "group velocities need the cell");
            const double *h = vec->cell;
            const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
            bool finite = std::isfinite(det);
            for (int k = 0; k < 9; k++) finite = finite && std::isfinite(h[k]);
            if (!finite || det == 0.0) return fail(c, UF3_EINVAL, who + "the cell must be finite and not singular");
            if (!(vec->cutoff >= 0.0) || !std::isfinite(vec->cutoff)) return fail(c, UF3_EINVAL, who + "the cut-off must be finite and not negative");
        }
    }
    const int N = n_atoms, nb = N * N;
    // stable counting sort of the terms by block (i, p mod N)
    std::vector<int> off((size_t)nb + 1, 0);
    for (int64_t e = 0; e < n_terms; e++) {
        const int32_t *t = terms + 5 * e;
        if (t[0] < 0 || t[0] >= N || t[1] < 0 || t[1] >= n_sc)
            return fail(c, UF3_EINVAL, who + "term " + std::to_string(e) + " names atom (" + std::to_string(t[0]) + ", " +
                                           std::to_string(t[1]) + ") outside the cell's " + std::to_string(N) + " or the supercell's " +
                                           std::to_string(n_sc) + " atoms");
        if (std::abs(t[2]) > (1 << 20) || std::abs(t[3]) > (1 << 20) || std::abs(t[4]) > (1 << 20) || !std::isfinite(term_w[e]))
            return fail(c, UF3_EINVAL, who + "term " + std::to_string(e) + " has a lattice vector beyond 2^20 cells or a weight that is not finite");
        off[(size_t)t[0] * N + t[1] % N + 1]++;
    }
    for (int k = 0; k < nb; k++) off[k + 1] += off[k];
    const size_t b_t = sizeof(PhTerm) * (size_t)n_terms, b_w = 8 * (size_t)n_terms, b_o = (4 * ((size_t)nb + 1) + 15) / 16 * 16;
    c->ph_stage.resize(b_t + b_w + b_o);
    PhTerm *ht = (PhTerm *)c->ph_stage.data();
    double *hw = (double *)(c->ph_stage.data() + b_t);
    {
        std::vector<int> cur(off.begin(), off.end() - 1);
        for (int64_t e = 0; e < n_terms; e++) {
            const int32_t *t = terms + 5 * e;
            const int at = cur[(size_t)t[0] * N + t[1] % N]++;
            ht[at].p = t[1]; ht[at].n0 = t[2]; ht[at].n1 = t[3]; ht[at].n2 = t[4];
            hw[at] = term_w[e];
        }
    }
    memcpy(c->ph_stage.data() + b_t + b_w, off.data(), 4 * ((size_t)nb + 1));
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, c->ph_ws.ensure(c->ph_stage.size()));
    char *ws = c->ph_ws.as<char>();
    HIPCHK(c, hipMemcpyAsync(ws, c->ph_stage.data(), c->ph_stage.size(), hipMemcpyHostToDevice, st));
    PhMeshArgs A;
    A.fc = d_fc; A.inv_sqrt_mass = d_ism; A.terms = (const PhTerm *)ws; A.term_w = (const double *)(ws + b_t);
    A.block_off = (const int *)(ws + b_t + b_w); A.q = d_q; A.lam = d_lam; A.status = d_status;
    A.nq = nq; A.ld = 3 * n_sc; A.natoms = N;
    A.evec = vec ? vec->d_evec : nullptr; A.gvel = vec ? vec->d_gvel : nullptr; A.cutoff = vec ? vec->cutoff : 0.0;
    for (int k = 0; k < 9; k++) A.cell[k] = vec && vec->d_gvel ? vec->cell[k] : 0.0;
    uf3_env_refresh();
    const bool force_wave = uf3_env("UF3_PHONON_WAVE") != nullptr;      // measurements: the wave-per-q kernel at 3N <= 6 as well
    if (N <= 2 && !force_wave) {
        const unsigned g = (unsigned)((nq + 63) / 64);
        if (vec && N == 1) hipLaunchKernelGGL((k_ph_mesh_lane<1, true>), dim3(g), dim3(64), 0, st, A);
        else if (vec) hipLaunchKernelGGL((k_ph_mesh_lane<2, true>), dim3(g), dim3(64), 0, st, A);
        else if (N == 1) hipLaunchKernelGGL(k_ph_mesh_lane<1>, dim3(g), dim3(64), 0, st, A);
        else hipLaunchKernelGGL(k_ph_mesh_lane<2>, dim3(g), dim3(64), 0, st, A);
    } else if (vec) {
        const size_t lds = ph_wave_lds(3 * N, true);
        if (lds > 65536) HIPCHK(c, lds_opt_in<k_ph_mesh_wave<true>>(c->device, lds));
        hipLaunchKernelGGL(k_ph_mesh_wave<true>, dim3((unsigned)nq), dim3(64), lds, st, A);
    } else {
        const size_t lds = ph_wave_lds(3 * N);
        if (lds > 65536) HIPCHK(c, lds_opt_in<k_ph_mesh_wave<false>>(c->device, lds));
        hipLaunchKernelGGL(k_ph_mesh_wave<false>, dim3((unsigned)nq), dim3(64), lds, st, A);
    }
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_phonon_mesh_dev(uf3_ctx *c, int32_t n_atoms, int64_t n_sc_atoms, const double *d_fc, const double *d_inv_sqrt_mass,
                                   int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *d_q,
                                   double *d_lam, int32_t *d_status) {
    return phonon_mesh_impl(c, n_atoms, n_sc_atoms, d_fc, d_inv_sqrt_mass, n_terms, terms, term_w, nq, d_q, d_lam, d_status);
}

extern "C" int uf3_phonon_mesh(uf3_ctx *c, int32_t n_atoms, int64_t n_sc_atoms, const double *fc, const double *inv_sqrt_mass,
                               int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *q, double *lam,
                               int32_t *status) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_mesh: ctx is NULL");
    if (!fc || !inv_sqrt_mass || !q || !lam || !status) return fail(c, UF3_EINVAL, "uf3_phonon_mesh: null argument");
    if (n_atoms < 1 || n_atoms > PH_MAX_ATOMS || nq < 1 || nq > (int64_t)1 << 30 || n_sc_atoms < n_atoms || n_sc_atoms > (int64_t)1 << 24)
        return phonon_mesh_impl(c, n_atoms, n_sc_atoms, fc, inv_sqrt_mass, n_terms, terms, term_w, nq, q, lam, status);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = 3 * (size_t)n_atoms;
    Stage S(c->ph_io, c->stream);
    const int s_fc = S.add(8 * n3 * 3 * (size_t)n_sc_atoms), s_m = S.add(8 * (size_t)n_atoms), s_q = S.add(24 * (size_t)nq),
              s_l = S.add(8 * n3 * (size_t)nq), s_s = S.add(4 * (size_t)nq);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_fc, fc}, {s_m, inv_sqrt_mass}, {s_q, q}}));
    int rc = phonon_mesh_impl(c, n_atoms, n_sc_atoms, S.at<double>(s_fc), S.at<double>(s_m), n_terms, terms, term_w, nq,
                              S.at<double>(s_q), S.at<double>(s_l), S.at<int32_t>(s_s));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_l, lam}, {s_s, status}}));
    return UF3_OK;
}

extern "C" int uf3_phonon_mesh_vec_dev(uf3_ctx *c, int32_t n_atoms, int64_t n_sc_atoms, const double *d_fc, const double *d_inv_sqrt_mass,
                                       int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *d_q,
                                       double *d_lam, int32_t *d_status, const double *cell, double cutoff_thz, double *d_evec,
                                       double *d_gvel) {
    const PhVecOut V{cell, cutoff_thz, d_evec, d_gvel};
    return phonon_mesh_impl(c, n_atoms, n_sc_atoms, d_fc, d_inv_sqrt_mass, n_terms, terms, term_w, nq, d_q, d_lam, d_status, &V);
}

extern "C" int uf3_phonon_mesh_vec(uf3_ctx *c, int32_t n_atoms, int64_t n_sc_atoms, const double *fc, const double *inv_sqrt_mass,
                                   int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *q, double *lam,
                                   int32_t *status, const double *cell, double cutoff_thz, double *evec, double *gvel) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_mesh_vec: ctx is NULL");
    if (!fc || !inv_sqrt_mass || !q || !lam || !status) return fail(c, UF3_EINVAL, "uf3_phonon_mesh_vec: null argument");
    if (n_atoms < 1 || n_atoms > PH_VEC_MAX_ATOMS || nq < 1 || nq > (int64_t)1 << 30 || n_sc_atoms < n_atoms || n_sc_atoms > (int64_t)1 << 24 ||
        (!evec && !gvel)) {
        const PhVecOut V{cell, cutoff_thz, evec, gvel};
        return phonon_mesh_impl(c, n_atoms, n_sc_atoms, fc, inv_sqrt_mass, n_terms, terms, term_w, nq, q, lam, status, &V);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = 3 * (size_t)n_atoms;
    Stage S(c->ph_io, c->stream);
    const int s_fc = S.add(8 * n3 * 3 * (size_t)n_sc_atoms), s_m = S.add(8 * (size_t)n_atoms), s_q = S.add(24 * (size_t)nq),
              s_l = S.add(8 * n3 * (size_t)nq), s_s = S.add(4 * (size_t)nq), s_v = S.add(16 * n3 * n3 * (size_t)nq, evec != nullptr),
              s_g = S.add(24 * n3 * (size_t)nq, gvel != nullptr);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_fc, fc}, {s_m, inv_sqrt_mass}, {s_q, q}}));
    const PhVecOut V{cell, cutoff_thz, S.at<double>(s_v), S.at<double>(s_g)};
    int rc = phonon_mesh_impl(c, n_atoms, n_sc_atoms, S.at<double>(s_fc), S.at<double>(s_m), n_terms, terms, term_w, nq,
                              S.at<double>(s_q), S.at<double>(s_l), S.at<int32_t>(s_s), &V);
    if (rc) return rc;
    HIPCHK(c, S.out({{s_l, lam}, {s_s, status}, {s_v, evec}, {s_g, gvel}}));
    return UF3_OK;
}

// the sum of the q-weights and the caller's small host arrays (a | b) into ph_ws: [wsum | a | b]
static int phonon_small_inputs(uf3_ctx *c, const int64_t *d_wq, int64_t nq, const double *a, size_t na, const double *b, size_t nb,
                               long long **d_wsum, double **d_a, double **d_b) {
    hipStream_t st = c->stream;
    c->ph_stage.resize(8 * (na + nb + 2));
    double *h = (double *)c->ph_stage.data();
    h[0] = h[1] = 0.0;
    if (na) memcpy(h + 2, a, 8 * na);
    if (nb) memcpy(h + 2 + na, b, 8 * nb);
    HIPCHK(c, c->ph_ws.ensure(c->ph_stage.size()));
    HIPCHK(c, hipMemcpyAsync(c->ph_ws.p, h, c->ph_stage.size(), hipMemcpyHostToDevice, st));
    *d_wsum = c->ph_ws.as<long long>();
    *d_a = c->ph_ws.as<double>() + 2;
    *d_b = c->ph_ws.as<double>() + 2 + na;
    hipLaunchKernelGGL(k_ph_wsum, dim3(1), dim3(256), 0, st, (const long long *)d_wq, (long long)nq, *d_wsum);
    return UF3_OK;
}

static int phonon_dos_impl(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_bins,
                           const double *edges, int64_t *d_counts, int32_t n_samples, const double *samples, double sigma,
                           double *d_dos) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_dos: ctx is NULL");
    if (n_modes < 1 || n_modes > PH_MAX_DIM) return fail(c, UF3_EINVAL, "uf3_phonon_dos: modes per q-point must be in [1, " + std::to_string(PH_MAX_DIM) + "]");
    if (nq < 1 || nq > (int64_t)1 << 30) return fail(c, UF3_EINVAL, "uf3_phonon_dos: nq must be in [1, 2^30]");
    if (!d_lam) return fail(c, UF3_EINVAL, "uf3_phonon_dos: null eigenvalues");
    if (!d_counts && !d_dos) return fail(c, UF3_EINVAL, "uf3_phonon_dos: neither output asked for (counts and dos both NULL)");
    if (d_counts) {
        if (n_bins < 1 || n_bins > (1 << 24) || !edges) return fail(c, UF3_EINVAL, "uf3_phonon_dos: counts need n_bins in [1, 2^24] and edges");
        for (int k = 0; k <= n_bins; k++)
            if (!std::isfinite(edges[k]) || (k && !(edges[k] > edges[k - 1])))
                return fail(c, UF3_EINVAL, "uf3_phonon_dos: edges must be finite and strictly increasing");
    } else n_bins = 0;
    if (d_dos) {
        if (n_samples < 1 || n_samples > (1 << 24) || !samples) return fail(c, UF3_EINVAL, "uf3_phonon_dos: dos needs n_samples in [1, 2^24] and sample frequencies");
        if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(c, UF3_EINVAL, "uf3_phonon_dos: sigma must be positive and finite");
        for (int k = 0; k < n_samples; k++)
            if (!std::isfinite(samples[k])) return fail(c, UF3_EINVAL, "uf3_phonon_dos: sample frequencies must be finite");
    } else n_samples = 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    long long *d_wsum;
    double *d_edges, *d_samples;
    int rc = phonon_small_inputs(c, d_wq, nq, edges, n_bins ? (size_t)n_bins + 1 : 0, samples, (size_t)n_samples, &d_wsum, &d_edges, &d_samples);
    if (rc) return rc;
    const long long total = (long long)nq * n_modes;
    if (d_counts) {
        HIPCHK(c, hipMemsetAsync(d_counts, 0, 8 * (size_t)n_bins, st));
        hipLaunchKernelGGL(k_ph_hist, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_lam, (const long long *)d_wq, total,
                           (int)n_modes, (const double *)d_edges, (int)n_bins, (unsigned long long *)d_counts);
    }
    if (d_dos) {
        // chunks: a function of the sizes alone (at most 1024 of them, whole tiles), so the sums do not depend on the device
        long long chunk = std::max<long long>(4096, (total + 1023) / 1024);
        chunk = (chunk + PH_DOS_TILE - 1) / PH_DOS_TILE * PH_DOS_TILE;
        const int n_chunks = (int)((total + chunk - 1) / chunk);
        HIPCHK(c, c->ph_part.ensure(8 * (size_t)n_chunks * (size_t)n_samples));
        double *part = c->ph_part.as<double>();
        const unsigned gs = (unsigned)((n_samples + 255) / 256);
        hipLaunchKernelGGL(k_ph_dos_part, dim3(gs, (unsigned)n_chunks), dim3(256), 0, st, d_lam, (const long long *)d_wq, total, (int)n_modes,
                           chunk, (const double *)d_samples, (int)n_samples, 1.0 / sigma, part);
        hipLaunchKernelGGL(k_ph_dos_sum, dim3(gs), dim3(256), 0, st, (const double *)part, n_chunks, (int)n_samples, 1.0 / sigma,
                           (const long long *)d_wsum, d_dos);
    }
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_phonon_dos_dev(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_bins,
                                  const double *edges, int64_t *d_counts, int32_t n_samples, const double *samples, double sigma,
                                  double *d_dos) {
    return phonon_dos_impl(c, n_modes, nq, d_lam, d_wq, n_bins, edges, d_counts, n_samples, samples, sigma, d_dos);
}

extern "C" int uf3_phonon_dos(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *lam, const int64_t *wq, int32_t n_bins,
                              const double *edges, int64_t *counts, int32_t n_samples, const double *samples, double sigma, double *dos) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_dos: ctx is NULL");
    if (!lam || n_modes < 1 || n_modes > PH_MAX_DIM || nq < 1 || nq > (int64_t)1 << 30 || (!counts && !dos) ||
        (counts && (n_bins < 1 || n_bins > (1 << 24))) || (dos && (n_samples < 1 || n_samples > (1 << 24))))
        return phonon_dos_impl(c, n_modes, nq, lam, wq, n_bins, edges, counts, n_samples, samples, sigma, dos);
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->ph_io, c->stream);
    const int s_l = S.add(8 * (size_t)n_modes * (size_t)nq), s_w = S.add(8 * (size_t)nq, wq != nullptr),
              s_c = S.add(8 * (size_t)n_bins, counts != nullptr), s_d = S.add(8 * (size_t)n_samples, dos != nullptr);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_l, lam}, {s_w, wq}}));
    int rc = phonon_dos_impl(c, n_modes, nq, S.at<double>(s_l), S.at<int64_t>(s_w), n_bins, edges, S.at<int64_t>(s_c), n_samples,
                             samples, sigma, S.at<double>(s_d));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_c, counts}, {s_d, dos}}));
    return UF3_OK;
}

static int phonon_thermo_impl(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_temps,
                              const double *temps, double cutoff_thz, double *d_out, double *d_zpe, int64_t *d_excluded) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_thermo: ctx is NULL");
    if (n_modes < 1 || n_modes > PH_MAX_DIM) return fail(c, UF3_EINVAL, "uf3_phonon_thermo: modes per q-point must be in [1, " + std::to_string(PH_MAX_DIM) + "]");
    if (nq < 1 || nq > (int64_t)1 << 30) return fail(c, UF3_EINVAL, "uf3_phonon_thermo: nq must be in [1, 2^30]");
    if (n_temps < 1 || n_temps > 65535) return fail(c, UF3_EINVAL, "uf3_phonon_thermo: the number of temperatures must be in [1, 65535]");
    if (!d_lam || !temps || !d_out || !d_zpe || !d_excluded) return fail(c, UF3_EINVAL, "uf3_phonon_thermo: null argument");
    for (int k = 0; k < n_temps; k++)
        if (!(temps[k] >= 0.0) || !std::isfinite(temps[k]))
            return fail(c, UF3_EINVAL, "uf3_phonon_thermo: temperatures must be finite and not negative");
    if (!(cutoff_thz >= 0.0) || !std::isfinite(cutoff_thz)) return fail(c, UF3_EINVAL, "uf3_phonon_thermo: the cut-off must be finite and not negative");
    HIPCHK(c, hipSetDevice(c->device));
    long long *d_wsum;
    double *d_t, *d_none;
    int rc = phonon_small_inputs(c, d_wq, nq, temps, (size_t)n_temps, nullptr, 0, &d_wsum, &d_t, &d_none);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ph_thermo, dim3((unsigned)n_temps), dim3(256), 0, c->stream, d_lam, (const long long *)d_wq, (long long)nq * n_modes,
                       (int)n_modes, (const double *)d_t, cutoff_thz, (const long long *)d_wsum, d_out, d_zpe, (long long *)d_excluded);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_phonon_thermo_dev(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_temps,
                                     const double *temps, double cutoff_thz, double *d_out, double *d_zpe, int64_t *d_excluded) {
    return phonon_thermo_impl(c, n_modes, nq, d_lam, d_wq, n_temps, temps, cutoff_thz, d_out, d_zpe, d_excluded);
}

extern "C" int uf3_phonon_thermo(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *lam, const int64_t *wq, int32_t n_temps,
                                 const double *temps, double cutoff_thz, double *out, double *zpe, int64_t *excluded) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_thermo: ctx is NULL");
    if (!lam || !out || !zpe || !excluded || n_modes < 1 || n_modes > PH_MAX_DIM || nq < 1 || nq > (int64_t)1 << 30 || n_temps < 1 ||
        n_temps > 65535)
        return phonon_thermo_impl(c, n_modes, nq, lam, wq, n_temps, temps, cutoff_thz, out, zpe, excluded);
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->ph_io, c->stream);
    const int s_l = S.add(8 * (size_t)n_modes * (size_t)nq), s_w = S.add(8 * (size_t)nq, wq != nullptr),
              s_o = S.add(32 * (size_t)n_temps), s_z = S.add(8), s_e = S.add(8);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_l, lam}, {s_w, wq}}));
    int rc = phonon_thermo_impl(c, n_modes, nq, S.at<double>(s_l), S.at<int64_t>(s_w), n_temps, temps, cutoff_thz, S.at<double>(s_o),
                                S.at<double>(s_z), S.at<int64_t>(s_e));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_o, out}, {s_z, zpe}, {s_e, excluded}}));
    return UF3_OK;
}

static int phonon_pdos_impl(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                            int32_t n_samples, const double *samples, double sigma, double *d_out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_pdos: ctx is NULL");
    if (n_modes < 1 || n_modes > 3 * PH_VEC_MAX_ATOMS || n_modes % 3)
        return fail(c, UF3_EINVAL, "uf3_phonon_pdos: modes per q-point must be a multiple of 3 in [3, " + std::to_string(3 * PH_VEC_MAX_ATOMS) + "]");
    if (nq < 1 || nq > (int64_t)1 << 30) return fail(c, UF3_EINVAL, "uf3_phonon_pdos: nq must be in [1, 2^30]");
    if (!d_lam || !d_evec || !d_out) return fail(c, UF3_EINVAL, "uf3_phonon_pdos: null argument");
    if (n_samples < 1 || n_samples > (1 << 24) || !samples) return fail(c, UF3_EINVAL, "uf3_phonon_pdos: needs n_samples in [1, 2^24] and sample frequencies");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(c, UF3_EINVAL, "uf3_phonon_pdos: sigma must be positive and finite");
    for (int k = 0; k < n_samples; k++)
        if (!std::isfinite(samples[k])) return fail(c, UF3_EINVAL, "uf3_phonon_pdos: sample frequencies must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    long long *d_wsum;
    double *d_samples, *d_none;
    int rc = phonon_small_inputs(c, d_wq, nq, samples, (size_t)n_samples, nullptr, 0, &d_wsum, &d_samples, &d_none);
    if (rc) return rc;
    // chunks: a function of the mode count alone (at most 256 of them, whole tiles)
    const long long total = (long long)nq * n_modes;
    long long chunk = std::max<long long>(4096, (total + 255) / 256);
    chunk = (chunk + PH_DOS_TILE - 1) / PH_DOS_TILE * PH_DOS_TILE;
    const int n_chunks = (int)((total + chunk - 1) / chunk);
    HIPCHK(c, c->ph_part.ensure(8 * (size_t)n_chunks * (size_t)n_modes * (size_t)n_samples));
    double *part = c->ph_part.as<double>();
    const unsigned gs = (unsigned)((n_samples + 255) / 256), gc = (unsigned)((n_modes + PH_PDOS_CH - 1) / PH_PDOS_CH);
    hipLaunchKernelGGL(k_ph_pdos_part, dim3(gs, (unsigned)n_chunks, gc), dim3(256), 0, st, d_lam, d_evec, (const long long *)d_wq, total,
                       (int)n_modes, chunk, (const double *)d_samples, (int)n_samples, 1.0 / sigma, part);
    hipLaunchKernelGGL(k_ph_pdos_sum, dim3(gs, (unsigned)n_modes), dim3(256), 0, st, (const double *)part, n_chunks, (int)n_modes,
                       (int)n_samples, 1.0 / sigma, (const long long *)d_wsum, d_out);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_phonon_pdos_dev(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                                   int32_t n_samples, const double *samples, double sigma, double *d_out) {
    return phonon_pdos_impl(c, n_modes, nq, d_lam, d_evec, d_wq, n_samples, samples, sigma, d_out);
}

extern "C" int uf3_phonon_pdos(uf3_ctx *c, int32_t n_modes, int64_t nq, const double *lam, const double *evec, const int64_t *wq,
                               int32_t n_samples, const double *samples, double sigma, double *out) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_pdos: ctx is NULL");
    if (!lam || !evec || !out || n_modes < 1 || n_modes > 3 * PH_VEC_MAX_ATOMS || n_modes % 3 || nq < 1 || nq > (int64_t)1 << 30 || n_samples < 1 ||
        n_samples > (1 << 24))
        return phonon_pdos_impl(c, n_modes, nq, lam, evec, wq, n_samples, samples, sigma, out);
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->ph_io, c->stream);
    const size_t nm = (size_t)n_modes;
    const int s_l = S.add(8 * nm * (size_t)nq), s_v = S.add(16 * nm * nm * (size_t)nq), s_w = S.add(8 * (size_t)nq, wq != nullptr),
              s_o = S.add(8 * nm * (size_t)n_samples);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_l, lam}, {s_v, evec}, {s_w, wq}}));
    int rc = phonon_pdos_impl(c, n_modes, nq, S.at<double>(s_l), S.at<double>(s_v), S.at<int64_t>(s_w), n_samples, samples, sigma,
                              S.at<double>(s_o));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_o, out}}));
    return UF3_OK;
}

// inv_sqrt_mass [N] is one of the small host arrays here, in both entries
static int phonon_tdisp_impl(uf3_ctx *c, int32_t n_atoms, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                             const double *inv_sqrt_mass, int32_t n_temps, const double *temps, double cutoff_thz, double *d_out,
                             int64_t *d_excluded) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_tdisp: ctx is NULL");
    if (n_atoms < 1 || n_atoms > PH_VEC_MAX_ATOMS)
        return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: the cell's atom count must be in [1, " + std::to_string(PH_VEC_MAX_ATOMS) + "]");
    if (nq < 1 || nq > (int64_t)1 << 30) return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: nq must be in [1, 2^30]");
    if (n_temps < 1 || n_temps > 65535) return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: the number of temperatures must be in [1, 65535]");
    if (!d_lam || !d_evec || !inv_sqrt_mass || !temps || !d_out || !d_excluded) return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: null argument");
    for (int k = 0; k < n_temps; k++)
        if (!(temps[k] >= 0.0) || !std::isfinite(temps[k]))
            return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: temperatures must be finite and not negative");
    for (int k = 0; k < n_atoms; k++)
        if (!(inv_sqrt_mass[k] > 0.0) || !std::isfinite(inv_sqrt_mass[k]))
            return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: inverse root masses must be positive and finite");
    if (!(cutoff_thz >= 0.0) || !std::isfinite(cutoff_thz)) return fail(c, UF3_EINVAL, "uf3_phonon_tdisp: the cut-off must be finite and not negative");
    HIPCHK(c, hipSetDevice(c->device));
    long long *d_wsum;
    double *d_t, *d_m;
    int rc = phonon_small_inputs(c, d_wq, nq, temps, (size_t)n_temps, inv_sqrt_mass, (size_t)n_atoms, &d_wsum, &d_t, &d_m);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ph_tdisp, dim3((unsigned)n_temps, (unsigned)n_atoms), dim3(256), 0, c->stream, d_lam, d_evec, (const long long *)d_wq,
                       (long long)nq * 3 * n_atoms, 3 * (int)n_atoms, (const double *)d_m, (const double *)d_t, cutoff_thz,
                       (const long long *)d_wsum, d_out, (long long *)d_excluded);
    HIPCHK(c, hipGetLastError());
    return UF3_OK;
}

extern "C" int uf3_phonon_tdisp_dev(uf3_ctx *c, int32_t n_atoms, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                                    const double *inv_sqrt_mass, int32_t n_temps, const double *temps, double cutoff_thz, double *d_out,
                                    int64_t *d_excluded) {
    return phonon_tdisp_impl(c, n_atoms, nq, d_lam, d_evec, d_wq, inv_sqrt_mass, n_temps, temps, cutoff_thz, d_out, d_excluded);
}

extern "C" int uf3_phonon_tdisp(uf3_ctx *c, int32_t n_atoms, int64_t nq, const double *lam, const double *evec, const int64_t *wq,
                                const double *inv_sqrt_mass, int32_t n_temps, const double *temps, double cutoff_thz, double *out,
                                int64_t *excluded) {
    if (!c) return fail(nullptr, UF3_EINVAL, "uf3_phonon_tdisp: ctx is NULL");
    if (!lam || !evec || !out || !excluded || n_atoms < 1 || n_atoms > PH_VEC_MAX_ATOMS || nq < 1 || nq > (int64_t)1 << 30 || n_temps < 1 ||
        n_temps > 65535)
        return phonon_tdisp_impl(c, n_atoms, nq, lam, evec, wq, inv_sqrt_mass, n_temps, temps, cutoff_thz, out, excluded);
    HIPCHK(c, hipSetDevice(c->device));
    Stage S(c->ph_io, c->stream);
    const size_t nm = 3 * (size_t)n_atoms;
    const int s_l = S.add(8 * nm * (size_t)nq), s_v = S.add(16 * nm * nm * (size_t)nq), s_w = S.add(8 * (size_t)nq, wq != nullptr),
              s_o = S.add(48 * (size_t)n_atoms * (size_t)n_temps), s_e = S.add(8);
    HIPCHK(c, S.alloc());
    HIPCHK(c, S.in({{s_l, lam}, {s_v, evec}, {s_w, wq}}));
    int rc = phonon_tdisp_impl(c, n_atoms, nq, S.at<double>(s_l), S.at<double>(s_v), S.at<int64_t>(s_w), inv_sqrt_mass, n_temps, temps,
                               cutoff_thz, S.at<double>(s_o), S.at<int64_t>(s_e));
    if (rc) return rc;
    HIPCHK(c, S.out({{s_o, out}, {s_e, excluded}}));
    return UF3_OK;
}

#ifdef UF3_PHASE_TIMING
// experiments only: read (and clear) the in-kernel phase timers
extern "C" int uf3_debug_phase(unsigned long long *out16) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 16);
    unsigned long long z[16] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z));
    return 0;
}
#endif
