// dff_host.hip -- host half of libdff_amd.so: the model handle (upload of the images dff_prep.hip prepares), scratch
// management, kernel dispatch and the model's part of the extern "C" ABI declared in include/dff.h
// (the stateless sample-analysis entry points are dff_analysis.hip).
#include "../../include/dff.h"
#include "dff_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// the two sampler kernels are their own translation units (dff_kernels.hip, dff_small.hip: they export variant
// lookups, dff_device.h); the sample-analysis entry points and their kernels are a third (dff_analysis.hip)
#include "dff_device.h"
#include "dff_host_common.h"
#include "dff_prep.h"

static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// ------------------------------------------------------------------------------------------
// model handle
// ------------------------------------------------------------------------------------------
struct dff_model {
    dff_config cfg;
    int device;
    DffModelDev dev;
    std::vector<void*> allocs;
    std::vector<std::vector<float>> sched;  // 12 tables, host fp32
    float* stash = nullptr;
    size_t stash_floats = 0;
    int group_override = 0;
    bool force_generic = false;   // debugging: never use the rows<=16 fast path
    int small_waves = 0;          // 0 auto, 4: never use the 8-wave variant
    bool last_small = false;
    unsigned long long* prof = nullptr;
    bool prof_on = false;
    int prof_wave = 0;
    // last launch
    const char* last_kernel = "";
    int last_grid = 0, last_lds = 0, last_G = 0, last_B = 0;
    unsigned long long last_stride = 0;
    int last_mt = 1;                           // row tiles of the <= 64-row variant that ran last (stash layout of the debug reads)
    // precomputed layer-0 tables (see ensure_l0_table), keyed independently: [0] one entry at tnorm (Langevin),
    // [1] one entry per noise level (DDPM) -- `sample.py --gen_mode langevin` uses both, alternately
    struct L0Table {
        float* tab = nullptr;
        size_t floats = 0;
        bool valid = false;
        int G = 0, waves = -1;
        float tnorm = 0.f;
        const void* variant = nullptr;
        bool split = false;
        unsigned long long used = 0;           // last use (dff_model::l0_clock): the slot that was idle longest is rebuilt
    } l0[2][3];                                // a few per kind: batches that alternate between group sizes / variants (ADVICE r05:
    unsigned long long l0_clock = 0;           // ala2 crossing 128 / 256 / 384 per GPU) keep their tables instead of rebuilding one slot
    bool l0_off = false;                       // debugging: never use the table
    int max_wgs = 2048;                        // workgroups per launch: bounds the stash (grid x stash slot) for big batches
    int last_base = 0;
    bool split = false;                        // split (fp16) images exist, SPW variants preferred (DFF_SPLIT_BF16=0 at model creation: never)
    bool small_split = false;                  // ... and the <= 16-row kernel has an SPW variant for this model
    bool fold_kv = false;                      // H == 64: k = v = LayerNorm output (W_k folded into W_q, W_v into W_o); DFF_FOLD_KV=0: never
    // PAIR variants (two workgroups per protein): partial-tile exchange slots and flags
    float* xchg = nullptr;
    size_t xchg_floats = 0;
    unsigned* xflag = nullptr;
    size_t xflag_n = 0;
    bool pair_off = false;                     // debugging: never use a PAIR variant
    int pair_slow = 0;                         // tests: 1 = PAIR variants always run the cross-XCD (agent-scope) exchange protocol; 2 = partners are
                                               // ADJACENT blocks (different XCDs under round-robin placement), protocol chosen by the handshake
    bool last_pair = false;
    unsigned sticky = 0;                       // the sticky error word as the host last read it (read_status): a non-zero one
                                               // refuses further PAIR launches WITHOUT touching the device
    int n_cus = 0;                             // hipDeviceAttributeMultiprocessorCount of `device`
    const float *sqrt_ac = nullptr, *sqrt_1mac = nullptr;   // forward-process tables on the device (dff_loss.hip; the kernels' DffModelDev has no use for them)
};

template <class T> static int upload(dff_model* m, const std::vector<T>& h, const T** out) {
    *out = nullptr;
    if (h.empty()) return DFF_OK;   // an image of an engine this model does not run
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, h.size() * sizeof(T)));
    m->allocs.push_back(p);
    HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return DFF_OK;
}
#define UP(vec, dst)                                  \
    do {                                              \
        int rc_ = upload(m, vec, &(dst));             \
        if (rc_) return rc_;                          \
    } while (0)

static bool env_flag(const char* name, char ch) {   // the variable is set and starts with `ch`
    const char* e = getenv(name);
    return e && e[0] == ch;
}
// input branches other than the shipped one (intrinsic coordinates only) run the GEN variants
static bool is_gen(const dff_config& c) { return !(c.use_intrinsic_coords == 1 && c.use_distances == 0 && c.use_abs_coords == 0); }

extern "C" int dff_model_create(const dff_config* cfg, const float* w, size_t n_weights, int device,
                                dff_model** out) {
    if (!cfg || !w || !out) return fail(DFF_EINVAL, "null argument");
    auto is01 = [](int v) { return v == 0 || v == 1; };
    if (!(is01(cfg->use_intrinsic_coords) && is01(cfg->use_distances) && is01(cfg->use_abs_coords) && is01(cfg->conservative)))
        return fail(DFF_EINVAL, "use_intrinsic_coords, use_distances, use_abs_coords and conservative must be 0 or 1");
    const int H = cfg->hidden, N = cfg->n_beads, L = cfg->n_layers;
    // hidden sizes with kernel variants: the shipped 64 / 96 / 128, and 256 (the reference's own smoke test,
    // models/graph_transformer.py:332-359; fp32 engine, <= 32 beads)
    if (!(H == 64 || H == 96 || H == 128 || H == 256)) return fail(DFF_EINVAL, "hidden must be 64, 96, 128 or 256 (got %d)", H);
    if (N < 2 || N > DFF_MAX_BEADS) return fail(DFF_EINVAL, "n_beads must be in [2,%d] (got %d)", DFF_MAX_BEADS, N);
    if (H != 128 && N > 32) return fail(DFF_EINVAL, "n_beads > 32 needs hidden = 128 in this build");
    // (four row tiles: 520 floats of LDS per bead row + 36 KB of tile arrays and bookkeeping -- 61 rows are what 160 KB hold;
    // the largest shipped model, protein G, has 56)
    if (N > DFF_MAX_BEADS_LDS) return fail(DFF_EINVAL, "n_beads > %d does not fit the LDS of this build's kernels (got %d)", DFF_MAX_BEADS_LDS, N);
    if (L < 1 || L > DFF_MAX_LAYERS) return fail(DFF_EINVAL, "n_layers must be in [1,%d]", DFF_MAX_LAYERS);
    if (cfg->timesteps < 1) return fail(DFF_EINVAL, "timesteps must be >= 1");
    if (n_weights != dff_weight_count(cfg))
        return fail(DFF_EINVAL, "expected %zu weights, got %zu", dff_weight_count(cfg), n_weights);
    ON_DEVICE(device);
    dff_model* m = new dff_model();
    struct Undo {   // any failure below frees what was uploaded so far
        dff_model* m;
        ~Undo() { if (m) dff_model_destroy(m); }
    } undo{m};
    m->cfg = *cfg;
    m->device = device;
    HIPCHK(hipDeviceGetAttribute(&m->n_cus, hipDeviceAttributeMultiprocessorCount, device));
    // weight GEMMs on the fp16 pipe (default) unless DFF_SPLIT_BF16=0: every GEMM on v_mfma_f32_16x16x4_f32; DFF_FOLD_KV=0: no k / v
    // fold.  The range guard (dff_prep.hip) has the last word on the engine, and says so on stderr.
    const void* fn_; unsigned lds_; const char* nm_;
    dff_prep::DffPrep p = dff_prep::dff_prepare(*cfg, w, !env_flag("DFF_SPLIT_BF16", '0'), !env_flag("DFF_FOLD_KV", '0'),
                                                N <= 10 && dff_small_pick(DFF_MODE_SCORE, H, 8, false, true, &fn_, &lds_, &nm_));
    fputs(p.note.c_str(), stderr);
    m->split = p.split; m->small_split = p.small_split; m->fold_kv = p.fold_kv;
    // Two workgroups per protein (PAIR variants) need both blocks of a pair resident at once, and the launches are not cooperative
    // (ADVICE r05): never where the GPU is known to be shared -- more local ranks than visible devices (torchrun's
    // LOCAL_WORLD_SIZE) -- or where the caller says so (DFF_PAIR=0).  dff_debug_pair(m, 1) turns them back on.
    const char* lw = getenv("LOCAL_WORLD_SIZE");
    int ndev = 0;
    if (env_flag("DFF_PAIR", '0')) m->pair_off = true;
    else if (lw && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && atoi(lw) > ndev) {
        m->pair_off = true;
        static bool said = false;
        if (!said) { said = true; fprintf(stderr, "dff: %s local ranks share %d GPU(s): the two-workgroups-per-protein kernels are off\n", lw, ndev); }
    }
    memset(&m->dev, 0, sizeof m->dev);
    m->dev.N = N; m->dev.H = H; m->dev.L = L; m->dev.T = cfg->timesteps;
    m->dev.in_intr = cfg->use_intrinsic_coords; m->dev.in_dist = cfg->use_distances; m->dev.in_abs = cfg->use_abs_coords;
    m->dev.wn_t = N + 3 * cfg->use_abs_coords;
    m->dev.conservative = cfg->conservative;
    m->dev.bdec = p.bdec;
    memcpy(m->dev.bdec3, p.bdec3, sizeof p.bdec3);
    UP(p.WnT, m->dev.WnT); UP(p.bn, m->dev.bn); UP(p.wdec, m->dev.wdec);
    for (int l = 0; l < L; ++l) {
        DffLayerDev& d = m->dev.layer[l];
#define X(T, n) UP(p.layer[l].n, d.n);
        DFF_LAYER_IMAGES(X)
#undef X
    }
    m->sched = std::move(p.sched);
    UP(m->sched[6], m->dev.sqrt_recip_ac);
    UP(m->sched[7], m->dev.sqrt_recipm1_ac);
    UP(m->sched[10], m->dev.post_c1);
    UP(m->sched[11], m->dev.post_c2);
    UP(m->sched[9], m->dev.post_logvar);
    UP(m->sched[3], m->sqrt_ac);
    UP(m->sched[4], m->sqrt_1mac);
    undo.m = nullptr;
    *out = m;
    return DFF_OK;
}

extern "C" void dff_model_destroy(dff_model* m) {
    if (!m) return;
    DeviceGuard g(m->device);
    for (void* p : m->allocs) (void)hipFree(p);
    if (m->stash) (void)hipFree(m->stash);
    if (m->xchg) (void)hipFree(m->xchg);
    if (m->xflag) (void)hipFree(m->xflag);
    if (m->prof) (void)hipFree(m->prof);
    for (auto& k : m->l0) for (auto& t : k) if (t.tab) (void)hipFree(t.tab);
    delete m;
}

extern "C" int dff_schedule(const dff_model* m, int which, float* out_host) {
    if (!m || !out_host || which < 0 || which >= 12) return fail(DFF_EINVAL, "bad schedule request");
    memcpy(out_host, m->sched[which].data(), m->sched[which].size() * sizeof(float));
    return DFF_OK;
}

// what the forward-process unit (dff_loss.hip) needs of the handle, which is private to this file
int dff_model_loss_view(const dff_model* m, DffLossView* v) {
    if (!m || !v) return fail(DFF_EINVAL, "null argument");
    v->device = m->device; v->n_beads = m->cfg.n_beads; v->timesteps = m->cfg.timesteps;
    v->sqrt_ac = m->sqrt_ac; v->sqrt_1mac = m->sqrt_1mac;
    return DFF_OK;
}

extern "C" int dff_set_group(dff_model* m, int g) {
    if (!m || g < 0) return fail(DFF_EINVAL, "bad group");
    m->group_override = g;
    return DFF_OK;
}

extern "C" int dff_debug_force_generic(dff_model* m, int on) {
    if (!m) return fail(DFF_EINVAL, "null model");
    m->force_generic = on != 0;
    return DFF_OK;
}

extern "C" int dff_debug_max_workgroups(dff_model* m, int n) {
    if (!m || n < 1) return fail(DFF_EINVAL, "bad workgroup limit");
    m->max_wgs = n;
    return DFF_OK;
}

static int clear_status(dff_model* m);
extern "C" int dff_debug_pair(dff_model* m, int on) {
    if (!m) return fail(DFF_EINVAL, "null model");
    m->pair_off = on == 0;
    m->pair_slow = on == 2 ? 1 : on == 3 ? 2 : 0;
    // turning the PAIR variants off is how a caller recovers from a partner timeout: the one-workgroup kernels do not look
    // at the word, so it is cleared here (it would otherwise fail every later status check of a model that works again)
    // (unconditionally -- ADVICE r04: the DEVICE word may be set before the host has looked at it; clear_status synchronises,
    // which a debug / recovery call may do)
    if (m->pair_off && m->xflag) return clear_status(m);
    return DFF_OK;
}

// Sticky status of the model's launches so far: bit 0 = a PAIR launch (two workgroups per protein) gave up waiting for a
// partner workgroup (bounded spin instead of a hang; the results of that launch are invalid).  The word lives at
// xflag[0], is only ever OR-ed by the kernels and is never cleared by a launch, so an error in ANY launch of a chunked
// run is still there when the caller looks.  Synchronises the device -- which is why only the status calls come here: the
// launch path never does (a PAIR kernel that finds the word set at entry leaves at once, and launch() refuses PAIR on the
// host's cached copy), so dff_score / dff_langevin_run / dff_ddpm_run stay asynchronous on the caller's stream.
static int read_status(dff_model* m, unsigned* word, bool clear) {
    *word = 0;
    if (!m->xflag) return DFF_OK;
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(word, m->xflag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (clear && *word) HIPCHK(hipMemset(m->xflag, 0, sizeof(unsigned)));
    m->sticky = clear ? 0u : *word;
    return DFF_OK;
}
static int clear_status(dff_model* m) {
    unsigned w = 0;
    return read_status(m, &w, true);
}

extern "C" int dff_model_status(dff_model* m, unsigned* status) {
    if (!m || !status) return fail(DFF_EINVAL, "null argument");
    return read_status(m, status, false);
}

extern "C" int dff_model_status_clear(dff_model* m) {
    if (!m) return fail(DFF_EINVAL, "null model");
    return clear_status(m);
}

// tests: set the DEVICE word behind the host's back (as a kernel that lost its partner would), host cache untouched
extern "C" int dff_debug_poke_status(dff_model* m, unsigned word) {
    if (!m) return fail(DFF_EINVAL, "null model");
    if (!m->xflag) return fail(DFF_EINVAL, "no two-workgroups launch has run on this model yet");
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(m->xflag, &word, sizeof(unsigned), hipMemcpyHostToDevice));
    return DFF_OK;
}

// debugging form: reads AND clears
extern "C" int dff_debug_pair_status(dff_model* m, int* status) {
    if (!m || !status) return fail(DFF_EINVAL, "null argument");
    unsigned w = 0;
    const int rc = read_status(m, &w, true);
    *status = (int)w;
    return rc;
}

extern "C" int dff_debug_l0_table(dff_model* m, int on) {
    if (!m) return fail(DFF_EINVAL, "null model");
    m->l0_off = on == 0;
    return DFF_OK;
}

extern "C" int dff_debug_small_waves(dff_model* m, int waves) {
    if (!m || !(waves == 0 || waves == 4 || waves == 8)) return fail(DFF_EINVAL, "waves must be 0 (auto), 4 or 8");
    m->small_waves = waves;
    return DFF_OK;
}

extern "C" int dff_last_launch(const dff_model* m, const char** name, int* grid, int* lds) {
    if (!m) return fail(DFF_EINVAL, "null model");
    if (name) *name = m->last_kernel;
    if (grid) *grid = m->last_grid;
    if (lds) *lds = m->last_lds;
    return DFF_OK;
}

static int grow(float*& p, size_t& have, size_t need) {   // a device buffer of at least `need` floats (contents are not kept)
    if (need <= have) return DFF_OK;
    if (p) HIPCHK(hipFree(p));
    p = nullptr; have = 0;
    HIPCHK(hipMalloc((void**)&p, need * sizeof(float)));
    have = need;
    return DFF_OK;
}

// Two workgroups per protein need both blocks of a pair RESIDENT at once, and the launch is not cooperative: a PAIR grid (blocks b
// and b + 8 share a protein, 16 blocks per 8 groups) must fit the device's CUs one block each, in ONE launch
static bool pairs_fit(const dff_model* m, int ngroups) {
    return 2 * 8 * ((ngroups + 7) / 8) <= (m->n_cus < m->max_wgs ? m->n_cus : m->max_wgs);
}

// what the launch path needs to know of a kernel variant at a group size
struct LaunchSpec {
    const void* fn;
    const char* name;
    unsigned lds;                 // bytes
    int nthreads;
    bool pair, small;             // two workgroups per protein; the <= 16-row kernel (stash layout of the debug reads)
    int mt, prof_waves;           // row tiles (<= 64-row kernel); waves dff_debug_profile can pick from (<= 16-row kernel; else wave 0)
    size_t stash, layer_stride;   // floats per workgroup, and per layer of it
    size_t xchg;                  // PAIR: exchange floats per pair
};

// rows <= 16: one-head-per-wave kernel (dff_small.hip)
static int small_spec(const dff_model* m, int mode, int G, bool pair, LaunchSpec* s) {
    const int N = m->cfg.n_beads, H = m->cfg.hidden;
    // 8 waves (two per SIMD, one head per wave) when the rows fit its 11-row head buffers
    const bool eight = (H == 64 || H == 96) && G * N <= 10 && m->small_waves != 4;
    const int NW = eight ? 8 : 4;
    if (!dff_small_pick(mode, H, NW, is_gen(m->cfg), eight && m->small_split, &s->fn, &s->lds, &s->name, m->fold_kv, pair))
        return fail(DFF_EINVAL, "no <= 16-row kernel for hidden=%d waves=%d in this build", H, NW);
    s->lds *= (unsigned)sizeof(float);
    if (s->lds > 160 * 1024) return fail(DFF_EINVAL, "LDS budget exceeded (%u bytes)", s->lds);
    const SmallStash sl = dff_small_stash(N, G, H, m->cfg.n_layers);
    s->nthreads = pair ? 256 : NW * 64; s->pair = pair; s->small = true; s->mt = 1; s->prof_waves = NW;
    s->stash = sl.total; s->layer_stride = sl.layer_stride;
    s->xchg = 4 * 1024;   // [half][parity][256 threads x 4 floats]
    return DFF_OK;
}
static bool small_pair_available(const dff_model* m, int mode, int G) {
    const int N = m->cfg.n_beads, H = m->cfg.hidden;
    const void* fn; unsigned lds; const char* name;
    // OPT-IN (DFF_SMALL_PAIR=1, read per launch): built and measured in round 6 -- chignolin at 128 / 100 / 32 per GPU 45.8 / 45.9 / 45.4 us
    // per step against 44.4 with one workgroup per protein.  The wave-private blocks do shrink (-19 k cycles per step: four waves,
    // one per SIMD), but each of the 12 exchanges costs ~1.8 k cycles inside its row stage -- a store's s_waitcnt vmcnt(0) also
    // waits for the weight units the wave has just requested for the next block (loads and stores retire through one in-order
    // counter), 0.25 - 0.45 us in tools_ubench/pair_exchange.hip without that -- and the 16-lanes-per-row stages issue more per thread
    // (profiles/r06/pair_small/).  Kept as a tested variant; not the default.
    if (!env_flag("DFF_SMALL_PAIR", '1')) return false;
    return H == 64 && G * N <= 10 && m->small_waves == 0 && m->small_split && m->fold_kv && !is_gen(m->cfg) && m->cfg.conservative &&
           dff_small_pick(mode, H, 8, false, true, &fn, &lds, &name, true, true);
}
// generic kernel (rows <= 64), variant already chosen
static int generic_spec(const dff_model* m, int G, const Variant* v, LaunchSpec* s) {
    const int N = m->cfg.n_beads, H = m->cfg.hidden;
    s->lds = v->lds_floats(N, G) * (unsigned)sizeof(float);
    if (s->lds > 160 * 1024) return fail(DFF_EINVAL, "LDS budget exceeded (%u bytes) for N=%d G=%d H=%d", s->lds, N, G, H);
    const StashLayout sl = dff_stash_layout(N, G, H, m->cfg.n_layers, v->MT);
    s->fn = v->fn; s->name = v->name; s->nthreads = DFF_NTHREADS; s->pair = v->pair; s->small = false; s->mt = v->MT; s->prof_waves = 0;
    s->stash = sl.total; s->layer_stride = sl.layer_stride;
    s->xchg = 4 * (size_t)(G * N) * (H + 4);   // [half][parity][rows x (H + 4)]
    return DFF_OK;
}

// one launch path for both kernels: grid, stash, PAIR buffers, the launches, the last_* record
static int run(dff_model* m, DffRunArgs& a, int G, const LaunchSpec& s, hipStream_t stream) {
    // PAIR: 16 blocks per 8 groups (a pair shares a GROUP of G proteins: ala2 two or three to a 16-row tile), ONE launch -- the caller
    // has checked pairs_fit
    const int ngroups = (a.B + G - 1) / G;
    const int npairs = s.pair ? 8 * ((ngroups + 7) / 8) : 0;
    const int grid_all = s.pair ? 2 * npairs : ngroups;
    // (so a PAIR grid is the single pass w0 = 0 of the loop below: b_base = w0 * G is the 0 the <= 16-row PAIR kernel expects)
    const int grid_max = s.pair ? grid_all : (grid_all < m->max_wgs ? grid_all : m->max_wgs);
    int rc = grow(m->stash, m->stash_floats, (size_t)grid_max * s.stash);
    if (rc) return rc;
    a.xchg = nullptr; a.xflag = nullptr; a.xpairs = npairs; a.xslow = m->pair_slow;
    if (s.pair) {
        // the exchange slots and the flag words -- error word, [pair][half] sequence flags, [pair][half] XCD ids; the sequence
        // numbers restart at every launch, the error word at [0] is NOT touched
        const size_t nflag = (size_t)4 * npairs + 1;
        if ((rc = grow(m->xchg, m->xchg_floats, (size_t)npairs * s.xchg))) return rc;
        if (!m->xflag) {   // once per model, sized for the largest grid a PAIR launch can have (one block per CU): no
                           // re-allocation -- and so no synchronisation -- on the launch path afterwards
            const size_t cap = 2 * (size_t)(m->n_cus > 256 ? m->n_cus : 256) + 1;   // 4 words per pair, at most n_cus / 2 pairs
            HIPCHK(hipMalloc((void**)&m->xflag, cap * sizeof(unsigned)));
            HIPCHK(hipMemsetAsync(m->xflag, 0, sizeof(unsigned), stream));
            m->xflag_n = cap;
        }
        if (nflag > m->xflag_n) return fail(DFF_EINVAL, "PAIR grid of %d pairs exceeds the flag array", npairs);
        HIPCHK(hipMemsetAsync(m->xflag + 1, 0, (nflag - 1) * sizeof(unsigned), stream));
        a.xchg = m->xchg; a.xflag = m->xflag;
    }
    m->last_small = s.small; m->last_pair = s.pair; m->last_mt = s.mt;
    a.G = G;
    a.prof = m->prof_on ? m->prof : nullptr;
    a.prof_wave = m->prof_wave < s.prof_waves ? m->prof_wave : 0;
    a.stash = m->stash;
    a.stash_stride = s.stash;
    HIPCHK(hipFuncSetAttribute(s.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
    // independent proteins: a batch larger than max_wgs workgroups runs as consecutive launches (same stream,
    // same stash), each over the whole step range
    for (int w0 = 0; w0 < grid_all; w0 += grid_max) {
        const int grid = grid_all - w0 < grid_max ? grid_all - w0 : grid_max;
        a.b_base = w0 * G;
        void* args[] = {(void*)&m->dev, (void*)&a};
        HIPCHK(hipLaunchKernel(s.fn, dim3(grid), dim3(s.nthreads), args, s.lds, stream));
        m->last_grid = grid; m->last_base = a.b_base;
        a.prof = nullptr;   // per-stage cycles: first launch only
    }
    m->last_kernel = s.name; m->last_lds = (int)s.lds; m->last_G = G; m->last_B = a.B;
    m->last_stride = s.stash;
    return DFF_OK;
}

// Layer-0 inputs do not depend on x (node features are [one-hot, t]): nodes_in and the
// [q|u|k|v] rows of layer 0 are functions of the noise level only.  They are computed ONCE per noise
// level by running the sampling kernel itself in score mode (one workgroup per level, x = 0) and
// copying the layer-0 slot of each workgroup's stash into a table, which the sampling loops then read
// instead of running layer 0's QKV GEMM: bit-identical values (same code produced them), one shared
// L2-resident copy instead of one per workgroup.  Langevin: one entry (its fixed t); DDPM: T entries,
// built in chunks so that the stash does not grow beyond what sampling needs anyway.
// v == nullptr: rows<=16 kernel, else that variant of the generic kernel.
static int ensure_l0_table(dff_model* m, int kind, float t_norm, int G, const Variant* v, hipStream_t stream, const float** out) {
    const int N = m->cfg.n_beads, T = m->cfg.timesteps;
    dff_model::L0Table* slot = nullptr;
    for (auto& c : m->l0[kind - 1]) {
        if (c.valid && c.G == G && c.waves == m->small_waves && c.variant == (const void*)v && c.split == m->small_split &&
            (kind == 2 || c.tnorm == t_norm)) {
            c.used = ++m->l0_clock;
            *out = c.tab;
            return DFF_OK;
        }
        if (!slot || (!c.valid && slot->valid) || (c.valid == slot->valid && c.used < slot->used)) slot = &c;
    }
    dff_model::L0Table& tb = *slot;
    *out = nullptr;
    const int nent = kind == 2 ? T : 1;
    tb.valid = false;   // invalid until filled
    LaunchSpec s;
    int rc = v ? generic_spec(m, G, v, &s) : small_spec(m, DFF_MODE_SCORE, G, false, &s);
    if (rc) return rc;
    const size_t layer_stride = s.layer_stride, total = s.stash;
    if ((rc = grow(tb.tab, tb.floats, (size_t)nent * layer_stride))) return rc;
    int CH = nent < 256 ? nent : 256;         // noise levels (= workgroups) per build launch ...
    if (CH > m->max_wgs) CH = m->max_wgs;     // ... each of which must be ONE kernel launch (its stash is copied out)
    const int Bmax = CH * G;
    struct Tmp {   // freed on every path
        float *xz = nullptr, *tnd = nullptr, *fo = nullptr;
        ~Tmp() { (void)hipFree(xz); (void)hipFree(fo); (void)hipFree(tnd); }
    } tmp;
    HIPCHK(hipMalloc((void**)&tmp.xz, (size_t)Bmax * N * 3 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&tmp.fo, (size_t)Bmax * N * 3 * sizeof(float)));
    HIPCHK(hipMalloc((void**)&tmp.tnd, (size_t)Bmax * sizeof(float)));
    HIPCHK(hipMemsetAsync(tmp.xz, 0, (size_t)Bmax * N * 3 * sizeof(float), stream));
    std::vector<float> tn((size_t)Bmax);
    for (int e0 = 0; e0 < nent; e0 += CH) {
        const int ne = nent - e0 < CH ? nent - e0 : CH;
        for (int e = 0; e < ne; ++e)
            for (int g = 0; g < G; ++g)
                tn[(size_t)e * G + g] = kind == 2 ? (1.0f * (float)(e0 + e)) / (float)T : t_norm;   // as the kernel forms t/T
        HIPCHK(hipMemcpyAsync(tmp.tnd, tn.data(), (size_t)ne * G * sizeof(float), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));   // tn is reused by the next chunk
        DffRunArgs a;
        memset(&a, 0, sizeof(a));
        a.mode = DFF_MODE_SCORE; a.B = ne * G; a.n_steps = 1; a.save_interval = 1;
        a.x_in = tmp.xz; a.tnorm = tmp.tnd; a.force_out = tmp.fo;
        if ((rc = run(m, a, G, s, stream))) return rc;
        // only the layer-0 slot of each workgroup's stash is kept
        HIPCHK(hipMemcpy2DAsync(tb.tab + (size_t)e0 * layer_stride, layer_stride * sizeof(float), m->stash,
                                total * sizeof(float), layer_stride * sizeof(float), (size_t)ne,
                                hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    tb.valid = true; tb.G = G; tb.waves = m->small_waves; tb.tnorm = t_norm; tb.variant = (const void*)v; tb.split = m->small_split;
    tb.used = ++m->l0_clock;
    *out = tb.tab;
    return DFF_OK;
}

// choose proteins-per-workgroup and the kernel variant, make sure scratch is large enough, launch
static int launch(dff_model* m, DffRunArgs& a, hipStream_t stream) {
    const int N = m->cfg.n_beads, H = m->cfg.hidden;
    ON_DEVICE(m->device);
    const int mt_min = (N + 15) / 16;
    // Proteins per workgroup, by measurement (profiles/r02/packing.jsonl).  Packing only ever pays inside the padded rows a
    // protein occupies anyway: ala2 (5 beads) fits three times into its 16-row tile, and a workgroup takes the same time for
    // one as for three, so as soon as the batch exceeds one workgroup per CU (256) three per workgroup win (P = 512:
    // 120 vs 179 us / step).  Spilling into a second row tile never pays: chignolin three to a 32-row tile of the generic
    // kernel runs at 0.20-0.26 of the fp32 roof against 0.40 for one per workgroup on the <= 16-row kernel, at every batch.
    int G = m->group_override;
    const bool auto_group = G <= 0;
    const int cap = (16 * mt_min) / N;  // proteins that fit the padded rows anyway
    if (auto_group) {
        G = 1;
        if (cap > 1 && a.B > 256) G = cap;
    }
    if (G > 16) G = 16;
    int mt = (G * N + 15) / 16;
    if (mt > 4) { G = 64 / N; mt = (G * N + 15) / 16; }
    // input branches other than the shipped one run the GEN variants of the generic kernel; with absolute
    // coordinates layer 0 depends on x, so there is no layer-0 table
    const bool gen = is_gen(m->cfg);
    const bool want_tab = a.mode != DFF_MODE_SCORE && !m->l0_off && !m->cfg.use_abs_coords;
    a.l0_tab = nullptr;
    const void* sfn_; unsigned slds_; const char* snm_;
    const bool have_small = dff_small_pick(DFF_MODE_SCORE, H, 4, gen, false, &sfn_, &slds_, &snm_) ||
                            dff_small_pick(DFF_MODE_SCORE, H, 8, gen, false, &sfn_, &slds_, &snm_);   // (hidden = 256: generic kernel only)
    // Hidden 96 (ala2) and 128: the <= 16-row kernel has no split variant for them (its split engine is written for hidden 64's unit
    // counts) and is bound by the fp32 matrix pipe; the one-row-tile split_f16 variant of the <= 64-row kernel is faster
    // (round 5: 81 vs 86 us / step at 256 per GPU, 89 vs 138 at 768 -- three proteins per workgroup --, 60 vs 85 at 128, where it
    // runs as two workgroups per protein; hidden 128 at 5 / 10 / 16 rows: 90 / 150 / 157 vs 184 / 300 / 307).  DFF_SMALL_H96=1 keeps the
    // <= 16-row kernel.
    static const bool small_h96 = env_flag("DFF_SMALL_H96", '1');
    const bool prefer_generic = (H == 96 || H == 128) && m->split && !small_h96 && m->small_waves == 0;   // (dff_debug_small_waves(m, 4 | 8) asks for the <= 16-row kernel)
    if (G * N <= 16 && !m->force_generic && have_small && !prefer_generic) {
        if (want_tab) {
            int rc = ensure_l0_table(m, a.mode == DFF_MODE_DDPM ? 2 : 1, a.t_norm, G, nullptr, stream, &a.l0_tab);
            if (rc) return rc;
        }
        // Two workgroups per protein when one per protein would leave at least half the CUs idle (round 6: the reference's published
        // protocol runs 100 trajectories, evaluate/sampling_commands.md:13; config 2 over 8 GPUs is 32 per GPU) -- same conditions as
        // the <= 64-row PAIR variants below: the whole grid resident one block per CU, no failure word seen, not switched off.
        const bool spair = a.mode != DFF_MODE_SCORE && !m->pair_off && !m->sticky && pairs_fit(m, (a.B + G - 1) / G) &&
                           small_pair_available(m, a.mode, G);
        LaunchSpec s;
        const int rc = small_spec(m, a.mode, G, spair, &s);
        return rc ? rc : run(m, a, G, s, stream);
    }
    const Variant* v = nullptr;
    auto pick = [&](int mt_) {
        const Variant* r = nullptr;
        int nv = 0;
        const Variant* vs = dff_fused_variants(&nv);
        for (int q = 0; q < nv; ++q) {
            const Variant& c = vs[q];
            // (a variant must also fit the 160 KB of LDS at this row count: e.g. the four-row-tile split variant does up to
            // 56 rows -- protein G --, beyond that the fp32 engine of the same shape runs; a shape that does not fit at all
            // -- hidden 128 at 32 rows in two row tiles -- hands over to the next larger one below)
            if (c.H == H && c.MT == mt_ && c.gen == gen && !c.pair && (!c.spw || m->split) && (!r || c.spw) &&
                c.lds_floats(N, G) * sizeof(float) <= 160u * 1024u) r = &c;
        }
        return r;
    };
    auto pick_pair = [&](int mt_, bool spw_) -> const Variant* {
        int nv = 0;
        const Variant* vs = dff_fused_variants(&nv);
        for (int q = 0; q < nv; ++q)
            if (vs[q].pair && vs[q].H == H && vs[q].MT == mt_ && vs[q].spw == spw_) return &vs[q];
        return nullptr;
    };
    auto pick_up = [&](int mt0) -> const Variant* {   // the smallest shape from mt0 row tiles up that exists and fits
        for (int mt_ = mt0; mt_ <= 4; ++mt_)
            if (const Variant* r = pick(mt_)) { mt = mt_; return r; }
        return nullptr;
    };
    v = pick_up(mt);
    if (!v) {  // fall back to one protein per workgroup
        G = 1;
        v = pick_up(mt_min);
    }
    if (!v) return fail(DFF_EINVAL, "no kernel variant for hidden=%d rows=%d", H, G * N);
    // Two workgroups per protein when one per protein would leave at least half the CUs idle (protein G at 128 per GPU:
    // 1087 -> ~700 us / step).  Both blocks of a pair must be RESIDENT at once, and the launch is not cooperative: the
    // variant is used only when the whole grid fits the device's CUs one block each (hipDeviceAttributeMultiprocessorCount
    // of THIS device -- a partitioned or CU-masked GPU reports fewer than 256 and gets the one-workgroup variant), and
    // only on the conservative, shipped input branch.  A previous PAIR launch that gave up on a partner (co-tenancy: another
    // process held the CUs) is reported here, before anything else is launched on top of its garbage.  (The layer-0 table
    // below is built by the one-workgroup variant: the stash layout is the same.)
    // Proteins that share a row tile anyway (ala2: up to three in 16 rows) are paired as a GROUP: the smallest group size
    // whose pairs fit the CUs -- ala2 at 256 per GPU runs as 128 groups of two on 256 workgroups instead of 256 single
    // proteins on 256 workgroups that each do all the heads.
    const Variant* vp = nullptr;
    // (no device access here: the launch path stays asynchronous.  A failure word the HOST has seen -- an earlier PAIR launch
    // timed out waiting for its partner: the GPU is shared or partitioned -- takes the PAIR variants out of the choice: the model
    // keeps working on the one-workgroup kernels (it used to refuse every launch until dff_model_status_clear).  One
    // the host has not seen yet makes a PAIR kernel leave at entry with NaN outputs, and the next status call reports it.)
    if (m->sticky && !m->pair_off) {
        static bool said = false;
        if (!said) {
            said = true;
            fprintf(stderr, "dff: an earlier two-workgroups-per-protein launch timed out waiting for its partner workgroup (its results were "
                            "invalid and have been reported): continuing on the one-workgroup kernels; dff_model_status_clear(m) re-arms\n");
        }
    }
    if (!gen && m->cfg.conservative && !m->pair_off && !m->sticky) {
        const Variant* const cand = pick_pair(mt, v->spw);
        const int g_lo = auto_group ? 1 : G, g_hi = auto_group ? (cap > 1 ? cap : 1) : G;
        const int G0 = G;
        for (int g = g_lo; cand && g <= g_hi; ++g) {
            if (!pairs_fit(m, (a.B + g - 1) / g) || (g * N + 15) / 16 > mt || cand->lds_floats(N, g) * sizeof(float) > 160u * 1024u) continue;
            // the one-workgroup variant of the same shape builds the layer-0 table at THIS group size: it must fit there too
            // (it had been picked and LDS-checked at the old G)
            G = g;
            const Variant* const v1 = pick(mt);
            if (!v1) { G = G0; continue; }
            v = v1; vp = cand;
            break;
        }
    }
    if (want_tab) {
        int rc = ensure_l0_table(m, a.mode == DFF_MODE_DDPM ? 2 : 1, a.t_norm, G, v, stream, &a.l0_tab);
        if (rc) return rc;
    }
    LaunchSpec s;
    const int rc = generic_spec(m, G, vp ? vp : v, &s);
    return rc ? rc : run(m, a, G, s, stream);
}

extern "C" int dff_score(dff_model* m, const float* x, const float* tnorm, int batch, float* force,
                         float* energy, void* stream) {
    if (!m || !x || !tnorm || !force) return fail(DFF_EINVAL, "null argument");
    if (batch <= 0) return batch == 0 ? DFF_OK : fail(DFF_EINVAL, "negative batch");
    if (energy && !m->cfg.conservative) return fail(DFF_EINVAL, "a non-conservative model has no energy (graph_transformer.py:106-113)");
    DffRunArgs a;
    memset(&a, 0, sizeof a);
    a.mode = DFF_MODE_SCORE; a.B = batch; a.n_steps = 1;
    a.x_in = x; a.tnorm = tnorm; a.force_out = force; a.energy_out = energy;
    a.save_interval = 1;
    return launch(m, a, (hipStream_t)stream);
}

// In-kernel noise (philox_normal, dff_device.h): counter word 1 is (item >> 32) ^ (bead << 8), so the item indices offset ..
// offset + count - 1 of a call must stay below 2^40, or (item ^ (d << 40), bead) would draw what (item, bead ^ d) draws.
static bool noise_items_ok(uint64_t offset, int count) {
    const uint64_t lim = 1ull << 40;
    return offset <= lim && (uint64_t)count <= lim - offset;
}

extern "C" int dff_langevin_run(dff_model* m, const dff_langevin_params* p, int n_traj, float* x, float* v,
                                const float* noise, uint64_t seed, uint64_t traj_offset, uint64_t step_offset,
                                int n_steps, int save_interval, float* frames, float* ke, void* stream) {
    if (!m || !p || !x) return fail(DFF_EINVAL, "null argument");
    if (!p->overdamped && !v) return fail(DFF_EINVAL, "v_dev required unless overdamped");
    if (n_traj <= 0 || n_steps < 0) return fail(DFF_EINVAL, "bad sizes");
    if (!noise && !noise_items_ok(traj_offset, n_traj))
        return fail(DFF_EINVAL, "traj_offset + n_traj = %llu + %d exceeds 2^40: the in-kernel noise is keyed by 40 bits of the trajectory index",
                    (unsigned long long)traj_offset, n_traj);
    if (n_steps == 0) return DFF_OK;
    if (save_interval <= 0) save_interval = n_steps;
    // "The save_interval must be a factor of the simulation length" (langevin_cgnet.py:305-309)
    if (frames && n_steps % save_interval != 0)
        return fail(DFF_EINVAL, "The save_interval must be a factor of the simulation length");
    DffRunArgs a;
    memset(&a, 0, sizeof a);
    a.mode = DFF_MODE_LANGEVIN; a.B = n_traj; a.n_steps = n_steps;
    a.x_io = x; a.v_io = v; a.noise = noise; a.seed = seed; a.item_offset = traj_offset; a.step_offset = step_offset;
    a.t_norm = p->t_norm; a.force_scale = p->force_scale; a.dt = p->dt; a.vscale = p->vscale;
    a.noisescale = p->noisescale; a.dtau = p->dtau; a.overdamped = p->overdamped;
    a.save_interval = save_interval; a.frames = frames; a.ke = ke;
    const float inv_beta = (float)(1.0 / (double)p->beta);
    for (int i = 0; i < m->cfg.n_beads; ++i) {
        const float mass = p->masses[i];
        if (!(mass > 0.f) && !p->overdamped) return fail(DFF_EINVAL, "masses must be positive");
        a.mass[i] = mass;
        a.inv_mass[i] = 1.0f / mass;
        a.noise_sigma[i] = sqrtf(inv_beta / mass);  // torch.sqrt(1.0 / beta / masses)  :465
    }
    a.brown_sigma = (float)std::sqrt(2.0 * (double)p->dtau / (double)p->beta);  // :497
    return launch(m, a, (hipStream_t)stream);
}

extern "C" int dff_ddpm_run(dff_model* m, int batch, float* x, const float* noise, uint64_t seed,
                            uint64_t sample_offset, int t_start, int t_end, int init_prior, int* clamp_flag,
                            void* stream) {
    if (!m || !x) return fail(DFF_EINVAL, "null argument");
    if (batch <= 0) return batch == 0 ? DFF_OK : fail(DFF_EINVAL, "negative batch");
    if (t_start >= m->cfg.timesteps || t_end < 0 || t_end > t_start) return fail(DFF_EINVAL, "bad timestep range");
    if (!noise && !noise_items_ok(sample_offset, batch))
        return fail(DFF_EINVAL, "sample_offset + batch = %llu + %d exceeds 2^40: the in-kernel noise is keyed by 40 bits of the sample index",
                    (unsigned long long)sample_offset, batch);
    DffRunArgs a;
    memset(&a, 0, sizeof a);
    a.mode = DFF_MODE_DDPM; a.B = batch; a.n_steps = t_start - t_end + 1;
    a.x_io = x; a.noise = noise; a.seed = seed; a.item_offset = sample_offset;
    a.t_start = t_start; a.init_prior = init_prior; a.clamp_flag = clamp_flag; a.save_interval = 1;
    return launch(m, a, (hipStream_t)stream);
}

extern "C" int dff_debug_gemm(int device, const float* A, const float* W, int M, int K, int Nout, float* out) {
    if (!A || !W || !out || M < 1 || M > 64 || Nout % 16 || !(K == 64 || K == 128))
        return fail(DFF_EINVAL, "dff_debug_gemm: M<=64, K in {64,128}, Nout%%16==0");
    ON_DEVICE(device);
    std::vector<float> Wp = dff_prep::pack_b({K, Nout, [&](int k, int n) { return (double)W[(size_t)k * Nout + n]; }});
    float *dA, *dW, *dO;
    HIPCHK(hipMalloc((void**)&dA, (size_t)M * K * 4));
    HIPCHK(hipMalloc((void**)&dW, Wp.size() * 4));
    HIPCHK(hipMalloc((void**)&dO, (size_t)M * Nout * 4));
    HIPCHK(hipMemcpy(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dW, Wp.data(), Wp.size() * 4, hipMemcpyHostToDevice));
    const size_t lds = (size_t)(64 * (K + 4) + 64) * 4;
    HIPCHK((hipError_t)dff_debug_gemm_launch(K, dA, dW, M, Nout, dO, lds));
    HIPCHK(hipMemcpy(out, dO, (size_t)M * Nout * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dW); (void)hipFree(dO);
    return DFF_OK;
}

extern "C" int dff_debug_stash(dff_model* m, int b, int layer, int what, float* out, size_t n) {
    if (!m || !out || !m->stash || m->last_G <= 0) return fail(DFF_EINVAL, "no stash (run dff_score first)");
    if (m->last_pair) return fail(DFF_EINVAL, "the last launch split every protein over two workgroups (dff_debug_pair(m, 0) turns that off)");
    const int N = m->cfg.n_beads, H = m->cfg.hidden, L = m->cfg.n_layers, G = m->last_G;
    if (b < 0 || b >= m->last_B || layer < 0 || layer >= L) return fail(DFF_EINVAL, "bad sample / layer");
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    if (b < m->last_base) return fail(DFF_EINVAL, "sample %d was not part of the last launch (it started at %d)", b, m->last_base);
    const int wg = (b - m->last_base) / G, g = (b - m->last_base) % G;
    // both kernels stash the same per-head blocks; they differ in offsets, allocated rows and P stride
    unsigned o_nodes, o_attn, o_ff, o_hpre, o_qkv, o_P, lstride, total;
    int R, PS;
    if (m->last_small) {
        const SmallStash ss = dff_small_stash(N, G, H, L);
        o_nodes = ss.nodes_in; o_attn = ss.attn_out; o_ff = ss.ff; o_hpre = ss.h_pre; o_qkv = ss.qkv; o_P = ss.P;
        lstride = ss.layer_stride; total = ss.total;
        R = G * N + 1;   // arrays carry one dummy row
        PS = 16;
    } else {
        const StashLayout sl = dff_stash_layout(N, G, H, L, m->last_mt);
        o_nodes = sl.nodes_in; o_attn = sl.attn_out; o_ff = sl.ff; o_hpre = sl.h_pre; o_qkv = sl.qkvx; o_P = sl.P;
        lstride = sl.layer_stride; total = sl.total;
        R = G * N;
        PS = (int)sl.PS;
    }
    const int Prows = m->last_small ? 16 : R;   // rows of one head's P block
    const float* sb = m->stash + (size_t)wg * total + (size_t)layer * lstride;
    auto rowsS = [&](unsigned off, int width) -> int {
        if (n != (size_t)N * width) return fail(DFF_EINVAL, "expected %d values", N * width);
        HIPCHK(hipMemcpy(out, sb + off + (size_t)g * N * width, (size_t)N * width * 4, hipMemcpyDeviceToHost));
        return DFF_OK;
    };
    auto heads = [&](int c0, int w, int dstw) -> int {
        // per head h: rows (g*N .. g*N+N) x [c0, c0+w) of its (R x 208) block -> out[row][h*w ..]
        std::vector<float> tmp((size_t)N * DFF_QKVW);
        for (int h = 0; h < DFF_HEADS; ++h) {
            HIPCHK(hipMemcpy(tmp.data(), sb + o_qkv + ((size_t)h * R + (size_t)g * N) * DFF_QKVW, tmp.size() * 4, hipMemcpyDeviceToHost));
            for (int r = 0; r < N; ++r)
                for (int c2 = 0; c2 < w; ++c2) out[(size_t)r * dstw + h * w + c2] = tmp[(size_t)r * DFF_QKVW + c0 + c2];
        }
        return DFF_OK;
    };
    switch (what) {
        case 0: return rowsS(o_nodes, H);
        case 1: return rowsS(o_attn, H);
        case 2: return rowsS(o_ff, H);
        case 3: return rowsS(o_hpre, 4 * H);
        case 4: if (n != (size_t)N * 512) return fail(DFF_EINVAL, "size"); return heads(0, 64, 512);
        case 5: if (n != (size_t)N * 512) return fail(DFF_EINVAL, "size"); return heads(80, 64, 512);
        case 6: if (n != (size_t)N * 512) return fail(DFF_EINVAL, "size"); return heads(144, 64, 512);
        case 8: {
            if (n != (size_t)N * 32) return fail(DFF_EINVAL, "size");
            memset(out, 0, n * 4);
            return heads(64, 3, 32);
        }
        case 7: {
            if (n != (size_t)DFF_HEADS * N * N) return fail(DFF_EINVAL, "size");
            std::vector<float> tmp((size_t)N * PS);
            for (int h = 0; h < DFF_HEADS; ++h) {
                HIPCHK(hipMemcpy(tmp.data(), sb + o_P + ((size_t)h * Prows + (size_t)g * N) * PS, tmp.size() * 4, hipMemcpyDeviceToHost));
                for (int i = 0; i < N; ++i)
                    for (int j = 0; j < N; ++j) out[((size_t)h * N + i) * N + j] = tmp[(size_t)i * PS + g * N + j];
            }
            return DFF_OK;
        }
    }
    return fail(DFF_EINVAL, "unknown stash item %d", what);
}

extern "C" int dff_debug_profile(dff_model* m, int enable) {
    if (!m) return fail(DFF_EINVAL, "null model");
#if !DFF_PROF
    if (enable) return fail(DFF_EINVAL, "this library was built without the stage ticks (./build.sh with DFF_EXTRA_FLAGS=-DDFF_PROF=1)");
#endif
    ON_DEVICE(m->device);
    if (enable && !m->prof) {
        HIPCHK(hipMalloc((void**)&m->prof, DFF_NPROF * sizeof(unsigned long long)));
        HIPCHK(hipMemset(m->prof, 0, DFF_NPROF * sizeof(unsigned long long)));
    }
    m->prof_on = enable != 0;
    m->prof_wave = enable > 1 ? enable - 1 : 0;   // enable = 1 + wave whose view is recorded (<= 16-row kernel)
    if (enable) HIPCHK(hipMemset(m->prof, 0, DFF_NPROF * sizeof(unsigned long long)));
    return DFF_OK;
}

extern "C" int dff_debug_profile_read(dff_model* m, unsigned long long* out) {
    if (!m || !out || !m->prof) return fail(DFF_EINVAL, "profiling was never enabled");
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, m->prof, DFF_NPROF * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return DFF_OK;
}

extern "C" const char* dff_last_error(void) { return g_err.c_str(); }
// DFF_SRC_SHA (build.sh): sha256 over csrc/* + include/dff.h, 16 hex digits -- ties rocprof evidence to the code it profiled
#ifndef DFF_SRC_SHA
#define DFF_SRC_SHA unknown
#endif
#define DFF_STR2(x) #x
#define DFF_STR(x) DFF_STR2(x)
// DFF_BUILD_FLAGS (build.sh, generated header): DFF_EXTRA_FLAGS / scheduler overrides the translation units were compiled with -- a
// development build names its knobs; they are hashed into DFF_SRC_SHA as well, so that it never shares the product build's hash.
#ifndef DFF_BUILD_FLAGS
#define DFF_BUILD_FLAGS ""
#endif
extern "C" const char* dff_version(void) {
    return "dff-amd 0.1 (gfx950; f16-split / f32 MFMA) flags=[" DFF_BUILD_FLAGS "] src=" DFF_STR(DFF_SRC_SHA);
}
