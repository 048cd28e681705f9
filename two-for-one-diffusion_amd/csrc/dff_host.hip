// dff_host.hip -- host half of libdff_amd.so: the model handle (upload of the images dff_prep.hip prepares), scratch
// management, kernel dispatch and the model's part of the extern "C" ABI declared in include/dff.h
// (the stateless sample-analysis entry points are the dff_an_*.hip units).
#include "../../include/dff.h"
#include "dff_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// the two sampler kernels are their own translation units (dff_kernels.hip, dff_small.hip: they export variant
// lookups, dff_device.h); the sample-analysis entry points and their kernels are units of their own, one per group of families (dff_an_*.hip)
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

// Everything kernel selection reads of a model, and nothing else: the config, the engines weight preparation chose (split: fp16
// images exist, SPW variants preferred -- DFF_SPLIT_BF16=0 at model creation: never; small_split: ... and the <= 16-row kernel has
// an SPW variant for this model; fold_kv: H == 64: k = v = LayerNorm output, W_k folded into W_q, W_v into W_o -- DFF_FOLD_KV=0:
// never), n_cus (hipDeviceAttributeMultiprocessorCount of the model's device), the knobs (group_override; small_waves: 0 auto, 4:
// never use the 8-wave variant; max_wgs: workgroups per launch, bounds the stash (grid x stash slot) for big batches; debugging:
// force_generic: never use the rows<=16 fast path, l0_off: never use the layer-0 table, pair_off: never use a PAIR variant),
// sticky (the sticky error word as the host last read it (read_status): a non-zero one refuses further PAIR launches WITHOUT
// touching the device) and the two environment opt-ins launch() reads.  The fields of the ABI's dff_dispatch, plus the config.
struct Dispatch : dff_dispatch {
    dff_config cfg;
};
// what the last launch was: dff_last_launch, and the stash layout of the debug reads (dff_debug_stash)
struct LaunchRecord {
    const char* kernel = "";
    int grid = 0, lds = 0, G = 0, B = 0, base = 0;
    int mt = 1;                                // row tiles of the <= 64-row variant that ran
    bool small = false, pair = false;          // the <= 16-row kernel; two workgroups per protein
};

// ------------------------------------------------------------------------------------------
// model handle
// ------------------------------------------------------------------------------------------
struct dff_model {
    Dispatch d = {};
    LaunchRecord last;
    int device;
    DffModelDev dev;
    std::vector<void*> allocs;
    std::vector<std::vector<float>> sched;  // 12 tables, host fp32
    float* stash = nullptr;
    size_t stash_floats = 0;
    unsigned long long* prof = nullptr;
    bool prof_on = false;
    int prof_wave = 0;
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
    // PAIR variants (two workgroups per protein): partial-tile exchange slots and flags
    float* xchg = nullptr;
    size_t xchg_floats = 0;
    unsigned* xflag = nullptr;
    size_t xflag_n = 0;
    int pair_slow = 0;                         // tests: 1 = PAIR variants always run the cross-XCD (agent-scope) exchange protocol; 2 = partners are
                                               // ADJACENT blocks (different XCDs under round-robin placement), protocol chosen by the handshake
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

// is there a <= 16-row kernel of this shape in the build (dff_small_pick without its outputs)
static bool small_exists(int mode, int H, int NW, bool gen, bool spw, bool fold = false, bool pair = false) {
    const void* fn; unsigned lds; const char* name;
    return dff_small_pick(mode, H, NW, gen, spw, &fn, &lds, &name, fold, pair);
}
// ... and a split (SPW) one for this model: what weight preparation is told, and what Dispatch::small_split then says
static bool small_split_exists(const dff_config& c) { return c.n_beads <= 10 && small_exists(DFF_MODE_SCORE, c.hidden, 8, false, true); }

// the configurations this build has kernels for (dff_model_create, dff_debug_plan_launch)
static int check_config(const dff_config* cfg) {
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
    return DFF_OK;
}

extern "C" int dff_model_create(const dff_config* cfg, const float* w, size_t n_weights, int device,
                                dff_model** out) {
    if (!cfg || !w || !out) return fail(DFF_EINVAL, "null argument");
    if (int rc = check_config(cfg)) return rc;
    const int H = cfg->hidden, N = cfg->n_beads, L = cfg->n_layers;
    if (n_weights != dff_weight_count(cfg))
        return fail(DFF_EINVAL, "expected %zu weights, got %zu", dff_weight_count(cfg), n_weights);
    ON_DEVICE(device);
    dff_model* m = new dff_model();
    struct Undo {   // any failure below frees what was uploaded so far
        dff_model* m;
        ~Undo() { if (m) dff_model_destroy(m); }
    } undo{m};
    m->d.cfg = *cfg;
    m->d.max_wgs = 2048;
    m->device = device;
    HIPCHK(hipDeviceGetAttribute(&m->d.n_cus, hipDeviceAttributeMultiprocessorCount, device));
    // weight GEMMs on the fp16 pipe (default) unless DFF_SPLIT_BF16=0: every GEMM on v_mfma_f32_16x16x4_f32; DFF_FOLD_KV=0: no k / v
    // fold.  The range guard (dff_prep.hip) has the last word on the engine, and says so on stderr.
    dff_prep::DffPrep p = dff_prep::dff_prepare(*cfg, w, !env_flag("DFF_SPLIT_BF16", '0'), !env_flag("DFF_FOLD_KV", '0'), small_split_exists(*cfg));
    fputs(p.note.c_str(), stderr);
    m->d.split = p.split; m->d.small_split = p.small_split; m->d.fold_kv = p.fold_kv;
    // Two workgroups per protein (PAIR variants) need both blocks of a pair resident at once, and the launches are not cooperative
    // (ADVICE r05): never where the GPU is known to be shared -- more local ranks than visible devices (torchrun's
    // LOCAL_WORLD_SIZE) -- or where the caller says so (DFF_PAIR=0).  dff_debug_pair(m, 1) turns them back on.
    const char* lw = getenv("LOCAL_WORLD_SIZE");
    int ndev = 0;
    if (env_flag("DFF_PAIR", '0')) m->d.pair_off = true;
    else if (lw && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && atoi(lw) > ndev) {
        m->d.pair_off = true;
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
    v->device = m->device; v->n_beads = m->d.cfg.n_beads; v->timesteps = m->d.cfg.timesteps;
    v->sqrt_ac = m->sqrt_ac; v->sqrt_1mac = m->sqrt_1mac;
    return DFF_OK;
}

extern "C" int dff_set_group(dff_model* m, int g) {
    if (!m || g < 0) return fail(DFF_EINVAL, "bad group");
    m->d.group_override = g;
    return DFF_OK;
}

extern "C" int dff_debug_force_generic(dff_model* m, int on) {
    if (!m) return fail(DFF_EINVAL, "null model");
    m->d.force_generic = on != 0;
    return DFF_OK;
}

extern "C" int dff_debug_max_workgroups(dff_model* m, int n) {
    if (!m || n < 1) return fail(DFF_EINVAL, "bad workgroup limit");
    m->d.max_wgs = n;
    return DFF_OK;
}

static int clear_status(dff_model* m);
extern "C" int dff_debug_pair(dff_model* m, int on) {
    if (!m) return fail(DFF_EINVAL, "null model");
    m->d.pair_off = on == 0;
    m->pair_slow = on == 2 ? 1 : on == 3 ? 2 : 0;
    // turning the PAIR variants off is how a caller recovers from a partner timeout: the one-workgroup kernels do not look
    // at the word, so it is cleared here (it would otherwise fail every later status check of a model that works again)
    // (unconditionally -- ADVICE r04: the DEVICE word may be set before the host has looked at it; clear_status synchronises,
    // which a debug / recovery call may do)
    if (m->d.pair_off && m->xflag) return clear_status(m);
    return DFF_OK;
}

// Sticky status of the model's launches so far: bit 0 = a PAIR launch (two workgroups per protein) gave up waiting for a
// partner workgroup (bounded spin instead of a hang; the results of that launch are invalid).  The word lives at
// xflag[0], is only ever OR-ed by the kernels and is never cleared by a launch, so an error in ANY launch of a chunked
// run is still there when the caller looks.  Synchronises the device -- which is why only the status calls come here: the
// launch path never does (a PAIR kernel that finds the word set at entry leaves at once, and plan_launch refuses PAIR on the
// host's cached copy), so dff_score / dff_langevin_run / dff_ddpm_run stay asynchronous on the caller's stream.
static int read_status(dff_model* m, unsigned* word, bool clear) {
    *word = 0;
    if (!m->xflag) return DFF_OK;
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(word, m->xflag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (clear && *word) HIPCHK(hipMemset(m->xflag, 0, sizeof(unsigned)));
    m->d.sticky = clear ? 0 : (int32_t)*word;
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
    m->d.l0_off = on == 0;
    return DFF_OK;
}

extern "C" int dff_debug_small_waves(dff_model* m, int waves) {
    if (!m || !(waves == 0 || waves == 4 || waves == 8)) return fail(DFF_EINVAL, "waves must be 0 (auto), 4 or 8");
    m->d.small_waves = waves;
    return DFF_OK;
}

extern "C" int dff_last_launch(const dff_model* m, const char** name, int* grid, int* lds) {
    if (!m) return fail(DFF_EINVAL, "null model");
    if (name) *name = m->last.kernel;
    if (grid) *grid = m->last.grid;
    if (lds) *lds = m->last.lds;
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

// ------------------------------------------------------------------------------------------
// kernel selection: Dispatch -> plan_launch -> LaunchPlan.  Pure host arithmetic over the variant tables of the kernel units:
// nothing from here to run() touches the device, the environment or stderr (dff_debug_plan_launch runs it without a GPU).
// ------------------------------------------------------------------------------------------
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
struct LaunchPlan {
    int G;                        // proteins per workgroup
    LaunchSpec spec;              // the kernel to run
    int grid_all, grid_max;       // workgroups in all, and per launch
    int table;                    // the sampling loop reads a layer-0 table (ensure_l0_table): 0 none, 1 one entry, 2 one per level ...
    const Variant* tab_variant;   // ... built by this variant of the <= 64-row kernel; null: by the <= 16-row kernel
};

static const unsigned LDS_MAX = 160u * 1024u;
static int n_groups(int B, int G) { return B / G + (B % G != 0); }                      // (no B + G - 1: B may be INT_MAX)
static long long pair_grid(int ngroups) { return 2 * 8 * ((ngroups + 7ll) / 8); }   // PAIR: 16 blocks per 8 groups
static int row_tiles(int rows) { return (rows + 15) / 16; }

// Two workgroups per protein need both blocks of a pair RESIDENT at once, and the launch is not cooperative: a PAIR grid (blocks b
// and b + 8 share a protein, 16 blocks per 8 groups) must fit the device's CUs one block each, in ONE launch
static bool pairs_fit(const Dispatch& d, int ngroups) {
    return pair_grid(ngroups) <= (d.n_cus < d.max_wgs ? d.n_cus : d.max_wgs);
}

// rows <= 16: one-head-per-wave kernel (dff_small.hip)
static int small_spec(const Dispatch& d, int mode, int G, bool pair, LaunchSpec* s) {
    const int N = d.cfg.n_beads, H = d.cfg.hidden;
    // 8 waves (two per SIMD, one head per wave) when the rows fit its 11-row head buffers
    const bool eight = (H == 64 || H == 96) && G * N <= 10 && d.small_waves != 4;
    const int NW = eight ? 8 : 4;
    if (!dff_small_pick(mode, H, NW, is_gen(d.cfg), eight && d.small_split, &s->fn, &s->lds, &s->name, d.fold_kv, pair))
        return fail(DFF_EINVAL, "no <= 16-row kernel for hidden=%d waves=%d in this build", H, NW);
    s->lds *= (unsigned)sizeof(float);
    if (s->lds > LDS_MAX) return fail(DFF_EINVAL, "LDS budget exceeded (%u bytes)", s->lds);
    const SmallStash sl = dff_small_stash(N, G, H, d.cfg.n_layers);
    s->nthreads = pair ? 256 : NW * 64; s->pair = pair; s->small = true; s->mt = 1; s->prof_waves = NW;
    s->stash = sl.total; s->layer_stride = sl.layer_stride;
    s->xchg = 4 * 1024;   // [half][parity][256 threads x 4 floats]
    return DFF_OK;
}
// generic kernel (rows <= 64), variant already chosen
static int generic_spec(const Dispatch& d, int G, const Variant* v, LaunchSpec* s) {
    const int N = d.cfg.n_beads, H = d.cfg.hidden;
    s->lds = v->lds_floats(N, G) * (unsigned)sizeof(float);
    if (s->lds > LDS_MAX) return fail(DFF_EINVAL, "LDS budget exceeded (%u bytes) for N=%d G=%d H=%d", s->lds, N, G, H);
    const StashLayout sl = dff_stash_layout(N, G, H, d.cfg.n_layers, v->MT);
    s->fn = v->fn; s->name = v->name; s->nthreads = DFF_NTHREADS; s->pair = v->pair; s->small = false; s->mt = v->MT; s->prof_waves = 0;
    s->stash = sl.total; s->layer_stride = sl.layer_stride;
    s->xchg = 4 * (size_t)(G * N) * (H + 4);   // [half][parity][rows x (H + 4)]
    return DFF_OK;
}
// The plan of one chosen kernel over B proteins, G to a workgroup -- v: that variant of the <= 64-row kernel, null: the <= 16-row
// kernel of `mode`, `small_pair` its two-workgroups form.  Where plan_launch ends, and what builds a layer-0 table (ensure_l0_table).
static int plan_variant(const Dispatch& d, int mode, int B, int G, const Variant* v, bool small_pair, LaunchPlan* p) {
    if (int rc = v ? generic_spec(d, G, v, &p->spec) : small_spec(d, mode, G, small_pair, &p->spec)) return rc;
    p->G = G;
    // PAIR: (a pair shares a GROUP of G proteins: ala2 two or three to a 16-row tile), ONE launch -- pairs_fit
    // has been checked (so a PAIR grid is the single pass w0 = 0 of run()'s loop: b_base = w0 * G is the 0 the <= 16-row PAIR kernel expects)
    p->grid_all = p->spec.pair ? (int)pair_grid(n_groups(B, G)) : n_groups(B, G);
    p->grid_max = p->spec.pair || p->grid_all < d.max_wgs ? p->grid_all : d.max_wgs;
    return DFF_OK;
}

// the <= 64-row variants of the model's hidden size and input branch
static const Variant* pick(const Dispatch& d, int mt, int G) {   // the one-workgroup variant of mt row tiles, split engine first
    const Variant* r = nullptr;
    int nv = 0;
    const Variant* vs = dff_fused_variants(&nv);
    for (int q = 0; q < nv; ++q) {
        const Variant& c = vs[q];
        // (a variant must also fit the 160 KB of LDS at this row count: e.g. the four-row-tile split variant does up to
        // 56 rows -- protein G --, beyond that the fp32 engine of the same shape runs; a shape that does not fit at all
        // -- hidden 128 at 32 rows in two row tiles -- hands over to the next larger one in pick_up)
        if (c.H == d.cfg.hidden && c.MT == mt && c.gen == is_gen(d.cfg) && !c.pair && (!c.spw || d.split) && (!r || c.spw) &&
            c.lds_floats(d.cfg.n_beads, G) * sizeof(float) <= LDS_MAX) r = &c;
    }
    return r;
}
static const Variant* pick_up(const Dispatch& d, int mt0, int G) {   // the smallest shape from mt0 row tiles up that exists and fits
    for (int mt = mt0; mt <= 4; ++mt)
        if (const Variant* r = pick(d, mt, G)) return r;
    return nullptr;
}
static const Variant* pick_pair(const Dispatch& d, int mt, bool spw) {
    int nv = 0;
    const Variant* vs = dff_fused_variants(&nv);
    for (int q = 0; q < nv; ++q)
        if (vs[q].pair && vs[q].H == d.cfg.hidden && vs[q].MT == mt && vs[q].spw == spw) return &vs[q];
    return nullptr;
}

// choose proteins-per-workgroup and the kernel variant for a call of `mode` over B proteins
static int plan_launch(const Dispatch& d, int mode, int B, LaunchPlan* p) {
    const int N = d.cfg.n_beads, H = d.cfg.hidden;
    const int mt_min = row_tiles(N);
    // Proteins per workgroup, by measurement (profiles/r02/packing.jsonl).  Packing only ever pays inside the padded rows a
    // protein occupies anyway: ala2 (5 beads) fits three times into its 16-row tile, and a workgroup takes the same time for
    // one as for three, so as soon as the batch exceeds one workgroup per CU (256) three per workgroup win (P = 512:
    // 120 vs 179 us / step).  Spilling into a second row tile never pays: chignolin three to a 32-row tile of the generic
    // kernel runs at 0.20-0.26 of the fp32 roof against 0.40 for one per workgroup on the <= 16-row kernel, at every batch.
    const bool auto_group = d.group_override <= 0;
    const int cap = (16 * mt_min) / N;  // proteins that fit the padded rows anyway
    const int G_asked = auto_group ? (cap > 1 && B > 256 ? cap : 1) : d.group_override;
    const int G_16 = G_asked > 16 ? 16 : G_asked;
    const int G0 = row_tiles(G_16 * N) > 4 ? 64 / N : G_16;
    // input branches other than the shipped one run the GEN variants of the generic kernel; with absolute
    // coordinates layer 0 depends on x, so there is no layer-0 table
    const bool gen = is_gen(d.cfg);
    p->table = mode == DFF_MODE_SCORE || d.l0_off || d.cfg.use_abs_coords ? 0 : mode == DFF_MODE_DDPM ? 2 : 1;
    p->tab_variant = nullptr;
    const bool have_small = small_exists(DFF_MODE_SCORE, H, 4, gen, false) || small_exists(DFF_MODE_SCORE, H, 8, gen, false);   // (hidden = 256: generic kernel only)
    // Hidden 96 (ala2) and 128: the <= 16-row kernel has no split variant for them (its split engine is written for hidden 64's unit
    // counts) and is bound by the fp32 matrix pipe; the one-row-tile split_f16 variant of the <= 64-row kernel is faster
    // (round 5: 81 vs 86 us / step at 256 per GPU, 89 vs 138 at 768 -- three proteins per workgroup --, 60 vs 85 at 128, where it
    // runs as two workgroups per protein; hidden 128 at 5 / 10 / 16 rows: 90 / 150 / 157 vs 184 / 300 / 307).  DFF_SMALL_H96=1 keeps the
    // <= 16-row kernel.
    const bool prefer_generic = (H == 96 || H == 128) && d.split && !d.small_h96 && d.small_waves == 0;   // (dff_debug_small_waves(m, 4 | 8) asks for the <= 16-row kernel)
    // A failure word the HOST has seen -- an earlier PAIR launch timed out waiting for its partner: the GPU is shared or partitioned --
    // takes the PAIR variants out of the choice, here and below: the model keeps working on the one-workgroup kernels (it
    // used to refuse every launch until dff_model_status_clear).  One the host has not seen yet makes a PAIR kernel leave at entry
    // with NaN outputs, and the next status call reports it.  (No device access: the launch path stays asynchronous.)
    const bool pair_allowed = !d.pair_off && !d.sticky;
    if (G0 * N <= 16 && !d.force_generic && have_small && !prefer_generic) {
        // Two workgroups per protein when one per protein would leave at least half the CUs idle (round 6: the reference's published
        // protocol runs 100 trajectories, evaluate/sampling_commands.md:13; config 2 over 8 GPUs is 32 per GPU) -- same conditions as
        // the <= 64-row PAIR variants below: the whole grid resident one block per CU, no failure word seen, not switched off.
        // OPT-IN (DFF_SMALL_PAIR=1, read per launch): built and measured in round 6 -- chignolin at 128 / 100 / 32 per GPU 45.8 / 45.9 / 45.4 us
        // per step against 44.4 with one workgroup per protein.  The wave-private blocks do shrink (-19 k cycles per step: four waves,
        // one per SIMD), but each of the 12 exchanges costs ~1.8 k cycles inside its row stage -- a store's s_waitcnt vmcnt(0) also
        // waits for the weight units the wave has just requested for the next block (loads and stores retire through one in-order
        // counter), 0.25 - 0.45 us in tools_ubench/pair_exchange.hip without that -- and the 16-lanes-per-row stages issue more per thread
        // (profiles/r06/pair_small/).  Kept as a tested variant; not the default.
        const bool spair = mode != DFF_MODE_SCORE && pair_allowed && pairs_fit(d, n_groups(B, G0)) && d.small_pair && H == 64 &&
                           G0 * N <= 10 && d.small_waves == 0 && d.small_split && d.fold_kv && !gen && d.cfg.conservative &&
                           small_exists(mode, H, 8, false, true, true, true);
        return plan_variant(d, mode, B, G0, nullptr, spair, p);
    }
    const Variant* const v0 = pick_up(d, row_tiles(G0 * N), G0);
    const int G1 = v0 ? G0 : 1;   // fall back to one protein per workgroup
    const Variant* const v1 = v0 ? v0 : pick_up(d, mt_min, 1);
    if (!v1) return fail(DFF_EINVAL, "no kernel variant for hidden=%d rows=%d", H, G1 * N);
    // Two workgroups per protein when one per protein would leave at least half the CUs idle (protein G at 128 per GPU:
    // 1087 -> ~700 us / step).  Both blocks of a pair must be RESIDENT at once, and the launch is not cooperative: the
    // variant is used only when the whole grid fits the device's CUs one block each (hipDeviceAttributeMultiprocessorCount
    // of THIS device -- a partitioned or CU-masked GPU reports fewer than 256 and gets the one-workgroup variant), and
    // only on the conservative, shipped input branch.  A previous PAIR launch that gave up on a partner (co-tenancy: another
    // process held the CUs) is reported by launch(), before anything else is launched on top of its garbage.  (The layer-0 table
    // is built by the one-workgroup variant: the stash layout is the same.)
    // Proteins that share a row tile anyway (ala2: up to three in 16 rows) are paired as a GROUP: the smallest group size
    // whose pairs fit the CUs -- ala2 at 256 per GPU runs as 128 groups of two on 256 workgroups instead of 256 single
    // proteins on 256 workgroups that each do all the heads.
    const Variant* const cand = !gen && d.cfg.conservative && pair_allowed ? pick_pair(d, v1->MT, v1->spw) : nullptr;
    const int g_lo = auto_group ? 1 : G1, g_hi = auto_group ? (cap > 1 ? cap : 1) : G1;
    for (int g = g_lo; cand && g <= g_hi; ++g) {
        if (!pairs_fit(d, n_groups(B, g)) || row_tiles(g * N) > v1->MT || cand->lds_floats(N, g) * sizeof(float) > LDS_MAX) continue;
        // the one-workgroup variant of the same shape builds the layer-0 table at THIS group size: it must fit there too
        // (it had been picked and LDS-checked at the old G)
        if (const Variant* const vt = pick(d, v1->MT, g)) {
            p->tab_variant = vt;
            return plan_variant(d, mode, B, g, cand, false, p);
        }
    }
    p->tab_variant = v1;
    return plan_variant(d, mode, B, G1, v1, false, p);
}

// one launch path for both kernels: stash, PAIR buffers, the launches, the LaunchRecord
static int run(dff_model* m, DffRunArgs& a, const LaunchPlan& p, hipStream_t stream) {
    const LaunchSpec& s = p.spec;
    const int npairs = s.pair ? p.grid_all / 2 : 0;
    int rc = grow(m->stash, m->stash_floats, (size_t)p.grid_max * s.stash);
    if (rc) return rc;
    a.xchg = nullptr; a.xflag = nullptr; a.xpairs = npairs; a.xslow = m->pair_slow;
    if (s.pair) {
        // the exchange slots and the flag words -- error word, [pair][half] sequence flags, [pair][half] XCD ids; the sequence
        // numbers restart at every launch, the error word at [0] is NOT touched
        const size_t nflag = (size_t)4 * npairs + 1;
        if ((rc = grow(m->xchg, m->xchg_floats, (size_t)npairs * s.xchg))) return rc;
        if (!m->xflag) {   // once per model, sized for the largest grid a PAIR launch can have (one block per CU): no
                           // re-allocation -- and so no synchronisation -- on the launch path afterwards
            const size_t cap = 2 * (size_t)(m->d.n_cus > 256 ? m->d.n_cus : 256) + 1;   // 4 words per pair, at most n_cus / 2 pairs
            HIPCHK(hipMalloc((void**)&m->xflag, cap * sizeof(unsigned)));
            HIPCHK(hipMemsetAsync(m->xflag, 0, sizeof(unsigned), stream));
            m->xflag_n = cap;
        }
        if (nflag > m->xflag_n) return fail(DFF_EINVAL, "PAIR grid of %d pairs exceeds the flag array", npairs);
        HIPCHK(hipMemsetAsync(m->xflag + 1, 0, (nflag - 1) * sizeof(unsigned), stream));
        a.xchg = m->xchg; a.xflag = m->xflag;
    }
    a.G = p.G;
    a.prof = m->prof_on ? m->prof : nullptr;
    a.prof_wave = m->prof_wave < s.prof_waves ? m->prof_wave : 0;
    a.stash = m->stash;
    a.stash_stride = s.stash;
    HIPCHK(hipFuncSetAttribute(s.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
    LaunchRecord& r = m->last;
    r.kernel = s.name; r.lds = (int)s.lds; r.G = p.G; r.B = a.B; r.mt = s.mt; r.small = s.small; r.pair = s.pair;
    // independent proteins: a batch larger than max_wgs workgroups runs as consecutive launches (same stream,
    // same stash), each over the whole step range
    for (int w0 = 0; w0 < p.grid_all; w0 += p.grid_max) {
        const int grid = p.grid_all - w0 < p.grid_max ? p.grid_all - w0 : p.grid_max;
        a.b_base = w0 * p.G;
        void* args[] = {(void*)&m->dev, (void*)&a};
        HIPCHK(hipLaunchKernel(s.fn, dim3(grid), dim3(s.nthreads), args, s.lds, stream));
        r.grid = grid; r.base = a.b_base;
        a.prof = nullptr;   // per-stage cycles: first launch only
    }
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
    const int N = m->d.cfg.n_beads, T = m->d.cfg.timesteps;
    dff_model::L0Table* slot = nullptr;
    for (auto& c : m->l0[kind - 1]) {
        if (c.valid && c.G == G && c.waves == m->d.small_waves && c.variant == (const void*)v && c.split == m->d.small_split &&
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
    int CH = nent < 256 ? nent : 256;         // noise levels (= workgroups) per build launch ...
    if (CH > m->d.max_wgs) CH = m->d.max_wgs; // ... each of which must be ONE kernel launch (its stash is copied out)
    const int Bmax = CH * G;
    LaunchPlan p;
    int rc = plan_variant(m->d, DFF_MODE_SCORE, Bmax, G, v, false, &p);
    if (rc) return rc;
    const size_t layer_stride = p.spec.layer_stride, total = p.spec.stash;
    if ((rc = grow(tb.tab, tb.floats, (size_t)nent * layer_stride))) return rc;
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
        p.grid_all = p.grid_max = ne;   // one workgroup per level of this chunk
        if ((rc = run(m, a, p, stream))) return rc;
        // only the layer-0 slot of each workgroup's stash is kept
        HIPCHK(hipMemcpy2DAsync(tb.tab + (size_t)e0 * layer_stride, layer_stride * sizeof(float), m->stash,
                                total * sizeof(float), layer_stride * sizeof(float), (size_t)ne,
                                hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    tb.valid = true; tb.G = G; tb.waves = m->d.small_waves; tb.tnorm = t_norm; tb.variant = (const void*)v; tb.split = m->d.small_split;
    tb.used = ++m->l0_clock;
    *out = tb.tab;
    return DFF_OK;
}

// the two environment opt-ins of Dispatch: DFF_SMALL_PAIR=1 is read at every launch, DFF_SMALL_H96=1 once per process
static void read_opt_ins(dff_dispatch* d) {
    static const bool small_h96 = env_flag("DFF_SMALL_H96", '1');
    d->small_pair = env_flag("DFF_SMALL_PAIR", '1');
    d->small_h96 = small_h96;
}

// plan the call, make sure the layer-0 table the plan wants exists, launch
static int launch(dff_model* m, DffRunArgs& a, hipStream_t stream) {
    ON_DEVICE(m->device);
    read_opt_ins(&m->d);
    LaunchPlan p;
    int rc = plan_launch(m->d, a.mode, a.B, &p);
    if (rc) return rc;
    if (m->d.sticky && !m->d.pair_off && !p.spec.small) {
        static bool said = false;
        if (!said) {
            said = true;
            fprintf(stderr, "dff: an earlier two-workgroups-per-protein launch timed out waiting for its partner workgroup (its results were "
                            "invalid and have been reported): continuing on the one-workgroup kernels; dff_model_status_clear(m) re-arms\n");
        }
    }
    a.l0_tab = nullptr;
    if (p.table && (rc = ensure_l0_table(m, p.table, a.t_norm, p.G, p.tab_variant, stream, &a.l0_tab))) return rc;
    return run(m, a, p, stream);
}

// host only: the model's Dispatch as the next launch would see it
extern "C" int dff_debug_dispatch(const dff_model* m, dff_dispatch* out) {
    if (!m || !out) return fail(DFF_EINVAL, "null argument");
    *out = m->d;
    read_opt_ins(out);
    return DFF_OK;
}

// host only, no GPU: plan_launch without a handle
extern "C" int dff_debug_plan_launch(const dff_config* cfg, const dff_dispatch* k, int mode, int batch, dff_launch_plan* out) {
    if (!cfg || !k || !out) return fail(DFF_EINVAL, "null argument");
    if (int rc = check_config(cfg)) return rc;
    if (mode < DFF_MODE_SCORE || mode > DFF_MODE_DDPM || batch < 1 || k->max_wgs < 1 || k->group_override < 0 ||
        !(k->small_waves == 0 || k->small_waves == 4 || k->small_waves == 8))
        return fail(DFF_EINVAL, "plan_launch: mode must be 0..2, batch and max_wgs >= 1, group_override >= 0, small_waves 0, 4 or 8");
    Dispatch d;
    static_cast<dff_dispatch&>(d) = *k;
    d.cfg = *cfg;
    LaunchPlan p, t;
    if (int rc = plan_launch(d, mode, batch, &p)) return rc;
    out->table_kernel = "";
    if (p.table) {
        if (int rc = plan_variant(d, DFF_MODE_SCORE, p.G, p.G, p.tab_variant, false, &t)) return rc;
        out->table_kernel = t.spec.name;
    }
    out->kernel = p.spec.name; out->G = p.G; out->workgroups = p.grid_all;
    out->launches = (p.grid_all - 1) / p.grid_max + 1;
    out->last_grid = p.grid_all - (out->launches - 1) * p.grid_max;
    out->lds_bytes = (int)p.spec.lds; out->threads = p.spec.nthreads; out->pair = p.spec.pair; out->table = p.table;
    return DFF_OK;
}

extern "C" int dff_score(dff_model* m, const float* x, const float* tnorm, int batch, float* force,
                         float* energy, void* stream) {
    if (!m || !x || !tnorm || !force) return fail(DFF_EINVAL, "null argument");
    if (batch <= 0) return batch == 0 ? DFF_OK : fail(DFF_EINVAL, "negative batch");
    if (energy && !m->d.cfg.conservative) return fail(DFF_EINVAL, "a non-conservative model has no energy (graph_transformer.py:106-113)");
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
    for (int i = 0; i < m->d.cfg.n_beads; ++i) {
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
    if (t_start >= m->d.cfg.timesteps || t_end < 0 || t_end > t_start) return fail(DFF_EINVAL, "bad timestep range");
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
    if (!m || !out || !m->stash || m->last.G <= 0) return fail(DFF_EINVAL, "no stash (run dff_score first)");
    if (m->last.pair) return fail(DFF_EINVAL, "the last launch split every protein over two workgroups (dff_debug_pair(m, 0) turns that off)");
    const int N = m->d.cfg.n_beads, H = m->d.cfg.hidden, L = m->d.cfg.n_layers, G = m->last.G;
    if (b < 0 || b >= m->last.B || layer < 0 || layer >= L) return fail(DFF_EINVAL, "bad sample / layer");
    ON_DEVICE(m->device);
    HIPCHK(hipDeviceSynchronize());
    if (b < m->last.base) return fail(DFF_EINVAL, "sample %d was not part of the last launch (it started at %d)", b, m->last.base);
    const int wg = (b - m->last.base) / G, g = (b - m->last.base) % G;
    // both kernels stash the same per-head blocks; they differ in offsets, allocated rows and P stride
    unsigned o_nodes, o_attn, o_ff, o_hpre, o_qkv, o_P, lstride, total;
    int R, PS;
    if (m->last.small) {
        const SmallStash ss = dff_small_stash(N, G, H, L);
        o_nodes = ss.nodes_in; o_attn = ss.attn_out; o_ff = ss.ff; o_hpre = ss.h_pre; o_qkv = ss.qkv; o_P = ss.P;
        lstride = ss.layer_stride; total = ss.total;
        R = G * N + 1;   // arrays carry one dummy row
        PS = 16;
    } else {
        const StashLayout sl = dff_stash_layout(N, G, H, L, m->last.mt);
        o_nodes = sl.nodes_in; o_attn = sl.attn_out; o_ff = sl.ff; o_hpre = sl.h_pre; o_qkv = sl.qkvx; o_P = sl.P;
        lstride = sl.layer_stride; total = sl.total;
        R = G * N;
        PS = (int)sl.PS;
    }
    const int Prows = m->last.small ? 16 : R;   // rows of one head's P block
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
