// dff_analysis.hip -- the sample-analysis half of libdff_amd.so: the stateless entry points of include/dff.h that work on
// structures already resident in HBM and never touch a dff_model (dff_pwd_*, dff_struct_*, dff_tica_*, dff_kmeans_*,
// dff_transition_counts, dff_rmsd_*, dff_superpose, dff_gromos_*, dff_struct_native_q, dff_core_states, dff_label_runs, dff_path_states, dff_autocorr, dff_micro_*, dff_msm_* with their batched counterparts, dff_msm_dirichlet_*, dff_sym_eig_*, dff_msm_propagate* and dff_hmm_*, dff_hmm_viterbi, dff_unit_hist and dff_resampled_js among them), and the kernels they launch.  The sampler kernels include none of these files.
#include "dff_host_common.h"
#include <atomic>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dff_pwd.hip"
#include "dff_struct.hip"
#include "dff_tica.hip"
#include "dff_states.hip"
#include "dff_ensemble.hip"
#include "dff_superpose.hip"
#include "dff_cluster.hip"
#include "dff_kinetics.hip"
#include "dff_paths.hip"
#include "dff_autocorr.hip"
#include "dff_msm.hip"
#include "dff_msm_batch.hip"
#include "dff_msm_passage.hip"
#include "dff_sym_eig.hip"
#include "dff_msm_propagate.hip"
#include "dff_hmm.hip"
#include "dff_hmm_viterbi.hip"
#include "dff_hmm_mstep.hip"
#include "dff_jsboot.hip"

// ---------------------------------------------------------------------------------------------
// Argument checks that several entry points share; `what` is the caller's name in the message
// ---------------------------------------------------------------------------------------------
// the bead range of everything that works on dihedrals or superpositions
static int check_beads(int N, const char* what) {
    if (N < 4 || N > DFF_MAX_BEADS) return fail(DFF_EINVAL, "%s: n_beads must be 4..%d", what, DFF_MAX_BEADS);
    return DFF_OK;
}

// a caller's workspace against the bytes its *_workspace_bytes function asks for (none needed: nothing to check)
static int check_workspace(const void* workspace, size_t workspace_bytes, long long need, const char* what) {
    if (need > 0 && (!workspace || (long long)workspace_bytes < need))
        return fail(DFF_EINVAL, "%s: workspace of %zu bytes, %lld needed", what, workspace_bytes, need);
    return DFF_OK;
}

// the same for a workspace the kernels read as 64-bit words
static int check_workspace8(const void* workspace, size_t workspace_bytes, long long need, const char* what) {
    if (int rc = check_workspace(workspace, workspace_bytes, need, what)) return rc;
    if (need > 0 && (uintptr_t)workspace % 8) return fail(DFF_EINVAL, "%s: the workspace must be 8-byte aligned", what);
    return DFF_OK;
}

// the frames of every tile kernel (struct_tiles): their tiles are counted in 32 bits
static int check_frames(long long n, const char* what) {
    if (n > 0x7fffffffLL * DFF_STRUCT_TILE) return fail(DFF_EINVAL, "%s: too many frames", what);
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// PWD histograms (dff_pwd.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_pwd_num_pairs(int n_beads, int offset) {
    if (n_beads < 1 || offset < 0) return 0;
    int np = 0;
    for (int i = 0; i < n_beads; ++i) np += (n_beads - i - offset > 0) ? n_beads - i - offset : 0;
    return np;
}

static int pwd_check(int device, const float* x, long long n, int N, int offset, int& npairs) {
    if ((!x && n > 0) || n < 0) return fail(DFF_EINVAL, "pwd: null input / negative count");
    if (N < 2 || N > DFF_MAX_BEADS) return fail(DFF_EINVAL, "pwd: n_beads must be 2..%d", DFF_MAX_BEADS);
    npairs = dff_pwd_num_pairs(N, offset);
    if (npairs <= 0) return fail(DFF_EINVAL, "pwd: no bead pairs at offset %d", offset);
    return DFF_OK;
}

// structures per workgroup: a multiple of the tile, enough workgroups to fill the chip, and long
// enough that the per-workgroup flush stays small next to the streaming part
static long long pwd_chunk(long long n, long long want_wgs, long long min_chunk) {
    long long chunk = (n + want_wgs - 1) / want_wgs;
    if (chunk < min_chunk) chunk = min_chunk;
    chunk = (chunk + DFF_PWD_TILE - 1) / DFF_PWD_TILE * DFF_PWD_TILE;
    return chunk;
}

extern "C" int dff_pwd_max(int device, const float* x, long long n, int N, int offset, float* max_out, void* stream_) {
    int npairs;
    int rc = pwd_check(device, x, n, N, offset, npairs);
    if (rc) return rc;
    ON_DEVICE(device);
    if (!max_out) return fail(DFF_EINVAL, "pwd: null output");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(max_out, 0, (size_t)npairs * sizeof(float), stream));
    if (n == 0) return DFF_OK;
    const long long chunk = pwd_chunk(n, 1024, 4 * DFF_PWD_TILE);
    const int grid = (int)((n + chunk - 1) / chunk);
    const unsigned lds = (unsigned)(DFF_PWD_TILE * 3 * N * sizeof(float) + 16);
    int pc_log2 = 0;
    while ((1 << pc_log2) < npairs && pc_log2 < 8) ++pc_log2;
    if (npairs > (DFF_PWD_MAXG << pc_log2)) return fail(DFF_EINVAL, "pwd: too many pairs (%d)", npairs);
    const int vec4 = ((uintptr_t)x % 16) == 0;
    hipLaunchKernelGGL(dff_pwd_max_kernel, dim3(grid), dim3(DFF_PWD_THREADS), lds, stream, x, n, N, offset, npairs,
                       pc_log2, chunk, (unsigned*)max_out, vec4);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// The launch layout of dff_pwd_hist_kernel for n structures of N beads and histograms of up to max_bins bins: pure host
// arithmetic, the one statement of it (dff_pwd_hist launches what it says, dff_pwd_hist_plan shows it to the tests).
// LDS holds one tile of structures + the privatised histograms.  The tile shrinks from 64 to 32 structures when that lets
// twice as many pairs keep their histograms in LDS (fewer passes over the structures); a smaller tile never helps, since
// DFF_PWD_LDS_BINS caps the slots at 32 structures already for every N <= DFF_MAX_BEADS.
static int pwd_hist_layout(int N, int offset, int max_bins, long long n, dff_pwd_plan* out) {
    if (N < 2 || N > DFF_MAX_BEADS) return fail(DFF_EINVAL, "pwd: n_beads must be 2..%d", DFF_MAX_BEADS);
    const int npairs = dff_pwd_num_pairs(N, offset);
    if (npairs <= 0) return fail(DFF_EINVAL, "pwd: no bead pairs at offset %d", offset);
    if (max_bins < 1) return fail(DFF_EINVAL, "pwd: need 1 <= max_bins <= ld");
    if (n < 0) return fail(DFF_EINVAL, "pwd: null input / negative count");
    const int ldl = max_bins | 1;   // odd leading dimension: pairs land in different LDS banks
    int tile_n = DFF_PWD_TILE, pc_log2 = -1, tile_bytes = 0;
    for (int tn = DFF_PWD_TILE; tn >= DFF_PWD_TILE / 2; tn >>= 1) {
        const int tb = tn * 3 * N * (int)sizeof(float);
        int slots = (160 * 1024 - 64 - tb) / (int)sizeof(unsigned);
        if (slots > DFF_PWD_LDS_BINS) slots = DFF_PWD_LDS_BINS;
        if (ldl > slots) continue;
        int lg = 8;                 // pair lanes per workgroup: the largest power of two whose histograms fit
        while (lg > 0 && ((1 << lg) * ldl > slots || (1 << (lg - 1)) >= npairs)) --lg;
        if (lg > pc_log2) { pc_log2 = lg; tile_n = tn; tile_bytes = tb; }
    }
    if (pc_log2 < 0) return fail(DFF_EINVAL, "pwd: %d bins per pair do not fit in LDS (at most %d)", max_bins, DFF_PWD_LDS_BINS - 1);
    const int PC = 1 << pc_log2;
    const int npc = (npairs + PC - 1) / PC;
    // each workgroup flushes up to PC * ldl bins: give it at least ~2x that many (pair, structure) items
    const long long min_chunk = (2LL * ldl + DFF_PWD_TILE - 1) / DFF_PWD_TILE * DFF_PWD_TILE;   // multiple of both tile sizes
    const long long chunk = pwd_chunk(n, (2048 + npc - 1) / npc, min_chunk);
    const long long nsc = (n + chunk - 1) / chunk;
    const long long nsc8 = (nsc + 7) / 8 * 8;       // whole XCD rounds (empty chunks return at once)
    const long long grid = nsc8 * npc;
    if (grid > 0x7fffffffLL) return fail(DFF_EINVAL, "pwd: grid too large");
    const unsigned lds = (unsigned)(tile_bytes + (size_t)PC * ldl * sizeof(unsigned) + 16);
    if (lds > 160 * 1024) return fail(DFF_EINVAL, "pwd: LDS budget exceeded (%u bytes)", lds);
    out->n_pairs = npairs; out->tile_n = tile_n; out->pc_log2 = pc_log2; out->npc = npc; out->ldl = ldl;
    out->lds_bytes = (int32_t)lds; out->chunk = chunk; out->chunks = nsc; out->chunks_rounded = nsc8; out->grid = grid;
    return DFF_OK;
}

extern "C" int dff_pwd_hist_plan(int n_beads, int offset, int max_bins, long long n, dff_pwd_plan* out) {
    if (!out) return fail(DFF_EINVAL, "pwd: null argument");
    return pwd_hist_layout(n_beads, offset, max_bins, n, out);
}

extern "C" int dff_pwd_hist(int device, const float* x, long long n, int N, int offset, const int32_t* nbins,
                            const float* hmax, int max_bins, int ld, uint32_t* hist, void* stream_) {
    int npairs;
    int rc = pwd_check(device, x, n, N, offset, npairs);
    if (rc) return rc;
    ON_DEVICE(device);
    if (!nbins || !hmax || !hist) return fail(DFF_EINVAL, "pwd: null argument");
    if (max_bins < 1 || ld < max_bins) return fail(DFF_EINVAL, "pwd: need 1 <= max_bins <= ld");
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(hist, 0, (size_t)npairs * ld * sizeof(uint32_t), stream));
    if (n == 0) return DFF_OK;
    dff_pwd_plan pl;
    if ((rc = pwd_hist_layout(N, offset, max_bins, n, &pl))) return rc;
    HIPCHK(hipFuncSetAttribute((const void*)&dff_pwd_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds_bytes));
    const int vec4 = ((uintptr_t)x % 16) == 0;
    hipLaunchKernelGGL(dff_pwd_hist_kernel, dim3((unsigned)pl.grid), dim3(DFF_PWD_HIST_THREADS), (unsigned)pl.lds_bytes, stream,
                       x, n, N, offset, npairs, nbins, hmax, ld, pl.pc_log2, pl.npc, pl.chunk, pl.ldl, hist, vec4, pl.tile_n);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Structure metrics: RMSD, dihedrals, TIC projection, contacts (dff_struct.hip)
// ---------------------------------------------------------------------------------------------
static int struct_check(const float* x, long long n, int N, const void* out, const char* what) {
    if ((!x && n > 0) || n < 0) return fail(DFF_EINVAL, "%s: null input / negative count", what);
    if (int rc = check_beads(N, what)) return rc;
    if (!out && n > 0) return fail(DFF_EINVAL, "%s: null output", what);
    return check_frames(n, what);
}

static unsigned struct_tile_bytes(int N) { return (unsigned)(DFF_STRUCT_TILE * struct_ld(N) * sizeof(float)); }

// Launch of a tile kernel, kernel(x, n, N, args..., magic, vec4) (struct_tiles, dff_struct.hip).  One wave per workgroup:
// enough of them to keep every CU streaming, at most `cap`, each walking tiles with a grid stride.
template <class... Params, class... Args>
static int struct_launch(void (*kernel)(const float*, long long, int, Params...), long long cap, unsigned lds,
                         void* stream, const float* x, long long n, int N, Args... args) {
    const long long ntiles = (n + DFF_STRUCT_TILE - 1) / DFF_STRUCT_TILE;
    const unsigned magic = (unsigned)((0x100000000ULL + 3 * N - 1) / (3 * N));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(ntiles < cap ? ntiles : cap)), dim3(DFF_STRUCT_TILE), lds,
                       (hipStream_t)stream, x, n, N, args..., magic, (int)(((uintptr_t)x % 16) == 0));
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" int dff_struct_rmsd(int device, const float* x, long long n, int N, const float* ref, float* rmsd,
                               void* stream_) {
    int rc = struct_check(x, n, N, rmsd, "struct_rmsd");
    if (rc) return rc;
    if (!ref) return fail(DFF_EINVAL, "struct_rmsd: null reference structure");
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    const unsigned lds = (unsigned)(((6 * N + 3) & ~3) * sizeof(float)) + struct_tile_bytes(N);
    return struct_launch(dff_struct_rmsd_kernel, 8192, lds, stream_, x, n, N, ref, rmsd);
}

extern "C" int dff_struct_dihedrals(int device, const float* x, long long n, int N, float* out, void* stream_) {
    int rc = struct_check(x, n, N, out, "struct_dihedrals");
    if (rc) return rc;
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    const unsigned lds = struct_tile_bytes(N) + (unsigned)(DFF_STRUCT_TILE * (N - 3) * sizeof(float));
    return struct_launch(dff_struct_dihedrals_kernel, 8192, lds, stream_, x, n, N, out);
}

extern "C" int dff_struct_tic_num_features(int n_beads) { return n_beads < 4 ? 0 : struct_tic_num_features(n_beads); }

static int tic_model_check(const double* mean, const double* coeff, int k, const char* what) {
    if (!mean || !coeff) return fail(DFF_EINVAL, "%s: null mean / coefficients", what);
    if (k < 1 || k > DFF_TIC_MAXK) return fail(DFF_EINVAL, "%s: k must be 1..%d", what, DFF_TIC_MAXK);
    return DFF_OK;
}

extern "C" int dff_struct_tic(int device, const float* x, long long n, int N, const double* mean, const double* coeff,
                              int k, double* out, void* stream_) {
    int rc = struct_check(x, n, N, out, "struct_tic");
    if (rc) return rc;
    if ((rc = tic_model_check(mean, coeff, k, "struct_tic"))) return rc;
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    return struct_launch(dff_struct_tic_kernel, 8192, struct_tile_bytes(N), stream_, x, n, N, mean, coeff, k, out);
}

extern "C" int dff_struct_contacts(int device, const float* x, long long n, int N, float cutoff, const uint8_t* folded,
                                   int offset, uint32_t* counts, uint32_t* mismatch, void* stream_) {
    int rc = struct_check(x, n, N, counts, "struct_contacts");
    if (rc) return rc;
    if (!counts) return fail(DFF_EINVAL, "struct_contacts: null counts");
    if (mismatch && !folded) return fail(DFF_EINVAL, "struct_contacts: per-frame mismatches need a folded contact map");
    if (offset < 0) return fail(DFF_EINVAL, "struct_contacts: negative offset");
    ON_DEVICE(device);
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)N * N * sizeof(uint32_t), (hipStream_t)stream_));
    if (n == 0) return DFF_OK;
    const unsigned lds = (unsigned)(N * N * sizeof(unsigned) + ((N * N + 15) & ~15)) + struct_tile_bytes(N);
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void*)&dff_struct_contacts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    // every workgroup flushes up to N (N + 1) / 2 counters: fewer, longer workgroups than the other metrics
    return struct_launch(dff_struct_contacts_kernel, 2048, lds, stream_, x, n, N, cutoff, folded, offset, counts, mismatch);
}

// LDS of dff_tica_features_kernel (dff_tica.hip): tile | stage
static unsigned tica_features_lds(int N) {
    return struct_tile_bytes(N) + (unsigned)(DFF_STRUCT_TILE * (DFF_TICA_FCH + 1) * sizeof(float));
}

extern "C" int dff_struct_tic_features(int device, const float* x, long long n, int N, float* out, void* stream_) {
    int rc = struct_check(x, n, N, out, "struct_tic_features");
    if (rc) return rc;
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    return struct_launch(dff_tica_features_kernel, 8192, tica_features_lds(N), stream_, x, n, N, out);
}

// ---------------------------------------------------------------------------------------------
// TICA moments (dff_tica.hip)
// ---------------------------------------------------------------------------------------------
// Shapes of the moments pipeline, from the bead count and the largest call only: F features, NB 64-feature blocks, NT
// upper-triangular tiles, C pair starts per chunk (256 MB of fp32 feature rows), at most `slices` pair slices per launch
// (NT * slices ~ DFF_TICA_WGS workgroups, and no more slices than a call of n_max frames has stages of pairs).
struct TicaShape {
    int F, NB, NT, slices;
    long long C;
    TicaShape(int N, long long n_max) {
        F = dff_struct_tic_num_features(N);
        NB = (F + DFF_TICA_T - 1) / DFF_TICA_T;
        NT = NB * (NB + 1) / 2;
        C = (1LL << 28) / (4LL * F) / DFF_TICA_K * DFF_TICA_K;
        const long long stages = ((n_max < C ? n_max : C) + DFF_TICA_K - 1) / DFF_TICA_K;
        const int want = (DFF_TICA_WGS + NT - 1) / NT;
        slices = stages < want ? (int)(stages > 1 ? stages : 1) : want;
    }
    size_t part_bytes() const { return (size_t)slices * NT * 2 * DFF_TICA_T * DFF_TICA_T * sizeof(double); }
    size_t psum_bytes() const { return (size_t)slices * NB * 2 * DFF_TICA_T * sizeof(double); }
    size_t feat_bytes(long long n_max, int lag) const {
        const long long rows = n_max < C + lag ? n_max : C + lag;
        return ((size_t)rows * F * sizeof(float) + 255) & ~(size_t)255;
    }
};

// The chunks of one call: runs of consecutive pair starts t (t and t + lag in one trajectory), at most DFF_TICA_RUNS runs
// per chunk, every pair start of a chunk below f0 + C (f0 = the chunk's first pair start), so that the chunk's feature
// rows f0 .. last pair start + lag number at most C + lag.  A run that would start at or past f0 + C opens a new chunk:
// frames that start no pair (a trajectory's last lag frames, trajectories of <= lag frames) may lie across that limit.
// chunk(f0, rows, runs, pairs) is called once per chunk, pairs > 0.
template <class Chunk>
static int tica_plan(long long C, const long long* lengths, int n_traj, int lag, Chunk chunk) {
    TicaRuns runs;
    runs.n = 0;
    long long f0 = 0, last = 0;
    int pairs = 0, rc;
    auto flush = [&]() -> int {
        runs.cum[runs.n] = pairs;
        const int r = chunk(f0, last + lag - f0, runs, pairs);
        runs.n = 0;
        pairs = 0;
        return r;
    };
    long long o = 0;
    for (int i = 0; i < n_traj; o += lengths[i], ++i) {
        long long a = o;
        const long long b = o + lengths[i] - lag;       // pair starts [a, b)
        while (a < b) {
            if (runs.n == DFF_TICA_RUNS || (runs.n && a >= f0 + C))
                if ((rc = flush())) return rc;
            if (runs.n == 0) f0 = a;
            const long long e = b < f0 + C ? b : f0 + C;  // > a: a < f0 + C here
            runs.row[runs.n] = (int)(a - f0);
            runs.cum[runs.n] = pairs;
            pairs += (int)(e - a);
            ++runs.n;
            last = e;                                   // one past the chunk's last pair start
            a = e;
        }
    }
    if (runs.n && (rc = flush())) return rc;
    return DFF_OK;
}

extern "C" long long dff_tica_workspace_bytes(int n_beads, long long n_frames_max, int lagtime) {
    if (check_beads(n_beads, "tica")) return -1;
    if (lagtime < 1) return fail(DFF_EINVAL, "tica: lagtime must be >= 1"), -1;
    if (n_frames_max < 0) return fail(DFF_EINVAL, "tica: negative frame count"), -1;
    const TicaShape sh(n_beads, n_frames_max);
    return (long long)(sh.feat_bytes(n_frames_max, lagtime) + sh.part_bytes() + sh.psum_bytes());
}

// trajectories back to back: n_traj lengths that sum to the n frames of the call
static int traj_check_lengths(const long long* lengths, int n_traj, long long n, const char* what) {
    if (n_traj < 0 || (n_traj > 0 && !lengths)) return fail(DFF_EINVAL, "%s: null / negative trajectory lengths", what);
    long long total = 0;
    for (int i = 0; i < n_traj; ++i) {
        if (lengths[i] < 0) return fail(DFF_EINVAL, "%s: trajectory %d has negative length", what, i);
        total += lengths[i];
    }
    if (total != n) return fail(DFF_EINVAL, "%s: trajectory lengths sum to %lld, not n = %lld", what, total, n);
    return DFF_OK;
}

extern "C" int dff_tica_moments(int device, const float* x, long long n, int N, const long long* lengths, int n_traj,
                                int lagtime, const double* shift, void* workspace, size_t workspace_bytes, double* sx,
                                double* sy, double* m0, double* mt, void* stream_) {
    int rc = struct_check(x, n, N, m0, "tica_moments");
    if (rc) return rc;
    if (lagtime < 1) return fail(DFF_EINVAL, "tica_moments: lagtime must be >= 1");
    if ((rc = traj_check_lengths(lengths, n_traj, n, "tica_moments"))) return rc;
    if (!shift || !sx || !sy || !m0 || !mt) return fail(DFF_EINVAL, "tica_moments: null shift / accumulator");
    const long long need = dff_tica_workspace_bytes(N, n, lagtime);
    if ((rc = check_workspace(workspace, workspace_bytes, need, "tica_moments"))) return rc;
    // the partial matrices and sums are doubles, at offsets that are multiples of 256
    if (need > 0 && (uintptr_t)workspace % sizeof(double)) return fail(DFF_EINVAL, "tica_moments: the workspace must be 8-byte aligned");
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    const TicaShape sh(N, n);
    float* feat = (float*)workspace;
    double* part = (double*)((char*)workspace + sh.feat_bytes(n, lagtime));
    double* psum = (double*)((char*)part + sh.part_bytes());
    HIPCHK(hipFuncSetAttribute((const void*)&dff_tica_moments_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               DFF_TICA_LDS_BYTES));
    return tica_plan(sh.C, lengths, n_traj, lagtime, [&](long long f0, long long rows, const TicaRuns& runs, int pairs) -> int {
        // the plan's guarantees, on which every index below rests (workspace rows, slices, grid)
        if (pairs <= 0 || pairs > sh.C || rows > sh.C + lagtime || rows > n - f0 || f0 < 0)
            return fail(DFF_EINVAL, "tica_moments: internal chunk plan error (f0 %lld, rows %lld, pairs %d)", f0, rows, pairs);
        if (int rc = struct_launch(dff_tica_features_kernel, 8192, tica_features_lds(N), stream, x + f0 * 3 * N, rows, N, feat))
            return rc;
        const int kst = (pairs + DFF_TICA_K - 1) / DFF_TICA_K;          // stages of pairs
        const int ns0 = kst < sh.slices ? kst : sh.slices;
        const int per = (kst + ns0 - 1) / ns0 * DFF_TICA_K;              // pairs per slice, a multiple of the stage
        const int ns = (pairs + per - 1) / per;                          // 1 .. sh.slices
        hipLaunchKernelGGL(dff_tica_moments_kernel, dim3((unsigned)(ns * sh.NT)), dim3(DFF_TICA_THREADS),
                           DFF_TICA_LDS_BYTES, stream, feat, sh.F, lagtime, shift, runs, pairs, per, sh.NB, sh.NT, part,
                           psum);
        HIPCHK(hipGetLastError());
        const long long nred = (long long)sh.NT * DFF_TICA_T * DFF_TICA_T + (long long)sh.NB * DFF_TICA_T;
        hipLaunchKernelGGL(dff_tica_reduce_kernel, dim3((unsigned)((nred + DFF_TICA_THREADS - 1) / DFF_TICA_THREADS)),
                           dim3(DFF_TICA_THREADS), 0, stream, part, psum, sh.F, sh.NB, sh.NT, ns, sx, sy, m0, mt);
        HIPCHK(hipGetLastError());
        return DFF_OK;
    });
}

extern "C" int dff_tica_debug_plan(int n_beads, const long long* lengths, int n_traj, int lagtime, long long chunk_pairs,
                                   long long* out_host, int max_runs) {
    if (check_beads(n_beads, "tica_debug_plan")) return -1;
    long long n = 0;
    for (int i = 0; i < n_traj && lengths; ++i) n += lengths[i] > 0 ? lengths[i] : 0;
    if (lagtime < 1) return fail(DFF_EINVAL, "tica_debug_plan: lagtime must be >= 1"), -1;
    if (traj_check_lengths(lengths, n_traj, n, "tica_debug_plan")) return -1;
    if (!out_host || max_runs < 0) return fail(DFF_EINVAL, "tica_debug_plan: null output"), -1;
    const long long C = chunk_pairs > 0 ? chunk_pairs : TicaShape(n_beads, n).C;
    int nrec = 0, chunk_id = 0;
    const int rc = tica_plan(C, lengths, n_traj, lagtime, [&](long long f0, long long rows, const TicaRuns& runs, int pairs) -> int {
        for (int r = 0; r < runs.n; ++r, ++nrec)
            if (nrec < max_runs) {
                long long* o = out_host + 6LL * nrec;
                o[0] = chunk_id; o[1] = f0; o[2] = rows; o[3] = pairs; o[4] = runs.row[r]; o[5] = runs.cum[r + 1] - runs.cum[r];
            }
        ++chunk_id;
        return DFF_OK;
    });
    return rc ? -1 : nrec;
}

// ---------------------------------------------------------------------------------------------
// States in TIC space and the transitions between them (dff_states.hip)
// ---------------------------------------------------------------------------------------------
// K states, called `noun` ("centres", "states") in the caller's message
static int states_check_count(int K, const char* what, const char* noun) {
    if (K < 1 || K > DFF_STATES_MAXK) return fail(DFF_EINVAL, "%s: the number of %s must be 1..%d", what, noun, DFF_STATES_MAXK);
    return DFF_OK;
}

extern "C" int dff_struct_tic_assign(int device, const float* x, long long n, int N, const double* mean,
                                     const double* coeff, int k, const double* centers, int K, int32_t* labels,
                                     double* proj, double* dist2, void* stream_) {
    int rc = struct_check(x, n, N, labels, "struct_tic_assign");
    if (rc) return rc;
    if ((rc = tic_model_check(mean, coeff, k, "struct_tic_assign"))) return rc;
    if (!centers) return fail(DFF_EINVAL, "struct_tic_assign: null centres");
    if ((rc = states_check_count(K, "struct_tic_assign", "centres"))) return rc;
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    return struct_launch(dff_struct_tic_assign_kernel, 8192, struct_tile_bytes(N), stream_, x, n, N, mean, coeff, k, centers,
                         K, labels, proj, dist2);
}

// workgroups of the k-means step: a function of n alone (the order of every sum follows from it)
static int kmeans_grid(long long n) {
    const long long g = (n + DFF_KM_THREADS - 1) / DFF_KM_THREADS;
    return (int)(g < DFF_KM_WGS ? g : DFF_KM_WGS);
}

static int kmeans_check_shape(long long n, int d, int K, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative point count", what);
    if (d < 1 || d > DFF_KM_MAXD) return fail(DFF_EINVAL, "%s: d must be 1..%d", what, DFF_KM_MAXD);
    return states_check_count(K, what, "centres");
}

extern "C" long long dff_kmeans_workspace_bytes(long long n, int d, int K) {
    if (kmeans_check_shape(n, d, K, "kmeans_workspace_bytes")) return -1;
    return (long long)kmeans_grid(n) * (K * d + K + 1) * (long long)sizeof(double);
}

// What both k-means steps do around their kernels, after the caller's shape check: pointers, the workspace (`need` bytes,
// `align`-byte aligned, when something is accumulated), the device, zeroed results at n == 0; then launch(accumulate), unless
// nothing is asked for.
template <class Launch>
static int kmeans_call(int device, const double* pts, long long n, int d, const double* centers, int K, const int32_t* labels,
                       const double* dist2, double* sums, uint64_t* counts, double* inertia, const void* workspace,
                       size_t workspace_bytes, long long need, size_t align, hipStream_t stream, const char* what,
                       Launch launch) {
    if (!pts && n > 0) return fail(DFF_EINVAL, "%s: null points", what);
    if (!centers) return fail(DFF_EINVAL, "%s: null centres", what);
    const bool accumulate = sums || counts || inertia;
    if (!accumulate) need = 0;                                      // and 0 at n = 0
    if (int rc = check_workspace(workspace, workspace_bytes, need, what)) return rc;
    if (need > 0 && (uintptr_t)workspace % align) return fail(DFF_EINVAL, "%s: the workspace must be %d-byte aligned", what, (int)align);
    ON_DEVICE(device);
    if (n == 0) {
        if (sums) HIPCHK(hipMemsetAsync(sums, 0, (size_t)K * d * sizeof(double), stream));
        if (counts) HIPCHK(hipMemsetAsync(counts, 0, (size_t)K * sizeof(uint64_t), stream));
        if (inertia) HIPCHK(hipMemsetAsync(inertia, 0, sizeof(double), stream));
        return DFF_OK;
    }
    if (!accumulate && !labels && !dist2) return DFF_OK;
    return launch(accumulate);
}

extern "C" int dff_kmeans_step(int device, const double* pts, long long n, int d, const double* centers, int K,
                               int32_t* labels, double* dist2, double* sums, uint64_t* counts, double* inertia,
                               void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = kmeans_check_shape(n, d, K, "kmeans_step")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    return kmeans_call(device, pts, n, d, centers, K, labels, dist2, sums, counts, inertia, workspace, workspace_bytes,
                       dff_kmeans_workspace_bytes(n, d, K), sizeof(double), stream, "kmeans_step", [&](bool accumulate) -> int {
        const int per = K * d + K + 1, grid = kmeans_grid(n);
        double* part = accumulate ? (double*)workspace : nullptr;
        hipLaunchKernelGGL(dff_kmeans_step_kernel, dim3(grid), dim3(DFF_KM_THREADS),
                           (unsigned)(4 * per * sizeof(double)), stream, pts, n, d, centers, K, labels, dist2, part);
        HIPCHK(hipGetLastError());
        if (accumulate) {
            hipLaunchKernelGGL(dff_kmeans_reduce_kernel, dim3(per), dim3(64), 0, stream, part, grid, d, K, sums,
                               (unsigned long long*)counts, inertia);
            HIPCHK(hipGetLastError());
        }
        return DFF_OK;
    });
}

// The launches of a call over n > 0 frames of trajectories back to back (lengths already checked): launch(runs) once per
// group of whole trajectories.  Equal lengths (what the sampler produces; empty trajectories hold no frame and are left
// out): one group with a period; otherwise groups of up to DFF_TC_RUNS trajectories with their start table.
template <class Launch>
static int traj_launches(const long long* lengths, int n_traj, long long n, Launch launch) {
    long long period = 0;
    bool equal = true;
    for (int i = 0; i < n_traj; ++i)
        if (lengths[i] > 0) {
            if (period == 0) period = lengths[i];
            else if (lengths[i] != period) equal = false;
        }
    TransRuns runs = {};
    if (equal) {
        runs.begin = 0; runs.end = n; runs.period = period;
        return launch(runs);
    }
    long long o = 0;
    for (int i = 0; i < n_traj; o += lengths[i], ++i) {
        if (lengths[i] == 0) continue;
        if (runs.n == 0) runs.begin = o;
        runs.start[runs.n++] = o;
        runs.start[runs.n] = runs.end = o + lengths[i];
        if (runs.n == DFF_TC_RUNS) {
            if (int rc = launch(runs)) return rc;
            runs.n = 0;
        }
    }
    return runs.n ? launch(runs) : DFF_OK;
}

// the launches of dff_transition_counts_kernel over checked arguments, n > 0, K <= DFF_STATES_MAXK, counts already zeroed
static int tc_launches(hipStream_t stream, const int32_t* labels, long long n, const long long* lengths, int n_traj,
                       const int32_t* lags, int n_lags, int K, uint64_t* counts) {
    const int per_group = DFF_TC_LDS_COUNTERS / (K * K) < n_lags ? DFF_TC_LDS_COUNTERS / (K * K) : n_lags;   // >= 2
    return traj_launches(lengths, n_traj, n, [&](const TransRuns& runs) -> int {
        const long long wgs = (runs.end - runs.begin + DFF_TC_THREADS - 1) / DFF_TC_THREADS;
        for (int l0 = 0; l0 < n_lags; l0 += per_group) {
            TransLags g;
            g.n = n_lags - l0 < per_group ? n_lags - l0 : per_group;
            for (int l = 0; l < DFF_TC_MAXLAGS; ++l) g.lag[l] = l < g.n ? lags[l0 + l] : 0;
            hipLaunchKernelGGL(dff_transition_counts_kernel, dim3((unsigned)(wgs < DFF_TC_WGS ? wgs : DFF_TC_WGS)),
                               dim3(DFF_TC_THREADS), (unsigned)(g.n * K * K * sizeof(unsigned)), stream, labels, K, runs, g,
                               (unsigned long long*)counts + (size_t)l0 * K * K);
            HIPCHK(hipGetLastError());
        }
        return DFF_OK;
    });
}

static int tc_check_lags(const int32_t* lags, int n_lags, const char* what) {
    if (!lags || n_lags < 1 || n_lags > DFF_TC_MAXLAGS)
        return fail(DFF_EINVAL, "%s: the number of lag times must be 1..%d", what, DFF_TC_MAXLAGS);
    for (int l = 0; l < n_lags; ++l)
        if (lags[l] < 1) return fail(DFF_EINVAL, "%s: lag time %d is %d, must be >= 1", what, l, (int)lags[l]);
    return DFF_OK;
}

extern "C" int dff_transition_counts(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj,
                                     const int32_t* lags, int n_lags, int K, uint64_t* counts, void* stream_) {
    if ((!labels && n > 0) || n < 0) return fail(DFF_EINVAL, "transition_counts: null labels / negative count");
    int rc = states_check_count(K, "transition_counts", "states");
    if (rc) return rc;
    if ((rc = tc_check_lags(lags, n_lags, "transition_counts"))) return rc;
    if ((rc = traj_check_lengths(lengths, n_traj, n, "transition_counts"))) return rc;
    if (!counts) return fail(DFF_EINVAL, "transition_counts: null counts");
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)n_lags * K * K * sizeof(uint64_t), stream));
    if (n == 0) return DFF_OK;
    return tc_launches(stream, labels, n, lengths, n_traj, lags, n_lags, K, counts);
}

// ---------------------------------------------------------------------------------------------
// RMSD between two ensembles: dense matrix and nearest candidate (dff_ensemble.hip)
// ---------------------------------------------------------------------------------------------
static int ens_check_shape(long long n, long long m, int N, const char* what) {
    if (n < 0 || m < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (int rc = check_beads(N, what)) return rc;
    if (m > 0x7fffffffLL) return fail(DFF_EINVAL, "%s: more than 2^31 - 1 candidates (the index half of the key is 32 bits)", what);
    return DFF_OK;
}

// One launch over queries x (n) and candidates y (m), both > 0.  The grid follows from the shapes alone -- and the result
// does not depend on it: one workgroup per (32-candidate tile, slice of the query tiles), enough slices to reach
// DFF_ENS_WGS workgroups, never more than there are groups of four query tiles.
template <bool NEAREST>
static int ens_launch(hipStream_t stream, const float* x, long long n, const float* y, long long m, int N,
                      long long self_first, float* out, unsigned long long* keys) {
    const long long nct = (m + DFF_ENS_TC - 1) / DFF_ENS_TC;
    const long long nq4 = ((n + DFF_ENS_TQ - 1) / DFF_ENS_TQ + 3) / 4;
    long long qsplit = (DFF_ENS_WGS + nct - 1) / nct;
    if (qsplit > nq4) qsplit = nq4;
    hipLaunchKernelGGL(dff_ens_rmsd_kernel<NEAREST>, dim3((unsigned)(nct * qsplit)), dim3(DFF_ENS_THREADS),
                       (unsigned)(ens_lds_doubles(ens_np(N)) * sizeof(double)), stream, x, n, y, m, N, (int)qsplit, self_first,
                       out, keys);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" long long dff_rmsd_nearest_workspace_bytes(long long n, long long m, int n_beads) {
    if (ens_check_shape(n, m, n_beads, "rmsd_nearest_workspace_bytes")) return -1;
    return (n < DFF_ENS_QCHUNK ? n : DFF_ENS_QCHUNK) * (long long)sizeof(unsigned long long);
}

extern "C" int dff_rmsd_nearest(int device, const float* x, long long n, const float* y, long long m, int N,
                                long long self_first, float* rmsd, long long* index, void* workspace,
                                size_t workspace_bytes, void* stream_) {
    int rc = ens_check_shape(n, m, N, "rmsd_nearest");
    if (rc) return rc;
    if ((!x && n > 0) || (!y && m > 0)) return fail(DFF_EINVAL, "rmsd_nearest: null frames");
    if (!rmsd && n > 0) return fail(DFF_EINVAL, "rmsd_nearest: null output");
    if (self_first < -1) return fail(DFF_EINVAL, "rmsd_nearest: self_first must be -1 or a candidate index");
    const long long need = dff_rmsd_nearest_workspace_bytes(n, m, N);
    // the keys are 64-bit words that an integer atomic minimum works on
    if ((rc = check_workspace8(workspace, workspace_bytes, need, "rmsd_nearest"))) return rc;
    if (n == 0) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    unsigned long long* keys = (unsigned long long*)workspace;
    for (long long o = 0; o < n; o += DFF_ENS_QCHUNK) {
        const long long c = n - o < DFF_ENS_QCHUNK ? n - o : DFF_ENS_QCHUNK;
        HIPCHK(hipMemsetAsync(keys, 0xff, (size_t)c * sizeof(unsigned long long), stream));
        if (m > 0 && (rc = ens_launch<true>(stream, x + o * 3 * N, c, y, m, N, self_first >= 0 ? self_first + o : -1,
                                            nullptr, keys)))
            return rc;
        hipLaunchKernelGGL(dff_ens_finish_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, stream, keys, c, rmsd + o,
                           index ? index + o : nullptr);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

extern "C" int dff_rmsd_matrix(int device, const float* x, long long n, const float* y, long long m, int N, float* out,
                               void* stream_) {
    int rc = ens_check_shape(n, m, N, "rmsd_matrix");
    if (rc) return rc;
    if ((!x && n > 0) || (!y && m > 0)) return fail(DFF_EINVAL, "rmsd_matrix: null frames");
    if (n > 0 && m > (1LL << 28) / n) return fail(DFF_EINVAL, "rmsd_matrix: n * m = %lld x %lld exceeds 2^28 entries", n, m);
    if (n == 0 || m == 0) return DFF_OK;
    if (!out) return fail(DFF_EINVAL, "rmsd_matrix: null output");
    ON_DEVICE(device);
    return ens_launch<false>((hipStream_t)stream_, x, n, y, m, N, -1, out, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Superposition on a reference: rotations, aligned frames, ensemble statistics (dff_superpose.hip)
// ---------------------------------------------------------------------------------------------
// workgroups of a call: a function of n alone (the slices of the workspace, and the order of every sum, follow from it)
static long long superpose_grid(long long n) {
    const long long ntiles = (n + DFF_STRUCT_TILE - 1) / DFF_STRUCT_TILE;
    return ntiles < DFF_SUP_WGS ? ntiles : DFF_SUP_WGS;
}

static int superpose_check_shape(long long n, int N, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (int rc = check_beads(N, what)) return rc;
    return check_frames(n, what);
}

extern "C" long long dff_superpose_workspace_bytes(long long n, int n_beads) {
    if (superpose_check_shape(n, n_beads, "superpose_workspace_bytes")) return -1;
    return superpose_grid(n) * superpose_per(n_beads) * (long long)sizeof(double);     // <= 4096 slices of 4 N + 1 doubles
}

extern "C" int dff_superpose(int device, const float* x, long long n, int N, const float* ref, float* aligned, double* rot,
                             float* rmsd, double* dsum, double* dsq, uint64_t* count, void* workspace,
                             size_t workspace_bytes, void* stream_) {
    int rc = superpose_check_shape(n, N, "superpose");
    if (rc) return rc;
    if (!x && n > 0) return fail(DFF_EINVAL, "superpose: null frames");
    if (!ref && n > 0) return fail(DFF_EINVAL, "superpose: null reference structure");
    const bool stats = dsum || dsq || count;
    const long long need = stats ? dff_superpose_workspace_bytes(n, N) : 0;
    if ((rc = check_workspace8(workspace, workspace_bytes, need, "superpose"))) return rc;
    if (!stats && !aligned && !rot && !rmsd) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) {
        if (dsum) HIPCHK(hipMemsetAsync(dsum, 0, (size_t)3 * N * sizeof(double), stream));
        if (dsq) HIPCHK(hipMemsetAsync(dsq, 0, (size_t)N * sizeof(double), stream));
        if (count) HIPCHK(hipMemsetAsync(count, 0, sizeof(uint64_t), stream));
        return DFF_OK;
    }
    // LDS: centred reference | tile | with statistics: staging buffer | accumulators (the table in dff_superpose.hip:
    // 8 176 / 25 392 bytes at N = 10, 50 944 / 69 888 at N = 64); above 64 KB the kernel has to be told
    unsigned lds = (unsigned)(superpose_ref_doubles(N) * sizeof(double)) + struct_tile_bytes(N);
    if (stats) lds += (unsigned)((DFF_STRUCT_TILE * DFF_SUP_LDS + 4 * N) * sizeof(double));
    if (lds > 160 * 1024) return fail(DFF_EINVAL, "superpose: LDS budget exceeded (%u bytes)", lds);
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void*)&dff_superpose_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double* part = stats ? (double*)workspace : nullptr;
    if ((rc = struct_launch(dff_superpose_kernel, DFF_SUP_WGS, lds, stream_, x, n, N, ref, aligned, rot, rmsd, part,
                            (int)(((uintptr_t)aligned % 16) == 0))))
        return rc;
    if (stats) {
        hipLaunchKernelGGL(dff_superpose_reduce_kernel, dim3(superpose_per(N)), dim3(64), 0, stream, part,
                           (int)superpose_grid(n), N, dsum, dsq, (unsigned long long*)count);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Clustering under the RMSD with a cutoff: neighbour bit-matrix and the greedy loop (dff_cluster.hip)
// ---------------------------------------------------------------------------------------------
static int cluster_check_frames(long long n, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (n > DFF_CLU_MAX_N) return fail(DFF_EINVAL, "%s: more than 2^18 frames (the bit matrix would exceed 8 GiB)", what);
    return DFF_OK;
}

extern "C" int dff_rmsd_neighbors(int device, const float* x, long long n, int N, float cutoff, uint64_t* adj, int* degree,
                                  void* stream_) {
    int rc = cluster_check_frames(n, "rmsd_neighbors");
    if (rc) return rc;
    if ((rc = check_beads(N, "rmsd_neighbors"))) return rc;
    if (!(cutoff >= 0.0f) || !(cutoff <= 3.402823466e38f))
        return fail(DFF_EINVAL, "rmsd_neighbors: cutoff must be finite and >= 0");
    if (n == 0) return DFF_OK;
    if (!x) return fail(DFF_EINVAL, "rmsd_neighbors: null frames");
    if (!adj) return fail(DFF_EINVAL, "rmsd_neighbors: null adjacency matrix");
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    const long long W = clu_words(n);
    HIPCHK(hipMemsetAsync(adj, 0, (size_t)(n * W) * sizeof(uint64_t), stream));
    const long long nct = (n + DFF_ENS_TC - 1) / DFF_ENS_TC;
    const long long nqt = (n + DFF_ENS_TQ - 1) / DFF_ENS_TQ;
    hipLaunchKernelGGL(dff_clu_neighbors_kernel, dim3((unsigned)nct, (unsigned)((nqt + DFF_CLU_GROUP - 1) / DFF_CLU_GROUP)),
                       dim3(DFF_ENS_THREADS), (unsigned)(ens_lds_doubles(ens_np(N)) * sizeof(double)), stream, x, n, N, cutoff,
                       (unsigned*)adj);
    HIPCHK(hipGetLastError());
    if (degree) {
        hipLaunchKernelGGL(dff_clu_degree_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream,
                           (const unsigned long long*)adj, n, degree);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

extern "C" long long dff_gromos_workspace_bytes(long long n) {
    if (cluster_check_frames(n, "gromos_workspace_bytes")) return -1;
    return (clu_words(n) + 1) * (long long)sizeof(uint64_t);           // alive | key
}

extern "C" int dff_gromos_steps(int device, const uint64_t* adj, long long n, int restart, int n_steps, int max_clusters,
                                int* labels, int* centers, int* sizes, int* progress, void* workspace, size_t workspace_bytes,
                                void* stream_) {
    int rc = cluster_check_frames(n, "gromos_steps");
    if (rc) return rc;
    if (n_steps < 0) return fail(DFF_EINVAL, "gromos_steps: negative n_steps");
    if (max_clusters < 1) return fail(DFF_EINVAL, "gromos_steps: max_clusters must be >= 1");
    if (!progress) return fail(DFF_EINVAL, "gromos_steps: null progress");
    if (n > 0 && !adj) return fail(DFF_EINVAL, "gromos_steps: null adjacency matrix");
    if (n > 0 && (!labels || !centers || !sizes)) return fail(DFF_EINVAL, "gromos_steps: null output");
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_gromos_workspace_bytes(n), "gromos_steps"))) return rc;
    if (!restart && n_steps == 0) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (restart) HIPCHK(hipMemsetAsync(progress, 0, 2 * sizeof(int), stream));
    if (n == 0) return DFF_OK;
    const int kmax = max_clusters < n ? max_clusters : (int)n;         // a cluster has at least one frame
    const unsigned long long* a = (const unsigned long long*)adj;
    unsigned long long* alive = (unsigned long long*)workspace;
    unsigned long long* key = alive + clu_words(n);
    if (restart) {
        hipLaunchKernelGGL(dff_clu_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, n, kmax, labels,
                           centers, sizes, progress, alive, key);
        HIPCHK(hipGetLastError());
    }
    for (int it = 0; it < n_steps; ++it) {
        hipLaunchKernelGGL(dff_clu_count_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, a, n, kmax, progress,
                           alive, key);
        hipLaunchKernelGGL(dff_clu_apply_kernel, dim3(1), dim3(DFF_CLU_APPLY_THREADS), 0, stream, a, n, kmax, labels, centers,
                           sizes, progress, alive, key);
    }
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Folding kinetics: native contacts per frame, core states, runs of labels (dff_kinetics.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_struct_native_q(int device, const float* x, long long n, int N, const int32_t* pairs, const float* r0,
                                   int n_pairs, double beta, double lambda, float* q, void* stream_) {
    int rc = struct_check(x, n, N, q, "struct_native_q");
    if (rc) return rc;
    if (n_pairs < 1 || n_pairs > N * (N - 1) / 2)
        return fail(DFF_EINVAL, "struct_native_q: n_pairs must be 1..%d for %d beads", N * (N - 1) / 2, N);
    if (!(beta > 0.0) || !(beta <= 1.7976931348623157e308))
        return fail(DFF_EINVAL, "struct_native_q: beta must be finite and > 0");
    if (!(lambda > 0.0) || !(lambda <= 1.7976931348623157e308))
        return fail(DFF_EINVAL, "struct_native_q: lambda must be finite and > 0");
    if (n == 0) return DFF_OK;
    if (!pairs || !r0) return fail(DFF_EINVAL, "struct_native_q: null pair list / native distances");
    ON_DEVICE(device);
    const unsigned lds = (unsigned)(native_q_r0_floats(n_pairs) * sizeof(float)) + struct_tile_bytes(N) +
                         (unsigned)(((n_pairs + 7) & ~7) * sizeof(unsigned short));
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void*)&dff_struct_native_q_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
    // every workgroup copies and checks the pair list: fewer, longer workgroups than the other metrics
    return struct_launch(dff_struct_native_q_kernel, 2048, lds, stream_, x, n, N, pairs, r0, n_pairs, beta, lambda, q);
}

static long long kin_blocks(long long n) { return (n + DFF_KIN_BLOCK - 1) / DFF_KIN_BLOCK; }

static int kin_check_frames(long long n, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (kin_blocks(n) > 0x7fffffffLL) return fail(DFF_EINVAL, "%s: too many frames", what);
    return DFF_OK;
}

extern "C" long long dff_kinetics_workspace_bytes(long long n) {
    if (kin_check_frames(n, "kinetics_workspace_bytes")) return -1;
    return kin_blocks(n) * (long long)sizeof(KinScan);              // one carry per DFF_KIN_BLOCK frames
}

// the core thresholds of dff_core_states and dff_path_states
static int kin_check_cores(float lo, float hi, const char* what) {
    if (!(fabsf(lo) <= 3.402823466e38f) || !(fabsf(hi) <= 3.402823466e38f))
        return fail(DFF_EINVAL, "%s: lo and hi must be finite", what);
    if (!(lo < hi)) return fail(DFF_EINVAL, "%s: lo must be < hi", what);
    return DFF_OK;
}

// The three launches of every group of trajectories of a call (dff_frame_scan.h): reduce -> carry -> apply(src, runs, fwd,
// rev if the call scans backwards, args...); the launch checks args against the kernel's parameters.  The workspace holds the
// forward carries of a launch's blocks, then the reverse ones of a call that has them (rev is never read otherwise).  count
// (may be NULL): the number of records, carried over the launches of the call; its first launch is the one that starts at
// frame 0.
template <class Src, class Apply, class... Args>
static int kin_scan(hipStream_t stream, Src src, const long long* lengths, int n_traj, long long n, void* workspace, long long* count,
                    Apply apply, Args... args) {
    return traj_launches(lengths, n_traj, n, [&](const TransRuns& runs) -> int {
        const unsigned nb = (unsigned)kin_blocks(runs.end - runs.begin);
        typename Src::Fwd* fwd = (typename Src::Fwd*)workspace;
        typename Src::Rev* rev = (typename Src::Rev*)(fwd + nb);
        hipLaunchKernelGGL(dff_scan_reduce_kernel<Src>, dim3(nb), dim3(DFF_KIN_THREADS), 0, stream, src, runs, fwd, rev);
        hipLaunchKernelGGL((dff_scan_carry_kernel<typename Src::Fwd, typename Src::Rev>), dim3(1), dim3(DFF_KIN_THREADS), 0, stream,
                           fwd, rev, (long long)nb, count, (int)(runs.begin == 0));
        if constexpr (scan_runs<typename Src::Rev>)
            hipLaunchKernelGGL(apply, dim3(nb), dim3(DFF_KIN_THREADS), 0, stream, src, runs, fwd, rev, args...);
        else
            hipLaunchKernelGGL(apply, dim3(nb), dim3(DFF_KIN_THREADS), 0, stream, src, runs, fwd, args...);
        HIPCHK(hipGetLastError());
        return DFF_OK;
    });
}

extern "C" int dff_core_states(int device, const float* cv, long long n, const long long* lengths, int n_traj, float lo,
                               float hi, int32_t* labels, int8_t* core, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    int rc = kin_check_frames(n, "core_states");
    if (rc) return rc;
    if ((rc = kin_check_cores(lo, hi, "core_states"))) return rc;
    if ((rc = traj_check_lengths(lengths, n_traj, n, "core_states"))) return rc;
    if (n == 0) return DFF_OK;
    if (!cv || !labels) return fail(DFF_EINVAL, "core_states: null cv / labels");
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_kinetics_workspace_bytes(n), "core_states"))) return rc;
    ON_DEVICE(device);
    return kin_scan((hipStream_t)stream_, KinCore{cv, lo, hi}, lengths, n_traj, n, workspace, nullptr, dff_kin_core_apply_kernel,
                    labels, core);
}

extern "C" int dff_label_runs(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj,
                              long long max_runs, long long* run_start, long long* run_length, int32_t* run_label,
                              uint8_t* run_flags, long long* n_runs, void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = kin_check_frames(n, "label_runs");
    if (rc) return rc;
    if (max_runs < 0) return fail(DFF_EINVAL, "label_runs: negative max_runs");
    if ((rc = traj_check_lengths(lengths, n_traj, n, "label_runs"))) return rc;
    if (n > 0 && (!labels || !n_runs)) return fail(DFF_EINVAL, "label_runs: null labels / n_runs");
    if (n > 0 && max_runs > 0 && (!run_start || !run_length || !run_label || !run_flags))
        return fail(DFF_EINVAL, "label_runs: null run output");
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_kinetics_workspace_bytes(n), "label_runs"))) return rc;
    if (n == 0 && !n_runs) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(n_runs, 0, sizeof(long long), stream));
        return DFF_OK;
    }
    return kin_scan(stream, KinRuns{labels}, lengths, n_traj, n, workspace, n_runs, dff_kin_runs_apply_kernel, max_runs, run_start,
                    run_length, run_label, run_flags);
}

// ---------------------------------------------------------------------------------------------
// Transition paths: previous and next core of every frame, frame classes, the path table (dff_paths.hip)
// ---------------------------------------------------------------------------------------------
extern "C" long long dff_path_states_workspace_bytes(long long n) {
    if (kin_check_frames(n, "path_states_workspace_bytes")) return -1;
    return kin_blocks(n) * (long long)(sizeof(PathFwd) + sizeof(PathBwd));   // one carry each way per DFF_KIN_BLOCK frames
}

extern "C" int dff_path_states(int device, const float* cv, long long n, const long long* lengths, int n_traj, float lo,
                               float hi, int8_t* prev, int8_t* next, long long* t_prev, long long* t_next, int8_t* cls,
                               long long max_paths, long long* path_exit, long long* path_entry, int8_t* path_dir,
                               long long* n_paths, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "path_states";
    int rc = kin_check_frames(n, what);
    if (rc) return rc;
    if ((rc = kin_check_cores(lo, hi, what))) return rc;
    if (max_paths < 0) return fail(DFF_EINVAL, "%s: negative max_paths", what);
    if ((rc = traj_check_lengths(lengths, n_traj, n, what))) return rc;
    if (n > 0 && !cv) return fail(DFF_EINVAL, "%s: null cv", what);
    if (n > 0 && n_paths && max_paths > 0 && (!path_exit || !path_entry || !path_dir))
        return fail(DFF_EINVAL, "%s: null path output", what);
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_path_states_workspace_bytes(n), what))) return rc;
    if (n == 0 && !n_paths) return DFF_OK;
    if (!prev && !next && !t_prev && !t_next && !cls && !n_paths) return DFF_OK;   // nothing is asked for
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(n_paths, 0, sizeof(long long), stream));
        return DFF_OK;
    }
    const PathOut out = {(signed char*)prev, (signed char*)next, t_prev, t_next, (signed char*)cls, n_paths ? max_paths : 0,
                         path_exit, path_entry, (signed char*)path_dir};
    return kin_scan(stream, PathSrc{{cv, lo, hi}}, lengths, n_traj, n, workspace, n_paths, dff_path_apply_kernel, out);
}

// ---------------------------------------------------------------------------------------------
// Lagged products inside trajectories: the sums behind the autocorrelation function (dff_autocorr.hip)
// ---------------------------------------------------------------------------------------------
static int ac_check_shape(long long n, int d, int max_lag, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (d < 1 || d > DFF_AC_MAXD) return fail(DFF_EINVAL, "%s: d must be 1..%d", what, DFF_AC_MAXD);
    if (max_lag < 0 || max_lag > DFF_AC_MAXLAG) return fail(DFF_EINVAL, "%s: max_lag must be 0..%d", what, DFF_AC_MAXLAG);
    if ((n + DFF_AC_TILE - 1) / DFF_AC_TILE > 0x7fffffffLL) return fail(DFF_EINVAL, "%s: too many frames", what);
    return DFF_OK;
}

// Shapes of a call over n > 0 frames, from (n, d, max_lag) alone: the grid is (slots, chunks, d), about DFF_AC_WGS
// workgroups and never more slots than tiles; the workspace is left (n ints, rounded up to 8 bytes) | partials.
struct AcShape {
    int nlags, chunks, slots;
    long long ntiles;
    AcShape(long long n, int d, int max_lag) {
        nlags = max_lag + 1;
        chunks = (nlags + DFF_AC_CHUNK - 1) / DFF_AC_CHUNK;
        ntiles = (n + DFF_AC_TILE - 1) / DFF_AC_TILE;
        const int want = (DFF_AC_WGS + chunks * d - 1) / (chunks * d);
        slots = ntiles < want ? (int)ntiles : want;
    }
    size_t left_bytes(long long n) const { return ((size_t)n * sizeof(int) + 7) & ~(size_t)7; }
    size_t part_bytes(int d) const { return (size_t)slots * (3 * d + 1) * nlags * sizeof(double); }
};

extern "C" long long dff_autocorr_workspace_bytes(long long n, int d, int max_lag) {
    if (ac_check_shape(n, d, max_lag, "autocorr_workspace_bytes")) return -1;
    if (n == 0) return 0;
    const AcShape sh(n, d, max_lag);
    return (long long)(sh.left_bytes(n) + sh.part_bytes(d));
}

extern "C" int dff_autocorr(int device, const double* series, long long n, int d, const long long* lengths, int n_traj,
                            int max_lag, const double* shift, double* sxy, double* sx, double* sy, uint64_t* count,
                            void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = ac_check_shape(n, d, max_lag, "autocorr");
    if (rc) return rc;
    if ((rc = traj_check_lengths(lengths, n_traj, n, "autocorr"))) return rc;
    if (!series && n > 0) return fail(DFF_EINVAL, "autocorr: null series");
    if (!sxy) return fail(DFF_EINVAL, "autocorr: null sxy");
    const long long need = dff_autocorr_workspace_bytes(n, d, max_lag);
    if ((rc = check_workspace8(workspace, workspace_bytes, need, "autocorr"))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    const size_t nlags = (size_t)max_lag + 1;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(sxy, 0, nlags * d * sizeof(double), stream));
        if (sx) HIPCHK(hipMemsetAsync(sx, 0, nlags * d * sizeof(double), stream));
        if (sy) HIPCHK(hipMemsetAsync(sy, 0, nlags * d * sizeof(double), stream));
        if (count) HIPCHK(hipMemsetAsync(count, 0, nlags * sizeof(uint64_t), stream));
        return DFF_OK;
    }
    const AcShape sh(n, d, max_lag);
    int* left = (int*)workspace;
    double* part = (double*)((char*)workspace + sh.left_bytes(n));
    if ((rc = traj_launches(lengths, n_traj, n, [&](const TransRuns& runs) -> int {
            const long long wgs = (runs.end - runs.begin + DFF_AC_THREADS - 1) / DFF_AC_THREADS;
            hipLaunchKernelGGL(dff_ac_left_kernel, dim3((unsigned)(wgs < 4096 ? wgs : 4096)), dim3(DFF_AC_THREADS), 0, stream,
                               runs, left);
            HIPCHK(hipGetLastError());
            return DFF_OK;
        })))
        return rc;
    const bool full = sx || sy || count;
    const int K = full ? 3 * d + 1 : d;
    const dim3 grid((unsigned)sh.slots, (unsigned)sh.chunks, (unsigned)d);
    if (full)
        hipLaunchKernelGGL(dff_ac_pairs_kernel<true>, grid, dim3(DFF_AC_THREADS), 0, stream, series, n, d, max_lag, shift,
                           (const int*)left, sh.ntiles, part);
    else
        hipLaunchKernelGGL(dff_ac_pairs_kernel<false>, grid, dim3(DFF_AC_THREADS), 0, stream, series, n, d, max_lag, shift,
                           (const int*)left, sh.ntiles, part);
    HIPCHK(hipGetLastError());
    const long long nred = (long long)K * sh.nlags;
    hipLaunchKernelGGL(dff_ac_reduce_kernel, dim3((unsigned)((nred + 15) / 16)), dim3(DFF_AC_THREADS), 0, stream, (const double*)part, sh.slots, d, sh.nlags, K, sxy, sx, sy,
                       (unsigned long long*)count);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Markov state models: microstate k-means, transition counts, reversible estimator (dff_msm.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_micro_chunk(void) { return DFF_MICRO_CHUNK; }

static int micro_check_count(int K, const char* what, const char* noun) {
    if (K < 1 || K > DFF_MSM_MAXK) return fail(DFF_EINVAL, "%s: the number of %s must be 1..%d", what, noun, DFF_MSM_MAXK);
    return DFF_OK;
}

static long long micro_chunks(long long n) { return (n + DFF_MICRO_CHUNK - 1) / DFF_MICRO_CHUNK; }

static int micro_check_shape(long long n, int d, int K, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative point count", what);
    if (micro_chunks(n) > 0x7fffffffLL) return fail(DFF_EINVAL, "%s: too many points", what);
    if (d < 1 || d > DFF_KM_MAXD) return fail(DFF_EINVAL, "%s: d must be 1..%d", what, DFF_KM_MAXD);
    return micro_check_count(K, what, "centres");
}

extern "C" long long dff_micro_kmeans_workspace_bytes(long long n, int d, int K) {
    if (micro_check_shape(n, d, K, "micro_kmeans_workspace_bytes")) return -1;
    return micro_chunks(n) * ((long long)K * (d + 1) + 1) * (long long)sizeof(double);
}

extern "C" int dff_micro_kmeans_step(int device, const double* pts, long long n, int d, const double* centers, int K,
                                     int32_t* labels, double* dist2, double* sums, uint64_t* counts, double* inertia,
                                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = micro_check_shape(n, d, K, "micro_kmeans_step")) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    return kmeans_call(device, pts, n, d, centers, K, labels, dist2, sums, counts, inertia, workspace, workspace_bytes,
                       dff_micro_kmeans_workspace_bytes(n, d, K), sizeof(double), stream, "micro_kmeans_step",
                       [&](bool accumulate) -> int {
        const unsigned grid = (unsigned)micro_chunks(n);
        const int groups = accumulate ? micro_groups(d, K) : 0;
        const unsigned lds = (unsigned)micro_lds_bytes(d, K, groups);              // <= 160 KB
        if (accumulate) {
            if (lds > 48 * 1024)
                HIPCHK(hipFuncSetAttribute((const void*)&dff_micro_kmeans_kernel<true>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(dff_micro_kmeans_kernel<true>, dim3(grid), dim3(DFF_MICRO_THREADS), lds, stream, pts, n, d,
                               centers, K, labels, dist2, (double*)workspace, groups);
            HIPCHK(hipGetLastError());
            const int per = K * (d + 1) + 1;
            hipLaunchKernelGGL(dff_micro_kmeans_reduce_kernel, dim3((unsigned)((per + 63) / 64)), dim3(256), 0, stream,
                               (const double*)workspace, (long long)grid, d, K, sums, (unsigned long long*)counts, inertia);
        } else {
            if (lds > 48 * 1024)
                HIPCHK(hipFuncSetAttribute((const void*)&dff_micro_kmeans_kernel<false>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(dff_micro_kmeans_kernel<false>, dim3(grid), dim3(DFF_MICRO_THREADS), lds, stream, pts, n, d,
                               centers, K, labels, dist2, (double*)nullptr, 1);
        }
        HIPCHK(hipGetLastError());
        return DFF_OK;
    });
}

extern "C" int dff_micro_transition_counts(int device, const int32_t* labels, long long n, const long long* lengths,
                                           int n_traj, const int32_t* lags, int n_lags, int K, uint64_t* counts,
                                           void* stream_) {
    if ((!labels && n > 0) || n < 0) return fail(DFF_EINVAL, "micro_transition_counts: null labels / negative count");
    int rc = micro_check_count(K, "micro_transition_counts", "states");
    if (rc) return rc;
    if ((rc = tc_check_lags(lags, n_lags, "micro_transition_counts"))) return rc;
    if ((rc = traj_check_lengths(lengths, n_traj, n, "micro_transition_counts"))) return rc;
    if (!counts) return fail(DFF_EINVAL, "micro_transition_counts: null counts");
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)n_lags * K * K * sizeof(uint64_t), stream));
    if (n == 0) return DFF_OK;
    // few states: the counters of a group of lags fit in LDS, and a metastable path hammers a handful of them -- the
    // privatised kernel of dff_transition_counts (integer counts: the same result either way)
    if (K <= DFF_STATES_MAXK) return tc_launches(stream, labels, n, lengths, n_traj, lags, n_lags, K, counts);
    TransLags g;
    g.n = n_lags;
    for (int l = 0; l < DFF_TC_MAXLAGS; ++l) g.lag[l] = l < n_lags ? lags[l] : 0;
    return traj_launches(lengths, n_traj, n, [&](const TransRuns& runs) -> int {
        const long long wgs = (runs.end - runs.begin + DFF_TC_THREADS - 1) / DFF_TC_THREADS;
        hipLaunchKernelGGL(dff_micro_tc_kernel, dim3((unsigned)(wgs < 4 * DFF_TC_WGS ? wgs : 4 * DFF_TC_WGS)),
                           dim3(DFF_TC_THREADS), 0, stream, labels, K, runs, g, (unsigned long long*)counts);
        HIPCHK(hipGetLastError());
        return DFF_OK;
    });
}

// which kernel drives the sweeps: 0 = by the number of states, 1 = one launch per sweep, 2 = one workgroup for all sweeps
static std::atomic<int> g_msm_driver{0};
#define DFF_MSM_LOOP_MAXK 32       // automatic choice: the one-workgroup loop up to this many states (measured: DESIGN.md section 17)

extern "C" int dff_debug_msm_driver(int driver) {
    if (driver < 0 || driver > 2) return fail(DFF_EINVAL, "debug_msm_driver: 0 (automatic), 1 (launch per sweep) or 2 (one workgroup)");
    g_msm_driver.store(driver);
    return DFF_OK;
}

// The driver for n_live problems of up to kmax states (the single call: n_live = 1).  One looping workgroup per problem pays no
// launch per sweep but uses one CU per problem, so beyond DFF_MSM_LOOP_MAXK states it wants enough problems to cover what the
// largest of them costs: measured it wins from 4 problems on at K = 64, from 8 at K = 128 and 256, from
// 16 at K = 512 and from 32 at K = 1024 -- never for one problem.
static int msm_driver(int kmax, int n_live) {
    const int driver = g_msm_driver.load();
    if (driver) return driver;
    if (kmax <= DFF_MSM_LOOP_MAXK) return 2;
    return (32LL * n_live >= kmax && n_live >= (kmax >= 128 ? 8 : 4)) ? 2 : 1;
}

// n_steps sweeps of the n_prob problems of `loc`, the largest of kmax states, enqueued on `stream`: driver 2, one looping
// workgroup per problem; driver 1, q0 <- (rowc, x), then one launch per sweep with q ping-ponging q0 <-> q1.  err: sweep s at
// err + s * loc.err_stride(), or null.
template <class Loc>
static int msm_sweeps(hipStream_t stream, Loc loc, int driver, int kmax, unsigned n_prob, const double* sym,
                      const double* rowc, double* x, int n_steps, double* q0, double* q1, unsigned long long* err) {
    if (driver == 2) {
        hipLaunchKernelGGL(dff_msm_loop_kernel<Loc>, dim3(n_prob), dim3(DFF_MSM_LOOP_THREADS), (unsigned)(3 * kmax * sizeof(double)),
                           stream, sym, rowc, loc, x, n_steps, err);
        HIPCHK(hipGetLastError());
        return DFF_OK;
    }
    double* q[2] = {q0, q1};
    hipLaunchKernelGGL(dff_msm_init_kernel<Loc>, dim3((unsigned)((kmax + 255) / 256), n_prob), dim3(256), 0, stream, rowc,
                       (const double*)x, loc, q[0]);
    const dim3 grid((unsigned)((kmax + DFF_MSM_THREADS / 64 - 1) / (DFF_MSM_THREADS / 64)), n_prob);
    for (int s = 0; s < n_steps; ++s)
        hipLaunchKernelGGL(dff_msm_sweep_kernel<Loc>, grid, dim3(DFF_MSM_THREADS), 0, stream, sym, rowc, loc, x,
                           (const double*)q[s & 1], q[(s + 1) & 1], err ? err + (size_t)s * loc.err_stride() : nullptr);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" int dff_msm_driver_for(int K) {
    if (micro_check_count(K, "msm_driver_for", "states")) return -1;
    return msm_driver(K, 1);
}

extern "C" long long dff_msm_workspace_bytes(int K) {
    if (micro_check_count(K, "msm_workspace_bytes", "states")) return -1;
    return 2LL * K * (long long)sizeof(double);                        // q ping | q pong
}

extern "C" int dff_msm_reversible_steps(int device, const double* sym, const double* rowc, int K, double* x, int n_steps,
                                        double* err, void* workspace, size_t workspace_bytes, void* stream_) {
    int rc = micro_check_count(K, "msm_reversible_steps", "states");
    if (rc) return rc;
    if (n_steps < 0) return fail(DFF_EINVAL, "msm_reversible_steps: negative n_steps");
    if (!sym || !rowc || !x) return fail(DFF_EINVAL, "msm_reversible_steps: null matrix / row counts / x");
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_msm_workspace_bytes(K), "msm_reversible_steps"))) return rc;
    if (n_steps == 0) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (err) HIPCHK(hipMemsetAsync(err, 0, (size_t)n_steps * sizeof(double), stream));
    return msm_sweeps(stream, MsmOne{K}, msm_driver(K, 1), K, 1, sym, rowc, x, n_steps, (double*)workspace,
                      (double*)workspace + K, (unsigned long long*)err);
}

// ---------------------------------------------------------------------------------------------
// Bootstrap of a Markov state model: resampled counts, batched estimator (dff_msm_batch.hip)
// ---------------------------------------------------------------------------------------------
// `cnt` 64-bit words of a host table into the workspace, as kernel arguments: nothing the stream could make the host wait for
static int msmb_upload(hipStream_t stream, const long long* src, long long cnt, long long* dst) {
    for (long long o = 0; o < cnt; o += DFF_MSMB_UPLOAD) {
        MsmbWords w;
        const int m = (int)(cnt - o < DFF_MSMB_UPLOAD ? cnt - o : DFF_MSMB_UPLOAD);
        for (int i = 0; i < m; ++i) w.v[i] = src[o + i];
        hipLaunchKernelGGL(dff_msmb_upload_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, stream, w, m, dst + o);
    }
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

static int msmb_check_batch(int B, const char* what, const char* noun) {
    if (B < 1 || B > DFF_MSMB_MAXB) return fail(DFF_EINVAL, "%s: the number of %s must be 1..%d", what, noun, DFF_MSMB_MAXB);
    return DFF_OK;
}

static int rc_check_units(int n_units, const char* what) {
    if (n_units < 1 || n_units > DFF_RC_MAXUNITS)
        return fail(DFF_EINVAL, "%s: the number of resampling units must be 1..%d", what, DFF_RC_MAXUNITS);
    return DFF_OK;
}

extern "C" long long dff_micro_resampled_counts_workspace_bytes(int n_traj, int n_units) {
    if (n_traj < 0) return fail(DFF_EINVAL, "micro_resampled_counts_workspace_bytes: negative trajectory count"), -1;
    if (rc_check_units(n_units, "micro_resampled_counts_workspace_bytes")) return -1;
    return ((long long)n_traj + 1 + (long long)n_units + 1) * (long long)sizeof(long long);   // trajectory starts | unit starts
}

extern "C" int dff_micro_resampled_counts(int device, const int32_t* labels, long long n, const long long* lengths,
                                          int n_traj, const long long* unit_lengths, int n_units, int lag, int K,
                                          const uint32_t* weights, int B, uint64_t* counts, void* workspace,
                                          size_t workspace_bytes, void* stream_) {
    const char* what = "micro_resampled_counts";
    if ((!labels && n > 0) || n < 0) return fail(DFF_EINVAL, "%s: null labels / negative count", what);
    if (n > (1LL << 31)) return fail(DFF_EINVAL, "%s: more than 2^31 frames", what);
    int rc = micro_check_count(K, what, "states");
    if (rc) return rc;
    if ((rc = msmb_check_batch(B, what, "resamples"))) return rc;
    if ((long long)B * K * K > DFF_RC_MAXCOUNTERS) return fail(DFF_EINVAL, "%s: B K^2 must not exceed 2^28 counters", what);
    if ((rc = rc_check_units(n_units, what))) return rc;
    if (lag < 1) return fail(DFF_EINVAL, "%s: lag time is %d, must be >= 1", what, lag);
    if ((rc = traj_check_lengths(lengths, n_traj, n, what))) return rc;
    if (!unit_lengths) return fail(DFF_EINVAL, "%s: null unit lengths", what);
    long long total = 0;
    for (int u = 0; u < n_units; ++u) {
        if (unit_lengths[u] < 0) return fail(DFF_EINVAL, "%s: unit %d has negative length", what, u);
        if (unit_lengths[u] > n - total) return fail(DFF_EINVAL, "%s: unit lengths sum to more than n = %lld", what, n);
        total += unit_lengths[u];
    }
    if (total != n) return fail(DFF_EINVAL, "%s: unit lengths sum to %lld, not n = %lld", what, total, n);
    if (!weights || !counts) return fail(DFF_EINVAL, "%s: null weights / counts", what);
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_micro_resampled_counts_workspace_bytes(n_traj, n_units), what)))
        return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)B * K * K * sizeof(uint64_t), stream));
    if (n == 0) return DFF_OK;
    std::vector<long long> starts((size_t)n_traj + 1 + n_units + 1);
    long long* ts = starts.data();
    long long* us = ts + n_traj + 1;
    ts[0] = us[0] = 0;
    for (int i = 0; i < n_traj; ++i) ts[i + 1] = ts[i] + lengths[i];
    for (int u = 0; u < n_units; ++u) us[u + 1] = us[u] + unit_lengths[u];
    if ((rc = msmb_upload(stream, ts, (long long)starts.size(), (long long*)workspace))) return rc;
    const long long* tstart = (const long long*)workspace;
    const long long wgs = (n + DFF_TC_THREADS - 1) / DFF_TC_THREADS;
    hipLaunchKernelGGL(dff_micro_rc_kernel, dim3((unsigned)(wgs < 4 * DFF_TC_WGS ? wgs : 4 * DFF_TC_WGS)), dim3(DFF_TC_THREADS), 0,
                       stream, labels, n, lag, K, tstart, n_traj, tstart + n_traj + 1, n_units, weights, B,
                       (unsigned long long*)counts);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" long long dff_msm_batched_workspace_bytes(int B, int Kmax) {
    if (msmb_check_batch(B, "msm_batched_workspace_bytes", "problems")) return -1;
    if (micro_check_count(Kmax, "msm_batched_workspace_bytes", "states")) return -1;
    return (2LL * B * Kmax + B) * (long long)sizeof(double);            // q ping | q pong | the live problems' descriptors
}

extern "C" int dff_msm_batched_driver_for(int B, int Kmax) {
    if (msmb_check_batch(B, "msm_batched_driver_for", "problems")) return -1;
    if (micro_check_count(Kmax, "msm_batched_driver_for", "states")) return -1;
    return msm_driver(Kmax, B);
}

// ---------------------------------------------------------------------------------------------
// What the batched solvers share: the problem table, the path knobs, the two-path launch
// ---------------------------------------------------------------------------------------------
// The problem table of a call (dff_msm_table.h), checked and packed on the host: one word per live problem, in order.
struct MsmTable {
    std::vector<long long> desc;
    int kmin_live = DFF_MSM_MAXK, kmax_live = 0;

    // ks[0 .. P - 1] against Kmax.  slot_of (null: problem p takes slot p) against n_slots, `noun` naming what a slot holds; a
    // null noun: the table carries no slots, bare counts.  agree: problems that share a slot must agree on K_p.  forced_max > 0:
    // the largest K_p a forced LDS path takes.  skip (or null): problems that are checked, but not live.  Refusals problem by problem.
    int build(const char* what, const int32_t* ks, int P, int Kmax, const int32_t* slot_of, int n_slots, const char* noun, bool agree,
              int forced_max, const uint8_t* skip) {
        std::vector<int> k_of(agree ? (size_t)n_slots : 0, 0);
        desc.reserve((size_t)P);
        for (int p = 0; p < P; ++p) {
            const int K = ks[p], slot = slot_of ? slot_of[p] : p;
            if (K < 1 || K > Kmax) return fail(DFF_EINVAL, "%s: problem %d has %d states, must be 1..Kmax = %d", what, p, K, Kmax);
            if (slot_of && (slot < 0 || slot >= n_slots))
                return fail(DFF_EINVAL, "%s: problem %d takes %s %d of %d", what, p, noun, slot, n_slots);
            if (agree) {
                int& km = k_of[(size_t)slot];
                if (km && km != K)
                    return fail(DFF_EINVAL, "%s: problem %d reads %s %d with %d states, an earlier problem with %d", what, p, noun, slot, K, km);
                km = K;
            }
            if (forced_max && K > forced_max)
                return fail(DFF_EINVAL, "%s: problem %d has %d states, the forced LDS path takes at most %d", what, p, K, forced_max);
            if (skip && skip[p]) continue;
            desc.push_back(msm_problem_pack(noun ? slot : 0, K));
            if (K > kmax_live) kmax_live = K;
            if (K < kmin_live) kmin_live = K;
        }
        return DFF_OK;
    }
    int upload(hipStream_t stream, long long* dst) const { return msmb_upload(stream, desc.data(), (long long)desc.size(), dst); }
};

// a process-wide debug knob that names a path, 0 .. max; anything else is refused with `refusal`
struct PathKnob {
    const int max;
    const char* const refusal;
    std::atomic<int> value{0};
    int set(int path) {
        if (path < 0 || path > max) return fail(DFF_EINVAL, "%s", refusal);
        value.store(path);
        return DFF_OK;
    }
};

// What differs between the three two-path calls.  A problem's SIZE is what its kernel compares with own_lo .. own_hi: K_p, or
// for the Dirichlet solver the interior count, at most K_p - 1 and known on the device only.
struct MsmTwoPath {
    const char* name;                   // as dff_debug_msm_batch_plan takes it
    const char* what;                   // the call, as its refusals name it
    PathKnob* knob;                     // 0 = by size, 1 = LDS, 2 (and above) = the other path
    int limit;                          // the largest size of the LDS path
    int size_off;                       // a problem's size is at most K_p - size_off
    int lo_all, hi_all;                 // own_lo / own_hi of "every size", as the kernels are handed them
    bool on_device;                     // sizes are found on the device: the LDS launch does not wait for a small K_p, and when
                                        // forced it takes hi_all
    size_t (*lds_bytes)(int size, bool ldsp);
    int forced_max(int path) const { return path == 1 ? limit + size_off : 0; }   // MsmTable::build's, in K_p
};

// THE selection rule of the three calls: launch[0] is the LDS kernel's, launch[1] the other path's.  Pure host arithmetic.
static dff_msm_batch_plan msm_two_path(const MsmTwoPath& r, int knob, int kmin_live, int kmax_live) {
    const int path = knob > 2 ? 2 : knob;
    dff_msm_batch_plan plan = {};
    if (path == 1 || (path == 0 && (r.on_device || kmin_live <= r.limit))) {
        const int size = kmax_live - r.size_off < r.limit ? kmax_live - r.size_off : r.limit;
        plan.launch[0] = {1, 1, r.lo_all, path == 1 && r.on_device ? r.hi_all : r.limit, size, (int32_t)r.lds_bytes(size, true)};
    }
    if (path == 2 || (path == 0 && kmax_live > r.limit)) {          // in K_p, whatever the size measure
        const int size = kmax_live - r.size_off;
        plan.launch[1] = {1, 2, path == 2 ? r.lo_all : r.limit + 1, r.hi_all, size, (int32_t)r.lds_bytes(size, false)};
    }
    return plan;
}

// one planned launch, one workgroup per problem; the kernel's arguments as the caller lists them (own_lo and own_hi among them)
template <class... Params, class... Args>
static int msm_launch_planned(void (*kernel)(Params...), const dff_msm_batch_launch& l, int P, int threads, hipStream_t stream,
                              Args... args) {
    if (!l.launched) return DFF_OK;
    if (l.lds_bytes > 64 * 1024)                                      // more than a launch gets unasked
        HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, l.lds_bytes));
    hipLaunchKernelGGL(kernel, dim3((unsigned)P), dim3((unsigned)threads), (unsigned)l.lds_bytes, stream, args...);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

static_assert(DFF_DIR_MAXP == DFF_EIG_MAXP && DFF_DIR_MAXP == DFF_PROP_MAXP, "one problem count for the batched solvers");
static int solver_check_batch(int P, int Kmax, const char* what) {
    if (P < 1 || P > DFF_DIR_MAXP) return fail(DFF_EINVAL, "%s: the number of problems must be 1..%d", what, DFF_DIR_MAXP);
    return micro_check_count(Kmax, what, "states");
}

extern "C" int dff_msm_reversible_steps_batched(int device, const double* sym, const double* rowc, const int32_t* ks,
                                                const uint8_t* skip, int B, int Kmax, double* x, int n_steps, double* err,
                                                void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "msm_reversible_steps_batched";
    int rc = msmb_check_batch(B, what, "problems");
    if (rc) return rc;
    if ((rc = micro_check_count(Kmax, what, "states"))) return rc;
    if (n_steps < 0) return fail(DFF_EINVAL, "%s: negative n_steps", what);
    if (!sym || !rowc || !x || !ks) return fail(DFF_EINVAL, "%s: null matrices / row counts / x / state counts", what);
    MsmTable live;
    if ((rc = live.build(what, ks, B, Kmax, nullptr, B, "matrix", false, 0, skip))) return rc;
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_msm_batched_workspace_bytes(B, Kmax), what))) return rc;
    if (n_steps == 0) return DFF_OK;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    if (err) HIPCHK(hipMemsetAsync(err, 0, (size_t)n_steps * B * sizeof(double), stream));
    if (live.desc.empty()) return DFF_OK;
    double* q0 = (double*)workspace;
    long long* live_dev = (long long*)(q0 + 2 * (size_t)B * Kmax);
    if ((rc = live.upload(stream, live_dev))) return rc;
    const int n_live = (int)live.desc.size();
    return msm_sweeps(stream, MsmLive{live_dev, Kmax, B}, msm_driver(live.kmax_live, n_live), live.kmax_live, (unsigned)n_live, sym,
                      rowc, x, n_steps, q0, q0 + (size_t)B * Kmax, (unsigned long long*)err);
}

// ---------------------------------------------------------------------------------------------
// Mean first-passage times and committors: the Dirichlet problem on a flux matrix (dff_msm_passage.hip)
// ---------------------------------------------------------------------------------------------
// which path factors a problem: 0 = by its interior count, 1 = LDS, 2 = the blocked one in the workspace (71 168 bytes of LDS)
static size_t dir_path_lds_bytes(int n, bool ldsp) { return ldsp ? dir_lds_bytes(n) : dir_blocked_lds_bytes(); }
static PathKnob g_dir_path{4, "debug_msm_dirichlet_path: 0 (by size), 1 (LDS), 2 (global), 3 (global, VALU) or 4 (global, MFMA)"};
static const MsmTwoPath k_dir_paths{"dirichlet", "msm_dirichlet_solve", &g_dir_path, DFF_DIR_LDS_LIMIT, 1, 0, 0x7fffffff, true,
                                    dir_path_lds_bytes};

extern "C" int dff_debug_msm_dirichlet_path(int path) { return g_dir_path.set(path); }

extern "C" int dff_msm_dirichlet_lds_limit(void) { return DFF_DIR_LDS_LIMIT; }

extern "C" long long dff_msm_dirichlet_workspace_bytes(int P, int Kmax) {
    if (solver_check_batch(P, Kmax, "msm_dirichlet_workspace_bytes")) return -1;
    return (long long)P * (1 + dir_slice_doubles(Kmax)) * (long long)sizeof(double);   // descriptors | one slice per problem
}

extern "C" int dff_msm_dirichlet_solve(int device, const double* flux, int n_flux, const int32_t* flux_of, const int32_t* ks,
                                       int P, int Kmax, const int32_t* role, const double* g, const double* s, double* u,
                                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
    const MsmTwoPath& paths = k_dir_paths;
    const char* what = paths.what;
    int rc = solver_check_batch(P, Kmax, what);
    if (rc) return rc;
    if (n_flux < 1 || n_flux > DFF_DIR_MAXP) return fail(DFF_EINVAL, "%s: the number of flux matrices must be 1..%d", what, DFF_DIR_MAXP);
    if (!flux || !ks || !role || !g || !s || !u || !status)
        return fail(DFF_EINVAL, "%s: null flux / state counts / roles / boundary values / sources / u / status", what);
    if (!flux_of && n_flux < P) return fail(DFF_EINVAL, "%s: %d flux matrices for %d problems and no flux_of", what, n_flux, P);
    const int knob = paths.knob->value.load();
    const int mfma = knob == 3 ? 0 : (knob == 4 ? 1 : DFF_DIR_MFMA);  // 3 and 4: the blocked path with a named trailing update
    MsmTable tab;
    if ((rc = tab.build(what, ks, P, Kmax, flux_of, n_flux, "flux matrix", false, paths.forced_max(knob), nullptr))) return rc;
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_msm_dirichlet_workspace_bytes(P, Kmax), what))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    long long* desc_dev = (long long*)workspace;
    if ((rc = tab.upload(stream, desc_dev))) return rc;
    double* work = (double*)(desc_dev + P);
    const long long slice = dir_slice_doubles(Kmax);
    const dff_msm_batch_plan plan = msm_two_path(paths, knob, tab.kmin_live, tab.kmax_live);
    const dff_msm_batch_launch &l0 = plan.launch[0], &l1 = plan.launch[1];
    if ((rc = msm_launch_planned(dff_dir_kernel<true>, l0, P, DFF_DIR_THREADS, stream, flux, (const long long*)desc_dev, Kmax, role, g,
                                 s, u, status, work, slice, l0.lo, l0.hi, mfma)))
        return rc;
    return msm_launch_planned(dff_dir_kernel<false>, l1, P, DFF_DIR_THREADS, stream, flux, (const long long*)desc_dev, Kmax, role, g, s,
                              u, status, work, slice, l1.lo, l1.hi, mfma);
}

// ---------------------------------------------------------------------------------------------
// The k largest eigenpairs of many symmetric matrices (dff_sym_eig.hip)
// ---------------------------------------------------------------------------------------------
// which path reduces a problem: 0 = by its size, 1 = LDS, 2 = the workspace
static PathKnob g_eig_path{2, "debug_sym_eig_path: 0 (by size), 1 (LDS) or 2 (workspace)"};
static const MsmTwoPath k_eig_paths{"eig", "sym_eig_topk", &g_eig_path, DFF_EIG_LDS_LIMIT, 0, 1, DFF_MSM_MAXK, false, eig_lds_bytes};

extern "C" int dff_debug_sym_eig_path(int path) { return g_eig_path.set(path); }

extern "C" int dff_sym_eig_lds_limit(void) { return DFF_EIG_LDS_LIMIT; }

extern "C" long long dff_sym_eig_workspace_bytes(int P, int Kmax) {
    if (solver_check_batch(P, Kmax, "sym_eig_workspace_bytes")) return -1;
    return (long long)P * (1 + eig_slice_doubles(Kmax)) * (long long)sizeof(double);   // state counts | one slice per problem
}

extern "C" int dff_sym_eig_topk(int device, const double* a, const int32_t* ks, int P, int Kmax, int k, double* w, double* v,
                                int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
    const MsmTwoPath& paths = k_eig_paths;
    const char* what = paths.what;
    int rc = solver_check_batch(P, Kmax, what);
    if (rc) return rc;
    if (k < 1 || k > DFF_EIG_MAXTOP) return fail(DFF_EINVAL, "%s: the number of eigenpairs must be 1..%d", what, DFF_EIG_MAXTOP);
    if (!a || !ks || !w || !status) return fail(DFF_EINVAL, "%s: null matrices / state counts / eigenvalues / status", what);
    const int knob = paths.knob->value.load();
    MsmTable tab;                                                     // bare counts: matrix p is problem p's
    if ((rc = tab.build(what, ks, P, Kmax, nullptr, P, nullptr, false, paths.forced_max(knob), nullptr))) return rc;
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_sym_eig_workspace_bytes(P, Kmax), what))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    long long* ks_dev = (long long*)workspace;
    if ((rc = tab.upload(stream, ks_dev))) return rc;
    double* work = (double*)(ks_dev + P);
    const long long slice = eig_slice_doubles(Kmax);
    const dff_msm_batch_plan plan = msm_two_path(paths, knob, tab.kmin_live, tab.kmax_live);
    const dff_msm_batch_launch &l0 = plan.launch[0], &l1 = plan.launch[1];
    if ((rc = msm_launch_planned(dff_sym_eig_kernel<true>, l0, P, EigCfg<true>::T, stream, a, (const long long*)ks_dev, Kmax, k, w, v,
                                 status, work, slice, l0.lo, l0.hi)))
        return rc;
    return msm_launch_planned(dff_sym_eig_kernel<false>, l1, P, EigCfg<false>::T, stream, a, (const long long*)ks_dev, Kmax, k, w, v,
                              status, work, slice, l1.lo, l1.hi);
}

// ---------------------------------------------------------------------------------------------
// Row vectors through a transition matrix, step after step (dff_msm_propagate.hip)
// ---------------------------------------------------------------------------------------------
// which path propagates a problem: 0 = by its size, 1 = LDS, 2 = the matrix streamed from global memory
static PathKnob g_prop_path{2, "debug_msm_propagate_path: 0 (by size), 1 (LDS) or 2 (workspace)"};
static const MsmTwoPath k_prop_paths{"propagate", "msm_propagate", &g_prop_path, DFF_PROP_LDS_LIMIT, 0, 1, DFF_MSM_MAXK, false,
                                     prop_lds_bytes};

extern "C" int dff_debug_msm_propagate_path(int path) { return g_prop_path.set(path); }

extern "C" int dff_msm_propagate_lds_limit(void) { return DFF_PROP_LDS_LIMIT; }

static int prop_check_batch(int P, int Kmax, int M, int R, const char* what) {
    if (P < 1 || P > DFF_PROP_MAXP) return fail(DFF_EINVAL, "%s: the number of problems must be 1..%d", what, DFF_PROP_MAXP);
    if (M < 1 || M > DFF_PROP_MAXROWS) return fail(DFF_EINVAL, "%s: the number of start vectors must be 1..%d", what, DFF_PROP_MAXROWS);
    if (R < 1 || R > DFF_PROP_MAXROWS) return fail(DFF_EINVAL, "%s: the number of observables must be 1..%d", what, DFF_PROP_MAXROWS);
    return micro_check_count(Kmax, what, "states");
}

extern "C" long long dff_msm_propagate_workspace_bytes(int P, int Kmax, int M, int R) {
    if (prop_check_batch(P, Kmax, M, R, "msm_propagate_workspace_bytes")) return -1;
    return (long long)P * (long long)sizeof(long long);              // the problem descriptors
}

extern "C" int dff_msm_propagate(int device, const double* t, int n_mat, const int32_t* mat_of, const int32_t* ks, int P, int Kmax,
                                 const double* w0, int M, const double* obs, int R, int S, double* out, double* w_last,
                                 int32_t* status, void* workspace, size_t workspace_bytes, void* stream_) {
    const MsmTwoPath& paths = k_prop_paths;
    const char* what = paths.what;
    int rc = prop_check_batch(P, Kmax, M, R, what);
    if (rc) return rc;
    if (S < 0 || S > DFF_PROP_MAXSTEPS) return fail(DFF_EINVAL, "%s: the number of steps must be 0..%d", what, DFF_PROP_MAXSTEPS);
    if ((long long)P * (S + 1) * M * R > DFF_PROP_MAXOUT)
        return fail(DFF_EINVAL, "%s: %lld output values, at most %lld per call", what, (long long)P * (S + 1) * M * R, DFF_PROP_MAXOUT);
    if (n_mat < 1 || n_mat > DFF_PROP_MAXP) return fail(DFF_EINVAL, "%s: the number of matrices must be 1..%d", what, DFF_PROP_MAXP);
    if (!t || !ks || !w0 || !obs || !out || !status)
        return fail(DFF_EINVAL, "%s: null matrices / state counts / start vectors / observables / out / status", what);
    if (!mat_of && n_mat < P) return fail(DFF_EINVAL, "%s: %d matrices for %d problems and no mat_of", what, n_mat, P);
    const int knob = paths.knob->value.load();
    MsmTable tab;
    if ((rc = tab.build(what, ks, P, Kmax, mat_of, n_mat, "matrix", true, paths.forced_max(knob), nullptr))) return rc;
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_msm_propagate_workspace_bytes(P, Kmax, M, R), what))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    long long* desc_dev = (long long*)workspace;
    if ((rc = tab.upload(stream, desc_dev))) return rc;
    const dff_msm_batch_plan plan = msm_two_path(paths, knob, tab.kmin_live, tab.kmax_live);
    const dff_msm_batch_launch &l0 = plan.launch[0], &l1 = plan.launch[1];
    if ((rc = msm_launch_planned(dff_prop_kernel<true>, l0, P, DFF_PROP_THREADS, stream, t, (const long long*)desc_dev, Kmax, w0, M, obs,
                                 R, S, out, w_last, status, l0.lo, l0.hi)))
        return rc;
    return msm_launch_planned(dff_prop_kernel<false>, l1, P, DFF_PROP_THREADS, stream, t, (const long long*)desc_dev, Kmax, w0, M, obs, R,
                              S, out, w_last, status, l1.lo, l1.hi);
}

// What one of the three calls above would launch for these state counts under its knob as it stands: host arithmetic only.
extern "C" int dff_debug_msm_batch_plan(const char* call, const int32_t* ks, int P, int Kmax, dff_msm_batch_plan* out) {
    const MsmTwoPath* paths = nullptr;
    for (const MsmTwoPath* c : {&k_dir_paths, &k_eig_paths, &k_prop_paths})
        if (call && !strcmp(call, c->name)) paths = c;
    if (!paths) return fail(DFF_EINVAL, "debug_msm_batch_plan: the call must be dirichlet, eig or propagate");
    if (!ks || !out) return fail(DFF_EINVAL, "debug_msm_batch_plan: null state counts / plan");
    int rc = solver_check_batch(P, Kmax, paths->what);
    if (rc) return rc;
    const int knob = paths->knob->value.load();
    MsmTable tab;
    if ((rc = tab.build(paths->what, ks, P, Kmax, nullptr, P, nullptr, false, paths->forced_max(knob), nullptr))) return rc;
    *out = msm_two_path(*paths, knob, tab.kmin_live, tab.kmax_live);
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: one E-step of Baum-Welch over all chains (dff_hmm.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_hmm_chunk(void) { return DFF_HMM_CHUNK; }

// how many of the call's launches run: 0 = all of them; 1 .. 5 = stop after the parameters, the chunk products, the carries, the
// apply pass, the emission counts (benchmarks: the share of every launch, by differences; the outputs are then unfinished)
static std::atomic<int> g_hmm_stages{0};

extern "C" int dff_debug_hmm_stages(int stages) {
    if (stages < 0 || stages > 5) return fail(DFF_EINVAL, "debug_hmm_stages: 0 (all) or 1 .. 5 launches");
    g_hmm_stages.store(stages);
    return DFF_OK;
}

// chains and chunks of a call, and (cpre != null) the chunks before every trajectory: cpre[0 .. n_traj]
static int hmm_plan(const long long* lengths, int n_traj, int lag, long long* n_chains, long long* n_chunks, long long* cpre,
                    const char* what) {
    if (lag < 1) return fail(DFF_EINVAL, "%s: lag must be >= 1", what);
    if (n_traj < 0 || (n_traj > 0 && !lengths)) return fail(DFF_EINVAL, "%s: null / negative trajectory lengths", what);
    if ((long long)n_traj * lag > DFF_HMM_MAXCHAINS)
        return fail(DFF_EINVAL, "%s: %lld chains, at most %d", what, (long long)n_traj * lag, DFF_HMM_MAXCHAINS);
    long long chunks = 0;
    for (int r = 0; r < n_traj; ++r) {
        if (lengths[r] < 0) return fail(DFF_EINVAL, "%s: trajectory %d has negative length", what, r);
        if (cpre) cpre[r] = chunks;
        const auto [q, rem] = hmm_split(lengths[r], lag);
        chunks += rem * hmm_chunks_of(q + 1) + (lag - rem) * hmm_chunks_of(q);
    }
    if (cpre) cpre[n_traj] = chunks;
    if (n_chains) *n_chains = (long long)n_traj * lag;
    if (n_chunks) *n_chunks = chunks;
    return DFF_OK;
}

extern "C" int dff_hmm_plan(const long long* lengths, int n_traj, int lag, long long* n_chains, long long* n_chunks) {
    return hmm_plan(lengths, n_traj, lag, n_chains, n_chunks, nullptr, "hmm_plan");
}

static int hmm_check_shape(long long n, int m, int K, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (n > (1LL << 31)) return fail(DFF_EINVAL, "%s: more than 2^31 frames", what);
    if (m < 1 || m > DFF_HMM_MAXM) return fail(DFF_EINVAL, "%s: the number of hidden states must be 1..%d", what, DFF_HMM_MAXM);
    return micro_check_count(K, what, "symbols");
}

// the packed statistics of an E-step: loglik | xi (m, m) | gamma0 (m) | gamma_sym (m, K)
static long long hmm_nstats(int m, int K) { return 1 + (long long)m * m + m + (long long)m * K; }

// f(std::integral_constant<int, MP>()) for MP = hmm_pad(m): the one place that turns m hidden states into a template argument
template <class F>
static int hmm_with_pad(int m, F f) {
    switch (hmm_pad(m)) {
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// a workspace cut into sections, each a multiple of 16 bytes.  Every hidden-Markov-model call starts its own with the
// trajectory table (HmmPlan) and the four flag words.
struct HmmSections {
    size_t total = 0, tab, flags;
    explicit HmmSections(int n_traj) {
        tab = take(2 * ((size_t)n_traj + 1) * sizeof(long long));
        flags = take(4 * sizeof(int));
    }
    size_t take(size_t bytes) {
        const size_t at = total;
        total += (bytes + 15) & ~(size_t)15;
        return at;
    }
};

struct HmmLayout : HmmSections {
    size_t a, p0, bt, prod, pexp, ain, bout, ll, post, part;
    HmmLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K) : HmmSections(n_traj) {
        const size_t MP = (size_t)hmm_pad(m), d = sizeof(double);
        a = take(MP * MP * d);
        p0 = take(MP * d);
        bt = take((size_t)K * MP * d);
        prod = take((size_t)n_chunks * MP * MP * d);                // the chunk products, then the chunks' sums of xi
        pexp = take((size_t)n_chunks * MP * sizeof(int));
        ain = take((size_t)n_chunks * MP * d);
        bout = take((size_t)n_chunks * MP * d);
        ll = take((size_t)n_chains * d);
        post = take((size_t)n * m * d);
        part = take((size_t)((n + DFF_HMM_GROUP - 1) / DFF_HMM_GROUP) * K * m * d);
    }
};

// the bytes of a call whose workspace is a Layout, or -1 behind the refusal that the call itself would give
template <class Layout>
static long long hmm_workspace_bytes(const char* what, long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    if (hmm_check_shape(n, m, K, what)) return -1;
    long long n_chains, n_chunks;
    if (hmm_plan(lengths, n_traj, lag, &n_chains, &n_chunks, nullptr, what)) return -1;
    if (traj_check_lengths(lengths, n_traj, n, what)) return -1;
    return (long long)Layout(n, n_traj, n_chains, n_chunks, m, K).total;
}

extern "C" long long dff_hmm_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<HmmLayout>("hmm_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

// What dff_hmm_estep, dff_hmm_fit_steps and dff_hmm_viterbi do before and after their own argument checks: check() is the
// refusals they share, in their order; workspace() follows the caller's own checks; upload(), behind ON_DEVICE, puts the
// trajectory table at the head of the workspace and names it in a plan.
struct HmmCall {
    const char* what;
    const long long* lengths = nullptr;
    int n_traj = 0, lag = 0;
    long long n_chains = 0, n_chunks = 0;
    std::vector<long long> tab;                                     // off[0 .. n_traj] | cpre[0 .. n_traj]; upload() fills off
    explicit HmmCall(const char* what) : what(what) {}

    // shape, null labels, plan, trajectory lengths
    int check(const int32_t* labels, long long n, const long long* lengths_, int n_traj_, int lag_, int m, int K) {
        lengths = lengths_, n_traj = n_traj_, lag = lag_;
        int rc = hmm_check_shape(n, m, K, what);
        if (rc) return rc;
        if (!labels && n > 0) return fail(DFF_EINVAL, "%s: null labels", what);
        tab.assign(2 * ((size_t)(n_traj > 0 ? n_traj : 0) + 1), 0);
        if ((rc = hmm_plan(lengths, n_traj, lag, &n_chains, &n_chunks, tab.data() + tab.size() / 2, what))) return rc;
        return traj_check_lengths(lengths, n_traj, n, what);
    }

    int workspace(const void* ws, size_t ws_bytes, const HmmSections& lay) const {
        const int rc = check_workspace(ws, ws_bytes, (long long)lay.total, what);
        if (rc) return rc;
        if ((uintptr_t)ws % sizeof(double)) return fail(DFF_EINVAL, "%s: the workspace must be 8-byte aligned", what);
        return DFF_OK;
    }

    int upload(hipStream_t stream, char* ws, const HmmSections& lay, HmmPlan* pl) {
        for (int r = 0; r < n_traj; ++r) tab[r + 1] = tab[r] + lengths[r];
        long long* dst = (long long*)(ws + lay.tab);
        pl->off = dst;
        pl->cpre = dst + tab.size() / 2;
        pl->n_traj = n_traj;
        pl->lag = lag;
        return msmb_upload(stream, tab.data(), (long long)tab.size(), dst);
    }
};

template <int MP>
static int hmm_launches(hipStream_t stream, const int32_t* labels, long long n, HmmPlan pl, long long n_chains, long long n_chunks,
                        int m, int K, const HmmLayout& lay, char* ws, double* stats, double* chain_ll, double* post) {
    const double* A = (const double*)(ws + lay.a);
    const double* p0 = (const double*)(ws + lay.p0);
    const double* Bt = (const double*)(ws + lay.bt);
    double* prod = (double*)(ws + lay.prod);
    int* pexp = (int*)(ws + lay.pexp);
    double* ain = (double*)(ws + lay.ain);
    double* bout = (double*)(ws + lay.bout);
    double* part = (double*)(ws + lay.part);
    int* flags = (int*)(ws + lay.flags);
    const long long n_groups = (n + DFF_HMM_GROUP - 1) / DFF_HMM_GROUP;
    const int stages = g_hmm_stages.load() ? g_hmm_stages.load() : 6;
    if (stages < 2) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_hmm_products_kernel<MP>, dim3((unsigned)((n_chunks * MP + DFF_HMM_THREADS - 1) / DFF_HMM_THREADS)),
                           dim3(DFF_HMM_THREADS), 0, stream, labels, pl, n_chunks, m, K, A, Bt, prod, pexp);
        HIPCHK(hipGetLastError());
    }
    if (stages < 3) return DFF_OK;
    if (n_chains > 0) {
        hipLaunchKernelGGL(dff_hmm_carry_kernel<MP>, dim3((unsigned)((n_chains + 63) / 64), 2), dim3(64), 0, stream, labels, pl,
                           n_chains, m, K, p0, Bt, (const double*)prod, (const int*)pexp, ain, bout, chain_ll, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 4) return DFF_OK;
    if (n_chunks > 0) {
        const int G = hmm_apply_groups(MP);
        const unsigned lds = (unsigned)((size_t)G * (DFF_HMM_CHUNK + 3) * MP * sizeof(double));
        if (lds > 48 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)&dff_hmm_apply_kernel<MP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dff_hmm_apply_kernel<MP>, dim3((unsigned)((n_chunks + G - 1) / G)), dim3(64), lds, stream, labels, pl,
                           n_chunks, m, K, A, p0, Bt, (const double*)ain, (const double*)bout, post, prod, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 5) return DFF_OK;
    if (n_chunks > 0) {
        const unsigned elds = (unsigned)(((size_t)K * m + (size_t)DFF_HMM_GROUP * m) * sizeof(double) + DFF_HMM_GROUP * sizeof(int));
        if (elds > 48 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)&dff_hmm_emit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)elds));
        hipLaunchKernelGGL(dff_hmm_emit_kernel, dim3((unsigned)n_groups), dim3(DFF_HMM_THREADS), elds, stream, labels, n, m, K,
                           (const double*)post, part);
        HIPCHK(hipGetLastError());
    }
    if (stages < 6) return DFF_OK;
    hipLaunchKernelGGL(dff_hmm_reduce_kernel<MP>, dim3((unsigned)hmm_nstats(m, K)), dim3(64), 0, stream, pl, n_chains, n_chunks, n_chunks > 0 ? n_groups : 0, m, K,
                       (const double*)chain_ll, (const double*)prod, (const double*)post, (const double*)part, stats);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// One E-step on the stream: the parameters into the workspace, hmm_launches, then status and NaN.  dff_hmm_estep is one pass,
// dff_hmm_fit_steps one per iteration: the fit's E-step is this code, not a copy of it.  chain_loglik and post may be null: the
// launches then work in the workspace's sections, and finish gets them as given, so it only rewrites what the caller sees.
// With dff_debug_hmm_stages set the pass stops where hmm_launches stopped, before finish.
static int hmm_estep_pass(hipStream_t stream, const int32_t* labels, long long n, const HmmPlan& pl, const HmmCall& call,
                          const double* trans, const double* emit, const double* init, int m, int K, const HmmLayout& lay,
                          char* ws, double* stats, double* chain_loglik, double* post, int32_t* status) {
    hipLaunchKernelGGL(dff_hmm_prep_kernel, dim3(1), dim3(1024), 0, stream, trans, emit, init, m, K, hmm_pad(m),
                       (double*)(ws + lay.a), (double*)(ws + lay.p0), (double*)(ws + lay.bt), (int*)(ws + lay.flags));
    HIPCHK(hipGetLastError());
    double* ll = chain_loglik ? chain_loglik : (double*)(ws + lay.ll);
    double* pp = post ? post : (double*)(ws + lay.post);
    const int rc = hmm_with_pad(m, [&](auto mp) {
        return hmm_launches<decltype(mp)::value>(stream, labels, n, pl, call.n_chains, call.n_chunks, m, K, lay, ws, stats, ll, pp);
    });
    if (rc || g_hmm_stages.load()) return rc;
    const long long nstats = hmm_nstats(m, K);
    long long most = nstats > call.n_chains ? nstats : call.n_chains;
    if (post && n * m > most) most = n * m;
    const long long blocks = (most + DFF_HMM_THREADS - 1) / DFF_HMM_THREADS;
    hipLaunchKernelGGL(dff_hmm_finish_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(DFF_HMM_THREADS), 0, stream,
                       (const int*)(ws + lay.flags), nstats, stats, call.n_chains, chain_loglik, n * m, post, status);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" int dff_hmm_estep(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                             const double* trans, const double* emit, const double* init, int m, int K, double* stats,
                             double* chain_loglik, double* post, int32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream_) {
    HmmCall call("hmm_estep");
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    if (!trans || !emit || !init || !stats || !status)
        return fail(DFF_EINVAL, "%s: null transition matrix / emissions / initial distribution / stats / status", call.what);
    const HmmLayout lay(n, n_traj, call.n_chains, call.n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;
    return hmm_estep_pass(stream, labels, n, pl, call, trans, emit, init, m, K, lay, ws, stats, chain_loglik, post, status);
}

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: Baum-Welch on the device, n_steps iterations per call (dff_hmm_mstep.hip)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dff_hmm_fit_state) == 32, "dff_hmm_fit_state is 32 bytes");

// the workspace of a fit: the sections of the E-step, then two more of the same kind, the E-step's packed statistics and its
// status word (one int in a section of 16 bytes)
struct HmmFitLayout : HmmLayout {
    size_t stats, status;
    HmmFitLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K)
        : HmmLayout(n, n_traj, n_chains, n_chunks, m, K) {
        stats = take((size_t)hmm_nstats(m, K) * sizeof(double));
        status = take(sizeof(int));
    }
};

extern "C" long long dff_hmm_fit_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<HmmFitLayout>("hmm_fit_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

extern "C" int dff_hmm_fit_steps(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                                 double* trans, double* emit, double* init, int m, int K, int reversible, int n_steps,
                                 double accuracy, double rev_tol, long long rev_max_sweeps, double* loglik, double* stationary,
                                 dff_hmm_fit_state* state, void* workspace, size_t workspace_bytes, void* stream_) {
    HmmCall call("hmm_fit_steps");
    const char* what = call.what;
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    if (!trans || !emit || !init || !loglik || !state)
        return fail(DFF_EINVAL, "%s: null transition matrix / emissions / initial distribution / log-likelihoods / state", what);
    if (reversible != 0 && reversible != 1) return fail(DFF_EINVAL, "%s: reversible must be 0 or 1", what);
    if (n_steps < 1) return fail(DFF_EINVAL, "%s: n_steps must be >= 1", what);
    if (!(accuracy > 0.0)) return fail(DFF_EINVAL, "%s: accuracy must be > 0", what);
    if (!(rev_tol > 0.0)) return fail(DFF_EINVAL, "%s: rev_tol must be > 0", what);
    if (rev_max_sweeps < 1) return fail(DFF_EINVAL, "%s: rev_max_sweeps must be >= 1", what);
    if ((uintptr_t)state % sizeof(double)) return fail(DFF_EINVAL, "%s: the state must be 8-byte aligned", what);
    if (g_hmm_stages.load()) return fail(DFF_EINVAL, "%s: dff_debug_hmm_stages is set: the E-step would stop early", what);
    const HmmFitLayout lay(n, n_traj, call.n_chains, call.n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;     // once per call
    double* stats = (double*)(ws + lay.stats);
    int* status = (int*)(ws + lay.status);
    for (int s = 0; s < n_steps; ++s) {
        // the E-step of dff_hmm_estep, no output but its statistics and its status, both in the workspace
        if ((rc = hmm_estep_pass(stream, labels, n, pl, call, trans, emit, init, m, K, lay, ws, stats, nullptr, nullptr, status)))
            return rc;
        // control and M-step: one workgroup
        hipLaunchKernelGGL(dff_hmm_fit_mstep_kernel, dim3(1), dim3(DFF_HMM_FIT_THREADS), 0, stream, (const double*)stats,
                           (const int*)status, state, trans, emit, init, m, K, reversible, accuracy, rev_tol, rev_max_sweeps,
                           loglik + s, stationary);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: the most probable hidden path of every chain (dff_hmm_viterbi.hip)
// ---------------------------------------------------------------------------------------------
// how many of the call's launches run: 0 = all of them; 1 .. 6 = stop after the parameters, the chunk products, the forward
// carries, the apply pass, the backward carries, the backtrack (benchmarks: the share of every launch, by differences; the
// outputs are then unfinished)
static std::atomic<int> g_vit_stages{0};

extern "C" int dff_debug_hmm_viterbi_stages(int stages) {
    if (stages < 0 || stages > 6) return fail(DFF_EINVAL, "debug_hmm_viterbi_stages: 0 (all) or 1 .. 6 launches");
    g_vit_stages.store(stages);
    return DFF_OK;
}

struct VitLayout : HmmSections {
    size_t la, lp, lbt, prod, din, psi, origin, end, endstate, clp;
    VitLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K) : HmmSections(n_traj) {
        const size_t MP = (size_t)hmm_pad(m), d = sizeof(double);
        la = take(MP * MP * d);
        lp = take(MP * d);
        lbt = take((size_t)K * MP * d);
        prod = take((size_t)n_chunks * MP * MP * d);
        din = take((size_t)n_chunks * MP * d);
        psi = take((size_t)n * sizeof(unsigned));                   // one word of back-pointers per frame, in chain order
        origin = take((size_t)n_chunks * sizeof(unsigned));
        end = take((size_t)n_chunks * sizeof(int));
        endstate = take((size_t)n_chains * sizeof(int));
        clp = take((size_t)n_chains * d);
    }
};

extern "C" long long dff_hmm_viterbi_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<VitLayout>("hmm_viterbi_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

template <int MP>
static int vit_launches(hipStream_t stream, const int32_t* labels, HmmPlan pl, long long n_chains, long long n_chunks, int K,
                        const VitLayout& lay, char* ws, int32_t* path, int chain_order, double* chain_lp) {
    const double* la = (const double*)(ws + lay.la);
    const double* lp = (const double*)(ws + lay.lp);
    const double* lbt = (const double*)(ws + lay.lbt);
    double* prod = (double*)(ws + lay.prod);
    double* din = (double*)(ws + lay.din);
    unsigned* psi = (unsigned*)(ws + lay.psi);
    unsigned* origin = (unsigned*)(ws + lay.origin);
    int* end = (int*)(ws + lay.end);
    int* endstate = (int*)(ws + lay.endstate);
    int* flags = (int*)(ws + lay.flags);
    const int stages = g_vit_stages.load() ? g_vit_stages.load() : 7;
    const unsigned lane_blocks = (unsigned)((n_chunks * MP + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS);
    if (stages < 2) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_products_kernel<MP>, dim3(lane_blocks), dim3(DFF_VIT_THREADS), 0, stream, labels, pl, n_chunks, K,
                           la, lbt, prod);
        HIPCHK(hipGetLastError());
    }
    if (stages < 3) return DFF_OK;
    if (n_chains > 0) {
        hipLaunchKernelGGL(dff_vit_forward_kernel<MP>, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, stream, labels, pl,
                           n_chains, K, lp, lbt, (const double*)prod, din, chain_lp);
        HIPCHK(hipGetLastError());
    }
    if (stages < 4) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_apply_kernel<MP>, dim3(lane_blocks), dim3(DFF_VIT_THREADS), 0, stream, labels, pl, n_chunks, K, la,
                           lbt, (const double*)din, psi, origin, endstate, chain_lp, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 5) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_backward_kernel, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, stream, pl, n_chains,
                           (const unsigned*)origin, (const int*)endstate, end);
        HIPCHK(hipGetLastError());
    }
    if (stages < 6) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_backtrack_kernel, dim3((unsigned)((n_chunks + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS)),
                           dim3(DFF_VIT_THREADS), 0, stream, pl, n_chunks, (const unsigned*)psi, (const int*)end, chain_order, path);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

extern "C" int dff_hmm_viterbi(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                               const double* logtrans, const double* logemit, const double* loginit, int m, int K, int32_t* path,
                               int chain_order, double* chain_logprob, int32_t* status, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    HmmCall call("hmm_viterbi");
    const char* what = call.what;
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    const long long n_chains = call.n_chains, n_chunks = call.n_chunks;
    if (!logtrans || !logemit || !loginit || !status || (!path && n > 0))
        return fail(DFF_EINVAL, "%s: null log transition matrix / log emissions / log initial distribution / path / status", what);
    if (chain_order != 0 && chain_order != 1) return fail(DFF_EINVAL, "%s: chain_order must be 0 (frame order) or 1 (chain order)", what);
    const VitLayout lay(n, n_traj, n_chains, n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;
    HIPCHK(hipMemsetAsync(ws + lay.flags, 0, 4 * sizeof(int), stream));
    long long pblocks = (n + 1023) / 1024;
    pblocks = pblocks < 1 ? 1 : (pblocks > 1024 ? 1024 : pblocks);
    hipLaunchKernelGGL(dff_vit_prep_kernel, dim3((unsigned)pblocks), dim3(1024), 0, stream, labels, n, logtrans, logemit, loginit, m,
                       K, hmm_pad(m), (double*)(ws + lay.la), (double*)(ws + lay.lp), (double*)(ws + lay.lbt), (int*)(ws + lay.flags));
    HIPCHK(hipGetLastError());
    double* clp = chain_logprob ? chain_logprob : (double*)(ws + lay.clp);
    rc = hmm_with_pad(m, [&](auto mp) {
        return vit_launches<decltype(mp)::value>(stream, labels, pl, n_chains, n_chunks, K, lay, ws, path, chain_order, clp);
    });
    if (rc || g_vit_stages.load()) return rc;
    const long long most = n > n_chains ? n : n_chains;
    const long long blocks = (most + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS;
    hipLaunchKernelGGL(dff_vit_finish_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks < 1024 ? blocks : 1024))), dim3(DFF_VIT_THREADS),
                       0, stream, (const int*)(ws + lay.flags), n, path, n_chains, chain_logprob, status);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Bootstrap of the Jensen-Shannon metrics: per-unit histograms, resample-and-score (dff_jsboot.hip)
// ---------------------------------------------------------------------------------------------
// which resample tile dff_resampled_js takes: 0 = by (B, C), else 1, 2, 4 or 8 resamples per workgroup
static std::atomic<int> g_jsb_path{0};

// the shape both calls share: units, channels, row stride, bins per channel (every one within the stride)
static int jsb_check_shape(int U, int C, int ld, const int32_t* nbins, const char* what) {
    if (U < 1 || U > DFF_JSB_MAXUNITS) return fail(DFF_EINVAL, "%s: the number of resampling units must be 1..%d", what, DFF_JSB_MAXUNITS);
    if (C < 1 || C > DFF_JSB_MAXCHANNELS) return fail(DFF_EINVAL, "%s: the number of channels must be 1..%d", what, DFF_JSB_MAXCHANNELS);
    if (ld < 1 || ld > DFF_JSB_MAXLD) return fail(DFF_EINVAL, "%s: the row stride ld must be 1..%d", what, DFF_JSB_MAXLD);
    if ((long long)U * C * ld > DFF_JSB_MAXCELLS) return fail(DFF_EINVAL, "%s: U C ld must not exceed 2^32", what);
    if (!nbins) return fail(DFF_EINVAL, "%s: null nbins", what);
    for (int c = 0; c < C; ++c)
        if (nbins[c] < 1 || nbins[c] > ld)
            return fail(DFF_EINVAL, "%s: channel %d has %d bins, must be 1..ld = %d", what, c, (int)nbins[c], ld);
    return DFF_OK;
}

static int jsb_check_counts(int U, int C, const char* what) {
    if (U < 1 || U > DFF_JSB_MAXUNITS) return fail(DFF_EINVAL, "%s: the number of resampling units must be 1..%d", what, DFF_JSB_MAXUNITS);
    if (C < 1 || C > DFF_JSB_MAXCHANNELS) return fail(DFF_EINVAL, "%s: the number of channels must be 1..%d", what, DFF_JSB_MAXCHANNELS);
    return DFF_OK;
}

// nbins (C) as 64-bit words into dst, as kernel arguments
static int jsb_upload_nbins(hipStream_t stream, const int32_t* nbins, int C, long long* dst) {
    std::vector<long long> nb64(nbins, nbins + C);
    return msmb_upload(stream, nb64.data(), C, dst);
}

extern "C" long long dff_unit_hist_workspace_bytes(int U, int C) {
    if (jsb_check_counts(U, C, "unit_hist_workspace_bytes")) return -1;
    return ((long long)U + 1 + C) * (long long)sizeof(long long);             // unit starts | nbins
}

extern "C" int dff_unit_hist(int device, const int32_t* bins, long long n, int C, const long long* unit_lengths, int U,
                             const int32_t* nbins, int ld, uint32_t* hist, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* what = "unit_hist";
    if ((!bins && n > 0) || n < 0) return fail(DFF_EINVAL, "%s: null bins / negative count", what);
    if (n > (1LL << 31)) return fail(DFF_EINVAL, "%s: more than 2^31 frames", what);
    int rc = jsb_check_shape(U, C, ld, nbins, what);
    if (rc) return rc;
    if (!unit_lengths) return fail(DFF_EINVAL, "%s: null unit lengths", what);
    long long total = 0;
    for (int u = 0; u < U; ++u) {
        if (unit_lengths[u] < 0) return fail(DFF_EINVAL, "%s: unit %d has negative length", what, u);
        if (unit_lengths[u] > n - total) return fail(DFF_EINVAL, "%s: unit lengths sum to more than n = %lld", what, n);
        total += unit_lengths[u];
    }
    if (total != n) return fail(DFF_EINVAL, "%s: unit lengths sum to %lld, not n = %lld", what, total, n);
    if (!hist) return fail(DFF_EINVAL, "%s: null output", what);
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_unit_hist_workspace_bytes(U, C), what))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    HIPCHK(hipMemsetAsync(hist, 0, (size_t)U * C * ld * sizeof(uint32_t), stream));
    if (n == 0) return DFF_OK;
    std::vector<long long> tab((size_t)U + 1 + C);
    tab[0] = 0;
    int max_bins = 1;
    for (int u = 0; u < U; ++u) tab[u + 1] = tab[u] + unit_lengths[u];
    for (int c = 0; c < C; ++c) {
        tab[(size_t)U + 1 + c] = nbins[c];
        if (nbins[c] > max_bins) max_bins = nbins[c];
    }
    long long* tab_dev = (long long*)workspace;
    if ((rc = msmb_upload(stream, tab.data(), (long long)tab.size(), tab_dev))) return rc;
    const int tiles = (max_bins + DFF_JSB_TILE_BINS - 1) / DFF_JSB_TILE_BINS;
    const long long items = (long long)U * C * tiles;                          // <= 2^32 / 8192 + 2^36: a grid-stride loop
    hipLaunchKernelGGL(dff_unit_hist_kernel, dim3((unsigned)(items < (1 << 20) ? items : (1 << 20))), dim3(DFF_JSB_THREADS), 0, stream,
                       bins, C, tab_dev, tab_dev + U + 1, ld, tiles, items, hist);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// resamples per workgroup: the largest tile, of at most DFF_JSB_MAXTILE and no wider than B needs, that still gives the call DFF_JSB_WANT_WGS workgroups (a one-channel grid at a few
// hundred resamples would otherwise run on a tenth of the chip); every tile gives the same bits
static int jsb_tile(int B, int C) {
    const int forced = g_jsb_path.load();
    if (forced) return forced;
    int tb = DFF_JSB_MAXTILE;
    while (tb > 1 && tb / 2 >= B) tb >>= 1;                                    // no tile wider than the batch needs
    while (tb > 1 && (long long)C * ((B + tb - 1) / tb) < DFF_JSB_WANT_WGS) tb >>= 1;
    return tb;
}

static int jsb_check_resamples(int B, const char* what) {
    if (B < 1 || B > DFF_JSB_MAXB) return fail(DFF_EINVAL, "%s: the number of resamples must be 1..%d", what, DFF_JSB_MAXB);
    return DFF_OK;
}

extern "C" int dff_debug_resampled_js_path(int path) {
    if (path != 0 && path != 1 && path != 2 && path != 4 && path != 8)
        return fail(DFF_EINVAL, "debug_resampled_js_path: 0 (by shape) or 1, 2, 4, 8 resamples per workgroup");
    g_jsb_path.store(path);
    return DFF_OK;
}

extern "C" int dff_resampled_js_path_for(int B, int C) {
    if (jsb_check_resamples(B, "resampled_js_path_for")) return -1;
    if (jsb_check_counts(1, C, "resampled_js_path_for")) return -1;
    return jsb_tile(B, C);
}

extern "C" long long dff_resampled_js_workspace_bytes(int U, int C) {
    if (jsb_check_counts(U, C, "resampled_js_workspace_bytes")) return -1;
    return ((long long)C + (long long)U * C + C) * 8;                          // nbins | unit totals (U, C) | reference sums
}

extern "C" int dff_resampled_js(int device, const uint32_t* hist, int U, int C, int ld, const int32_t* nbins, const uint32_t* weights,
                                int B, const double* ref, double* js, uint64_t* total, void* workspace, size_t workspace_bytes,
                                void* stream_) {
    const char* what = "resampled_js";
    int rc = jsb_check_shape(U, C, ld, nbins, what);
    if (rc) return rc;
    if ((rc = jsb_check_resamples(B, what))) return rc;
    if (!hist || !weights || !ref || !js) return fail(DFF_EINVAL, "%s: null histograms / weights / reference / output", what);
    if ((rc = check_workspace8(workspace, workspace_bytes, dff_resampled_js_workspace_bytes(U, C), what))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    long long* nb_dev = (long long*)workspace;
    unsigned long long* utot = (unsigned long long*)(nb_dev + C);
    double* refsum = (double*)(utot + (size_t)U * C);
    if ((rc = jsb_upload_nbins(stream, nbins, C, nb_dev))) return rc;
    const long long rows = (long long)U * C;
    const long long tblocks = (rows + 3) / 4;
    hipLaunchKernelGGL(dff_jsb_unit_totals_kernel, dim3((unsigned)(tblocks < (1 << 16) ? tblocks : (1 << 16))), dim3(DFF_JSB_THREADS), 0,
                       stream, hist, rows, C, ld, (const long long*)nb_dev, utot);
    hipLaunchKernelGGL(dff_jsb_ref_kernel, dim3((unsigned)C), dim3(DFF_JSB_THREADS), 0, stream, ref, ld, (const long long*)nb_dev, refsum);
    const int tb = jsb_tile(B, C);
    const dim3 grid((unsigned)(C >= 8 ? (C + 7) / 8 * 8 : C) * (unsigned)((B + tb - 1) / tb));
    auto launch = [&](auto tile) {
        hipLaunchKernelGGL(dff_resampled_js_kernel<decltype(tile)::value>, grid, dim3(DFF_JSB_THREADS), 0, stream, hist, U, C, ld,
                           (const long long*)nb_dev, weights, B, ref, (const unsigned long long*)utot, (const double*)refsum, js,
                           (unsigned long long*)total);
    };
    switch (tb) {
        case 8: launch(std::integral_constant<int, 8>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        default: launch(std::integral_constant<int, 1>{}); break;
    }
    HIPCHK(hipGetLastError());
    return DFF_OK;
}
