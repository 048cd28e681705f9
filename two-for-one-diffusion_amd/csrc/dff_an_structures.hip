// dff_an_structures.hip -- the sample-analysis entry points of include/dff.h that work frame by frame on (n, N, 3) structures
// already resident in HBM, and the kernels they launch: dff_pwd_*, dff_struct_* (dff_struct_native_q is with the
// trajectories), dff_tica_*, dff_kmeans_*, dff_transition_counts, dff_rmsd_*, dff_superpose, dff_gromos_*.  One of four
// analysis units (dff_analysis_host.h names them); none of them touches a dff_model, and the sampler kernels include none
// of their files.
#include "dff_analysis_host.h"

#include "dff_pwd.hip"
#include "dff_struct.hip"
#include "dff_tica.hip"
#include "dff_states.hip"
#include "dff_ensemble.hip"
#include "dff_superpose.hip"
#include "dff_cluster.hip"

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

// the launches of dff_transition_counts_kernel over checked arguments, n > 0, K <= DFF_STATES_MAXK, counts already zeroed
int tc_launches(hipStream_t stream, const int32_t* labels, long long n, const long long* lengths, int n_traj,
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
