// dff_an_trajectories.hip -- the sample-analysis entry points of include/dff.h that follow an observable along trajectories
// back to back, and the kernels they launch: dff_struct_native_q, dff_core_states, dff_label_runs, dff_path_states,
// dff_autocorr, dff_unit_hist and dff_resampled_js.  One of four analysis units (dff_analysis_host.h names them).
#include "dff_analysis_host.h"

#include "dff_kinetics.hip"
#include "dff_paths.hip"
#include "dff_autocorr.hip"
#include "dff_jsboot.hip"

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
    return upload_words(stream, nb64.data(), C, dst);
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
    if ((rc = upload_words(stream, tab.data(), (long long)tab.size(), tab_dev))) return rc;
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
