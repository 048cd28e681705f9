// dff_analysis_host.h -- what the sample-analysis units (dff_an_structures.hip, dff_an_trajectories.hip, dff_an_markov.hip,
// dff_an_hmm.hip) share on the host: argument checks, the launch of a tile kernel, the launches over trajectories back to
// back, the prologue of both k-means steps.  Host code only: no kernel file includes it.  Everything here is static or a
// template; the two functions that launch another unit's kernel (upload_words, tc_launches) are declared, not defined.
#pragma once
#include "dff_host_common.h"
#include <atomic>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dff_frames.h"   // DFF_STRUCT_TILE, struct_ld
#include "dff_traj.h"     // TransRuns, DFF_TC_*, DFF_STATES_MAXK
#include "dff_upload.h"   // upload_words

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
// Tile kernels over (n, N, 3) frames (dff_frames.h): the checks and the launch
// ---------------------------------------------------------------------------------------------
static int struct_check(const float* x, long long n, int N, const void* out, const char* what) {
    if ((!x && n > 0) || n < 0) return fail(DFF_EINVAL, "%s: null input / negative count", what);
    if (int rc = check_beads(N, what)) return rc;
    if (!out && n > 0) return fail(DFF_EINVAL, "%s: null output", what);
    return check_frames(n, what);
}

static unsigned struct_tile_bytes(int N) { return (unsigned)(DFF_STRUCT_TILE * struct_ld(N) * sizeof(float)); }

// Launch of a tile kernel, kernel(x, n, N, args..., magic, vec4) (struct_tiles, dff_frames.h).  One wave per workgroup:
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

// ---------------------------------------------------------------------------------------------
// Trajectories, state counts, k-means, lag times
// ---------------------------------------------------------------------------------------------
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

// K states, called `noun` ("centres", "states") in the caller's message
static int states_check_count(int K, const char* what, const char* noun) {
    if (K < 1 || K > DFF_STATES_MAXK) return fail(DFF_EINVAL, "%s: the number of %s must be 1..%d", what, noun, DFF_STATES_MAXK);
    return DFF_OK;
}

static int micro_check_count(int K, const char* what, const char* noun) {
    if (K < 1 || K > DFF_MSM_MAXK) return fail(DFF_EINVAL, "%s: the number of %s must be 1..%d", what, noun, DFF_MSM_MAXK);
    return DFF_OK;
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

static int tc_check_lags(const int32_t* lags, int n_lags, const char* what) {
    if (!lags || n_lags < 1 || n_lags > DFF_TC_MAXLAGS)
        return fail(DFF_EINVAL, "%s: the number of lag times must be 1..%d", what, DFF_TC_MAXLAGS);
    for (int l = 0; l < n_lags; ++l)
        if (lags[l] < 1) return fail(DFF_EINVAL, "%s: lag time %d is %d, must be >= 1", what, l, (int)lags[l]);
    return DFF_OK;
}

// the launches of dff_transition_counts_kernel over checked arguments, n > 0, K <= DFF_STATES_MAXK, counts already zeroed (defined in dff_an_structures.hip, next to its kernel)
__attribute__((visibility("hidden"))) int tc_launches(hipStream_t stream, const int32_t* labels, long long n, const long long* lengths, int n_traj,
                                                      const int32_t* lags, int n_lags, int K, uint64_t* counts);
