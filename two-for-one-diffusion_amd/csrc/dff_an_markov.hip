// dff_an_markov.hip -- the Markov-state-model entry points of include/dff.h and the kernels they launch: dff_micro_* (k-means,
// transition counts, resampled counts), dff_msm_* with their batched counterparts and dff_debug_msm_*, dff_msm_dirichlet_*,
// dff_sym_eig_*, dff_msm_propagate*.  Also upload_words (dff_upload.h), whose kernel is compiled here.  One of four analysis
// units (dff_analysis_host.h names them).
#include "dff_analysis_host.h"

#include "dff_msm.hip"
#include "dff_msm_batch.hip"
#include "dff_msm_passage.hip"
#include "dff_sym_eig.hip"
#include "dff_msm_propagate.hip"

// ---------------------------------------------------------------------------------------------
// Markov state models: microstate k-means, transition counts, reversible estimator (dff_msm.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_micro_chunk(void) { return DFF_MICRO_CHUNK; }

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
int upload_words(hipStream_t stream, const long long* src, long long cnt, long long* dst) {
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
    if ((rc = upload_words(stream, ts, (long long)starts.size(), (long long*)workspace))) return rc;
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
    int upload(hipStream_t stream, long long* dst) const { return upload_words(stream, desc.data(), (long long)desc.size(), dst); }
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
