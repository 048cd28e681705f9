// dff_paths.hip -- transition paths from an order parameter on the GPU: for every frame the last core visited (what
// dff_core_states gives) AND the next core visited, with the frames of both visits, the class of the frame (in a core, on a
// path A->B / B->A, on a loop out of a core and back, undetermined) and the table of the transition paths.
//
// The reference plots per-trajectory RMSD and contact dynamics and stops there (evaluate/evaluators.py); transition-path
// times (Chung & Eaton), p(TP | q) (Best & Hummer) and the empirical committor all need, per frame, the core reached NEXT,
// which a forward scan cannot know: the same scan run backwards.
//
// One bidirectional scan, in the three launches of dff_kinetics.hip (block reduce -> one-workgroup carry scan -> apply,
// DFF_KIN_BLOCK frames per workgroup, the carries in the workspace): no workgroup waits on another, no atomics, integers
// only, so the results are exact and the same from call to call.  What a stretch of frames gives to the scan (PathScan):
//   last   the maximum of the forward keys: frame << 2 | code of the decisive frames of dff_core_states (in a core,
//          non-finite, or the trajectory's first frame; code 0 / 1 / 2 = history unknown / core A / core B), -1 for none.
//          The inclusive prefix is the previous core visit, bit for bit the label of dff_core_states.
//   bwd    the minimum of the backward keys: the same keys, with the trajectory's LAST frame decisive in place of its first,
//          LLONG_MAX for none.  The inclusive SUFFIX is the next core visit.
//   cnt    the number of path records in the stretch: a record is a pair of CONSECUTIVE decisive frames in two different
//          cores, written by the later of the two (the entry).  That is no sum of per-frame values -- whether the
//          first core visit of a block ends a path depends on the blocks before it -- so the stretch also carries
//   first  the minimum of the forward keys (LLONG_MAX for none), and the join adds one where the left stretch's `last` and the
//          right stretch's `first` lie in different cores.  A trajectory's first frame gives `first` with code 0 even inside a
//          core: nothing before it can end a path there.  The join is associative and NOT commutative: a thread owns
//          DFF_KIN_ITERS consecutive frames, threads and blocks are joined in frame order.
// The entry frame of a path reads the exit from the exclusive prefix (`last` of everything before it) and the record's index
// from its `cnt`: the table is compacted by the scan itself, in ascending entry, with no atomic.
// Trajectories come as the run tables of dff_transition_counts (TransRuns): a launch's frames are whole trajectories, so both
// scans start from nothing; only the path count is carried from one launch to the next, by the carry scan's one workgroup.
#pragma once
#include "dff_kinetics.hip"   // DFF_KIN_*, KinCore, TransRuns, last_le

#define DFF_PATH_NONE 0x7fffffffffffffffLL

struct PathScan {
    long long cnt, first, last, bwd;
};
__device__ __forceinline__ PathScan path_none() { return PathScan{0, DFF_PATH_NONE, -1, DFF_PATH_NONE}; }
// does a path end between two consecutive decisive frames: `last` of the stretch before, `first` of the stretch after
__device__ __forceinline__ int path_between(long long last, long long first) {
    const int a = (int)(last & 3), b = (int)(first & 3);           // -1 & 3 = 3, DFF_PATH_NONE & 3 = 3: no core
    return (a == 1 && b == 2) || (a == 2 && b == 1);
}
// a: the frames before those of b.  bwd is not joined here: it runs the other way (path_block_scan)
__device__ __forceinline__ PathScan path_join(PathScan a, PathScan b) {
    return PathScan{a.cnt + b.cnt + path_between(a.last, b.first), a.first < b.first ? a.first : b.first,
                    a.last > b.last ? a.last : b.last, DFF_PATH_NONE};
}
__device__ __forceinline__ long long path_min(long long a, long long b) { return a < b ? a : b; }

// Both scans over the workgroup in thread order.  v: this thread's stretch.  Returns the join of the threads BEFORE this one
// (cnt, first, last) with, in bwd, the minimum over the threads AFTER it; `total` is the whole workgroup's.  wtot: one slot
// per wave in LDS.
__device__ __forceinline__ PathScan path_block_scan(PathScan v, PathScan* wtot, PathScan& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long w = v.bwd;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const PathScan o = {__shfl_up(v.cnt, d), __shfl_up(v.first, d), __shfl_up(v.last, d), 0};
        const long long ow = __shfl_down(w, d);
        if (lane >= d) v = path_join(o, v);
        if (lane + d < 64) w = path_min(w, ow);
    }
    // v: the inclusive prefix inside the wave, w: the inclusive suffix
    PathScan before = {__shfl_up(v.cnt, 1), __shfl_up(v.first, 1), __shfl_up(v.last, 1), 0};
    long long after = __shfl_down(w, 1);
    if (lane == 0) before = path_none();
    if (lane == 63) after = DFF_PATH_NONE;
    __syncthreads();                                            // the slots are free of their previous use
    if (lane == 63) { wtot[wave].cnt = v.cnt; wtot[wave].first = v.first; wtot[wave].last = v.last; }
    if (lane == 0) wtot[wave].bwd = w;
    __syncthreads();
    PathScan pre = path_none();
    long long post = DFF_PATH_NONE, all = DFF_PATH_NONE;
    total = path_none();
#pragma unroll
    for (int k = 0; k < DFF_KIN_THREADS / 64; ++k) {
        const PathScan s = wtot[k];
        if (k < wave) pre = path_join(pre, s);
        if (k > wave) post = path_min(post, s.bwd);
        total = path_join(total, s);
        all = path_min(all, s.bwd);
    }
    total.bwd = all;
    PathScan excl = path_join(pre, before);
    excl.bwd = path_min(post, after);
    return excl;
}

// The frames of one thread, DFF_KIN_ITERS consecutive ones from t0: which are live, their codes, which are their trajectory's
// first / last frame (bit k of the masks: frame t0 + k).
struct PathFrames {
    int code[DFF_KIN_ITERS];
    unsigned live, first, lastf;
    __device__ __forceinline__ void load(const KinCore& src, const TransRuns& runs, long long t0) {
        live = first = lastf = 0;
        long long b = 0, e = 0;                                 // the trajectory of the current frame: frames b .. e - 1
        int i = 0;
        if (t0 < runs.end) {
            if (runs.period > 0) {
                b = t0 - (t0 - runs.begin) % runs.period;
                e = b + runs.period;
            } else {
                i = last_le(runs.start, runs.n, t0);
                b = runs.start[i];
                e = runs.start[i + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < DFF_KIN_ITERS; ++k) {
            const long long t = t0 + k;
            code[k] = 3;
            if (t < runs.end) {
                if (t == e) {                                   // t < runs.end: there is a next trajectory
                    b = e;
                    e = runs.period > 0 ? b + runs.period : runs.start[++i + 1];
                }
                live |= 1u << k;
                if (t == b) first |= 1u << k;
                if (t + 1 == e) lastf |= 1u << k;
                code[k] = src.code(t);
            }
        }
    }
    // what frame k (live) gives to the scan
    __device__ __forceinline__ PathScan item(long long t0, int k) const {
        const long long key = (t0 + k) << 2;
        const int c = code[k];
        const bool f = (first >> k) & 1, l = (lastf >> k) & 1;
        if (c != 3) return PathScan{0, f ? key : key | c, key | c, key | c};
        return PathScan{0, f ? key : DFF_PATH_NONE, f ? key : -1, l ? key : DFF_PATH_NONE};
    }
    // the join of this thread's frames
    __device__ __forceinline__ PathScan stretch(long long t0) const {
        PathScan v = path_none();
        long long w = DFF_PATH_NONE;
#pragma unroll
        for (int k = 0; k < DFF_KIN_ITERS; ++k)
            if ((live >> k) & 1) {
                const PathScan it = item(t0, k);
                v = path_join(v, it);
                w = path_min(w, it.bwd);
            }
        v.bwd = w;
        return v;
    }
};

// phase 1: agg[b] = the join of the frames of block b of the launch
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_path_reduce_kernel(KinCore src, TransRuns runs, PathScan* __restrict__ agg) {
    __shared__ PathScan wtot[DFF_KIN_THREADS / 64];
    const long long t0 = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK + (long long)threadIdx.x * DFF_KIN_ITERS;
    PathFrames fr;
    fr.load(src, runs, t0);
    PathScan total;
    path_block_scan(fr.stretch(t0), wtot, total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// phase 2, one workgroup: agg[b] -> (cnt, first, last) of the blocks before b and bwd of the blocks after b, in place.  The
// prefix walks the blocks upwards and the suffix downwards in the same loop; every entry is read and written by one thread
// only.  count (may be NULL): the running number of paths over the launches of a call, as in dff_kin_carry_kernel.
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_path_carry_kernel(PathScan* __restrict__ agg, long long nb,
                                                                          long long* __restrict__ count, int first) {
    __shared__ PathScan wtot[DFF_KIN_THREADS / 64];
    PathScan run = path_none();
    run.cnt = (count && !first) ? *count : 0;
    const long long chunks = (nb + DFF_KIN_THREADS - 1) / DFF_KIN_THREADS;
    for (long long c = 0; c < chunks; ++c) {
        const long long i = c * DFF_KIN_THREADS + threadIdx.x;                  // upwards
        const long long j = (chunks - 1 - c) * DFF_KIN_THREADS + threadIdx.x;   // downwards
        PathScan v = i < nb ? agg[i] : path_none();
        v.bwd = j < nb ? agg[j].bwd : DFF_PATH_NONE;
        PathScan total;
        const PathScan excl = path_block_scan(v, wtot, total);
        if (i < nb) {
            const PathScan p = path_join(run, excl);
            agg[i].cnt = p.cnt; agg[i].first = p.first; agg[i].last = p.last;
        }
        if (j < nb) agg[j].bwd = path_min(run.bwd, excl.bwd);
        const long long w = path_min(run.bwd, total.bwd);
        run = path_join(run, total);
        run.bwd = w;
    }
    if (count && threadIdx.x == 0) *count = run.cnt;            // every thread read it before the loop's barriers
}

struct PathOut {
    signed char *prev, *next;
    long long *t_prev, *t_next;
    signed char* cls;
    long long max_paths;                                        // 0 when there is no table
    long long *path_exit, *path_entry;
    signed char* path_dir;
};

// phase 3: every frame writes its own outputs, the entry frame of a path the path's record
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_path_apply_kernel(KinCore src, TransRuns runs,
                                                                          const PathScan* __restrict__ carry, PathOut out) {
    __shared__ PathScan wtot[DFF_KIN_THREADS / 64];
    const long long t0 = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK + (long long)threadIdx.x * DFF_KIN_ITERS;
    PathFrames fr;
    fr.load(src, runs, t0);
    PathScan total;
    const PathScan excl = path_block_scan(fr.stretch(t0), wtot, total);
    const PathScan c = carry[blockIdx.x];
    long long nxt[DFF_KIN_ITERS];                               // the inclusive suffix of every frame
    long long w = path_min(c.bwd, excl.bwd);
#pragma unroll
    for (int k = DFF_KIN_ITERS - 1; k >= 0; --k) {
        if ((fr.live >> k) & 1) w = path_min(w, fr.item(t0, k).bwd);
        nxt[k] = w;
    }
    PathScan run = path_join(c, excl);                          // everything before frame t0 + k
#pragma unroll
    for (int k = 0; k < DFF_KIN_ITERS; ++k) {
        if (!((fr.live >> k) & 1)) continue;
        const long long t = t0 + k;
        const PathScan it = fr.item(t0, k);
        const PathScan v = path_join(run, it);
        // v.last >= 0 and nxt < DFF_PATH_NONE: the trajectory's first and last frames are decisive
        const int p = (int)(v.last & 3) - 1, q = (int)(nxt[k] & 3) - 1, code = fr.code[k];
        if (out.prev) out.prev[t] = (signed char)p;
        if (out.next) out.next[t] = (signed char)q;
        if (out.t_prev) out.t_prev[t] = p >= 0 ? v.last >> 2 : -1;
        if (out.t_next) out.t_next[t] = q >= 0 ? nxt[k] >> 2 : -1;
        if (out.cls)
            out.cls[t] = (signed char)(code == 1 ? 0 : code == 2 ? 1 : (code == 3 && p >= 0 && q >= 0) ? (p == q ? 4 + p : 2 + p) : -1);
        if (v.cnt != run.cnt && run.cnt < out.max_paths) {      // t ends a path: run.cnt paths end before it
            out.path_exit[run.cnt] = run.last >> 2;
            out.path_entry[run.cnt] = t;
            out.path_dir[run.cnt] = (signed char)(code - 1);
        }
        run = v;
    }
}
