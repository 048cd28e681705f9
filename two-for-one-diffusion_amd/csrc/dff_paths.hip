// dff_paths.hip -- transition paths from an order parameter on the GPU: for every frame the last core visited (what
// dff_core_states gives) AND the next core visited, with the frames of both visits, the class of the frame (in a core, on a
// path A->B / B->A, on a loop out of a core and back, undetermined) and the table of the transition paths.
//
// The reference plots per-trajectory RMSD and contact dynamics and stops there (evaluate/evaluators.py); transition-path
// times (Chung & Eaton), p(TP | q) (Best & Hummer) and the empirical committor all need, per frame, the core reached NEXT,
// which a forward scan cannot know: the same scan run backwards.
//
// The scan of dff_frame_scan.h in both directions, on the keys of dff_core_states (core_keys, dff_kinetics.hip).  What a
// stretch of frames gives to the forward scan (PathFwd):
//   last   the maximum of the forward keys.  The inclusive prefix is the previous core visit: the label of dff_core_states,
//          from the same function.
//   cnt    the number of path records in the stretch: a record is a pair of CONSECUTIVE decisive frames in two different
//          cores, written by the later of the two (the entry).  That is no sum of per-frame values -- whether the
//          first core visit of a block ends a path depends on the blocks before it -- so the stretch also carries
//   first  the minimum of the forward keys (DFF_CORE_NONE for none), and the join adds one where the left stretch's `last` and
//          the right stretch's `first` lie in different cores.  A trajectory's first frame gives `first` with code 0 even inside
//          a core: nothing before it can end a path there.  This join is associative and NOT commutative.
// and to the reverse scan (PathBwd): the minimum of the backward keys.  The inclusive SUFFIX is the next core visit.
// The entry frame of a path reads the exit from the exclusive prefix (`last` of everything before it) and the record's index
// from its `cnt`: the table is compacted by the scan itself, in ascending entry, with no atomic.
#pragma once
#include "dff_kinetics.hip"   // KinCore, core_keys, the scan

struct PathFwd {
    long long cnt, first, last;
    static __device__ __forceinline__ PathFwd none() { return PathFwd{0, DFF_CORE_NONE, -1}; }
    // does a path end between two consecutive decisive frames: `last` of the stretch before, `first` of the stretch after
    static __device__ __forceinline__ int between(long long last, long long first) {
        const int a = (int)(last & 3), b = (int)(first & 3);       // -1 & 3 = 3, DFF_CORE_NONE & 3 = 3: no core
        return (a == 1 && b == 2) || (a == 2 && b == 1);
    }
    static __device__ __forceinline__ PathFwd join(PathFwd a, PathFwd b) {
        return PathFwd{a.cnt + b.cnt + between(a.last, b.first), a.first < b.first ? a.first : b.first,
                       a.last > b.last ? a.last : b.last};
    }
};
struct PathBwd {
    long long key;
    static __device__ __forceinline__ PathBwd none() { return PathBwd{DFF_CORE_NONE}; }
    static __device__ __forceinline__ PathBwd join(PathBwd a, PathBwd b) { return a.key < b.key ? a : b; }
};

struct PathSrc : KinCore {
    using Fwd = PathFwd;
    using Rev = PathBwd;
    struct Frames : KinCore::Frames {
        __device__ __forceinline__ PathFwd fwd(int k) const {
            const long long key = keys(k).fwd;
            return PathFwd{0, is(first, k) ? (t0 + k) << 2 : key >= 0 ? key : DFF_CORE_NONE, key};
        }
        __device__ __forceinline__ PathBwd rev(int k) const { return PathBwd{keys(k).bwd}; }
    };
};

struct PathOut {
    signed char *prev, *next;
    long long *t_prev, *t_next;
    signed char* cls;
    long long max_paths;                                        // 0 when there is no table
    long long *path_exit, *path_entry;
    signed char* path_dir;
};

// phase 3: every frame writes its own outputs, the entry frame of a path the path's record
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_path_apply_kernel(PathSrc src, TransRuns runs,
                                                                          const PathFwd* __restrict__ before,
                                                                          const PathBwd* __restrict__ after, PathOut out) {
    PathSrc::Frames fr;
    fr.load(src, runs);
    PathBwd w;                                                  // everything after frame t0 + k
    PathFwd run = scan_before(fr, before, after, w);            // everything before it
    long long nxt[DFF_KIN_ITERS];                               // the inclusive suffix of every frame
#pragma unroll
    for (int k = DFF_KIN_ITERS - 1; k >= 0; --k) {
        if (fr.is(fr.live, k)) w = PathBwd::join(fr.rev(k), w);
        nxt[k] = w.key;
    }
#pragma unroll
    for (int k = 0; k < DFF_KIN_ITERS; ++k) {
        if (!fr.is(fr.live, k)) continue;
        const long long t = fr.t0 + k;
        const PathFwd v = PathFwd::join(run, fr.fwd(k));
        // v.last >= 0 and nxt < DFF_CORE_NONE: the trajectory's first and last frames are decisive
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
