// dff_frame_scan.h -- the scan over the frames of trajectories that dff_core_states, dff_label_runs and dff_path_states share.
//
// Three launches, block reduce -> carry scan -> apply, the carries in the workspace: no workgroup waits on another, no atomics,
// integers only, so the results are exact and the same from call to call.
//   layout   a workgroup owns DFF_KIN_BLOCK frames, a thread DFF_KIN_ITERS CONSECUTIVE ones: a thread joins its own frames in
//            a loop, and every kernel runs one workgroup scan.
//   element  a struct of long long fields with none(), its neutral element, and join(before, after).  A join need not be
//            commutative: frames, threads, waves and blocks are joined strictly in frame order.  A forward element has a
//            field `cnt`, the records of its stretch (0 throughout for a call without records): the carry scan reads it.
//   reverse  next to the forward scan (a prefix over the frames) a call may scan backwards (a suffix) on an element type of its
//            own: the same code with lanes, waves and blocks taken from the top, step by step next to the forward scan and
//            behind the same barrier.  ScanNone in its place: the call scans forwards only.
//   source   Src, the kernel argument of a call: its element types Fwd and Rev and a thread's view of its frames, Frames
//            (TrajFrames and what the frames hold; load(src, runs), fwd(k), rev(k): what frame t0 + k gives to either scan).
//   reduce   dff_scan_reduce_kernel<Src>: fwd[b], rev[b] = the join of the frames of block b.
//   carry    dff_scan_carry_kernel, one workgroup: fwd[b] -> the join of the blocks before b, rev[b] -> of those after b.
//   apply    the call's own kernel (Src, TransRuns, fwd, rev if the call scans backwards, ...): scan_before gives a thread the
//            join of everything before (after) its frames.
// Trajectories come as the run tables of dff_transition_counts (TransRuns): up to DFF_TC_RUNS trajectories per launch, or any
// number of equal-length ones.  A launch's frames are whole trajectories, so its scans start from nothing; only a count of
// records (the `cnt` of the forward element) is carried from one launch of a call to the next, by the carry scan.
#pragma once
#include <type_traits>

#include "dff_traj.h"   // TransRuns, last_le

#define DFF_KIN_THREADS 256
#define DFF_KIN_ITERS 8
#define DFF_KIN_BLOCK (DFF_KIN_THREADS * DFF_KIN_ITERS)   // frames per workgroup: one carry each
#define DFF_KIN_WAVES (DFF_KIN_THREADS / 64)

enum ScanDir { SCAN_FWD, SCAN_REV };
// the element of a scan that does not run: nothing to join, nothing in memory
struct ScanNone {
    static __device__ __forceinline__ ScanNone none() { return {}; }
    static __device__ __forceinline__ ScanNone join(ScanNone, ScanNone) { return {}; }
};
template <class T>
constexpr bool scan_runs = !std::is_same<T, ScanNone>::value;

// ---- the workgroup scan, in thread order (SCAN_REV: from the last thread down)
// the place of lane / wave i of n in scan order
template <ScanDir D>
__device__ __forceinline__ int scan_place(int i, int n) { return D == SCAN_FWD ? i : n - 1 - i; }
// the join of `acc`, what the scan has met so far, with what it meets next: the arguments of join stay in frame order
template <ScanDir D, class T>
__device__ __forceinline__ T scan_join(T acc, T next) { return D == SCAN_FWD ? T::join(acc, next) : T::join(next, acc); }
// v of the lane d places earlier in scan order
template <ScanDir D, class T>
__device__ __forceinline__ T scan_shfl(T v, int d) {
    if constexpr (scan_runs<T>) {
        static_assert(sizeof(T) % sizeof(long long) == 0, "an element is a struct of long long fields");
        long long w[sizeof(T) / sizeof(long long)];
        __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
        for (unsigned k = 0; k < sizeof(T) / sizeof(long long); ++k) w[k] = D == SCAN_FWD ? __shfl_up(w[k], d) : __shfl_down(w[k], d);
        __builtin_memcpy(&v, w, sizeof(T));
    }
    return v;
}
// one step of the scan inside the wave
template <ScanDir D, class T>
__device__ __forceinline__ T scan_step(T v, int d) {
    const T o = scan_shfl<D>(v, d);
    return scan_place<D>(threadIdx.x & 63, 64) >= d ? scan_join<D>(o, v) : v;
}
// after the steps: the wave's total into its slot -> the join of the lanes before this one
template <ScanDir D, class T>
__device__ __forceinline__ T scan_slot(T v, T* wtot) {
    const int lane = scan_place<D>(threadIdx.x & 63, 64);
    if (lane == 63) wtot[scan_place<D>(threadIdx.x >> 6, DFF_KIN_WAVES)] = v;
    v = scan_shfl<D>(v, 1);
    return lane == 0 ? T::none() : v;
}
// a barrier later: -> the join of the threads before this one, `total` the workgroup's
template <ScanDir D, class T>
__device__ __forceinline__ T scan_waves(const T* wtot, T excl, T& total) {
    const int wave = scan_place<D>(threadIdx.x >> 6, DFF_KIN_WAVES);
    T pre = total = T::none();
#pragma unroll
    for (int k = 0; k < DFF_KIN_WAVES; ++k) {
        if (k < wave) pre = scan_join<D>(pre, wtot[k]);
        total = scan_join<D>(total, wtot[k]);
    }
    return scan_join<D>(pre, excl);
}
// In: this thread's values; out: f the join of the threads before it, r of those after it, ftot / rtot the workgroup's.  A
// kernel that scans twice puts a barrier between the two: the slots are in use until every thread is through.
template <class F, class R>
__device__ __forceinline__ void block_scan(F& f, F& ftot, R& r, R& rtot) {
    __shared__ F wf[DFF_KIN_WAVES];
    __shared__ R wr[DFF_KIN_WAVES];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                          // two independent chains of shuffles: they overlap
        f = scan_step<SCAN_FWD>(f, d);
        r = scan_step<SCAN_REV>(r, d);
    }
    f = scan_slot<SCAN_FWD>(f, wf);
    r = scan_slot<SCAN_REV>(r, wr);
    __syncthreads();
    f = scan_waves<SCAN_FWD>(wf, f, ftot);
    r = scan_waves<SCAN_REV>(wr, r, rtot);
}

// ---- a thread's frames
// The frames of one thread, DFF_KIN_ITERS consecutive ones from t0: which are live (inside the launch), which are their
// trajectory's first / last frame (bit k of the masks: frame t0 + k).  One lookup of the trajectory of t0, then a walk.
struct TrajFrames {
    long long t0;
    unsigned live, first, lastf;
    __device__ __forceinline__ bool is(unsigned mask, int k) const { return (mask >> k) & 1; }
    __device__ __forceinline__ ScanNone rev(int) const { return {}; }
    __device__ __forceinline__ void load(const TransRuns& runs) {
        t0 = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK + (long long)threadIdx.x * DFF_KIN_ITERS;
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
            if (t < runs.end) {
                if (t == e) {                                   // t < runs.end: there is a next trajectory
                    b = e;
                    e = runs.period > 0 ? b + runs.period : runs.start[++i + 1];
                }
                live |= 1u << k;
                if (t == b) first |= 1u << k;
                if (t + 1 == e) lastf |= 1u << k;
            }
        }
    }
};

// the workgroup scan over the joins of every thread's live frames, in frame order
template <class Frames, class F, class R>
__device__ __forceinline__ void scan_frames(const Frames& fr, F& f, F& ftot, R& r, R& rtot) {
    f = F::none();
    r = R::none();
#pragma unroll
    for (int k = 0; k < DFF_KIN_ITERS; ++k)
        if (fr.is(fr.live, k)) {
            f = F::join(f, fr.fwd(k));
            r = R::join(r, fr.rev(k));
        }
    block_scan(f, ftot, r, rtot);
}

// ---- the phases
// phase 1
template <class Src>
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_scan_reduce_kernel(Src src, TransRuns runs, typename Src::Fwd* __restrict__ fwd,
                                                                           typename Src::Rev* __restrict__ rev) {
    typename Src::Frames fr;
    fr.load(src, runs);
    typename Src::Fwd f, ftot;
    typename Src::Rev r, rtot;
    scan_frames(fr, f, ftot, r, rtot);
    if (threadIdx.x == 0) {
        fwd[blockIdx.x] = ftot;
        if constexpr (scan_runs<typename Src::Rev>) rev[blockIdx.x] = rtot;
    }
}

// Phase 2, one workgroup, DFF_KIN_THREADS blocks at a time, in place: the prefix walks the blocks upwards and the suffix
// downwards in the same loop; every entry is read and written by one thread only.  count (may be NULL): the running number of
// records over the launches of a call -- read unless this is the call's first launch, added to every carry, written back
// with this launch's records added.
template <class F, class R>
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_scan_carry_kernel(F* __restrict__ fwd, R* __restrict__ rev, long long nb,
                                                                          long long* __restrict__ count, int first) {
    F up = F::none(), a, atot;                                  // up: the blocks below this chunk
    R down = R::none(), b = R::none(), btot;                    // down: the blocks above this chunk
    up.cnt = (count && !first) ? *count : 0;
    const long long chunks = (nb + DFF_KIN_THREADS - 1) / DFF_KIN_THREADS;
    for (long long c = 0; c < chunks; ++c) {
        const long long i = c * DFF_KIN_THREADS + threadIdx.x, j = (chunks - 1 - c) * DFF_KIN_THREADS + threadIdx.x;
        a = i < nb ? fwd[i] : F::none();
        if constexpr (scan_runs<R>) b = j < nb ? rev[j] : R::none();
        __syncthreads();                                        // the slots are free of the chunk before
        block_scan(a, atot, b, btot);
        if (i < nb) fwd[i] = F::join(up, a);
        if constexpr (scan_runs<R>)
            if (j < nb) rev[j] = R::join(b, down);
        up = F::join(up, atot);
        down = R::join(btot, down);
    }
    if (count && threadIdx.x == 0) *count = up.cnt;             // every thread read it before the loop's barriers
}

// phase 3, in the call's own kernel: -> the join of everything before this thread's frames -- the blocks before its own (fwd,
// what phase 2 left) and the threads before it -- and r = of everything after them
template <class Frames, class F, class R>
__device__ __forceinline__ F scan_before(const Frames& fr, const F* __restrict__ fwd, const R* __restrict__ rev, R& r) {
    const F below = fwd[blockIdx.x];
    F f, ftot;
    R above = R::none(), rtot;
    if constexpr (scan_runs<R>) above = rev[blockIdx.x];
    scan_frames(fr, f, ftot, r, rtot);
    r = R::join(r, above);
    return F::join(below, f);
}
// the same for a call that scans forwards only
template <class Frames, class F>
__device__ __forceinline__ F scan_before(const Frames& fr, const F* __restrict__ fwd) {
    ScanNone none;
    return scan_before(fr, fwd, (const ScanNone*)nullptr, none);
}
