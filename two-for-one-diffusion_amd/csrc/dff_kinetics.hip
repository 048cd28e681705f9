// dff_kinetics.hip -- folding kinetics from an order parameter on the GPU: the fraction of native contacts per frame, the
// dual-cutoff (core-set) state of every frame along its trajectory, and the runs of equal labels inside trajectories.
//
// The reference looks at per-trajectory RMSD and contact dynamics (evaluate/evaluators.py: RmsdEvaluator.eval(save_dynamics=True),
// _plot_rmsd_dynamics, _eval_bce_dynamics) and stops at plots; these kernels turn the same series into states, dwell runs and
// rates (the reductions over runs stay on the host: evaluate.py, dwell_summary).
//
// dff_struct_native_q_kernel   the layout of dff_struct.hip (one wave per workgroup, one lane per frame, tiles through LDS).
//     Q_s = (1 / P) sum_p 1 / (1 + exp(beta (r_p(s) - lambda r0_p))) (Best, Hummer & Eaton 2013), everything in fp64 from the
//     fp32 coordinates, the sum in list order, rounded to fp32 once: a frame's value depends on nothing else in the call.
//     Every workgroup checks the pair list while it copies it to LDS (packed to two bytes per pair; lambda r0 as doubles); a
//     pair with an index outside 0 .. N - 1 or with i == j makes every frame NaN, and no coordinate is read through it.
// The two scans are block reduce -> carry scan -> apply, three launches, the carries in the workspace: no workgroup waits on
// another.  Both work on one value per frame, KinScan {cnt, last}, joined by (sum, max); integers only, so the results are
// exact and the same from call to call.
// dff_core_states   "the latest decisive frame wins".  A frame is decisive when it is in a core, is non-finite or is its
//     trajectory's first frame; its key is frame << 2 | kind + 1 (kind -1 / 0 / 1), -1 for every other frame.  The label
//     of a frame is the kind in the inclusive maximum of the keys up to it.  A trajectory's first frame is always
//     decisive, so nothing crosses a trajectory boundary.
// dff_label_runs    a frame starts a run when it is its trajectory's first or differs from its predecessor: cnt sums the
//     starts (the run's index + 1), last is the latest start (the run's first frame).  The frame that ENDS a run -- the
//     next frame starts one, or the launch's frames end -- knows both and writes the run's whole record.
// Trajectories come as the run tables of dff_transition_counts (TransRuns, last_le): up to DFF_TC_RUNS trajectories per
// launch, or any number of equal-length ones.  A launch's frames are whole trajectories, so its scan starts from nothing;
// only the run count is carried from one launch to the next, by the single workgroup of the carry scan.
#pragma once
#include "dff_states.hip"   // TransRuns, last_le, struct_tiles

#define DFF_KIN_THREADS 256
#define DFF_KIN_ITERS 8
#define DFF_KIN_BLOCK (DFF_KIN_THREADS * DFF_KIN_ITERS)   // frames per workgroup: one carry each

// ---- soft fraction of native contacts.  LDS: lambda r0 (P doubles, rounded up to 16 bytes) | tile | packed pairs (P x 2 bytes)
__host__ __device__ __forceinline__ int native_q_r0_floats(int P) { return 2 * ((P + 1) & ~1); }

__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_native_q_kernel(const float* __restrict__ x, long long n, int N,
                                                                               const int* __restrict__ pairs,
                                                                               const float* __restrict__ r0, int P,
                                                                               double beta, double lambda,
                                                                               float* __restrict__ q, unsigned magic,
                                                                               int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    double* lr0 = (double*)smem;
    float* tile = smem + native_q_r0_floats(P);
    unsigned short* pk = (unsigned short*)(tile + DFF_STRUCT_TILE * struct_ld(N));
    bool bad = false;
    for (int p = threadIdx.x; p < P; p += DFF_STRUCT_TILE) {
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        const bool ok = (unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N && i != j;
        bad = bad || !ok;
        pk[p] = (unsigned short)(ok ? (i | (j << 8)) : 0);
        lr0[p] = lambda * (double)r0[p];
    }
    bad = __any(bad) != 0;                                      // the workgroup is one wave
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        if (live) {
            bool good = !bad;
            for (int k = 0; k < 3 * N; ++k) good = good && isfinite(xs[k]);
            double acc = 0.0;
            if (good)
                for (int p = 0; p < P; ++p) {                   // wave-uniform: broadcast LDS reads
                    const int i = 3 * (pk[p] & 0xff), j = 3 * (pk[p] >> 8);
                    const double dx = (double)xs[i] - (double)xs[j], dy = (double)xs[i + 1] - (double)xs[j + 1],
                                 dz = (double)xs[i + 2] - (double)xs[j + 2];
                    const double r = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
                    acc += 1.0 / (1.0 + exp(beta * (r - lr0[p])));   // exp overflows to +inf: the term is 0
                }
            q[s0 + lane] = good ? (float)(acc / (double)P) : __builtin_nanf("");
        }
    });
}

// ---- the scans
struct KinScan {
    long long cnt, last;
};
__device__ __forceinline__ KinScan kin_none() { return KinScan{0, -1}; }
__device__ __forceinline__ KinScan kin_join(KinScan a, KinScan b) {
    return KinScan{a.cnt + b.cnt, a.last > b.last ? a.last : b.last};
}

// Scan over the workgroup in thread order: returns the inclusive value of this thread, `excl` the one of the threads before
// it, `total` the one of the whole workgroup.  wtot: one slot per wave in LDS.
__device__ __forceinline__ KinScan kin_block_scan(KinScan v, KinScan* wtot, KinScan& excl, KinScan& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const KinScan o = {__shfl_up(v.cnt, d), __shfl_up(v.last, d)};
        if (lane >= d) v = kin_join(o, v);
    }
    KinScan before = {__shfl_up(v.cnt, 1), __shfl_up(v.last, 1)};
    if (lane == 0) before = kin_none();
    __syncthreads();                                            // the slots are free of their previous use
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    KinScan pre = kin_none();
    total = kin_none();
#pragma unroll
    for (int w = 0; w < DFF_KIN_THREADS / 64; ++w) {
        if (w < wave) pre = kin_join(pre, wtot[w]);
        total = kin_join(total, wtot[w]);
    }
    excl = kin_join(pre, before);
    return kin_join(pre, v);
}

// is t the first frame of its trajectory (runs.begin <= t < runs.end)
__device__ __forceinline__ bool kin_traj_first(const TransRuns& runs, long long t) {
    if (runs.period > 0) return (t - runs.begin) % runs.period == 0;
    return runs.start[last_le(runs.start, runs.n, t)] == t;
}

// what a frame gives to the scan
struct KinCore {
    const float* cv;
    float lo, hi;
    // 0: non-finite, 1: cv <= lo, 2: cv >= hi, 3: between the cores
    __device__ __forceinline__ int code(long long t) const {
        const float c = cv[t];
        return !isfinite(c) ? 0 : c <= lo ? 1 : c >= hi ? 2 : 3;
    }
    __device__ __forceinline__ KinScan item(const TransRuns& runs, long long t) const {
        const int c = code(t);
        if (c != 3) return KinScan{0, (t << 2) | c};
        return KinScan{0, kin_traj_first(runs, t) ? (t << 2) : -1};
    }
};
struct KinRuns {
    const int* labels;
    __device__ __forceinline__ bool starts(const TransRuns& runs, long long t) const {
        return kin_traj_first(runs, t) || labels[t] != labels[t - 1];
    }
    __device__ __forceinline__ KinScan item(const TransRuns& runs, long long t) const {
        return starts(runs, t) ? KinScan{1, t} : kin_none();
    }
};

// phase 1: agg[b] = the join of the frames of block b of the launch (frames runs.begin + b * DFF_KIN_BLOCK ...)
template <class Src>
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_reduce_kernel(Src src, TransRuns runs, KinScan* __restrict__ agg) {
    __shared__ KinScan wtot[DFF_KIN_THREADS / 64];
    const long long base = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK;
    KinScan v = kin_none();
#pragma unroll
    for (int it = 0; it < DFF_KIN_ITERS; ++it) {
        const long long t = base + it * DFF_KIN_THREADS + threadIdx.x;
        if (t < runs.end) v = kin_join(v, src.item(runs, t));
    }
    KinScan excl, total;
    kin_block_scan(v, wtot, excl, total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// phase 2, one workgroup: agg[b] -> the join of the blocks before b, in place.  count (may be NULL): the running number of
// runs over the launches of a call -- read unless this is the call's first launch, added to every carry, written back with
// this launch's runs added.
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_carry_kernel(KinScan* __restrict__ agg, long long nb,
                                                                         long long* __restrict__ count, int first) {
    __shared__ KinScan wtot[DFF_KIN_THREADS / 64];
    KinScan run = {(count && !first) ? *count : 0, -1};
    for (long long i0 = 0; i0 < nb; i0 += DFF_KIN_THREADS) {
        const long long i = i0 + threadIdx.x;
        KinScan excl, total;
        kin_block_scan(i < nb ? agg[i] : kin_none(), wtot, excl, total);
        if (i < nb) agg[i] = kin_join(run, excl);
        run = kin_join(run, total);
    }
    if (count && threadIdx.x == 0) *count = run.cnt;            // every thread read it before the loop's barriers
}

// phase 3 of dff_core_states
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_core_apply_kernel(KinCore src, TransRuns runs,
                                                                              const KinScan* __restrict__ carry,
                                                                              int* __restrict__ labels,
                                                                              signed char* __restrict__ core) {
    __shared__ KinScan wtot[DFF_KIN_THREADS / 64];
    const long long base = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK;
    KinScan run = carry[blockIdx.x];
    for (int it = 0; it < DFF_KIN_ITERS; ++it) {                // uniform over the workgroup: the scan has barriers
        const long long t = base + it * DFF_KIN_THREADS + threadIdx.x;
        const bool live = t < runs.end;
        KinScan excl, total;
        const KinScan v = kin_join(run, kin_block_scan(live ? src.item(runs, t) : kin_none(), wtot, excl, total));
        if (live) {
            labels[t] = (int)(v.last & 3) - 1;                  // v.last >= 0: the trajectory's first frame is decisive
            if (core) {
                const int c = src.code(t);
                core[t] = (signed char)(c == 1 ? 0 : c == 2 ? 1 : -1);
            }
        }
        run = kin_join(run, total);
    }
}

// phase 3 of dff_label_runs: the last frame of a run writes the run
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_runs_apply_kernel(KinRuns src, TransRuns runs,
                                                                              const KinScan* __restrict__ carry,
                                                                              long long max_runs,
                                                                              long long* __restrict__ run_start,
                                                                              long long* __restrict__ run_length,
                                                                              int* __restrict__ run_label,
                                                                              unsigned char* __restrict__ run_flags) {
    __shared__ KinScan wtot[DFF_KIN_THREADS / 64];
    const long long base = runs.begin + (long long)blockIdx.x * DFF_KIN_BLOCK;
    KinScan run = carry[blockIdx.x];
    for (int it = 0; it < DFF_KIN_ITERS; ++it) {
        const long long t = base + it * DFF_KIN_THREADS + threadIdx.x;
        const bool live = t < runs.end;
        KinScan excl, total;
        const KinScan v = kin_join(run, kin_block_scan(live ? src.item(runs, t) : kin_none(), wtot, excl, total));
        if (live) {
            const bool traj_last = t + 1 == runs.end || kin_traj_first(runs, t + 1);
            const long long r = v.cnt - 1;                      // v.cnt >= 1, v.last = the run's first frame
            if ((traj_last || src.labels[t + 1] != src.labels[t]) && r < max_runs) {
                run_start[r] = v.last;
                run_length[r] = t + 1 - v.last;
                run_label[r] = src.labels[t];
                run_flags[r] = (unsigned char)((kin_traj_first(runs, v.last) ? 1 : 0) | (traj_last ? 2 : 0));
            }
        }
        run = kin_join(run, total);
    }
}
