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
// The two scans are instances of dff_frame_scan.h (block reduce -> carry scan -> apply, forwards only): both work on one value
// per frame, KinScan {cnt, last}, joined by (sum, max).
// dff_core_states   "the latest decisive frame wins".  A frame is decisive when it is in a core, is non-finite or is its
//     trajectory's first frame; its key is frame << 2 | kind + 1 (kind -1 / 0 / 1), -1 for every other frame (core_keys, the
//     rule dff_path_states shares).  The label of a frame is the kind in the inclusive maximum of the keys up to it.  A
//     trajectory's first frame is always decisive, so nothing crosses a trajectory boundary.
// dff_label_runs    a frame starts a run when it is its trajectory's first or differs from its predecessor: cnt sums the
//     starts (the run's index + 1), last is the key of the latest start (the run's first frame): frame << 1 | whether it is
//     its trajectory's first.  The frame that ENDS a run -- the next frame starts one, or the trajectory ends -- knows both
//     and writes the run's whole record.
#pragma once
#include "dff_frame_scan.h"   // the scan, DFF_KIN_*, TrajFrames
#include "dff_frames.h"       // struct_tiles

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
    static __device__ __forceinline__ KinScan none() { return KinScan{0, -1}; }
    static __device__ __forceinline__ KinScan join(KinScan a, KinScan b) {
        return KinScan{a.cnt + b.cnt, a.last > b.last ? a.last : b.last};
    }
};

#define DFF_CORE_NONE 0x7fffffffffffffffLL
// The key rule of the core sets, for frame t with its code (KinCore::code).  fwd: frame << 2 | code where the frame is decisive
// for the frames after it -- it is in a core, is non-finite or is its trajectory's first frame, whose history is unknown
// (code 0) unless it lies in a core itself -- else -1; the maximum of the keys so far is the previous core visit.  bwd: the
// same with the trajectory's LAST frame decisive in place of its first, else DFF_CORE_NONE; the minimum of the keys from a
// frame on is the next core visit.
struct CoreKeys {
    long long fwd, bwd;
};
__device__ __forceinline__ CoreKeys core_keys(int code, long long t, bool traj_first, bool traj_last) {
    const long long key = (t << 2) | (code == 3 ? 0 : code);
    return CoreKeys{code != 3 || traj_first ? key : -1, code != 3 || traj_last ? key : DFF_CORE_NONE};
}

// what the calls hand to the kernels, and what a thread holds of its frames
struct KinCore {
    const float* cv;
    float lo, hi;
    // 0: non-finite, 1: cv <= lo, 2: cv >= hi, 3: between the cores
    __device__ __forceinline__ int code(long long t) const {
        const float c = cv[t];
        return !isfinite(c) ? 0 : c <= lo ? 1 : c >= hi ? 2 : 3;
    }
    using Fwd = KinScan;
    using Rev = ScanNone;
    struct Frames : TrajFrames {
        int code[DFF_KIN_ITERS];
        __device__ __forceinline__ void load(const KinCore& src, const TransRuns& runs) {
            TrajFrames::load(runs);
#pragma unroll
            for (int k = 0; k < DFF_KIN_ITERS; ++k) code[k] = is(live, k) ? src.code(t0 + k) : 3;
        }
        __device__ __forceinline__ CoreKeys keys(int k) const { return core_keys(code[k], t0 + k, is(first, k), is(lastf, k)); }
        __device__ __forceinline__ KinScan fwd(int k) const { return KinScan{0, keys(k).fwd}; }
    };
};
struct KinRuns {
    const int* labels;
    using Fwd = KinScan;
    using Rev = ScanNone;
    struct Frames : TrajFrames {
        int lab[DFF_KIN_ITERS + 2];                             // the labels of frames t0 - 1 .. t0 + DFF_KIN_ITERS
        __device__ __forceinline__ void load(const KinRuns& src, const TransRuns& runs) {
            TrajFrames::load(runs);
#pragma unroll
            for (int k = 0; k < DFF_KIN_ITERS + 2; ++k) {
                const long long t = t0 - 1 + k;
                lab[k] = (t >= runs.begin && t < runs.end) ? src.labels[t] : 0;
            }
        }
        __device__ __forceinline__ bool starts(int k) const { return is(first, k) || lab[k + 1] != lab[k]; }
        __device__ __forceinline__ bool ends(int k) const { return is(lastf, k) || lab[k + 2] != lab[k + 1]; }
        __device__ __forceinline__ KinScan fwd(int k) const {
            return starts(k) ? KinScan{1, ((t0 + k) << 1) | (long long)is(first, k)} : KinScan::none();
        }
    };
};

// phase 3 of dff_core_states
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_core_apply_kernel(KinCore src, TransRuns runs,
                                                                              const KinScan* __restrict__ carry,
                                                                              int* __restrict__ labels, signed char* __restrict__ core) {
    KinCore::Frames fr;
    fr.load(src, runs);
    KinScan run = scan_before(fr, carry);
#pragma unroll
    for (int k = 0; k < DFF_KIN_ITERS; ++k) {
        if (!fr.is(fr.live, k)) continue;
        run = KinScan::join(run, fr.fwd(k));
        labels[fr.t0 + k] = (int)(run.last & 3) - 1;            // run.last >= 0: the trajectory's first frame is decisive
        if (core) core[fr.t0 + k] = (signed char)(fr.code[k] == 1 ? 0 : fr.code[k] == 2 ? 1 : -1);
    }
}

// phase 3 of dff_label_runs: the last frame of a run writes the run
__global__ __launch_bounds__(DFF_KIN_THREADS) void dff_kin_runs_apply_kernel(KinRuns src, TransRuns runs,
                                                                              const KinScan* __restrict__ carry,
                                                                              long long max_runs, long long* __restrict__ run_start,
                                                                              long long* __restrict__ run_length, int* __restrict__ run_label,
                                                                              unsigned char* __restrict__ run_flags) {
    KinRuns::Frames fr;
    fr.load(src, runs);
    KinScan run = scan_before(fr, carry);
#pragma unroll
    for (int k = 0; k < DFF_KIN_ITERS; ++k) {
        if (!fr.is(fr.live, k)) continue;
        run = KinScan::join(run, fr.fwd(k));
        const long long r = run.cnt - 1, start = run.last >> 1; // run.cnt >= 1, run.last: the key of the run's first frame
        if (fr.ends(k) && r < max_runs) {
            run_start[r] = start;
            run_length[r] = fr.t0 + k + 1 - start;
            run_label[r] = fr.lab[k + 1];
            run_flags[r] = (unsigned char)((run.last & 1) | (fr.is(fr.lastf, k) ? 2 : 0));
        }
    }
}
