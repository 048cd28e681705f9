// dff_states.hip -- the "Dynamics" analysis of the reference on the GPU: frames -> states in TIC space -> counts of the
// transitions between them.
//
// Replaces, for (n, N, 3) structures already resident in HBM (evaluate/evaluate_fastfolders.ipynb, cells 20-24):
//   tic_evaluator.tica(get_tic_features(sampled_mol)) followed by
//   MiniBatchKMeans(max_iter=0, initial_centers=preset).fit_transform(...)     cell 22  (dff_struct_tic_assign_kernel)
//   the "standard K-means clustering" the presets came from                     cell 21  (dff_kmeans_step_kernel + _reduce)
//   TransitionCountEstimator.count("sliding", [assignments], lagtime=1)         cell 22  (dff_transition_counts_kernel)
// The row normalisation, the Lloyd loop around the step and the k-means++ draws stay on the host (evaluate.py).
//
// Assignment rule, the same in both kernels that assign (state_nearest): d2_c = sum_j (p_j - centre_cj)^2, one fp64 FMA
// per coordinate in coordinate order; the label is the smallest d2, the lowest index among equals.  A point with a
// non-finite coordinate gets label -1 and d2 = NaN and takes part in no sum.
//
// dff_struct_tic_assign_kernel   the layout of dff_struct_tic_kernel (one wave per workgroup, one lane per frame, tiles
//     through LDS) and its projection (the same function, struct_tic_project: the same bits); the k projections stay in
//     registers, the K centres are wave-uniform loads.
// dff_kmeans_step_kernel         256 threads, one point per lane, grid-stride.  Per 64 points and per cluster present among
//     them (ballot), the members' coordinates are summed by a butterfly over the wave -- a fixed tree, every lane ends
//     with the same bits -- and lane 0 adds them to its wave's LDS accumulators in the order the wave meets its points.
//     A workgroup writes (wave 0 + wave 1) + wave 2 + wave 3 to its slot of the workspace; dff_kmeans_reduce_kernel adds
//     the slots of one accumulator with one wave (lane l: slots l, l + 64, ... in order, then the same butterfly).  The
//     grid is a function of n alone, so every sum has one order: bit-identical from call to call, no floating-point
//     atomics.
// dff_transition_counts_kernel   256 threads, one frame per lane, grid-stride over the frames of up to DFF_TC_RUNS
//     trajectories (or of any number of equal-length ones: period > 0).  A frame looks up where its trajectory ends,
//     then adds one to the workgroup's private 32-bit LDS counter [lag][label t][label t + lag] for every lag that stays
//     inside the trajectory.  Counters go out with one 64-bit integer atomic per non-zero counter, at the end and after
//     every 2^31 frames a workgroup has seen (a counter grows by at most one per frame).  Integer sums do not depend
//     on their order: the result is exact and reproducible.
#pragma once
#include "dff_frames.h"   // struct_tiles, struct_tic_project, wave_sum
#include "dff_traj.h"     // state_nearest, TransRuns, TransLags, DFF_TC_*

#define DFF_KM_THREADS 256
#define DFF_KM_WGS 512             // workgroups, at most: the partial slots the second stage walks

// ---- frames -> state labels.  LDS: tile.  mean (F,), A (F, k), centres (K, k): wave-uniform loads
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_tic_assign_kernel(
    const float* __restrict__ x, long long n, int N, const double* __restrict__ mean, const double* __restrict__ A, int k,
    const double* __restrict__ centers, int K, int* __restrict__ labels, double* __restrict__ proj,
    double* __restrict__ dist2, unsigned magic, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tile = smem;
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        if (live) {
            double acc[DFF_TIC_MAXK];
            struct_tic_project(xs, N, mean, A, k, acc);
            double best;
            labels[s0 + lane] = state_nearest<DFF_TIC_MAXK>(acc, k, centers, K, best);
            if (dist2) dist2[s0 + lane] = best;
            if (proj) {
                double* o = proj + (s0 + lane) * k;
#pragma unroll
                for (int c = 0; c < DFF_TIC_MAXK; ++c)
                    if (c < k) o[c] = acc[c];
            }
        }
    });
}

// ---- one Lloyd step.  Per-workgroup partials: part[block * per + i], per = K d + K + 1: the K x d coordinate sums, the
// K member counts (64-bit integers in the same 8-byte slots), the inertia.  part == NULL: assignment only.
// LDS: 4 waves x per slots
__global__ __launch_bounds__(DFF_KM_THREADS) void dff_kmeans_step_kernel(const double* __restrict__ pts, long long n, int d,
                                                                          const double* __restrict__ centers, int K,
                                                                          int* __restrict__ labels,
                                                                          double* __restrict__ dist2,
                                                                          double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double kacc[];
    const int per = K * d + K + 1, nsum = K * d;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* wacc = kacc + wave * per;
    unsigned long long* wcnt = (unsigned long long*)(wacc + nsum);
    if (part)
        for (int i = lane; i < per; i += 64) {
            if (i >= nsum && i < nsum + K) wcnt[i - nsum] = 0ull; else wacc[i] = 0.0;
        }
    __syncthreads();
    for (long long base = (long long)blockIdx.x * DFF_KM_THREADS; base < n; base += (long long)gridDim.x * DFF_KM_THREADS) {
        const long long t = base + threadIdx.x;
        const bool live = t < n;
        double p[DFF_KM_MAXD];
#pragma unroll
        for (int j = 0; j < DFF_KM_MAXD; ++j) p[j] = (live && j < d) ? pts[t * d + j] : 0.0;
        double best;
        int lab = state_nearest<DFF_KM_MAXD>(p, d, centers, K, best);
        if (!live) lab = -1;
        if (live && labels) labels[t] = lab;
        if (live && dist2) dist2[t] = best;
        if (part) {
            for (int c = 0; c < K; ++c) {
                const bool mine = lab == c;
                const unsigned long long bal = __ballot(mine);
                if (!bal) continue;                                  // wave-uniform
#pragma unroll
                for (int j = 0; j < DFF_KM_MAXD; ++j)
                    if (j < d) {
                        const double s = wave_sum(mine ? p[j] : 0.0);
                        if (lane == 0) wacc[c * d + j] += s;
                    }
                if (lane == 0) wcnt[c] += (unsigned long long)__popcll(bal);
            }
            const double s = wave_sum(lab >= 0 ? best : 0.0);
            if (lane == 0) wacc[nsum + K] += s;
        }
    }
    __syncthreads();
    if (part)
        for (int i = threadIdx.x; i < per; i += DFF_KM_THREADS) {
            double* dst = part + (size_t)blockIdx.x * per + i;
            if (i >= nsum && i < nsum + K) {
                const unsigned long long* c = (const unsigned long long*)kacc;
                *(unsigned long long*)dst = c[i] + c[per + i] + c[2 * per + i] + c[3 * per + i];
            } else {
                *dst = ((kacc[i] + kacc[per + i]) + kacc[2 * per + i]) + kacc[3 * per + i];
            }
        }
}

// ---- slots -> results.  One wave per accumulator: lane l adds slots l, l + 64, ... in that order, then the butterfly
// over the wave -- one fixed tree per slot count.  The results are overwritten.
__global__ __launch_bounds__(64) void dff_kmeans_reduce_kernel(const double* __restrict__ part, int nslots, int d, int K,
                                                               double* __restrict__ sums,
                                                               unsigned long long* __restrict__ counts,
                                                               double* __restrict__ inertia) {
    const int per = K * d + K + 1, nsum = K * d;
    const int i = blockIdx.x, lane = threadIdx.x;              // grid = per
    if (i >= nsum && i < nsum + K) {
        unsigned long long c = 0ull;
        for (int g = lane; g < nslots; g += 64) c += ((const unsigned long long*)part)[(size_t)g * per + i];
        c = wave_sum(c);
        if (counts && lane == 0) counts[i - nsum] = c;
    } else {
        double s = 0.0;
        for (int g = lane; g < nslots; g += 64) s += part[(size_t)g * per + i];
        s = wave_sum(s);
        if (lane == 0) {
            if (i < nsum) { if (sums) sums[i] = s; }
            else if (inertia) inertia[0] = s;
        }
    }
}

// ---- sliding-window transition counts of the lags of one group.  counts: this group's first (K, K) matrix.
// LDS: lags.n x K x K counters
__global__ __launch_bounds__(DFF_TC_THREADS) void dff_transition_counts_kernel(const int* __restrict__ labels, int K,
                                                                                TransRuns runs, TransLags lags,
                                                                                unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned tcl[];
    const int ncnt = lags.n * K * K;
    for (int i = threadIdx.x; i < ncnt; i += DFF_TC_THREADS) tcl[i] = 0u;
    __syncthreads();
    auto flush = [&]() {
        __syncthreads();
        for (int i = threadIdx.x; i < ncnt; i += DFF_TC_THREADS) {
            const unsigned v = tcl[i];
            if (v) {
                atomicAdd(&counts[i], (unsigned long long)v);
                tcl[i] = 0u;
            }
        }
        __syncthreads();
    };
    int iters = 0;
    for (long long base = runs.begin + (long long)blockIdx.x * DFF_TC_THREADS; base < runs.end;
         base += (long long)gridDim.x * DFF_TC_THREADS) {
        const long long t = base + threadIdx.x;
        if (t < runs.end) {
            const int a = labels[t];
            if ((unsigned)a < (unsigned)K) {
                long long e;                                        // one past the last frame of t's trajectory
                if (runs.period > 0) {
                    e = runs.begin + ((t - runs.begin) / runs.period + 1) * runs.period;
                } else {
                    e = runs.start[last_le(runs.start, runs.n, t) + 1];
                }
#pragma unroll
                for (int l = 0; l < DFF_TC_MAXLAGS; ++l)
                    if (l < lags.n && t + lags.lag[l] < e) {
                        const int b = labels[t + lags.lag[l]];
                        if ((unsigned)b < (unsigned)K) atomicAdd(&tcl[(l * K + a) * K + b], 1u);
                    }
            }
        }
        if (++iters == DFF_TC_FLUSH_ITERS) {                         // uniform over the workgroup
            flush();
            iters = 0;
        }
    }
    flush();
}
