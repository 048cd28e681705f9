// dff_msm_batch.hip -- what a bootstrap of a Markov state model needs B times over, in one call each: the count matrices of
// B weighted resamples of the trajectories (or of blocks of them), and the reversible estimator's sweeps on B problems at once.
//
// dff_msmb_upload_kernel        host tables (segment starts, problem descriptors) travel as kernel ARGUMENTS, DFF_MSMB_UPLOAD
//     64-bit words per launch, into the workspace: ordered on the stream, no host-to-device copy that could wait for it.
// dff_micro_rc_kernel           the frame loop of dff_micro_tc_kernel at one lag.  A pair (t, t + lag) belongs to the unit of
//     frame t; trajectory ends and unit starts are tables in the workspace, searched once per wave (its first frame) and
//     again only by the lanes past that segment's end.  A wave aggregates equal (i, j, unit) triples: the first pending
//     lane's triple is broadcast, the lanes that hold it are counted by a ballot, and then the LANES RUN OVER THE RESAMPLES:
//     lane l adds count * weights[b][unit] to counts[b][i][j] for b = l, l + 64, ... -- one 64-bit integer atomic per
//     (triple, resample with a non-zero weight), 64 of them in flight per instruction, each to another matrix.  The weight
//     is uniform over the aggregated lanes by construction, so no reduction over the wave is needed.  Integer adds: exact,
//     the same whatever the order.
// MsmLive                       the problem locator that runs the kernels of dff_msm.hip on many problems per launch: problem b
//     has K_b states, its compact (K_b, K_b) matrix in slot b of Kmax^2 doubles, its vectors in slots of Kmax.  The live (not
//     skipped) problems are a table of descriptors b * 2048 + K_b in the workspace.  dff_msm_sweep_kernel<MsmLive>: one launch
//     per sweep, grid (ceil(max K_b / 4), live problems); dff_msm_loop_kernel<MsmLive>: one workgroup per live problem.  The
//     same kernels as the single call's, hence its bits, problem by problem.  err is (n_steps, B): sweep s of problem b at
//     err[s * B + b].
#pragma once
#include "dff_msm.hip"       // the estimator kernels that MsmLive instantiates
#include "dff_msm_table.h"   // the live problems' descriptors
#include "dff_upload.h"      // MsmbWords, DFF_MSMB_UPLOAD

#define DFF_MSMB_MAXB 4096           // resamples / problems per call
#define DFF_RC_MAXUNITS (1 << 20)    // resampling units per call
#define DFF_RC_MAXCOUNTERS (1LL << 28)   // B K^2 counters per call (2 GiB)

__global__ __launch_bounds__(64) void dff_msmb_upload_kernel(MsmbWords words, int cnt, long long* __restrict__ dst) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < cnt) dst[i] = words.v[i];
}

// ---- weighted sliding-window counts of B resamples into counts (B, K, K), zeroed before.  tstart (n_traj + 1) and ustart
// (n_units + 1): ascending frame indices from 0 to n; weights (B, n_units).
__global__ __launch_bounds__(DFF_TC_THREADS) void dff_micro_rc_kernel(const int* __restrict__ labels, long long n, int lag,
                                                                       int K, const long long* __restrict__ tstart,
                                                                       int n_traj, const long long* __restrict__ ustart,
                                                                       int n_units, const unsigned* __restrict__ weights,
                                                                       int B, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const size_t KK = (size_t)K * K;
    for (long long base = (long long)blockIdx.x * DFF_TC_THREADS; base < n;
         base += (long long)gridDim.x * DFF_TC_THREADS) {                 // uniform over the workgroup
        const long long t = base + threadIdx.x;
        const long long t0 = t - lane;                                      // the wave's first frame
        int key = -1, u = 0;
        if (t < n) {                                                        // t0 <= t < n
            const int a = labels[t];
            if ((unsigned)a < (unsigned)K) {
                const long long e = tstart[rc_segment(tstart, n_traj, t, t0) + 1];   // one past t's trajectory, <= n
                if (t + lag < e) {
                    const int b = labels[t + lag];
                    if ((unsigned)b < (unsigned)K) {
                        key = a * K + b;                                    // < 2^20
                        u = rc_segment(ustart, n_units, t, t0);             // 0 .. n_units - 1
                    }
                }
            }
        }
        bool pend = key >= 0;
        for (;;) {                                                          // at most 64 rounds: one per distinct triple
            const unsigned long long m = __ballot(pend);
            if (!m) break;                                                  // wave-uniform
            const int lead = __ffsll((long long)m) - 1;
            const int k0 = __shfl(key, lead), u0 = __shfl(u, lead);
            const bool same = pend && key == k0 && u == u0;
            const unsigned long long cnt = (unsigned long long)__popcll(__ballot(same));
            for (int b = lane; b < B; b += 64) {
                const unsigned long long w = weights[(size_t)b * n_units + u0];
                if (w) atomicAdd(&counts[(size_t)b * KK + k0], w * cnt);   // <= 2^32 * 2^31 in all: no overflow
            }
            pend = pend && !same;
        }
    }
}

// ---- the batched estimator: the locator of dff_msm.hip's kernels over a table of live problems, live[p] = b <<
// DFF_MSM_KBITS | K_b (dff_msm_table.h), in slots of Kmax; err is (n_steps, B)
struct MsmLive {
    const long long* live;
    int Kmax, B;
    __device__ MsmAt at(unsigned p) const {
        const int desc = (int)live[p];
        return {MSM_PROBLEM_SLOT(desc), MSM_PROBLEM_K(desc)};
    }
    __host__ __device__ int stride() const { return Kmax; }
    __host__ __device__ int err_stride() const { return B; }
};
