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
// dff_msmb_*                    the kernels of dff_msm.hip with a problem index: problem b has K_b states, its compact
//     (K_b, K_b) matrix in slot b of Kmax^2 doubles, its vectors in slots of Kmax.  The live (not skipped) problems are a
//     table of descriptors b * 2048 + K_b in the workspace.  dff_msmb_sweep_kernel: one launch per sweep, grid
//     (ceil(max K_b / 4), live problems), row i = 4 blockIdx.x + wave of problem blockIdx.y; q ping-pongs in the workspace.
//     dff_msmb_loop_kernel: one workgroup per live problem runs all n_steps sweeps with q in LDS.  Rows go through msm_row /
//     msm_q / msm_finish of dff_msm_rows.h, the one copy of the arithmetic: the bits of dff_msm_reversible_steps, problem by
//     problem.  err is (n_steps, B): sweep s of problem b at err[s * B + b].
#pragma once
#include "dff_msm.hip"

#define DFF_MSMB_MAXB 4096           // resamples / problems per call
#define DFF_RC_MAXUNITS (1 << 20)    // resampling units per call
#define DFF_RC_MAXCOUNTERS (1LL << 28)   // B K^2 counters per call (2 GiB)
#define DFF_MSMB_UPLOAD 448          // 64-bit words per upload launch: 3.5 KB of kernel arguments
#define DFF_MSMB_KBITS 11            // a descriptor is b << 11 | K_b, K_b <= 1024 < 2^11

struct MsmbWords {
    long long v[DFF_MSMB_UPLOAD];
};

__global__ __launch_bounds__(64) void dff_msmb_upload_kernel(MsmbWords words, int cnt, long long* __restrict__ dst) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < cnt) dst[i] = words.v[i];
}

// the segment (trajectory, unit) of frame t: start[0] = 0 <= t < start[n]; t0 <= t is the wave's first frame
__device__ __forceinline__ int rc_segment(const long long* __restrict__ start, int n, long long t, long long t0) {
    const int r0 = last_le(start, n, t0);                           // the same addresses in every lane
    return t < start[r0 + 1] ? r0 : last_le(start, n, t);
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

// ---- the batched estimator.  live[p] = b << DFF_MSMB_KBITS | K_b
__global__ __launch_bounds__(256) void dff_msmb_init_kernel(const double* __restrict__ rowc, const double* __restrict__ x,
                                                            int Kmax, const long long* __restrict__ live,
                                                            double* __restrict__ q) {
    const int desc = (int)live[blockIdx.y];
    const int b = desc >> DFF_MSMB_KBITS, K = desc & ((1 << DFF_MSMB_KBITS) - 1);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t o = (size_t)b * Kmax;
    if (i < K) q[o + i] = msm_q(rowc[o + i], x[o + i]);
}

// one sweep of every live problem: row i = 4 blockIdx.x + wave of problem live[blockIdx.y].  err: this sweep's row of B
__global__ __launch_bounds__(DFF_MSM_THREADS) void dff_msmb_sweep_kernel(const double* __restrict__ S,
                                                                         const double* __restrict__ rowc, int Kmax,
                                                                         double* __restrict__ x,
                                                                         const double* __restrict__ qin,
                                                                         double* __restrict__ qout,
                                                                         const long long* __restrict__ live,
                                                                         unsigned long long* __restrict__ err) {
    const int desc = (int)live[blockIdx.y];
    const int b = desc >> DFF_MSMB_KBITS, K = desc & ((1 << DFF_MSMB_KBITS) - 1);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (DFF_MSM_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= K) return;                                             // wave-uniform
    const size_t o = (size_t)b * Kmax;
    double xn = msm_row(S + o * Kmax + (size_t)i * K, qin + o, qin[o + i], K, lane);
    const double xo = x[o + i], ci = rowc[o + i];
    if (!(ci > 0.0 && xo > 0.0)) xn = __builtin_nan("");
    if (lane == 0) {
        x[o + i] = xn;
        qout[o + i] = msm_q(ci, xn);
        msm_finish(xn, xo, err ? err + b : nullptr);
    }
}

// all n_steps sweeps of problem live[blockIdx.x] by one workgroup.  LDS: q ping | q pong | x (3 K_b doubles)
__global__ __launch_bounds__(DFF_MSM_LOOP_THREADS) void dff_msmb_loop_kernel(const double* __restrict__ S,
                                                                             const double* __restrict__ rowc, int Kmax,
                                                                             double* __restrict__ x, int n_steps,
                                                                             const long long* __restrict__ live, int B,
                                                                             unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double mqb[];
    const int desc = (int)live[blockIdx.x];
    const int b = desc >> DFF_MSMB_KBITS, K = desc & ((1 << DFF_MSMB_KBITS) - 1);
    const size_t o = (size_t)b * Kmax;
    S += o * Kmax;
    rowc += o;
    x += o;
    double* qa = mqb;
    double* qb = mqb + K;
    double* xs = mqb + 2 * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < K; i += DFF_MSM_LOOP_THREADS) {
        xs[i] = x[i];
        qa[i] = msm_q(rowc[i], xs[i]);
    }
    __syncthreads();
    for (int s = 0; s < n_steps; ++s) {
        for (int i = wave; i < K; i += DFF_MSM_LOOP_THREADS / 64) {  // wave-uniform
            double xn = msm_row(S + (size_t)i * K, qa, qa[i], K, lane);
            const double xo = xs[i], ci = rowc[i];
            if (!(ci > 0.0 && xo > 0.0)) xn = __builtin_nan("");
            if (lane == 0) {
                xs[i] = xn;
                qb[i] = msm_q(ci, xn);
                msm_finish(xn, xo, err ? err + (size_t)s * B + b : nullptr);
            }
        }
        __syncthreads();
        double* t = qa; qa = qb; qb = t;
    }
    for (int i = threadIdx.x; i < K; i += DFF_MSM_LOOP_THREADS) x[i] = xs[i];
}
