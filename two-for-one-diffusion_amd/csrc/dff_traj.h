// dff_traj.h -- state labels along trajectories: the limits, the assignment rule and the tables that the state, kinetics,
// autocorrelation and Markov-model files share.  Device helpers and plain structs only: no kernel lives here.
#pragma once
#include "dff_frames.h"   // last_le

#define DFF_STATES_MAXK 64         // states / cluster centres
#define DFF_KM_MAXD 8              // coordinates per point (= DFF_TIC_MAXK)
#define DFF_TC_THREADS 256
#define DFF_TC_WGS 1024
#define DFF_TC_MAXLAGS 8
#define DFF_TC_RUNS 64             // trajectories per launch (kernel argument)
#define DFF_TC_LDS_COUNTERS 8192   // 32 KB of private counters: lags are processed in groups of DFF_TC_LDS_COUNTERS / K^2
#define DFF_TC_FLUSH_ITERS (1 << 23)   // x 256 threads = 2^31 frames per workgroup between flushes

// label of the nearest of K centres (K, d) row-major to p (d <= MAXD coordinates), best = its squared distance
template <int MAXD>
__device__ __forceinline__ int state_nearest(const double (&p)[MAXD], int d, const double* __restrict__ centers, int K,
                                             double& best) {
    bool finite = true;
#pragma unroll
    for (int j = 0; j < MAXD; ++j)
        if (j < d) finite = finite && isfinite(p[j]);
    int lab = 0;
    best = 0.0;
    for (int c = 0; c < K; ++c) {
        double d2 = 0.0;
#pragma unroll
        for (int j = 0; j < MAXD; ++j)
            if (j < d) {
                const double e = p[j] - centers[c * d + j];
                d2 = fma(e, e, d2);
            }
        if (c == 0 || d2 < best) { best = d2; lab = c; }
    }
    if (!finite) { lab = -1; best = __builtin_nan(""); }
    return lab;
}

// the trajectories of one launch: frames begin .. end.  period > 0: back-to-back trajectories of `period` frames each
// from `begin` on; else trajectory r holds frames start[r] .. start[r + 1] - 1 (start[0] = begin, start[n] = end)
struct TransRuns {
    long long begin, end, period;
    int n;
    long long start[DFF_TC_RUNS + 1];
};
struct TransLags {
    int n;
    int lag[DFF_TC_MAXLAGS];
};

// the segment (trajectory, unit) of frame t: start[0] = 0 <= t < start[n]; t0 <= t is the wave's first frame
__device__ __forceinline__ int rc_segment(const long long* __restrict__ start, int n, long long t, long long t0) {
    const int r0 = last_le(start, n, t0);                           // the same addresses in every lane
    return t < start[r0 + 1] ? r0 : last_le(start, n, t);
}
