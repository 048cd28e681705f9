// dff_msm_rows.h -- the arithmetic of one row of the reversible estimator's sweep, x_i' = sum_j S_ij / (q_i + q_j) with
// q_j = c_j / x_j: ONE copy for both drivers of dff_msm.hip (one launch per sweep; one looping workgroup), whether they run
// on one problem or on many per launch (dff_msm_batch.hip), so that all of them give the same bits.
#pragma once
#include "dff_frames.h"   // wave_sum

// q of a state from its row count and its x; NaN where the estimator is not defined (c <= 0, x <= 0, either NaN)
__device__ __forceinline__ double msm_q(double c, double x) { return (c > 0.0 && x > 0.0) ? c / x : __builtin_nan(""); }

// sum_j S_ij / (q_i + q_j) over one row, by one wave: lane l takes j = l, l + 64, ... in order, then the butterfly; a pair
// with S_ij == 0 adds exactly +0.0, whatever its quotient.  The same bits in every lane.
__device__ __forceinline__ double msm_row(const double* __restrict__ srow, const double* q, double qi, int K, int lane) {
    double acc = 0.0;
#pragma unroll 4
    for (int j = lane; j < K; j += 64) {                            // loads first, no branch: the row is latency-bound
        const double s = srow[j];
        const double t = s / (qi + q[j]);
        acc += (s != 0.0) ? t : 0.0;                                // +0.0 leaves acc's bits alone
    }
    return wave_sum(acc);
}

// the row's new x, its relative change into err (an integer max on the bit pattern: both non-negative or NaN)
__device__ __forceinline__ void msm_finish(double xn, double xo, unsigned long long* err) {
    if (err) atomicMax(err, (unsigned long long)__double_as_longlong(fabs(xn - xo) / xo));
}
