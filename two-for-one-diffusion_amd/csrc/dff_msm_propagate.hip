// dff_msm_propagate.hip -- row vectors through a transition matrix, step after step: w_{s+1} = w_s T for up to 16 start vectors
// per problem, and after every step their scalar products with up to 16 observables, out[s][m][r] = sum_j w_s[m][j] obs[r][j].
// Many problems per call, ONE workgroup of 512 threads per problem for all S steps (the Chapman-Kolmogorov test, relaxations
// and autocorrelations of Markov state models).  T is a general dense (K, K) fp64 matrix: nothing assumes that it is stochastic.
//
// The vectors live in LDS as wbuf[i][16] (state-major, the 16 rows of a state side by side): a thread that owns a column reads
// the rows' values of state i as one broadcast.  ONE buffer: the products of a step stay in registers until every thread has
// read w_s (barrier), are written over it (barrier), and the next step starts.  Two barriers per step.
//
// prop_step      (w_s T)[m][j] = sum_i w_s[m][i] T[i][j] as ONE chain of fused multiply-adds over i = 0, 1, ..., K - 1 from +0.
//     The order is the same on both paths and whichever thread holds (m, j): the bits of row m follow from row m and T alone.
//   dff_prop_kernel<true>   K <= DFF_PROP_LDS_LIMIT: T is copied into LDS once.  Thread (q, j) = (tid / 128, tid % 128) owns
//     column j of rows 4 q .. 4 q + 3: T[i][j] is a conflict-free LDS read, the four w a 32-byte broadcast.
//   dff_prop_kernel<false>  larger K: T streams from global memory every step, row by row, coalesced (thread t owns columns
//     t and t + 512); all rows of the problem in the same thread (4, 8 or 16 accumulators per column, by M: idle rows are
//     skipped, the chains of the live ones are the same), so T is read ONCE per step whatever M.
// prop_project   out[s][m][r]: thread (m, slot) = (tid % 16, tid / 16) adds w_s[m][j] obs[r][j] over j = slot, slot + 32, ... by
//     fused multiply-adds; the four slots of a wave are added by a butterfly (lanes ^ 16, ^ 32), the eight waves in wave order.
//     It reads the same w_s as prop_step and runs between the same two barriers.  The observables: LDS (obsl[j][16]) on the
//     LDS path, global memory on the other.
// Non-finite entries (below K_p) in T, w0 or obs: status 1, every output of the problem NaN.  A NaN that finite inputs produce
// on the way (an overflow to infinity, then inf - inf or 0 inf) shows in out, because every w_s[m][j] enters out[s][m][.]:
// status 2, every output NaN.  Status 0 never comes with a NaN.  No atomics, no workgroup waits on another.
#pragma once
#include <hip/hip_runtime.h>
#include "dff_msm_table.h"   // the problems' descriptors

#define DFF_PROP_THREADS 512
#define DFF_PROP_MAXP 16384           // problems per call
#define DFF_PROP_MAXROWS 16           // start vectors per problem, observables per problem
#define DFF_PROP_MAXSTEPS 65535
#define DFF_PROP_MAXOUT (1LL << 28)   // doubles of out per call (2 GiB)
#define DFF_PROP_LDS_FIT 120          // the largest K whose matrix, vectors, observables and partial sums fit 160 KB of LDS
#define DFF_PROP_LDS_LIMIT 120        // the largest K propagated out of LDS: measured, LDS wins up to where it fits
#define DFF_PROP_SLOTS (DFF_PROP_THREADS / DFF_PROP_MAXROWS)   // 32 column slots of prop_project
#define DFF_PROP_WAVES (DFF_PROP_THREADS / 64)

// dynamic LDS: wbuf (K x 16) | partial sums (8 waves x 256) | LDS path only: obsl (K x 16) | T (K x K)
__host__ inline size_t prop_lds_bytes(int K, bool ldsp) {
    long long v = (long long)K * DFF_PROP_MAXROWS + DFF_PROP_WAVES * DFF_PROP_MAXROWS * DFF_PROP_MAXROWS;
    if (ldsp) v += (long long)K * DFF_PROP_MAXROWS + (long long)K * K;
    return (size_t)v * sizeof(double);
}

static_assert(DFF_PROP_LDS_LIMIT <= DFF_PROP_LDS_FIT, "the LDS path's matrix must fit");

__device__ __forceinline__ bool prop_finite(double x) { return x - x == 0.0; }

// ---- acc[c][r] = sum_i wbuf[i][row0 + r] A[i][j0 + c jstep], i ascending, one fma chain each.  A: (K, K) row-major, LDS or global.
template <int ROWS, int NC>
__device__ __forceinline__ void prop_step(const double* __restrict__ A, int K, const double* wbuf, int row0, int j0, int jstep,
                                          double (&acc)[NC][ROWS]) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[c][r] = 0.0;
    bool live[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) live[c] = j0 + c * jstep < K;
    const double* a = A + j0;
    const double* w = wbuf + row0;
    constexpr int UNR = ROWS * NC >= 32 ? 2 : (ROWS * NC >= 16 ? 4 : 8);   // rows of T in flight: as many as the registers take
#pragma unroll UNR
    for (int i = 0; i < K; ++i) {
        double t[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) t[c] = live[c] ? a[(size_t)i * K + c * jstep] : 0.0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double wr = w[i * DFF_PROP_MAXROWS + r];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c][r] = fma(wr, t[c], acc[c][r]);
        }
    }
}

template <int ROWS, int NC>
__device__ __forceinline__ void prop_store(double* wbuf, int K, int row0, int j0, int jstep, const double (&acc)[NC][ROWS]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = j0 + c * jstep;
        if (j < K)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) wbuf[j * DFF_PROP_MAXROWS + row0 + r] = acc[c][r];
    }
}

// the global path's step for ROWS live rows: products into registers, barrier, over w_s, barrier
template <int ROWS>
__device__ __forceinline__ void prop_step_global(const double* __restrict__ A, int K, double* wbuf) {
    const int tid = threadIdx.x;
    if (K <= DFF_PROP_THREADS) {
        double acc[1][ROWS];
        if (tid < K) prop_step<ROWS, 1>(A, K, wbuf, 0, tid, DFF_PROP_THREADS, acc);
        __syncthreads();
        if (tid < K) prop_store<ROWS, 1>(wbuf, K, 0, tid, DFF_PROP_THREADS, acc);
    } else {
        double acc[2][ROWS];
        prop_step<ROWS, 2>(A, K, wbuf, 0, tid, DFF_PROP_THREADS, acc);
        __syncthreads();
        prop_store<ROWS, 2>(wbuf, K, 0, tid, DFF_PROP_THREADS, acc);
    }
}

// ---- the partial sums of out[s] of this wave into part[wave][m][r] (see the head of the file).  obs element (r, j) at
// obs[r * ro + j * jo]: (ro, jo) = (1, 16) for obsl, (Kmax, 1) for global memory.
__device__ __forceinline__ void prop_project(const double* wbuf, const double* __restrict__ obs, int ro, int jo, int K, int M, int R,
                                             double* part) {
    const int tid = threadIdx.x, m = tid & (DFF_PROP_MAXROWS - 1), slot = tid >> 4;
    double acc[DFF_PROP_MAXROWS];
#pragma unroll
    for (int r = 0; r < DFF_PROP_MAXROWS; ++r) acc[r] = 0.0;
    if (m < M)
        for (int j = slot; j < K; j += DFF_PROP_SLOTS) {
            const double wv = wbuf[j * DFF_PROP_MAXROWS + m];
            const double* o = obs + (size_t)j * jo;
#pragma unroll
            for (int r = 0; r < DFF_PROP_MAXROWS; ++r)
                if (r < R) acc[r] = fma(wv, o[(size_t)r * ro], acc[r]);
        }
#pragma unroll
    for (int r = 0; r < DFF_PROP_MAXROWS; ++r) {
        if (r < R) {                                                 // uniform over the workgroup
            double v = acc[r];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if ((tid & 63) < DFF_PROP_MAXROWS) part[((tid >> 6) * DFF_PROP_MAXROWS + m) * DFF_PROP_MAXROWS + r] = v;
        }
    }
}

// ---- one workgroup per problem.  desc[p] = matrix slot << DFF_MSM_KBITS | K_p (dff_msm_table.h); t: slots of Kmax^2; w0 (P, M, Kmax); obs
// (P, R, Kmax); out (P, S + 1, M, R); wlast (P, M, Kmax) or NULL.  The workgroup owns the problem when own_lo <= K_p <= own_hi,
// else it leaves at once (the other path's launch takes it).
template <bool LDSP>
__global__ __launch_bounds__(DFF_PROP_THREADS) void dff_prop_kernel(const double* __restrict__ t, const long long* __restrict__ desc,
                                                                    int Kmax, const double* __restrict__ w0, int M,
                                                                    const double* __restrict__ obs, int R, int S,
                                                                    double* __restrict__ out, double* __restrict__ wlast,
                                                                    int* __restrict__ status, int own_lo, int own_hi) {
    constexpr int T = DFF_PROP_THREADS, MR = DFF_PROP_MAXROWS;
    extern __shared__ __attribute__((aligned(16))) unsigned char prop_lds[];
    const unsigned pr = blockIdx.x;
    const long long d = desc[pr];
    const int K = MSM_PROBLEM_K(d), tid = threadIdx.x;
    if (K < own_lo || K > own_hi) return;
    const double* A = t + (size_t)MSM_PROBLEM_SLOT(d) * Kmax * Kmax;
    double* wbuf = (double*)prop_lds;
    double* part = wbuf + (size_t)K * MR;
    double* obsl = part + DFF_PROP_WAVES * MR * MR;                  // LDS path only
    double* tl = obsl + (size_t)K * MR;                              // LDS path only
    w0 += (size_t)pr * M * Kmax;
    obs += (size_t)pr * R * Kmax;
    out += (size_t)pr * (S + 1) * M * R;
    if (wlast) wlast += (size_t)pr * M * Kmax;
    int bad = 0;
    for (int idx = tid; idx < K * K; idx += T) {                    // T: checked on both paths, kept on one
        const double x = A[idx];
        bad |= !prop_finite(x);
        if constexpr (LDSP) tl[idx] = x;
    }
    for (int idx = tid; idx < K * MR; idx += T) {                   // rows beyond M are zero: they are computed, never stored
        const int j = idx / MR, m = idx - j * MR;
        const double x = m < M ? w0[(size_t)m * Kmax + j] : 0.0;
        bad |= !prop_finite(x);
        wbuf[idx] = x;
    }
    for (int idx = tid; idx < K * R; idx += T) {
        const int r = idx / K, j = idx - r * K;
        const double x = obs[(size_t)r * Kmax + j];
        bad |= !prop_finite(x);
        if constexpr (LDSP) obsl[j * MR + r] = x;
    }
    bad = __syncthreads_or(bad);                                    // ... and w_0, T, obs are in place
    int nan_seen = 0;
    if (!bad) {
        const int q = tid >> 7, jl = tid & 127;                     // LDS path: column jl of rows 4 q .. 4 q + 3
        const bool mine = 4 * q < M && jl < K;
        const int pm = tid >> 4, pq = tid & (MR - 1);               // the pair (m, r) whose out this thread finishes
        for (int s = 0; s <= S; ++s) {
            if constexpr (LDSP) prop_project(wbuf, obsl, 1, MR, K, M, R, part);
            else prop_project(wbuf, obs, Kmax, 1, K, M, R, part);
            const bool step = s < S;
            if constexpr (LDSP) {
                double acc[1][4];
                if (step && mine) prop_step<4, 1>(tl, K, wbuf, 4 * q, jl, 0, acc);
                __syncthreads();
                if (step && mine) prop_store<4, 1>(wbuf, K, 4 * q, jl, 0, acc);
            } else if (!step) {
                __syncthreads();
            } else if (M <= 4) {
                prop_step_global<4>(A, K, wbuf);
            } else if (M <= 8) {
                prop_step_global<8>(A, K, wbuf);
            } else {
                prop_step_global<16>(A, K, wbuf);
            }
            if (tid < MR * MR && pm < M && pq < R) {                // the waves' partial sums in wave order
                double v = 0.0;
#pragma unroll
                for (int w = 0; w < DFF_PROP_WAVES; ++w) v += part[(w * MR + pm) * MR + pq];
                nan_seen |= v != v;
                out[((size_t)s * M + pm) * R + pq] = v;
            }
            __syncthreads();
        }
    }
    nan_seen = __syncthreads_or(nan_seen);
    const double nan = __builtin_nan("");
    if (bad || nan_seen)
        for (long long idx = tid; idx < (long long)(S + 1) * M * R; idx += T) out[idx] = nan;
    if (wlast)
        for (int idx = tid; idx < M * K; idx += T) {
            const int m = idx / K, j = idx - m * K;
            wlast[(size_t)m * Kmax + j] = (bad || nan_seen) ? nan : wbuf[j * MR + m];
        }
    if (tid == 0) status[pr] = bad ? 1 : (nan_seen ? 2 : 0);
}
