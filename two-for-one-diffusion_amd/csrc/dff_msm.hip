// dff_msm.hip -- Markov state models at microstate resolution: k-means with up to DFF_MSM_MAXK centres, transition counts
// between that many states, and the sweeps of the reversible maximum-likelihood estimator.  The semantics of the K <= 64
// calls of dff_states.hip (assignment rule, trajectories, skipped labels) carry over unchanged; what changes is where the
// K-sized state lives: centres and accumulators in LDS, counters in global memory.
//
// dff_micro_kmeans_kernel        one workgroup of 256 threads per CHUNK of DFF_MICRO_CHUNK points -- never a grid stride, so
//     the order of every sum follows from (n, d, K) and the chunk size alone.  Phase 1, assignment: the K x d centres sit
//     in LDS, every lane carries DFF_MICRO_PPL points in registers and walks the centres in index order (state_nearest's
//     rule and arithmetic: the same bits); one broadcast LDS read feeds DFF_MICRO_PPL FMAs.  Phase 2, accumulation (only with a
//     workspace): labels and coordinates of the chunk are staged in LDS, the centres' LDS is reused for K (d + 1)
//     accumulator slots, slot c (d + 1) + j = coordinate j of cluster c (j = d: its 64-bit member count).  The 256 threads
//     form G = 4, 2 or 1 groups of T = 256 / G (micro_groups: a function of (d, K), as many sets of slots as LDS holds);
//     group g walks its G-th of the chunk's points, in point order, into its own set.  Thread o of a group OWNS the slots s
//     with s mod T == o: for a point of cluster c the owner of slot c (d + 1) + j is thread (c (d + 1) + j) mod T, so each
//     thread finds at most one j in 0 .. d that is its own and adds that one value.  A slot is only ever touched by its
//     owner, in point order: sequential per slot, no atomics, and no loop over K.  The sets are added in group order.  The inertia of the chunk: every lane adds its points in order, a butterfly per wave, then
//     ((w0 + w1) + w2) + w3.  The chunk's partial (K (d + 1) slots + the inertia) goes to its row of the workspace.
// dff_micro_kmeans_reduce_kernel rows -> results.  64 accumulators per workgroup, one per lane (coalesced rows); wave w adds
//     the rows w, w + 4, ... in that order, the four waves are combined ((w0 + w1) + w2) + w3.
// dff_micro_tc_kernel            the frame loop of dff_transition_counts_kernel with the counters in global memory: K^2
//     counters per lag do not fit in LDS.  Before the 64-bit integer atomic a wave aggregates equal (lag, i, j) keys: up
//     to DFF_MICRO_TC_ROUNDS times the first pending lane's key is broadcast, the lanes that hold it are counted by a
//     ballot and that lane adds the count; what is still pending adds one each.  A metastable trajectory hits the
//     diagonal: mostly one or two atomics per wave and lag.
// dff_msm_*                      x_i' = sum_j S_ij / (q_i + q_j), q_j = c_j / x_j: one wave per row, lanes stride over j,
//     then the butterfly (msm_row: one order, whichever kernel calls it).  x is updated in place by the wave that owns
//     the row; q is read by every row and ping-pongs.  Two drivers with the same bits: dff_msm_sweep_kernel, one launch
//     per sweep (K / 4 workgroups per problem), q ping-pongs in the workspace; dff_msm_loop_kernel, ONE workgroup per
//     problem that runs all n_steps sweeps with q in LDS and a workgroup barrier between sweeps (no launch boundary: the
//     faster one for few states).  Each is a template over a problem locator: MsmOne (one problem, carried by value:
//     dff_msm_reversible_steps) or MsmLive of dff_msm_batch.hip (a table of problems: the batched call).  err_s = max_i |x_i' - x_i| / x_i by an integer atomic max on the bits of the non-negative double (a NaN
//     has the largest pattern: one NaN row makes err NaN).
#pragma once
#include "dff_traj.h"       // state_nearest's rule, DFF_KM_MAXD, TransRuns, TransLags, last_le
#include "dff_msm_rows.h"   // msm_q, msm_row, msm_finish

#define DFF_MICRO_CHUNK 1024       // points per workgroup: at K = 1024, d = 8 the largest power of two whose coordinates
                                    // (64 KB) + labels (4 KB) + accumulators (72 KB) fit in the 160 KB of LDS
#define DFF_MICRO_THREADS 256
#define DFF_MICRO_PPL (DFF_MICRO_CHUNK / DFF_MICRO_THREADS)   // points per lane
#define DFF_MICRO_TC_ROUNDS 4
#define DFF_MSM_THREADS 256         // 4 rows per workgroup
#define DFF_MSM_LOOP_THREADS 1024   // 16 rows in flight in the one-workgroup driver

// LDS of dff_micro_kmeans_kernel in doubles: centres, reused for the accumulator slots | 4 wave inertias | coordinates |
// labels (ints)
// (one set of slots per group of threads, each rounded up to an even count: what follows stays 16-byte aligned)
__host__ __device__ inline int micro_set_doubles(int d, int K) { return (K * (d + 1) + 1) & ~1; }
__host__ inline size_t micro_lds_bytes(int d, int K, int groups) {       // groups == 0: assignment only
    if (!groups) return (size_t)K * d * sizeof(double);
    return (size_t)groups * micro_set_doubles(d, K) * sizeof(double) + 4 * sizeof(double) +
           (size_t)DFF_MICRO_CHUNK * d * sizeof(double) + DFF_MICRO_CHUNK * sizeof(int);
}
// Accumulator sets per workgroup, a function of (d, K) alone: 4, 2 or 1 groups of 64, 128 or 256 threads, each walking its
// own quarter / half / all of the chunk into its own set -- as many as fit without costing the second workgroup per CU
// that one set would leave room for.
__host__ inline int micro_groups(int d, int K) {
    const size_t lds = 160 * 1024;
    const size_t want = lds / micro_lds_bytes(d, K, 1) < 2 ? lds / micro_lds_bytes(d, K, 1) : 2;
    for (int g = 4; g > 1; g >>= 1)
        if (micro_lds_bytes(d, K, g) <= lds && lds / micro_lds_bytes(d, K, g) >= want) return g;
    return 1;
}

// ---- one Lloyd step over chunk blockIdx.x.  part == NULL: assignment only (LDS: the centres alone).
// part[chunk * per + s], per = K (d + 1) + 1: the slots above, then the chunk's inertia.
template <bool ACC>
__global__ __launch_bounds__(DFF_MICRO_THREADS) void dff_micro_kmeans_kernel(const double* __restrict__ pts, long long n,
                                                                              int d, const double* __restrict__ centers,
                                                                              int K, int* __restrict__ labels,
                                                                              double* __restrict__ dist2,
                                                                              double* __restrict__ part, int groups) {
    extern __shared__ __attribute__((aligned(16))) double msm[];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * DFF_MICRO_CHUNK;
    const int cnt = (int)(n - base < DFF_MICRO_CHUNK ? n - base : DFF_MICRO_CHUNK);
    double* cen = msm;                                              // K d, later K (d + 1) slots
    const int nslot = K * (d + 1);
    const int nset = micro_set_doubles(d, K);
    double* winert = msm + groups * nset;                           // ACC only
    double* spts = winert + 4;
    int* slab = (int*)(spts + DFF_MICRO_CHUNK * d);
    for (int i = tid; i < K * d; i += DFF_MICRO_THREADS) cen[i] = centers[i];

    // this lane's points: base + q * 256 + tid
    double p[DFF_MICRO_PPL][DFF_KM_MAXD];
    bool finite[DFF_MICRO_PPL];
#pragma unroll
    for (int q = 0; q < DFF_MICRO_PPL; ++q) {
        const int i = q * DFF_MICRO_THREADS + tid;
        finite[q] = true;
#pragma unroll
        for (int j = 0; j < DFF_KM_MAXD; ++j) {
            p[q][j] = (i < cnt && j < d) ? pts[(base + i) * d + j] : 0.0;
            if (j < d) finite[q] = finite[q] && isfinite(p[q][j]);
        }
    }
    __syncthreads();

    // state_nearest for DFF_MICRO_PPL points at once: centres in index order, one FMA per coordinate in coordinate order,
    // strict <
    double best[DFF_MICRO_PPL];
    int lab[DFF_MICRO_PPL];
#pragma unroll
    for (int q = 0; q < DFF_MICRO_PPL; ++q) { best[q] = 0.0; lab[q] = 0; }
    for (int c = 0; c < K; ++c) {
        double d2[DFF_MICRO_PPL];
#pragma unroll
        for (int q = 0; q < DFF_MICRO_PPL; ++q) d2[q] = 0.0;
#pragma unroll
        for (int j = 0; j < DFF_KM_MAXD; ++j)
            if (j < d) {
                const double cj = cen[c * d + j];
#pragma unroll
                for (int q = 0; q < DFF_MICRO_PPL; ++q) {
                    const double e = p[q][j] - cj;
                    d2[q] = fma(e, e, d2[q]);
                }
            }
#pragma unroll
        for (int q = 0; q < DFF_MICRO_PPL; ++q)
            if (c == 0 || d2[q] < best[q]) { best[q] = d2[q]; lab[q] = c; }
    }
    double inert = 0.0;
#pragma unroll
    for (int q = 0; q < DFF_MICRO_PPL; ++q) {
        const int i = q * DFF_MICRO_THREADS + tid;
        if (!finite[q]) { lab[q] = -1; best[q] = __builtin_nan(""); }
        if (i < cnt) {
            if (labels) labels[base + i] = lab[q];
            if (dist2) dist2[base + i] = best[q];
            if (lab[q] >= 0) inert += best[q];
        }
    }
    if (!ACC) return;

    __syncthreads();                                                // every wave is done with the centres
#pragma unroll
    for (int q = 0; q < DFF_MICRO_PPL; ++q) {
        const int i = q * DFF_MICRO_THREADS + tid;
        if (i < cnt) {
            slab[i] = lab[q];
#pragma unroll
            for (int j = 0; j < DFF_KM_MAXD; ++j)
                if (j < d) spts[i * d + j] = p[q][j];
        }
    }
    for (int s = tid; s < groups * nset; s += DFF_MICRO_THREADS) ((unsigned long long*)cen)[s] = 0ull;   // +0.0 and 0 alike
    inert = wave_sum(inert);
    if ((tid & 63) == 0) winert[tid >> 6] = inert;
    __syncthreads();

    // group g = T threads, T = 256 / groups: walks the points [g C / groups, (g + 1) C / groups) of the chunk into set g;
    // thread o of the group owns the slots s with s mod T == o
    const int dp = d + 1, T = DFF_MICRO_THREADS / groups, g = tid / T, o = tid - g * T;
    double* acc = cen + g * nset;
    const int lo = g * (DFF_MICRO_CHUNK / groups);
    const int hi = cnt < lo + DFF_MICRO_CHUNK / groups ? cnt : lo + DFF_MICRO_CHUNK / groups;
    // four points per round: their labels in one read, the values this thread owns fetched before the adds; the adds stay
    // in point order
    int i = lo;
    for (; i + 4 <= hi; i += 4) {
        const int4 c4 = *(const int4*)(slab + i);
        const int cs[4] = {c4.x, c4.y, c4.z, c4.w};
        int s[4];
        bool count[4];
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = (o - cs[q] * dp) & (T - 1);                   // the one j with (c dp + j) mod T == o, if <= d
            const bool mine = cs[q] >= 0 && j <= d;
            s[q] = mine ? cs[q] * dp + j : -1;
            count[q] = j == d;                                          // the member count's slot
            v[q] = (mine && j < d) ? spts[(i + q) * d + j] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (s[q] >= 0) {
                if (count[q]) ((unsigned long long*)acc)[s[q]] += 1ull;
                else acc[s[q]] += v[q];
            }
    }
    for (; i < hi; ++i) {
        const int c = slab[i];                                      // the same for every thread of the group
        if (c < 0) continue;
        const int j = (o - c * dp) & (T - 1);
        if (j <= d) {
            const int s = c * dp + j;
            if (j < d) acc[s] += spts[i * d + j];
            else ((unsigned long long*)acc)[s] += 1ull;
        }
    }
    __syncthreads();
    // the sets in group order, ((g0 + g1) + g2) + g3; member counts as integers
    double* dst = part + (size_t)blockIdx.x * (nslot + 1);
    for (int s = tid; s < nslot; s += DFF_MICRO_THREADS) {
        double t = cen[s];
        unsigned long long ti = ((const unsigned long long*)cen)[s];
        for (int gg = 1; gg < groups; ++gg) {
            t += cen[gg * nset + s];
            ti += ((const unsigned long long*)cen)[gg * nset + s];
        }
        if ((s % dp) == d) ((unsigned long long*)dst)[s] = ti; else dst[s] = t;
    }
    if (tid == 0) dst[nslot] = ((winert[0] + winert[1]) + winert[2]) + winert[3];
}

// ---- rows of the workspace -> results (overwritten).  grid = ceil(per / 64), 256 threads.
__global__ __launch_bounds__(256) void dff_micro_kmeans_reduce_kernel(const double* __restrict__ part, long long nrows, int d,
                                                                      int K, double* __restrict__ sums,
                                                                      unsigned long long* __restrict__ counts,
                                                                      double* __restrict__ inertia) {
    __shared__ double red[4][64];
    const int dp = d + 1, nslot = K * dp, per = nslot + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * 64 + lane;
    const bool live = s < per;
    const bool is_count = live && s < nslot && (s % dp) == d;
    double acc = 0.0;
    unsigned long long cacc = 0ull;
    if (live)
        for (long long g = wave; g < nrows; g += 4) {
            const double v = part[(size_t)g * per + s];
            if (is_count) cacc += (unsigned long long)__double_as_longlong(v); else acc += v;
        }
    red[wave][lane] = is_count ? __longlong_as_double((long long)cacc) : acc;
    __syncthreads();
    if (wave == 0 && live) {
        if (is_count) {
            unsigned long long t = 0ull;
            for (int w = 0; w < 4; ++w) t += (unsigned long long)__double_as_longlong(red[w][lane]);
            if (counts) counts[s / dp] = t;
        } else {
            const double t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
            if (s == nslot) { if (inertia) inertia[0] = t; }
            else if (sums) sums[(s / dp) * d + (s % dp)] = t;
        }
    }
}

// ---- sliding-window transition counts of up to DFF_TC_MAXLAGS lags into counts (lags.n, K, K) in global memory.
__global__ __launch_bounds__(DFF_TC_THREADS) void dff_micro_tc_kernel(const int* __restrict__ labels, int K, TransRuns runs,
                                                                       TransLags lags,
                                                                       unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    for (long long base = runs.begin + (long long)blockIdx.x * DFF_TC_THREADS; base < runs.end;
         base += (long long)gridDim.x * DFF_TC_THREADS) {                 // uniform over the workgroup
        const long long t = base + threadIdx.x;
        int a = -1;
        long long e = 0;                                                   // one past the last frame of t's trajectory
        if (t < runs.end) {
            a = labels[t];
            if (runs.period > 0) e = runs.begin + ((t - runs.begin) / runs.period + 1) * runs.period;
            else e = runs.start[last_le(runs.start, runs.n, t) + 1];
        }
        const bool from = (unsigned)a < (unsigned)K;
        for (int l = 0; l < lags.n; ++l) {                                  // uniform
            int key = -1;
            if (from && t + lags.lag[l] < e) {
                const int b = labels[t + lags.lag[l]];
                if ((unsigned)b < (unsigned)K) key = (l * K + a) * K + b;  // < 8 * 2^20
            }
            bool pend = key >= 0;
            for (int r = 0; r < DFF_MICRO_TC_ROUNDS; ++r) {
                const unsigned long long m = __ballot(pend);
                if (!m) break;                                              // wave-uniform
                const int lead = __ffsll((long long)m) - 1;
                const int k0 = __shfl(key, lead);
                const bool same = pend && key == k0;
                const unsigned long long sm = __ballot(same);
                if (lane == lead) atomicAdd(&counts[k0], (unsigned long long)__popcll(sm));
                pend = pend && !same;
            }
            if (pend) atomicAdd(&counts[key], 1ull);
        }
    }
}

// ---- the reversible estimator's fixed-point sweeps: msm_q, msm_row and msm_finish of dff_msm_rows.h.  ONE set of kernels for
// one problem and for many per launch, templated on a problem locator `Loc`: loc.at(p) is problem p of the launch -- its
// index b and its number of states K; its matrix is slot b of loc.stride()^2 doubles of S, its vectors slot b of
// loc.stride() doubles of rowc, x and q, its err of sweep s at err[s * loc.err_stride() + b].
struct MsmAt {
    int b, K;
};

// one problem: no table, b = 0 -- every offset folds away when the kernel is compiled
struct MsmOne {
    int K;
    __device__ MsmAt at(unsigned) const { return {0, K}; }
    __host__ __device__ int stride() const { return K; }
    __host__ __device__ int err_stride() const { return 1; }
};

// grid (ceil(max K / blockDim.x), problems)
template <class Loc>
__global__ void dff_msm_init_kernel(const double* __restrict__ rowc, const double* __restrict__ x, Loc loc,
                                    double* __restrict__ q) {
    const MsmAt p = loc.at(blockIdx.y);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t o = (size_t)p.b * loc.stride();
    if (i < p.K) q[o + i] = msm_q(rowc[o + i], x[o + i]);
}

// one sweep, grid (ceil(max K / 4), problems): row i = 4 blockIdx.x + wave of problem blockIdx.y.  qin -> x (in place, by
// the row's own wave), qout.  err: this sweep's row of the err array
template <class Loc>
__global__ __launch_bounds__(DFF_MSM_THREADS) void dff_msm_sweep_kernel(const double* __restrict__ S,
                                                                        const double* __restrict__ rowc, Loc loc,
                                                                        double* __restrict__ x,
                                                                        const double* __restrict__ qin,
                                                                        double* __restrict__ qout,
                                                                        unsigned long long* __restrict__ err) {
    const MsmAt p = loc.at(blockIdx.y);
    const int K = p.K;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (DFF_MSM_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= K) return;                                             // wave-uniform
    const size_t o = (size_t)p.b * loc.stride();
    double xn = msm_row(S + o * loc.stride() + (size_t)i * K, qin + o, qin[o + i], K, lane);
    const double xo = x[o + i], ci = rowc[o + i];
    if (!(ci > 0.0 && xo > 0.0)) xn = __builtin_nan("");
    if (lane == 0) {
        x[o + i] = xn;
        qout[o + i] = msm_q(ci, xn);
        msm_finish(xn, xo, err ? err + p.b : nullptr);
    }
}

// all n_steps sweeps of problem blockIdx.x by one workgroup.  LDS: q ping | q pong | x (3 K doubles)
template <class Loc>
__global__ __launch_bounds__(DFF_MSM_LOOP_THREADS) void dff_msm_loop_kernel(const double* __restrict__ S,
                                                                            const double* __restrict__ rowc, Loc loc,
                                                                            double* __restrict__ x, int n_steps,
                                                                            unsigned long long* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) double mq[];
    const MsmAt p = loc.at(blockIdx.x);
    const int K = p.K;
    const size_t o = (size_t)p.b * loc.stride();
    S += o * loc.stride();
    rowc += o;
    x += o;
    double* qa = mq;
    double* qb = mq + K;
    double* xs = mq + 2 * K;
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
                msm_finish(xn, xo, err ? err + (size_t)s * loc.err_stride() + p.b : nullptr);
            }
        }
        __syncthreads();
        double* t = qa; qa = qb; qb = t;
    }
    for (int i = threadIdx.x; i < K; i += DFF_MSM_LOOP_THREADS) x[i] = xs[i];
}
