// dff_autocorr.hip -- lagged products of a scalar or few-component observable inside trajectories: the sums behind the
// autocorrelation function, the integrated autocorrelation time and the effective sample size (evaluate.py: autocorrelation).
//
// For every lag l = 0 .. max_lag, over the pairs (t, t + l) of one trajectory whose two frames are usable (all d components
// finite), with g = series - shift in fp64:   count[l] = #pairs,  sx = sum g_t,  sy = sum g_{t+l},  sxy = sum g_t g_{t+l}.
// An unusable frame is staged as g = 0 with validity v = 0, a usable one with v = 1, so the four sums are the products
//     sxy = sum g_t g_{t+l}    sx = sum g_t v_{t+l}    sy = sum v_t g_{t+l}    count = sum v_t v_{t+l}
// over the pairs inside a trajectory, and the only test in the loop is the trajectory boundary.
//
// dff_ac_left_kernel     left[t] = frames from t to the end of its trajectory (>= 1), from the run tables of
//     dff_transition_counts (TransRuns: up to DFF_TC_RUNS unequal trajectories per launch, or any number of equal ones).
//     The pair (t, t + l) lies inside a trajectory exactly when l < left[t]: one compare per lag.
// dff_ac_pairs_kernel    256 threads; workgroup (slot, lag chunk, component).  A chunk is DFF_AC_CHUNK = 512 lags: lane k of
//     every wave owns the DFF_AC_R = 8 consecutive lags l0 + 8 k .. l0 + 8 k + 7.  A tile is DFF_AC_TILE = 512 start frames,
//     128 per wave; g and v of the start frames, and of the DFF_AC_WIN = 512 + 512 + 8 window frames t0 + l0 ... that hold their
//     partners, are staged in LDS as fp64, for the workgroup's component.  Per start frame a lane reads g_t and v_t (one address for the wave: broadcast) and ONE new
//     element of its sliding register windows of g and v, then does 8 x 4 fp64 FMAs.  Frame i of the window lies at
//     (i mod 8) * DFF_AC_ROW + i / 8, so the lanes' new elements -- frame indices 8 apart -- are consecutive doubles: a
//     stride-1 8-byte read, conflict-free.  A tile whose start frames all have left > the chunk's last lag skips the
//     boundary compare; a tile none of whose start frames reaches the chunk's first lag is skipped before it is staged.
//     A workgroup walks the tiles slot, slot + slots, ... with its sums in registers; at the end the four waves' sums are
//     added in wave order through LDS and written to the workgroup's own cells of the workspace: every cell is written.
// dff_ac_reduce_kernel   sixteen threads per (sum, lag): each adds every sixteenth slot's partial in slot order, then the sixteen
//     are added in thread order.  No floating-point atomics; the order of every addition follows from (n, d, max_lag)
//     alone, so the results are bit-identical from call to call.
#pragma once
#include "dff_traj.h"   // TransRuns, last_le

#define DFF_AC_THREADS 256
#define DFF_AC_MAXD 8
#define DFF_AC_MAXLAG 65535
#define DFF_AC_R 8                                                  // consecutive lags per lane
#define DFF_AC_CHUNK (64 * DFF_AC_R)                                // lags per workgroup
#define DFF_AC_TILE 512                                             // start frames per tile
#define DFF_AC_SUB (DFF_AC_TILE / (DFF_AC_THREADS / 64))            // ... per wave
#define DFF_AC_WIN (DFF_AC_TILE + DFF_AC_CHUNK + DFF_AC_R)          // frames staged per tile
#define DFF_AC_ROW (DFF_AC_WIN / DFF_AC_R)
#ifndef DFF_AC_WAVES
#define DFF_AC_WAVES 2                                              // waves per SIMD the pair kernel is compiled for
#endif
#define DFF_AC_WGS 2048                                             // workgroups aimed at: slots = DFF_AC_WGS / (chunks * d)
static_assert(DFF_AC_R == 8 && DFF_AC_SUB % DFF_AC_R == 0 && DFF_AC_WIN % DFF_AC_R == 0, "the window layout assumes 8 lags per lane");

__device__ __forceinline__ int ac_phys(int i) { return (i & (DFF_AC_R - 1)) * DFF_AC_ROW + (i >> 3); }

__global__ __launch_bounds__(DFF_AC_THREADS) void dff_ac_left_kernel(TransRuns runs, int* __restrict__ left) {
    for (long long t = runs.begin + (long long)blockIdx.x * DFF_AC_THREADS + threadIdx.x; t < runs.end;
         t += (long long)gridDim.x * DFF_AC_THREADS) {
        long long e;                                                // one past the last frame of t's trajectory
        if (runs.period > 0) e = runs.begin + ((t - runs.begin) / runs.period + 1) * runs.period;
        else e = runs.start[last_le(runs.start, runs.n, t) + 1];
        left[t] = e - t > 0x7fffffffLL ? 0x7fffffff : (int)(e - t);
    }
}

// the start frames tb0 .. tb0 + DFF_AC_SUB - 1 of a staged tile against the lane's lags L .. L + 7
template <bool FULL, bool COUNT, bool MASK>
__device__ __forceinline__ void ac_tile(const double* __restrict__ sa, const double* __restrict__ sva,
                                        const double* __restrict__ sg, const double* __restrict__ sv,
                                        const int* __restrict__ sleft, int tb0, int lane, int L, double (&axy)[DFF_AC_R],
                                        double (&ax)[DFF_AC_R], double (&ay)[DFF_AC_R], double (&an)[DFF_AC_R]) {
    double w[DFF_AC_R], vw[DFF_AC_R];
#pragma unroll
    for (int k = 0; k < DFF_AC_R; ++k) {                            // window frames tb0 + 8 lane + k: tb0 is a multiple of 8
        w[k] = sg[k * DFF_AC_ROW + (tb0 >> 3) + lane];
        vw[k] = sv[k * DFF_AC_ROW + (tb0 >> 3) + lane];
    }
    // g_t, v_t and left[t] are fetched one start frame ahead; the scheduling barrier keeps the compiler from hoisting the
    // LDS reads of all eight unrolled start frames to the top (264 VGPRs, one wave per SIMD, without it)
    double a = sa[tb0], vt = sva[tb0];
    int lf = MASK ? sleft[tb0] : 0;
    for (int tb = tb0; tb < tb0 + DFF_AC_SUB; tb += DFF_AC_R) {
#pragma unroll
        for (int j = 0; j < DFF_AC_R; ++j) {
            // start frame t = tb + j; sa, sva and sleft have one entry past the tile
            const double a_next = sa[tb + j + 1], vt_next = sva[tb + j + 1];
            const int lf_next = MASK ? sleft[tb + j + 1] : 0;
#pragma unroll
            for (int r = 0; r < DFF_AC_R; ++r) {
                const double wv = w[(j + r) & (DFF_AC_R - 1)], vv = vw[(j + r) & (DFF_AC_R - 1)];
                double am = a, vm = vt;
                if (MASK) {
                    const bool in = L + r < lf;
                    am = in ? a : 0.0;
                    vm = in ? vt : 0.0;
                }
                axy[r] = fma(am, wv, axy[r]);
                if (FULL) {
                    ax[r] = fma(am, vv, ax[r]);
                    ay[r] = fma(vm, wv, ay[r]);
                }
                if (COUNT) an[r] = fma(vm, vv, an[r]);
            }
            // window frame t + 8 lane + 8 replaces t + 8 lane, which no later start frame needs
            w[j] = sg[j * DFF_AC_ROW + (tb >> 3) + 1 + lane];
            vw[j] = sv[j * DFF_AC_ROW + (tb >> 3) + 1 + lane];
            a = a_next;
            vt = vt_next;
            lf = lf_next;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// part: (slots, K, max_lag + 1) doubles, K = 3 d + 1 with FULL (sxy | sx | sy of the d components, then the count), else d
template <bool FULL>
__global__ __launch_bounds__(DFF_AC_THREADS, DFF_AC_WAVES) void dff_ac_pairs_kernel(const double* __restrict__ series, long long n,
                                                                          int d, int max_lag,
                                                                          const double* __restrict__ shift,
                                                                          const int* __restrict__ left, long long ntiles,
                                                                          double* __restrict__ part) {
    __shared__ double sa[DFF_AC_TILE + 1], sva[DFF_AC_TILE + 1], sg[DFF_AC_WIN], sv[DFF_AC_WIN];
    __shared__ double red[(DFF_AC_THREADS / 64) * DFF_AC_CHUNK];
    __shared__ int sleft[DFF_AC_TILE + 1], wflag[2 * (DFF_AC_THREADS / 64)];
    const int slot = blockIdx.x, slots = gridDim.x, l0 = blockIdx.y * DFF_AC_CHUNK, c = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = l0 + lane * DFF_AC_R;
    const int lmax = l0 + DFF_AC_CHUNK - 1 < max_lag ? l0 + DFF_AC_CHUNK - 1 : max_lag;
    const bool count = FULL && c == 0;                              // the count comes from the workgroups of component 0
    const double sh = shift ? shift[c] : 0.0;
    double axy[DFF_AC_R] = {}, ax[DFF_AC_R] = {}, ay[DFF_AC_R] = {}, an[DFF_AC_R] = {};
    for (long long tile = slot; tile < ntiles; tile += slots) {     // uniform over the workgroup: the loop has barriers
        const long long t0 = tile * DFF_AC_TILE;
        __syncthreads();                                            // the previous tile has been read
        bool all_in = true, any_in = false;
        if (threadIdx.x == 0) {
            sleft[DFF_AC_TILE] = 0;
            sa[DFF_AC_TILE] = 0.0;
            sva[DFF_AC_TILE] = 0.0;
        }
        for (int i = threadIdx.x; i < DFF_AC_TILE; i += DFF_AC_THREADS) {
            const int lf = t0 + i < n ? left[t0 + i] : 0;
            sleft[i] = lf;
            all_in = all_in && lf > lmax;
            any_in = any_in || lf > l0;
        }
        all_in = __all(all_in) != 0;
        any_in = __any(any_in) != 0;
        if (lane == 0) {
            wflag[2 * wave] = all_in;
            wflag[2 * wave + 1] = any_in;
        }
        __syncthreads();
        all_in = wflag[0] && wflag[2] && wflag[4] && wflag[6];
        any_in = wflag[1] || wflag[3] || wflag[5] || wflag[7];
        if (!any_in) continue;                                      // no pair of this tile reaches the chunk's first lag
        // g and v of frame f: zeros for an unusable frame and past the series
        auto stage = [&](long long f, double& g, double& v) {
            g = 0.0;
            v = 0.0;
            if (f < n) {
                bool ok = true;
                double mine = 0.0;
                for (int k = 0; k < d; ++k) {
                    const double x = series[f * d + k];
                    ok = ok && isfinite(x);
                    if (k == c) mine = x;
                }
                if (ok) {
                    g = mine - sh;
                    v = 1.0;
                }
            }
        };
        for (int i = threadIdx.x; i < DFF_AC_TILE; i += DFF_AC_THREADS) stage(t0 + i, sa[i], sva[i]);
        for (int i = threadIdx.x; i < DFF_AC_WIN; i += DFF_AC_THREADS)       // the partners: window frame i is t0 + l0 + i
            stage(t0 + l0 + i, sg[ac_phys(i)], sv[ac_phys(i)]);
        __syncthreads();
        const int tb0 = wave * DFF_AC_SUB;
        if (all_in) {
            if (count) ac_tile<FULL, true, false>(sa, sva, sg, sv, sleft, tb0, lane, L, axy, ax, ay, an);
            else ac_tile<FULL, false, false>(sa, sva, sg, sv, sleft, tb0, lane, L, axy, ax, ay, an);
        } else {
            if (count) ac_tile<FULL, true, true>(sa, sva, sg, sv, sleft, tb0, lane, L, axy, ax, ay, an);
            else ac_tile<FULL, false, true>(sa, sva, sg, sv, sleft, tb0, lane, L, axy, ax, ay, an);
        }
    }
    // the waves' sums in wave order, one kind after the other
    const int nlags = max_lag + 1, K = FULL ? 3 * d + 1 : d;
    auto flush = [&](const double (&acc)[DFF_AC_R], int k) {
        __syncthreads();                                            // `red` is free (and the last tile has been read)
#pragma unroll
        for (int r = 0; r < DFF_AC_R; ++r) red[wave * DFF_AC_CHUNK + lane * DFF_AC_R + r] = acc[r];
        __syncthreads();
        for (int q = threadIdx.x; q < DFF_AC_CHUNK; q += DFF_AC_THREADS)
            if (l0 + q <= max_lag)
                part[((long long)slot * K + k) * nlags + l0 + q] =
                    ((red[q] + red[DFF_AC_CHUNK + q]) + red[2 * DFF_AC_CHUNK + q]) + red[3 * DFF_AC_CHUNK + q];
    };
    flush(axy, c);
    if (FULL) {
        flush(ax, d + c);
        flush(ay, 2 * d + c);
        if (count) flush(an, 3 * d);                                // uniform over the workgroup
    }
}

// 16 consecutive (sum, lag) cells per workgroup, 16 threads per cell: thread g adds the slots g, g + 16, ... in that order (the
// loads of 8 slots in flight at once), then the 16 partial sums are added in the order of g.
__global__ __launch_bounds__(DFF_AC_THREADS) void dff_ac_reduce_kernel(const double* __restrict__ part, int slots, int d,
                                                                        int nlags, int K, double* __restrict__ sxy,
                                                                        double* __restrict__ sx, double* __restrict__ sy,
                                                                        unsigned long long* __restrict__ count) {
    __shared__ double acc[16][17];
    const int cell = threadIdx.x & 15, g = threadIdx.x >> 4;
    const long long idx = (long long)blockIdx.x * 16 + cell, cells = (long long)K * nlags;
    double s = 0.0;
    if (idx < cells) {
#pragma unroll 8
        for (int p = g; p < slots; p += 16) s += part[(long long)p * cells + idx];
    }
    acc[g][cell] = s;
    __syncthreads();
    if (g != 0 || idx >= cells) return;
    s = acc[0][cell];
#pragma unroll
    for (int k = 1; k < 16; ++k) s += acc[k][cell];
    const int k = (int)(idx / nlags), lag = (int)(idx % nlags);
    const int kind = k / d, c = k % d;
    if (kind == 0) sxy[(long long)lag * d + c] = s;
    else if (kind == 1) { if (sx) sx[(long long)lag * d + c] = s; }
    else if (kind == 2) { if (sy) sy[(long long)lag * d + c] = s; }
    else if (count) count[lag] = (unsigned long long)s;             // a sum of 0 / 1 products: an exact integer below 2^53
}
