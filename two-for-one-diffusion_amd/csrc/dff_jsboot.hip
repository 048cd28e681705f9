// dff_jsboot.hip -- what a block bootstrap of a Jensen-Shannon metric between histograms needs: the histogram of every
// resampling unit, once, and then for B weighted resamples x C channels the resampled histogram REDUCED to its JS against the
// reference histogram without ever being written out.  A histogram is additive over frames: resample b's is
// sum_u w[b][u] hist[u], so no frame is looked at twice.
//
// dff_unit_hist_kernel          one work item per (unit, channel, tile of DFF_JSB_TILE_BINS bins), walked by a grid-stride loop:
//     the unit's frames are counted into an LDS tile with 32-bit integer LDS atomics and the tile is stored (not added) to
//     hist[u][c][k0 ..].  An item owns its slice of the output, so no global atomic and no order: exact.  The channels of a frame
//     lie side by side, so a workgroup reads one int of every C: wide-channel inputs (many pairs) are read through L2 many
//     times; the bootstrap's PWD route does not come here (dff_pwd_hist per unit), one- and few-channel grids do.
// dff_jsb_unit_totals_kernel    utot[u][c] = sum_k hist[u][c][k], one wave per row: the per-(b, c) totals follow from these, so
//     the JS kernel needs one pass over the bins.
// dff_jsb_ref_kernel            refsum[c] = sum_k ref[c][k] in one fixed order, or NaN when the channel cannot be scored (a
//     negative or non-finite entry, a sum that is 0 or not finite).
// dff_resampled_js_kernel<TB>   one workgroup per (channel, tile of TB resamples), threads along the bins: thread t holds bins
//     k = t, t + 256, ... and for each of them TB 64-bit accumulators h[i] += w[b0 + i][u] * hist[u][c][k] over the units -- one
//     coalesced 4-byte load of hist per (u, k) and TB 32 x 32 -> 64 multiply-adds, the tile's weights broadcast from LDS
//     (DFF_JSB_UCHUNK units at a time).  With tot[b] = sum_u w[b][u] utot[u][c] known beforehand, the bin's two terms
//     p ln(p / m) + q ln(q / m) are added to the thread's sum at once and h is dropped.  A thread adds its bins in ascending
//     order, the 64 lanes of a wave by a butterfly, the four waves as (0 + 1) + (2 + 3): the order depends on nbins[c] alone,
//     not on TB, B or the resample's place in the batch, and the integer sums are exact -- every TB gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#define DFF_JSB_THREADS 256
#define DFF_JSB_TILE_BINS 8192           // bins per LDS tile of dff_unit_hist (32 KB)
#define DFF_JSB_MAXUNITS 65536
#define DFF_JSB_MAXCHANNELS (1 << 18)      // 8 ceil(C / 8) ceil(B / tile) workgroups stay below 2^31
#define DFF_JSB_MAXLD (1 << 20)
#define DFF_JSB_MAXCELLS (1LL << 32)     // U C ld
#define DFF_JSB_MAXB 4096
#define DFF_JSB_UCHUNK 1024              // units whose weights are in LDS at a time (32 KB at 8 resamples)
#define DFF_JSB_MAXTILE 8                // resamples per workgroup, at most
#define DFF_JSB_AHEAD 4                  // units whose hist loads are issued together
#define DFF_JSB_WANT_WGS 512             // the tile shrinks until a call has this many workgroups (two per CU)

// ---- per-unit histograms.  ustart (U + 1): ascending frame indices from 0 to n; nbins (C) as 64-bit words.
__global__ __launch_bounds__(DFF_JSB_THREADS) void dff_unit_hist_kernel(const int* __restrict__ bins, int C,
                                                                         const long long* __restrict__ ustart,
                                                                         const long long* __restrict__ nbins, int ld, int tiles,
                                                                         long long items, unsigned* __restrict__ hist) {
    __shared__ unsigned cnt[DFF_JSB_TILE_BINS];
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {      // uniform over the workgroup
        const int tile = (int)(item % tiles);
        const long long uc = item / tiles;
        const int c = (int)(uc % C);
        const long long u = uc / C;
        const int nb = (int)nbins[c];
        const int k0 = tile * DFF_JSB_TILE_BINS;
        const long long t0 = ustart[u], t1 = ustart[u + 1];
        if (k0 >= nb || t0 == t1) continue;                                    // the output was zeroed
        const unsigned kn = (unsigned)(nb - k0 < DFF_JSB_TILE_BINS ? nb - k0 : DFF_JSB_TILE_BINS);
        for (unsigned k = threadIdx.x; k < kn; k += DFF_JSB_THREADS) cnt[k] = 0;
        __syncthreads();
        for (long long t = t0 + threadIdx.x; t < t1; t += DFF_JSB_THREADS) {
            // unsigned wrap: a negative index, one below k0 and one from nbins[c] on all land at or above kn
            const unsigned b = (unsigned)bins[t * C + c] - (unsigned)k0;
            if (b < kn) atomicAdd(&cnt[b], 1u);
        }
        __syncthreads();
        unsigned* __restrict__ row = hist + (size_t)uc * ld + k0;
        for (unsigned k = threadIdx.x; k < kn; k += DFF_JSB_THREADS) row[k] = cnt[k];
        __syncthreads();
    }
}

// ---- utot[r] = sum of row r of hist (rows = U C, nbins of channel r % C), one wave per row
__global__ __launch_bounds__(DFF_JSB_THREADS) void dff_jsb_unit_totals_kernel(const unsigned* __restrict__ hist, long long rows,
                                                                               int C, int ld, const long long* __restrict__ nbins,
                                                                               unsigned long long* __restrict__ utot) {
    const int lane = threadIdx.x & 63;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * 4) {
        const int nb = (int)nbins[r % C];
        const unsigned* __restrict__ row = hist + (size_t)r * ld;
        unsigned long long s = 0;
        for (int k = lane; k < nb; k += 64) s += row[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) utot[r] = s;
    }
}

// the workgroup's sum of v in one order: the lanes of a wave by a butterfly, the waves as (0 + 1) + (2 + 3); red: 4 doubles
__device__ __forceinline__ double jsb_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return v;
}

// ---- refsum[c]: the sum of the channel's reference histogram, NaN when the channel cannot be scored
__global__ __launch_bounds__(DFF_JSB_THREADS) void dff_jsb_ref_kernel(const double* __restrict__ ref, int ld,
                                                                       const long long* __restrict__ nbins,
                                                                       double* __restrict__ refsum) {
    __shared__ double red[4];
    __shared__ int bad;
    const int c = blockIdx.x;
    const int nb = (int)nbins[c];
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const double* __restrict__ row = ref + (size_t)c * ld;
    double s = 0.0;
    bool mine = false;
    for (int k = threadIdx.x; k < nb; k += DFF_JSB_THREADS) {
        const double r = row[k];
        mine = mine || !(r >= 0.0) || !(r - r == 0.0);                         // negative, NaN or an infinity
        s += r;
    }
    if (mine) bad = 1;                                                         // every writer writes 1
    s = jsb_block_sum(s, red);                                                 // its barriers order `bad` too
    if (threadIdx.x == 0) refsum[c] = (bad || !(s > 0.0) || !(s - s == 0.0)) ? __builtin_nan("") : s;
}

// ---- the JS of TB resamples of one channel per workgroup: grid ceil(B / TB) x C workgroups (C rounded up to 8 from 8 channels on)
template <int TB>
__global__ __launch_bounds__(DFF_JSB_THREADS) void dff_resampled_js_kernel(const unsigned* __restrict__ hist, int U, int C, int ld,
                                                                            const long long* __restrict__ nbins,
                                                                            const unsigned* __restrict__ weights, int B,
                                                                            const double* __restrict__ ref,
                                                                            const unsigned long long* __restrict__ utot,
                                                                            const double* __restrict__ refsum,
                                                                            double* __restrict__ js,
                                                                            unsigned long long* __restrict__ total) {
    __shared__ unsigned wl[DFF_JSB_UCHUNK * TB];                               // [unit in chunk][resample in tile]
    __shared__ unsigned long long totw[4][TB];
    __shared__ double red[4];
    // the workgroups of one channel read the same U x nbins[c] slab of hist once per resample tile: keep them on ONE XCD and next
    // to each other in dispatch order, so that the slab is served by that XCD's L2 (workgroup id % 8 says which blocks share an
    // XCD; speed only).  Channel c goes to group c % 8, its resample tiles are consecutive there; with fewer than 8 channels
    // every XCD takes tiles of the same channel instead.
    const int nbt = (B + TB - 1) / TB;
    int c, bt;
    if (C >= 8) {
        const unsigned slot = blockIdx.x >> 3;
        c = (int)(slot / nbt) * 8 + (int)(blockIdx.x & 7);
        bt = (int)(slot % nbt);
        if (c >= C) return;                                                    // uniform: the padding of the last group of 8
    } else {
        c = (int)(blockIdx.x / nbt);
        bt = (int)(blockIdx.x % nbt);
    }
    const int b0 = bt * TB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = (int)nbins[c];
    const double rs = refsum[c];

    // tot[i] = sum_u w[b0 + i][u] utot[u][c]: integers, any order
    unsigned long long tot[TB];
#pragma unroll
    for (int i = 0; i < TB; ++i) tot[i] = 0;
    for (int u = tid; u < U; u += DFF_JSB_THREADS) {
        const unsigned long long ut = utot[(size_t)u * C + c];
#pragma unroll
        for (int i = 0; i < TB; ++i)
            if (b0 + i < B) tot[i] += (unsigned long long)weights[(size_t)(b0 + i) * U + u] * ut;
    }
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        for (int o = 32; o > 0; o >>= 1) tot[i] += __shfl_xor(tot[i], o);
        if (lane == 0) totw[wave][i] = tot[i];
    }
    __syncthreads();
    double rtot[TB];
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        tot[i] = totw[0][i] + totw[1][i] + totw[2][i] + totw[3][i];
        rtot[i] = (double)tot[i];
    }

    double acc[TB];
#pragma unroll
    for (int i = 0; i < TB; ++i) acc[i] = 0.0;
    const size_t ustride = (size_t)C * ld;
    for (int k0 = 0; k0 < nb; k0 += DFF_JSB_THREADS) {                         // uniform
        const int k = k0 + tid;
        const bool active = k < nb;
        unsigned long long h[TB];
#pragma unroll
        for (int i = 0; i < TB; ++i) h[i] = 0;
        for (int u0 = 0; u0 < U; u0 += DFF_JSB_UCHUNK) {                       // uniform
            const int un = U - u0 < DFF_JSB_UCHUNK ? U - u0 : DFF_JSB_UCHUNK;
            if (U > DFF_JSB_UCHUNK || k0 == 0) {                               // all units fit: staged once
                __syncthreads();
#pragma unroll
                for (int i = 0; i < TB; ++i)
                    for (int ul = tid; ul < un; ul += DFF_JSB_THREADS)
                        wl[ul * TB + i] = b0 + i < B ? weights[(size_t)(b0 + i) * U + u0 + ul] : 0u;
                __syncthreads();
            }
            if (active) {
                const unsigned* __restrict__ hp = hist + ((size_t)u0 * C + c) * ld + k;
                int ul = 0;
                for (; ul + DFF_JSB_AHEAD <= un; ul += DFF_JSB_AHEAD) {        // the loads of DFF_JSB_AHEAD units in flight before the first use
                    unsigned hv[DFF_JSB_AHEAD];
#pragma unroll
                    for (int j = 0; j < DFF_JSB_AHEAD; ++j) hv[j] = hp[(size_t)(ul + j) * ustride];
#pragma unroll
                    for (int j = 0; j < DFF_JSB_AHEAD; ++j)
#pragma unroll
                        for (int i = 0; i < TB; ++i) h[i] += (unsigned long long)wl[(ul + j) * TB + i] * hv[j];
                }
                for (; ul < un; ++ul) {
                    const unsigned hv = hp[(size_t)ul * ustride];
#pragma unroll
                    for (int i = 0; i < TB; ++i) h[i] += (unsigned long long)wl[ul * TB + i] * hv;
                }
            }
        }
        if (active) {
            const double q = ref[(size_t)c * ld + k] / rs + 1e-10;
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                const double p = (double)h[i] / rtot[i] + 1e-10;
                const double m = (p + q) / 2;
                acc[i] += p * log(p / m) + q * log(q / m);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TB; ++i) {
        const double v = jsb_block_sum(acc[i], red);
        if (tid == 0 && b0 + i < B) {
            js[(size_t)(b0 + i) * C + c] = (tot[i] == 0 || rs != rs) ? __builtin_nan("") : 0.5 * v;
            if (total) total[(size_t)(b0 + i) * C + c] = tot[i];
        }
    }
}
