// dff_hmm_viterbi.hip -- the most probable hidden path (Viterbi) of every chain of a labelled trajectory set under a discrete
// hidden Markov model: a chunked max-plus scan.  Chains, chunks and the plan are those of dff_hmm.hip (HmmPlan, hmm_chain,
// hmm_locate, hmm_pad, DFF_HMM_CHUNK): chain (r, f) holds the frames f, f + lag, ... of trajectory r, chains are r-major, f-minor,
// a chunk holds DFF_HMM_CHUNK of a chain's own frames.  Everything is fp64 and in the LOG domain: la (m, m) = ln A, lb (m, K) =
// ln B, lp (m) = ln p0 come from the caller, -inf is an impossible transition / emission.  le_t = lb[:, o_t], or zeros for a negative
// label (a missing observation).  The device only adds, compares and selects: no log, no exp, no product (so nothing to fuse), no
// floating-point atomics.  A max is exact, so only the order of the ADDITIONS matters for the bits; it is stated at every kernel.
//
// The hidden states are padded to MP = 2, 4 or 8 (hmm_pad(m)) with states whose la rows and columns and whose lp are -inf: their
// delta is -inf at every frame, and since every argmax takes the LOWEST index attaining the max, a padding state (index >= m) never
// wins ahead of a real one.  Their emission entries are +0.
//
// dff_vit_prep_kernel       block 0: la (MP, MP), lp (MP), lb SYMBOL-MAJOR (K, MP) into the workspace, flag 0 = a NaN or +inf
//     parameter; all blocks: flag 1 = a label >= K (the flags are cleared by the host part before this launch).
// dff_vit_products_kernel   thread (chunk, row i): P starts as the max-plus identity (0 on the diagonal, -inf elsewhere); for every
//     frame t of the chunk, the chain's first frame left out, P'(i, j) = (max_k (P(i, k) + la[k][j])) + le_t(j).  No rescaling:
//     the values stay near n |log|.
// dff_vit_forward_kernel    one thread per chain, serially over its chunks: din(first chunk) = lp + le_0, din(next) = dout,
//     dout(j) = max_i (din(i) + P(i, j)); every chunk's din is stored.  The next chunk's P is fetched while this one's is used.
// dff_vit_apply_kernel      MP lanes per chunk; lane j keeps column j of la and delta(j), delta is exchanged by __shfl inside the
//     group.  From the chunk's din, for every frame t of the chunk (the chain's first frame left out):
//     delta'(j) = (max_i (delta(i) + la[i][j])) + le_t(j), psi_t(j) = the lowest i attaining the max; the MP back-pointers of a frame
//     pack into one 32-bit word (3 bits each, state j at bits 3 j ..), stored at the frame's CHAIN-ORDER position (chains back to
//     back).  The chunk's back map is carried along: origin'(j) = origin(psi_t(j)) from the identity; at the end it names, for
//     every end state j, the state at the previous chunk's last frame (packed the same way).  A chain's last chunk stores the
//     lowest argmax of its final delta and the max itself: the chain's log-probability (-inf: flag 2).
// dff_vit_backward_kernel   one thread per chain, serially from its last chunk: end(c - 1) = origin_c(end(c)); every chunk's end
//     state is stored.  The origin words are fetched eight chunks at a time.
// dff_vit_backtrack_kernel  one thread per chunk, from end(c) back through the chunk's psi words; the path is written in frame
//     order or in chain order.
// dff_vit_finish_kernel     status from the flags; on a non-zero status every path entry becomes -1, every chain_logprob NaN.
// No workgroup waits on another; every launch is sized by the host plan alone.  Every index that is read from the workspace is a
// 3-bit field (0 .. 7 < 8 = the largest MP) shifted by at most 21 bits, whatever the parameters: nothing read there addresses
// memory outside the word it came from.
#pragma once
#include "dff_hmm.hip"

#define DFF_VIT_THREADS 256

// the chain-order position of the first frame of chain f of trajectory r: the chains of a trajectory lie back to back
__device__ __forceinline__ long long vit_chain_start(const HmmPlan& pl, int r, int f) {
    const auto [q, rem] = hmm_split(pl.off[r + 1] - pl.off[r], pl.lag);
    return pl.off[r] + (f < rem ? f * (q + 1) : rem * (q + 1) + (f - rem) * q);
}

__device__ __forceinline__ bool vit_bad(double x) { return !(x < __builtin_inf()); }      // NaN or +inf

// ---- parameters into the workspace, flags
__global__ __launch_bounds__(1024) void dff_vit_prep_kernel(const int32_t* __restrict__ labels, long long n,
                                                            const double* __restrict__ ltrans, const double* __restrict__ lemit,
                                                            const double* __restrict__ linit, int m, int K, int MP,
                                                            double* __restrict__ la, double* __restrict__ lp,
                                                            double* __restrict__ lbt, int* __restrict__ flags) {
    const int tid = threadIdx.x;
    const double ninf = -__builtin_inf();
    if (blockIdx.x == 0) {
        int bad = 0;
        for (int idx = tid; idx < MP * MP; idx += 1024) {
            const int i = idx / MP, j = idx - i * MP;
            const double x = (i < m && j < m) ? ltrans[i * m + j] : ninf;
            bad |= vit_bad(x);
            la[idx] = x;
        }
        for (int idx = tid; idx < MP; idx += 1024) {
            const double x = idx < m ? linit[idx] : ninf;
            bad |= vit_bad(x);
            lp[idx] = x;
        }
        for (int i = 0; i < MP; ++i)
            for (int s = tid; s < K; s += 1024) {
                const double x = i < m ? lemit[(size_t)i * K + s] : 0.0;
                bad |= vit_bad(x);
                lbt[(size_t)s * MP + i] = x;
            }
        bad = __syncthreads_or(bad);
        if (tid == 0 && bad) flags[0] = 1;
    }
    int over = 0;
    const long long stride = (long long)gridDim.x * 1024;
    for (long long t = (long long)blockIdx.x * 1024 + tid; t < n; t += stride) over |= labels[t] >= K;
    over = __syncthreads_or(over);
    if (tid == 0 && over) flags[1] = 1;
}

// the log-emission column of a label: lb[:, lab], or zeros for a missing observation or a label >= K
template <int MP>
__device__ __forceinline__ void vit_emission(const double* __restrict__ lbt, int lab, int K, double (&b)[MP]) {
    if (lab >= 0 && lab < K) {
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = lbt[(size_t)lab * MP + j];
    } else {
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = 0.0;
    }
}

// ---- chunk products: thread = (chunk, row)
template <int MP>
__global__ __launch_bounds__(DFF_VIT_THREADS) void dff_vit_products_kernel(const int32_t* __restrict__ labels, HmmPlan pl,
                                                                           long long n_chunks, int K,
                                                                           const double* __restrict__ la,
                                                                           const double* __restrict__ lbt,
                                                                           double* __restrict__ prod) {
    const long long gid = (long long)blockIdx.x * DFF_VIT_THREADS + threadIdx.x;
    const long long c = gid / MP;
    const int i = (int)(gid - c * MP);
    if (c >= n_chunks) return;
    long long chain, k;
    const HmmChain ch = hmm_locate(pl, c, chain, k);
    const auto [t0, t1, ts] = hmm_span(ch, k);
    double a[MP][MP];
#pragma unroll
    for (int x = 0; x < MP; ++x)
#pragma unroll
        for (int y = 0; y < MP; ++y) a[x][y] = la[x * MP + y];
    double row[MP];
#pragma unroll
    for (int j = 0; j < MP; ++j) row[j] = j == i ? 0.0 : -__builtin_inf();
    const int32_t* lab = labels + ch.first;
    const long long lag = pl.lag;
    // the emission column is fetched one frame ahead, the label two
    double bn[MP];
    int l2 = -1;
    if (ts < t1) vit_emission<MP>(lbt, lab[ts * lag], K, bn);
    if (ts + 1 < t1) l2 = lab[(ts + 1) * lag];
    for (long long t = ts; t < t1; ++t) {
        double b[MP];
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = bn[j];
        if (t + 1 < t1) vit_emission<MP>(lbt, l2, K, bn);
        if (t + 2 < t1) l2 = lab[(t + 2) * lag];
        double nw[MP];
#pragma unroll
        for (int j = 0; j < MP; ++j) {
            double best = row[0] + a[0][j];
#pragma unroll
            for (int x = 1; x < MP; ++x) {
                const double v = row[x] + a[x][j];
                best = v > best ? v : best;
            }
            nw[j] = best + b[j];
        }
#pragma unroll
        for (int j = 0; j < MP; ++j) row[j] = nw[j];
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) prod[((size_t)c * MP + i) * MP + j] = row[j];
}

// ---- forward carries: thread = chain
template <int MP>
__device__ __forceinline__ void vit_load_prod(const double* __restrict__ prod, long long c, double (&P)[MP][MP]) {
#pragma unroll
    for (int i = 0; i < MP; ++i)
#pragma unroll
        for (int j = 0; j < MP; ++j) P[i][j] = prod[((size_t)c * MP + i) * MP + j];
}

template <int MP>
__global__ __launch_bounds__(64) void dff_vit_forward_kernel(const int32_t* __restrict__ labels, HmmPlan pl, long long n_chains,
                                                             int K, const double* __restrict__ lp,
                                                             const double* __restrict__ lbt, const double* __restrict__ prod,
                                                             double* __restrict__ din, double* __restrict__ chain_lp) {
    const long long chain = (long long)blockIdx.x * 64 + threadIdx.x;
    if (chain >= n_chains) return;
    const int r = (int)(chain / pl.lag), f = (int)(chain - (long long)r * pl.lag);
    const HmmChain ch = hmm_chain(pl, r, f);
    if (ch.L == 0) {
        chain_lp[chain] = 0.0;
        return;
    }
    double v[MP], P[MP][MP], Q[MP][MP];
    double b[MP];
    vit_emission<MP>(lbt, labels[ch.first], K, b);
#pragma unroll
    for (int j = 0; j < MP; ++j) v[j] = lp[j] + b[j];
    vit_load_prod<MP>(prod, ch.c0, P);
    for (long long k = 0; k < ch.nch; ++k) {
        if (k + 1 < ch.nch) vit_load_prod<MP>(prod, ch.c0 + k + 1, Q);
#pragma unroll
        for (int j = 0; j < MP; ++j) din[(size_t)(ch.c0 + k) * MP + j] = v[j];
        double nw[MP];
#pragma unroll
        for (int j = 0; j < MP; ++j) {
            double best = v[0] + P[0][j];
#pragma unroll
            for (int i = 1; i < MP; ++i) {
                const double x = v[i] + P[i][j];
                best = x > best ? x : best;
            }
            nw[j] = best;
        }
#pragma unroll
        for (int j = 0; j < MP; ++j) v[j] = nw[j];
        if (k + 1 < ch.nch) {
#pragma unroll
            for (int i = 0; i < MP; ++i)
#pragma unroll
                for (int j = 0; j < MP; ++j) P[i][j] = Q[i][j];
        }
    }
}

// ---- apply: MP lanes per chunk
template <int MP>
__device__ __forceinline__ unsigned vit_pack(int value, int j) {    // the group's values, 3 bits each, in every lane of the group
    unsigned w = (unsigned)value << (3 * j);
#pragma unroll
    for (int d = 1; d < MP; d <<= 1) w |= (unsigned)__shfl_xor((int)w, d, MP);
    return w;
}

template <int MP>
__global__ __launch_bounds__(DFF_VIT_THREADS) void dff_vit_apply_kernel(const int32_t* __restrict__ labels, HmmPlan pl,
                                                                        long long n_chunks, int K, const double* __restrict__ la,
                                                                        const double* __restrict__ lbt,
                                                                        const double* __restrict__ din,
                                                                        unsigned* __restrict__ psi, unsigned* __restrict__ origin,
                                                                        int* __restrict__ endstate, double* __restrict__ chain_lp,
                                                                        int* __restrict__ flags) {
    constexpr int C = DFF_HMM_CHUNK;
    const long long gid = (long long)blockIdx.x * DFF_VIT_THREADS + threadIdx.x;
    const long long c = gid / MP;
    const int j = (int)(gid - c * MP);
    if (c >= n_chunks) return;                                      // whole groups leave together: a group is MP consecutive lanes
    long long chain, k;
    const HmmChain ch = hmm_locate(pl, c, chain, k);
    const int r = (int)(chain / pl.lag), f = (int)(chain - (long long)r * pl.lag);
    const long long pos0 = vit_chain_start(pl, r, f);
    const auto [t0, t1, ts] = hmm_span(ch, k);
    const long long lag = pl.lag;
    const int32_t* lab = labels + ch.first;
    double acol[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) acol[i] = la[i * MP + j];
    double d = din[(size_t)c * MP + j];
    int org = j;
    // the emission is fetched one frame ahead, the label two
    double len = 0.0;
    int l2 = -1;
    if (ts < t1) { const int l = lab[ts * lag]; len = (l >= 0 && l < K) ? lbt[(size_t)l * MP + j] : 0.0; }
    if (ts + 1 < t1) l2 = lab[(ts + 1) * lag];
    for (long long t = ts; t < t1; ++t) {
        const double le = len;
        if (t + 1 < t1) len = (l2 >= 0 && l2 < K) ? lbt[(size_t)l2 * MP + j] : 0.0;
        if (t + 2 < t1) l2 = lab[(t + 2) * lag];
        double best = __shfl(d, 0, MP) + acol[0];
        int arg = 0;
#pragma unroll
        for (int i = 1; i < MP; ++i) {
            const double x = __shfl(d, i, MP) + acol[i];
            if (x > best) { best = x; arg = i; }                    // strictly greater: the lowest index keeps a tie
        }
        d = best + le;
        org = __shfl(org, arg, MP);
        const unsigned w = vit_pack<MP>(arg, j);
        if (j == 0) psi[pos0 + t] = w;
    }
    const unsigned ow = vit_pack<MP>(org, j);
    if (j == 0) origin[c] = ow;
    if (k + 1 == ch.nch) {                                          // the chain's last chunk: its end state and log-probability
        double best = __shfl(d, 0, MP);
        int arg = 0;
#pragma unroll
        for (int i = 1; i < MP; ++i) {
            const double x = __shfl(d, i, MP);
            if (x > best) { best = x; arg = i; }
        }
        if (j == 0) {
            endstate[chain] = arg;
            chain_lp[chain] = best;
            if (best == -__builtin_inf()) flags[2] = 1;
        }
    }
}

// ---- backward carries: thread = chain; end[c] = the state at chunk c's last frame
__global__ __launch_bounds__(64) void dff_vit_backward_kernel(HmmPlan pl, long long n_chains, const unsigned* __restrict__ origin,
                                                              const int* __restrict__ endstate, int* __restrict__ end) {
    const long long chain = (long long)blockIdx.x * 64 + threadIdx.x;
    if (chain >= n_chains) return;
    const int r = (int)(chain / pl.lag), f = (int)(chain - (long long)r * pl.lag);
    const HmmChain ch = hmm_chain(pl, r, f);
    if (ch.L == 0) return;
    int s = endstate[chain] & 7;
    for (long long k = ch.nch - 1; k >= 0; k -= 8) {                // chunks k, k - 1, ..., k - 7
        unsigned w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = k - u >= 0 ? origin[ch.c0 + k - u] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k - u >= 0) {
                end[ch.c0 + k - u] = s;
                s = (int)((w[u] >> (3 * s)) & 7u);                  // the state at chunk k - u - 1's last frame
            }
    }
}

// ---- backtrack: thread = chunk
__global__ __launch_bounds__(DFF_VIT_THREADS) void dff_vit_backtrack_kernel(HmmPlan pl, long long n_chunks,
                                                                            const unsigned* __restrict__ psi,
                                                                            const int* __restrict__ end, int chain_order,
                                                                            int32_t* __restrict__ path) {
    const long long c = (long long)blockIdx.x * DFF_VIT_THREADS + threadIdx.x;
    if (c >= n_chunks) return;
    long long chain, k;
    const HmmChain ch = hmm_locate(pl, c, chain, k);
    const int r = (int)(chain / pl.lag), f = (int)(chain - (long long)r * pl.lag);
    const long long pos0 = vit_chain_start(pl, r, f);
    const auto [t0, t1, ts] = hmm_span(ch, k);
    const long long base = chain_order ? pos0 : ch.first, step = chain_order ? 1 : pl.lag;
    int s = end[c] & 7;
    for (long long t = t1 - 1; t >= t0; --t) {
        path[base + t * step] = s;
        if (t > t0) s = (int)((psi[pos0 + t] >> (3 * s)) & 7u);     // t > t0 >= 0: a word that the apply pass of this chunk wrote
    }
}

// ---- status; -1 over the path and NaN over the log-probabilities when it is not 0
__global__ __launch_bounds__(DFF_VIT_THREADS) void dff_vit_finish_kernel(const int* __restrict__ flags, long long n,
                                                                         int32_t* __restrict__ path, long long n_chains,
                                                                         double* __restrict__ chain_lp, int* __restrict__ status) {
    const int st = hmm_status(flags);
    const long long q = (long long)blockIdx.x * DFF_VIT_THREADS + threadIdx.x;
    if (q == 0) *status = st;
    if (st == 0) return;
    const double nan = __builtin_nan("");
    const long long stride = (long long)gridDim.x * DFF_VIT_THREADS;
    for (long long idx = q; idx < n; idx += stride) path[idx] = -1;
    if (chain_lp)
        for (long long idx = q; idx < n_chains; idx += stride) chain_lp[idx] = nan;
}
