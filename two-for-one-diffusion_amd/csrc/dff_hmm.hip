// dff_hmm.hip -- one E-step of Baum-Welch for a discrete hidden Markov model over all chains of a labelled trajectory set:
// chunked forward-backward.  m <= DFF_HMM_MAXM hidden states, K <= DFF_MSM_MAXK symbols, fp64 throughout.  With
// M_t = A diag(B[:, o_t]) the forward recursion is alpha_t ~ alpha_{t-1} M_t and the backward one beta_{t-1} ~ M_t beta_t: products of
// the same matrices, so a chain is cut into chunks of DFF_HMM_CHUNK of its own (strided) frames and every chunk is independent
// work, whatever the number of trajectories.  Chain (r, f), f = 0 .. lag - 1: frames f, f + lag, ... of trajectory r; chains
// are ordered r-major, f-minor, the chunks chain after chain.  A negative label is a missing observation: emission factor 1.
//
// The hidden states are padded to MP = 2, 4 or 8 (hmm_pad(m)) with states that nothing reaches and that emit nothing: their
// entries are exact zeros, and adding +0 changes no bit.
//
// dff_hmm_prep_kernel      parameters -> the workspace: A (MP, MP), p0 (MP), B SYMBOL-MAJOR (K, MP) -- a frame's emission column
//     is one contiguous read of 8 MP bytes -- and the three flags (a non-finite or negative parameter; cleared: label >= K, a
//     vanished chain).
// dff_hmm_products_kernel  P = prod M_t over the chunk's frames, the chain's first frame left out.  Thread (chunk, row i): row i of
//     P in registers, all of A in registers; row <- (row A) b_t, every (row A)_j one chain of fused multiply-adds over k = 0 ..
//     MP - 1 from +0.  After every step the row is rescaled by the POWER OF TWO of its own sum (frexp / ldexp): the scaling is
//     exact, so the stored row is the unscaled row's bits with another exponent, and the "logarithm of the scale" is an integer.
//     A row whose sum is zero gets the exponent HMM_NOEXP.  One exponent per row instead of one scale per matrix costs the
//     carries one ldexp per row and the products no traffic between lanes.
// dff_hmm_carry_kernel     one THREAD per (chain, direction), serially over the chain's chunks: forward, alpha <- alpha P (the
//     rows' exponents applied relative to the largest one among the rows that alpha reaches, rescaled by the power of two of
//     its sum) -> the alpha ENTERING each chunk (that of the frame before its first), and the chain's log-likelihood =
//     ln(sum alpha_last) + ln 2 (sum of all exponents); backward, beta <- P beta -> the beta LEAVING each chunk (that of its last
//     frame).  The next chunk's P is fetched while this one's is used.
// dff_hmm_apply_kernel     MP lanes per chunk, one wave per workgroup.  Forward from the true alpha: lane j keeps column j of A,
//     u_t[j] = (sum_i u_{t-1}[i] A_ij) b_t[j] / sum(u_{t-1}); the u_t of the chunk stay in LDS.  Backward from the true beta: lane
//     j keeps row j of A; per frame gamma_t = u_t beta_t / G_t, G_t = sum_i u_t[i] beta_t[i], written to the posteriors, and
//     xi_t(i, j) = u_{t-1}[i] A_ij w_t[j] / G_{t-1} with w_t = b_t beta_t / sum(beta_t) and beta_{t-1} = A w_t -- G_{t-1} IS the sum of
//     the u_{t-1}[i] A_ij w_t[j], so xi_t is normalised by its own sum and no scale is carried between the passes.  Lane j adds
//     column j of the chunk's sum of xi_t, in the backward pass's order of frames.
// dff_hmm_emit_kernel      Gamma[i, s] = sum of gamma_t(i) over the frames with label s: one workgroup per group of
//     DFF_HMM_GROUP frames, accumulator (s, i) in LDS owned by thread (s m + i) mod 256 and added in frame order (the scheme
//     of dff_micro_kmeans_kernel); the group's partial goes to the workspace.
// dff_hmm_reduce_kernel    stats: the groups' partials in group order, the chunks' xi in chunk order, gamma0 over the chains'
//     first frames in chain order, the log-likelihood in chain order; one wave per output, 64 terms fetched at a time and
//     added one after the other.
// dff_hmm_finish_kernel    status from the flags; on a non-zero status every output becomes NaN.
// No floating-point atomics, no workgroup waits on another; every launch is sized by the host plan alone.
#pragma once
#include <hip/hip_runtime.h>

#ifndef DFF_HMM_CHUNK
#define DFF_HMM_CHUNK 128          // frames of a chain per chunk: measured among 64 / 128 / 256 / 512
#endif
#define DFF_HMM_GROUP 1024         // frames per workgroup of dff_hmm_emit_kernel
#define DFF_HMM_THREADS 256
#define DFF_HMM_MAXCHAINS (1 << 20)
#define HMM_NOEXP (-(1 << 28))     // the exponent of a row that vanished
#define HMM_LDS_BUDGET (72 * 1024) // LDS of one apply workgroup (one wave): two of them per CU

__host__ __device__ inline int hmm_pad(int m) { return m <= 2 ? 2 : (m <= 4 ? 4 : 8); }
// chunks of a chain of L frames
__host__ __device__ inline long long hmm_chunks_of(long long L) { return (L + DFF_HMM_CHUNK - 1) / DFF_HMM_CHUNK; }
// chunk groups (of MP lanes) per apply workgroup: as many as one wave has lanes for and the LDS budget holds
__host__ __device__ inline int hmm_apply_groups(int MP) {
    const int fit = HMM_LDS_BUDGET / ((DFF_HMM_CHUNK + 3) * MP * (int)sizeof(double));
    return fit < 64 / MP ? fit : 64 / MP;
}

// the trajectory table in the workspace: off[r] (n_traj + 1 frame offsets), then cpre[r] (n_traj + 1: chunks before trajectory r)
struct HmmPlan {
    const long long* off;
    const long long* cpre;
    int n_traj, lag;
};

struct HmmChain {
    long long first;      // global index of the chain's first frame
    long long L;          // frames
    long long c0;         // its first chunk
    long long nch;        // chunks
};

// a trajectory of len frames at a lag: its first rem chains hold q + 1 frames, the other lag - rem hold q
struct HmmSplit {
    long long q, rem;
};

__host__ __device__ __forceinline__ HmmSplit hmm_split(long long len, long long lag) {
    HmmSplit s;
    s.q = len / lag;
    s.rem = len - s.q * lag;
    return s;
}

// the frames [t0, t1) of its chain that chunk k holds, and ts, the first of them that is a factor: the chain's first frame is none
struct HmmSpan {
    long long t0, t1, ts;
};

__device__ __forceinline__ HmmSpan hmm_span(const HmmChain& ch, long long k) {
    HmmSpan s;
    s.t0 = k * DFF_HMM_CHUNK;
    s.t1 = ch.L - s.t0 < DFF_HMM_CHUNK ? ch.L : s.t0 + DFF_HMM_CHUNK;
    s.ts = s.t0 > 0 ? s.t0 : 1;
    return s;
}

// chain f of trajectory r
__device__ __forceinline__ HmmChain hmm_chain(const HmmPlan& pl, int r, int f) {
    const auto [q, rem] = hmm_split(pl.off[r + 1] - pl.off[r], pl.lag);
    const long long nA = hmm_chunks_of(q + 1), nB = hmm_chunks_of(q);
    HmmChain c;
    c.first = pl.off[r] + f;
    c.L = f < rem ? q + 1 : q;
    c.nch = f < rem ? nA : nB;
    c.c0 = pl.cpre[r] + (f < rem ? f * nA : rem * nA + (f - rem) * nB);
    return c;
}

// chunk c (< the plan's number of chunks) -> its chain (index r * lag + f) and its place k in it
__device__ __forceinline__ HmmChain hmm_locate(const HmmPlan& pl, long long c, long long& chain, long long& k) {
    int lo = 0, hi = pl.n_traj;                                     // the last r with cpre[r] <= c: cpre[0] = 0 <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pl.cpre[mid] <= c) lo = mid; else hi = mid;
    }
    const int r = lo;
    const auto [q, rem] = hmm_split(pl.off[r + 1] - pl.off[r], pl.lag);
    const long long nA = hmm_chunks_of(q + 1), nB = hmm_chunks_of(q);
    const long long cl = c - pl.cpre[r];
    int f;
    if (cl < rem * nA) { f = (int)(cl / nA); k = cl - f * nA; }
    else { const long long c2 = cl - rem * nA; f = (int)(rem + c2 / nB); k = c2 - (c2 / nB) * nB; }
    chain = (long long)r * pl.lag + f;
    return hmm_chain(pl, r, f);
}

__device__ __forceinline__ bool hmm_ok(double x) { return x >= 0.0 && x < __builtin_inf(); }

// v (> 0, finite) = f 2^e, 0.5 <= f < 1: e; anything else: 0
__device__ __forceinline__ int hmm_exp(double v) {
    int e = 0;
    if (v > 0.0 && v < __builtin_inf()) frexp(v, &e);
    return e;
}

__device__ __forceinline__ double hmm_scale(double v, int e) {      // v 2^e, e clamped to where the result is 0 anyway
    return ldexp(v, e < -4000 ? -4000 : (e > 4000 ? 4000 : e));
}

// ---- parameters into the workspace, flags
__global__ __launch_bounds__(1024) void dff_hmm_prep_kernel(const double* __restrict__ trans, const double* __restrict__ emit,
                                                            const double* __restrict__ init, int m, int K, int MP,
                                                            double* __restrict__ A, double* __restrict__ p0,
                                                            double* __restrict__ Bt, int* __restrict__ flags) {
    const int tid = threadIdx.x;
    int bad = 0;
    for (int idx = tid; idx < MP * MP; idx += 1024) {
        const int i = idx / MP, j = idx - i * MP;
        const double x = (i < m && j < m) ? trans[i * m + j] : 0.0;
        bad |= !hmm_ok(x);
        A[idx] = x;
    }
    for (int idx = tid; idx < MP; idx += 1024) {
        const double x = idx < m ? init[idx] : 0.0;
        bad |= !hmm_ok(x);
        p0[idx] = x;
    }
    for (int i = 0; i < MP; ++i)
        for (int s = tid; s < K; s += 1024) {
            const double x = i < m ? emit[(size_t)i * K + s] : 0.0;
            bad |= !hmm_ok(x);
            Bt[(size_t)s * MP + i] = x;
        }
    bad = __syncthreads_or(bad);
    if (tid == 0) { flags[0] = bad; flags[1] = 0; flags[2] = 0; flags[3] = 0; }
}

// the emission column of a label: B[:, lab], or ones (on the m real states) for a missing observation or a label >= K
template <int MP>
__device__ __forceinline__ void hmm_emission(const double* __restrict__ Bt, int lab, int K, int m, double (&b)[MP]) {
    if (lab >= 0 && lab < K) {
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = Bt[(size_t)lab * MP + j];
    } else {
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = j < m ? 1.0 : 0.0;
    }
}

// ---- chunk products: thread = (chunk, row)
template <int MP>
__global__ __launch_bounds__(DFF_HMM_THREADS) void dff_hmm_products_kernel(const int32_t* __restrict__ labels, HmmPlan pl,
                                                                           long long n_chunks, int m, int K,
                                                                           const double* __restrict__ A,
                                                                           const double* __restrict__ Bt,
                                                                           double* __restrict__ prod, int* __restrict__ pexp) {
    const long long gid = (long long)blockIdx.x * DFF_HMM_THREADS + threadIdx.x;
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
        for (int y = 0; y < MP; ++y) a[x][y] = A[x * MP + y];
    double row[MP];
#pragma unroll
    for (int j = 0; j < MP; ++j) row[j] = j == i ? 1.0 : 0.0;
    int e = 0;
    bool dead = false;
    const int32_t* lab = labels + ch.first;
    const long long lag = pl.lag;
    // the emission column is fetched one frame ahead, the label two
    double bn[MP];
    int l2 = -1;
    if (ts < t1) hmm_emission<MP>(Bt, lab[ts * lag], K, m, bn);
    if (ts + 1 < t1) l2 = lab[(ts + 1) * lag];
    for (long long t = ts; t < t1; ++t) {
        double b[MP];
#pragma unroll
        for (int j = 0; j < MP; ++j) b[j] = bn[j];
        if (t + 1 < t1) hmm_emission<MP>(Bt, l2, K, m, bn);
        if (t + 2 < t1) l2 = lab[(t + 2) * lag];
        double nw[MP];
#pragma unroll
        for (int j = 0; j < MP; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int x = 0; x < MP; ++x) acc = fma(row[x], a[x][j], acc);
            nw[j] = acc * b[j];
        }
        double s = nw[0];
#pragma unroll
        for (int j = 1; j < MP; ++j) s += nw[j];
        const int se = hmm_exp(s);
        dead |= !(s > 0.0 && s < __builtin_inf());
        e += se;
#pragma unroll
        for (int j = 0; j < MP; ++j) row[j] = ldexp(nw[j], -se);
    }
#pragma unroll
    for (int j = 0; j < MP; ++j) prod[((size_t)c * MP + i) * MP + j] = dead ? 0.0 : row[j];
    pexp[(size_t)c * MP + i] = dead ? HMM_NOEXP : e;
}

// ---- carries: thread = (chain, direction); blockIdx.y = 0 forward, 1 backward
template <int MP>
__device__ __forceinline__ void hmm_load_prod(const double* __restrict__ prod, const int* __restrict__ pexp, long long c,
                                              double (&P)[MP][MP], int (&pe)[MP]) {
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        pe[i] = pexp[(size_t)c * MP + i];
#pragma unroll
        for (int j = 0; j < MP; ++j) P[i][j] = prod[((size_t)c * MP + i) * MP + j];
    }
}

// alpha <- alpha P, rescaled by the power of two of its sum; returns the exponents taken out (HMM_NOEXP: it vanished)
template <int MP>
__device__ __forceinline__ int hmm_carry_forward(double (&v)[MP], const double (&P)[MP][MP], const int (&pe)[MP]) {
    int emax = HMM_NOEXP;
#pragma unroll
    for (int i = 0; i < MP; ++i)
        if (v[i] > 0.0 && pe[i] > emax) emax = pe[i];
    if (emax == HMM_NOEXP) {
#pragma unroll
        for (int j = 0; j < MP; ++j) v[j] = 0.0;
        return HMM_NOEXP;
    }
    double vs[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) vs[i] = pe[i] == HMM_NOEXP ? 0.0 : hmm_scale(v[i], pe[i] - emax);
    double nw[MP], s = 0.0;
#pragma unroll
    for (int j = 0; j < MP; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < MP; ++i) acc = fma(vs[i], P[i][j], acc);
        nw[j] = acc;
        s += acc;
    }
    if (!(s > 0.0 && s < __builtin_inf())) {
#pragma unroll
        for (int j = 0; j < MP; ++j) v[j] = 0.0;
        return HMM_NOEXP;
    }
    const int se = hmm_exp(s);
#pragma unroll
    for (int j = 0; j < MP; ++j) v[j] = ldexp(nw[j], -se);
    return emax + se;
}

// beta <- P beta, rescaled by the power of two of its sum
template <int MP>
__device__ __forceinline__ void hmm_carry_backward(double (&v)[MP], const double (&P)[MP][MP], const int (&pe)[MP]) {
    double y[MP];
    int emax = HMM_NOEXP;
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < MP; ++j) acc = fma(P[i][j], v[j], acc);
        y[i] = acc;
        if (acc > 0.0 && pe[i] > emax) emax = pe[i];
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        y[i] = (pe[i] == HMM_NOEXP || emax == HMM_NOEXP) ? 0.0 : hmm_scale(y[i], pe[i] - emax);
        s += y[i];
    }
    const int se = hmm_exp(s);
#pragma unroll
    for (int i = 0; i < MP; ++i) v[i] = ldexp(y[i], -se);
}

template <int MP>
__global__ __launch_bounds__(64) void dff_hmm_carry_kernel(const int32_t* __restrict__ labels, HmmPlan pl, long long n_chains,
                                                           int m, int K, const double* __restrict__ p0,
                                                           const double* __restrict__ Bt, const double* __restrict__ prod,
                                                           const int* __restrict__ pexp, double* __restrict__ ain,
                                                           double* __restrict__ bout, double* __restrict__ chain_ll,
                                                           int* __restrict__ flags) {
    const long long chain = (long long)blockIdx.x * 64 + threadIdx.x;
    if (chain >= n_chains) return;
    const int r = (int)(chain / pl.lag), f = (int)(chain - (long long)r * pl.lag);
    const HmmChain ch = hmm_chain(pl, r, f);
    const bool forward = blockIdx.y == 0;
    if (ch.L == 0) {
        if (forward) chain_ll[chain] = 0.0;
        return;
    }
    double v[MP], P[MP][MP], Q[MP][MP];
    int pe[MP], qe[MP];
    if (forward) {
        double b[MP];
        hmm_emission<MP>(Bt, labels[ch.first], K, m, b);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < MP; ++j) { v[j] = p0[j] * b[j]; s += v[j]; }
        long long E = 0;
        bool gone = !(s > 0.0 && s < __builtin_inf());
        if (!gone) {
            const int se = hmm_exp(s);
#pragma unroll
            for (int j = 0; j < MP; ++j) v[j] = ldexp(v[j], -se);
            E = se;
        }
        hmm_load_prod<MP>(prod, pexp, ch.c0, P, pe);
        for (long long k = 0; k < ch.nch; k += 2) {                  // two chunks per turn: P and Q swap roles, no copies
            if (k + 1 < ch.nch) hmm_load_prod<MP>(prod, pexp, ch.c0 + k + 1, Q, qe);
            if (k > 0)
#pragma unroll
                for (int j = 0; j < MP; ++j) ain[(size_t)(ch.c0 + k) * MP + j] = v[j];
            int de = hmm_carry_forward<MP>(v, P, pe);
            gone |= de == HMM_NOEXP;
            E += de;
            if (k + 1 < ch.nch) {
                if (k + 2 < ch.nch) hmm_load_prod<MP>(prod, pexp, ch.c0 + k + 2, P, pe);
#pragma unroll
                for (int j = 0; j < MP; ++j) ain[(size_t)(ch.c0 + k + 1) * MP + j] = v[j];
                de = hmm_carry_forward<MP>(v, Q, qe);
                gone |= de == HMM_NOEXP;
                E += de;
            }
        }
        double s1 = 0.0;
#pragma unroll
        for (int j = 0; j < MP; ++j) s1 += v[j];
        gone |= !(s1 > 0.0 && s1 < __builtin_inf());
        chain_ll[chain] = gone ? __builtin_nan("") : fma((double)E, 0.6931471805599453094, log(s1));
        if (gone) flags[2] = 1;
    } else {
#pragma unroll
        for (int j = 0; j < MP; ++j) v[j] = j < m ? 1.0 : 0.0;
        long long k = ch.nch - 1;                                    // bout[k] = beta of chunk k's last frame
        if (k > 0) hmm_load_prod<MP>(prod, pexp, ch.c0 + k, P, pe);
        for (; k >= 0; k -= 2) {
#pragma unroll
            for (int j = 0; j < MP; ++j) bout[(size_t)(ch.c0 + k) * MP + j] = v[j];
            if (k == 0) break;
            if (k - 1 > 0) hmm_load_prod<MP>(prod, pexp, ch.c0 + k - 1, Q, qe);
            hmm_carry_backward<MP>(v, P, pe);                       // through chunk k: the beta of chunk k - 1's last frame
#pragma unroll
            for (int j = 0; j < MP; ++j) bout[(size_t)(ch.c0 + k - 1) * MP + j] = v[j];
            if (k - 1 == 0) break;
            if (k - 2 > 0) hmm_load_prod<MP>(prod, pexp, ch.c0 + k - 2, P, pe);
            hmm_carry_backward<MP>(v, Q, qe);
        }
    }
}

// ---- apply: MP lanes per chunk, one wave per workgroup, G = hmm_apply_groups(MP) chunks per workgroup.
// LDS per group: u[(CHUNK + 1)][MP] (slot 0: the alpha entering, slot s + 1: frame s of the chunk) | xch[2][MP]
template <int MP>
__global__ __launch_bounds__(64) void dff_hmm_apply_kernel(const int32_t* __restrict__ labels, HmmPlan pl, long long n_chunks,
                                                           int m, int K, const double* __restrict__ A,
                                                           const double* __restrict__ p0, const double* __restrict__ Bt,
                                                           const double* __restrict__ ain, const double* __restrict__ bout,
                                                           double* __restrict__ post, double* __restrict__ xi_part,
                                                           int* __restrict__ flags) {
    constexpr int C = DFF_HMM_CHUNK, PER = (C + 3) * MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char hmm_lds[];
    const int G = hmm_apply_groups(MP);
    const int tid = threadIdx.x, g = tid / MP, j = tid - g * MP;
    const long long c = (long long)blockIdx.x * G + g;
    const bool own = g < G;                                         // lanes beyond the last group hold no LDS: they only keep the barriers
    const bool live = own && c < n_chunks;
    double* u = (double*)hmm_lds + (size_t)(own ? g : 0) * PER;
    double* xch = u + (C + 1) * MP;
    long long chain = 0, k = 0;
    HmmChain ch = {0, 0, 0, 0};
    if (live) ch = hmm_locate(pl, c, chain, k);
    const long long t0 = k * C;
    const int cnt = live ? (int)(ch.L - t0 < C ? ch.L - t0 : C) : 0;
    const long long lag = pl.lag;
    const int32_t* lab = labels + ch.first + t0 * lag;
    double acol[MP], arow[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) { acol[i] = A[i * MP + j]; arow[i] = A[j * MP + i]; }
    const double mine = j < m ? 1.0 : 0.0;
    int badlab = 0;
    // ---- forward
    if (live) u[j] = k > 0 ? ain[(size_t)c * MP + j] : 0.0;
    __syncthreads();
    for (int s = 0; s < C; ++s) {
        if (s < cnt) {
            const int l = lab[s * lag];
            badlab |= l >= K;
            const double bj = (l >= 0 && l < K) ? Bt[(size_t)l * MP + j] : mine;
            double un;
            if (k == 0 && s == 0) {
                un = p0[j] * bj;
            } else {
                double sum = 0.0, acc = 0.0;
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    const double x = u[s * MP + i];
                    sum += x;
                    acc = fma(x, acol[i], acc);
                }
                un = acc * bj / sum;
            }
            u[(s + 1) * MP + j] = un;
        }
        __syncthreads();
    }
    // ---- backward
    double beta = live ? (k + 1 < ch.nch ? bout[(size_t)c * MP + j] : mine) : 0.0;
    double wpend = 0.0, xi[MP];
    bool pending = false;
#pragma unroll
    for (int i = 0; i < MP; ++i) xi[i] = 0.0;
    for (int s = C - 1; s >= -1; --s) {
        double* x = xch + ((s + 1) & 1) * MP;
        if (own) x[j] = beta;
        __syncthreads();
        const bool frame = s >= 0 && s < cnt;                       // a frame of the chunk
        const bool entry = s == -1 && cnt > 0 && k > 0;             // the frame before it: only xi is owed there
        if (frame || entry) {
            double ut[MP], bt[MP], Gs = 0.0, sb = 0.0;
#pragma unroll
            for (int i = 0; i < MP; ++i) {
                ut[i] = u[(s + 1) * MP + i];
                bt[i] = x[i];
                Gs = fma(ut[i], bt[i], Gs);
                sb += bt[i];
            }
            if (frame && j < m) post[(size_t)(ch.first + (t0 + s) * lag) * m + j] = u[(s + 1) * MP + j] * beta / Gs;
            if (pending) {
                const double q = wpend / Gs;
#pragma unroll
                for (int i = 0; i < MP; ++i) xi[i] = fma(ut[i] * acol[i], q, xi[i]);
            }
            pending = false;
            if (frame && t0 + s >= 1) {                             // beta of the frame before, and the xi this frame owes
                const int l = lab[s * lag];
                double b[MP];
                hmm_emission<MP>(Bt, l, K, m, b);
                double nb = 0.0;
#pragma unroll
                for (int i = 0; i < MP; ++i) {
                    const double w = b[i] * bt[i] / sb;
                    nb = fma(arow[i], w, nb);
                    if (i == j) wpend = w;
                }
                beta = nb;
                pending = true;
            }
        }
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < MP; ++i) xi_part[((size_t)c * MP + i) * MP + j] = xi[i];
        if (badlab) flags[1] = 1;
    }
}

// ---- emission counts of one group of DFF_HMM_GROUP frames: part[group][s * m + i].  LDS: acc (K m) | gamma (GROUP m) | labels
__global__ __launch_bounds__(DFF_HMM_THREADS) void dff_hmm_emit_kernel(const int32_t* __restrict__ labels, long long n, int m,
                                                                       int K, const double* __restrict__ post,
                                                                       double* __restrict__ part) {
    constexpr int T = DFF_HMM_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char hmm_lds[];
    double* acc = (double*)hmm_lds;
    double* gam = acc + (size_t)K * m;
    int* lab = (int*)(gam + (size_t)DFF_HMM_GROUP * m);
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * DFF_HMM_GROUP;
    const int cnt = (int)(n - f0 < DFF_HMM_GROUP ? n - f0 : DFF_HMM_GROUP);
    for (int idx = tid; idx < K * m; idx += T) acc[idx] = 0.0;
    for (int idx = tid; idx < cnt * m; idx += T) gam[idx] = post[(size_t)f0 * m + idx];
    for (int idx = tid; idx < cnt; idx += T) lab[idx] = labels[f0 + idx];
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
        const int s = lab[t];
        if (s < 0 || s >= K) continue;                              // uniform over the workgroup
        const int i = (tid - s * m) & (T - 1);                      // slot s m + i is this thread's when i < m
        if (i < m) acc[s * m + i] += gam[t * m + i];
    }
    __syncthreads();
    double* out = part + (size_t)blockIdx.x * K * m;
    for (int idx = tid; idx < K * m; idx += T) out[idx] = acc[idx];
}

// ---- stats = loglik (1) | xi (m, m) | gamma0 (m) | gamma_sym (m, K).  One WAVE per output: its terms x_0, x_1, ... are added in
// that order -- the lanes fetch 64 consecutive terms at once, then every lane adds all 64 in index order (v_readlane: a term
// goes from its lane to all).  A term past the end, and gamma0's term of a chain without a frame, is +0: it changes no bit.
__device__ __forceinline__ double hmm_lane(double x, int l) {       // l: a constant
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

template <int MP>
__global__ __launch_bounds__(64) void dff_hmm_reduce_kernel(HmmPlan pl, long long n_chains, long long n_chunks, long long n_groups,
                                                            int m, int K, const double* __restrict__ chain_ll,
                                                            const double* __restrict__ xi_part, const double* __restrict__ post,
                                                            const double* __restrict__ part, double* __restrict__ stats) {
    const long long q = blockIdx.x;
    const int lane = threadIdx.x;
    int kind;                                                       // 0 loglik, 1 xi, 2 gamma0, 3 gamma_sym
    long long N;
    const double* p = nullptr;
    size_t stride = 0;
    int j = 0;
    if (q == 0) { kind = 0; N = n_chains; p = chain_ll; stride = 1; }
    else if (q < 1 + m * m) {
        const int i = (int)(q - 1) / m;
        j = (int)(q - 1) - i * m;
        kind = 1; N = n_chunks; p = xi_part + (size_t)i * MP + j; stride = (size_t)MP * MP;
    } else if (q < 1 + m * m + m) { kind = 2; N = n_chains; j = (int)(q - 1 - m * m); }
    else {
        const long long e = q - 1 - m * m - m;
        const int i = (int)(e / K), s = (int)(e - (long long)i * K);
        kind = 3; N = n_groups; p = part + (size_t)s * m + i; stride = (size_t)K * m;
    }
    double v = 0.0;
    for (long long base = 0; base < N; base += 64) {
        const long long idx = base + lane;
        double x = 0.0;
        if (idx < N) {
            if (kind == 2) {
                const int r = (int)(idx / pl.lag), f = (int)(idx - (long long)r * pl.lag);
                if (f < pl.off[r + 1] - pl.off[r]) x = post[(size_t)(pl.off[r] + f) * m + j];
            } else {
                x = p[(size_t)idx * stride];
            }
        }
#pragma unroll
        for (int l = 0; l < 64; ++l) v += hmm_lane(x, l);
    }
    if (lane == 0) stats[q] = v;
}

// the status of a call from its flags: 1 a bad parameter, 3 a label >= K, 2 a chain that vanished, in that order of precedence
__device__ __forceinline__ int hmm_status(const int* __restrict__ flags) {
    return flags[0] ? 1 : (flags[1] ? 3 : (flags[2] ? 2 : 0));
}

// ---- status; NaN over every output when it is not 0
__global__ __launch_bounds__(DFF_HMM_THREADS) void dff_hmm_finish_kernel(const int* __restrict__ flags, long long nstats,
                                                                         double* __restrict__ stats, long long n_chains,
                                                                         double* __restrict__ chain_ll, long long npost,
                                                                         double* __restrict__ post, int* __restrict__ status) {
    const int st = hmm_status(flags);
    const long long q = (long long)blockIdx.x * DFF_HMM_THREADS + threadIdx.x;
    if (q == 0) *status = st;
    if (st == 0) return;
    const double nan = __builtin_nan("");
    const long long stride = (long long)gridDim.x * DFF_HMM_THREADS;
    for (long long idx = q; idx < nstats; idx += stride) stats[idx] = nan;
    if (chain_ll)
        for (long long idx = q; idx < n_chains; idx += stride) chain_ll[idx] = nan;
    if (post)
        for (long long idx = q; idx < npost; idx += stride) post[idx] = nan;
}
