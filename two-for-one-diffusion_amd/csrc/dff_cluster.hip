// dff_cluster.hip -- clustering of one ensemble under the minimum RMSD with a cutoff (Daura et al. 1999, the method of
// `gmx cluster -method gromos`): the neighbour matrix of the ensemble against itself as ONE BIT per pair
// (dff_rmsd_neighbors) and the greedy loop on that matrix (dff_gromos_steps).
//
// Bit matrix.  n rows of W = ceil(n / 64) uint64_t words; bit r & 63 of word s * W + (r >> 6) says that frames s and r
//   are neighbours.  The kernels address it as 2 W 32-bit half-words per row (little endian: bit r & 31 of half-word
//   r >> 5 is the same bit), because one workgroup holds 32 candidates.
//
// Neighbours.  The value of a pair is the one dff_ens_rmsd_kernel<false> (dff_ensemble.hip) writes with the LOWER index as
//   the query: the same centring expressions, bead b in k-step b / 4, slot b % 4, the same calls horn_key ->
//   sym4_jacobi<false> -> kabsch_rmsd on the same operands.  Only pairs s < r are computed; the pair (r, s) gets the same
//   bit, so the matrix is symmetric by construction.  The diagonal bit of a finite frame is set by definition.
//   Workgroup (ct, qs) holds candidate tile ct (32 frames) in LDS and takes the 16-query tiles qt <= 2 ct + 1 (those
//   with a query below the tile's last candidate), DFF_CLU_QPW per wave.  A lane tests its four pairs of a 16 x 16 MFMA
//   tile; a wave ballot per result register turns them into row bits (bits 16 kq .. 16 kq + 15 of the ballot are the 16
//   candidates of query row kq + 4 r), two sub-tiles make the 32-bit half-word of (query, candidate tile).
//     qt < 2 ct     every candidate of the tile is above every query: the half-word is complete in the wave and goes out
//                   with one plain store; no other wave writes it.
//     qt >= 2 ct    the 32 x 32 block on the diagonal: it is shared by two query tiles and receives its own transposed
//                   bits, so both directions go out with atomicOr.
//   The transposed bits of a 16-query tile are 16 consecutive bits of ONE half-word of every candidate's row (16 | q0):
//   the four lanes of a candidate column combine their 4-bit pieces with two shuffles and one lane issues one atomicOr.
//   The matrix is zeroed first (hipMemsetAsync on the caller's stream): the half-words below the diagonal only ever
//   receive ORs.  An OR of integers does not depend on the order of its operands: the matrix is the same for every run.
//
// Greedy loop.  State: `alive` (W words) and one 64-bit key in the caller's workspace.  One iteration is two launches,
//   ordered by the kernel boundary -- no workgroup ever waits on another:
//     count   one wave per alive row: popcount(row & alive), key = degree << 32 | ~index, atomicMax on the key: the
//             largest degree and, among equal degrees, the lowest index (a maximum of integers: order-independent)
//     apply   one workgroup: the centre's alive neighbours get the label, leave `alive`; the key is reset.  Largest
//             degree 1: every alive frame becomes a singleton in ascending index order (a scan over the words' popcounts).
//   Degrees are RECOUNTED every iteration (DESIGN.md section 14 says why not decremented edge by edge).
#pragma once
#include "dff_ensemble.hip"

#define DFF_CLU_MAX_N (1LL << 18)   // frames: 2^36 bits = 8 GiB
#define DFF_CLU_QPW 8               // 16-query tiles per wave and workgroup: a workgroup pairs its 32 candidates with 512 queries
#define DFF_CLU_GROUP (4 * DFF_CLU_QPW)
#define DFF_CLU_APPLY_THREADS 256

__host__ __device__ __forceinline__ long long clu_words(long long n) { return (n + 63) >> 6; }

// grid (nct, ceil(nqt / DFF_CLU_GROUP)): workgroup (ct, qs) pairs candidate tile ct with the query tiles
// qs * DFF_CLU_GROUP + wave + 4 k, k < DFF_CLU_QPW, that are <= 2 ct + 1; workgroups without one leave at once.
__global__ __launch_bounds__(DFF_ENS_THREADS) void dff_clu_neighbors_kernel(const float* __restrict__ x, long long n, int N,
                                                                            float cutoff, unsigned* __restrict__ adj) {
    const long long ct = blockIdx.x;
    const long long nqt = (n + DFF_ENS_TQ - 1) / DFF_ENS_TQ;
    const long long qt_end = 2 * ct + 2 < nqt ? 2 * ct + 2 : nqt;      // query tiles of this candidate tile
    const long long qt_first = (long long)blockIdx.y * DFF_CLU_GROUP;
    if (qt_first >= qt_end) return;
    extern __shared__ __attribute__((aligned(16))) double ens_lds[];
    const int Np = ens_np(N), N3 = 3 * N, KS = Np >> 2;
    double* yc = ens_lds;
    double* cen = ens_lds + DFF_ENS_TC * 3 * Np;
    double* GbL = cen + 3 * DFF_ENS_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long c0 = ct * DFF_ENS_TC;
    const int cc = (int)(n - c0 < DFF_ENS_TC ? n - c0 : DFF_ENS_TC);
    const long long W2 = 2 * clu_words(n);                             // half-words per row

    // ---- the candidate tile: centres, centred image, Gb (the statements of dff_ens_rmsd_kernel)
    if (tid < 3 * DFF_ENS_TC) {
        const int f = tid & (DFF_ENS_TC - 1), c = tid / DFF_ENS_TC;
        double s = 0.0;
        if (f < cc) {
            const float* p = x + (c0 + f) * N3 + c;
            for (int b = 0; b < N; ++b) s += p[3 * b];
            s /= N;
        }
        cen[c * DFF_ENS_TC + f] = s;
    }
    __syncthreads();
    for (int e = tid; e < DFF_ENS_TC * 3 * Np; e += DFF_ENS_THREADS) {
        const int fi = e & 15, rest = e >> 4;
        const int bead = rest % Np, sc = rest / Np, c = sc % 3, sub = sc / 3;
        const int f = sub * 16 + fi;
        const double m0 = cen[f], m1 = cen[DFF_ENS_TC + f], m2 = cen[2 * DFF_ENS_TC + f];
        double v = 0.0;
        if (f < cc && bead < N && isfinite(m0) && isfinite(m1) && isfinite(m2))
            v = (double)x[(c0 + f) * N3 + 3 * bead + c] - (c == 0 ? m0 : c == 1 ? m1 : m2);
        yc[e] = v;
    }
    __syncthreads();
    if (tid < DFF_ENS_TC) {
        const int f = tid, sub = f >> 4, fi = f & 15;
        const bool ok = f < cc && isfinite(cen[f]) && isfinite(cen[DFF_ENS_TC + f]) && isfinite(cen[2 * DFF_ENS_TC + f]);
        const double* p = yc + sub * 3 * 16 * Np + fi;
        double G = 0.0;
        for (int b = 0; b < N; ++b) {
            const double a0 = p[16 * b], a1 = p[16 * (Np + b)], a2 = p[16 * (2 * Np + b)];
            G = fma(a0, a0, fma(a1, a1, fma(a2, a2, G)));
        }
        GbL[f] = ok ? G : __builtin_nan("");
    }
    __syncthreads();

    // ---- query tiles
    const int qi = lane & 15, kq = lane >> 4;
    for (int k = 0; k < DFF_CLU_QPW; ++k) {
        const long long qt = qt_first + wave + 4 * k;
        if (qt >= qt_end) break;                                       // wave-uniform
        const bool diag = qt >= 2 * ct;                                // the tile holds pairs with query >= candidate
        const long long q0 = qt * DFF_ENS_TQ;
        const int qc = (int)(n - q0 < DFF_ENS_TQ ? n - q0 : DFF_ENS_TQ);
        const float* xq = x + (q0 + qi) * N3;                          // frame lane & 15 (dereferenced only when qi < qc)
        double s = 0.0;
        if (lane < 48 && qi < qc) {
            for (int b = 0; b < N; ++b) s += xq[3 * b + kq];
            s /= N;
        }
        const double ca0 = __shfl(s, qi), ca1 = __shfl(s, qi + 16), ca2 = __shfl(s, qi + 32);
        const bool qfin = qi < qc && isfinite(ca0) && isfinite(ca1) && isfinite(ca2);
        double Ga = __builtin_nan("");
        if (qfin) {
            Ga = 0.0;
            for (int b = 0; b < N; ++b) {
                const double a0 = xq[3 * b] - ca0, a1 = xq[3 * b + 1] - ca1, a2 = xq[3 * b + 2] - ca2;
                Ga = fma(a0, a0, fma(a1, a1, fma(a2, a2, Ga)));
            }
        }
        double GaR[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) GaR[r] = __shfl(Ga, kq + 4 * r);   // the query of this lane's result row r
        unsigned rowbits[4] = {0u, 0u, 0u, 0u};                        // half-word of query row kq + 4 r, complete after both sub-tiles
        for (int sub = 0; sub * 16 < cc; ++sub) {
            f64x4 S[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) S[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
            const double* yb = yc + sub * 3 * 16 * Np + lane;
            for (int ks = 0; ks < KS; ++ks) {
                const int bead = 4 * ks + kq;
                double av[3] = {0.0, 0.0, 0.0};
                if (qfin && bead < N) {
                    av[0] = (double)xq[3 * bead] - ca0;
                    av[1] = (double)xq[3 * bead + 1] - ca1;
                    av[2] = (double)xq[3 * bead + 2] - ca2;
                }
                double bv[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) bv[c] = yb[c * 16 * Np + 64 * ks];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], S[a][b], 0, 0, 0);
            }
            const int col = sub * 16 + qi;                             // result column lane & 15: the candidate
            const double Gb = GbL[col];
            const long long cand = c0 + col;
            unsigned colbits = 0u;                                     // this lane's queries that are neighbours of `cand`, bit = row
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq + 4 * r;                            // result row: the query
                const long long q = q0 + row;
                const bool fin = GaR[r] == GaR[r] && Gb == Gb && row < qc && col < cc;
                bool hit = false;
                if (fin && q < cand) {
                    const Sym4 K = horn_key(S[0][0][r], S[0][1][r], S[0][2][r], S[1][0][r], S[1][1][r], S[1][2][r], S[2][0][r],
                                            S[2][1][r], S[2][2][r]);
                    const float d = kabsch_rmsd(GaR[r], Gb, sym4_jacobi<false>(K), N);
                    hit = d <= cutoff;
                }
                if (hit) colbits |= 1u << row;
                const unsigned long long b = __ballot(hit || (fin && q == cand));   // the diagonal bit: by definition
                rowbits[r] |= (unsigned)((b >> (16 * kq)) & 0xffffu) << (16 * sub);
            }
            colbits |= __shfl_xor(colbits, 16);
            colbits |= __shfl_xor(colbits, 32);
            // row `cand`, half-word q0 >> 5, bits (q0 & 16) ..: never a half-word that a plain store writes
            if (kq == 0 && colbits) atomicOr(&adj[cand * W2 + (q0 >> 5)], colbits << (int)(q0 & 16));
        }
        if (qi == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq + 4 * r;
                if (row < qc) {
                    unsigned* p = &adj[(q0 + row) * W2 + ct];
                    if (!diag) *p = rowbits[r];
                    else if (rowbits[r]) atomicOr(p, rowbits[r]);
                }
            }
        }
    }
}

// degree[s] = popcount of row s: one wave per row
__global__ __launch_bounds__(256) void dff_clu_degree_kernel(const unsigned long long* __restrict__ adj, long long n,
                                                             int* __restrict__ degree) {
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n) return;
    const int lane = threadIdx.x & 63;
    const long long W = clu_words(n);
    int cnt = 0;
    for (long long w = lane; w < W; w += 64) cnt += __popcll(adj[s * W + w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) degree[s] = cnt;
}

// ---- the greedy loop
// workspace: alive (W words) | key (one word).  progress = {clusters so far, finite frames not yet in a cluster}

// restart: labels = -1, centers = -1, sizes = 0, alive = the diagonal bits, key = 0; progress[1] += the diagonal bits
// (progress is zeroed by a memset before the launch; an integer sum)
__global__ __launch_bounds__(256) void dff_clu_init_kernel(const unsigned long long* __restrict__ adj, long long n,
                                                           int max_clusters, int* __restrict__ labels, int* __restrict__ centers,
                                                           int* __restrict__ sizes, int* __restrict__ progress,
                                                           unsigned long long* __restrict__ alive,
                                                           unsigned long long* __restrict__ key) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long W = clu_words(n);
    bool on = false;
    if (s < n) {
        labels[s] = -1;
        on = (adj[s * W + (s >> 6)] >> (s & 63)) & 1ULL;
    }
    if (s < max_clusters) {
        centers[s] = -1;
        sizes[s] = 0;
    }
    const unsigned long long b = __ballot(on);                          // wave = 64 consecutive frames = one word
    if ((threadIdx.x & 63) == 0 && s < n) {
        alive[s >> 6] = b;
        if (b) atomicAdd(&progress[1], __popcll(b));
    }
    if (s == 0) *key = 0ULL;
}

__device__ __forceinline__ bool clu_done(const int* progress, int max_clusters) {
    return progress[1] <= 0 || progress[0] >= max_clusters;
}

// count: key = max over alive rows s of (popcount(row s & alive) << 32 | ~s)
__global__ __launch_bounds__(256) void dff_clu_count_kernel(const unsigned long long* __restrict__ adj, long long n,
                                                            int max_clusters, const int* __restrict__ progress,
                                                            const unsigned long long* __restrict__ alive,
                                                            unsigned long long* __restrict__ key) {
    if (clu_done(progress, max_clusters)) return;
    __shared__ unsigned long long wk[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * 4 + wave;
    const long long W = clu_words(n);
    unsigned long long k = 0ULL;
    if (s < n && ((alive[s >> 6] >> (s & 63)) & 1ULL)) {
        int cnt = 0;
        for (long long w = lane; w < W; w += 64) cnt += __popcll(adj[s * W + w] & alive[w]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        k = ((unsigned long long)(unsigned)cnt << 32) | (0xffffffffu - (unsigned)s);
    }
    if (lane == 0) wk[wave] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) k = wk[i] > k ? wk[i] : k;
        if (k) atomicMax(key, k);
    }
}

// apply: one workgroup.  The key names the centre; degree 1 = nothing but singletons is left.
__global__ __launch_bounds__(DFF_CLU_APPLY_THREADS) void dff_clu_apply_kernel(const unsigned long long* __restrict__ adj,
                                                                              long long n, int max_clusters,
                                                                              int* __restrict__ labels, int* __restrict__ centers,
                                                                              int* __restrict__ sizes, int* __restrict__ progress,
                                                                              unsigned long long* __restrict__ alive,
                                                                              unsigned long long* __restrict__ key) {
    __shared__ int part[DFF_CLU_APPLY_THREADS];
    const int tid = threadIdx.x;
    const int k0 = progress[0], left = progress[1];
    const unsigned long long best = *key;
    __syncthreads();                                                    // everybody has read progress and the key
    if (left <= 0 || k0 >= max_clusters || best == 0ULL) return;
    if (tid == 0) *key = 0ULL;
    const int deg = (int)(best >> 32);
    const long long c = (long long)(0xffffffffu - (unsigned)(best & 0xffffffffULL));
    const int W = (int)clu_words(n);
    if (deg > 1) {
        const unsigned long long* row = adj + c * W;
        for (int w = tid; w < W; w += DFF_CLU_APPLY_THREADS) {
            const unsigned long long a = alive[w];
            unsigned long long mem = row[w] & a;
            if (!mem) continue;
            alive[w] = a & ~mem;
            while (mem) {
                const int b = __builtin_ctzll(mem);
                mem &= mem - 1;
                labels[(long long)w * 64 + b] = k0;
            }
        }
        if (tid == 0) {
            centers[k0] = (int)c;
            sizes[k0] = deg;
            progress[0] = k0 + 1;
            progress[1] = left - deg;
        }
        return;
    }
    // singletons: alive frame number i (ascending index) becomes cluster k0 + i while that is below max_clusters.
    // Thread t owns the contiguous words [t per, (t + 1) per); an exclusive scan over the threads' popcounts.
    const int per = (W + DFF_CLU_APPLY_THREADS - 1) / DFF_CLU_APPLY_THREADS;
    const int w0 = tid * per, w1 = w0 + per < W ? w0 + per : W;
    int cnt = 0;
    for (int w = w0; w < w1; ++w) cnt += __popcll(alive[w]);
    part[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < DFF_CLU_APPLY_THREADS; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int id = k0 + part[tid] - cnt;                                      // exclusive prefix
    const int total = part[DFF_CLU_APPLY_THREADS - 1];
    for (int w = w0; w < w1; ++w) {
        unsigned long long a = alive[w], keep = a;
        while (a && id < max_clusters) {
            const int b = __builtin_ctzll(a);
            a &= a - 1;
            const long long s = (long long)w * 64 + b;
            labels[s] = id;
            centers[id] = (int)s;
            sizes[id] = 1;
            keep &= ~(1ULL << b);
            ++id;
        }
        id += __popcll(a);                                              // frames beyond the cap keep -1 and stay alive
        alive[w] = keep;
    }
    if (tid == 0) {
        const int made = k0 + total < max_clusters ? total : max_clusters - k0;
        progress[0] = k0 + made;
        progress[1] = left - made;
    }
}
