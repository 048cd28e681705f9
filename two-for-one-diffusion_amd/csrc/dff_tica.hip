// dff_tica.hip -- fitting a TICA model on the GPU: the TIC features of time-ordered frames and their lag-tau second
// moments, the heavy part of TICA(lagtime, dim).fit_transform(get_tic_features(sorted data)), evaluate/evaluators.py:384-420.
//
// Replaces, for (n, N, 3) structures already resident in HBM:
//   get_tic_features(xyz)                          evaluate/evaluators.py:433-445 (dff_tica_features_kernel)
//   the running sums of deeptime's symmetrised,    evaluators.py:404 (TICA.fit_transform -> its covariance estimator)
//   mean-free covariance estimator                 (dff_tica_moments_kernel + dff_tica_reduce_kernel)
// The covariances (one rank-2 correction of the sums) and the eigen-decomposition stay on the host, in numpy fp64
// (evaluate.py: tica_covariances, tica_from_covariances).
//
// Moments.  With g_t = f_t - s (fp64; s fixed by the caller) and the pairs (t, t + tau) of frames of one trajectory
// (a_t = 1), the kernels add
//   S_x = sum a_t g_t,   S_y = sum a_t g_{t+tau},
//   M_0 = sum a_t (g_t g_t^T + g_{t+tau} g_{t+tau}^T),   M_tau = sum a_t (g_t g_{t+tau}^T + g_{t+tau} g_t^T)
// (sum a_t g_{t+tau} = sum b_t g_t: b_t = a_{t-tau}).  They are computed as two plain SYRKs over the pairs,
//   P = sum u u^T, Q = sum v v^T,  u = g_t + g_{t+tau}, v = g_t - g_{t+tau};  M_0 = (P + Q) / 2, M_tau = (P - Q) / 2,
// and S_x + S_y = sum u, S_x - S_y = sum v: two products instead of three, with the same operand traffic.
//
// Pipeline, per chunk of <= C pair starts (C from the feature count only):
//   1. dff_tica_features_kernel writes the fp32 features of the chunk's frames, tau frames of overlap included, into the
//      workspace (row-major, F per row).  Its feature loop is deliberately a second one next to struct_tic_walk
//      (dff_frames.h): it stops every DFF_TICA_FCH features, in the middle of the distance block, to flush its LDS
//      stage, and carries the pair (i, j) across the stops.  Both call struct_dihedral / pwd_dist2: the same bits.
//   2. dff_tica_moments_kernel: one workgroup (4 waves) per (64 x 64 upper-triangular output tile, slice of pairs).  Per
//      stage of 32 pairs it converts rows t and t + tau of the tile's two 64-feature blocks to fp64 u, v in LDS, then
//      each wave runs v_mfma_f64_16x16x4_f64 on its 32 x 32 quarter (2 x 2 blocks, P and Q).  It writes its partial tile
//      (and, on diagonal tiles, the partial feature sums).  The slice count depends on the shapes only.
//   3. dff_tica_reduce_kernel sums the slices in slice order and adds to the caller's accumulators: no atomics, the
//      result is bit-identical from call to call.
// v_mfma_f64_16x16x4_f64 operands: A[i][k] = lane (i = lane & 15, k = lane >> 4), B[k][j] likewise, one f64 each;
// C/D: register r of lane l is D[row = (l >> 4) + 4 r][col = l & 15] -- NOT the f32 16x16x4 map (row = 4 (l >> 4) + r).
#pragma once
#include "dff_frames.h"   // struct_tiles, struct_dihedral, pwd_dist2, f64x4

#define DFF_TICA_T 64          // output tile edge (features)
#define DFF_TICA_K 32          // pairs per LDS stage
#define DFF_TICA_LD 80         // LDS row stride in doubles: 640 B = 128 B mod 256, the two pair rows of a ds_read_b64
                               // half-wave land on disjoint banks
#define DFF_TICA_RUNS 64       // runs of consecutive pairs per launch (kernel argument)
#define DFF_TICA_WGS 1024      // workgroups the MFMA pass aims for: 256 CUs x 4
#define DFF_TICA_FCH 32        // features per staging chunk of the feature kernel
#define DFF_TICA_THREADS 256
#define DFF_TICA_LDS_BYTES (4 * DFF_TICA_K * DFF_TICA_LD * 8)

// the pairs of one launch: run r holds pairs cum[r] .. cum[r + 1] - 1, the first of them starting at feature row row[r]
struct TicaRuns {
    int n;
    int row[DFF_TICA_RUNS];
    int cum[DFF_TICA_RUNS + 1];
};

// ---- TIC features, fp32, row s at out[s * F]: dihedrals, then distances in triu_indices(N, N, 1) order -- the
// values dff_struct_tic projects (same struct_dihedral / pwd_dist2).  LDS: tile | stage (64 x (FCH + 1))
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_tica_features_kernel(const float* __restrict__ x, long long n,
                                                                             int N, float* __restrict__ out,
                                                                             unsigned magic, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tile = smem;
    float* stage = smem + DFF_STRUCT_TILE * struct_ld(N);
    const int F = struct_tic_num_features(N);
    constexpr int ls = DFF_TICA_FCH + 1;
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        int i = 0, j = 1;                                   // next pair of the distance features (wave-uniform)
        for (int f0 = 0; f0 < F; f0 += DFF_TICA_FCH) {
            const int w = F - f0 < DFF_TICA_FCH ? F - f0 : DFF_TICA_FCH;
            for (int c = 0; c < w; ++c) {
                const int f = f0 + c;
                float v;
                if (f < N - 3) {
                    v = struct_dihedral(xs, f);
                } else {
                    v = pwd_dist2(xs, 3 * i, 3 * j);
                    if (++j == N) { ++i; j = i + 1; }
                }
                if (live) stage[lane * ls + c] = v;
            }
            __syncthreads();
            float* dst = out + s0 * F + f0;
            for (int k = lane; k < cnt * w; k += DFF_STRUCT_TILE) {
                const int r = k / w, c = k - r * w;
                dst[(long long)r * F + c] = stage[r * ls + c];
            }
            __syncthreads();
        }
    });
}

// upper-triangular tile t (row-major over block rows: block row b holds NB - b tiles) -> (bi, bj), bi <= bj
__device__ __forceinline__ void tica_tile(int t, int NB, int& bi, int& bj) {
    int b = 0;
    while (t >= NB - b) { t -= NB - b; ++b; }
    bi = b;
    bj = b + t;
}

// ---- P, Q partial tiles.  grid = nslices * NT; part[((slice * NT + tile) * 2 + {P, Q}) * 4096 + row * 64 + col],
// psum[((slice * NB + b) * 2 + {u, v}) * 64 + l] (diagonal tiles only).  LDS: uI | vI | uJ | vJ, K x LD doubles each
__global__ __launch_bounds__(DFF_TICA_THREADS) void dff_tica_moments_kernel(const float* __restrict__ feat, int F, int lag,
                                                                             const double* __restrict__ shift,
                                                                             TicaRuns runs, int npairs, int per, int NB,
                                                                             int NT, double* __restrict__ part,
                                                                             double* __restrict__ psum) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int K = DFF_TICA_K, LD = DFF_TICA_LD;
    const int tile = blockIdx.x % NT, slice = blockIdx.x / NT;
    int bi, bj;
    tica_tile(tile, NB, bi, bj);
    const bool diag = bi == bj;
    double* uI = lds;
    double* vI = lds + K * LD;
    const double* uJ = diag ? uI : lds + 2 * K * LD;
    const double* vJ = diag ? vI : lds + 3 * K * LD;
    const int I0 = bi * DFF_TICA_T, J0 = bj * DFF_TICA_T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wi = wave >> 1, wj = wave & 1;
    const bool fI = I0 + lane < F, fJ = J0 + lane < F;
    const double shI = fI ? shift[I0 + lane] : 0.0, shJ = fJ ? shift[J0 + lane] : 0.0;
    const long long ldlag = (long long)lag * F;
    const int q_begin = slice * per;
    const int q_end = q_begin + per < npairs ? q_begin + per : npairs;
    f64x4 P[2][2], Q[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) P[a][b] = Q[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double su = 0.0, sv = 0.0;
    for (int q0 = q_begin; q0 < q_end; q0 += K) {
        __syncthreads();
        // stage: pair p = 4 m + wave (wave-uniform, so the run lookup is scalar), feature = lane of the block
#pragma unroll 2
        for (int m = 0; m < K / 4; ++m) {
            const int p = 4 * m + wave, q = q0 + p;
            double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
            if (q < q_end) {
                const int lo = last_le(runs.cum, runs.n, q);
                const float* f0 = feat + (long long)(runs.row[lo] + (q - runs.cum[lo])) * F;
                if (fI) { a = (double)f0[I0 + lane] - shI; b = (double)f0[ldlag + I0 + lane] - shI; }
                if (!diag && fJ) { c = (double)f0[J0 + lane] - shJ; d = (double)f0[ldlag + J0 + lane] - shJ; }
            }
            uI[p * LD + lane] = a + b;
            vI[p * LD + lane] = a - b;
            if (!diag) {
                lds[2 * K * LD + p * LD + lane] = c + d;
                lds[3 * K * LD + p * LD + lane] = c - d;
            }
        }
        __syncthreads();
        if (diag && wave == 0)
            for (int p = 0; p < K; ++p) { su += uI[p * LD + lane]; sv += vI[p * LD + lane]; }
#pragma unroll
        for (int ks = 0; ks < K / 4; ++ks) {
            const int o = (4 * ks + (lane >> 4)) * LD + (lane & 15);
            double aU[2], aV[2], bU[2], bV[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                aU[h] = uI[o + 32 * wi + 16 * h];
                aV[h] = vI[o + 32 * wi + 16 * h];
                bU[h] = uJ[o + 32 * wj + 16 * h];
                bV[h] = vJ[o + 32 * wj + 16 * h];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    P[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aU[a], bU[b], P[a][b], 0, 0, 0);
                    Q[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aV[a], bV[b], Q[a][b], 0, 0, 0);
                }
        }
    }
    double* dst = part + ((size_t)slice * NT + tile) * 2 * (DFF_TICA_T * DFF_TICA_T);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 32 * wi + 16 * a + (lane >> 4) + 4 * r, col = 32 * wj + 16 * b + (lane & 15);
                dst[row * DFF_TICA_T + col] = P[a][b][r];
                dst[DFF_TICA_T * DFF_TICA_T + row * DFF_TICA_T + col] = Q[a][b][r];
            }
    if (diag && wave == 0) {
        double* ps = psum + ((size_t)slice * NB + bi) * 2 * DFF_TICA_T;
        ps[lane] = su;
        ps[DFF_TICA_T + lane] = sv;
    }
}

// ---- slices -> accumulators, in slice order: m0 / mt (F x F row-major, upper triangle i <= j) += (P +- Q) / 2,
// sx / sy (F) += (sum u +- sum v) / 2.  One thread per tile element, then one per feature.
__global__ __launch_bounds__(DFF_TICA_THREADS) void dff_tica_reduce_kernel(const double* __restrict__ part,
                                                                            const double* __restrict__ psum, int F, int NB,
                                                                            int NT, int nslices, double* __restrict__ sx,
                                                                            double* __restrict__ sy,
                                                                            double* __restrict__ m0,
                                                                            double* __restrict__ mt) {
    constexpr int TT = DFF_TICA_T * DFF_TICA_T;
    const long long gid = (long long)blockIdx.x * DFF_TICA_THREADS + threadIdx.x;
    const long long nel = (long long)NT * TT;
    if (gid < nel) {
        const int tile = (int)(gid / TT), e = (int)(gid % TT);
        int bi, bj;
        tica_tile(tile, NB, bi, bj);
        const int i = bi * DFF_TICA_T + e / DFF_TICA_T, j = bj * DFF_TICA_T + e % DFF_TICA_T;
        if (i >= F || j >= F || i > j) return;
        double p = 0.0, q = 0.0;
        for (int s = 0; s < nslices; ++s) {
            const double* src = part + ((size_t)s * NT + tile) * 2 * TT + e;
            p += src[0];
            q += src[TT];
        }
        m0[(size_t)i * F + j] += 0.5 * (p + q);
        mt[(size_t)i * F + j] += 0.5 * (p - q);
    } else if (gid < nel + (long long)NB * DFF_TICA_T) {
        const int k = (int)(gid - nel), b = k / DFF_TICA_T, l = k % DFF_TICA_T, f = b * DFF_TICA_T + l;
        if (f >= F) return;
        double u = 0.0, v = 0.0;
        for (int s = 0; s < nslices; ++s) {
            const double* src = psum + ((size_t)s * NB + b) * 2 * DFF_TICA_T + l;
            u += src[0];
            v += src[DFF_TICA_T];
        }
        sx[f] += 0.5 * (u + v);
        sy[f] += 0.5 * (u - v);
    }
}
