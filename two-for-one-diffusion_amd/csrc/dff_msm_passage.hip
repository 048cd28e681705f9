// dff_msm_passage.hip -- mean first-passage times and committors of a reversible Markov state model: the Dirichlet problem
//   u_i = g_i on the boundary,   sum_{j != i} X_ij (u_i - u_j) = (sum_j X_ij) s_i on the interior
// on a symmetric flux matrix X, many problems per call, ONE workgroup of 256 threads per problem from the roles to u.
//
// dir_compact    wave 0 walks the roles 64 at a time (a ballot and a prefix count per step): cmap[j] = the compact index of an
//     interior state, 0xFFFF for a boundary state; imap[c] = the full index of interior state c; n = the interior count.
// dir_form       W = diag(d) - offdiag(X_II), lower triangle, and the right-hand side b as ROW n under it ("augmented": the
//     factorisation then carries the forward substitution along and needs no pass of its own).  One wave per interior row i:
//     lanes stride over all K columns, d_i = sum_{j != i} X_ij and sum_{j boundary} X_ij g_j each in that order, then the
//     butterfly; b_i = (d_i + X_ii) s_i + that sum.  d_i is SUMMED, never formed as pi_i - X_ii.
// factorisation  W = L D L^T, the square-root-free Cholesky (pivot d_j, unit L), right-looking.  What is stored under the
//     diagonal is c_ij = l_ij d_j (the column as the updates left it); the trailing update is A_ik -= l_ij c_kj.  Row n ends
//     as D L^-1 b, its l as w = D^-1 L^-1 b.  A pivot that is not finite or not above n 2^-52 d_i (dir_pivot_ok) stops the
//     problem: status 1 + the full index of its state; a state whose b_i is not finite gets a NaN pivot.
//   dff_dir_kernel<true>   n <= DFF_DIR_LDS_LIMIT: the packed lower triangle (rows 0 .. n) in LDS, one column per step, two
//     barriers per column; the 256 threads tile the trailing triangle 16 x 16.
//   dff_dir_kernel<false>  larger n: the matrix in the problem's slice of the workspace, panels of DFF_DIR_NB columns.  Per
//     panel: the diagonal block is factored in LDS; every row below it is solved against the block by one thread (the row in
//     registers, the block read as LDS broadcasts) and leaves c in the matrix and l in a panel buffer; the trailing matrix
//     is updated in 64 x 64 tiles, the two 64 x NB strips of a tile staged in LDS: 4 x 4 results per thread on the fp64 VALU,
//     or v_mfma_f64_16x16x4_f64 on a 32 x 32 quarter per wave (DFF_DIR_MFMA picks; measured in DESIGN.md section 19).
// back substitution   L^T u = w as u_j = w_j - (sum_{i > j} c_ij u_i) / d_j, j descending: after u_j, row j of the matrix is
//     added into the running sums t_k, k < j (row j - 1 is fetched while row j is used).
// Every sum has ONE order that follows from the problem's K, roles and path alone: nothing depends on the batch, on the
// problem's place in it, or on what the workspace held.  No atomics, and no workgroup waits on another.
#pragma once
#include <cfloat>
#include "../../include/dff.h"   // DFF_MSM_MAXK
#include "dff_frames.h"          // wave_sum
#include "dff_msm_table.h"       // the problems' descriptors

#define DFF_DIR_THREADS 256
#define DFF_DIR_MAXP 16384            // problems per call
#define DFF_DIR_LDS_LIMIT 128         // interior states factored out of LDS: 129 * 130 / 2 + 129 + 3 * 128 doubles + the maps
                                      // = 75 280 bytes, two workgroups per CU.  Measured: LDS wins 1.3 - 4 x
                                      // up to here at every batch size; at 160 and 192 (one workgroup per CU) the blocked path wins
#define DFF_DIR_MFMA 1                // the trailing update of the blocked path: 1 = fp64 MFMA, 0 = fp64 VALU
#define DFF_DIR_NB 32                 // panel width of the blocked factorisation
#define DFF_DIR_TILE 64               // trailing tiles
#define DFF_DIR_LDP (DFF_DIR_NB + 1)  // odd leading dimension of the LDS strips and of the diagonal block: no bank conflicts
#define DFF_DIR_NOSTATE 0xFFFFu

__host__ __device__ inline long long dir_tri(long long rows) { return rows * (rows + 1) / 2; }
// doubles of a problem's slice of the workspace: the matrix (Kmax rows) | the panel's l (Kmax rows of NB)
__host__ __device__ inline long long dir_slice_doubles(int Kmax) { return (long long)Kmax * Kmax + (long long)Kmax * DFF_DIR_NB; }
// dynamic LDS of dff_dir_kernel<true> for up to nl interior states: cmap | imap (1024 ushorts each) | triangle | lcol | w | t | dref
__host__ inline size_t dir_lds_bytes(int nl) {
    return 2 * DFF_MSM_MAXK * sizeof(unsigned short) + (size_t)(dir_tri(nl + 1) + (nl + 1) + 3 * nl) * sizeof(double);
}

struct DirLds {                                                      // packed lower triangle, row-major
    double* a;
    __device__ __forceinline__ double& at(int i, int k) const { return a[((i * (i + 1)) >> 1) + k]; }
};
struct DirGlb {                                                      // full rows in global memory
    double* a;
    int ld;
    __device__ __forceinline__ double& at(int i, int k) const { return a[(size_t)i * ld + k]; }
};

// A pivot must be finite and exceed n 2^-52 of its state's own d_i: an interior component without a path to the boundary is
// singular in exact arithmetic and leaves a pivot of rounding size (or zero, or a negative one), far below that; the pivots of
// a connected problem stay above it up to cond(W) ~ 1 / (n 2^-52) (measured: 592 x the guard at cond 1e13, n = 297).
__device__ __forceinline__ bool dir_pivot_ok(double p, double d, int n) { return p > (double)n * 0x1p-52 * d && p <= DBL_MAX; }

// roles -> maps.  Returns the interior count; bad = a role outside {0, 1}.  Ends with a barrier.
__device__ inline int dir_compact(const int* __restrict__ role, int K, unsigned short* cmap, unsigned short* imap, int* sh,
                                  bool& bad) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        int base = 0, wrong = 0;
        for (int c = 0; c < K; c += 64) {
            const int j = c + lane;
            const int r = j < K ? role[j] : 1;
            const bool in = j < K && r == 0;
            wrong |= (r != 0 && r != 1);
            const unsigned long long m = __ballot(in);
            const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (j < K) cmap[j] = in ? (unsigned short)pos : (unsigned short)DFF_DIR_NOSTATE;
            if (in) imap[pos] = (unsigned short)j;                  // pos < K <= 1024
            base += __popcll(m);
        }
        const unsigned long long w = __ballot(wrong != 0);
        if (lane == 0) { sh[0] = base; sh[1] = w != 0; }
    }
    __syncthreads();
    bad = sh[1] != 0;
    return sh[0];
}

// W (lower triangle) and b (row n) from the problem's compact (K, K) flux matrix
template <class Mat>
__device__ inline void dir_form(const double* __restrict__ X, int K, const unsigned short* cmap, const unsigned short* imap,
                                int n, const double* __restrict__ g, const double* __restrict__ s, Mat M, double* dref) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int ic = wave; ic < n; ic += DFF_DIR_THREADS / 64) {
        const int fi = imap[ic];
        const double* row = X + (size_t)fi * K;
        double d = 0.0, bg = 0.0;
        for (int j = lane; j < K; j += 64) {
            const double x = row[j];
            const unsigned cj = cmap[j];
            if (cj == DFF_DIR_NOSTATE) bg = fma(x, g[j], bg);       // g is read at boundary states only
            else if ((int)cj < ic) M.at(ic, (int)cj) = -x;
            if (j != fi) d += x;
        }
        d = wave_sum(d);
        bg = wave_sum(bg);
        if (lane == 0) {
            const double b = fma(d + row[fi], s[fi], bg);           // s is read at interior states only
            M.at(ic, ic) = (b - b == 0.0) ? d : __builtin_nan("");  // a right-hand side that is not finite (X_ii, g or s NaN /
            M.at(n, ic) = b;                                        // Inf) fails the state's pivot: never status 0 with NaN in u
            dref[ic] = d;
        }
    }
}

// u over the problem's K states: NaN everywhere (a failure), or g on the boundary (the interior follows)
__device__ inline void dir_fill(double* __restrict__ u, const double* __restrict__ g, const unsigned short* cmap, int K,
                                bool nan) {
    for (int j = threadIdx.x; j < K; j += DFF_DIR_THREADS) {
        if (nan) u[j] = __builtin_nan("");
        else if (cmap[j] == DFF_DIR_NOSTATE) u[j] = g[j];
    }
}

// L^T u = w by running sums over the rows of M, j descending; t zeroed here.  One barrier per row.
template <class Mat>
__device__ inline void dir_back(Mat M, int n, const double* w, double* t, const unsigned short* imap, double* __restrict__ u) {
    const int tid = threadIdx.x;
    for (int k = tid; k < n; k += DFF_DIR_THREADS) t[k] = 0.0;
    double cur[DFF_MSM_MAXK / DFF_DIR_THREADS], nxt[DFF_MSM_MAXK / DFF_DIR_THREADS], dcur, dnxt = 1.0;
    {
        const int j = n - 1;
        dcur = M.at(j, j);
#pragma unroll
        for (int q = 0; q < DFF_MSM_MAXK / DFF_DIR_THREADS; ++q) {
            const int k = tid + q * DFF_DIR_THREADS;
            cur[q] = k < j ? M.at(j, k) : 0.0;
        }
    }
    __syncthreads();
    for (int j = n - 1; j >= 0; --j) {
        if (j > 0) {                                                // row j - 1 travels while row j is used
            dnxt = M.at(j - 1, j - 1);
#pragma unroll
            for (int q = 0; q < DFF_MSM_MAXK / DFF_DIR_THREADS; ++q) {
                const int k = tid + q * DFF_DIR_THREADS;
                nxt[q] = k < j - 1 ? M.at(j - 1, k) : 0.0;
            }
        }
        const double uj = w[j] - t[j] / dcur;                       // the same bits in every thread
        if (tid == 0) u[imap[j]] = uj;
#pragma unroll
        for (int q = 0; q < DFF_MSM_MAXK / DFF_DIR_THREADS; ++q) {
            const int k = tid + q * DFF_DIR_THREADS;
            if (k < j) t[k] = fma(cur[q], uj, t[k]);
        }
        __syncthreads();
        dcur = dnxt;
#pragma unroll
        for (int q = 0; q < DFF_MSM_MAXK / DFF_DIR_THREADS; ++q) cur[q] = nxt[q];
    }
}

// ---- the factorisation in LDS: rows 0 .. n of the packed triangle.  Returns the compact index of a failed pivot, or -1.
__device__ inline int dir_factor_lds(DirLds M, int n, double* lcol, double* w, const double* dref) {
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    for (int j = 0; j < n; ++j) {
        __syncthreads();                                            // column j is final
        const double p = M.at(j, j);
        if (!dir_pivot_ok(p, dref[j], n)) return j;                 // the same p in every thread
        for (int i = j + 1 + tid; i <= n; i += DFF_DIR_THREADS) {
            const double l = M.at(i, j) / p;
            lcol[i] = l;
            if (i == n) w[j] = l;
        }
        __syncthreads();
        for (int i = j + 1 + ty; i <= n; i += 16) {
            const double lij = lcol[i];
            const int kend = i < n ? i : n - 1;                     // row n has no diagonal entry
            for (int k = j + 1 + tx; k <= kend; k += 16) M.at(i, k) = fma(-lij, M.at(k, j), M.at(i, k));
        }
    }
    __syncthreads();
    return -1;
}

// ---- the blocked factorisation in global memory: rows 0 .. n of A (leading dimension ld), the panel's l in Lp (rows of NB).
// Db, Ls, Cs: LDS blocks of (NB, LDP), (TILE, LDP), (TILE, LDP) doubles.  Returns the failed pivot's compact index, or -1.
__device__ inline int dir_factor_blocked(double* A, int ld, double* Lp, int n, double* Db, double* lcol, double* Ls,
                                         double* Cs, double* w, const double* dref, long long* ticks, int mfma) {
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    constexpr int NB = DFF_DIR_NB, LDP = DFF_DIR_LDP, TILE = DFF_DIR_TILE;
    for (int p0 = 0; p0 < n; p0 += NB) {
        const int wd = n - p0 < NB ? n - p0 : NB;
        __syncthreads();                                            // the last panel's tiles are written, Db is free
        const long long t0 = wall_clock64();
        for (int e = tid; e < NB * NB; e += DFF_DIR_THREADS) {      // the diagonal block, padded with the identity
            const int r = e / NB, c = e % NB;
            Db[r * LDP + c] = (r < wd && c <= r) ? A[(size_t)(p0 + r) * ld + p0 + c] : (r == c ? 1.0 : 0.0);
        }
        for (int j = 0; j < wd; ++j) {
            __syncthreads();
            const double p = Db[j * LDP + j];
            if (!dir_pivot_ok(p, dref[p0 + j], n)) return p0 + j;
            if (tid > j && tid < wd) lcol[tid] = Db[tid * LDP + j] / p;
            __syncthreads();
            for (int e = tid; e < NB * NB; e += DFF_DIR_THREADS) {
                const int i = e / NB, k = e % NB;
                if (i > j && i < wd && k > j && k <= i) Db[i * LDP + k] = fma(-lcol[i], Db[k * LDP + j], Db[i * LDP + k]);
            }
        }
        __syncthreads();
        for (int e = tid; e < NB * NB; e += DFF_DIR_THREADS) {      // back to the matrix: the back substitution reads it
            const int r = e / NB, c = e % NB;
            if (r < wd && c <= r) A[(size_t)(p0 + r) * ld + p0 + c] = Db[r * LDP + c];
        }
        // the rows below the block, one thread each: c_i = a_i - sum l_i c^T over the block's columns, l_i = c_i / d
        for (int i = p0 + wd + tid; i <= n; i += DFF_DIR_THREADS) {
            double row[NB];                                         // static indices only: the row stays in registers
#pragma unroll
            for (int c = 0; c < NB; ++c) row[c] = c < wd ? A[(size_t)i * ld + p0 + c] : 0.0;
#pragma unroll 1
            for (int c2 = 0; c2 < NB; ++c2) {                       // column c2 of the block against the rest of the row
                double v = 0.0;
#pragma unroll
                for (int c = 0; c < NB; ++c) v = c == c2 ? row[c] : v;
                const double l = v / Db[c2 * LDP + c2];             // padding: 0 / 1
                Lp[(size_t)i * NB + c2] = l;
                if (i == n && c2 < wd) w[p0 + c2] = l;
#pragma unroll
                for (int c = 0; c < NB; ++c) row[c] = c > c2 ? fma(-l, Db[c * LDP + c2], row[c]) : row[c];
            }
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (c < wd) A[(size_t)i * ld + p0 + c] = row[c];
        }
        __syncthreads();
        const long long t1 = wall_clock64();
        // the trailing matrix, rows r0 .. n, columns r0 .. n - 1, lower tiles
        const int r0 = p0 + wd;
        for (int ti = r0; ti <= n; ti += TILE)
            for (int tk = r0; tk <= ti && tk < n; tk += TILE) {
                __syncthreads();                                    // the rows are written; the strips are free
                for (int e = tid; e < TILE * NB; e += DFF_DIR_THREADS) {
                    const int r = e / NB, c = e % NB;
                    Ls[r * LDP + c] = ti + r <= n ? Lp[(size_t)(ti + r) * NB + c] : 0.0;
                    Cs[r * LDP + c] = (tk + r <= n && c < wd) ? A[(size_t)(tk + r) * ld + p0 + c] : 0.0;
                }
                __syncthreads();
                if (mfma) {
                    // v_mfma_f64_16x16x4_f64 (operand maps: dff_tica.hip's header): each wave takes a 32 x 32 quarter of the tile
                    // as 2 x 2 blocks of 16 x 16, eight steps of four panel columns.  A[i][k] = l of tile row i, B[k][j] = c of
                    // tile column j, both in lane (i or j = lane & 15, k = lane >> 4); register r of lane l is
                    // D[row = (l >> 4) + 4 r][col = l & 15].
                    typedef double dir_v4 __attribute__((ext_vector_type(4)));
                    const int lane = tid & 63, wv = tid >> 6, rb = 32 * (wv >> 1), cb = 32 * (wv & 1);
                    const int lo = lane & 15, hi = lane >> 4;
                    dir_v4 acc4[2][2] = {};
#pragma unroll
                    for (int c0 = 0; c0 < NB; c0 += 4) {
                        double av[2], bv[2];
#pragma unroll
                        for (int a = 0; a < 2; ++a) av[a] = Ls[(rb + 16 * a + lo) * LDP + c0 + hi];
#pragma unroll
                        for (int b = 0; b < 2; ++b) bv[b] = Cs[(cb + 16 * b + lo) * LDP + c0 + hi];
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b)
                                acc4[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc4[a][b], 0, 0, 0);
                    }
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int i = ti + rb + 16 * a + hi + 4 * r, k = tk + cb + 16 * b + lo;
                                if (i <= n && k < n && k <= i) A[(size_t)i * ld + k] -= acc4[a][b][r];
                            }
                    continue;
                }
                double acc[4][4] = {};
#pragma unroll 4
                for (int c = 0; c < NB; ++c) {
                    double li[4], ck[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) li[a] = Ls[(ty + 16 * a) * LDP + c];
#pragma unroll
                    for (int b = 0; b < 4; ++b) ck[b] = Cs[(tx + 16 * b) * LDP + c];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = fma(li[a], ck[b], acc[a][b]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = ti + ty + 16 * a, k = tk + tx + 16 * b;
                        if (i <= n && k < n && k <= i) A[(size_t)i * ld + k] -= acc[a][b];
                    }
            }
        __syncthreads();
        const long long t2 = wall_clock64();
        ticks[0] += t1 - t0;                                        // diagonal block and the rows under it
        ticks[1] += t2 - t1;                                        // trailing update
    }
    __syncthreads();
    return -1;
}

// ---- one workgroup per problem.  desc[p] = flux slot << DFF_MSM_KBITS | K_p (dff_msm_table.h); slots of Kmax^2 (flux), Kmax (role, g, s, u).  The
// workgroup owns the problem when own_lo <= its interior count <= own_hi, else it leaves at once (the other path's launch
// takes it).  work: slices of `slice` doubles (LDSP: unused).
template <bool LDSP>
__global__ __launch_bounds__(DFF_DIR_THREADS) void dff_dir_kernel(const double* __restrict__ flux,
                                                                  const long long* __restrict__ desc, int Kmax,
                                                                  const int* __restrict__ role, const double* __restrict__ g,
                                                                  const double* __restrict__ s, double* __restrict__ u,
                                                                  int* __restrict__ status, double* work, long long slice,
                                                                  int own_lo, int own_hi, int mfma) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dir_lds[];
    __shared__ int sh[2];
    unsigned short* cmap = (unsigned short*)dir_lds;
    unsigned short* imap = cmap + DFF_MSM_MAXK;
    double* dbl = (double*)(imap + DFF_MSM_MAXK);
    const unsigned p = blockIdx.x;
    const long long de = desc[p];
    const int K = MSM_PROBLEM_K(de);
    const double* X = flux + (size_t)MSM_PROBLEM_SLOT(de) * Kmax * Kmax;
    role += (size_t)p * Kmax;
    g += (size_t)p * Kmax;
    s += (size_t)p * Kmax;
    u += (size_t)p * Kmax;
    bool bad;
    const int n = dir_compact(role, K, cmap, imap, sh, bad);
    if (n < own_lo || n > own_hi) return;
    if (bad || n == K || n == 0) {                                  // a bad role, no boundary, or nothing to solve: u = g
        dir_fill(u, g, cmap, K, bad || n == K);
        if (threadIdx.x == 0) status[p] = bad ? -2 : (n == K ? -1 : 0);
        return;
    }
    int failed;
    if constexpr (LDSP) {
        DirLds M{dbl};
        double* lcol = dbl + dir_tri(n + 1);
        double* w = lcol + (n + 1);
        double* t = w + n;
        double* dref = t + n;
        dir_form(X, K, cmap, imap, n, g, s, M, dref);
        failed = dir_factor_lds(M, n, lcol, w, dref);
        if (failed < 0) {
            dir_fill(u, g, cmap, K, false);
            dir_back(M, n, w, t, imap, u);
        }
    } else {
        double* A = work + (size_t)p * slice;
        double* Lp = A + (size_t)Kmax * Kmax;
        double* Db = dbl;
        double* Ls = Db + DFF_DIR_NB * DFF_DIR_LDP;
        double* Cs = Ls + DFF_DIR_TILE * DFF_DIR_LDP;
        double* lcol = Cs + DFF_DIR_TILE * DFF_DIR_LDP;
        double* w = lcol + DFF_DIR_NB;
        double* t = w + DFF_MSM_MAXK;
        double* dref = t + DFF_MSM_MAXK;
        DirGlb M{A, Kmax};
        long long ticks[2] = {0, 0};
        const long long c0 = wall_clock64();
        dir_form(X, K, cmap, imap, n, g, s, M, dref);
        __syncthreads();
        const long long c1 = wall_clock64();
        failed = dir_factor_blocked(A, Kmax, Lp, n, Db, lcol, Ls, Cs, w, dref, ticks, mfma);
        const long long c2 = wall_clock64();
        if (failed < 0) {
            dir_fill(u, g, cmap, K, false);
            dir_back(M, n, w, t, imap, u);
            // For the benchmark: where the time went, in ticks of the constant 100 MHz clock, left in the first four doubles of
            // the problem's slice once nothing reads it any more: formation | panels | trailing updates | back substitution.
            if (threadIdx.x == 0) {
                A[0] = (double)(c1 - c0); A[1] = (double)ticks[0]; A[2] = (double)ticks[1]; A[3] = (double)(wall_clock64() - c2);
            }
        }
    }
    if (failed >= 0) dir_fill(u, g, cmap, K, true);
    if (threadIdx.x == 0) status[p] = failed >= 0 ? 1 + (int)imap[failed] : 0;
}

// dynamic LDS of dff_dir_kernel<false>: the maps | diagonal block | two strips | lcol | w | t | dref
__host__ inline size_t dir_blocked_lds_bytes() {
    return 2 * DFF_MSM_MAXK * sizeof(unsigned short) +
           (size_t)(DFF_DIR_NB * DFF_DIR_LDP + 2 * DFF_DIR_TILE * DFF_DIR_LDP + DFF_DIR_NB + 3 * DFF_MSM_MAXK) * sizeof(double);
}
