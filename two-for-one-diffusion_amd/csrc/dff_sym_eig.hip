// dff_sym_eig.hip -- the k algebraically largest eigenvalues, and optionally their eigenvectors, of many dense symmetric fp64
// matrices of differing sizes K <= 1024 (the symmetrised transition matrices of Markov state models), ONE workgroup per problem
// from the matrix to the vectors.  Four stages:
//
// eig_tridiag    Householder reduction A = Q T Q^T of the lower triangle on a working copy (LAPACK's dsytd2, lower): per column
//     j the reflector H_j = I - tau v v^T (v_{j+1} = 1) that zeroes the column under the sub-diagonal, p = tau A v,
//     w = p - (tau / 2)(p^T v) v, A -= v w^T + w v^T.  The rank-2 update of column j is NOT applied on its own: it is pending
//     while column j + 1 alone is brought up to date, v_{j+1} is formed from it, and ONE pass over the trailing triangle applies
//     the pending update to a row and multiplies the updated row with v_{j+1} -- each entry is read and written once per column.
//     A row belongs to a GROUP of G lanes (lane l of the group holds columns c0 + l, c0 + l + G, ...): the row's product with v is a
//     butterfly over the group, its contributions to the rows above (the transposed half of the symmetric product) are summed per
//     lane in registers over the group's rows in row order, and the groups' partial sums are added in group order.  A column
//     that is already zero under the sub-diagonal gets tau = 0 and no division; the column norm is taken of the column divided by
//     its largest entry.  The reflectors stay in the working copy for the back-transformation: in place of the column (LDS), or
//     in row j of the unused upper triangle (workspace), where a wave reads them contiguously.
// eig_bisect     the kk = min(k, K) largest eigenvalues of T by Sturm counts (LAPACK's dstebz recurrence with its pivmin
//     safeguard), multisection: every eigenvalue has threads / 32 shifts per round inside its own bracket, all counts of a round
//     run at once, and a bracket shrinks to the two neighbouring shifts that enclose the wanted count.  A bracket is done when no
//     shift lies strictly inside it any more.
// eig_vectors    inverse iteration on T - lambda I as LAPACK's dstein runs it: a tridiagonal LU with partial pivoting (one
//     thread; the recurrences are serial), a start vector from a fixed hash, at most DFF_EIG_MAXITS solves, eigenvalues closer
//     than 10 ulp pushed apart, every vector orthogonalised against ALL earlier ones by modified Gram-Schmidt at every iteration
//     (dstein does so inside clusters closer than 1e-3 |T|_1 only, which leaves eps |T| / gap between the vectors of separated
//     eigenvalues; with k <= 32 vectors the full sweep costs nothing); the matrix is not split at zero off-diagonals, so exactly
//     repeated eigenvalues get an orthonormal basis from the same mechanism.
// eig_back       v = Q z: the reflectors from the last to the first, a vector per group, its components in registers; unit
//     2-norm, the component of largest magnitude positive (the lowest index wins a tie).
//
//   dff_sym_eig_kernel<true>   K <= DFF_EIG_LDS_LIMIT: the packed lower triangle in LDS, 256 threads, groups of 16 lanes
//   dff_sym_eig_kernel<false>  larger K: the matrix in the problem's slice of the workspace, 512 threads, a wave per row
// Every sum has ONE order that follows from the problem's K and the path alone.  No atomics, no workgroup waits on another.
#pragma once
#include <cfloat>
#include <type_traits>
#include "../../include/dff.h"   // DFF_MSM_MAXK
#include "dff_frames.h"          // wave_sum

#define DFF_EIG_MAXP 16384            // problems per call
#define DFF_EIG_MAXTOP 32             // eigenpairs per problem
#define DFF_EIG_LDS_LIMIT 176         // the largest K reduced out of LDS: 158 912 bytes, one workgroup per CU (179 is the largest
                                      // that fits 160 KB).  Measured: LDS wins 1.2 - 1.7 x at every size up to
                                      // here and every batch size (2.3 - 2.8 x at K <= 96, P = 1024, where two workgroups share a CU)
#define DFF_EIG_MAXITS 5              // inverse iterations per vector (dstein's MAXITS)
#define DFF_EIG_EXTRA 2               // further iterations after the growth criterion is first met (dstein's EXTRA)
#define DFF_EIG_ROUNDS 64             // multisection rounds at the most: a bracket shrinks at least ninefold per round
#define DFF_EIG_TICKS 4               // doubles at the head of a slice: 100 MHz ticks of reduction | bisection | vectors | unused

template <bool LDSP> struct EigCfg;
template <> struct EigCfg<true> {
    static constexpr int T = 256, G = 16, NG = T / G, NACC = (DFF_EIG_LDS_LIMIT + G - 1) / G;
};
template <> struct EigCfg<false> {
    static constexpr int T = 512, G = 64, NG = T / G, NACC = (DFF_MSM_MAXK + G - 1) / G;
};

__host__ __device__ inline long long eig_tri(long long rows) { return rows * (rows + 1) / 2; }
// doubles of a problem's slice of the workspace: the ticks | the working copy (Kmax rows)
__host__ __device__ inline long long eig_slice_doubles(int Kmax) { return DFF_EIG_TICKS + (long long)Kmax * Kmax; }
// doubles of LDS besides the matrix: d e tau va vb w p (7 K) | part (NG K; the LU of eig_vectors: 6 K) | lam lo hi (3 x 32) |
// red (16) | counts (T ints)
__host__ __device__ inline long long eig_lds_vector_doubles(int K, int NG, int T) {
    return (long long)(7 + NG) * K + 3 * DFF_EIG_MAXTOP + 16 + T / 2;
}
__host__ inline size_t eig_lds_bytes(int K, bool ldsp) {
    const long long v = ldsp ? eig_lds_vector_doubles(K, EigCfg<true>::NG, EigCfg<true>::T) + eig_tri(K)
                             : eig_lds_vector_doubles(K, EigCfg<false>::NG, EigCfg<false>::T);
    return (size_t)v * sizeof(double);
}

struct EigLds {                                                      // packed lower triangle, row-major; reflector j in column j
    double* a;
    __device__ __forceinline__ double& at(int i, int k) const { return a[((i * (i + 1)) >> 1) + k]; }
    __device__ __forceinline__ double& refl(int j, int i) const { return at(i, j); }
};
struct EigGlb {                                                      // full rows in global memory; reflector j in row j, upper part
    double* a;
    int ld;
    __device__ __forceinline__ double& at(int i, int k) const { return a[(size_t)i * ld + k]; }
    __device__ __forceinline__ double& refl(int j, int i) const { return a[(size_t)j * ld + i]; }
};

template <int G> __device__ __forceinline__ double eig_group_sum(double v) {   // butterfly over G lanes: one order, every lane the sum
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sums and maxima over the workgroup: the waves' butterflies, then the waves in order.  Two barriers; every thread gets the same bits.
template <int T> __device__ inline double eig_blk_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}
template <int T> __device__ inline double eig_blk_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < T / 64; ++w) s = fmax(s, red[w]);
    __syncthreads();
    return s;
}

// ---- A = Q T Q^T.  d (K), e (K - 1), tau (K - 1) out; va, vb, w, p: K doubles each; part: NG * K.  Ends with a barrier.
template <bool LDSP, class Mat>
__device__ inline void eig_tridiag(Mat M, int K, double* d, double* e, double* tau, double* va, double* vb, double* w, double* p,
                                   double* part, double* red) {
    constexpr int T = EigCfg<LDSP>::T, G = EigCfg<LDSP>::G, NG = EigCfg<LDSP>::NG, NACC = EigCfg<LDSP>::NACC;
    const int tid = threadIdx.x, grp = tid / G, gl = tid % G;
    double* vp = va;                                                // the reflector of the pending update (with w)
    double* vn = vb;                                                // the reflector of this column
    bool pend = false;
    for (int j = 0; j + 1 < K; ++j) {
        // column j up to date; the diagonal entry is final, the rest is the column x to be zeroed (kept in p)
        for (int i = j + tid; i < K; i += T) {
            double a = M.at(i, j);
            if (pend) {
                a -= vp[i] * w[j] + w[i] * vp[j];
                M.at(i, j) = a;
            }
            if (i == j) d[j] = a;
            else p[i] = a;
        }
        __syncthreads();
        const double alpha = p[j + 1];
        double m = 0.0;
        for (int i = j + 2 + tid; i < K; i += T) m = fmax(m, fabs(p[i]));
        const double scale = eig_blk_max<T>(m, red);
        double tauj = 0.0;
        if (scale == 0.0) {                                         // nothing to zero: H = I
            if (tid == 0) { e[j] = alpha; tau[j] = 0.0; }
        } else {
            double s = 0.0;
            for (int i = j + 2 + tid; i < K; i += T) {
                const double q = p[i] / scale;
                s = fma(q, q, s);
            }
            const double xnorm = scale * sqrt(eig_blk_sum<T>(s, red));
            const double big = fmax(fabs(alpha), xnorm);
            const double qa = alpha / big, qx = xnorm / big;
            const double beta = -copysign(big * sqrt(qa * qa + qx * qx), alpha);
            tauj = (beta - alpha) / beta;
            const double inv = 1.0 / (alpha - beta);
            for (int i = j + 2 + tid; i < K; i += T) {
                const double vi = p[i] * inv;
                vn[i] = vi;
                M.refl(j, i) = vi;
            }
            if (tid == 0) { vn[j + 1] = 1.0; e[j] = beta; tau[j] = tauj; }
        }
        if (tauj == 0.0 && !pend) continue;                         // (eig_blk_max's barriers separate the uses of p)
        if (tauj == 0.0)
            for (int i = j + 1 + tid; i < K; i += T) vn[i] = 0.0;
        __syncthreads();
        // one pass over rows c0 .. K - 1, columns c0 .. the diagonal: the pending update, then the products with vn
        const int c0 = j + 1;
        double acc[NACC], vnk[NACC];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int k = c0 + gl + G * q;
            acc[q] = 0.0;
            vnk[q] = k < K ? vn[k] : 0.0;
        }
        double cur[NACC], nxt[NACC];
        {
            const int i = c0 + grp;
#pragma unroll
            for (int q = 0; q < NACC; ++q) {
                const int k = c0 + gl + G * q;
                cur[q] = (i < K && k <= i) ? M.at(i, k) : 0.0;
            }
        }
        for (int i = c0 + grp; i < K; i += NG) {
            const int in = i + NG;                                  // the group's next row travels while this one is used
#pragma unroll
            for (int q = 0; q < NACC; ++q) {
                const int k = c0 + gl + G * q;
                nxt[q] = (in < K && k <= in) ? M.at(in, k) : 0.0;
            }
            const double vni = vn[i];
            double r = 0.0;
            if (pend) {
                const double vpi = vp[i], wi = w[i];
#pragma unroll
                for (int q = 0; q < NACC; ++q) {
                    const int k = c0 + gl + G * q;
                    if (k <= i) {
                        cur[q] -= vpi * w[k] + wi * vp[k];
                        M.at(i, k) = cur[q];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NACC; ++q) {
                const int k = c0 + gl + G * q;
                r = fma(cur[q], vnk[q], r);                         // cur is zero beyond the diagonal
                if (k < i) acc[q] = fma(cur[q], vni, acc[q]);
            }
            r = eig_group_sum<G>(r);
            if (gl == 0) p[i] = r;
#pragma unroll
            for (int q = 0; q < NACC; ++q) cur[q] = nxt[q];
        }
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int k = c0 + gl + G * q;
            if (k < K) part[grp * K + k] = acc[q];
        }
        __syncthreads();
        if (tauj != 0.0) {
            double pd = 0.0;
            for (int k = c0 + tid; k < K; k += T) {
                double s = p[k];
#pragma unroll
                for (int g = 0; g < NG; ++g) s += part[g * K + k];
                s *= tauj;
                p[k] = s;
                pd = fma(s, vn[k], pd);
            }
            const double alpha2 = -0.5 * tauj * eig_blk_sum<T>(pd, red);
            for (int k = c0 + tid; k < K; k += T) w[k] = fma(alpha2, vn[k], p[k]);
        }
        pend = tauj != 0.0;
        double* t = vp; vp = vn; vn = t;
        __syncthreads();
    }
    if (tid == 0) d[K - 1] = M.at(K - 1, K - 1);                    // the last column's pass has applied what was pending
    __syncthreads();
}

// the number of eigenvalues of T below x (dstebz): e2 = the squared off-diagonals
__device__ inline int eig_count(const double* d, const double* e2, int K, double x, double pivmin) {
    double t = d[0] - x;
    if (fabs(t) < pivmin) t = -pivmin;
    int c = t <= 0.0;
    for (int i = 1; i < K; ++i) {
        t = d[i] - e2[i - 1] / t - x;
        if (fabs(t) < pivmin) t = -pivmin;
        c += t <= 0.0;
    }
    return c;
}

// ---- lam[0 .. kk - 1]: the kk largest eigenvalues of T, descending.  e2, lo, hi, cnt: scratch.  Ends with a barrier.
template <int T>
__device__ inline void eig_bisect(const double* d, const double* e, int K, int kk, double* e2, double* lam, double* lo, double* hi,
                                  int* cnt, double* red) {
    constexpr int S = T / DFF_EIG_MAXTOP;                            // shifts per eigenvalue and round
    const int tid = threadIdx.x;
    double me = 0.0, gmin = DBL_MAX, gmax = -DBL_MAX;
    for (int i = tid; i < K; i += T) {
        const double el = i > 0 ? fabs(e[i - 1]) : 0.0, er = i + 1 < K ? fabs(e[i]) : 0.0;
        if (i + 1 < K) { e2[i] = e[i] * e[i]; me = fmax(me, e2[i]); }
        gmin = fmin(gmin, d[i] - el - er);
        gmax = fmax(gmax, d[i] + el + er);
    }
    const double pivmin = DBL_MIN * fmax(1.0, eig_blk_max<T>(me, red));
    double gl = -eig_blk_max<T>(-gmin, red), gu = eig_blk_max<T>(gmax, red);            // Gershgorin
    const double tnorm = fmax(fabs(gl), fabs(gu));
    const double pad = 2.1 * tnorm * 0x1p-52 * K + 2.1 * 2.0 * pivmin;
    gl -= pad;
    gu += pad;
    if (tid < kk) { lo[tid] = gl; hi[tid] = gu; }
    __syncthreads();
    const int j = tid / S, s = tid % S;
    for (int round = 0; round < DFF_EIG_ROUNDS; ++round) {
        double x = 0.0;
        int c = -1;                                                 // -1: at or below lo; K + 1: at or above hi
        if (j < kk) {
            const double a = lo[j], b = hi[j];
            x = a + (b - a) * ((double)(s + 1) / (double)(S + 1));
            if (x >= b) c = K + 1;
            else if (x > a) c = eig_count(d, e2, K, x, pivmin);
        }
        cnt[tid] = c;
        __syncthreads();
        bool open = false;
        if (j < kk && s == 0) {                                     // the first shift with at least K - j eigenvalues below it
            const int want = K - j;
            const double a = lo[j], b = hi[j];
            double na = a, nb = b;
            for (int q = 0; q < S; ++q) {
                const int cq = cnt[j * S + q];
                const double xq = a + (b - a) * ((double)(q + 1) / (double)(S + 1));
                open |= cq >= 0 && cq <= K;
                if (cq >= want) { nb = fmin(nb, xq); break; }
                if (cq >= 0) na = fmax(na, xq);
            }
            lo[j] = na;
            hi[j] = nb;
        }
        if (__syncthreads_or(open) == 0) break;
    }
    if (tid < kk) {                                                 // hi of a closed bracket is the smallest double at or above the
        const double a = lo[tid], b = hi[tid], mid = 0.5 * a + 0.5 * b;   // eigenvalue: exact for a diagonal T
        lam[tid] = (mid > a && mid < b) ? mid : b;
    }
    __syncthreads();
}

__device__ __forceinline__ double eig_start(int i, int j) {         // the start vector of inverse iteration: a fixed hash in (-1, 1)
    unsigned long long h = (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull + (unsigned long long)(j + 1) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31; h *= 0x94D049BB133111EBull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return ((double)(h >> 11) + 0.5) * 0x1p-52 - 1.0;
}

// ---- z_j of T for lam[0 .. kk - 1] into rows j of vout (stride Kmax), unit 2-norm.  lu: 6 K doubles.  Returns false when a
// vector did not reach the growth criterion in DFF_EIG_MAXITS solves.  Ends with a barrier.
template <int T>
__device__ inline bool eig_vectors(const double* d, const double* e, int K, int kk, const double* lam, double* lu,
                                   double* __restrict__ vout, int Kmax, double* red) {
    const int tid = threadIdx.x;
    double* ua = lu;                // U's diagonal
    double* ub = ua + K;            // U's first super-diagonal
    double* uc = ub + K;            // U's second super-diagonal
    double* ml = uc + K;            // the multipliers
    double* sw = ml + K;            // 1.0 where rows i and i + 1 were swapped
    double* x = sw + K;
    double nr = 0.0;
    for (int i = tid; i < K; i += T)
        nr = fmax(nr, fabs(d[i]) + (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < K ? fabs(e[i]) : 0.0));
    double onenrm = eig_blk_max<T>(nr, red);
    if (onenrm == 0.0) onenrm = 1.0;
    const double eps = 0x1p-52, ortol = 1e-3 * onenrm, dtpcrt = sqrt(0.1 / K);
    double xjm = 0.0;
    int gpind = 0;                                                  // the first vector of the current cluster (the growth criterion)
    for (int j = 0; j < kk; ++j) {
        double xj = lam[j];
        if (j > 0) {
            const double pertol = 10.0 * fabs(eps * xj);
            if (xjm - xj < pertol) xj = xjm - pertol;
            if (fabs(xj - xjm) > ortol) gpind = j;
        }
        if (tid == 0) {                                             // P (T - xj I) = L U, rows swapped where the sub-diagonal is larger
            double a = d[0] - xj, b = K > 1 ? e[0] : 0.0, umax = 0.0;
            for (int i = 0; i + 1 < K; ++i) {
                const double c = e[i], an = d[i + 1] - xj, bn = i + 2 < K ? e[i + 1] : 0.0;
                if (fabs(c) <= fabs(a)) {
                    const double mult = a != 0.0 ? c / a : 0.0;
                    ua[i] = a; ub[i] = b; uc[i] = 0.0; ml[i] = mult; sw[i] = 0.0;
                    a = an - mult * b;
                    b = bn;
                } else {
                    const double mult = a / c;
                    ua[i] = c; ub[i] = an; uc[i] = bn; ml[i] = mult; sw[i] = 1.0;
                    a = b - mult * an;
                    b = -mult * bn;
                }
                umax = fmax(umax, fmax(fabs(ua[i]), fmax(fabs(ub[i]), fabs(uc[i]))));
            }
            ua[K - 1] = a; ub[K - 1] = 0.0; uc[K - 1] = 0.0;
            umax = fmax(umax, fabs(a));
            red[15] = eps * fmax(umax, onenrm);                     // a pivot below this is replaced by it (dlagts, job = -1)
        }
        for (int i = tid; i < K; i += T) x[i] = eig_start(i, j);
        __syncthreads();
        const double ptol = red[15], last = fabs(ua[K - 1]);
        int nrmchk = 0;
        bool ok = false;
        for (int its = 0; its < DFF_EIG_MAXITS && !ok; ++its) {
            double m = 0.0;
            for (int i = tid; i < K; i += T) m = fmax(m, fabs(x[i]));
            m = eig_blk_max<T>(m, red);
            if (!(m > 0.0 && m <= DBL_MAX)) break;
            const double scl = (double)K * onenrm * fmax(eps, last) / m;
            for (int i = tid; i < K; i += T) x[i] *= scl;
            __syncthreads();
            if (tid == 0) {
                for (int i = 0; i + 1 < K; ++i) {
                    if (sw[i] == 0.0) x[i + 1] -= ml[i] * x[i];
                    else { const double t = x[i]; x[i] = x[i + 1]; x[i + 1] = t - ml[i] * x[i]; }
                }
                for (int i = K - 1; i >= 0; --i) {
                    double t = x[i];
                    if (i + 1 < K) t -= ub[i] * x[i + 1];
                    if (i + 2 < K) t -= uc[i] * x[i + 2];
                    double ak = ua[i];
                    if (fabs(ak) < ptol) ak = copysign(ptol, ak);
                    x[i] = t / ak;
                }
            }
            __syncthreads();
            for (int c = 0; c < j; ++c) {                           // modified Gram-Schmidt against ALL earlier vectors (see above)
                const double* z = vout + (size_t)c * Kmax;
                double s = 0.0;
                for (int i = tid; i < K; i += T) s = fma(x[i], z[i], s);
                s = eig_blk_sum<T>(s, red);
                for (int i = tid; i < K; i += T) x[i] = fma(-s, z[i], x[i]);
                __syncthreads();
            }
            m = 0.0;
            for (int i = tid; i < K; i += T) m = fmax(m, fabs(x[i]));
            m = eig_blk_max<T>(m, red);
            // dstein's growth criterion.  Member c of a cluster sits c perturbations of 10 ulp away from the cluster, so a solve
            // grows it c times less than the first member: the criterion is scaled by c (a NaN keeps iterating and fails).
            if (!(m * (double)(j - gpind + 1) >= dtpcrt)) continue;
            ok = ++nrmchk >= DFF_EIG_EXTRA + 1;
        }
        double s = 0.0;
        for (int i = tid; i < K; i += T) s = fma(x[i], x[i], s);
        s = sqrt(eig_blk_sum<T>(s, red));
        if (!ok || !(s > 0.0 && s <= DBL_MAX)) return false;        // the same in every thread
        double* z = vout + (size_t)j * Kmax;
        for (int i = tid; i < K; i += T) z[i] = x[i] / s;
        __syncthreads();
        xjm = xj;
    }
    return true;
}

// ---- v = Q z on rows 0 .. kk - 1 of vout, then unit 2-norm and the sign rule.  A vector per group, no barrier.
template <bool LDSP, class Mat>
__device__ inline void eig_back(Mat M, int K, int kk, const double* tau, double* __restrict__ vout, int Kmax) {
    constexpr int G = EigCfg<LDSP>::G, NG = EigCfg<LDSP>::NG, NACC = EigCfg<LDSP>::NACC;
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    for (int c = grp; c < kk; c += NG) {
        double* z = vout + (size_t)c * Kmax;
        double zr[NACC];
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int i = gl + G * q;
            zr[q] = i < K ? z[i] : 0.0;
        }
        for (int j = K - 3; j >= 0; --j) {
            const double t = tau[j];
            if (t == 0.0) continue;
            double vj[NACC], dot = 0.0;
#pragma unroll
            for (int q = 0; q < NACC; ++q) {
                const int i = gl + G * q;
                vj[q] = (i > j + 1 && i < K) ? M.refl(j, i) : (i == j + 1 ? 1.0 : 0.0);
                dot = fma(vj[q], zr[q], dot);
            }
            dot = eig_group_sum<G>(dot) * t;
#pragma unroll
            for (int q = 0; q < NACC; ++q) zr[q] = fma(-dot, vj[q], zr[q]);
        }
        double s = 0.0, best = -1.0;
        int at = 0;
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            s = fma(zr[q], zr[q], s);
            if (fabs(zr[q]) > best) { best = fabs(zr[q]); at = gl + G * q; }   // entries beyond K are zero: they never win
        }
        s = sqrt(eig_group_sum<G>(s));
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
        }
        const int src = (threadIdx.x & 63) - gl + at % G;           // the lane of the group that holds component `at`
        double top = 0.0;
#pragma unroll
        for (int q = 0; q < NACC; ++q)
            if (at / G == q) top = zr[q];
        top = __shfl(top, src, 64);
        const double scl = (top < 0.0 ? -1.0 : 1.0) / s;
#pragma unroll
        for (int q = 0; q < NACC; ++q) {
            const int i = gl + G * q;
            if (i < K) z[i] = zr[q] * scl;
        }
    }
}

// ---- one workgroup per problem.  ks[p] = K_p; a: slots of Kmax^2; w (P, k); v (P, k, Kmax) or NULL.  The workgroup owns the
// problem when own_lo <= K_p <= own_hi, else it leaves at once (the other path's launch takes it).
template <bool LDSP>
__global__ __launch_bounds__(EigCfg<LDSP>::T) void dff_sym_eig_kernel(const double* __restrict__ a, const long long* __restrict__ ks,
                                                                      int Kmax, int k, double* __restrict__ wout,
                                                                      double* __restrict__ vout, int* __restrict__ status,
                                                                      double* work, long long slice, int own_lo, int own_hi) {
    constexpr int T = EigCfg<LDSP>::T, NG = EigCfg<LDSP>::NG;
    extern __shared__ __attribute__((aligned(16))) unsigned char eig_lds[];
    const unsigned pr = blockIdx.x;
    const int K = (int)ks[pr], tid = threadIdx.x;
    if (K < own_lo || K > own_hi) return;
    const int kk = k < K ? k : K;
    double* d = (double*)eig_lds;
    double* e = d + K;
    double* tau = e + K;
    double* va = tau + K;
    double* vb = va + K;
    double* w = vb + K;
    double* p = w + K;
    double* part = p + K;
    double* lam = part + (size_t)NG * K;
    double* lo = lam + DFF_EIG_MAXTOP;
    double* hi = lo + DFF_EIG_MAXTOP;
    double* red = hi + DFF_EIG_MAXTOP;
    int* cnt = (int*)(red + 16);
    double* tri = (double*)(cnt + T);
    const double* A = a + (size_t)pr * Kmax * Kmax;
    double* sl = work + (size_t)pr * slice;
    wout += (size_t)pr * k;
    if (vout) vout += (size_t)pr * k * Kmax;
    typename std::conditional<LDSP, EigLds, EigGlb>::type M;
    if constexpr (LDSP) M = EigLds{tri};
    else M = EigGlb{sl + DFF_EIG_TICKS, Kmax};
    const long long c0 = wall_clock64();
    int bad = 0;                                                    // the working copy of the lower triangle
    for (int idx = tid; idx < K * K; idx += T) {
        const int i = idx / K, c = idx - i * K;
        if (c <= i) {
            const double x = A[idx];
            bad |= !(x - x == 0.0);
            M.at(i, c) = x;
        }
    }
    bad = __syncthreads_or(bad);
    bool vec_ok = true;
    long long c1 = c0, c2 = c0;
    if (!bad) {
        eig_tridiag<LDSP>(M, K, d, e, tau, va, vb, w, p, part, red);
        c1 = wall_clock64();
        eig_bisect<T>(d, e, K, kk, w, lam, lo, hi, cnt, red);
        c2 = wall_clock64();
        if (vout) {
            vec_ok = eig_vectors<T>(d, e, K, kk, lam, part, vout, Kmax, red);
            if (vec_ok) eig_back<LDSP>(M, K, kk, tau, vout, Kmax);
        }
    }
    const double nan = __builtin_nan("");
    for (int j = tid; j < k; j += T) wout[j] = (bad || j >= kk) ? nan : lam[j];
    if (vout)
        for (int idx = tid; idx < k * K; idx += T) {
            const int j = idx / K, i = idx - j * K;
            if (bad || !vec_ok || j >= kk) vout[(size_t)j * Kmax + i] = nan;
        }
    if (tid == 0) {
        status[pr] = bad ? 1 : (vec_ok ? 0 : 2);
        sl[0] = (double)(c1 - c0); sl[1] = (double)(c2 - c1); sl[2] = (double)(wall_clock64() - c2); sl[3] = 0.0;
    }
}
