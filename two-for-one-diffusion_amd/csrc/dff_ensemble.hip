// dff_ensemble.hip -- minimum RMSD over proper rotations between every frame of one ensemble and every frame of another:
// the dense matrix (dff_rmsd_matrix) and, without storing it, the nearest candidate of every query (dff_rmsd_nearest).
//
// Replaces, for (n, N, 3) queries and (m, N, 3) candidates already resident in HBM:
//   md.rmsd(traj, frame) * 10 of evaluate/evaluators.py:656-662, applied once per candidate frame -- on the parent
//   library m launches of dff_struct_rmsd, each re-reading all n query frames.
//
// Arithmetic (per pair the quantity dff_struct_rmsd computes, dff_struct.hip):
//   centring     every frame on its unweighted mean in fp64: the three coordinate sums in bead order, / N; G = sum |a|^2
//                of the centred frame, one fp64 FMA per coordinate in bead order (the same expressions as dff_struct_rmsd)
//   correlation  S_ab = sum_beads a_a b_b, a, b in {x, y, z}, of the centred pair in fp64 on the matrix cores,
//                v_mfma_f64_16x16x4_f64 (operand and result maps: dff_tica.hip's header).  Beads are padded to Np, the
//                next multiple of 4, with zero rows; bead b always sits in k-step b / 4, slot b % 4, so the value of a
//                pair does not depend on the tile, the wave or the workgroup that computes it.
//   RMSD         from S, Ga and Gb by the solver of dff_kabsch.h: lambda_max of Horn's symmetric 4x4 key matrix by cyclic
//                Jacobi (its header says why not Newton on the quartic), msd = (Ga + Gb - 2 lambda) / N
//
// Layout.  One workgroup = 4 waves holds DFF_ENS_TC = 32 candidates, centred, in LDS while 16-query tiles stream past it.
//   LDS image yc[sub][c][bead][16] (sub = which 16 of the 32 candidates, c = x / y / z; frame index fastest), fp64: the B
//   operand of k-step ks and component c is yc[(sub * 3 + c) * 16 Np + 64 ks + lane], 64 consecutive doubles -- each
//   32-lane half of the ds_read_b64 covers the 64 banks once, no padding needed.  | centres (3 x 32) | Gb (32; NaN = the
//   candidate is absent or has a non-finite coordinate).
//   A wave takes 16 queries at a time: lanes 0 .. 47 add up the 48 (frame, component) coordinate sums, each lane fetches
//   the centre of frame lane & 15 with three shuffles, and the A operand of k-step ks, component c is
//   (double) x[q0 + (lane & 15)][4 ks + (lane >> 4)][c] - centre, formed in registers from the fp32 frames (L2-resident:
//   16 frames), zero for padded beads.  The wave's 48 x 48 output is ordered BY COMPONENT: the 16 x 16 MFMA tile (a, b)
//   holds S_ab of the same 16 x 16 pairs at the same lane / register positions, so lane l ends up with all nine S values
//   of its four pairs (query (l >> 4) + 4 r, candidate l & 15) in registers: nine accumulators, no exchange through LDS.
//   The queries' centres and G are thus recomputed once per (query, 32-candidate tile), 1 / 32 per pair: that keeps
//   dff_rmsd_matrix free of a workspace and the two calls on one kernel; the cost is a few per cent of the Jacobi work.
//
// Nearest candidate.  Per query one 64-bit key (fp32 bits of the RMSD << 32 | candidate index), initialised to all ones.
//   Non-negative floats order as unsigned integers, so the smallest key is the smallest RMSD and, among equal RMSDs, the
//   lowest index.  Each lane keeps the minimum over its pairs, the 16 lanes of a query row reduce with shuffles and one lane
//   issues one atomicMin on the query's key.  A minimum of integers does not depend on the order of its operands: the result
//   is the same for every grid size, every split of the candidates and every run.  No floating-point atomics.
#pragma once
#include "dff_internal.h"
#include "dff_kabsch.h"
#include "dff_frames.h"   // f64x4

#define DFF_ENS_THREADS 256
#define DFF_ENS_TC 32              // candidates per workgroup: two 16-column MFMA tiles
#define DFF_ENS_TQ 16              // queries per wave pass: one 16-row MFMA tile
#define DFF_ENS_WGS 4096           // workgroups a launch aims for when the candidate tiles alone are fewer
#define DFF_ENS_QCHUNK (1LL << 20) // queries per launch of dff_rmsd_nearest: bounds the key workspace (8 MB)
#define DFF_ENS_NOKEY 0xffffffffffffffffULL

__host__ __device__ __forceinline__ int ens_np(int N) { return (N + 3) & ~3; }
// LDS doubles: yc | centres | Gb
__host__ __device__ __forceinline__ int ens_lds_doubles(int Np) { return DFF_ENS_TC * 3 * Np + 3 * DFF_ENS_TC + DFF_ENS_TC; }

// grid = nct * qsplit: workgroup (ct, qs) pairs candidate tile ct with the query tiles qs * 4 + wave, + 4 qsplit, ...
// The RMSD of a pair comes from its correlation matrix S (row = component of the query, column = component of the
// candidate) by the same calls on both paths, so that they agree bit for bit.
// NEAREST: keys[q] = min(keys[q], key of the pair), the pair (q, self_first + q) left out when self_first >= 0.
// else:    out[q * m + cand] = RMSD, NaN where either frame has a non-finite coordinate.
template <bool NEAREST>
__global__ __launch_bounds__(DFF_ENS_THREADS) void dff_ens_rmsd_kernel(const float* __restrict__ x, long long n,
                                                                       const float* __restrict__ y, long long m, int N,
                                                                       int qsplit, long long self_first,
                                                                       float* __restrict__ out,
                                                                       unsigned long long* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) double ens_lds[];
    const int Np = ens_np(N), N3 = 3 * N, KS = Np >> 2;
    double* yc = ens_lds;
    double* cen = ens_lds + DFF_ENS_TC * 3 * Np;
    double* GbL = cen + 3 * DFF_ENS_TC;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long ct = blockIdx.x / qsplit;
    const int qs = (int)(blockIdx.x - ct * qsplit);
    const long long c0 = ct * DFF_ENS_TC;
    const int cc = (int)(m - c0 < DFF_ENS_TC ? m - c0 : DFF_ENS_TC);

    // ---- the candidate tile: centres, centred image, Gb
    if (tid < 3 * DFF_ENS_TC) {
        const int f = tid & (DFF_ENS_TC - 1), c = tid / DFF_ENS_TC;
        double s = 0.0;
        if (f < cc) {
            const float* p = y + (c0 + f) * N3 + c;
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
            v = (double)y[(c0 + f) * N3 + 3 * bead + c] - (c == 0 ? m0 : c == 1 ? m1 : m2);
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
    const long long nqt = (n + DFF_ENS_TQ - 1) / DFF_ENS_TQ;
    const int qi = lane & 15, kq = lane >> 4;
    for (long long qt = (long long)qs * 4 + wave; qt < nqt; qt += 4LL * qsplit) {
        const long long q0 = qt * DFF_ENS_TQ;
        const int qc = (int)(n - q0 < DFF_ENS_TQ ? n - q0 : DFF_ENS_TQ);
        const float* xq = x + (q0 + qi) * N3;            // frame lane & 15 (dereferenced only when qi < qc)
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
        for (int r = 0; r < 4; ++r) GaR[r] = __shfl(Ga, kq + 4 * r);     // the query of this lane's result row r
        unsigned long long best[4] = {DFF_ENS_NOKEY, DFF_ENS_NOKEY, DFF_ENS_NOKEY, DFF_ENS_NOKEY};
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
            const int col = sub * 16 + qi;                 // result column lane & 15: the candidate
            const double Gb = GbL[col];
            const long long cand = c0 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = kq + 4 * r;                // result row: the query
                const bool fin = GaR[r] == GaR[r] && Gb == Gb;
                float d = __builtin_nanf("");
                if (fin) {
                    const Sym4 K = horn_key(S[0][0][r], S[0][1][r], S[0][2][r], S[1][0][r], S[1][1][r], S[1][2][r], S[2][0][r],
                                            S[2][1][r], S[2][2][r]);
                    d = kabsch_rmsd(GaR[r], Gb, sym4_jacobi<false>(K), N);
                }
                if (NEAREST) {
                    if (fin && !(self_first >= 0 && cand == self_first + q0 + row)) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)cand;
                        best[r] = key < best[r] ? key : best[r];
                    }
                } else if (row < qc && col < cc) {
                    out[(q0 + row) * m + cand] = d;
                }
            }
        }
        if (NEAREST) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                unsigned long long k = best[r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    const unsigned long long other = __shfl_xor(k, o);
                    k = other < k ? other : k;
                }
                if (qi == 0 && kq + 4 * r < qc && k != DFF_ENS_NOKEY) atomicMin(&keys[q0 + kq + 4 * r], k);
            }
        }
    }
}

// keys -> (rmsd, index): a key still all ones (no usable candidate, or a query with a non-finite coordinate) gives NaN, -1
__global__ __launch_bounds__(256) void dff_ens_finish_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                             float* __restrict__ rmsd, long long* __restrict__ index) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const unsigned long long k = keys[s];
    const bool none = k == DFF_ENS_NOKEY;
    rmsd[s] = none ? __builtin_nanf("") : __uint_as_float((unsigned)(k >> 32));
    if (index) index[s] = none ? -1LL : (long long)(k & 0xffffffffULL);
}
