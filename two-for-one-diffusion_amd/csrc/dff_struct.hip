// dff_struct.hip -- per-frame structure metrics of the reference's evaluators on the GPU.
//
// Replaces, for (n, N, 3) structures already resident in HBM:
//   md.rmsd(traj, folded) * 10                   evaluate/evaluators.py:656-662  (RmsdEvaluator.eval)
//   md.compute_dihedrals(traj, [[i..i+3]])       evaluate/evaluators_CGflowmatching.py:30-36, evaluators.py:433-445
//   tica.transform(get_tic_features(xyz))        evaluate/evaluators.py:433-445, :460-461  (TicEvaluator)
//   _get_samp_contacts + sum / _eval_bce_dynamics evaluate/evaluators.py:781-806, :829-859  (ContactEvaluator)
// The small histogram and divergence reductions stay on the host (evaluate.py); only (n,) / (n, k)-sized
// results and one (N, N) count matrix come back.
//
// Layout of every kernel: one wave per workgroup, one lane per frame.  A tile of 64 frames is streamed
// into LDS with coalesced 16-byte loads; frame s of the tile sits at tile[s * ld], ld = 3N | 1 (an odd
// stride: the 64 lanes read 64 different banks).  Everything that loops over beads, pairs or features is
// then uniform across the wave, so per-bead / per-feature constants (the reference structure, the TICA
// mean and coefficients, the folded contact map) are wave-uniform loads.  No MFMA: this is HBM-bound work
// (TIC at protein-G size is bound by its fp64 loop instead).
//
// Arithmetic:
//   distance   pwd_dist2 (dff_frames.h): sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) in fp32, bit-equal to torch.norm
//   dihedral   mdtraj's formula in fp32: b1 = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3, c2 = b1 x b2,
//              phi = atan2((b1 . c1) |b2|, c1 . c2), no FMA contraction (the same bits in every kernel that uses it)
//   RMSD       fp64 centring, 3x3 correlation and inner products; the minimum over proper rotations by the solver of
//              dff_kabsch.h (lambda_max of Horn's key matrix by cyclic Jacobi: its header says why not Newton)
//   TIC        features (N - 3 dihedrals, then the N (N - 1) / 2 distances in triu_indices(N, N, 1) order) in fp32,
//              never stored; out[s, c] = sum_f ((double) feat_f - mean_f) * A[f, c] accumulated in fp64
#pragma once
#include "dff_internal.h"
#include "dff_kabsch.h"
#include "dff_frames.h"   // the tile machinery, struct_dihedral, struct_tic_project, struct_frame_key, pwd_dist2

// ---- RMSD to a reference structure (fp64; the solver is dff_kabsch.h).  LDS: tile | centred reference (N x 3 doubles)
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_rmsd_kernel(const float* __restrict__ x, long long n,
                                                                           int N, const float* __restrict__ ref,
                                                                           float* __restrict__ out, unsigned magic,
                                                                           int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    double* rc = (double*)smem;                              // N * 3 centred reference coordinates
    float* tile = smem + ((6 * N + 3) & ~3);
    double m0, m1, m2;
    struct_centre_ref(ref, N, rc, m0, m1, m2);
    __syncthreads();
    const double Gb = struct_ref_norm2(rc, N);
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        if (live) {
            bool finite = true;
            double c0, c1, c2, Ga;
            const Sym4 K = struct_frame_key(xs, rc, N, finite, c0, c1, c2, Ga);
            const double l = finite ? sym4_jacobi<false>(K) : 0.0;
            out[s0 + lane] = finite ? kabsch_rmsd(Ga, Gb, l, N) : __builtin_nanf("");
        }
    });
}

// ---- dihedrals of consecutive quadruples.  LDS: tile | out staging (64 x (N - 3))
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_dihedrals_kernel(const float* __restrict__ x, long long n,
                                                                                int N, float* __restrict__ out,
                                                                                unsigned magic, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tile = smem;
    const int nd = N - 3;
    float* stage = smem + DFF_STRUCT_TILE * struct_ld(N);
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        if (live)
            for (int i = 0; i < nd; ++i) stage[lane * nd + i] = struct_dihedral(xs, i);
        __syncthreads();
        float* dst = out + s0 * nd;
        for (int k = lane; k < cnt * nd; k += DFF_STRUCT_TILE) dst[k] = stage[k];
    });
}

// ---- TIC projection.  LDS: tile.  mean (F,), A (F, k) row-major: wave-uniform loads
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_tic_kernel(const float* __restrict__ x, long long n, int N,
                                                                          const double* __restrict__ mean,
                                                                          const double* __restrict__ A, int k,
                                                                          double* __restrict__ out, unsigned magic,
                                                                          int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* tile = smem;
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        if (live) {
            double acc[DFF_TIC_MAXK];
            struct_tic_project(xs, N, mean, A, k, acc);
            double* o = out + (s0 + lane) * k;
#pragma unroll
            for (int c = 0; c < DFF_TIC_MAXK; ++c)
                if (c < k) o[c] = acc[c];
        }
    });
}

// ---- contacts d_ij < cutoff.  LDS: tile | counts (N x N, upper triangle incl. diagonal) | folded map (N x N bytes)
// The contact bit of pair (i, j) is uniform in (i, j): the wave's count over its 64 frames is one ballot + popcount,
// added by lane 0 to the workgroup's private LDS counter; the counters go out with one atomic each at the end.
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_struct_contacts_kernel(const float* __restrict__ x, long long n,
                                                                               int N, float cutoff,
                                                                               const unsigned char* __restrict__ folded,
                                                                               int offset, unsigned* __restrict__ counts,
                                                                               unsigned* __restrict__ mismatch,
                                                                               unsigned magic, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned* cl = (unsigned*)smem;                                  // N * N
    unsigned char* fl = (unsigned char*)(cl + N * N);               // N * N (rounded up to 16 bytes)
    float* tile = (float*)(fl + ((N * N + 15) & ~15));
    for (int k = threadIdx.x; k < N * N; k += DFF_STRUCT_TILE) {
        cl[k] = 0u;
        fl[k] = folded ? folded[k] : (unsigned char)0;
    }
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs) {
        unsigned mis = 0;
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) {
                const bool c = live && pwd_dist2(xs, 3 * i, 3 * j) < cutoff;
                const unsigned long long bal = __ballot(c);
                if (lane == 0 && bal) cl[i * N + j] += (unsigned)__popcll(bal);
                if (j >= i + offset) mis += (unsigned)(c != (fl[i * N + j] != 0));
            }
        if (mismatch && live) mismatch[s0 + lane] = mis;
    });
    __syncthreads();
    for (int k = threadIdx.x; k < N * N; k += DFF_STRUCT_TILE) {
        const int i = k / N, j = k - i * N;
        if (j < i) continue;
        const unsigned v = cl[k];
        if (v) {
            atomicAdd(&counts[k], v);
            if (j != i) atomicAdd(&counts[j * N + i], v);
        }
    }
}
