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
//   distance   pwd_dist2 (dff_pwd.hip): sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) in fp32, bit-equal to torch.norm
//   dihedral   mdtraj's formula in fp32: b1 = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3, c2 = b1 x b2,
//              phi = atan2((b1 . c1) |b2|, c1 . c2), no FMA contraction (the same bits in every kernel that uses it)
//   RMSD       fp64 centring, 3x3 correlation and inner products; the minimum over proper rotations by the solver of
//              dff_kabsch.h (lambda_max of Horn's key matrix by cyclic Jacobi: its header says why not Newton)
//   TIC        features (N - 3 dihedrals, then the N (N - 1) / 2 distances in triu_indices(N, N, 1) order) in fp32,
//              never stored; out[s, c] = sum_f ((double) feat_f - mean_f) * A[f, c] accumulated in fp64
#pragma once
#include "dff_internal.h"
#include "dff_kabsch.h"
#include "dff_pwd.hip"   // pwd_dist2, f32x4

#define DFF_STRUCT_TILE 64     // frames per tile = lanes per workgroup (one wave)
#define DFF_TIC_MAXK 8         // TIC components per call

__host__ __device__ __forceinline__ int struct_ld(int N) { return (3 * N) | 1; }

// TIC features of an N-bead frame (N >= 4): the dihedrals and the pair distances
__host__ __device__ inline int struct_tic_num_features(int N) { return (N - 3) + N * (N - 1) / 2; }

// the last r in 0 .. n - 1 with start[r] <= v (start ascending, start[0] <= v)
template <class T>
__device__ __forceinline__ int last_le(const T* start, int n, T v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sum over the wave by a butterfly: the same tree, and the same bits, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// The flat elements 0 .. cnt * 3N - 1 of a tile's frames in global memory, dealt to the 64 lanes in coalesced order:
// quad(k, at) for elements 4 k .. 4 k + 3 (one 16-byte access; vec4 only), one(k, at(k)) for the rest.  at(f) is where flat
// element f sits in LDS, s * ld + offset within frame s.  magic = ceil(2^32 / 3N): the frame of flat element f < 64 * 3N is
// __umulhi(f, magic) exactly (the rounding error f / 2^32 < 1 / 3N).
template <class Quad, class One>
__device__ __forceinline__ void struct_tile_walk(int cnt, int N3, int ld, unsigned magic, bool vec4, Quad quad, One one) {
    const auto at = [=](unsigned f) {
        const unsigned s = __umulhi(f, magic);
        return s * ld + (f - s * N3);
    };
    const int nf = cnt * N3;
    int k0 = 0;
    if (vec4) {
        const int n4 = nf >> 2;
        for (int k = threadIdx.x; k < n4; k += DFF_STRUCT_TILE) quad(k, at);
        k0 = n4 << 2;
    }
    for (int k = k0 + threadIdx.x; k < nf; k += DFF_STRUCT_TILE) one(k, at((unsigned)k));
}

// coalesced load of cnt frames starting at s0 into tile[s * ld + k]
__device__ __forceinline__ void struct_load_tile(float* tile, const float* __restrict__ x, long long s0, int cnt,
                                                 int N3, int ld, unsigned magic, bool vec4) {
    const float* src = x + s0 * N3;
    struct_tile_walk(
        cnt, N3, ld, magic, vec4,
        [&](int k, auto at) {
            const f32x4 v = __builtin_nontemporal_load((const f32x4*)src + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[at((unsigned)(4 * k + e))] = v[e];
        },
        [&](int k, unsigned o) { tile[o] = src[k]; });
}

// its counterpart: coalesced store of the cnt frames in tile to dst + s0 * 3N
__device__ __forceinline__ void struct_store_tile(const float* tile, float* dst, long long s0, int cnt, int N3, int ld,
                                                  unsigned magic, bool vec4) {
    dst += s0 * N3;
    struct_tile_walk(
        cnt, N3, ld, magic, vec4,
        [&](int k, auto at) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = tile[at((unsigned)(4 * k + e))];
            *((f32x4*)dst + k) = v;
        },
        [&](int k, unsigned o) { dst[k] = tile[o]; });
}

// Each product and sum rounded on its own, as numpy's float32 formula (mdtraj) rounds it: without the pragma, which
// products the compiler fuses into FMAs depends on how it packs the code around the call, and the TIC projection,
// the dihedral and the TIC feature kernels would differ from one another by a few ulps.
__device__ __forceinline__ float struct_dihedral(const float* xs, int i) {
#pragma clang fp contract(off)
    const float* p = xs + 3 * i;
    const float b1x = p[3] - p[0], b1y = p[4] - p[1], b1z = p[5] - p[2];
    const float b2x = p[6] - p[3], b2y = p[7] - p[4], b2z = p[8] - p[5];
    const float b3x = p[9] - p[6], b3y = p[10] - p[7], b3z = p[11] - p[8];
    const float c1x = b2y * b3z - b2z * b3y, c1y = b2z * b3x - b2x * b3z, c1z = b2x * b3y - b2y * b3x;
    const float c2x = b1y * b2z - b1z * b2y, c2y = b1z * b2x - b1x * b2z, c2z = b1x * b2y - b1y * b2x;
    const float p1 = (b1x * c1x + b1y * c1y + b1z * c1z) * sqrtf(b2x * b2x + b2y * b2y + b2z * b2z);
    const float p2 = c1x * c2x + c1y * c2y + c1z * c2z;
    return atan2f(p1, p2);
}

// the TIC features of the frame xs in order, fn(f, value): dihedrals 0 .. N - 4, then the distances in
// triu_indices(N, N, 1) order
template <class Fn>
__device__ __forceinline__ void struct_tic_walk(const float* xs, int N, Fn fn) {
    int f = 0;
    for (; f < N - 3; ++f) fn(f, struct_dihedral(xs, f));
    for (int i = 0; i < N - 1; ++i)
        for (int j = i + 1; j < N; ++j, ++f) fn(f, pwd_dist2(xs, 3 * i, 3 * j));
}

// acc[c] = sum_f ((double) feat_f - mean_f) * A[f, c], c < k: one fp64 FMA per feature and component, in feature order
__device__ __forceinline__ void struct_tic_project(const float* xs, int N, const double* __restrict__ mean,
                                                   const double* __restrict__ A, int k, double (&acc)[DFF_TIC_MAXK]) {
#pragma unroll
    for (int c = 0; c < DFF_TIC_MAXK; ++c) acc[c] = 0.0;
    struct_tic_walk(xs, N, [&](int f, float feat) {
        const double v = (double)feat - mean[f];
#pragma unroll
        for (int c = 0; c < DFF_TIC_MAXK; ++c)
            if (c < k) acc[c] = fma(v, A[(size_t)f * k + c], acc[c]);
    });
}

// grid-stride loop over tiles: body(s0, cnt, lane, live, xs) once per tile, xs = this lane's frame in LDS
template <class Body>
__device__ __forceinline__ void struct_tiles(float* tile, const float* __restrict__ x, long long n, int N, unsigned magic,
                                             int vec4, Body body) {
    const int N3 = 3 * N, ld = struct_ld(N);
    const long long ntiles = (n + DFF_STRUCT_TILE - 1) / DFF_STRUCT_TILE;
    const int lane = threadIdx.x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long s0 = t * DFF_STRUCT_TILE;
        const int cnt = (int)(n - s0 < DFF_STRUCT_TILE ? n - s0 : DFF_STRUCT_TILE);
        __syncthreads();
        struct_load_tile(tile, x, s0, cnt, N3, ld, magic, vec4 != 0);
        __syncthreads();
        body(s0, cnt, lane, lane < cnt, (const float*)(tile + lane * ld));
    }
}

// ---- RMSD to a reference structure (fp64; the solver is dff_kabsch.h).  LDS: tile | centred reference (N x 3 doubles)
// Centre the reference into rc (every lane the same sums, in bead order: no reduction order to depend on) and hand out
// its centroid.  The caller synchronises before rc is read.
__device__ __forceinline__ void struct_centre_ref(const float* __restrict__ ref, int N, double* rc, double& m0, double& m1,
                                                  double& m2) {
    m0 = 0; m1 = 0; m2 = 0;
    for (int b = 0; b < N; ++b) { m0 += ref[3 * b]; m1 += ref[3 * b + 1]; m2 += ref[3 * b + 2]; }
    m0 /= N; m1 /= N; m2 /= N;
    for (int b = threadIdx.x; b < N; b += DFF_STRUCT_TILE) {
        rc[3 * b] = ref[3 * b] - m0;
        rc[3 * b + 1] = ref[3 * b + 1] - m1;
        rc[3 * b + 2] = ref[3 * b + 2] - m2;
    }
}

// Gb = sum |r_b|^2 of the centred reference
__device__ __forceinline__ double struct_ref_norm2(const double* rc, int N) {
    double Gb = 0;
    for (int b = 0; b < N; ++b) Gb += rc[3 * b] * rc[3 * b] + rc[3 * b + 1] * rc[3 * b + 1] + rc[3 * b + 2] * rc[3 * b + 2];
    return Gb;
}

// One frame xs against the centred reference rc: Horn's key matrix of their correlation.  Also hands out the frame's
// centroid c and Ga = sum |a_b|^2 of the centred frame, and clears `finite` when a coordinate is not finite.
__device__ __forceinline__ Sym4 struct_frame_key(const float* xs, const double* rc, int N, bool& finite, double& c0,
                                                 double& c1, double& c2, double& Ga) {
    c0 = 0; c1 = 0; c2 = 0;
    for (int b = 0; b < N; ++b) {
        const float a0 = xs[3 * b], a1 = xs[3 * b + 1], a2 = xs[3 * b + 2];
        finite = finite && isfinite(a0) && isfinite(a1) && isfinite(a2);
        c0 += a0; c1 += a1; c2 += a2;
    }
    c0 /= N; c1 /= N; c2 /= N;
    Ga = 0;
    double Sxx = 0, Sxy = 0, Sxz = 0, Syx = 0, Syy = 0, Syz = 0, Szx = 0, Szy = 0, Szz = 0;
    for (int b = 0; b < N; ++b) {
        const double a0 = xs[3 * b] - c0, a1 = xs[3 * b + 1] - c1, a2 = xs[3 * b + 2] - c2;
        const double r0 = rc[3 * b], r1 = rc[3 * b + 1], r2 = rc[3 * b + 2];
        Ga = fma(a0, a0, fma(a1, a1, fma(a2, a2, Ga)));
        Sxx = fma(a0, r0, Sxx); Sxy = fma(a0, r1, Sxy); Sxz = fma(a0, r2, Sxz);
        Syx = fma(a1, r0, Syx); Syy = fma(a1, r1, Syy); Syz = fma(a1, r2, Syz);
        Szx = fma(a2, r0, Szx); Szy = fma(a2, r1, Szy); Szz = fma(a2, r2, Szz);
    }
    return horn_key(Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz);
}

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
