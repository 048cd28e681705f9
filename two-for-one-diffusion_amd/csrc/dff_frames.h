// dff_frames.h -- what the sample-analysis kernel files share on the device, whatever their family: the small vector types,
// the wave butterfly, the search in an ascending table, and the frame-tile machinery of the structure kernels with the
// per-frame arithmetic (distance, dihedral, TIC features and projection, Horn's key matrix against a reference) that every
// kernel over (n, N, 3) frames must do with the same bits.  Device helpers and template code only: no kernel lives here.
//
// Tile layout: one wave per workgroup, one lane per frame.  A tile of 64 frames is streamed into LDS with coalesced 16-byte
// loads; frame s of the tile sits at tile[s * ld], ld = 3N | 1 (an odd stride: the 64 lanes read 64 different banks).
#pragma once
#include "dff_internal.h"
#include "dff_kabsch.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// distance of two beads of a frame, bit-equal to torch.norm in fp32 (dff_pwd.hip says what is pinned)
__device__ __forceinline__ float pwd_dist2(const float* xs, int oi, int oj) {
    const float* a = xs + oi;
    const float* b = xs + oj;
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    // sqrtf and '/' are correctly rounded here (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt);
    // the __fsqrt_rn / __fdiv_rn intrinsics are NOT (they lower to the fast native ops)
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

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

// ---- a frame against a reference structure (fp64; the solver is dff_kabsch.h)
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
