// dff_superpose.hip -- optimal superposition of every frame on one reference structure: the rotation that the RMSD
// kernels solve for and throw away, the frames moved into the reference's frame, and the sums a mean structure and a
// per-bead fluctuation (RMSF) are made of.
//
// Replaces, for (n, N, 3) structures already resident in HBM:
//   traj.superpose(traj, 0)                      datasets/dataset_utils_empty.py:319-321
//
// Layout: that of dff_struct_rmsd_kernel (dff_struct.hip) -- one wave per workgroup, one lane per frame, the 64-frame
// tile streamed into LDS with struct_load_tile (odd leading dimension), a grid-stride loop over tiles, the reference
// centred once per workgroup.  Per finite frame, all in fp64: centre on the unweighted mean, the 3 x 3 correlation and
// Horn's 4 x 4 key matrix K by the functions dff_struct_rmsd_kernel calls (struct_frame_key), then the solver of
// dff_kabsch.h with the eigenvector: cyclic Jacobi on K with the plane rotations accumulated, the eigenvector of the
// largest eigenvalue as a unit quaternion q, and R quadratic in q (a half turn, a collinear frame: see that header).
//   K = 0 (all beads coincident): no sweep runs, q = (1, 0, 0, 0), R = I.
//
// Outputs.  The rotated frame goes back into the lane's own row of the tile (each bead is read before it is written, and
// a row belongs to one lane), then the tile is stored with coalesced 16-byte writes: the whole tile is in LDS before any
// of it is written and tiles are disjoint, which is what makes aligned == x (in place) legal.
// Statistics: d = R (x_b - c_x) - (ref_b - c_ref) in fp64, before any rounding to fp32.  Beads go through an fp64 staging
// buffer eight at a time (64 frames x 32 columns: 24 coordinates of d, 8 values |d_b|^2; leading dimension 33 doubles);
// lane l adds column l & 31 over frames 32 (l >> 5) .. + 31 in order, the two halves meet in one shuffle, and the sum is
// added to the workgroup's fp64 accumulators in LDS.  A lane without a finite frame stages zeros.  At the end the
// workgroup writes its 4 N + 1 partials (3 N of dsum, N of dsq, the frame count as a 64-bit integer in the same 8-byte
// slot) to its slice of the workspace; dff_superpose_reduce_kernel adds the slices in a fixed order.  No atomics.
//
// LDS bytes: reference 8 (3 N rounded up to even) | tile 256 (3 N | 1) | with statistics: staging 64 * 33 * 8 = 16 896 |
// accumulators 32 N
//   N = 10:   240 +  7 936 (+ 16 896 +   320) =  8 176 / 25 392
//   N = 35:   848 + 26 880 (+ 16 896 + 1 120) = 27 728 / 45 744
//   N = 64: 1 536 + 49 408 (+ 16 896 + 2 048) = 50 944 / 69 888        (limit 163 840)
#pragma once
#include "dff_frames.h"   // struct_tiles, struct_store_tile, struct_centre_ref, struct_frame_key

#define DFF_SUP_WGS 4096          // workgroups at most: each owns one slice of partials in the workspace
#define DFF_SUP_CB 8              // beads per pass through the staging buffer
#define DFF_SUP_COLS (4 * DFF_SUP_CB)
#define DFF_SUP_LDS (DFF_SUP_COLS + 1)   // leading dimension of the staging buffer in doubles: odd

__host__ __device__ __forceinline__ int superpose_ref_doubles(int N) { return (3 * N + 1) & ~1; }   // 16-byte multiple
__host__ __device__ __forceinline__ int superpose_per(int N) { return 4 * N + 1; }

// x and aligned are NOT __restrict__: they may be the same pointer.
// part == NULL: no statistics (and no staging buffer / accumulators behind the tile).
__global__ __launch_bounds__(DFF_STRUCT_TILE) void dff_superpose_kernel(const float* x, long long n, int N,
                                                                         const float* __restrict__ ref, float* aligned,
                                                                         double* __restrict__ rot,
                                                                         float* __restrict__ rmsd,
                                                                         double* __restrict__ part, int vec4_out,
                                                                         unsigned magic, int vec4) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N3 = 3 * N, ld = struct_ld(N);
    double* rc = (double*)smem;                              // N * 3 centred reference coordinates
    float* tile = smem + 2 * superpose_ref_doubles(N);
    double* stage = (double*)(tile + DFF_STRUCT_TILE * ld);  // 64 x DFF_SUP_LDS      (64 * ld floats: a multiple of 16 bytes)
    double* acc = stage + DFF_STRUCT_TILE * DFF_SUP_LDS;     // 4 N: dsum | dsq
    double m0, m1, m2;
    struct_centre_ref(ref, N, rc, m0, m1, m2);
    const bool ref_ok = isfinite(m0) && isfinite(m1) && isfinite(m2);   // fp64 sums of floats do not overflow
    if (part)
        for (int i = threadIdx.x; i < 4 * N; i += DFF_STRUCT_TILE) acc[i] = 0.0;
    __syncthreads();
    const double Gb = struct_ref_norm2(rc, N);
    unsigned long long nfin = 0ull;                          // finite frames of this workgroup's tiles (the same in every lane)
    const int nch = (N + DFF_SUP_CB - 1) / DFF_SUP_CB;
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs_) {
        float* xs = tile + lane * ld;                         // this lane's row: read as the frame, written as its image
        bool finite = live && ref_ok;
        double c0 = 0, c1 = 0, c2 = 0;
        double R[9];
        if (live) {
            double Ga;
            const Sym4 K = struct_frame_key(xs, rc, N, finite, c0, c1, c2, Ga);
            double q[4] = {1.0, 0.0, 0.0, 0.0};
            const double l = finite ? sym4_jacobi<true>(K, q) : 0.0;   // the quaternion of the optimal proper rotation
            quat_to_rot(q, R);
            if (rmsd) rmsd[s0 + lane] = finite ? kabsch_rmsd(Ga, Gb, l, N) : __builtin_nanf("");
            if (rot) {
                double* o = rot + (s0 + lane) * 9;
#pragma unroll
                for (int e = 0; e < 9; ++e) o[e] = finite ? R[e] : __builtin_nan("");
            }
        }
        if (part) nfin += (unsigned long long)__popcll(__ballot(finite));
        if (!aligned && !part) return;                        // wave-uniform
        // the image of every bead: into the lane's row (fp32, one rounding) and, eight beads at a time, through the staging
        // buffer into the column sums
        for (int ch = 0; ch < nch; ++ch) {
            const int b0 = ch * DFF_SUP_CB, b1 = b0 + DFF_SUP_CB < N ? b0 + DFF_SUP_CB : N;
            if (live)
                for (int b = b0; b < b1; ++b) {
                    const double a0 = xs[3 * b] - c0, a1 = xs[3 * b + 1] - c1, a2 = xs[3 * b + 2] - c2;
                    const double y0 = fma(R[0], a0, fma(R[1], a1, R[2] * a2));
                    const double y1 = fma(R[3], a0, fma(R[4], a1, R[5] * a2));
                    const double y2 = fma(R[6], a0, fma(R[7], a1, R[8] * a2));
                    if (aligned) {
                        xs[3 * b] = finite ? (float)(y0 + m0) : __builtin_nanf("");
                        xs[3 * b + 1] = finite ? (float)(y1 + m1) : __builtin_nanf("");
                        xs[3 * b + 2] = finite ? (float)(y2 + m2) : __builtin_nanf("");
                    }
                    if (part) {
                        const double d0 = finite ? y0 - rc[3 * b] : 0.0, d1 = finite ? y1 - rc[3 * b + 1] : 0.0;
                        const double d2 = finite ? y2 - rc[3 * b + 2] : 0.0;
                        double* st = stage + lane * DFF_SUP_LDS;
                        st[3 * (b - b0)] = d0; st[3 * (b - b0) + 1] = d1; st[3 * (b - b0) + 2] = d2;
                        st[3 * DFF_SUP_CB + (b - b0)] = fma(d0, d0, fma(d1, d1, d2 * d2));
                    }
                }
            if (part) {
                if (!live) {
                    double* st = stage + lane * DFF_SUP_LDS;
                    for (int c = 0; c < DFF_SUP_COLS; ++c) st[c] = 0.0;
                }
                __syncthreads();
                // column c of this pass: coordinate 3 b0 + c of dsum (c < 24), bead b0 + c - 24 of dsq
                const int c = lane & (DFF_SUP_COLS - 1), half = lane >> 5;
                const int bead = c < 3 * DFF_SUP_CB ? b0 + c / 3 : b0 + c - 3 * DFF_SUP_CB;
                const int slot = c < 3 * DFF_SUP_CB ? 3 * b0 + c : N3 + b0 + c - 3 * DFF_SUP_CB;
                double sum = 0.0;
                if (bead < b1) {
                    const double* col = stage + half * 32 * DFF_SUP_LDS + c;
                    for (int i = 0; i < 32; ++i) sum += col[i * DFF_SUP_LDS];
                }
                sum += __shfl_xor(sum, 32);
                if (bead < b1 && half == 0) acc[slot] += sum;
                __syncthreads();
            }
        }
        if (aligned) {
            __syncthreads();
            struct_store_tile(tile, aligned, s0, cnt, N3, ld, magic, vec4_out != 0);
        }
    });
    if (part) {
        __syncthreads();
        const int per = superpose_per(N);
        double* dst = part + (size_t)blockIdx.x * per;
        for (int i = threadIdx.x; i < 4 * N; i += DFF_STRUCT_TILE) dst[i] = acc[i];
        if (threadIdx.x == 0) *(unsigned long long*)(dst + 4 * N) = nfin;
    }
}

// ---- slices -> results.  One wave per accumulator, as dff_kmeans_reduce_kernel: lane l adds slices l, l + 64, ... in that
// order, then the butterfly over the wave -- one fixed tree per slice count.  The results are overwritten.
__global__ __launch_bounds__(64) void dff_superpose_reduce_kernel(const double* __restrict__ part, int nslices, int N,
                                                                  double* __restrict__ dsum, double* __restrict__ dsq,
                                                                  unsigned long long* __restrict__ count) {
    const int per = superpose_per(N);
    const int i = blockIdx.x, lane = threadIdx.x;              // grid = per
    if (i == 4 * N) {
        unsigned long long c = 0ull;
        for (int g = lane; g < nslices; g += 64) c += ((const unsigned long long*)part)[(size_t)g * per + i];
        c = wave_sum(c);
        if (count && lane == 0) count[0] = c;
    } else {
        double s = 0.0;
        for (int g = lane; g < nslices; g += 64) s += part[(size_t)g * per + i];
        s = wave_sum(s);
        if (lane == 0) {
            if (i < 3 * N) { if (dsum) dsum[i] = s; }
            else if (dsq) dsq[i - 3 * N] = s;
        }
    }
}
