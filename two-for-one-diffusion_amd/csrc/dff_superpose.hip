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
// Horn's 4 x 4 key matrix K exactly as dff_struct_rmsd_kernel builds them, cyclic Jacobi on K with the plane rotations
// accumulated into the 4 x 4 eigenvector matrix (the rotation formula, the sweep cap and the stop rule of
// sym4_lambda_max), the eigenvector of the largest eigenvalue as a unit quaternion q, and R from the formula that is
// QUADRATIC in q: no division by q0, so a half turn (q0 = 0) is an ordinary input.
//   K = 0 (all beads coincident): no sweep runs, q = (1, 0, 0, 0), R = I.
//   degenerate largest eigenvalue (collinear frame or reference): Jacobi still ends with an orthonormal eigenbasis; the
//   column it ends with is A maximiser -- a proper rotation that reaches the minimal RMSD, one of a continuum.
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
#include "dff_struct.hip"
#include "dff_states.hip"   // wave_sum

#define DFF_SUP_WGS 4096          // workgroups at most: each owns one slice of partials in the workspace
#define DFF_SUP_CB 8              // beads per pass through the staging buffer
#define DFF_SUP_COLS (4 * DFF_SUP_CB)
#define DFF_SUP_LDS (DFF_SUP_COLS + 1)   // leading dimension of the staging buffer in doubles: odd

__host__ __device__ __forceinline__ int superpose_ref_doubles(int N) { return (3 * N + 1) & ~1; }   // 16-byte multiple
__host__ __device__ __forceinline__ int superpose_per(int N) { return 4 * N + 1; }

// jacobi_rot (dff_struct.hip) that also hands out the rotation: c = 1, s = 0 when there is nothing to rotate
__host__ __device__ __forceinline__ void jacobi_rot_cs(double& app, double& aqq, double& apq, double& arp, double& arq,
                                                       double& asp, double& asq, double& c, double& s) {
    c = 1.0;
    s = 0.0;
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = fabs(theta) > 1e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
    c = 1.0 / sqrt(fma(t, t, 1.0));
    s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double g = arp, h = arq, u = asp, v = asq;
    arp = c * g - s * h;
    arq = s * g + c * h;
    asp = c * u - s * v;
    asq = s * u + c * v;
}

// columns p and q of the eigenvector matrix follow the rotation: (vp, vq) <- (c vp - s vq, s vp + c vq), row by row
__host__ __device__ __forceinline__ void jacobi_vec(double c, double s, double& v0p, double& v0q, double& v1p, double& v1q,
                                                    double& v2p, double& v2q, double& v3p, double& v3q) {
    double g = v0p, h = v0q;
    v0p = c * g - s * h; v0q = s * g + c * h;
    g = v1p; h = v1q;
    v1p = c * g - s * h; v1q = s * g + c * h;
    g = v2p; h = v2q;
    v2p = c * g - s * h; v2q = s * g + c * h;
    g = v3p; h = v3q;
    v3p = c * g - s * h; v3q = s * g + c * h;
}

// Largest eigenvalue of the symmetric 4x4 [[a00 a01 a02 a03] [. a11 a12 a13] [. . a22 a23] [. . . a33]] and a unit
// eigenvector q of it: the sweeps of sym4_lambda_max with the rotations accumulated.  Each sweep costs 6 x 16 more
// products than the eigenvalue alone.  Among equal diagonal entries at the end the lowest index is taken.
__host__ __device__ __forceinline__ double sym4_eig_max(double a00, double a01, double a02, double a03, double a11,
                                                        double a12, double a13, double a22, double a23, double a33,
                                                        double (&q)[4]) {
    const double nrm = a00 * a00 + a11 * a11 + a22 * a22 + a33 * a33 +
                       2.0 * (a01 * a01 + a02 * a02 + a03 * a03 + a12 * a12 + a13 * a13 + a23 * a23);
    double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
    double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
    double c, s;
    for (int sweep = 0; sweep < 8; ++sweep) {
        const double off = a01 * a01 + a02 * a02 + a03 * a03 + a12 * a12 + a13 * a13 + a23 * a23;
        if (!(off > 1e-30 * nrm)) break;                       // also ends at once on K = 0
        jacobi_rot_cs(a00, a11, a01, a02, a12, a03, a13, c, s);     // (0, 1): others 2, 3
        jacobi_vec(c, s, v00, v01, v10, v11, v20, v21, v30, v31);
        jacobi_rot_cs(a00, a22, a02, a01, a12, a03, a23, c, s);     // (0, 2): others 1, 3
        jacobi_vec(c, s, v00, v02, v10, v12, v20, v22, v30, v32);
        jacobi_rot_cs(a00, a33, a03, a01, a13, a02, a23, c, s);     // (0, 3): others 1, 2
        jacobi_vec(c, s, v00, v03, v10, v13, v20, v23, v30, v33);
        jacobi_rot_cs(a11, a22, a12, a01, a02, a13, a23, c, s);     // (1, 2): others 0, 3
        jacobi_vec(c, s, v01, v02, v11, v12, v21, v22, v31, v32);
        jacobi_rot_cs(a11, a33, a13, a01, a03, a12, a23, c, s);     // (1, 3): others 0, 2
        jacobi_vec(c, s, v01, v03, v11, v13, v21, v23, v31, v33);
        jacobi_rot_cs(a22, a33, a23, a02, a03, a12, a13, c, s);     // (2, 3): others 0, 1
        jacobi_vec(c, s, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    const double l = fmax(fmax(a00, a11), fmax(a22, a33));
    const int m = a00 == l ? 0 : a11 == l ? 1 : a22 == l ? 2 : 3;
    q[0] = m == 0 ? v00 : m == 1 ? v01 : m == 2 ? v02 : v03;
    q[1] = m == 0 ? v10 : m == 1 ? v11 : m == 2 ? v12 : v13;
    q[2] = m == 0 ? v20 : m == 1 ? v21 : m == 2 ? v22 : v23;
    q[3] = m == 0 ? v30 : m == 1 ? v31 : m == 2 ? v32 : v33;
    // the product of plane rotations is orthogonal to rounding; one normalisation keeps R^T R = I at the 1e-15 level
    const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
    return l;
}

// R (row-major) of the unit quaternion q = (q0; qx, qy, qz): quadratic in q, valid at q0 = 0
__host__ __device__ __forceinline__ void quat_to_rot(const double (&q)[4], double (&R)[9]) {
    const double ww = q[0] * q[0], xx = q[1] * q[1], yy = q[2] * q[2], zz = q[3] * q[3];
    const double wx = q[0] * q[1], wy = q[0] * q[2], wz = q[0] * q[3];
    const double xy = q[1] * q[2], xz = q[1] * q[3], yz = q[2] * q[3];
    R[0] = ww + xx - yy - zz; R[1] = 2.0 * (xy - wz);    R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);    R[4] = ww - xx + yy - zz; R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);    R[7] = 2.0 * (yz + wx);    R[8] = ww - xx - yy + zz;
}

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
    // centre the reference (every lane the same sums, in order: no reduction order to depend on)
    double m0 = 0, m1 = 0, m2 = 0;
    for (int b = 0; b < N; ++b) { m0 += ref[3 * b]; m1 += ref[3 * b + 1]; m2 += ref[3 * b + 2]; }
    m0 /= N; m1 /= N; m2 /= N;
    const bool ref_ok = isfinite(m0) && isfinite(m1) && isfinite(m2);   // fp64 sums of floats do not overflow
    for (int b = threadIdx.x; b < N; b += DFF_STRUCT_TILE) {
        rc[3 * b] = ref[3 * b] - m0;
        rc[3 * b + 1] = ref[3 * b + 1] - m1;
        rc[3 * b + 2] = ref[3 * b + 2] - m2;
    }
    if (part)
        for (int i = threadIdx.x; i < 4 * N; i += DFF_STRUCT_TILE) acc[i] = 0.0;
    __syncthreads();
    double Gb = 0;
    for (int b = 0; b < N; ++b) Gb += rc[3 * b] * rc[3 * b] + rc[3 * b + 1] * rc[3 * b + 1] + rc[3 * b + 2] * rc[3 * b + 2];
    unsigned long long nfin = 0ull;                          // finite frames of this workgroup's tiles (the same in every lane)
    const int nch = (N + DFF_SUP_CB - 1) / DFF_SUP_CB;
    struct_tiles(tile, x, n, N, magic, vec4, [&](long long s0, int cnt, int lane, bool live, const float* xs_) {
        float* xs = tile + lane * ld;                         // this lane's row: read as the frame, written as its image
        bool finite = live && ref_ok;
        double c0 = 0, c1 = 0, c2 = 0;
        double R[9];
        if (live) {
            for (int b = 0; b < N; ++b) {
                const float a0 = xs[3 * b], a1 = xs[3 * b + 1], a2 = xs[3 * b + 2];
                finite = finite && isfinite(a0) && isfinite(a1) && isfinite(a2);
                c0 += a0; c1 += a1; c2 += a2;
            }
            c0 /= N; c1 /= N; c2 /= N;
            double Ga = 0, Sxx = 0, Sxy = 0, Sxz = 0, Syx = 0, Syy = 0, Syz = 0, Szx = 0, Szy = 0, Szz = 0;
            for (int b = 0; b < N; ++b) {
                const double a0 = xs[3 * b] - c0, a1 = xs[3 * b + 1] - c1, a2 = xs[3 * b + 2] - c2;
                const double r0 = rc[3 * b], r1 = rc[3 * b + 1], r2 = rc[3 * b + 2];
                Ga = fma(a0, a0, fma(a1, a1, fma(a2, a2, Ga)));
                Sxx = fma(a0, r0, Sxx); Sxy = fma(a0, r1, Sxy); Sxz = fma(a0, r2, Sxz);
                Syx = fma(a1, r0, Syx); Syy = fma(a1, r1, Syy); Syz = fma(a1, r2, Syz);
                Szx = fma(a2, r0, Szx); Szy = fma(a2, r1, Szy); Szz = fma(a2, r2, Szz);
            }
            // Horn's symmetric key matrix K (trace 0); its top eigenvector is the quaternion of the optimal proper rotation
            const double k00 = Sxx + Syy + Szz, k01 = Syz - Szy, k02 = Szx - Sxz, k03 = Sxy - Syx;
            const double k11 = Sxx - Syy - Szz, k12 = Sxy + Syx, k13 = Szx + Sxz;
            const double k22 = -Sxx + Syy - Szz, k23 = Syz + Szy;
            const double k33 = -Sxx - Syy + Szz;
            double q[4] = {1.0, 0.0, 0.0, 0.0};
            const double l = finite ? sym4_eig_max(k00, k01, k02, k03, k11, k12, k13, k22, k23, k33, q) : 0.0;
            quat_to_rot(q, R);
            if (rmsd) {
                const double msd = (Ga + Gb - 2.0 * l) / N;
                rmsd[s0 + lane] = finite ? (float)sqrt(msd > 0.0 ? msd : 0.0) : __builtin_nanf("");
            }
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
            // coalesced store of the tile, the mirror image of struct_load_tile
            float* dst = aligned + s0 * N3;
            const int nf = cnt * N3;
            int k0 = 0;
            if (vec4_out) {
                const int n4 = nf >> 2;
                for (int k = threadIdx.x; k < n4; k += DFF_STRUCT_TILE) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned f = (unsigned)(4 * k + e);
                        const unsigned s = __umulhi(f, magic);
                        v[e] = tile[s * ld + (f - s * N3)];
                    }
                    *((f32x4*)dst + k) = v;
                }
                k0 = n4 << 2;
            }
            for (int k = k0 + threadIdx.x; k < nf; k += DFF_STRUCT_TILE) {
                const unsigned s = __umulhi((unsigned)k, magic);
                dst[k] = tile[s * ld + (k - s * N3)];
            }
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
