// dff_kabsch.h -- the optimal superposition of two centred point sets, as arithmetic: from the 3 x 3 correlation S and the
// inner products Ga, Gb to the minimum RMSD over PROPER rotations (as mdtraj) and, on request, the rotation that reaches
// it.  Every kernel that needs either (dff_struct.hip, dff_ensemble.hip, dff_superpose.hip) calls these functions: the stop
// rule, the sweep cap, the overflow guard and the tie-break below are decided here and nowhere else.
// No thread index, no memory: plain fp64 functions of their arguments, host and device.
//
//   K        Horn's symmetric 4 x 4 key matrix of S (trace 0): lambda_max(K) = max over proper rotations of tr(R S), and
//            its eigenvector is that rotation's unit quaternion
//   Jacobi   lambda_max by cyclic Jacobi in fp64 (<= 8 sweeps, stop when the off-diagonal is below 1e-15 ||K||).  Not
//            Newton on K's characteristic quartic (QCP, Theobald 2005): for an elongated frame or reference the two
//            largest eigenvalues nearly coincide, the quartic has a near-double root that it fixes only to ~sqrt(eps)
//            lambda, and Newton stopped up to 4.4e-2 A off on straight chains.  Jacobi is backward-stable: lambda_max to
//            ~eps ||K||, whatever the spacing of the eigenvalues.
//   RMSD     msd = (Ga + Gb - 2 lambda) / N, sqrt(max(msd, 0)) in fp64, rounded to fp32 once
//   R        from the formula that is QUADRATIC in q: no division by q0, so a half turn (q0 = 0) is an ordinary input.
//            K = 0 (all points coincident): no sweep runs, q keeps the caller's value.  A degenerate largest eigenvalue
//            (collinear points): Jacobi still ends with an orthonormal eigenbasis; the column it ends with is A maximiser --
//            a proper rotation that reaches the minimal RMSD, one of a continuum.
#pragma once
#include <hip/hip_runtime.h>

// the upper triangle of a symmetric 4 x 4 matrix [[a00 a01 a02 a03] [. a11 a12 a13] [. . a22 a23] [. . . a33]]
struct Sym4 {
    double a00, a01, a02, a03, a11, a12, a13, a22, a23, a33;
};

// Horn's key matrix of the correlation S (row = component of the moving set, column = component of the reference)
__host__ __device__ __forceinline__ Sym4 horn_key(double Sxx, double Sxy, double Sxz, double Syx, double Syy, double Syz,
                                                  double Szx, double Szy, double Szz) {
    Sym4 k;
    k.a00 = Sxx + Syy + Szz; k.a01 = Syz - Szy; k.a02 = Szx - Sxz; k.a03 = Sxy - Syx;
    k.a11 = Sxx - Syy - Szz; k.a12 = Sxy + Syx; k.a13 = Szx + Sxz;
    k.a22 = -Sxx + Syy - Szz; k.a23 = Syz + Szy;
    k.a33 = -Sxx - Syy + Szz;
    return k;
}

// One Jacobi rotation of the symmetric 4x4 matrix in the (p, q) plane: a_pq -> 0.  (r, s) are the other two indices;
// arp = a_rp, arq = a_rq, asp = a_sp, asq = a_sq.  t = tan of the rotation angle, the smaller root of t^2 + 2 theta t = 1;
// 1 / (2 theta) when theta^2 would overflow (a_pq negligible next to a_qq - a_pp).  Hands out the rotation: c = 1, s = 0
// when there is nothing to rotate.
__host__ __device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq,
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

// Largest eigenvalue of the symmetric 4x4 m by cyclic Jacobi.  The off-diagonal mass falls quadratically, so a few sweeps
// reach the stop; the cap only bounds the loop.
// VEC: the plane rotations are accumulated as well (6 x 16 more products per sweep) and q receives a unit eigenvector of
// that eigenvalue -- among equal diagonal entries at the end, the column of the lowest index.  Without VEC q is not touched.
template <bool VEC>
__host__ __device__ __forceinline__ double sym4_jacobi(const Sym4& m, double* q = nullptr) {
    double a00 = m.a00, a01 = m.a01, a02 = m.a02, a03 = m.a03, a11 = m.a11;
    double a12 = m.a12, a13 = m.a13, a22 = m.a22, a23 = m.a23, a33 = m.a33;
    const double nrm = a00 * a00 + a11 * a11 + a22 * a22 + a33 * a33 +
                       2.0 * (a01 * a01 + a02 * a02 + a03 * a03 + a12 * a12 + a13 * a13 + a23 * a23);
    double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
    double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
    double c, s;
    for (int sweep = 0; sweep < 8; ++sweep) {
        const double off = a01 * a01 + a02 * a02 + a03 * a03 + a12 * a12 + a13 * a13 + a23 * a23;
        if (!(off > 1e-30 * nrm)) break;                       // also ends at once on K = 0
        jacobi_rot(a00, a11, a01, a02, a12, a03, a13, c, s);        // (0, 1): others 2, 3
        if constexpr (VEC) jacobi_vec(c, s, v00, v01, v10, v11, v20, v21, v30, v31);
        jacobi_rot(a00, a22, a02, a01, a12, a03, a23, c, s);        // (0, 2): others 1, 3
        if constexpr (VEC) jacobi_vec(c, s, v00, v02, v10, v12, v20, v22, v30, v32);
        jacobi_rot(a00, a33, a03, a01, a13, a02, a23, c, s);        // (0, 3): others 1, 2
        if constexpr (VEC) jacobi_vec(c, s, v00, v03, v10, v13, v20, v23, v30, v33);
        jacobi_rot(a11, a22, a12, a01, a02, a13, a23, c, s);        // (1, 2): others 0, 3
        if constexpr (VEC) jacobi_vec(c, s, v01, v02, v11, v12, v21, v22, v31, v32);
        jacobi_rot(a11, a33, a13, a01, a03, a12, a23, c, s);        // (1, 3): others 0, 2
        if constexpr (VEC) jacobi_vec(c, s, v01, v03, v11, v13, v21, v23, v31, v33);
        jacobi_rot(a22, a33, a23, a02, a03, a12, a13, c, s);        // (2, 3): others 0, 1
        if constexpr (VEC) jacobi_vec(c, s, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    const double l = fmax(fmax(a00, a11), fmax(a22, a33));
    if constexpr (VEC) {
        const int i = a00 == l ? 0 : a11 == l ? 1 : a22 == l ? 2 : 3;
        q[0] = i == 0 ? v00 : i == 1 ? v01 : i == 2 ? v02 : v03;
        q[1] = i == 0 ? v10 : i == 1 ? v11 : i == 2 ? v12 : v13;
        q[2] = i == 0 ? v20 : i == 1 ? v21 : i == 2 ? v22 : v23;
        q[3] = i == 0 ? v30 : i == 1 ? v31 : i == 2 ? v32 : v33;
        // the product of plane rotations is orthogonal to rounding; one normalisation keeps R^T R = I at the 1e-15 level
        const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
    }
    return l;
}

// the minimum RMSD of two centred sets of N points from their inner products and lambda_max of their key matrix
__host__ __device__ __forceinline__ float kabsch_rmsd(double Ga, double Gb, double l, int N) {
    const double msd = (Ga + Gb - 2.0 * l) / N;
    return (float)sqrt(msd > 0.0 ? msd : 0.0);
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
