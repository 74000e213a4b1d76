// Moore-Penrose inverse of ONE symmetric 3x3 matrix by cyclic Jacobi (include/fr_hotpath.h, "shape-from-shading term"), written
// once for the host and the device: the kernel of fr_sfs.hip and the host export fr_debug_sfs_pinv instantiate this function.
//
// Fixed work: FR_SFS_SWEEPS sweeps over the pairs (0,1), (0,2), (1,2) -- no convergence test, no data-dependent loop.  A rotation
// whose off-diagonal element is exactly zero is skipped by a branch (a NaN is not zero: it goes through the arithmetic and spreads).
// Cyclic Jacobi converges quadratically once the off-diagonal mass is below the eigenvalue gaps.  On the 12,600 matrices of
// tests/test_sfs_cpu.py (Y Y^T of 1-64 unit vectors, rank 1 and 2, equal eigenvalues, scales 1e-30 and 1e30) the largest
// |P - numpy pinv| / ||pinv|| is 1.2e-6 after three sweeps and 9.8e-14 -- the float64 floor at condition 1e3 -- after four, five
// and six alike (two sweeps still miss ranks): six leaves two in hand.
// The angle is formed from a RATIO of elements, (a_qq - a_pp) / (2 a_pq), so the scale of the matrix never enters a square: no
// overflow or underflow between 1e-300 and 1e300.  Every operation is a separately rounded double one (-ffp-contract=off).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FR_SFS_HD __host__ __device__
#else
#define FR_SFS_HD
#endif

#define FR_SFS_SWEEPS 6

// one Jacobi rotation in the (p, q) plane: app, aqq, apq the 2x2 block, arp / arq the third row's two elements, v?p / v?q the
// two eigenvector columns
FR_SFS_HD inline void fr_sfs_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                    double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));   // |theta| = Inf gives t = 0
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

// m6, p6 = xx, xy, xz, yy, yz, zz.  Keeps eigenvalue i iff lambda_i > rcond * lambda_max and lambda_i > 0; P = sum over the kept
// ones, in the order the solver leaves them (the diagonal's order), of v_i v_i^T / lambda_i.  *rank = how many were kept.
// A matrix with a NaN or an Inf in it gives six NaNs and rank 0.
FR_SFS_HD inline void fr_sfs_pinv3(const double* m6, double rcond, double* p6, int* rank) {
    double a00 = m6[0], a01 = m6[1], a02 = m6[2], a11 = m6[3], a12 = m6[4], a22 = m6[5];
    const double poison = (((((a00 + a01) + a02) + a11) + a12) + a22) * 0.0;   // +-0 for a finite matrix, NaN otherwise
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < FR_SFS_SWEEPS; sweep++) {
        fr_sfs_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0,1): third row 2
        fr_sfs_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0,2): third row 1
        fr_sfs_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1,2): third row 0
    }
    const double lmax = fmax(a00, fmax(a11, a22));
    const double cut = rcond * lmax;
    const bool k0 = a00 > cut && a00 > 0.0, k1 = a11 > cut && a11 > 0.0, k2 = a22 > cut && a22 > 0.0;
    const double i0 = k0 ? 1.0 / a00 : 0.0, i1 = k1 ? 1.0 / a11 : 0.0, i2 = k2 ? 1.0 / a22 : 0.0;
    // column i of V is eigenvector i: (v0i, v1i, v2i)
#define FR_SFS_PIJ(r0, r1, r2, c0, c1, c2) \
    (((k0 ? ((r0) * (c0)) * i0 : 0.0) + (k1 ? ((r1) * (c1)) * i1 : 0.0)) + (k2 ? ((r2) * (c2)) * i2 : 0.0))
    const bool bad = !(poison == 0.0);
    const double nan = poison;   // (a NaN when bad)
    p6[0] = bad ? nan : FR_SFS_PIJ(v00, v01, v02, v00, v01, v02);
    p6[1] = bad ? nan : FR_SFS_PIJ(v00, v01, v02, v10, v11, v12);
    p6[2] = bad ? nan : FR_SFS_PIJ(v00, v01, v02, v20, v21, v22);
    p6[3] = bad ? nan : FR_SFS_PIJ(v10, v11, v12, v10, v11, v12);
    p6[4] = bad ? nan : FR_SFS_PIJ(v10, v11, v12, v20, v21, v22);
    p6[5] = bad ? nan : FR_SFS_PIJ(v20, v21, v22, v20, v21, v22);
#undef FR_SFS_PIJ
    *rank = bad ? 0 : (int)k0 + (int)k1 + (int)k2;
}
