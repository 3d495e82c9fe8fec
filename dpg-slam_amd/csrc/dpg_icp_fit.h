// dpg_icp_fit.h -- the part of an ICP iteration after the rigid-fit sums, shared by the three ICP
// kernels (grid, k-d tree, angular): the closed-form fit (R5), the move of a source point, the
// composition of the 2x3 float transform, the convergence rule (R6) and the result record (R8).
// The rounding order of these expressions is what "bit-exact against the oracle" means
// (oracle/dpg_oracle.c rigid_from_sums and its callers), so there is one copy of them.  Every
// expression is one rounding per operation (-ffp-contract=off).  Also the two small helpers the
// kernels' index builds and LDS layouts share.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "dpg_atan2f.h"
#include "dpg_internal.h"
#include "dpg_icp_tree.h"

namespace dpg_icp {

__host__ __device__ __forceinline__ size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// float -> uint32 with the same order (sort keys)
__device__ __forceinline__ uint32_t orderable(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one iteration's fit: the rotation (cos, sin) and translation as pcl::transformCloud takes them
// (float), and the mean squared distance of the correspondences the fit was made from
struct Fit {
    float cf, sf, txf, tyf;
    double mse;
};

// R5 planar closed form from the eight tree sums (S[0] > 0)
__device__ __forceinline__ Fit rigid_from_sums(const double* S) {
    const double n = S[0];
    double a, b;
    dpg_tree::fit_ab(S, a, b);
    const double hh = sqrt(a * a + b * b);
    double c = 1.0, s = 0.0;
    if (hh > 0.0) { c = a / hh; s = b / hh; }
    const double mpx = S[2] / n, mpy = S[3] / n, mqx = S[4] / n, mqy = S[5] / n;
    const double txd = mqx - (c * mpx - s * mpy);
    const double tyd = mqy - (s * mpx + c * mpy);
    return Fit{(float)c, (float)s, (float)txd, (float)tyd, S[1] / S[0]};
}

// a source point moved by the fit, as pcl::transformCloud does it in place
__device__ __forceinline__ void move_point(const Fit& f, float& x, float& y) {
    const float nsf = -f.sf;
    const float x0 = x, y0 = y;
    x = (f.cf * x0 + nsf * y0) + f.txf;
    y = (f.sf * x0 + f.cf * y0) + f.tyf;
}

// F <- fit o F, the cumulative 2x3 transform (rows)
__device__ __forceinline__ void compose(const Fit& f, float (&F)[6]) {
    const float cf = f.cf, sf = f.sf, nsf = -f.sf;
    float Nf[6];
    Nf[0] = cf * F[0] + nsf * F[3];
    Nf[1] = cf * F[1] + nsf * F[4];
    Nf[2] = (cf * F[2] + nsf * F[5]) + f.txf;
    Nf[3] = sf * F[0] + cf * F[3];
    Nf[4] = sf * F[1] + cf * F[4];
    Nf[5] = (sf * F[2] + cf * F[5]) + f.tyf;
#pragma unroll
    for (int q = 0; q < 6; ++q) F[q] = Nf[q];
}

// R6 DefaultConvergenceCriteria after iteration k (counted from 1) with this fit.  One expression
// on purpose: with early returns the angular kernel's code grows.
__device__ __forceinline__ bool stops(const Fit& f, int k, double prev_mse, const dpg_icp_kparams& kp) {
    const float tr = ((f.cf + f.cf) + 1.0f) - 1.0f;
    const double cos_angle = 0.5 * (double)tr;
    const double tsq = (double)(f.txf * f.txf + f.tyf * f.tyf);
    return k >= kp.max_iter || (cos_angle >= kp.rot_thr && tsq <= kp.eps) || fabs(f.mse - prev_mse) < kp.mse_abs;
}

// R8 the result record of one edge (called by one thread)
__device__ __forceinline__ void write_result(dpg_icp_result* out, const float (&F)[6], int converged, int k, int cnt,
                                             int status, double mse) {
    dpg_icp_result R;
#pragma unroll
    for (int q = 0; q < 6; ++q) R.T[q] = F[q];
    R.z[0] = F[2];
    R.z[1] = F[5];
    R.z[2] = dpg_atan2f(F[3], F[0]);   // Rotation2Df::fromRotationMatrix -> std::atan2(float, float)
    R.converged = converged;
    R.iterations = k;
    R.n_corr = cnt;
    R.status = status;
    R.pad = 0;
    R.fitness = mse;
    *out = R;
}

}  // namespace dpg_icp
