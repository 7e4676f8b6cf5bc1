// scan_deskew_kernels.hpp — motion compensation ("deskewing") of a device-resident scan under a constant twist.
//
// The rule (include/nos.h): a point p measured at time s, re-expressed in the sensor frame at s_ref, is
//   p' = Exp(tau xi) p = R(phi) p + V(phi) u,   tau = s - s_ref,  phi = tau w,  u = tau v        (the SE(3) exponential)
// Evaluated about the UNIT axis k = w / |w|, which is the same for every point, with the signed angle theta = tau |w|:
//   R(phi) p = p + sin(theta) (k x p) + (1 - cos(theta)) (k x (k x p))
//   V(phi) u = tau v + tau h(theta) (k x v) + tau g(theta) (k x (k x v))
//   h = (1 - cos(theta)) / theta,   g = (theta - sin(theta)) / theta
// so k, |w|, k x v and k x (k x v) are computed once on the host in double (|w| by hypot: (1e-170)^2 does not underflow
// there) and reach the kernel by value, in scalar registers.  Per point: one sincos of theta / 2, two divisions, about
// forty multiply-adds.  The traps:
//   theta == 0   (tau == 0, w == 0): every coefficient is 0 — divisions go through theta_safe = 1, nothing is 0/0;
//   1 - cos      cancels: 2 sin^2(theta / 2), from the same sincos that gives sin(theta) = 2 sin(theta/2) cos(theta/2);
//   theta - sin  cancels for small theta: below kDeskewSeriesTheta the series of g in theta^2 (six terms: the first one
//                left out is 4e-19 of the sum at the threshold); both arms are computed and one is selected.
// tau == 0 gives p' == p and xi == 0 gives p' == p: every added term is then an exact zero (a -0.0 comes back as +0.0).
// One lane per stored position and no communication between lanes: the bits of a point's result are a function of
// (p, s, s_ref, xi) alone, whatever the launch geometry, the stored position or the neighbours.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nos {

constexpr double kDeskewSeriesTheta = 0.25;  // |theta| below it: g by its series (pipeline.py keeps the same number)

// words of the deskew's device-side error block
enum ScanDeskewWord {
  kDeskewNoTime = 0,   // 1 + stored position of a point whose original index is >= n_times (atomicMax; 0 = none)
  kDeskewBadTime = 1,  // 1 + stored position of a point whose time stamp is not finite (atomicMax; 0 = none)
  kDeskewWords = 2
};

// everything that is the same for all points; by value, so it lives in scalar registers
struct ScanDeskewParams {
  double v[3];    // translational velocity, body frame
  double k[3];    // unit rotation axis w / |w| (zero when w == 0)
  double kv[3];   // k x v
  double kkv[3];  // k x (k x v)
  double wn;      // |w|
  double s_ref;
};

// order == nullptr: the scan was never sorted nor filtered, a point's original index is its position.
__global__ __launch_bounds__(256) void scan_deskew_kernel(const double* __restrict__ planes, const uint32_t* __restrict__ order,
                                                          uint32_t n, const double* __restrict__ times, uint64_t n_times,
                                                          ScanDeskewParams P, double* __restrict__ out_planes,
                                                          unsigned int* __restrict__ info) {
  const uint32_t pos = blockIdx.x * 256 + threadIdx.x;  // n < 2^32 - 1 and the grid covers n: no wrap
  if (pos >= n) return;
  const uint32_t orig = order != nullptr ? order[pos] : pos;
  if (orig >= n_times) {
    atomicMax(&info[kDeskewNoTime], pos + 1u);
    return;
  }
  const double s = times[orig];
  if (!(fabs(s) < __builtin_huge_val())) {  // a NaN fails the test
    atomicMax(&info[kDeskewBadTime], pos + 1u);
    return;
  }
  const double x = planes[pos], y = planes[size_t(n) + pos], z = planes[2 * size_t(n) + pos];
  const double tau = s - P.s_ref;
  const double theta = tau * P.wn;
  double sh, ch;
  sincos(0.5 * theta, &sh, &ch);
  const double sn = 2.0 * sh * ch;     // sin(theta)
  const double vers = 2.0 * sh * sh;   // 1 - cos(theta)
  const double theta_safe = theta != 0.0 ? theta : 1.0;
  const double h = vers / theta_safe;
  const double q = theta * theta;
  double series = fma(q, -1.0 / 6227020800.0, 1.0 / 39916800.0);
  series = fma(q, series, -1.0 / 362880.0);
  series = fma(q, series, 1.0 / 5040.0);
  series = fma(q, series, -1.0 / 120.0);
  series = fma(q, series, 1.0 / 6.0);
  series *= q;
  const double g = fabs(theta) < kDeskewSeriesTheta ? series : (theta - sn) / theta_safe;
  // k x p and k x (k x p)
  const double cx = P.k[1] * z - P.k[2] * y, cy = P.k[2] * x - P.k[0] * z, cz = P.k[0] * y - P.k[1] * x;
  const double dx = P.k[1] * cz - P.k[2] * cy, dy = P.k[2] * cx - P.k[0] * cz, dz = P.k[0] * cy - P.k[1] * cx;
  const double th = tau * h, tg = tau * g;
  // the small terms first, the point last: p + (sum of corrections)
  const double ox = fma(sn, cx, fma(vers, dx, fma(tau, P.v[0], fma(th, P.kv[0], tg * P.kkv[0]))));
  const double oy = fma(sn, cy, fma(vers, dy, fma(tau, P.v[1], fma(th, P.kv[1], tg * P.kkv[1]))));
  const double oz = fma(sn, cz, fma(vers, dz, fma(tau, P.v[2], fma(th, P.kv[2], tg * P.kkv[2]))));
  out_planes[pos] = x + ox;
  out_planes[size_t(n) + pos] = y + oy;
  out_planes[2 * size_t(n) + pos] = z + oz;
}

}  // namespace nos
