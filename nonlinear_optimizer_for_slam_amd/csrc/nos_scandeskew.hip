// nos_scandeskew.hip — motion compensation of a device-resident scan under a constant twist (nos_scan_deskew).
// The kernel and the way the rule is evaluated: scan_deskew_kernels.hpp.
#include "nos_internal.hpp"

#include "scan_deskew_kernels.hpp"

#include <cmath>

using namespace nosd;

extern "C" {

int nos_scan_deskew(nos_scan* scan, const double* times, size_t n_times, double reference_time, const double twist[6],
                    nos_scan** out_scan) {
  nosd::CtxGuard guard_(scan ? scan->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!scan || !out_scan || !twist) return fail(NOS_ERR_INVALID_ARGUMENT, "scan / out_scan / twist is NULL");
  const size_t n = scan->n;
  if (!times && n > 0) return fail(NOS_ERR_INVALID_ARGUMENT, "times is NULL");
  if (!std::isfinite(reference_time)) return fail(NOS_ERR_INVALID_ARGUMENT, "reference_time is not finite");
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(twist[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "twist[%d] is not finite", k);
  nos_ctx* ctx = scan->ctx;
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "the scan deskew needs a single-device context");
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points");
  // everything that is the same for all points, once, in double (scan_deskew_kernels.hpp)
  nos::ScanDeskewParams P{};
  const double* v = twist;
  const double* w = twist + 3;
  P.wn = std::hypot(w[0], w[1], w[2]);  // no underflow of the squares: |w| = 1e-170 stays 1e-170
  for (int k = 0; k < 3; ++k) {
    P.v[k] = v[k];
    P.k[k] = P.wn > 0.0 ? w[k] / P.wn : 0.0;
  }
  P.kv[0] = P.k[1] * v[2] - P.k[2] * v[1];
  P.kv[1] = P.k[2] * v[0] - P.k[0] * v[2];
  P.kv[2] = P.k[0] * v[1] - P.k[1] * v[0];
  P.kkv[0] = P.k[1] * P.kv[2] - P.k[2] * P.kv[1];
  P.kkv[1] = P.k[2] * P.kv[0] - P.k[0] * P.kv[2];
  P.kkv[2] = P.k[0] * P.kv[1] - P.k[1] * P.kv[0];
  P.s_ref = reference_time;
  NewScan out(ctx);
  if (!out) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  DeviceSlot& slot = ctx->slots[0];
  hipStream_t st = slot.stream;
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess && n == 0) e = out.alloc(0, false);  // an empty scan deskews to an empty scan
  if (e != hipSuccess) return hip_fail(e, "scan deskew");
  if (n == 0) {
    *out_scan = out.release();
    return NOS_OK;
  }
  unsigned int h_info[nos::kDeskewWords] = {0, 0};
  {
    DeviceBuffers buf(&slot);  // arena (pooled slabs) for the time stamps and the info words; goes back when this block ends
    buf.reserve(n_times * sizeof(double) + 512);
    double* d_times = nullptr;
    unsigned int* info = nullptr;
    e = buf.alloc(&d_times, n_times);
    if (e == hipSuccess) e = buf.alloc(&info, size_t(nos::kDeskewWords));
    if (e == hipSuccess) e = out.alloc(n, scan->d_order != nullptr);  // the order array goes along when the source has one
    if (e == hipSuccess && n_times > 0) e = hipMemcpyAsync(d_times, times, n_times * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(info, 0, sizeof h_info, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::scan_deskew_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, scan->d_planes, scan->d_order,
                         uint32_t(n), d_times, uint64_t(n_times), P, out.scan->d_planes, info);
      e = hipGetLastError();
    }
    if (e == hipSuccess && scan->d_order != nullptr)
      e = hipMemcpyAsync(out.scan->d_order, scan->d_order, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_info, info, sizeof h_info, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait
  }
  if (e != hipSuccess) return hip_fail(e, "scan deskew");
  if (h_info[nos::kDeskewNoTime] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "the point at position %u has no time stamp: its original index is >= n_times = %zu",
                h_info[nos::kDeskewNoTime] - 1u, n_times);
  if (h_info[nos::kDeskewBadTime] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "the time stamp of the point at position %u is not finite", h_info[nos::kDeskewBadTime] - 1u);
  *out_scan = out.release();
  return NOS_OK;
}

}  // extern "C"
