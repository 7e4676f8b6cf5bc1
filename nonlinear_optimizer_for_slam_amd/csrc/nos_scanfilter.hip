// nos_scanfilter.hip — voxel-grid filter of a device-resident scan (nos_scan_filter) and the way back to the host
// (nos_scan_points).  The kernels and the algorithm: scan_filter_kernels.hpp; the select: a rocPRIM call through group_host.hpp.
#include "group_host.hpp"

#include "scan_filter_kernels.hpp"

using namespace nosd;

extern "C" {

int nos_scan_filter(nos_scan* scan, double voxel_size, nos_scan** out_scan) {
  nosd::CtxGuard guard_(scan ? scan->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!scan || !out_scan) return fail(NOS_ERR_INVALID_ARGUMENT, "scan / out_scan is NULL");
  if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) return fail(NOS_ERR_INVALID_ARGUMENT, "bad voxel size");
  nos_ctx* ctx = scan->ctx;
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "the scan filter needs a single-device context");
  const size_t n = scan->n;
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points");
  const double inv_res = 1.0 / voxel_size;  // once, in double: the factor voxel_key_kernel multiplies by
  NewScan out(ctx);
  if (!out) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  DeviceSlot& slot = ctx->slots[0];
  hipStream_t st = slot.stream;
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess && n == 0) e = out.alloc(0, false);  // an empty scan filters to an empty scan
  if (e != hipSuccess) return hip_fail(e, "scan filter");
  if (n == 0) {
    *out_scan = out.release();
    return NOS_OK;
  }
  size_t table_size = 16;
  while (table_size < 2 * n) table_size <<= 1;  // load factor <= 1/2 even when every point has a cell of its own
  uint32_t n_kept = 0;
  unsigned int h_info[nos::kFilterWords] = {0, 0, 0, 0};
  {
    DeviceBuffers buf(&slot);  // arena (pooled slabs) for the temporaries; goes back when this block ends
    // table: 8 B key + 4 B first per entry; per point: 4 B entry + 4 B kept position; select temporaries behind them
    buf.reserve(table_size * (sizeof(uint64_t) + sizeof(uint32_t)) + n * 2 * sizeof(uint32_t) + (size_t(8) << 20));
    void* table = nullptr;
    uint32_t *entry = nullptr, *kept = nullptr, *d_count = nullptr;
    unsigned int* info = nullptr;
    PrimTmp t_select;
    e = buf.alloc_bytes(&table, table_size * (sizeof(uint64_t) + sizeof(uint32_t)));
    if (e == hipSuccess) e = buf.alloc(&entry, n);
    if (e == hipSuccess) e = buf.alloc(&kept, n);
    if (e == hipSuccess) e = buf.alloc(&d_count, 1);
    if (e == hipSuccess) e = buf.alloc(&info, size_t(nos::kFilterWords));
    unsigned long long* tab_key = static_cast<unsigned long long*>(table);
    uint32_t* tab_first = reinterpret_cast<uint32_t*>(tab_key + table_size);
    const nos::ScanFilterKeep keep{tab_first, entry, scan->d_order};
    const rocprim::counting_iterator<uint32_t> positions(0u);
    const auto select = [&](void* tmp, size_t& bytes) { return rocprim::select(tmp, bytes, positions, kept, d_count, n, keep, st); };
    if (e == hipSuccess) e = prim_plan(buf, select, t_select);
    // free entries are kEmptyCell and first = 0xFFFFFFFF: one fill of all-ones bytes over both arrays
    if (e == hipSuccess) e = hipMemsetAsync(table, 0xFF, table_size * (sizeof(uint64_t) + sizeof(uint32_t)), st);
    if (e == hipSuccess) e = hipMemsetAsync(info, 0, sizeof h_info, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::scan_filter_claim_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, scan->d_planes,
                         scan->d_planes + n, scan->d_planes + 2 * n, scan->d_order, uint32_t(n), inv_res, tab_key, tab_first,
                         uint32_t(table_size - 1), entry, info);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = prim_run(select, t_select);
    if (e == hipSuccess) e = hipMemcpyAsync(&n_kept, d_count, sizeof n_kept, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_info, info, sizeof h_info, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait: the kept count sizes the new scan
    if (e == hipSuccess && h_info[nos::kFilterBadPoint] != 0)
      return fail(NOS_ERR_INVALID_ARGUMENT, "point %u has a non-finite coordinate", h_info[nos::kFilterBadPoint] - 1u);
    if (e == hipSuccess && h_info[nos::kFilterFarPoint] != 0)
      return fail(NOS_ERR_UNSUPPORTED, "point %u lies outside the addressable grid", h_info[nos::kFilterFarPoint] - 1u);
    if (e == hipSuccess && (h_info[nos::kFilterProbeError] != 0 || n_kept == 0 || n_kept > n))
      return fail(NOS_ERR_HIP, "scan filter: inconsistent table (kept %u of %zu)", n_kept, n);
    if (e == hipSuccess) e = out.alloc(n_kept, true);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::scan_filter_gather_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, st, scan->d_planes, uint32_t(n),
                         scan->d_order, kept, n_kept, out.scan->d_planes, out.scan->d_order);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the gather has read `kept` before the arena takes it back
  }
  if (e != hipSuccess) return hip_fail(e, "scan filter");
  *out_scan = out.release();
  return NOS_OK;
}

int nos_scan_points(const nos_scan* scan, double* points_xyz_out) {
  nosd::CtxGuard guard_(scan ? scan->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!scan || (!points_xyz_out && scan->n > 0)) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  const size_t n = scan->n;
  if (n == 0) return NOS_OK;
  std::vector<double> planes;
  try {
    planes.resize(3 * n);
  } catch (const std::bad_alloc&) {
    return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  DeviceSlot& slot = scan->ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  NOS_HIP_CHECK(hipMemcpyAsync(planes.data(), scan->d_planes, 3 * n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  for (size_t i = 0; i < n; ++i) {  // 3 planes → [n][3]
    points_xyz_out[3 * i] = planes[i];
    points_xyz_out[3 * i + 1] = planes[n + i];
    points_xyz_out[3 * i + 2] = planes[2 * n + i];
  }
  return NOS_OK;
}

}  // extern "C"
