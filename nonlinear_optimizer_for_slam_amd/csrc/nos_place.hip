// nos_place.hip — place recognition: the Scan Context descriptor of a device-resident scan (nos_scan_descriptor) and a
// database of descriptors that is searched exhaustively on the device (nos_place_db_*).
// The kernels, the slot format and the way the rule is evaluated: place_kernels.hpp.
#include "nos_internal.hpp"

#include "place_kernels.hpp"

#include <cmath>
#include <memory>

using namespace nosd;

struct nos_place_db {
  nos_ctx* ctx = nullptr;
  nos::PlaceDev P{};
  size_t size = 0;
  size_t capacity = 0;        // slots behind d_slots
  double* d_slots = nullptr;  // [capacity] slots (place_kernels.hpp: column-major descriptor + column norms)
};

namespace {

constexpr size_t kPlaceMinCapacity = 16;

int check_params(const nos_place_params* p) {
  if (p->n_rings < 1 || p->n_rings > nos::kPlaceMaxRings)
    return fail(NOS_ERR_INVALID_ARGUMENT, "n_rings = %d is outside 1 ... %d", int(p->n_rings), nos::kPlaceMaxRings);
  if (p->n_sectors < 1 || p->n_sectors > nos::kPlaceMaxSectors)
    return fail(NOS_ERR_INVALID_ARGUMENT, "n_sectors = %d is outside 1 ... %d", int(p->n_sectors), nos::kPlaceMaxSectors);
  if (!std::isfinite(p->max_range) || !(p->max_range > 0.0))
    return fail(NOS_ERR_INVALID_ARGUMENT, "max_range = %g is not a finite number > 0", p->max_range);
  if (!std::isfinite(p->z_floor)) return fail(NOS_ERR_INVALID_ARGUMENT, "z_floor = %g is not finite", p->z_floor);
  return NOS_OK;
}

nos::PlaceDev make_dev(const nos_place_params* p) {
  nos::PlaceDev P{};
  P.n_rings = p->n_rings;
  P.n_sectors = p->n_sectors;
  P.max_range = p->max_range;
  P.z_floor = p->z_floor;
  P.two_pi = 2.0 * M_PI;
  P.ring_scale = double(p->n_rings) / p->max_range;
  P.sector_scale = double(p->n_sectors) / P.two_pi;
  return P;
}

inline size_t cells_of(const nos::PlaceDev& P) { return size_t(P.n_rings) * size_t(P.n_sectors); }
inline size_t slot_doubles(const nos::PlaceDev& P) { return nos::place_slot_doubles(P.n_rings, P.n_sectors); }

// What every call that takes a scan rejects of it and of its context; the context's slot on success.
int check_scan(const nos_scan* scan, const nos_ctx* want_ctx, DeviceSlot** slot) {
  if (want_ctx != nullptr && scan->ctx != want_ctx)
    return fail(NOS_ERR_INVALID_ARGUMENT, "the scan belongs to another context than the database");
  if (scan->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "place recognition needs a single-device context");
  if (scan->n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points");
  *slot = &scan->ctx->slots[0];
  return NOS_OK;
}

// The scan's descriptor into `slot_out` (device), its n_used into d_used[0]; d_keys: cells + 1 words of scratch, d_used =
// d_keys + cells.  Everything on the stream, no wait.
hipError_t enqueue_descriptor(const nos_scan* scan, const nos::PlaceDev& P, DeviceSlot& slot, unsigned long long* d_keys,
                              double* slot_out) {
  const size_t cells = cells_of(P);
  hipStream_t st = slot.stream;
  hipError_t e = hipMemsetAsync(d_keys, 0, (cells + 1) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const size_t n = scan->n;
  if (n > 0) {
    const size_t want = (n + nos::kPlacePointsPerBlock - 1) / nos::kPlacePointsPerBlock;
    const unsigned grid = unsigned(std::min<size_t>(want, size_t(4) * size_t(std::max(slot.num_cus, 1))));
    if (cells <= size_t(nos::kPlaceSmallBins))
      hipLaunchKernelGGL(nos::place_descriptor_kernel<nos::kPlaceSmallBins>, dim3(grid), dim3(256), 0, st, scan->d_planes, n, P,
                         d_keys, d_keys + cells);
    else
      hipLaunchKernelGGL(nos::place_descriptor_kernel<nos::kPlaceMaxBins>, dim3(grid), dim3(256), 0, st, scan->d_planes, n, P,
                         d_keys, d_keys + cells);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(nos::place_finish_kernel, dim3(1), dim3(128), 0, st, d_keys, static_cast<const double*>(nullptr), P.n_rings,
                     P.n_sectors, P.z_floor, slot_out);
  return hipGetLastError();
}

// Host descriptors (ring-major, n of them, already on the device at d_src) into n consecutive slots.
hipError_t enqueue_slots(const double* d_src, int n, const nos::PlaceDev& P, hipStream_t st, double* slots_out) {
  hipLaunchKernelGGL(nos::place_finish_kernel, dim3(unsigned(n)), dim3(128), 0, st, static_cast<const unsigned long long*>(nullptr),
                     d_src, P.n_rings, P.n_sectors, P.z_floor, slots_out);
  return hipGetLastError();
}

hipError_t enqueue_search(const nos_place_db* db, const double* d_qslots, int n_queries, size_t first, size_t count,
                          hipStream_t st, double* d_distance, int32_t* d_shift) {
  const unsigned grid = unsigned(std::min<size_t>(count, 16384));
  const size_t lds = cells_of(db->P) * sizeof(double);  // <= 64 KB
  if (db->P.n_sectors <= 64)
    hipLaunchKernelGGL(nos::place_search_kernel<1>, dim3(grid), dim3(64), lds, st, d_qslots, n_queries, db->d_slots, first, count,
                       db->P.n_rings, db->P.n_sectors, d_distance, d_shift);
  else
    hipLaunchKernelGGL(nos::place_search_kernel<2>, dim3(grid), dim3(64), lds, st, d_qslots, n_queries, db->d_slots, first, count,
                       db->P.n_rings, db->P.n_sectors, d_distance, d_shift);
  return hipGetLastError();
}

int hip_status(hipError_t e, const char* what) {
  (void)hipGetLastError();  // a failed allocation must not surface as the next call's launch error
  return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// Room for one more slot: the store grows by doubling, with a device-to-device copy (as the voxel store does).
int ensure_room(nos_place_db* db, DeviceSlot& slot) {
  if (db->size < db->capacity) return NOS_OK;
  const size_t new_cap = std::max(kPlaceMinCapacity, 2 * db->capacity);
  const size_t sd = slot_doubles(db->P);
  double* grown = nullptr;
  hipError_t e = device_alloc(slot, &grown, new_cap * sd * sizeof(double));
  if (e != hipSuccess) return hip_status(e, "growing the place database");
  if (db->size > 0) {
    e = hipMemcpyAsync(grown, db->d_slots, db->size * sd * sizeof(double), hipMemcpyDeviceToDevice, slot.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);
    if (e != hipSuccess) {
      (void)hipFree(grown);
      return hip_status(e, "growing the place database");
    }
  }
  if (db->d_slots) (void)hipFree(db->d_slots);
  db->d_slots = grown;
  db->capacity = new_cap;
  return NOS_OK;
}

// The search of qslots (device) and the way back of its results; the one wait.  d_used != NULL: its word comes back too.
int search_and_fetch(nos_place_db* db, DeviceSlot& slot, DeviceBuffers& buf, const double* d_qslots, int n_queries, size_t first,
                     size_t count, double* distance_out, int32_t* shift_out, const unsigned long long* d_used, size_t* n_used) {
  hipStream_t st = slot.stream;
  const size_t pairs = size_t(n_queries) * count;
  double* d_distance = nullptr;
  int32_t* d_shift = nullptr;
  unsigned long long h_used = 0;
  hipError_t e = hipSuccess;
  if (pairs > 0) {
    e = buf.alloc(&d_distance, pairs);
    if (e == hipSuccess) e = buf.alloc(&d_shift, pairs);
    if (e == hipSuccess) e = enqueue_search(db, d_qslots, n_queries, first, count, st, d_distance, d_shift);
    if (e == hipSuccess) e = hipMemcpyAsync(distance_out, d_distance, pairs * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(shift_out, d_shift, pairs * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess && d_used != nullptr) e = hipMemcpyAsync(&h_used, d_used, sizeof h_used, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait
  if (e != hipSuccess) return hip_status(e, "place search");
  if (n_used) *n_used = size_t(h_used);
  return NOS_OK;
}

}  // namespace

extern "C" {

int nos_scan_descriptor(nos_scan* scan, const nos_place_params* params, double* desc_out, size_t* n_used) {
  nosd::CtxGuard guard_(scan ? scan->ctx : nullptr);
  if (!params || !desc_out) return fail(NOS_ERR_INVALID_ARGUMENT, "params / desc_out is NULL");
  if (int rc = check_params(params)) return rc;
  if (!scan) return fail(NOS_ERR_INVALID_ARGUMENT, "scan is NULL");
  DeviceSlot* slot = nullptr;
  if (int rc = check_scan(scan, nullptr, &slot)) return rc;
  const nos::PlaceDev P = make_dev(params);
  const size_t cells = cells_of(P);
  hipStream_t st = slot->stream;
  hipError_t e = hipSetDevice(slot->device);
  if (e != hipSuccess) return hip_status(e, "scan descriptor");
  unsigned long long h_used = 0;
  {
    DeviceBuffers buf(slot);
    buf.reserve((cells + 1) * 8 + slot_doubles(P) * 8 + cells * 8 + 1024);
    unsigned long long* d_keys = nullptr;
    double* d_slot = nullptr;
    double* d_desc = nullptr;
    e = buf.alloc(&d_keys, cells + 1);
    if (e == hipSuccess) e = buf.alloc(&d_slot, slot_doubles(P));
    if (e == hipSuccess) e = buf.alloc(&d_desc, cells);
    if (e == hipSuccess) e = enqueue_descriptor(scan, P, *slot, d_keys, d_slot);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::place_unslot_kernel, dim3(1), dim3(128), 0, st, d_slot, P.n_rings, P.n_sectors, d_desc);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(desc_out, d_desc, cells * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_used, d_keys + cells, sizeof h_used, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait
  }
  if (e != hipSuccess) return hip_status(e, "scan descriptor");
  if (n_used) *n_used = size_t(h_used);
  return NOS_OK;
}

int nos_place_db_create(nos_ctx* ctx, const nos_place_params* params, size_t reserve, nos_place_db** out_db) {
  nosd::CtxGuard guard_(ctx);
  if (!params || !out_db) return fail(NOS_ERR_INVALID_ARGUMENT, "params / out_db is NULL");
  if (int rc = check_params(params)) return rc;
  if (!ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "place recognition needs a single-device context");
  std::unique_ptr<nos_place_db> db(new (std::nothrow) nos_place_db());
  if (!db) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  db->ctx = ctx;
  db->P = make_dev(params);
  if (reserve > 0) {
    DeviceSlot& slot = ctx->slots[0];
    hipError_t e = hipSetDevice(slot.device);
    if (e == hipSuccess) e = device_alloc(slot, &db->d_slots, reserve * slot_doubles(db->P) * sizeof(double));
    if (e != hipSuccess) return hip_status(e, "reserving the place database");
    db->capacity = reserve;
  }
  *out_db = db.release();
  return NOS_OK;
}

int nos_place_db_destroy(nos_place_db* db) {
  if (!db) return NOS_OK;
  {
    nosd::CtxGuard guard_(db->ctx);
    DeviceSlot& slot = db->ctx->slots[0];
    (void)hipSetDevice(slot.device);
    if (db->d_slots) {
      (void)hipStreamSynchronize(slot.stream);
      (void)hipFree(db->d_slots);
    }
  }
  delete db;
  return NOS_OK;
}

size_t nos_place_db_size(const nos_place_db* db) { return db ? db->size : 0; }

int nos_place_db_add(nos_place_db* db, const double* desc, size_t* index) {
  nosd::CtxGuard guard_(db ? db->ctx : nullptr);
  if (!db || !desc) return fail(NOS_ERR_INVALID_ARGUMENT, "db / desc is NULL");
  DeviceSlot& slot = db->ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e != hipSuccess) return hip_status(e, "place database add");
  if (int rc = ensure_room(db, slot)) return rc;
  const size_t cells = cells_of(db->P);
  {
    DeviceBuffers buf(&slot);
    double* d_src = nullptr;
    e = buf.alloc(&d_src, cells);
    if (e == hipSuccess) e = hipMemcpyAsync(d_src, desc, cells * sizeof(double), hipMemcpyHostToDevice, slot.stream);
    if (e == hipSuccess) e = enqueue_slots(d_src, 1, db->P, slot.stream, db->d_slots + db->size * slot_doubles(db->P));
    if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);  // desc is the caller's again; the staging goes back
  }
  if (e != hipSuccess) return hip_status(e, "place database add");
  if (index) *index = db->size;
  db->size += 1;
  return NOS_OK;
}

int nos_place_db_add_scan(nos_place_db* db, nos_scan* scan, size_t* index, size_t* n_used) {
  nosd::CtxGuard guard_(db ? db->ctx : nullptr);
  if (!db || !scan) return fail(NOS_ERR_INVALID_ARGUMENT, "db / scan is NULL");
  DeviceSlot* slot = nullptr;
  if (int rc = check_scan(scan, db->ctx, &slot)) return rc;
  hipError_t e = hipSetDevice(slot->device);
  if (e != hipSuccess) return hip_status(e, "place database add");
  if (int rc = ensure_room(db, *slot)) return rc;
  const size_t cells = cells_of(db->P);
  unsigned long long h_used = 0;
  {
    DeviceBuffers buf(slot);
    unsigned long long* d_keys = nullptr;
    e = buf.alloc(&d_keys, cells + 1);
    if (e == hipSuccess) e = enqueue_descriptor(scan, db->P, *slot, d_keys, db->d_slots + db->size * slot_doubles(db->P));
    if (e == hipSuccess) e = hipMemcpyAsync(&h_used, d_keys + cells, sizeof h_used, hipMemcpyDeviceToHost, slot->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(slot->stream);  // the one wait
  }
  if (e != hipSuccess) return hip_status(e, "place database add");
  if (index) *index = db->size;
  if (n_used) *n_used = size_t(h_used);
  db->size += 1;
  return NOS_OK;
}

int nos_place_db_get(nos_place_db* db, size_t index, double* desc_out) {
  nosd::CtxGuard guard_(db ? db->ctx : nullptr);
  if (!db || !desc_out) return fail(NOS_ERR_INVALID_ARGUMENT, "db / desc_out is NULL");
  if (index >= db->size) return fail(NOS_ERR_INVALID_ARGUMENT, "index %zu is outside the database (size %zu)", index, db->size);
  DeviceSlot& slot = db->ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e != hipSuccess) return hip_status(e, "place database get");
  const size_t cells = cells_of(db->P);
  {
    DeviceBuffers buf(&slot);
    double* d_desc = nullptr;
    e = buf.alloc(&d_desc, cells);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::place_unslot_kernel, dim3(1), dim3(128), 0, slot.stream, db->d_slots + index * slot_doubles(db->P),
                         db->P.n_rings, db->P.n_sectors, d_desc);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(desc_out, d_desc, cells * sizeof(double), hipMemcpyDeviceToHost, slot.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);
  }
  if (e != hipSuccess) return hip_status(e, "place database get");
  return NOS_OK;
}

int nos_place_db_search(nos_place_db* db, const double* queries, int32_t n_queries, size_t first, size_t count,
                        double* distance_out, int32_t* shift_out) {
  nosd::CtxGuard guard_(db ? db->ctx : nullptr);
  if (!db) return fail(NOS_ERR_INVALID_ARGUMENT, "db is NULL");
  if (n_queries < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_queries = %d is negative", int(n_queries));
  if (first > db->size || count > db->size - first)
    return fail(NOS_ERR_INVALID_ARGUMENT, "first + count = %zu + %zu is beyond the database (size %zu)", first, count, db->size);
  if (n_queries == 0 || count == 0) return NOS_OK;
  if (!queries || !distance_out || !shift_out) return fail(NOS_ERR_INVALID_ARGUMENT, "queries / distance_out / shift_out is NULL");
  DeviceSlot& slot = db->ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e != hipSuccess) return hip_status(e, "place search");
  const size_t cells = cells_of(db->P);
  const size_t sd = slot_doubles(db->P);
  DeviceBuffers buf(&slot);
  buf.reserve(size_t(n_queries) * (cells + sd) * 8 + size_t(n_queries) * count * 12 + 4096);
  double* d_src = nullptr;
  double* d_qslots = nullptr;
  e = buf.alloc(&d_src, size_t(n_queries) * cells);
  if (e == hipSuccess) e = buf.alloc(&d_qslots, size_t(n_queries) * sd);
  if (e == hipSuccess) e = hipMemcpyAsync(d_src, queries, size_t(n_queries) * cells * sizeof(double), hipMemcpyHostToDevice, slot.stream);
  if (e == hipSuccess) e = enqueue_slots(d_src, n_queries, db->P, slot.stream, d_qslots);
  if (e != hipSuccess) return hip_status(e, "place search");
  return search_and_fetch(db, slot, buf, d_qslots, n_queries, first, count, distance_out, shift_out, nullptr, nullptr);
}

int nos_place_db_search_scan(nos_place_db* db, nos_scan* scan, size_t first, size_t count, double* distance_out,
                             int32_t* shift_out, size_t* n_used) {
  nosd::CtxGuard guard_(db ? db->ctx : nullptr);
  if (!db || !scan) return fail(NOS_ERR_INVALID_ARGUMENT, "db / scan is NULL");
  if (first > db->size || count > db->size - first)
    return fail(NOS_ERR_INVALID_ARGUMENT, "first + count = %zu + %zu is beyond the database (size %zu)", first, count, db->size);
  if (count > 0 && (!distance_out || !shift_out)) return fail(NOS_ERR_INVALID_ARGUMENT, "distance_out / shift_out is NULL");
  DeviceSlot* slot = nullptr;
  if (int rc = check_scan(scan, db->ctx, &slot)) return rc;
  hipError_t e = hipSetDevice(slot->device);
  if (e != hipSuccess) return hip_status(e, "place search");
  const size_t cells = cells_of(db->P);
  DeviceBuffers buf(slot);
  buf.reserve((cells + 1) * 8 + slot_doubles(db->P) * 8 + count * 12 + 4096);
  unsigned long long* d_keys = nullptr;
  double* d_qslot = nullptr;
  e = buf.alloc(&d_keys, cells + 1);
  if (e == hipSuccess) e = buf.alloc(&d_qslot, slot_doubles(db->P));
  if (e == hipSuccess) e = enqueue_descriptor(scan, db->P, *slot, d_keys, d_qslot);
  if (e != hipSuccess) return hip_status(e, "place search");
  return search_and_fetch(db, *slot, buf, d_qslot, 1, first, count, distance_out, shift_out, d_keys + cells, n_used);
}

}  // extern "C"
