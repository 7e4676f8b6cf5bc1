// match_host.hpp — host side of a match, shared by nos_ndt_match (nos_match.hip), nos_ndt_match_indexed (nos_indexed.hip),
// nos_voxel_map_match, nos_voxel_map_match_indexed and nos_voxel_map_match_map (nos_voxelmap.hip); DESIGN.md §18.  The
// last runs over a second store's voxels where the others run over a scan's points (Items, below).  Otherwise the routes
// differ in their SOURCE only, as the two batched registrations differ in their Launcher (register_host.hpp).  A source
// has view,
// d_count, d_error (NULL for a snapshot: its search cannot fail), launch (starts a kernel of its view), kWhat (for
// messages) and three constants, which keep differences between the routes that nothing requires:
//   kTallyLaunches, kRecordLastKernel   only the store routes report to the bracket profiler / set the slot's last_kernel
//   kOutOfMemory                        the status of hipErrorOutOfMemory during the match: NOS_ERR_HIP from a snapshot
// Three more are spelled in the entry points: nos_ndt_match_indexed clears *out_ds ahead of the context check; the store
// routes reject an unknown dtype ahead of max_neighbors (check_match_call's dtype); the store's flat route writes *out_ds
// on success only, where nos_ndt_match hands it to dataset_new.  A later change can decide about each deliberately.
#pragma once

#include "nos_internal.hpp"

namespace nosd {

// A snapshot (nos_ndt_map).  args: the kernel's arguments between the view and the counter.
struct SnapshotSource {
  const nos::MapView& view;
  unsigned long long* d_count;
  unsigned int* d_error = nullptr;
  static constexpr const char* kWhat = "matching";
  static constexpr bool kTallyLaunches = false, kRecordLastKernel = false;
  static constexpr int kOutOfMemory = NOS_ERR_HIP;
  explicit SnapshotSource(const nos_ndt_map* map) : view(map->view), d_count(map->d_n_matches) {}
  template <typename Kernel, typename... Args>
  void launch(Kernel kernel, dim3 grid, hipStream_t st, Args... args) const {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, view, args..., d_count);
  }
};

// The live voxel store (voxel_query_host.hpp's live_store); its kernels end with the probe-error word.
struct StoreSource : LiveStore {
  static constexpr const char* kWhat = "matching against the voxel store";
  static constexpr bool kTallyLaunches = true, kRecordLastKernel = true;
  static constexpr int kOutOfMemory = NOS_ERR_OUT_OF_MEMORY;
  template <typename Kernel, typename... Args>
  void launch(Kernel kernel, dim3 grid, hipStream_t st, Args... args) const {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, view, args..., d_count, d_error);
  }
};

// The rejections all four entry points share, in their order.  map_ctx: the map's context, NULL for a NULL map.  dtype:
// passed by the store routes only; the snapshot routes leave theirs to dataset_new / indexed_from_device.
inline int check_match_call(const nos_ctx* map_ctx, const nos_scan* scan, const double* R, const double* t, nos_dataset** out_ds,
                            int max_neighbors, int dtype = NOS_F64) {
  if (!map_ctx || !scan || !R || !t || !out_ds) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (map_ctx != scan->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "map and scan belong to different contexts");
  if (dtype != NOS_F64 && dtype != NOS_F32) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
  if (max_neighbors < 1 || max_neighbors > 2) return fail(NOS_ERR_UNSUPPORTED, "max_neighbors must be 1 or 2");
  return NOS_OK;
}

// What a match runs over, one thread per item.  Items have n(), kForm (what a message of the flat match calls the route)
// and lead(f): f(the kernel's arguments between the view and the item count).  A scan's points are the items of every
// match but the map-to-map one, whose items are a second store's voxels (voxel_query_host.hpp's StoreVoxels).
struct ScanPoints {
  const nos_scan* scan;
  static constexpr const char* kForm = "";
  size_t n() const { return scan->n; }
  template <typename F>
  void lead(F f) const {
    const double *px = scan->d_planes, *py = px + scan->n, *pz = py + scan->n;
    f(px, py, pz);
  }
};

// What every match begins with, queued on the slot's stream: counter and probe-error word cleared, then `kernel`, one
// thread per item, on (view, the items' arguments, n, pose, max_neighbors, tail…, counter[, error word]).
template <typename Src, typename Kernel, typename Items, typename... Tail>
hipError_t start_match_over(const Src& src, DeviceSlot& slot, Kernel kernel, const Items& items, const nos::PosePod& pose,
                            int max_neighbors, Tail... tail) {
  const size_t n = items.n();
  hipError_t e = hipMemsetAsync(src.d_count, 0, sizeof(unsigned long long), slot.stream);
  if (e == hipSuccess && src.d_error) e = hipMemsetAsync(src.d_error, 0, sizeof(unsigned int), slot.stream);
  if (e != hipSuccess || n == 0) return e;
  items.lead([&](auto... lead) {
    src.launch(kernel, dim3(unsigned((n + 255) / 256)), slot.stream, lead..., uint64_t(n), pose, max_neighbors, tail...);
  });
  if (Src::kRecordLastKernel) slot.last_kernel = reinterpret_cast<const void*>(kernel);
  if (Src::kTallyLaunches && slot.prof_on && slot.prof_every == 0) ++slot.prof_launches;  // SELF-REPORTED (bracket profiler)
  return hipGetLastError();
}

// start_match_over a scan's points: (view, the scan's planes, n, pose, max_neighbors, tail…, counter[, error word]).
template <typename Src, typename Kernel, typename... Tail>
hipError_t start_match(const Src& src, DeviceSlot& slot, Kernel kernel, const nos_scan* scan, const nos::PosePod& pose,
                       int max_neighbors, Tail... tail) {
  return start_match_over(src, slot, kernel, ScanPoints{scan}, pose, max_neighbors, tail...);
}

// After start_match (e: what queuing gave): both words to the host, the call's one wait for the matcher → the match's status.
template <typename Src>
int read_match_words(const Src& src, hipError_t e, hipStream_t st, const char* form, size_t* n_matches) {
  unsigned long long count = 0;
  unsigned int probe_error = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&count, src.d_count, sizeof count, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && src.d_error) e = hipMemcpyAsync(&probe_error, src.d_error, sizeof probe_error, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const int hip_status = e == hipErrorOutOfMemory ? Src::kOutOfMemory : NOS_ERR_HIP;
  if (e != hipSuccess) return fail(hip_status, "%s%s failed: %s", form, Src::kWhat, hipGetErrorString(e));
  if (probe_error != 0) return fail(NOS_ERR_HIP, "%s%s failed: a table probe ran through the whole table", form, Src::kWhat);
  if (n_matches) *n_matches = size_t(count);
  return NOS_OK;
}

// The flat match: a dataset of two slots per item (out_ds goes to dataset_new), the view's match kernel by element
// type (k64, k32), the dataset's padding, the count.  One wait.  Call after check_match_call and whatever else the route
// rejects.
template <typename Src, typename K64, typename K32, typename Items>
int run_match_over(const Src& src, K64 k64, K32 k32, nos_ctx* ctx, const Items& items, const nos::PosePod& pose,
                   int max_neighbors, int dtype, nos_dataset** out_ds, size_t* n_matches) {
  nos_dataset* ds = nullptr;
  int rc = dataset_new(ctx, kKindNdt, 2 * items.n(), dtype, out_ds, &ds);
  if (rc != NOS_OK) return rc;
  Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess)
    e = dtype == NOS_F64 ? start_match_over(src, slot, k64, items, pose, max_neighbors, sh.layout, static_cast<double*>(sh.data))
                         : start_match_over(src, slot, k32, items, pose, max_neighbors, sh.layout, static_cast<float*>(sh.data));
  if (e == hipSuccess) {
    rc = zero_pad(dtype, nos::kNdtStored, sh.layout, sh.data, slot.stream);  // the dataset's padding: a launch when there is some
    if (Src::kTallyLaunches && slot.prof_on && slot.prof_every == 0 && sh.layout.n_padded > sh.layout.n) ++slot.prof_launches;
  }
  if (rc == NOS_OK) rc = read_match_words(src, e, slot.stream, Items::kForm, n_matches);
  if (rc != NOS_OK) {
    nos_dataset_destroy(ds);
    return rc;
  }
  *out_ds = ds;
  return NOS_OK;
}

// run_match_over a scan's points: two slots per scan point.
template <typename Src, typename K64, typename K32>
int run_match(const Src& src, K64 k64, K32 k32, nos_ctx* ctx, const nos_scan* scan, const nos::PosePod& pose, int max_neighbors,
              int dtype, nos_dataset** out_ds, size_t* n_matches) {
  return run_match_over(src, k64, k32, ctx, ScanPoints{scan}, pose, max_neighbors, dtype, out_ds, n_matches);
}

// The first half of an indexed match: the two id planes *d_idx = [2][n] from the call's arena `buf`, the view's index
// kernel, the count.  more(ids): what else the route queues on the stream before the wait (the store's compact table;
// nothing for a snapshot) → a HIP status.  One wait; indexed_from_device, the second half, has the other.
template <typename Src, typename Kernel, typename More>
int run_match_ids(const Src& src, Kernel index_kernel, nos_ctx* ctx, DeviceBuffers& buf, const nos_scan* scan,
                  const nos::PosePod& pose, int max_neighbors, int32_t** d_idx, size_t* n_matches, const More& more) {
  DeviceSlot& slot = ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess) e = buf.alloc(d_idx, 2 * scan->n);
  if (e == hipSuccess) e = start_match(src, slot, index_kernel, scan, pose, max_neighbors, *d_idx, *d_idx + scan->n);
  if (e == hipSuccess) e = more(*d_idx);
  return read_match_words(src, e, slot.stream, "indexed ", n_matches);
}

}  // namespace nosd
