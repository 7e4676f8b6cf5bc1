// nos_dataset.hip — flat datasets: layout, ingestion (planes, device planes, records) and the entry points that create
// and destroy them (C ABI of include/nos.h).  Device-resident tiled-SoA storage; buffers come from the context's pool.
#include "nos_internal.hpp"
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>  // full-line non-temporal stores of the host-pack ingestion
#endif

namespace nosd {

// Default layout by element type (-1 = this rule; NOS_TILE_LOG2 / the "tile_log2" option / nos_ctx_set_layout override it):
//   fp64: planar planes with a skew (measured best and robust across sizes);
//   fp32: tiles of 1024 correspondences — one kernel chunk (512 lanes x 2) is one contiguous 60 KB block of memory;
//         measured at 10 M: planar 16-byte loads 6.37 TB/s, tiled 8-byte loads with the next chunk prefetched 6.94 TB/s
//         (profiles/r02_tune_f32_layout.txt).
constexpr int kDefaultTileLog2F32 = 10;

size_t elem_size(int dtype) { return dtype == NOS_F32 ? sizeof(float) : sizeof(double); }

// ------------------------------------------------------------------ layout

// n_fields: stored planes.  Flat NDT (nos::kNdtStored = 21): the 12 streamed planes (p, mu, A) in the layout below, the 9
// planes of S behind them in a region of the same shape (nos::TiledLayout) — planar with the plane skew for fp64, tiles of
// 2^10 items whose 12 streamed fields are contiguous for fp32.
nos::TiledLayout make_layout(size_t n, int n_fields, int tile_log2, int plane_skew) {
  const int stored = n_fields;
  if (n_fields == nos::kNdtStored) n_fields = nos::kNdtStreamed;
  nos::TiledLayout L{};
  L.n = n;
  if (tile_log2 <= 0) {
    // planar: pad to the largest chunk any kernel variant uses
    const size_t pad = 4096;
    L.n_padded = ((n + pad - 1) / pad) * pad;
    if (L.n_padded == 0) L.n_padded = pad;
    L.tile_stride = 0;
    // planes are skewed against each other so that the 15 concurrent streams of a block never start at the same
    // offset modulo a large power of two (n_padded itself often is one)
    L.field_stride = L.n_padded + size_t(plane_skew);
    L.tile_shift = 40;
    L.tile_mask = 0xFFFFFFFFu;
  } else {
    const size_t tile = size_t(1) << tile_log2;
    L.n_padded = ((n + tile - 1) / tile) * tile;
    if (L.n_padded == 0) L.n_padded = tile;
    L.tile_stride = tile * size_t(n_fields);
    L.field_stride = tile;
    L.tile_shift = uint32_t(tile_log2);
    L.tile_mask = uint32_t(tile - 1);
  }
  if (stored == nos::kNdtStored) {
    L.s_offset = (L.tile_stride == 0 ? L.field_stride : L.n_padded) * size_t(nos::kNdtStreamed);
    L.s_tile_stride = L.tile_stride == 0 ? 0 : L.field_stride * size_t(nos::kNdtStored - nos::kNdtStreamed);
  }
  return L;
}

// planes a dataset stores (flat NDT: 21, see make_layout); ds->n_fields are the planes of the caller's view (nos.h)
int stored_planes(const nos_dataset* ds) { return ds->kind == kKindNdt ? nos::kNdtStored : ds->n_fields; }

size_t layout_elems(const nos::TiledLayout& L, int n_fields) {
  return (L.tile_stride == 0 ? L.field_stride : L.n_padded) * size_t(n_fields);
}

// ------------------------------------------------------------------ dataset construction

int dataset_tile_log2(const nos_ctx* ctx, int dtype) {
  const int tile_log2 = ctx->tile_log2 >= 0 ? ctx->tile_log2 : ctx->settings.tile_log2;
  return tile_log2 < 0 ? (dtype == NOS_F32 ? kDefaultTileLog2F32 : 0) : tile_log2;
}

int alloc_shards(nos_ctx* ctx, nos_dataset* ds) {
  const int n_shards = int(ctx->slots.size());
  const size_t n = ds->n;
  const size_t per = (n + n_shards - 1) / size_t(n_shards);  // contiguous equal ranges
  const int tile_log2 = dataset_tile_log2(ctx, ds->dtype);
  if (tile_log2 != 0 && (tile_log2 < 10 || tile_log2 > 24)) return fail(NOS_ERR_INVALID_ARGUMENT, "tile_log2 out of range");
  ds->tile = tile_log2 > 0 ? (size_t(1) << tile_log2) : 0;
  ds->shards.resize(n_shards);
  size_t begin = 0;
  for (int s = 0; s < n_shards; ++s) {
    const size_t cnt = begin < n ? std::min(per, n - begin) : 0;
    Shard& sh = ds->shards[s];
    sh.slot = s;
    sh.layout = make_layout(cnt, stored_planes(ds), tile_log2, ctx->settings.plane_skew);
    sh.bytes = layout_elems(sh.layout, stored_planes(ds)) * elem_size(ds->dtype);
    NOS_HIP_CHECK(hipSetDevice(ctx->slots[s].device));
    int prc = pool_alloc(ctx->slots[s], sh.bytes, &sh.data, &sh.capacity);
    if (prc != NOS_OK) return prc;
    sh.pooled = true;
    sh.layout.base = sh.data;
    begin += cnt;
  }
  return NOS_OK;
}

template <typename SRC>
int retile_dispatch(const nos::PlanePtrs& src, int n_fields, const nos::TiledLayout& L, void* dst, int dtype,
                    hipStream_t stream) {
  if (n_fields == NOS_NDT_PLANES) {  // flat NDT: one item per thread, its U planes computed on the way
    const dim3 grid1(unsigned((L.n_padded + 255) / 256));
    if (dtype == NOS_F64)
      hipLaunchKernelGGL((nos::retile_ndt_kernel<SRC, double>), grid1, dim3(256), 0, stream, src, L, static_cast<double*>(dst));
    else
      hipLaunchKernelGGL((nos::retile_ndt_kernel<SRC, float>), grid1, dim3(256), 0, stream, src, L, static_cast<float*>(dst));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NOS_ERR_HIP, "retile launch failed: %s", hipGetErrorString(e));
    return NOS_OK;
  }
  dim3 grid(unsigned((L.n_padded + 255) / 256), unsigned(n_fields));
  if (dtype == NOS_F64)
    hipLaunchKernelGGL((nos::retile_kernel<SRC, double>), grid, dim3(256), 0, stream, src, n_fields, L,
                       static_cast<double*>(dst));
  else
    hipLaunchKernelGGL((nos::retile_kernel<SRC, float>), grid, dim3(256), 0, stream, src, n_fields, L,
                       static_cast<float*>(dst));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "retile launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

int dataset_new(nos_ctx* ctx, int kind, size_t n, int dtype, nos_dataset** out, nos_dataset** made) {
  if (!ctx || !out) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / out pointer is NULL");
  if (dtype != NOS_F64 && dtype != NOS_F32) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
  *out = nullptr;
  nos_dataset* ds = new (std::nothrow) nos_dataset();
  if (!ds) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  ds->ctx = ctx;
  ds->kind = kind;
  ds->dtype = dtype;
  ds->n_fields = (kind == kKindNdt) ? NOS_NDT_PLANES : NOS_REPROJ_PLANES;
  ds->n = n;
  int rc = alloc_shards(ctx, ds);
  if (rc != NOS_OK) {
    nos_dataset_destroy(ds);
    return rc;
  }
  *made = ds;
  return NOS_OK;
}

int create_from_host_planes(nos_ctx* ctx, int kind, size_t n, const double* const* planes, int dtype,
                            nos_dataset** out) {
  if (!planes) return fail(NOS_ERR_INVALID_ARGUMENT, "planes is NULL");
  nos_dataset* ds = nullptr;
  int rc = dataset_new(ctx, kind, n, dtype, out, &ds);
  if (rc != NOS_OK) return rc;
  for (int f = 0; f < ds->n_fields; ++f)
    if (!planes[f] && n > 0) {
      nos_dataset_destroy(ds);
      return fail(NOS_ERR_INVALID_ARGUMENT, "plane %d is NULL", f);
    }
  size_t begin = 0;
  for (Shard& sh : ds->shards) {
    DeviceSlot& slot = ctx->slots[sh.slot];
    const size_t cnt = sh.layout.n;
    hipError_t e = hipSetDevice(slot.device);
    void* staging = nullptr;
    const size_t plane_bytes = cnt * sizeof(double);
    if (e == hipSuccess && cnt > 0) e = device_alloc(slot, &staging, plane_bytes * ds->n_fields);
    nos::PlanePtrs src{};
    for (int f = 0; f < ds->n_fields && e == hipSuccess && cnt > 0; ++f) {
      char* d = static_cast<char*>(staging) + plane_bytes * f;
      e = hipMemcpyAsync(d, planes[f] + begin, plane_bytes, hipMemcpyHostToDevice, slot.stream);
      src.p[f] = d;
    }
    if (e == hipSuccess) {
      rc = retile_dispatch<double>(src, ds->n_fields, sh.layout, sh.data, dtype, slot.stream);
      if (rc == NOS_OK) e = hipStreamSynchronize(slot.stream);
    }
    if (staging) (void)hipFree(staging);
    if (e != hipSuccess || rc != NOS_OK) {
      nos_dataset_destroy(ds);
      if (rc != NOS_OK) return rc;
      return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "dataset upload failed: %s",
                  hipGetErrorString(e));
    }
    begin += cnt;
  }
  *out = ds;
  return NOS_OK;
}

int create_from_device_planes(nos_ctx* ctx, int kind, size_t n, const void* const* d_planes, int src_dtype,
                              int dtype, nos_dataset** out) {
  if (!d_planes) return fail(NOS_ERR_INVALID_ARGUMENT, "d_planes is NULL");
  if (!ctx || ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "from_device needs a single-device context");
  if (src_dtype != NOS_F64 && src_dtype != NOS_F32) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown src dtype");
  nos_dataset* ds = nullptr;
  int rc = dataset_new(ctx, kind, n, dtype, out, &ds);
  if (rc != NOS_OK) return rc;
  Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[0];
  nos::PlanePtrs src{};
  for (int f = 0; f < ds->n_fields; ++f) {
    if (!d_planes[f] && n > 0) {
      nos_dataset_destroy(ds);
      return fail(NOS_ERR_INVALID_ARGUMENT, "device plane %d is NULL", f);
    }
    src.p[f] = d_planes[f];
  }
  rc = (src_dtype == NOS_F64) ? retile_dispatch<double>(src, ds->n_fields, sh.layout, sh.data, dtype, slot.stream)
                              : retile_dispatch<float>(src, ds->n_fields, sh.layout, sh.data, dtype, slot.stream);
  hipError_t e = (rc == NOS_OK) ? hipStreamSynchronize(slot.stream) : hipSuccess;
  if (rc != NOS_OK || e != hipSuccess) {
    nos_dataset_destroy(ds);
    if (rc != NOS_OK) return rc;
    return fail(NOS_ERR_HIP, "retile failed: %s", hipGetErrorString(e));
  }
  *out = ds;
  return NOS_OK;
}

template <typename DST>
int unpack_launch(const unsigned char* d_rec, size_t stride, const nos::FieldOffsets& fo, int n_fields, size_t first,
                  size_t count, const nos::TiledLayout& L, void* dst, hipStream_t stream) {
  hipLaunchKernelGGL((nos::unpack_records_kernel<DST>), dim3(unsigned((count + 255) / 256)), dim3(256), 0, stream,
                     d_rec, uint64_t(stride), fo, n_fields, uint64_t(first), uint64_t(count), L,
                     static_cast<DST*>(dst));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "unpack launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

template <typename DST>
int zero_pad_launch(int n_fields, const nos::TiledLayout& L, void* dst, hipStream_t stream) {
  const size_t pads = L.n_padded - L.n;
  if (pads == 0) return NOS_OK;
  hipLaunchKernelGGL((nos::zero_pad_kernel<DST>), dim3(unsigned((pads + 255) / 256)), dim3(256), 0, stream, n_fields, L,
                     static_cast<DST*>(dst));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "zero-pad launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

// AoS ingestion: records are streamed in chunks through two device staging buffers so
// the H2D copy of chunk k+1 overlaps the unpack kernel of chunk k.
// Host-pack ingestion (first form: AoS → pinned SoA → H2D, double buffered): T host threads gather
// the n_fields used doubles out of every record into a pinned planar chunk (converted to the dataset's element type),
// the chunk's planes are copied straight into their final place in the planar layout while the threads pack the next
// chunk.  Moves 120 (60) instead of 304 bytes per NDT record over PCIe; pays when there are enough host threads, so it
// is chosen for large inputs only (see create_from_records).  Planar planes and tiled layouts alike.
// `pinned` is the staging image of one chunk: planar (tile_log2 = 0: field f of record j at f * chunk + j) or in the
// dataset's tiled order (record j of the chunk at (j >> T) * n_fields * 2^T + f * 2^T + (j mod 2^T); chunks start on
// tile boundaries), so that the image is one contiguous piece of the dataset.  [lo, lo + count) = this thread's records.
// Flat NDT in tiles (ndt): the image has the two regions of the stored layout — [tiles][12][2^T] with p, mu in fields 0-5
// (the A fields are computed on the device afterwards), then at 12 * chunk [tiles][9][2^T] of S — each one contiguous piece.
// Records are taken a cache line of OUTPUT at a time (8 doubles / 16 floats per field): the line's worth of every field is
// gathered into a small block first and leaves with full-line non-temporal stores — the staging image is written once and
// read only by the copy engine, so the destination lines need not be fetched for ownership first (4.2 instead of 5.4 GB of
// host memory traffic per 10 M NDT records) and 15 interleaved 8-byte store streams do not fight over the core's
// write-combining buffers.
template <typename T>
void pack_range(const unsigned char* host, size_t stride, const nos::FieldOffsets& fo, int n_fields, bool ndt, size_t first,
                size_t lo, size_t count, size_t chunk, int tile_log2, T* pinned) {
  const size_t tile = size_t(1) << tile_log2, mask = tile - 1;
  [[maybe_unused]] const size_t pitch = tile_log2 == 0 ? chunk : tile;
  auto dst_of = [&](size_t j, int f) -> T* {
    if (tile_log2 == 0) return pinned + size_t(f) * chunk + j;
    if (ndt && f >= 6)
      return pinned + size_t(nos::kNdtStreamed) * chunk + (j >> tile_log2) * (tile * size_t(nos::kNdtStored - nos::kNdtStreamed)) +
             size_t(f - 6) * tile + (j & mask);
    const size_t tile_fields = ndt ? size_t(nos::kNdtStreamed) : size_t(n_fields);
    return pinned + (j >> tile_log2) * (tile * tile_fields) + size_t(f) * tile + (j & mask);
  };
  auto one = [&](size_t j) {
    const unsigned char* rec = host + (first + j) * stride;
    for (int f = 0; f < n_fields; ++f) {
      double v;
      memcpy(&v, rec + fo.off[f], sizeof v);
      *dst_of(j, f) = T(v);
    }
  };
  [[maybe_unused]] constexpr size_t kLine = 64 / sizeof(T);  // records per output cache line
  size_t j = lo;
  const size_t end = lo + count;
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  if (n_fields <= 16 && (reinterpret_cast<uintptr_t>(pinned) & 63u) == 0 && pitch % kLine == 0) {
    for (; j < end && (j % kLine) != 0; ++j) one(j);  // up to the next line boundary of the image
    alignas(64) T block[16][kLine];
    for (; j + kLine <= end; j += kLine) {
      for (size_t r = 0; r < kLine; ++r) {
        const unsigned char* rec = host + (first + j + r) * stride;
        for (int f = 0; f < n_fields; ++f) {
          double v;
          memcpy(&v, rec + fo.off[f], sizeof v);
          block[f][r] = T(v);
        }
      }
      for (int f = 0; f < n_fields; ++f) {  // a line never straddles a tile: tiles are multiples of 1 024 records
        const __m128d* src = reinterpret_cast<const __m128d*>(block[f]);
        double* line = reinterpret_cast<double*>(dst_of(j, f));
        _mm_stream_pd(line + 0, src[0]);
        _mm_stream_pd(line + 2, src[1]);
        _mm_stream_pd(line + 4, src[2]);
        _mm_stream_pd(line + 6, src[3]);
      }
    }
    _mm_sfence();  // the non-temporal stores are globally visible before this thread reports the chunk packed
  }
#endif
  for (; j < end; ++j) one(j);
}

int ingest_host_pack(nos_ctx* ctx, nos_dataset* ds, Shard& sh, const unsigned char* host, size_t stride,
                     const nos::FieldOffsets& fo, int threads) {
  DeviceSlot& slot = ctx->slots[sh.slot];
  const size_t cnt = sh.layout.n;
  const size_t es = elem_size(ds->dtype);
  const size_t chunk = size_t(256) << 10;  // records per chunk: 31 MB of fp64 planes
  const bool ndt = ds->kind == kKindNdt;
  const int tile_log2 = sh.layout.tile_stride == 0 ? 0 : int(sh.layout.tile_shift);  // 0 = planar planes
  // image of one chunk: the planes as given (planar), or the stored layout's tiles (flat NDT: 21 fields, A left to the device)
  const size_t need = chunk * size_t(ndt && tile_log2 != 0 ? nos::kNdtStored : ds->n_fields) * es;
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess && slot.copy_stream == nullptr) e = hipStreamCreateWithFlags(&slot.copy_stream, hipStreamNonBlocking);
  for (int b = 0; b < 2 && e == hipSuccess; ++b)
    if (slot.pack_done[b] == nullptr) e = hipEventCreateWithFlags(&slot.pack_done[b], hipEventDisableTiming);
  if (e == hipSuccess && slot.pack_bytes < need) {
    for (int b = 0; b < 2; ++b) {
      if (slot.pack_pinned[b]) (void)hipHostFree(slot.pack_pinned[b]);
      slot.pack_pinned[b] = nullptr;
    }
    slot.pack_bytes = 0;
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
      e = hipHostMalloc(&slot.pack_pinned[b], need, hipHostMallocDefault);
      if (e == hipSuccess) e = debug_fill(slot, slot.pack_pinned[b], need, /*host=*/true);
    }
    if (e == hipSuccess) slot.pack_bytes = need;
  }
  // Worker threads live for the whole call; per chunk they are released by `go` (chunk number) and report through
  // `arrived`.  The calling thread waits for the pinned buffer to be free, releases the workers, waits for them, enqueues
  // the chunk's plane copies and moves on while those copies run.
  const size_t n_chunks = (cnt + chunk - 1) / chunk;
  std::atomic<long> go{-1};
  std::atomic<int> arrived{0};
  void* const pinned2[2] = {slot.pack_pinned[0], slot.pack_pinned[1]};
  const int n_fields = ds->n_fields;
  const bool f64 = ds->dtype == NOS_F64;
  std::vector<std::thread> pool;
  const int n_workers = (e == hipSuccess && n_chunks > 0) ? threads : 0;
  for (int w = 0; w < n_workers; ++w) {
    pool.emplace_back([&, w]() {
      for (size_t c = 0; c < n_chunks; ++c) {
        while (go.load(std::memory_order_acquire) < long(c)) std::this_thread::yield();
        if (go.load(std::memory_order_acquire) == LONG_MAX) return;  // the caller gave up
        const size_t first = c * chunk, count = std::min(chunk, cnt - first);
        const size_t per = (count + size_t(n_workers) - 1) / size_t(n_workers);
        const size_t lo = std::min(count, size_t(w) * per), hi = std::min(count, lo + per);
        if (lo < hi) {
          if (f64)
            pack_range<double>(host, stride, fo, n_fields, ndt, first, lo, hi - lo, chunk, tile_log2,
                               static_cast<double*>(pinned2[c & 1]));
          else
            pack_range<float>(host, stride, fo, n_fields, ndt, first, lo, hi - lo, chunk, tile_log2,
                              static_cast<float*>(pinned2[c & 1]));
        }
        arrived.fetch_add(1, std::memory_order_release);
      }
    });
  }
  bool used[2] = {false, false};
  for (size_t c = 0; c < n_chunks && e == hipSuccess; ++c) {
    const int buf = int(c & 1);
    const size_t first = c * chunk, count = std::min(chunk, cnt - first);
    if (used[buf]) e = hipEventSynchronize(slot.pack_done[buf]);  // its previous copies have left the pinned buffer
    if (e != hipSuccess) break;
    go.store(long(c), std::memory_order_release);
    while (arrived.load(std::memory_order_acquire) < int(c + 1) * n_workers) std::this_thread::yield();
    if (tile_log2 == 0) {
      for (int f = 0; f < n_fields && e == hipSuccess; ++f) {
        char* dst = static_cast<char*>(sh.data) + nos::plane_offset(sh.layout, first, ndt ? nos::ndt_stored_plane(f) : f) * es;
        const char* src = static_cast<const char*>(slot.pack_pinned[buf]) + size_t(f) * chunk * es;
        e = hipMemcpyAsync(dst, src, count * es, hipMemcpyHostToDevice, slot.copy_stream);
      }
    } else {  // the chunk's tiles are one contiguous piece of the dataset (the pads of the last tile are zeroed below)
      const size_t tile = size_t(1) << tile_log2;
      const size_t tiles = (count + tile - 1) / tile;
      char* dst = static_cast<char*>(sh.data) + (first >> tile_log2) * sh.layout.tile_stride * es;
      e = hipMemcpyAsync(dst, slot.pack_pinned[buf], tiles * sh.layout.tile_stride * es, hipMemcpyHostToDevice, slot.copy_stream);
      if (ndt && e == hipSuccess) {  // the S region's tiles of the chunk
        char* dst_s = static_cast<char*>(sh.data) + (sh.layout.s_offset + (first >> tile_log2) * sh.layout.s_tile_stride) * es;
        const char* src_s = static_cast<const char*>(slot.pack_pinned[buf]) + size_t(nos::kNdtStreamed) * chunk * es;
        e = hipMemcpyAsync(dst_s, src_s, tiles * sh.layout.s_tile_stride * es, hipMemcpyHostToDevice, slot.copy_stream);
      }
    }
    if (e == hipSuccess) e = hipEventRecord(slot.pack_done[buf], slot.copy_stream);
    used[buf] = true;
  }
  go.store(LONG_MAX, std::memory_order_release);  // releases workers still waiting (error path); no-op otherwise
  for (std::thread& th : pool) th.join();
  if (e == hipSuccess) e = hipStreamSynchronize(slot.copy_stream);
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "host-pack ingestion failed: %s", hipGetErrorString(e));
  if (ndt && cnt > 0) {  // U (S = QU) from the S just copied, in the dataset's element type
    const dim3 grid(unsigned((cnt + 255) / 256));
    if (f64)
      hipLaunchKernelGGL((nos::ndt_u_planes_kernel<double>), grid, dim3(256), 0, slot.stream, sh.layout,
                         static_cast<double*>(sh.data), uint64_t(0), uint64_t(cnt));
    else
      hipLaunchKernelGGL((nos::ndt_u_planes_kernel<float>), grid, dim3(256), 0, slot.stream, sh.layout,
                         static_cast<float*>(sh.data), uint64_t(0), uint64_t(cnt));
    NOS_HIP_CHECK(hipGetLastError());
  }
  int rc = (ds->dtype == NOS_F64) ? zero_pad_launch<double>(stored_planes(ds), sh.layout, sh.data, slot.stream)
                                  : zero_pad_launch<float>(stored_planes(ds), sh.layout, sh.data, slot.stream);
  if (rc != NOS_OK) return rc;
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  return NOS_OK;
}

int create_from_records(nos_ctx* ctx, int kind, size_t n, const void* records, size_t stride,
                        const size_t* field_offsets, int dtype, nos_dataset** out) {
  if ((!records && n > 0) || !field_offsets) return fail(NOS_ERR_INVALID_ARGUMENT, "records / offsets is NULL");
  nos_dataset* ds = nullptr;
  int rc = dataset_new(ctx, kind, n, dtype, out, &ds);
  if (rc != NOS_OK) return rc;
  nos::FieldOffsets fo{};
  for (int f = 0; f < ds->n_fields; ++f) {
    if (field_offsets[f] + sizeof(double) > stride || (field_offsets[f] % sizeof(double)) != 0) {
      nos_dataset_destroy(ds);
      return fail(NOS_ERR_INVALID_ARGUMENT, "field offset %d out of record / misaligned", f);
    }
    fo.off[f] = uint32_t(field_offsets[f]);
  }
  if (stride % sizeof(double) != 0) {
    nos_dataset_destroy(ds);
    return fail(NOS_ERR_INVALID_ARGUMENT, "record stride must be a multiple of 8");
  }
  const size_t chunk_records = std::max<size_t>(1, (size_t(64) << 20) / stride);
  const unsigned char* host = static_cast<const unsigned char*>(records);
  // Which ingestion: "unpack" ships the raw records and unpacks on the device (no host work, 304 B/record over PCIe);
  // "pack" gathers on the host with a few threads and ships planes (120 / 60 B/record).  auto = pack for large planar
  // inputs when the host has threads to spare (NOS_INGEST=pack|unpack forces, NOS_INGEST_THREADS sets the count).
  const std::string mode = ctx->settings.ingest == 1 ? "pack" : (ctx->settings.ingest == 2 ? "unpack" : "auto");
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  int pack_threads = ctx->settings.ingest_threads > 0 ? ctx->settings.ingest_threads : int(std::min(16u, hw / 2));
  // planar planes, or tiles that divide the 256 Ki-record chunk of the pack path (the fp32 default: 1 024-item tiles)
  const bool packable = ds->tile == 0 || (ds->tile <= (size_t(256) << 10) && ((size_t(256) << 10) % ds->tile) == 0);
  const bool use_pack = packable && pack_threads >= 1 &&
                        (mode == "pack" || (mode == "auto" && n >= size_t(800000) && pack_threads >= 8));
  size_t begin = 0;
  for (Shard& sh : ds->shards) {
    if (use_pack) {
      rc = ingest_host_pack(ctx, ds, sh, host + begin * stride, stride, fo, pack_threads);
      if (rc != NOS_OK) {
        nos_dataset_destroy(ds);
        return rc;
      }
      begin += sh.layout.n;
      continue;
    }
    DeviceSlot& slot = ctx->slots[sh.slot];
    const size_t cnt = sh.layout.n;
    hipError_t e = hipSetDevice(slot.device);
    // persistent per-device ingestion resources (stream, events, staging buffers sized to what this call needs)
    const size_t want_stage = std::min(chunk_records, std::max<size_t>(cnt, 1)) * stride;
    if (e == hipSuccess && slot.copy_stream == nullptr) e = hipStreamCreateWithFlags(&slot.copy_stream, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b)
      if (slot.ing_done[b] == nullptr) e = hipEventCreateWithFlags(&slot.ing_done[b], hipEventDisableTiming);
    if (e == hipSuccess && slot.ing_copied == nullptr) e = hipEventCreateWithFlags(&slot.ing_copied, hipEventDisableTiming);
    if (e == hipSuccess && slot.stage_bytes < want_stage) {
      for (int b = 0; b < 2; ++b) {
        if (slot.stage[b]) (void)hipFree(slot.stage[b]);
        slot.stage[b] = nullptr;
      }
      slot.stage_bytes = 0;
      const size_t grow = std::max(want_stage, size_t(4) << 20);
      for (int b = 0; b < 2 && e == hipSuccess; ++b) e = device_alloc(slot, &slot.stage[b], grow);
      if (e == hipSuccess) slot.stage_bytes = grow;
    }
    void** stage = slot.stage;
    hipEvent_t* done = slot.ing_done;
    hipStream_t copy_stream = slot.copy_stream;
    hipEvent_t copied = slot.ing_copied;
    int buf = 0;
    bool used[2] = {false, false};
    for (size_t first = 0; first < cnt && e == hipSuccess && rc == NOS_OK; first += chunk_records, buf ^= 1) {
      const size_t count = std::min(chunk_records, cnt - first);
      if (used[buf]) e = hipStreamWaitEvent(copy_stream, done[buf], 0);  // unpack of the previous use finished
      if (e == hipSuccess)
        e = hipMemcpyAsync(stage[buf], host + (begin + first) * stride, count * stride, hipMemcpyHostToDevice,
                           copy_stream);
      if (e == hipSuccess) e = hipEventRecord(copied, copy_stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(slot.stream, copied, 0);
      if (e == hipSuccess) {
        rc = (dtype == NOS_F64)
                 ? unpack_launch<double>(static_cast<unsigned char*>(stage[buf]), stride, fo, ds->n_fields, first, count,
                                         sh.layout, sh.data, slot.stream)
                 : unpack_launch<float>(static_cast<unsigned char*>(stage[buf]), stride, fo, ds->n_fields, first, count,
                                        sh.layout, sh.data, slot.stream);
        if (rc == NOS_OK) e = hipEventRecord(done[buf], slot.stream);
        used[buf] = true;
      }
    }
    if (e == hipSuccess && rc == NOS_OK)
      rc = (dtype == NOS_F64) ? zero_pad_launch<double>(stored_planes(ds), sh.layout, sh.data, slot.stream)
                              : zero_pad_launch<float>(stored_planes(ds), sh.layout, sh.data, slot.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    if (e != hipSuccess || rc != NOS_OK) {
      nos_dataset_destroy(ds);
      if (rc != NOS_OK) return rc;
      return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "record ingestion failed: %s",
                  hipGetErrorString(e));
    }
    begin += cnt;
  }
  *out = ds;
  return NOS_OK;
}

int zero_pad(int dtype, int n_fields, const nos::TiledLayout& L, void* dst, hipStream_t stream) {
  return dtype == NOS_F64 ? zero_pad_launch<double>(n_fields, L, dst, stream) : zero_pad_launch<float>(n_fields, L, dst, stream);
}

int unpack_records(int dtype, const unsigned char* d_rec, size_t stride, const nos::FieldOffsets& fo, int n_fields,
                   size_t first, size_t count, const nos::TiledLayout& L, void* dst, hipStream_t stream) {
  return dtype == NOS_F64 ? unpack_launch<double>(d_rec, stride, fo, n_fields, first, count, L, dst, stream)
                          : unpack_launch<float>(d_rec, stride, fo, n_fields, first, count, L, dst, stream);
}

}  // namespace nosd

using namespace nosd;

// ====================================================================== C ABI

extern "C" {

int nos_ndt_dataset_create(nos_ctx* ctx, size_t n, const double* const planes[NOS_NDT_PLANES], int dtype,
                           nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_host_planes(ctx, kKindNdt, n, planes, dtype, out_ds);
}

int nos_reproj_dataset_create(nos_ctx* ctx, size_t n, const double* const planes[NOS_REPROJ_PLANES], int dtype,
                              nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_host_planes(ctx, kKindReproj, n, planes, dtype, out_ds);
}

int nos_ndt_dataset_create_from_device(nos_ctx* ctx, size_t n, const void* const d_planes[NOS_NDT_PLANES],
                                       int src_dtype, int dtype, nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_device_planes(ctx, kKindNdt, n, d_planes, src_dtype, dtype, out_ds);
}

int nos_reproj_dataset_create_from_device(nos_ctx* ctx, size_t n, const void* const d_planes[NOS_REPROJ_PLANES],
                                          int src_dtype, int dtype, nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_device_planes(ctx, kKindReproj, n, d_planes, src_dtype, dtype, out_ds);
}

int nos_ndt_dataset_create_from_records(nos_ctx* ctx, size_t n, const void* records, size_t stride_bytes,
                                        const size_t field_offsets[NOS_NDT_PLANES], int dtype,
                                        nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_records(ctx, kKindNdt, n, records, stride_bytes, field_offsets, dtype, out_ds);
}

int nos_reproj_dataset_create_from_records(nos_ctx* ctx, size_t n, const void* records, size_t stride_bytes,
                                           const size_t field_offsets[NOS_REPROJ_PLANES], int dtype,
                                           nos_dataset** out_ds) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  return create_from_records(ctx, kKindReproj, n, records, stride_bytes, field_offsets, dtype, out_ds);
}

int nos_dataset_destroy(nos_dataset* ds) {
  nosd::CtxGuard guard_(ds ? ds->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!ds) return NOS_OK;
  for (Shard& sh : ds->shards) {
    if (sh.data || sh.index || sh.table) (void)hipSetDevice(ds->ctx->slots[sh.slot].device);
    if (sh.data) {
      // the stream may still be reading the buffer (asynchronous entry points): wait before it is handed on
      if (sh.pooled) {
        (void)hipStreamSynchronize(ds->ctx->slots[sh.slot].stream);
        pool_release(ds->ctx->slots[sh.slot], sh.data, sh.capacity);
      } else {
        (void)hipFree(sh.data);
      }
    }
    if (sh.index && !sh.one_block) (void)hipFree(sh.index);
    if (sh.table && !sh.one_block) (void)hipFree(sh.table);
  }
  delete ds;
  return NOS_OK;
}

int nos_dataset_set_simd_class(nos_dataset* ds, int on) {
  if (!ds) return fail(NOS_ERR_INVALID_ARGUMENT, "dataset is NULL");
  nosd::CtxGuard guard_(ds->ctx);
  ds->simd_class = on != 0 ? 1 : 0;
  return NOS_OK;
}
size_t nos_dataset_size(const nos_dataset* ds) { return ds ? ds->n : 0; }
int nos_dataset_dtype(const nos_dataset* ds) { return ds ? ds->dtype : -1; }
size_t nos_dataset_stream_bytes(const nos_dataset* ds) {
  if (!ds) return 0;
  if (ds->kind == kKindNdtIndexed)  // point (3 values) + one 4-byte voxel id per slot; the voxel table is cache resident
    return ds->n * (3 * elem_size(ds->dtype) + sizeof(int32_t) * size_t(ds->shards.empty() ? 0 : ds->shards[0].n_slots));
  // flat datasets: the planes of the caller's record (nos.h).  Flat NDT kernels stream 12 of the 15 (p, mu, U with S = QU;
  // fp32 3-DoF: p, mu, S) — the figure stays the record's, which the test suite pins.
  return ds->n * size_t(ds->n_fields) * elem_size(ds->dtype);
}

}  // extern "C"
