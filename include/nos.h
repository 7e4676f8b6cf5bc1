/*
 * nos.h — C ABI of the MI355X (gfx950) Gauss-Newton normal-equation assembly path.
 *
 * This is the drop-in boundary for the one data-parallel hot path of
 * ChanghyeonKim93/nonlinear_optimizer_for_slam: per-correspondence residual +
 * analytic Jacobian + robust weight, reduced into the upper triangle of JᵀJ, Jᵀr and
 * the robust cost.  Every entry point replaces one piece of the reference's CPU path;
 * the reference location is cited next to each declaration (paths are relative to the
 * reference checkout, `NO/` = nonlinear_optimizer/, `MDM/` =
 * NO/mahalanobis_distance_minimizer/, `REM/` = NO/reprojection_error_minimizer/).
 *
 * Conventions
 *   - plain C, no exceptions cross this boundary; every function returns a nos_status
 *     (0 = NOS_OK) and never a torch / Eigen / STL type.
 *   - rotation matrices are row-major double[9]; translations double[3].
 *   - parameter order of gradient / Hessian is (t_x, t_y, t_z, w_x, w_y, w_z), the
 *     order the reference's update step uses (MDM/..._analytic_simd.cc:86-87).
 *   - NDT planes are ordered  px py pz  mx my mz  s00 s01 s02 s10 s11 s12 s20 s21 s22
 *     (point, NDT mean, row-major sqrt-information) — the 15 scalars the analytic
 *     solvers read from each 304-byte Correspondence (MDM/types.h:11-26,
 *     MDM/..._analytic.cc:164-168); reprojection planes are  X Y Z  u v
 *     (REM/types.h:25-28).
 *   - results:  out28 = { H upper triangle row-major (21) | g (6) | cost (1) },
 *               out10 = { H upper triangle row-major (6)  | g (3) | cost (1) }.
 *     The same 28 / 10 numbers the reference returns in PartialResult
 *     (MDM/mahalanobis_distance_minimizer.h:14-18).
 *   - all N correspondences are processed (the single-thread scalar class's behaviour,
 *     MDM/..._analytic.cc:98-100), no SIMD tail is dropped.
 */
#ifndef NOS_H_
#define NOS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NOS_NDT_PLANES 15
#define NOS_REPROJ_PLANES 5
#define NOS_NDT6_OUT 28
#define NOS_NDT3_OUT 10
#define NOS_REPROJ_OUT 28

typedef enum nos_status {
  NOS_OK = 0,
  NOS_ERR_INVALID_ARGUMENT = 1,
  NOS_ERR_NO_DEVICE = 2,     /* no HIP device / runtime not usable: there is NO CPU fallback */
  NOS_ERR_HIP = 3,           /* a HIP runtime call failed; see nos_last_error() */
  NOS_ERR_OUT_OF_MEMORY = 4,
  NOS_ERR_WRONG_KIND = 5,    /* e.g. an NDT entry point given a reprojection dataset */
  NOS_ERR_UNSUPPORTED = 6
} nos_status;

/* Storage / arithmetic type of a device-resident dataset.  NOS_F64 mirrors the scalar
 * fp64 classes (MDM/..._analytic.cc), NOS_F32 mirrors the SIMD classes which cast to
 * float at pack time (MDM/..._analytic_simd.cc:25-27).  Reductions are always fp64. */
typedef enum nos_dtype { NOS_F64 = 0, NOS_F32 = 1 } nos_dtype;

/* Device-side restatement of NO/loss_function.h (a host virtual cannot cross to the
 * GPU).  kind NONE: rho = s, w = 1 (loss_function_ == nullptr branch,
 * MDM/..._analytic.cc:44-48).  EXPONENTIAL(a = c1, b = c2): NO/loss_function.h:28-33.
 * HUBER(a = threshold): NO/loss_function.h:57-66. */
typedef enum nos_loss_kind {
  NOS_LOSS_NONE = 0,
  NOS_LOSS_EXPONENTIAL = 1,
  NOS_LOSS_HUBER = 2
} nos_loss_kind;

typedef struct nos_loss {
  int32_t kind; /* nos_loss_kind */
  int32_t reserved;
  double a; /* c1 (exponential) | threshold (huber) */
  double b; /* c2 (exponential) */
} nos_loss;

typedef struct nos_ctx nos_ctx;
typedef struct nos_dataset nos_dataset;

/* ---- context ------------------------------------------------------------------
 * Replaces MultiThreadExecutor (NO/multi_thread_executor.h:51-73): instead of a pool
 * of pinned threads the context owns, per listed device, one HIP stream, a block-partial
 * workspace and a pinned result slot.  One process per GPU passes n_devices = 1 and
 * all-reduces the 28 scalars with RCCL itself (see nos_*_accumulate_async); listing
 * several devices gives the single-process fan-out the reference's thread pool had
 * (correspondences are split into contiguous ranges, partials are summed on the
 * caller in device order — MDM/..._analytic_simd.cc:55-76).
 * The same device may be listed more than once (useful for testing the sharded path
 * on a one-GPU box). */
int nos_ctx_create(const int* device_ids, int n_devices, nos_ctx** out_ctx);
int nos_ctx_destroy(nos_ctx* ctx);
int nos_ctx_num_devices(const nos_ctx* ctx);
/* Make shard `shard`'s launches go to an externally owned hipStream_t (e.g. the
 * stream torch uses), so that collectives enqueued by the caller order after them.
 * Passing NULL restores the context's own stream. */
int nos_ctx_set_stream(nos_ctx* ctx, int shard, void* hip_stream);
/* Block until all work enqueued on the context's streams has finished. */
int nos_ctx_synchronize(nos_ctx* ctx);

/* ---- inter-process reduction (one process per GPU) ------------------------------
 * The reference sums per-thread partials on the caller (MDM/..._analytic_simd.cc:70-75); with
 * one process per GPU that sum is a single RCCL all-reduce of the 28 (10) doubles over xGMI.
 * Rank 0 calls nos_comm_get_unique_id and hands the 128 bytes to every rank out of band
 * (torch.distributed / MPI / a file); every rank then calls nos_ctx_comm_init (collective).
 * From then on every *_accumulate / *_accumulate_async on that context returns the sum over
 * all ranks (identical bits on every rank), so the unchanged host LM loop runs in lock-step.
 * RCCL is loaded with dlopen on first use. */
#define NOS_COMM_ID_BYTES 128
int nos_comm_get_unique_id(unsigned char id[NOS_COMM_ID_BYTES]);
int nos_ctx_comm_init(nos_ctx* ctx, int n_ranks, int rank, const unsigned char id[NOS_COMM_ID_BYTES]);
int nos_ctx_comm_size(const nos_ctx* ctx); /* 0 if no communicator */
/* Ranks RCCL itself reports for the context's communicator (ncclCommCount); *count = 0 without an RCCL communicator. */
int nos_ctx_comm_rccl_count(const nos_ctx* ctx, int* count);
/* One line of JSON: HIP version the library was built with, HIP runtime / driver version mapped into this process,
 * the files the runtime and librccl were loaded from, RCCL's version, and two verdicts — "same_rocm_tree" (runtime and
 * librccl come from one directory) and "runtime_matches_build" (major.minor).  librccl is bound on first use: from
 * $NOS_RCCL_PATH, else from the directory of the HIP runtime already in the process, else the loader's default. */
int nos_runtime_info(char* buf, size_t capacity);
/* Alternative communicator for ranks on ONE node: a mailbox in POSIX shared memory (name, starting with '/',
 * chosen by the caller and identical on every rank).  Collective: rank 0 unlinks any segment of that name, creates a
 * fresh one exclusively and acknowledges every other rank; the other ranks open the name (retrying) and accept a
 * mapping only once rank 0 has acknowledged THEIR random hello word — a segment left behind by a crashed run is never
 * joined (bounded by NOS_SHM_ATTACH_TIMEOUT_MS, default 30 s).  Rank 0 may call nos_comm_shm_unlink once all ranks have returned.  The sums are then exchanged INSIDE the launch: the workgroup
 * that completes a GPU's sums stores them in its mailbox slot, waits (bounded) for the other ranks' slots and adds
 * them in rank order, so nos_*_accumulate and nos_*_solve return identical bits on every rank with no extra
 * kernel, no RCCL call and no host step per iteration.  This is the reference's "sum the per-thread partials"
 * (MDM/..._analytic_simd.cc:70-75) across processes.  At most 64 ranks; all ranks must issue the same sequence of
 * calls; a rank that never arrives makes the others return NOS_ERR_HIP after 8 s instead of hanging. */
int nos_ctx_comm_init_shm(nos_ctx* ctx, int n_ranks, int rank, const char* shm_name);
/* The same communicator with its SLOTS in device memory: every rank allocates its slot buffer as fine-grained device
 * memory, exports it with hipIpcGetMemHandle through the shared-memory segment (which keeps the handshake and control
 * words only) and opens the buffers of its peers; inside the launch a rank then writes its 28 sums and its round number
 * straight into every peer's buffer — device to device (between GPUs of a node presumably over xGMI; not verified on more than
 * one GPU) — and polls only its own memory.  Same
 * slots, same round numbers, same rank-order sum: bit-identical to the host-memory form.  NOS_ERR_UNSUPPORTED when the
 * platform refuses the fine-grained allocation or the IPC export / import.
 * With this communicator nos_*_solve keeps the whole LM loop in ONE launch on every rank: the exchange is a third stage of the
 * in-launch all-reduce (8-byte {tag | half} granules pushed into the peers' buffers, bounded wait of 8 s).  If a rank has to
 * give up (GPU shared with other processes), all ranks abandon that launch together, redo the solve with one launch per
 * iteration (nos_lm_report.fallback = 1) and pause the one-launch form for the next 64 solves, doubling on repeats — counted
 * in solves so that all ranks switch back in the same call. */
int nos_ctx_comm_init_shm_device(nos_ctx* ctx, int n_ranks, int rank, const char* shm_name);
int nos_comm_shm_unlink(const char* shm_name);
/* Leaves whichever communicator the context has (collective for RCCL); nos_ctx_destroy does it implicitly. */
int nos_ctx_comm_destroy(nos_ctx* ctx);
/* Sum `count` (<= 28) host doubles over the ranks, in place (diagnostic / self-test). */
int nos_ctx_comm_allreduce(nos_ctx* ctx, double* values, int count);

/* ---- datasets ------------------------------------------------------------------
 * Replaces the per-Solve AoS→SoA pack (SOAData, MDM/..._analytic_simd.h:15-19 and
 * .cc:19-28; AlignedBufferVarious, MDM/..._analytic_simd_various.h:14-44; AlignedBuffer,
 * REM/..._analytic_simd.h:15-35).  The handle owns device memory in the library's
 * tiled SoA layout; the caller keeps ownership of the host arrays (they are copied). */
int nos_ndt_dataset_create(nos_ctx* ctx, size_t n, const double* const planes[NOS_NDT_PLANES],
                           int dtype, nos_dataset** out_ds);
int nos_reproj_dataset_create(nos_ctx* ctx, size_t n,
                              const double* const planes[NOS_REPROJ_PLANES], int dtype,
                              nos_dataset** out_ds);
/* Same, from planes that already live in device memory of the context's FIRST device
 * (element type given by src_dtype, planes contiguous, length n each).  The data is
 * re-tiled on the device; the source planes are not referenced afterwards.
 * Only valid for single-device contexts. */
int nos_ndt_dataset_create_from_device(nos_ctx* ctx, size_t n,
                                       const void* const d_planes[NOS_NDT_PLANES],
                                       int src_dtype, int dtype, nos_dataset** out_ds);
int nos_reproj_dataset_create_from_device(nos_ctx* ctx, size_t n,
                                          const void* const d_planes[NOS_REPROJ_PLANES],
                                          int src_dtype, int dtype, nos_dataset** out_ds);
/* Ingest the reference's array-of-structures records directly: `records` points at n
 * host records of `stride_bytes` each; the 15 (or 5) doubles are found at the given
 * byte offsets inside a record (for the reference's 304-byte Correspondence:
 * point @0, ndt.mean @128, ndt.sqrt_information @224 column-major — Eigen default —
 * see INTEGRATION.md).  Records are staged through pinned memory and unpacked on the
 * device (K6 in SURVEY.md §2.2). */
int nos_ndt_dataset_create_from_records(nos_ctx* ctx, size_t n, const void* records,
                                        size_t stride_bytes,
                                        const size_t field_offsets[NOS_NDT_PLANES], int dtype,
                                        nos_dataset** out_ds);
int nos_reproj_dataset_create_from_records(nos_ctx* ctx, size_t n, const void* records,
                                           size_t stride_bytes,
                                           const size_t field_offsets[NOS_REPROJ_PLANES],
                                           int dtype, nos_dataset** out_ds);
int nos_dataset_destroy(nos_dataset* ds);
size_t nos_dataset_size(const nos_dataset* ds);
int nos_dataset_dtype(const nos_dataset* ds);
/* Bytes of the dataset's correspondences as the caller gives them: n × planes × sizeof(element).  Flat NDT datasets
 * also store U of every sqrt-information S = QU (triangular, computed on the device when the dataset is made), and the 6-DoF and fp64
 * 3-DoF kernels stream p, mu and U only — 12 of these 15 planes' worth (96 / 48 B per fp64 / fp32 correspondence), so
 * a pass moves 0.8 × this figure; the fp32 3-DoF kernels stream p, mu and S (all 15). */
size_t nos_dataset_stream_bytes(const nos_dataset* ds);

/* Semantics of the reference's fp32 ("SIMD") solver classes for solves and accumulates on this dataset (0 = off, the
 * default: the scalar classes' semantics at whatever element type the dataset has):
 *   NDT (6- and 3-DoF): the LM loop keeps lambda and previous_cost in float
 *     (MDM/mahalanobis_distance_minimizer_analytic_simd.cc:38-39,99-101; ..._3dof_simd.cc:73-74,201-207);
 *   reprojection: a correspondence counts when its depth is > 0 (instead of >= min_depth), the mask multiplies the
 *     WEIGHT only — the robust loss of a masked correspondence is still added to the cost
 *     (REM/reprojection_error_minimizer_analytic_simd.cc:66,92,134).
 * The classes' tail drop (only floor(N/8)*8 correspondences are used) and their float 1/fx are the caller's side: create
 * the dataset from the first floor(N/8)*8 records (the drop-in classes do, HipOptions::simd_class).  The lane arithmetic of
 * the un-vendored simd_helper library is NOT reproduced digit for digit (parity unpinned for it). */
int nos_dataset_set_simd_class(nos_dataset* ds, int on);

/* Copy a dataset back to host planes (n_fields arrays of nos_dataset_size doubles, plane order
 * as above).  Diagnostics / tests only. */
int nos_dataset_download(nos_dataset* ds, double* const planes[]);

/* ---- correspondence matching on the device -----------------
 * Replaces MatchPointCloud of the reference's test harness
 * (MDM/tests/simple_optimization_test.cc:296-342): FLANN KDTreeSingleIndex over the valid
 * voxel means + radiusSearch(radius = 1.0 on L2_Simple, i.e. squared distance, max_neighbors
 * = 2) becomes a uniform-grid lookup on the GPU: cell edge sqrt(search_radius_sq) (1 + 2^-30), 27
 * cells per point — the slack makes the search complete under rounding at a cell face, so every
 * valid mean with squared distance < search_radius_sq is a candidate.  nos_ndt_match writes {local point, mean,
 * sqrt-information} for the (up to) two nearest voxels of every scan point straight into a
 * device dataset: slot 2*i + k holds the k-th nearest voxel of point i, an absent neighbour is
 * an all-zero record (contributes nothing).  The dataset is then used with nos_ndt6_accumulate /
 * nos_ndt3_accumulate like any other; nothing returns to the host between matching and solving.
 * means_xyz: [n_voxels][3], sqrt_infos: [n_voxels][9] row-major, valid: optional [n_voxels]
 * (NDT::is_valid, MDM/types.h:21; NULL = all valid), points_xyz: [n_points][3] in the scan's
 * local frame.  Single-device contexts only. */
typedef struct nos_ndt_map nos_ndt_map;
typedef struct nos_scan nos_scan;
int nos_ndt_map_create(nos_ctx* ctx, size_t n_voxels, const double* means_xyz,
                       const double* sqrt_infos, const unsigned char* valid,
                       double search_radius_sq, nos_ndt_map** out_map);
int nos_ndt_map_destroy(nos_ndt_map* map);
size_t nos_ndt_map_size(const nos_ndt_map* map); /* valid voxels */
int nos_scan_create(nos_ctx* ctx, size_t n_points, const double* points_xyz, nos_scan** out_scan);
int nos_scan_destroy(nos_scan* scan);
size_t nos_scan_size(const nos_scan* scan);
/* Optional, once per scan: reorder the points by grid cell of edge cell_edge (in the scan's own frame) so that
 * the points one wavefront of the matcher handles are spatial neighbours (a rigid pose keeps them so).  The
 * matcher's output slots then follow the new order; nos_scan_order gives order[j] = index, in the array handed
 * to nos_scan_create, of the point now stored at position j (identity if the scan was never sorted).  The
 * solver does not care about correspondence order (sums), the reference's harness pushes them in scan order
 * (MDM/tests/simple_optimization_test.cc:296-342). */
int nos_scan_sort_by_cell(nos_scan* scan, double cell_edge);
int nos_scan_order(const nos_scan* scan, uint32_t* order_out);
/* Voxel-grid filter on the device: a NEW, independent scan that holds the first point of every voxel.
 * Replaces FilterPoints of the reference's test harness (MDM/tests/simple_optimization_test.cc:206-223).
 * Rule (exact):
 *   cell     a point's cell is (floor(x * inv_res), floor(y * inv_res), floor(z * inv_res)) with inv_res = 1.0 / voxel_size
 *            computed once on the host in double: one rounded multiply, then floor — the expression the map build and
 *            the voxel map evaluate.  Points that lie exactly on a cell face (the reference's room at 0.1 m and 0.05 m)
 *            make every other formulation (a division, a fused multiply) give another result.
 *   kept     point i is kept iff no point with a smaller ORIGINAL index lies in the same cell.  The original index is
 *            what nos_scan_order reports: the index in the array given to nos_scan_create (the position itself for a
 *            scan that was never sorted nor filtered).  The kept set therefore does not depend on whether
 *            nos_scan_sort_by_cell ran first.
 *   identity two points share a voxel iff their three integer cells are equal.  The reference's Cantor-paired `int`
 *            key agrees with this wherever its arithmetic does not overflow.
 *   output   the kept points in the input's stored order: ascending index for a never-sorted scan (the reference's
 *            push_back order), the spatial order for a cell-sorted one.  nos_scan_order(out) gives every kept point's
 *            original index in the source array; a later nos_scan_sort_by_cell(out) composes with it as usual.  The
 *            input scan is unchanged.
 * The result is the same bytes from run to run and does not depend on launch geometry or on the size of the hash table
 * the call builds (an integer minimum per cell decides, never arrival order).
 * Cells are limited to +-2^20 per axis; single-device contexts only.  A rejected call writes nothing, *out_scan included:
 *   NOS_ERR_INVALID_ARGUMENT  scan or out_scan is NULL; voxel_size is not a finite number > 0; a point has a non-finite
 *                             coordinate
 *   NOS_ERR_UNSUPPORTED       a point's cell lies outside the addressable grid; the scan has >= 2^32 - 1 points
 *   NOS_ERR_OUT_OF_MEMORY     the temporaries (12 B per table entry, the table a power of two >= 2 n entries, plus 8 B per
 *                             point) or the new scan do not fit; nothing stays allocated
 * An empty scan filters to an empty scan. */
int nos_scan_filter(nos_scan* scan, double voxel_size, nos_scan** out_scan);
/* points_xyz_out: [nos_scan_size][3], the points in stored order (diagnostics, tests, callers that need them back) */
int nos_scan_points(const nos_scan* scan, double* points_xyz_out);
/* Motion compensation ("deskewing") on the device: a NEW, independent scan whose points are re-expressed in the sensor
 * frame at one reference instant, under a constant-twist model of the sensor's motion during the sweep.
 * Rule: the sensor pose at time s is T(s) = T(s_ref) Exp((s - s_ref) xi), the twist xi = (v, w) in the body frame and per
 * unit of the time stamps.  A point p measured at time s in the sensor's own frame becomes
 *   tau = s - s_ref,   phi = tau w,   u = tau v,   theta = |phi|
 *   p' = Exp(tau xi) p = R(phi) p + V(phi) u
 *   R(phi) p = p + a (phi x p) + b (phi x (phi x p))
 *   V(phi) u = u + b (phi x u) + c (phi x (phi x u))
 *   a = sin(theta) / theta,  b = (1 - cos(theta)) / theta^2,  c = (theta - sin(theta)) / theta^3   (1, 1/2, 1/6 at theta = 0)
 * — the SE(3) exponential, not the split SO(3) x R^3 interpolation.  twist[6] is translation first, rotation second
 * (v, then w): the parameter order of the 6-DoF solver and of the reference's pose_optimizer update.
 *   times    host array indexed by a point's ORIGINAL index — what nos_scan_order reports: the stored position for a scan
 *            that was never sorted nor filtered, otherwise order[j].  A cell-sorted or a filtered scan is therefore
 *            deskewed with the time stamps of the array it came from.  Only entries a stored point refers to are examined.
 *   output   same n, same stored order; nos_scan_order(out) is a copy of the input's (absent if the input has none).  The
 *            input scan is unchanged.  An empty scan deskews to an empty scan.
 *   exact    tau == 0 leaves a point's coordinates equal (==) to the input's, and so does xi == 0 (a -0.0 may come back as
 *            +0.0).  The bits of a point's result are a function of (p, s, s_ref, xi) alone: the same from run to run,
 *            whatever the stored position or the launch geometry — deskewing a sorted or filtered scan gives the rows
 *            [order] of the deskew of the source.  Large theta is legal (the math library reduces the argument).
 *            Point coordinates are not validated: IEEE arithmetic carries non-finite ones through.
 * Single-device contexts only.  A rejected call writes nothing, *out_scan included, and leaves nothing allocated:
 *   NOS_ERR_INVALID_ARGUMENT  scan, out_scan or twist is NULL; times is NULL while the scan has points; reference_time or
 *                             a twist component is not finite; a stored point's original index is >= n_times; a stored
 *                             point's time stamp is not finite (the error text names the stored position for these two)
 *   NOS_ERR_UNSUPPORTED       the context has more than one device; the scan has >= 2^32 - 1 points
 *   NOS_ERR_OUT_OF_MEMORY     the time stamps (8 B per entry of times) or the new scan do not fit */
int nos_scan_deskew(nos_scan* scan, const double* times, size_t n_times, double reference_time,
                    const double twist[6], nos_scan** out_scan);
/* Place recognition on the device: the Scan Context descriptor of a scan (Kim & Kim, IROS 2018) and a database of stored
 * descriptors that is searched exhaustively — every stored place at every yaw — in one launch.
 *
 * Parameters.  n_rings 1 ... 64, n_sectors 1 ... 128, max_range finite and > 0, z_floor finite; anything else is
 * NOS_ERR_INVALID_ARGUMENT before any device is touched.
 *
 * Descriptor of a scan: n_rings x n_sectors doubles, ring-major, desc[i * n_sectors + j].  Points are taken in the scan's
 * own sensor frame (no pose; the stored order does not matter).  Operation by operation, in double:
 *   used     a point (x, y, z) is used when x, y, z are all finite, z >= z_floor, and r = sqrt(x*x + y*y) < max_range
 *            (x*x + y*y may be fused);
 *   ring     i = min(int(floor(r * (n_rings / max_range))), n_rings - 1) — the quotient n_rings / max_range formed once;
 *            a ring boundary belongs to the outer ring;
 *   sector   a = atan2(y, x); if a < 0: a = a + 2 pi; j = int(floor(a * (n_sectors / (2 pi)))), and j = j - n_sectors when
 *            that gives n_sectors (a rounded up to 2 pi).  A point with x == 0 && y == 0 goes to sector 0;
 *   bin      max(z) over its points, then ONE subtraction per bin: value = max(z) - z_floor, so the value is one rounding
 *            of a double the scan contains.  An empty bin holds 0.0;
 *   n_used   the number of points that were used.
 * The maximum is an integer maximum of an order-preserving key of z: the result is the same bits from run to run and
 * for every order of the points.  An empty scan gives the all-zero descriptor and n_used = 0.
 *
 * Distance between a query q and a candidate c of the same parameters (R = n_rings, S = n_sectors):
 *   norm     |a_j| = sqrt(sum_i a[i][j]^2), i ascending;
 *   shift    for s = 0 ... S - 1:  d_s = (sum_j (1 - (sum_i q[i][j] * c[i][(j + s) mod S]) / (|q_j| * |c_(j+s)|))) / m
 *            over the columns j, ascending, for which both |q_j| > 0 and |c_(j+s)| > 0; m is their number; i ascending;
 *            d_s = 1.0 when m == 0;
 *   result   d = min_s d_s and the smallest s that attains it.  d is not clamped (rounding can leave -1e-16).
 *
 * Sign of the yaw.  The descriptor q of a scan taken from a sensor yawed by +phi about z relative to the sensor of a
 * stored scan c of the same place has q_j ~ c_(j+s) with s ~ phi * S / (2 pi): a point at azimuth a in the stored frame is
 * at a - phi in the query's.  The rough pose of the query is therefore T_stored o Rz(2 pi s / S).
 *
 *   nos_scan_descriptor       the descriptor of a scan to the host, and n_used (may be NULL).
 *   nos_place_db_create       an empty database of one parameter set; reserve: slots allocated up front (0: none).  The
 *                             store grows by doubling with a device-to-device copy.
 *   nos_place_db_add          appends a host descriptor (any doubles; ring-major); *index (may be NULL) = its position.
 *   nos_place_db_add_scan     appends the descriptor of a scan without it visiting the host; n_used may be NULL.
 *   nos_place_db_get          stored descriptor `index`, ring-major — the doubles that were added, bit for bit.
 *   nos_place_db_search       n_queries host descriptors against entries first ... first + count - 1: distance_out and
 *                             shift_out are [n_queries][count].  One launch, one host wait.  first + count > size is
 *                             NOS_ERR_INVALID_ARGUMENT; count == 0 or n_queries == 0 succeeds and writes nothing.
 *   nos_place_db_search_scan  the same for the descriptor of a scan, built and searched on the device: one host wait.
 * A pair's distance and shift are a function of the two descriptors alone: the same bits whatever the number of queries,
 * the window, the database's capacity, and whether the query came from the host or from a scan.
 * Single-device contexts only (NOS_ERR_UNSUPPORTED); a scan of >= 2^32 - 1 points is NOS_ERR_UNSUPPORTED.  NULL arguments
 * (n_used and index excepted) and a scan of another context than the database's are NOS_ERR_INVALID_ARGUMENT, rejected
 * before any device is touched with nothing written.  nos_place_db_destroy(NULL) is NOS_OK; nos_place_db_size(NULL) is 0.
 * The database must be destroyed before its context. */
typedef struct nos_place_params {
  int32_t n_rings;
  int32_t n_sectors;
  double max_range;
  double z_floor;
} nos_place_params;
typedef struct nos_place_db nos_place_db;
int nos_scan_descriptor(nos_scan* scan, const nos_place_params* params, double* desc_out, size_t* n_used);
int nos_place_db_create(nos_ctx* ctx, const nos_place_params* params, size_t reserve, nos_place_db** out_db);
int nos_place_db_destroy(nos_place_db* db);
size_t nos_place_db_size(const nos_place_db* db);
int nos_place_db_add(nos_place_db* db, const double* desc, size_t* index);
int nos_place_db_add_scan(nos_place_db* db, nos_scan* scan, size_t* index, size_t* n_used);
int nos_place_db_get(nos_place_db* db, size_t index, double* desc_out);
int nos_place_db_search(nos_place_db* db, const double* queries, int32_t n_queries, size_t first, size_t count,
                        double* distance_out /*[n_queries][count]*/, int32_t* shift_out /*[n_queries][count]*/);
int nos_place_db_search_scan(nos_place_db* db, nos_scan* scan, size_t first, size_t count, double* distance_out,
                             int32_t* shift_out, size_t* n_used);
int nos_ndt_match(nos_ndt_map* map, nos_scan* scan, const double R[9], const double t[3],
                  int max_neighbors, int dtype, nos_dataset** out_ds, size_t* n_matches);
/* Tail drop of the reference's solver classes for a matcher-written dataset.  The scalar 3-DoF class uses only the
 * first floor(N/4)*4 entries of the correspondence vector (MDM/..._analytic_3dof.cc:33-36; the 6-DoF lines of
 * the reference's results directory were captured from a revision that did the same), the SIMD classes floor(N/8)*8
 * (MDM/..._analytic_simd.cc:46-51).  The reference's vector holds matches only, in scan order, nearest first
 * (MDM/tests/simple_optimization_test.cc:320-340); here absent neighbours are zero records, so "drop the last k
 * entries" is: clear the last n_drop NON-EMPTY records in slot order (on the device, asynchronously on the context's
 * stream).  "Empty" is decided by the sqrt-information: a record whose nine S entries are all zero counts as an absent
 * neighbour (what the matcher writes for one) — a real match whose S is identically zero would be taken for empty, but it
 * contributes nothing to the sums either way.  Flat NDT datasets on single-device contexts. */
int nos_dataset_drop_last_matches(nos_dataset* ds, size_t n_drop);

/* ---- voxel-indexed NDT datasets (additive; SURVEY.md §8d "voxel-indexed layout") ------
 * The reference copies the full NDT into every correspondence (MDM/types.h:23-26, :336 of the
 * test harness), hence the flat 120-byte layout.  When many points share a voxel the same sums
 * can be formed from {point, voxel id(s)} plus a table of voxel records: 24 B + 4 B per slot
 * instead of 120 B per correspondence; the table stays in L2 / Infinity Cache and the kernel
 * becomes fp64-ALU bound.  Such a dataset is used with nos_ndt6_accumulate / nos_ndt3_accumulate
 * (and their _async forms) exactly like a flat one and gives the same sums (to rounding: the
 * summation order differs).  index_planes[k][i] = voxel id of point i's k-th correspondence, or
 * -1 for none (n_slots = 1 or 2).  sort_by_voxel != 0 reorders the points by slot-0 voxel id on
 * the device so that a wave's table reads hit a few cache lines (order does not affect the sums).
 * nos_ndt_match_indexed is nos_ndt_match producing this form directly.
 * Roofline accounting: nos_dataset_stream_bytes() = n * (3 * sizeof(elem) + 4 * n_slots); never
 * compare it with the 120-byte figure of the flat layout. */
int nos_ndt_indexed_dataset_create(nos_ctx* ctx, size_t n_points,
                                   const double* const point_planes[3], int n_slots,
                                   const int32_t* const index_planes[], size_t n_voxels,
                                   const double* means_xyz, const double* sqrt_infos, int dtype,
                                   int sort_by_voxel, nos_dataset** out_ds);
int nos_ndt_match_indexed(nos_ndt_map* map, nos_scan* scan, const double R[9], const double t[3],
                          int max_neighbors, int dtype, int sort_by_voxel, nos_dataset** out_ds,
                          size_t* n_matches);

/* Inspection of a voxel-indexed dataset, however it was made (any output pointer may be NULL; a flat dataset:
 * NOS_ERR_WRONG_KIND).  n_slots: id planes; n_voxels: table rows.  The download gives the ids in stored order —
 * index_planes[k] receives nos_dataset_size entries, k < n_slots — and the table [n_voxels][16] = {mean(3), U(6), 7 pads}
 * widened to double. */
int nos_indexed_dataset_info(const nos_dataset* ds, int* n_slots, size_t* n_voxels);
int nos_indexed_dataset_download(nos_dataset* ds, int32_t* const index_planes[], double* table /* [n_voxels][16] */);

/* ---- NDT map construction on the device --------------------
 * Replaces UpdateNdtMap of the reference's test harness
 * (MDM/tests/simple_optimization_test.cc:236-281): voxelise points_xyz ([n][3], map frame) at
 * voxel_resolution, accumulate count / sum / moment per voxel (moment starts at identity,
 * MDM/types.h:14), mean, covariance, symmetric 3x3 eigen-decomposition, eigenvalue flooring and
 * sqrt_information = diag(eigvals^-1/2) * eigenvectors; a voxel is valid with >= 5 points and a
 * largest eigenvalue >= 0.01.  The result is a ready-to-match nos_ndt_map; *out_stats (optional)
 * gives the per-voxel numbers back (voxels ordered by ascending integer cell coordinates).
 * Voxel coordinates are limited to +-2^20 cells per axis, and the statistics are as accurate at that limit as at the
 * origin: count / sum / moment are taken about the corner of the point's cell (cell * voxel_resolution), where the
 * harness's cov = moment / n - mean mean^T cancels eps * resolution^2 instead of eps * |p|^2 (6.7e-4 at 2^20 cells of 1 m,
 * against a floored eigenvalue of 8e-4), and mean = corner + sum / n.  NOS_MAP_REFERENCE_EXACT keeps the raw sums. */
typedef struct nos_map_stats nos_map_stats;
/* flags: 0 reproduces the harness formula sqrt_information = D^-1/2 * V (:275-276), whose result
 * depends on the eigenvector sign convention (here: the first near-largest component of every
 * eigenvector is positive; Eigen's own convention is not reproducible without Eigen);
 * NOS_MAP_PROPER_SQRT_INFORMATION uses D^-1/2 * V^T, the true square root of the inverse
 * covariance, which is sign- and degenerate-subspace-invariant. */
#define NOS_MAP_PROPER_SQRT_INFORMATION 1
/* NOS_MAP_REFERENCE_EXACT: the harness formula with the reference BINARY's rounding — count / sum / moment accumulated per
 * voxel sequentially in point order, Eigen::SelfAdjointEigenSolver<Matrix3d> restated step by step, multiply-adds fused
 * exactly where the reference's -O2 -march=native x86-64 build fuses them (options "map_fma_mask", "map_eigen_version").
 * The map then equals the one the reference's test drivers build bit for bit (tests/golden/ndt_reference_map.npz), and
 * map build -> nos_ndt_match -> nos_ndt6_solve / nos_ndt3_solve reproduce the captured COST / iter lines of the reference's results directory.
 * QUALIFICATION: identical when no voxel with >= 5 points is rejected by the eigenvalue test.  The reference's UpdateNdtMap
 * leaves the function (`return`, not `continue`: .../tests/simple_optimization_test.cc:263-266) at the first such voxel, so
 * every voxel its unordered_map walk would have visited later stays invalid; that order-dependent quirk is deliberately NOT
 * reproduced — voxels are treated independently here (the reference's own room scene has no such voxel).  The defaults of
 * "map_fma_mask" (which multiply-adds are fused, element by element) and the N/4 tail drop the captured 6-DoF runs need are
 * CALIBRATED to the captured x86-64 runs, not derived from today's sources: parity unpinned for other builds
 * of the reference (its aarch64 captures are followed with map_fma_mask = 0, as a band).
 * Voxels are listed in first-seen order (stats and voxel ids).  Not combinable with NOS_MAP_PROPER_SQRT_INFORMATION. */
#define NOS_MAP_REFERENCE_EXACT 2
int nos_ndt_map_build(nos_ctx* ctx, size_t n_points, const double* points_xyz,
                      double voxel_resolution, double search_radius_sq, int flags,
                      nos_ndt_map** out_map, nos_map_stats** out_stats);
size_t nos_map_stats_size(const nos_map_stats* stats);
/* Any output pointer may be NULL.  means [V][3], sqrt_infos [V][9] row-major, valid [V],
 * counts [V], cells [V][3]. */
int nos_map_stats_get(const nos_map_stats* stats, double* means_xyz, double* sqrt_infos,
                      unsigned char* valid, uint32_t* counts, int64_t* cells_xyz);
/* NOS_MAP_REFERENCE_EXACT builds only: eigenvalues [V][3] ascending, before flooring; eigenvectors [V][9] row-major V
 * (column k = eigenvector k) as Eigen returns them. */
int nos_map_stats_get_eigen(const nos_map_stats* stats, double* eigenvalues, double* eigenvectors);
int nos_map_stats_destroy(nos_map_stats* stats);

/* ---- incremental NDT voxel map on the device ---------------------
 * UpdateNdtMap of the reference's test harness is an UPDATE (MDM/tests/simple_optimization_test.cc:236-281): it adds a
 * batch of points to the count / sum / moment of the voxels they fall into, in a map that already exists (:240-252), and
 * re-derives mean, covariance, eigen-decomposition and sqrt-information for the touched voxels only
 * (updated_voxel_key_set, :254-280).  nos_ndt_map_build above is the one-shot form; a nos_voxel_map is the map that
 * exists between calls: a growable, device-resident store of per-voxel key, count, the nine sums about the cell corner,
 * mean, sqrt-information and validity.  An insert costs what its batch costs, never what the points already absorbed would.
 *   flags: 0 (harness formula) or NOS_MAP_PROPER_SQRT_INFORMATION.  NOS_MAP_REFERENCE_EXACT is rejected with
 *   NOS_ERR_UNSUPPORTED: its sequential, calibrated accumulation in point order is a different piece of work (one-shot
 *   builds only).  capacity_hint (voxels) only avoids early growth: arrays and table double as needed.  Single-device
 *   contexts only, like the map build; voxel coordinates are limited to +-2^20 cells per axis (with the accuracy of the
 *   origin throughout, as for the map build: sums about the cell corner), a voxel to 2^32 - 1 points.
 * Voxel ids (the order of nos_voxel_map_stats, the matcher's tie-break in a snapshot) are a function of the sequence of
 * batches alone: batch of first appearance, then ascending integer cell coordinates.  One insert into an empty store
 * gives the statistics of nos_ndt_map_build bit for bit; sums are merged per voxel as store + batch, so results after
 * several inserts agree with a one-shot build to rounding (exactly when the sums are exact).
 * A batch that holds a non-finite coordinate (NOS_ERR_INVALID_ARGUMENT), a point outside the addressable grid or
 * points that would take the voxel they fall into past 2^32 - 1 points (both NOS_ERR_UNSUPPORTED) is rejected as a whole
 * and leaves the store unchanged, like every rejected call here (a rejected call writes nothing, *n_touched included).
 * n_points == 0 is a no-op.  *n_touched (optional) = voxels the batch fell into.
 * The count limit, for nos_voxel_map_insert, _insert_scan, _merge and _import(NOS_IMPORT_ADD) alike: a
 * call that lands a voxel exactly on 2^32 - 1 points is accepted; one that would take ANY destination voxel past it
 * returns NOS_ERR_UNSUPPORTED, and nos_voxel_map_export (cells, counts, sums, stamps, epoch), nos_voxel_map_stats and
 * nos_voxel_map_info are bit for bit what they were; the store stays usable.  The message names a point of the batch
 * that falls into such a voxel — its original index: nos_scan_order's for a cell-sorted scan, else its position —, for a
 * merge a source voxel id, for an add a voxel of the state.  For insert, insert_scan and merge the limit is found on the
 * device after room for the batch was reserved, so capacity, bytes and generation of nos_voxel_map_memory may have
 * grown by the rejected call; results never depend on them.  The check adds no launch and no host wait. */
typedef struct nos_voxel_map nos_voxel_map;
int nos_voxel_map_create(nos_ctx* ctx, double voxel_resolution, double search_radius_sq, int flags,
                         size_t capacity_hint, nos_voxel_map** out);
/* points_xyz: [n_points][3] host memory, map frame (:240-252) */
int nos_voxel_map_insert(nos_voxel_map* map, size_t n_points, const double* points_xyz, size_t* n_touched);
/* The points of a device-resident scan (local frame), warped by R p + t on the device with the operation order of the
 * matcher's warp: what the harness does between OptimizePose and the next UpdateNdtMap.  Only the pose crosses PCIe. */
int nos_voxel_map_insert_scan(nos_voxel_map* map, nos_scan* scan, const double R[9], const double t[3],
                              size_t* n_touched);
/* Any output pointer may be NULL.  n_voxels: voxels that hold at least one point; n_valid: NDT::is_valid among them
 * (MDM/types.h:21); n_points: points absorbed. */
int nos_voxel_map_info(const nos_voxel_map* map, size_t* n_voxels, size_t* n_valid, unsigned long long* n_points);
/* A ready-to-match nos_ndt_map of the store as it is now: an ordinary, independent map (destroy it with
 * nos_ndt_map_destroy) that stays valid after later inserts and after the store is destroyed. */
int nos_voxel_map_snapshot(nos_voxel_map* map, nos_ndt_map** out_map);
/* The per-voxel numbers in voxel-id order; read with nos_map_stats_get, free with nos_map_stats_destroy. */
int nos_voxel_map_stats(nos_voxel_map* map, nos_map_stats** out_stats);
/* The matcher on the LIVE store: MatchPointCloud of the reference's test harness
 * (MDM/tests/simple_optimization_test.cc:296-342) — every scan point warped by R p + t and matched to its (up to)
 * max_neighbors nearest valid voxel means with squared distance < search_radius_sq — without a snapshot.  Arguments and
 * results are those of nos_ndt_match.  Contract: the returned flat dataset and *n_matches are bit for bit what
 * nos_voxel_map_snapshot followed by nos_ndt_match returns for the same arguments, subject to the caveat below.
 * The candidates of a point are the voxel cells its search ball touches, looked up in the key -> slot table the inserts
 * maintain: the call sorts nothing, allocates nothing proportional to the map, launches one kernel plus the dataset's
 * padding and waits once: its work follows the scan, not the size of the map (time not measured yet).  The dataset is independent of the
 * store (the records are copied into it): later inserts, prunes or the store's destruction do not touch it.  The store is
 * not modified: voxels, epoch, generation and stamps stay as they were.
 * Caveat: a voxel is looked for in its own cell.  The cells visited per axis are floor((q - r - g) / resolution) ...
 * floor((q + r + g) / resolution) with r = sqrt(search_radius_sq) and the guard band g = resolution / 1024, so a voxel
 * whose stored mean lies outside its own cell by more than g may be missed where a snapshot would find it.  Rounding alone
 * does not get there: g covers every store with (points in a voxel) x (largest |cell coordinate| + 1) <= 2^42.
 * Rejected before anything runs, *out_ds unwritten: NOS_ERR_INVALID_ARGUMENT for a NULL argument (n_matches may be
 * NULL), a scan of another context, an unknown dtype; NOS_ERR_UNSUPPORTED for max_neighbors outside 1-2, a multi-device
 * context, and a search ball that spans more than 9 cells per axis, i.e. 2 r / resolution + 2 > 9 (at a resolution below
 * r / 3.5 the snapshot's coarser grid is the better structure); NOS_ERR_HIP for a store an earlier failure left undefined. */
int nos_voxel_map_match(nos_voxel_map* map, nos_scan* scan, const double R[9], const double t[3],
                        int max_neighbors, int dtype, nos_dataset** out_ds, size_t* n_matches);
/* nos_voxel_map_match producing the voxel-indexed form of nos_ndt_match_indexed, with a COMPACT voxel table
 * (DESIGN.md §17): no snapshot, and a table sized by the scan, not by the map.
 * Correspondences: those of nos_voxel_map_match — the same warp, distance, strict radius test and tie-break by slot, the
 * same guard band g = resolution / 1024 with its caveat, the same limit of 9 cells per axis; *n_matches equals
 * nos_voxel_map_match's.
 * Table: one row per DISTINCT store slot that any slot plane of this scan references, in ascending store-slot order; a
 * point's id is the rank of its voxel in that list, or -1 for none.  A row is {mean(3), U(6) of S = QU, pad} in the
 * dataset's element type, computed from the store's mean and sqrt-information by the expression every voxel-indexed
 * dataset's table is built with.  The dataset's n_voxels (nos_indexed_dataset_info) is the number of distinct referenced
 * voxels, 0 when nothing matched (the table allocation still holds one readable row).
 * sort_by_voxel as in nos_ndt_match_indexed: a stable order by slot-0 id, absent ids last; 0 keeps the scan's stored order.
 * Consequence: for every point and slot the referenced row holds the values of the row the snapshot route references, and
 * the assemble kernel's geometry depends on the padded point count alone — so with sort_by_voxel = 0 every accumulate and
 * every solve on the returned dataset is bit for bit that of nos_voxel_map_snapshot + nos_ndt_match_indexed(sort_by_voxel
 * = 0), in both element types; with sort_by_voxel = 1 the ids are numbered differently (rank of the store slot here,
 * position in the snapshot's cell order there), so the point order differs and the results are equal to rounding.
 * Work follows the scan: the search, a radix sort of the ids over the bits a slot can have, a unique, a rank pass and the
 * dataset build; no kernel has a grid or trip count proportional to the store's capacity or voxel count and nothing
 * allocated is proportional to them; two host waits (the table's size, the finished dataset).  The store is not
 * modified (nos_voxel_map_memory, voxels, epoch, generation, stamps) and the dataset is independent of it afterwards.
 * Rejections: those of nos_voxel_map_match, same statuses, *out_ds unwritten (and NOS_ERR_UNSUPPORTED for a scan of 2^31
 * points or more: ids and ranks are 32-bit); a table probe that ran through the whole table returns NOS_ERR_HIP and nothing. */
int nos_voxel_map_match_indexed(nos_voxel_map* map, nos_scan* scan, const double R[9], const double t[3],
                                int max_neighbors, int dtype, int sort_by_voxel,
                                nos_dataset** out_ds, size_t* n_matches);
/* Sliding window: removes voxels by a box around a point and / or by age, compacts the survivors on the device and
 * rebuilds the key -> slot table.  The store can shrink.
 * Keep rule (exact):
 *   NOS_PRUNE_BOX: the voxel with integer cell (cx, cy, cz) is kept iff on every axis k
 *       floor((center[k] - half_extent[k]) * inv_res) <= c_k <= floor((center[k] + half_extent[k]) * inv_res),
 *     both bounds computed on the host in double with inv_res = 1.0 / voxel_resolution (the factor an insert multiplies a
 *     coordinate by before floor()), then clamped to the addressable +-2^20 cells (a box that lies wholly beyond them
 *     keeps nothing).  In words: a voxel survives iff its cell [c res, (c + 1) res) meets the closed box; both faces are
 *     inclusive.
 *   NOS_PRUNE_AGE: kept iff epoch - stamp <= max_age, where epoch counts the inserts that returned NOS_OK with at least
 *     one point (a rejected insert does not advance it) and a voxel's stamp is the epoch of the last insert that touched
 *     it.  max_age = 0 keeps only what the last insert touched.  Stamps are the low 32 bits of the 64-bit epoch and the
 *     age is formed modulo 2^32: ages are exact, across epoch 2^32 too, as long as no live voxel is 2^32 or more inserts
 *     old; a max_age of 2^32 - 1 or more keeps every such voxel.
 *   With both bits set a voxel must pass both tests.
 * Voxel ids stay a function of the sequence of calls alone: a prune renumbers the survivors by their rank among the
 * survivors (their relative order is kept); a cell that was removed and is seen again is a new voxel, appended by the
 * usual rule, starting from zero count and zero sums.  n_points of nos_voxel_map_info drops by the removed voxels' counts.
 * When nothing is to be removed the call writes nothing, allocates nothing and leaves `generation` as it was.  When the
 * survivors fit in a quarter of the capacity, the capacity becomes the smallest power of two >= 2 * survivors (never
 * below 16 nor below the capacity the store was created with); otherwise it is unchanged.  Results never depend on it.
 * NOS_ERR_INVALID_ARGUMENT, store unchanged: what == NULL, what->what == 0 or unknown bits, struct_size <
 * sizeof(nos_voxel_prune), (NOS_PRUNE_BOX) a non-finite center or half_extent or a negative half_extent.  A failure
 * half-way (e.g. out of memory for the new block) leaves the store exactly as it was.  *n_removed (optional) = voxels
 * removed; a rejected call does not write it. */
#define NOS_PRUNE_BOX 1
#define NOS_PRUNE_AGE 2
typedef struct nos_voxel_prune {
  size_t struct_size;            /* sizeof(nos_voxel_prune), for later growth */
  int what;                      /* NOS_PRUNE_BOX | NOS_PRUNE_AGE, at least one */
  double center[3];              /* map frame, metric */
  double half_extent[3];         /* >= 0, finite */
  unsigned long long max_age;    /* in inserts */
} nos_voxel_prune;
int nos_voxel_map_prune(nos_voxel_map* map, const nos_voxel_prune* what, size_t* n_removed);
/* Line-of-sight carving, the third prune rule: a ray that ends beyond a voxel has passed through it, so
 * that voxel is free space.  Every point p of `scan` (its local frame) is a ray from the sensor origin; the rays are walked
 * through the grid on the device and the voxels that enough rays cross and (almost) none end in are removed as a prune
 * removes them.  Rule (exact; every operation is an IEEE double operation, fused only where it says so):
 *   Ray.  o = R origin + t and e = R p + t, both with the multiply-adds of nos_voxel_map_insert_scan's warp (per row
 *     fma(R2, z, fma(R0, x, R1 * y)) + t).  d = e - o per component, len = sqrt((dx dx + dy dy) + dz dz), not fused.
 *     The ray is SKIPPED (counted in *n_skipped, counts nothing) iff e has a non-finite component, or !(len > min_range),
 *     or !(len > end_margin), or one of the cells floor(o inv_res), floor(b inv_res), floor(e inv_res) lies outside the
 *     addressable +-2^20 per axis (b below; inv_res = 1.0 / voxel_resolution, the factor an insert multiplies by).
 *     s = (len - end_margin) / len when len <= max_range, else s = max_range / len (a longer ray is walked up to
 *     max_range, not dropped).  Walked segment: a = o, b_k = o_k + s d_k (product rounded, then the sum).
 *   Walk.  ca = floor(a inv_res), cb = floor(b inv_res) per axis.  Axis k makes n_k = |cb_k - ca_k| steps of
 *     sign(cb_k - ca_k).  Its j-th crossing (j = 1 ... n_k) lies at g = double(ca_k + j) res going up and at
 *     double(ca_k - j + 1) res going down, with parameter tau = (g - a_k) / (b_k - a_k): computed from j, never
 *     accumulated (product, two differences, quotient: each rounded once).  An axis with n_k = 0 has no crossing and
 *     nothing is divided for it.  Starting in ca, the walk repeatedly takes the pending crossing with the smallest tau —
 *     equal tau go to x before y before z — and steps that axis.  It visits exactly 1 + n_x + n_y + n_z cells, the first
 *     and the last included, always ends in cb, and visits no cell twice.  Every visited cell the store holds gets
 *     crossings[voxel] += 1.
 *   Hits.  The cell floor(e inv_res) of every ray that is not skipped, if the store holds it, gets hits[voxel] += 1.
 *   Removal.  A voxel goes iff crossings >= min_crossings and hits < min_hits.  The survivors keep their relative order
 *     and are renumbered by rank; the table, n_points, n_valid, generation and the capacity rule behave exactly as
 *     nos_voxel_map_prune with the same keep flags.  epoch and the stamps are untouched (a carve is not an insert).  With
 *     nothing to remove, or with dry_run, nothing of the store is written and generation stays as it was.
 * The counts are integers added by integer atomics: they do not depend on the order of the points or of the lanes.
 * *n_removed (optional): voxels removed; with dry_run, the voxels that would go.  *n_skipped (optional): rays skipped.
 * crossings_out, hits_out (optional): host arrays of n_voxels entries each, n_voxels as nos_voxel_map_info reports it
 * BEFORE the call, in voxel-id order — what a caller needs to accumulate evidence over several scans by a policy of
 * their own.  An empty scan or an empty store is a no-op (zero counts).
 * Rejected, the store and every output unwritten; every NOS_ERR_INVALID_ARGUMENT check comes before any device is touched:
 *   NOS_ERR_INVALID_ARGUMENT  map, scan, R, t or what NULL; struct_size < sizeof(nos_voxel_carve); a non-finite entry of
 *                             R, t or origin; end_margin or min_range negative or not finite; max_range not finite or
 *                             not above 0; min_crossings == 0 or min_hits == 0; a scan of another context;
 *   NOS_ERR_UNSUPPORTED       a multi-device context; 3 (ceil(max_range / voxel_resolution) + 1) > NOS_CARVE_MAX_CELLS,
 *                             the bound on a ray's trip count; a scan of 2^32 - 1 points or more;
 *   NOS_ERR_HIP               a store left undefined by an earlier failure.
 * A failure half-way leaves the store exactly as it was.  Work: one table probe per visited cell and one integer atomic
 * per visited cell the store holds, plus a prune's; one host wait when nothing goes or with dry_run, two otherwise. */
#define NOS_CARVE_MAX_CELLS 4096
typedef struct nos_voxel_carve {
  size_t struct_size;        /* sizeof(nos_voxel_carve), for later growth */
  double origin[3];          /* sensor origin in the SCAN's frame (usually 0, 0, 0) */
  double end_margin;         /* metres cut off the ray before its endpoint, >= 0 */
  double min_range;          /* rays no longer than this are skipped, >= 0 */
  double max_range;          /* longer rays are walked up to this length; finite, > 0 */
  uint32_t min_crossings;    /* >= 1 */
  uint32_t min_hits;         /* >= 1: a voxel with this many endpoints of THIS scan in its cell is protected */
  int dry_run;               /* 1: count only, remove nothing */
} nos_voxel_carve;
int nos_voxel_map_carve(nos_voxel_map* map, nos_scan* scan, const double R[9], const double t[3],
                        const nos_voxel_carve* what, size_t* n_removed, size_t* n_skipped,
                        uint32_t* crossings_out, uint32_t* hits_out);
/* Ray casting: what would a sensor at this pose see?  Every point p of `rays` (any scan, its local frame)
 * is a beam from the sensor origin through p: a measured scan asks what the map predicts along each measured beam, a
 * pattern of unit vectors renders a view.  Each beam is walked through the grid on the device with the carve's walk and
 * ends at the first voxel it hits; the hit test is the one of NDT occupancy maps (Saarinen et al. 2013): the
 * maximum-likelihood point of the voxel's Gaussian along the ray, taken inside the cell.  The store is only read.
 * Rule (every operation an IEEE double operation, fused only where it says so):
 *   Ray.  a = R origin + t and e = R p + t with the carve's warp (per row fma(R2, z, fma(R0, x, R1 * y)) + t).
 *     d = e - a per component, len = sqrt((dx dx + dy dy) + dz dz), not fused.  sc = max_range / len,
 *     b_k = a_k + sc d_k (product rounded, then the sum), w_k = b_k - a_k.  The ray is SKIPPED (voxel -1, range 0.0,
 *     counted in *n_skipped) iff e has a non-finite component, or !(len > 0), or one of the cells floor(a inv_res),
 *     floor(b inv_res) lies outside the addressable +-2^20 per axis (inv_res = 1.0 / voxel_resolution).
 *   Walk.  The walk of nos_voxel_map_carve from a to b: crossing parameters from their index, equal parameters to x
 *     before y before z, 1 + n_x + n_y + n_z cells.  A visited cell has tau_in (0 for the first cell, else the tau of the
 *     crossing that entered it) and tau_out (the tau of the crossing that leaves it, 1 for the last cell).
 *   Test.  Only where the store holds the cell, the voxel v is valid and count[v] >= min_points.  m = mean_v - a;
 *     Sw = S_v w and Sm = S_v m with the stored row-major sqrt-information; den = Sw.Sw, no hit unless den > 0;
 *     tau* = (Sw.Sm) / den; tau_c = min(max(tau*, tau_in), tau_out); r = S_v (tau_c w - m), m2 = r.r.  Hit iff
 *     m2 <= max_mahalanobis_sq and tau_c max_range >= min_range; a NaN is no hit.  Inside this block the compiler may
 *     fuse and reorder: m2 and the range are defined to rounding error, not to the bit.
 *   Result.  The first hit in walk order ends the walk: voxel_out[i] = v, range_out[i] = tau_c max_range.  No hit: -1
 *     and 0.0.  A ray's result depends on that ray, the pose and the store alone, so it does not depend on the order of
 *     the points, on the other points, nor on how often the call is made.
 * voxel_out, range_out (optional): host arrays of nos_scan_size(rays) entries, indexed like the scan's STORED positions
 * (nos_scan_order maps them to input indices).  *n_hit, *n_skipped (optional): rays that hit, rays skipped.
 * *out_scan (optional): a new scan of the hits only, compacted in stored order; a hit point is
 * origin + (range / len)(p - origin) per component (quotient, difference, product, sum: each rounded once), in the rays'
 * frame, and the new scan's order is the original index of each hit's ray, composed with the order of `rays` as
 * nos_scan_filter composes it.  Free it with nos_scan_destroy.
 * An empty scan or an empty store is a no-op: every entry -1 and 0.0, both counts 0, an empty *out_scan.
 * Rejected, every output unwritten, before any device work:
 *   NOS_ERR_INVALID_ARGUMENT  map, rays, R, t or what NULL; struct_size < sizeof(nos_voxel_raycast); a non-finite entry of
 *                             R, t or origin; max_range not finite or not above 0; min_range or max_mahalanobis_sq
 *                             negative or not finite; a scan of another context;
 *   NOS_ERR_UNSUPPORTED       a multi-device context; 3 (ceil(max_range / voxel_resolution) + 1) > NOS_CARVE_MAX_CELLS;
 *                             a scan of 2^32 - 1 points or more;
 *   NOS_ERR_HIP               a store left undefined by an earlier failure.
 * Work: one table probe per visited cell, twelve doubles read per visited valid voxel; one host wait, two when
 * *out_scan is asked for and a ray hit. */
typedef struct nos_voxel_raycast {
  size_t struct_size;        /* sizeof(nos_voxel_raycast), for later growth */
  double origin[3];          /* sensor origin in the RAYS' frame (usually 0, 0, 0) */
  double min_range;          /* a hit nearer than this is passed over, >= 0 */
  double max_range;          /* every beam is walked up to this length; finite, > 0 */
  double max_mahalanobis_sq; /* finite, >= 0 */
  uint32_t min_points;       /* a voxel with fewer points is passed through */
} nos_voxel_raycast;
int nos_voxel_map_raycast(nos_voxel_map* map, nos_scan* rays, const double R[9], const double t[3],
                          const nos_voxel_raycast* what, int32_t* voxel_out, double* range_out,
                          nos_scan** out_scan, size_t* n_hit, size_t* n_skipped);
/* Any output pointer may be NULL.  capacity: slots the arrays have room for; bytes: device memory the store holds;
 * epoch: see NOS_PRUNE_AGE; generation: times the store's device block was replaced (growth, a prune that removed
 * something). */
int nos_voxel_map_memory(const nos_voxel_map* map, size_t* capacity, size_t* bytes,
                         unsigned long long* epoch, unsigned long long* generation);
/* Merge one voxel store into another under a pose: every voxel of `src` (its count and nine sums, nothing else) is moved by
 * p' = R p + t into the grid of `dst` and added to the voxel it lands in — submaps composed at corrected poses, two
 * sessions joined, a coarser level of a map pyramid — at a cost that follows the VOXELS of src, not its points.
 *   With n = count, s and M the sums about the corner o of the source cell, mu = o + s / n:
 *   destination cell c' = floor((R mu + t)_k * inv_res) per axis, inv_res = 1.0 / dst's resolution and the multiply-adds
 *   of nos_voxel_map_insert_scan's warp: the cell an insert_scan would put a point at the source voxel's mean into.  The
 *   WHOLE voxel goes there (a voxel is never split); means that lie in their cell stay there under the convex
 *   combinations a merge forms, which is what nos_voxel_map_match (see its caveat) relies on.
 *   With o' the corner of c' and b = (R o + t) - o' (formed once):  s' = R s + n b,
 *   M' = R M R^T + (R s) b^T + b (R s)^T + n b b^T;  source voxels that land in one cell are added in ascending source
 *   voxel id, then count += n', sums += (s', M') and the usual per-voxel finish, as an insert does.
 * Exact (bit for bit an insert of the transformed points) when every product and sum above is exact: an axis rotation, a
 * translation by whole cells, power-of-two resolutions and points on a binary lattice.  Otherwise mean and covariance
 * differ from an insert of the transformed points by rounding, and a voxel whose points straddle destination cells goes
 * to the cell of its mean where an insert would have split it.  Voxels below min_points contribute like any other.
 * src is read-only: its voxels, epoch, generation and stamps stay as they were.  src and dst may differ in resolution,
 * search radius and flags.  Voxel ids follow the rule of an insert: a merge is ONE batch, new voxels are appended in
 * ascending destination cell; dst's epoch advances by one and the touched voxels are stamped with it; n_points grows by
 * src's.  R is not checked for orthonormality.  An empty src is a no-op that leaves the epoch alone.
 * *n_touched (optional) = destination voxels touched.  Rejected before anything runs or is written, *n_touched included:
 *   NOS_ERR_INVALID_ARGUMENT  dst, src, R or t NULL, dst == src, different contexts, a non-finite entry of R or t (or
 *                             finite entries so large that a source voxel's moments overflow);
 *   NOS_ERR_HIP               either store was left undefined by an earlier failure;
 *   NOS_ERR_UNSUPPORTED       a destination cell outside +-2^20 per axis, or source voxels that would take the voxel of
 *                             dst they land in past 2^32 - 1 points — together with what that voxel already holds (the
 *                             count limit above) or among themselves: the message names a source voxel id, dst is bit for
 *                             bit as before (the limit against dst's own count is found after room was reserved: dst's
 *                             capacity, bytes and generation may have grown). */
int nos_voxel_map_merge(nos_voxel_map* dst, const nos_voxel_map* src, const double R[9], const double t[3], size_t* n_touched);
/* One store matched against another: distribution-to-distribution NDT (Stoyanov et al. 2012).  Every valid
 * voxel of `source` is warped by q = R mean_s + t (the matcher's warp) and matched to its (up to) max_neighbors nearest
 * valid voxel means of `target` — the search of nos_voxel_map_match for the point mean_s: same radius test, guard band
 * with its caveat, tie-break by slot and limit of 9 cells per axis, all of them the TARGET's.  Each match becomes one
 * ordinary flat NDT correspondence: p = mean_s (source frame), mu = mean_j, and a sqrt-information S with
 *   S^T S = A = (Sigma_j + R Sigma_s R^T)^-1,   Sigma_x = (S_x^T S_x)^-1 of the store's sqrt_information S_x
 * (so the eigenvalue floor of the voxel finish is in it, and NOS_MAP_PROPER_SQRT_INFORMATION does not matter).  A is
 * evaluated at the pose of the call and is a constant of the dataset: a solve holds it fixed as it holds the
 * correspondences fixed; the next match re-evaluates both.  S is the inverse of the Cholesky factor of the combined
 * covariance (lower triangular).  R is not checked for orthonormality.
 * The dataset has 2 * n_voxels(source) slots: source voxel v owns slots 2v (nearest) and 2v + 1 (second nearest).  All-zero
 * records, not counted in *n_matches: an invalid source voxel, a missing neighbour, slot 2v + 1 when max_neighbors = 1, a
 * pair whose combined covariance is not finite or not positive definite.  Every accumulate and solve entry point takes it.
 * Both stores are read only (target == source is allowed) and may differ in resolution, radius and flags; one kernel plus
 * the dataset's padding, one wait; the work follows the source's voxels.  An empty source gives an empty dataset.
 * Rejected before anything runs, *out_ds unwritten: NOS_ERR_INVALID_ARGUMENT for a NULL argument (n_matches may be NULL),
 * stores of different contexts, an unknown dtype; NOS_ERR_UNSUPPORTED for max_neighbors outside 1-2, a multi-device
 * context, a search ball of the target that spans more than 9 cells per axis; NOS_ERR_HIP for a store (either) an earlier
 * failure left undefined. */
int nos_voxel_map_match_map(nos_voxel_map* target, nos_voxel_map* source, const double R[9], const double t[3],
                            int max_neighbors, int dtype, nos_dataset** out_ds, size_t* n_matches);
/* ---- a store's state: export, restore, page voxels out and in ----
 * A voxel IS its cell, its count, its nine sums about the cell corner and its stamp; mean, sqrt-information and validity
 * are a pure function of (sums, count, cell, flags, resolution) — the one per-voxel finish every kernel shares.  So the
 * state below is all that has to leave the device for a store to outlive its process, or for a voxel a prune removes to
 * come back later, and both contracts are bit for bit: no tolerance anywhere.
 *
 * nos_voxel_map_export: a host-side copy of the store's voxels (all of them, or one half of the partition a prune would
 * make), a nos_voxel_state, handled like a nos_map_stats: read with nos_voxel_state_size / _info / _get, free with
 * nos_voxel_state_destroy; it is independent of the store afterwards.
 *   select == NULL: every voxel (side is still checked).  Otherwise `select` is read exactly as nos_voxel_map_prune reads
 *   it — the same host-computed box bounds, the same age test against the store's epoch, the same validation and
 *   statuses — and side picks the half: NOS_STATE_KEPT the voxels that prune would keep, NOS_STATE_REMOVED the ones it
 *   would remove.  The two halves are disjoint and together are the store.
 *   The selected voxels come out in voxel-id order; KEPT is, entry for entry, what an export of everything gives after
 *   that prune.  An empty selection (or an empty store) gives a state of size 0.
 *   The store is not modified: nos_voxel_map_memory, the voxels, epoch, generation and the stamps stay as they were.
 *   Work: with select == NULL four copies of n_voxels entries and one host wait, nothing launched; with a selection a
 *   prune's keep flags and scan, one gather kernel into arena memory, the copies, and two host waits (how many, then the
 *   data); nothing is allocated or launched in proportion to anything but n_voxels.
 *   Rejected before anything runs, *out_state unwritten: NOS_ERR_INVALID_ARGUMENT for map or out_state NULL, a side
 *   outside 0-1 and everything nos_voxel_map_prune rejects in `select`; NOS_ERR_UNSUPPORTED for a multi-device context;
 *   NOS_ERR_HIP for a store an earlier failure left undefined.
 * nos_voxel_state_info (any pointer may be NULL): resolution, search radius, flags and epoch of the store at the export;
 *   n_points = the points of the voxels in the state.
 * nos_voxel_state_get (any pointer may be NULL): cells [n][3], counts [n], sums [n][9] = sx sy sz | mxx mxy mxz myy myz mzz
 *   about the corner cell * voxel_resolution (the store's own numbers, not re-derived), stamps [n] (low 32 bits of the
 *   epoch of the last insert that touched the voxel). */
typedef struct nos_voxel_state nos_voxel_state;
#define NOS_STATE_KEPT    0   /* the voxels a prune with `select` would keep   */
#define NOS_STATE_REMOVED 1   /* the voxels it would remove                    */
int nos_voxel_map_export(nos_voxel_map* map, const nos_voxel_prune* select /* NULL: every voxel */, int side,
                         nos_voxel_state** out_state);
size_t nos_voxel_state_size(const nos_voxel_state* state);
int nos_voxel_state_info(const nos_voxel_state* state, double* voxel_resolution, double* search_radius_sq, int* flags,
                         unsigned long long* epoch, unsigned long long* n_points);
int nos_voxel_state_get(const nos_voxel_state* state, int64_t* cells_xyz, uint32_t* counts, double* sums, uint32_t* stamps);
int nos_voxel_state_destroy(nos_voxel_state* state);
/* nos_voxel_map_import: n voxels given as cells [n][3], counts [n], sums [n][9] (about the corner of their cell, at
 * voxel_resolution) and, for a restore, stamps [n] go into the store.  Counts and sums are taken as given, with no
 * arithmetic on them; moments that belong to no point set get whatever the per-voxel finish makes of them, never a fault.
 *   NOS_IMPORT_RESTORE, into a store that holds no voxel: voxel i of the arrays becomes voxel id i with the count and the
 *   nine sums as given and stamp stamps[i] (stamps == NULL: uint32(epoch) for every voxel); the store's epoch becomes
 *   `epoch`; mean, sqrt-information and validity are the per-voxel finish with the STORE's flags and resolution; the key ->
 *   slot table, n_valid and n_points follow.  The capacity doubles from the store's current one until n fits.
 *   Consequence: a store restored from nos_voxel_map_export(map, NULL, ...) of a store with the same resolution and flags
 *   cannot be told from it by any entry point — nos_voxel_map_stats bit for bit, the ids, the epoch, and the results of
 *   every later call (inserts, age prunes, carves, merges, matches, scores) — except by capacity and generation
 *   (nos_voxel_map_memory), on which results never depend.  n == 0 only sets the epoch.
 *   NOS_IMPORT_ADD, into any store: the state is ONE batch, exactly as the runs of an insert are.  A cell the store holds
 *   gets count += n and sums = sums + s (the store's first, as a merge adds); cells it does not hold are appended in
 *   ascending cell order; the epoch advances by one and every touched voxel is stamped with it; n_points grows by the
 *   state's.  stamps and epoch are ignored.  n == 0 is a no-op that leaves the epoch alone.
 *   Consequence: a voxel that was exported and removed comes back, when its cell is absent, with the same count and sums
 *   and therefore the same mean, sqrt-information and validity, bit for bit (its id and stamp are new).
 * *n_touched (optional) = n.  Rejected with the store and *n_touched unwritten; the checks that need no device come
 * first, and a repeated cell is found on the device before anything of the store is written:
 *   NOS_ERR_INVALID_ARGUMENT  map NULL; an unknown mode; cells_xyz, counts or sums NULL with n > 0; voxel_resolution not
 *                             equal, bit for bit, to the store's (the sums are about the corner cell * resolution); a
 *                             count of 0; a non-finite sum; the same cell twice (the message names one such cell);
 *                             NOS_IMPORT_RESTORE into a store that holds a voxel;
 *   NOS_ERR_UNSUPPORTED       a multi-device context; more than 2^30 voxels; a cell outside +-2^20 per axis;
 *                             NOS_IMPORT_ADD that would take a voxel past 2^32 - 1 points (the message names the voxel of
 *                             the state);
 *   NOS_ERR_HIP               a store an earlier failure left undefined.
 * A restore fills a fresh device block and adopts it only when nothing failed: a failure half-way leaves the store
 * exactly as it was.  Work: the copies of the arrays and one kernel with one lane per voxel (restore, one host wait); a
 * sort of the n keys, one kernel with one lane per voxel and the back half of an insert (add, two host waits). */
#define NOS_IMPORT_RESTORE 0
#define NOS_IMPORT_ADD     1
int nos_voxel_map_import(nos_voxel_map* map, int mode, double voxel_resolution, size_t n, const int64_t* cells_xyz,
                         const uint32_t* counts, const double* sums, const uint32_t* stamps /* may be NULL */,
                         unsigned long long epoch, size_t* n_touched);
int nos_voxel_map_destroy(nos_voxel_map* map);

/* ---- the hot path -------------------------------------------------------------
 * nos_ndt6_accumulate replaces
 *   MahalanobisDistanceMinimizerAnalyticSIMD::ComputeCostAndDerivatives
 *     (MDM/..._analytic_simd.cc:113-177) and its scalar twin
 *   MahalanobisDistanceMinimizerAnalytic::ComputeCostAndDerivatives
 *     (MDM/..._analytic.cc:12-52, 159-218)
 * plus the thread fan-out / partial sum around them (MDM/..._analytic_simd.cc:55-76).
 * Blocking; out28 is host memory. */
int nos_ndt6_accumulate(nos_dataset* ds, const double R[9], const double t[3],
                        const nos_loss* loss, double out28[NOS_NDT6_OUT]);
/* nos_ndt3_accumulate replaces the planar (x, y, yaw) loops
 *   MDM/..._analytic_3dof.cc:36-69,110-139 and MDM/..._analytic_3dof_simd.cc:85-158.
 * R2 is the row-major 2×2 rotation, t2 the planar translation. */
int nos_ndt3_accumulate(nos_dataset* ds, const double R2[4], const double t2[2],
                        const nos_loss* loss, double out10[NOS_NDT3_OUT]);
/* nos_reproj_accumulate replaces REM/..._analytic.cc:31-64,107-162 and the SIMD loop
 * REM/..._analytic_simd.cc:55-138.  intr = {inv_fx, inv_fy, cx, cy}; points whose
 * transformed depth is < min_depth contribute nothing (scalar class: 0.03,
 * REM/..._analytic.cc:111,119-123). */
int nos_reproj_accumulate(nos_dataset* ds, const double R[9], const double t[3],
                          const double intr[4], const nos_loss* loss, double min_depth,
                          double out28[NOS_REPROJ_OUT]);

/* Asynchronous forms for one-process-per-GPU use: enqueue kernel + final reduce on
 * the context's stream (single-device contexts only) and leave the 28 / 10 doubles
 * in DEVICE memory at d_out, e.g. a torch tensor that the caller then hands to
 * ncclAllReduce / torch.distributed.all_reduce on the same stream.  This is the
 * reference's "sum the per-thread partials" step (MDM/..._analytic_simd.cc:70-75)
 * moved onto RCCL.  No host synchronisation happens inside. */
int nos_ndt6_accumulate_async(nos_dataset* ds, const double R[9], const double t[3],
                              const nos_loss* loss, double* d_out28);
int nos_ndt3_accumulate_async(nos_dataset* ds, const double R2[4], const double t2[2],
                              const nos_loss* loss, double* d_out10);
int nos_reproj_accumulate_async(nos_dataset* ds, const double R[9], const double t[3],
                                const double intr[4], const nos_loss* loss, double min_depth,
                                double* d_out28);

/* ---- the whole Levenberg-Marquardt loop, device resident ---------------------------------
 * nos_ndt6_solve / nos_ndt3_solve / nos_reproj_solve replace the body of the reference's Solve():
 *   MDM/..._analytic_simd.cc:30-108 (= ..._analytic.cc:57-157), MDM/..._analytic_3dof.cc:17-108,
 *   REM/reprojection_error_minimizer_analytic.cc:15-105
 * i.e. per iteration: ComputeCostAndDerivatives, H_kk *= 1 + lambda, ldlt().solve(-g), right-multiplicative
 * pose update, the two convergence tests after the update, lambda *= 2 / 0.6 clamped to [1e-6, 1e-2].
 * The loop state stays in device memory: the workgroup that completes the sums of a launch runs that
 * loop body and leaves the new pose for the next launch, so consecutive iterations run back-to-back on
 * the GPU with no host step in between (the host keeps `launches_in_flight` launches queued and reads
 * one pinned log entry per iteration).  Semantics are those of the host loop around nos_*_accumulate
 * (same source for the loop body); only floating-point contraction may differ in the last bits.
 * Small and mid-size problems run the whole loop in ONE launch: below 1 024 NDT / 3 072 reprojection
 * correspondences inside a single workgroup; up to 131 072 correspondences with one 512-correspondence chunk per
 * workgroup held in registers and a bounded epoch hand-off between iterations (if the grid cannot become resident
 * in time the launch gives up and the solve is redone with one launch per iteration) — report->launches tells
 * which form ran.
 * With a communicator (nos_ctx_comm_init) each launch is followed by the all-reduce and a one-wave step
 * kernel; every rank ends with identical bits.  Single-device contexts only (NOS_ERR_UNSUPPORTED
 * otherwise: use the host loop).  R / t are in-out. */
typedef struct nos_lm_options {
  int32_t max_iterations;      /* Options::max_iterations (options.h) */
  int32_t launches_in_flight;  /* 0 = default (3) */
  double gradient_tolerance;   /* Options::convergence_handle.gradient_tolerance */
  double parameter_tolerance;  /* Options::convergence_handle.parameter_tolerance */
  double* cost_history;        /* NULL, or room for max_iterations costs (one per executed iteration) */
} nos_lm_options;

typedef struct nos_lm_report {
  int32_t iterations;   /* loop index at exit: the "iter:" of the reference's stderr line */
  int32_t ok;           /* 0 if the damped solve met a non-positive pivot */
  int32_t launches;     /* kernels enqueued (>= iterations executed; the surplus exits at once) */
  int32_t fallback;     /* 1: the one-launch form of the loop gave up (GPU shared with another process, or the LDS it needs
                           refused) and the solve was re-run with one launch per iteration — same result, slower */
  double printed_cost;  /* previous_cost at exit: the "COST:" of that line */
  double last_cost;
  double final_lambda;
} nos_lm_report;

int nos_ndt6_solve(nos_dataset* ds, double R[9], double t[3], const nos_loss* loss,
                   const nos_lm_options* options, nos_lm_report* report);
int nos_ndt3_solve(nos_dataset* ds, double R2[4], double t2[2], const nos_loss* loss,
                   const nos_lm_options* options, nos_lm_report* report);
int nos_reproj_solve(nos_dataset* ds, double R[9], double t[3], const double intr[4],
                     const nos_loss* loss, double min_depth, const nos_lm_options* options,
                     nos_lm_report* report);

/* ---- many small pose problems in one launch ------------------------------------------
 * n_problems independent solves, one pose each: problem i ends with exactly what nos_*_solve(ds[i], R + 9i, t + 3i, ...)
 * would give it (planar: R2 + 4i, t2 + 2i) — pose, report and cost history.  Flat datasets of n x planes ≤ the context
 * option "batch_max_elements" (NOS_BATCH_MAX_ELEMENTS; default 15 360, the single-workgroup size of nos_*_solve: 1 024
 * NDT / 3 072 reprojection correspondences) run in ONE launch, one workgroup per problem (reports[i].launches = 1); the
 * others — voxel-indexed datasets and larger problems — run one after the other through nos_*_solve after it.  A raised
 * budget lets one workgroup loop over a larger problem: more problems per second when there are hundreds of them, more
 * latency per problem.  The same dataset may appear several times (multi-start: datasets are only read).
 * options->cost_history is NULL or has room for n_problems x max_iterations: row i starts at i * max_iterations and only
 * its executed entries are written.  reprojection: intr [n][4], one set per problem.  One loss for all problems.
 * n_problems == 0 returns NOS_OK.  Checked before anything runs (a rejected call writes nothing): NULL arrays,
 * n_problems < 0, datasets of different contexts or element types (NOS_ERR_INVALID_ARGUMENT), a dataset of the wrong kind
 * (NOS_ERR_WRONG_KIND), a multi-device context or one with a communicator (NOS_ERR_UNSUPPORTED: batches are process
 * local). */
int nos_ndt6_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R, double* t, const nos_loss* loss,
                         const nos_lm_options* options, nos_lm_report* reports);
int nos_ndt3_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R2, double* t2, const nos_loss* loss,
                         const nos_lm_options* options, nos_lm_report* reports);
int nos_reproj_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R, double* t, const double* intr,
                           const nos_loss* loss, double min_depth, const nos_lm_options* options,
                           nos_lm_report* reports);

/* ---- many scan-to-map registrations in one launch ------------------------------------
 * The outer loop of the reference's test drivers (OptimizePoseAnalytic, MDM/tests/simple_optimization_test.cc:474-503):
 * up to max_outer_iterations rounds of {MatchPointCloud at the current pose (:296-342, here nos_ndt_match), the solver
 * class's tail drop (nos_dataset_drop_last_matches), Solve()}, stopping once the pose moved by less than 1e-5 in
 * translation and in the quaternion vector part — for n_problems scans against ONE map, in ONE launch with one workgroup
 * per problem: matching, tail drop, the LM loop of the single-workgroup nos_*_solve and the stopping test all run on the
 * device, every round.  Problem i ends with what the Python loop pipeline.scan_to_map gives scans[i] from (R + 9i, t + 3i):
 * pose, outer_iter and per round matches / used / iterations / printed cost — bit for bit for scans of ≤ 512 points (their
 * 2n ≤ 1 024 slots are what nos_*_solve runs in one workgroup), to rounding above (the lone solve then sums in another
 * order, in its multi-workgroup form).
 * Every problem runs inside the launch, whatever its size: a large scan is slower here than through scan_to_map, one CU
 * doing what the lone one-launch solve spreads over the chip (DESIGN.md §12 has the measured crossover); a caller with one
 * large scan keeps using the lone path.  The context option batch_max_elements is not consulted.
 * nos_ndt3_register_batch: R [n][9], t [n][3] stay full 3-D poses; every round solves for the top-left 2x2 and (x, y) and
 * writes only those back (MahalanobisDistanceMinimizerHip3DOF), z, roll and pitch pass through.
 * The same scan may appear several times (multi-start); scans and map are only read.  Per-problem scratch datasets,
 * descriptors and results come from the context's buffer pool: one upload, one launch, one copy back, one synchronisation.
 * A round whose solve fails (ok = 0, e.g. no match at all) ends that problem: its pose stays at the value before that
 * round, reports[i].ok = 0 and outer_iter = that round (scan_to_map raises there); the other problems are unaffected.
 * Checked before anything runs (a rejected call writes nothing): NULL arrays, n_problems < 0, scans or map of another
 * context, max_outer_iterations < 1, keep_multiple < 0, an unknown dtype or loss, max_iterations < 0, or
 * options->cost_history != NULL (NOS_ERR_INVALID_ARGUMENT); max_neighbors outside 1-2, a multi-device context or one with a
 * communicator (NOS_ERR_UNSUPPORTED).  n_problems == 0 returns NOS_OK.
 * Not covered: voxel-indexed matching, the simd_class semantics, one map per problem, multi-device batches. */
typedef struct nos_register_round {
  uint64_t matches;     /* real matches of the round (nos_ndt_match's n_matches) */
  uint64_t used;        /* matches the solve summed: matches - matches % keep_multiple */
  int32_t iterations;   /* the round's "iter:" */
  int32_t ok;           /* 0: the round's solve failed */
  double printed_cost;  /* the round's "COST:" */
  double last_cost;
} nos_register_round;

typedef struct nos_register_options {
  int32_t max_outer_iterations;  /* rounds at most (10 in OptimizePoseAnalytic) */
  int32_t max_neighbors;         /* 1 or 2 (the reference: 2) */
  int32_t keep_multiple;         /* 0 = no tail drop; k > 0: each round sums the first floor(N/k)*k of its N matches
                                    (4: the scalar 3-DoF class and the captured 6-DoF runs; 8: the SIMD classes) */
  int32_t dtype;                 /* NOS_F64 / NOS_F32: element type of the matched records */
  nos_register_round* round_log; /* NULL, or n_problems x max_outer_iterations entries: row i starts at
                                    i * max_outer_iterations, its first reports[i].rounds entries are written, the rest
                                    zeroed */
} nos_register_options;

typedef struct nos_register_report {
  int32_t outer_iter;  /* index of the round that met the stopping test, max_outer_iterations if none did (the reference's
                          printed loop variable), or the round whose solve failed */
  int32_t rounds;      /* rounds run */
  int32_t ok;          /* 0: a round's solve failed */
  int32_t pad;
} nos_register_report;

int nos_ndt6_register_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                            const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                            nos_register_report* reports);
int nos_ndt3_register_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                            const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                            nos_register_report* reports);

/* ---- the same, against the LIVE voxel store ---------------------------
 * nos_ndt6_register_batch / nos_ndt3_register_batch with a nos_voxel_map in place of the nos_ndt_map: every round of every
 * problem is matched against the store as it is now, through the key -> slot table the inserts maintain (the matcher of
 * nos_voxel_map_match), inside the one launch.  Arguments, reports, round log, the failure of a single problem and the
 * "a rejected call writes nothing" rule are those of nos_ndt*_register_batch.
 * Contract: problem i ends, bit for bit and at any scan size, with what nos_voxel_map_snapshot followed by
 * nos_ndt*_register_batch gives it — pose, outer_iter, and per round matches / used / iterations / ok / printed and last
 * cost — subject to the guard-band caveat of nos_voxel_map_match (a voxel is looked for in its own cell, widened by
 * resolution / 1024).  It therefore also ends with what pipeline.scan_to_map on the store gives: bit for bit for scans of
 * ≤ 512 points, to rounding above.
 * The call is one upload, one launch, one copy back and one synchronisation; nothing is sorted and nothing is allocated in
 * proportion to the map.  The store is only read: voxels, epoch, generation and stamps stay as they were (the one word of
 * it the call writes is its internal probe-error flag, cleared before the launch and brought back with the results).
 * An empty store is not an error: every problem fails alone in round 0 (ok = 0, its pose kept).
 * Rejected before anything runs: everything nos_ndt*_register_batch rejects, with the same status (a scan of another
 * context than the store's: NOS_ERR_INVALID_ARGUMENT, as there and as in nos_voxel_map_match); a search ball that spans
 * more than 9 cells per axis, 2 r / resolution + 2 > 9 (NOS_ERR_UNSUPPORTED, as nos_voxel_map_match); a store an earlier
 * failure left undefined (NOS_ERR_HIP).  A table probe that runs through the whole table (it cannot at the store's load
 * factor) makes the call return NOS_ERR_HIP with R, t, reports and round_log unwritten.
 * Not covered: what nos_ndt*_register_batch does not cover. */
int nos_voxel_map_register6_batch(nos_voxel_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                                  nos_register_report* reports);
int nos_voxel_map_register3_batch(nos_voxel_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                                  nos_register_report* reports);

/* ---- how well a scan fits the map at a pose: many poses scored in one call -------------
 * nos_ndt_score_batch: n_problems (scan, pose) pairs against one map, three numbers each, nothing written in between.
 * They are taken over the correspondences nos_ndt_match (nos_voxel_map_match for the store) produces for
 * (scans[b], R[b], t[b], max_neighbors) with dtype = NOS_F64:
 *   matches         that call's *n_matches;
 *   matched_points  the scan points with at least one match (a non-empty slot 2i);
 *   cost            Σ ρ over those correspondences — every term is, bit for bit, the value nos_ndt6_accumulate adds to
 *                   out[27] for the record the matcher writes (the same search, the same U, the item's own arithmetic);
 *                   only the order of the sum differs from that route.
 * The sum is deterministic and its shape follows the scan's point count alone (chunks of 1 024 points, one workgroup
 * each, the chunks of a problem added in ascending order): a row is the same bits from run to run, whatever
 * n_problems is, wherever the row stands in the batch and whatever the other rows are; and for the same arguments the
 * rows of nos_voxel_map_score_batch and of nos_ndt_score_batch on that store's nos_voxel_map_snapshot are equal bit
 * for bit (subject to the guard-band caveat of nos_voxel_map_match).
 * The same scan may appear several times (one scan, many poses); scans and map are only read — of the store, only its
 * internal probe-error flag is written, as in nos_voxel_map_register6_batch.  Descriptors, chunk partials and rows
 * come from the context's buffer pool: one upload, the launches, one copy back, one synchronisation; nothing is
 * allocated or iterated in proportion to the map.  loss: NULL = none; one loss for the whole call.
 * Rejected before anything runs, scores unwritten: NULL arrays with n_problems > 0, n_problems < 0, a scan of another
 * context than the map's, an unknown loss kind (NOS_ERR_INVALID_ARGUMENT); max_neighbors outside 1-2, a multi-device
 * context, and for the store a search ball that spans more than 9 cells per axis (NOS_ERR_UNSUPPORTED); a store an
 * earlier failure left undefined (NOS_ERR_HIP).  n_problems == 0 returns NOS_OK; an empty scan gives a zero row, an
 * empty map or store zero rows.  A table probe that runs through the whole table (it cannot at the store's load
 * factor) makes the call return NOS_ERR_HIP with scores unwritten.
 * Not covered: fp32 scoring, the planar cost, H and g per pose, one map per problem, multi-device contexts. */
typedef struct nos_pose_score {
  uint64_t matches;
  uint64_t matched_points;
  double cost;
  double reserved;   /* 0 */
} nos_pose_score;

int nos_ndt_score_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, const double* R /*[n][9]*/,
                        const double* t /*[n][3]*/, const nos_loss* loss, int max_neighbors, nos_pose_score* scores);
int nos_voxel_map_score_batch(nos_voxel_map* map, nos_scan* const* scans, int32_t n_problems, const double* R /*[n][9]*/,
                              const double* t /*[n][3]*/, const nos_loss* loss, int max_neighbors, nos_pose_score* scores);

/* Test hook: ONE step of the device-resident loop on given sums and a given loop state — the stand-alone step kernel
 * (the same single-lane function every device loop form calls).  dof 6: sums[28], dof 3: sums[10].
 * state[22] = R (9, row-major; planar: R[0..3] = the 2x2 rotation) | t (3) | q w x y z (4) | lambda | previous_cost | cost |
 * iteration | done | ok; settings[4] = max_iterations | gradient_tolerance | parameter_tolerance | float_schedule.
 * state is updated in place.  The host's own step for the same arguments: nos_host_lm_advance in libnos_host.so. */
int nos_debug_lm_step(nos_ctx* ctx, int dof, const double* sums, const double settings[4], double state[22]);

/* Test hook: the per-voxel finish of the map build and the voxel store — mean, covariance, eigen-decomposition, validity,
 * flooring, sqrt-information — computed ON THE HOST by the function the kernels call (no GPU call, no context).
 * sums[9] = sx sy sz | mxx mxy mxz myy myz mzz of d = p - cell * voxel_resolution over the voxel's `count` points;
 * params[3] = min_points | min largest eigenvalue | eigenvalue floor ratio (5, 0.01, 0.01 in the build);
 * flags: 0 or NOS_MAP_PROPER_SQRT_INFORMATION.  An invalid voxel: sqrt_information identity, *valid = 0 (and mean 0 below min_points).
 * count is used as the unsigned 32-bit number it is, up to 2^32 - 1.  Against 50 digits at 2^32 - 1 points (exact lattice
 * sums, cells 0 and +-(2^20 - 1)): validity equal, mean 0 ulp, floored eigenvalues 1.1e-15, information
 * matrix 1.5e-13 relative. */
int nos_debug_voxel_finish(uint32_t count, const double sums[9], const int64_t cell[3], double voxel_resolution,
                           const double params[3], int flags, double mean[3], double sqrt_information[9], unsigned char* valid);

/* Test hook: the moment transform of nos_voxel_map_merge computed ON THE HOST by the function its kernel calls (no GPU
 * call, no context).  count >= 1 and sums[9] about the corner of `cell` in a grid of edge src_resolution (as
 * nos_debug_voxel_finish takes them) -> cell_out, the destination cell in a grid of edge dst_resolution, and sums_out[9]
 * about that cell's corner.  NOS_ERR_UNSUPPORTED when the destination cell is not representable in 64 bits.
 * Against 50 digits at 2^32 - 1 points: bit for bit under the identity and a whole-cell translation; under
 * a general pose the mean the finish forms is off by 0.47 ulp at most and the scatter by 0.0006 x 128 x 2^-52 n L^2. */
int nos_debug_voxel_moments(uint32_t count, const double sums[9], const int64_t cell[3], double src_resolution,
                            const double R[9], const double t[3], double dst_resolution,
                            int64_t cell_out[3], double sums_out[9]);

/* Test hook: the combined information of nos_voxel_map_match_map computed ON THE HOST by the function its kernel calls (no
 * GPU call, no context).  S_target, S_source: row-major sqrt-informations; R row-major.  S_out: lower triangular with
 * S_out^T S_out = ((S_target^T S_target)^-1 + R (S_source^T S_source)^-1 R^T)^-1 and *ok = 1, or all zero and *ok = 0 when
 * an input is not finite or singular or the combined covariance is not finite or not positive definite (NOS_OK either way). */
int nos_debug_voxel_pair_information(const double S_target[9], const double S_source[9], const double R[9],
                                     double S_out[9], unsigned char* ok);

/* ---- pose-graph optimisation (BASELINE.json configs[4]) --------
 * The reference's PoseGraphOptimizerAnalytic::Solve is an empty loop
 * (NO/pose_graph_optimizer/pose_graph_optimizer_analytic.cc:12-51); only the Ceres path is real.
 * These entry points provide what its TODO comments ask for (:36-42 "Make sparse Hessian / Solve
 * normal equation / Update poses / Check convergence") for the residual Ceres minimises
 * (NO/pose_graph_optimizer/ceres_cost_functor.h:17-53, switchable :55-98):
 *   r_t = (p_q - p_r) - q_r (x) t_m,  r_R = 2 vec(q_q^* q_r q_m);  loop constraints: r <- s r and a
 *   seventh residual (1 - s) * 1e-9 with a free switch s.
 * poses [n][7] = px py pz qw qx qy qz (PoseParameter, pose_graph_optimizer.h:16-19);
 * meas [m][7] = relative_pose_from_reference_to_query, same packing (types.h:13-19);
 * switch_init / switch_free / fixed may be NULL.  One Gauss-Newton / LM iteration is
 *   nos_pgo_linearize → nos_pgo_solve (block-Jacobi PCG on the damped normal equations, matrix
 *   free) → nos_pgo_retract (p += dp, q = normalize(q (x) Exp(dw)), s += ds).
 * The normal matrix is never stored: every sweep re-derives the per-constraint Jacobian blocks
 * from the poses ("owner computes", no atomics, bit-reproducible).  Single-device contexts. */
typedef struct nos_pose_graph nos_pose_graph;
int nos_pgo_create(nos_ctx* ctx, size_t n_poses, const double* poses, size_t n_edges,
                   const int32_t* ref, const int32_t* qry, const double* meas,
                   const double* switch_init, const unsigned char* switch_free,
                   const unsigned char* fixed, nos_pose_graph** out_pg);
/* The same graph with a 6 x 6 information matrix per constraint.
 * THE RULE.  A constraint measures the pose of the query frame in the reference frame, (t_m, q_m).  Its information
 * Omega (6 x 6, symmetric, positive semi-definite) is over the error xi = (dt, dtheta) of that measurement, with
 *   t_true = t_m + dt  in the reference frame,   R_true = R_m Exp(dtheta).
 * These are the coordinates (t_x ... w_z) and the update (t += dt, R <- R Exp(dw)) of the 6-DoF NDT solvers: the 21
 * numbers H of nos_ndt6_accumulate / nos_voxel_map_match_map's sums at the pose the registration returns (target =
 * reference, source = query) are an Omega as they stand (tests/test_pgo_information_pipeline.py checks it).
 * Per constraint, with e = q_q^* q_r q_m, r_R = 2 vec(e), u = R_r^T (p_q - p_r):
 *   residual  r~ = (u - t_m, r_R).  dtheta = -r_R to first order, so the off-diagonal 3 x 3 blocks of Omega change
 *             sign: Omega' = D Omega D, D = diag(I, -I) (done once at upload);
 *   Jacobians under p += dp, q <- q Exp(dw):  reference end [-R_r^T | [u]x ; 0 | B],  query end [R_r^T | 0 ; 0 | C]
 *             (B = (e_w I + [e_v]x) R_m^T, C = -e_w I + [e_v]x).  The world-frame r_t of nos_pgo_create is NOT used:
 *             rotating Omega into the world frame at the current estimate drops a Jacobian term of the size of the residual;
 *   cost      s^2 r~^T Omega' r~ (+ (1 - s)^2 c^2);   gradient g_i += s^2 J~^T Omega' r~;   H_ii += s^2 J~^T Omega' J~;
 *   product   v = s (J~_i x_i + J~_j x_j) + r~ x_s,  out += s J~^T Omega' v;
 *   switches  row (Omega' r~) . s (J~_r x_r + J~_q x_q) + h_s (1 + lambda) x_s,  h_s = r~^T Omega' r~ + c^2,
 *             g_s = s r~^T Omega' r~ - c^2 (1 - s).
 * With Omega = I the cost is the same function of the poses as nos_pgo_create's, and cost and gradient agree with it to
 * rounding; the diagonal blocks do not (the Jacobians belong to another residual with the same norm).
 * information: [n_edges][21], upper triangle row-major; NULL = nos_pgo_create.  NOS_ERR_INVALID_ARGUMENT, with nothing
 * created, *out_pg untouched and before any device work, for a matrix with a non-finite entry, a zero matrix, or one whose
 * smallest eigenvalue is below -1e-12 x its largest; semi-definite matrices (a registration in a corridor) are accepted.
 * A direction that NO constraint observes (every information matrix around a pose has it in its null space) leaves a zero
 * pivot in that pose's diagonal block, which the damping lambda diag(H) does not lift.  Where the zeros are exact (identity
 * rotations) the solve never enters it; under general rotations the pivot is of rounding size, the block-Jacobi inverse
 * huge and the step along that direction meaningless: give such a pose a weak prior constraint instead.
 * A graph with information runs the owner-computes product (no block lists: nos_pgo_layout_info entries = 0) and the
 * probed coarse operator, whatever pgo_block / pgo_coarse_probe say.  Every other nos_pgo_* call works on it. */
int nos_pgo_create_weighted(nos_ctx* ctx, size_t n_poses, const double* poses, size_t n_edges,
                            const int32_t* ref, const int32_t* qry, const double* meas,
                            const double* switch_init, const unsigned char* switch_free,
                            const unsigned char* fixed, const double* information, nos_pose_graph** out_pg);
/* A robust loss on the constraints of a graph WITH information: the back end's defence against a wrong loop closure that
 * no switch was declared for.
 * THE RULE.  For constraint e, with r~, Omega', J~, s as above, q = r~^T Omega' r~, c the switch prior, rho the loss and
 * w = rho'(q):
 *   cost      s^2 rho(q) (+ (1 - s)^2 c^2);
 *   gradient  g_i += s^2 w J~^T Omega' r~;         diagonal blocks  H_ii += s^2 w J~^T Omega' J~;
 *   product   v = s (J~_i x_i + J~_j x_j) + r~ x_s,  out += s w J~^T Omega' v;
 *   switches  row w (Omega' r~) . s (J~_r x_r + J~_q x_q) + h_s (1 + lambda) x_s,
 *             g_s = s rho(q) - c^2 (1 - s),  h_s = rho(q) + c^2.
 * Iteratively reweighted Gauss-Newton without a second-order (Triggs) correction, as in the NDT solvers: rho and w are
 * evaluated once per nos_pgo_linearize and stay fixed through the products and solves that follow.  The 2 x 2 Schur
 * complement of a switch is rho + c^2 - w q (a projection <= 1); a concave rho with rho(0) = 0 has rho(q) >= q rho'(q),
 * so the matrix stays positive semi-definite and neither kind below needs a guard.
 *   NOS_LOSS_NONE                        rho = q,  w = 1;
 *   NOS_LOSS_HUBER (a = delta)           q <= delta^2: rho = q, w = 1;  else rho = 2 delta sqrt(q) - delta^2, w = delta / sqrt(q);
 *   NOS_LOSS_EXPONENTIAL (a = c1, b = c2)  rho = c1 - c1 exp(-c2 q),  w = c1 c2 exp(-c2 q).
 * THE WEIGHT IS THE DERIVATIVE OF THE COST THAT IS REPORTED.  For the exponential kind that is HALF the output[1] =
 * 2 c1 c2 exp(-c2 q) of the reference's loss_function.h:31, which the NDT entry points above follow for parity with the
 * reference's captured runs; the pose graph has no captured run to follow, and with the doubled weight the gradient is not
 * the gradient of the cost.  exp, sqrt and the division are the accurate library ones (one evaluation per constraint and
 * linearisation).
 * robust: [n_edges] flags of the constraints the loss applies to (usually the loop closures), NULL = all; a constraint
 * that is not flagged has rho = q, w = 1.  The flags are copied.
 * Callable at any time, any number of times; loss == NULL or kind NONE removes the loss.  It takes effect at the NEXT
 * nos_pgo_linearize: nos_pgo_matvec / nos_pgo_solve / nos_pgo_precondition before that keep the weights of the last
 * linearisation — an annealed schedule (large threshold first, then smaller) is a loop of set_loss, linearize, solve,
 * retract in the caller.  A graph with information and no loss computes the bits it computed before this call existed, and
 * so does one whose loss never leaves its quadratic zone (Huber with a huge delta).
 * NOS_ERR_INVALID_ARGUMENT, the graph's loss unchanged: an unknown kind; a Huber threshold that is not finite or <= 0;
 * exponential c1 or c2 not finite or < 0.  NOS_ERR_UNSUPPORTED: a loss (other than NONE) on a graph created without
 * information — create it with identity matrices. */
int nos_pgo_set_loss(nos_pose_graph* pg, const nos_loss* loss, const unsigned char* robust /*[n_edges] or NULL*/);
int nos_pgo_destroy(nos_pose_graph* pg);
size_t nos_pgo_num_unknowns(const nos_pose_graph* pg); /* 6 n_poses + n_edges */
int nos_pgo_linearize(nos_pose_graph* pg, double* cost, double* gradient_norm);
int nos_pgo_solve(nos_pose_graph* pg, double lambda, int max_iterations, double rel_tolerance,
                  int* iterations, double* rel_residual, double* step_norm);
int nos_pgo_retract(nos_pose_graph* pg);
int nos_pgo_get_state(nos_pose_graph* pg, double* poses, double* switches);
/* which: 0 gradient, 1 last step (both 6 planes of n_poses then n_edges switch entries),
 * 2 diagonal blocks (21 planes of n_poses, upper triangle row-major), 3 the weight w of every constraint at the last
 * nos_pgo_linearize (n_edges values: 1.0 where no loss applied, all ones on a graph without information or without a
 * loss) — how a caller sees which loop closures the loss has rejected.  Diagnostics. */
int nos_pgo_get_vector(nos_pose_graph* pg, int which, double* out);
/* y = (J^T J with its diagonal scaled by 1 + lambda) x for host vectors.  Diagnostics. */
int nos_pgo_matvec(nos_pose_graph* pg, double lambda, const double* x, double* y);
/* z = M^-1 r for a host vector (tests): the preconditioner nos_pgo_solve would use at this lambda (context options
 * pgo_precond, pgo_agg, pgo_coarse_probe honoured).  Vector order of nos_pgo_matvec; must follow nos_pgo_linearize.
 * Switch rows: r_s / (h_s (1 + lambda)) where a switch is free, r_s / (1 + lambda) otherwise.  Diagnostics. */
int nos_pgo_precondition(nos_pose_graph* pg, double lambda, const double* r, double* z);
/* What the sweeps have to touch (bench.py's byte models): info[0] poses, [1] constraints, [2] entries of the block-local
 * product (one per constraint and block it touches; 0 = the owner-computes product is in use), [3] poses per block,
 * [4] blocks, [5] halo poses over all blocks, [6] aggregates of the coarse level, [7] PCR levels (6, 7: 0 before the
 * first two-level solve). */
int nos_pgo_layout_info(const nos_pose_graph* pg, unsigned long long info[8]);
/* Timing aid (bench.py): `repeats` device-resident products of the kind a PCG iteration makes (x = the gradient of the
 * last nos_pgo_linearize), back to back on the context's stream between one pair of HIP events → milliseconds per
 * product.  which: 0 the product of a PCG iteration (with its in-launch p.Ap sum), 1 the linearisation sweeps. */
int nos_pgo_time_sweep(nos_pose_graph* pg, int which, double lambda, int repeats, double* ms_per_sweep);

/* ---- thread safety ----------------------------------------------------------------
 * Every entry point that takes a context, or an object created on one (dataset, map, scan, pose graph), holds that
 * context's lock for its whole duration: calls on ONE context are serialised, calls on different contexts run
 * concurrently.  The drop-in solver classes share one context per device list, so two threads that each own a solver
 * object are safe (their solves take turns) — the guarantee the reference's independent solver objects give.
 * nos_ctx_destroy must not race with any other call on that context.
 *
 * ---- experiment knobs ----------------------------------------------------------------
 * Read from the environment once, in nos_ctx_create (NOS_SC1, NOS_NT, NOS_FUSED, NOS_LM_FUSED, NOS_LM_WINDOW,
 * NOS_LM_SINGLE, NOS_LM_CLUSTER, NOS_POOL, NOS_TILE_LOG2, NOS_PLANE_SKEW, NOS_INGEST, NOS_INGEST_THREADS,
 * NOS_INDEXED_BPC, NOS_MATCH_DENSE, NOS_PGO_HOST_SCALARS, NOS_PGO_PRECOND, NOS_PGO_AGG, NOS_BATCH_MAX_ELEMENTS; option only: "map_fma_mask",
 * "map_eigen_version"); afterwards only through these setters (keys =
 * the names in lower case without the prefix, e.g. "lm_cluster"; "ingest": 0 auto, 1 pack, 2 unpack;
 * "debug_cluster_abort": test hook, makes the next one-launch solve give up and fall back).  Nothing on the solve /
 * accumulate path reads the environment.
 *   "debug_alloc_fill" / "debug_alloc_filled"  test hooks (option only).  debug_alloc_fill: 0 (default) off; -1 = every
 *                 device block handed out from now on — a buffer of the pool, parked or fresh, over its whole capacity;
 *                 every allocation made for an object or a call; the pinned staging blocks allocated on first use — is
 *                 filled with the word 0x00000000 first; 1 … 0x7FFFFFFF = with that 32-bit word.  The context's own
 *                 workspaces exist before the option can be set and are not filled.  No result may depend on the word.
 *                 debug_alloc_filled counts the blocks filled (saturating); setting it to 0 resets it, no other value is
 *                 accepted.
 *   "lm_cluster"  1 (default) the device-resident loop runs in ONE launch wherever it can: correspondences resident on chip
 *                 up to the register + LDS capacity, streamed from HBM every iteration beyond it; 4 = one launch only for
 *                 resident data (one launch per iteration above), 5 = as 1 with the all-reduce's first stage always through
 *                 sc1 stores, 3 = the arrival-counter all-reduce, 2 = at most one correspondence per lane, 0 = off.
 *   "tile_log2"   layout of datasets created afterwards: -1 (default) by element type — fp64 planar planes, fp32 tiles of
 *                 1024 correspondences; 0 planar; 10…24 tiles of 2^k.
 *   "stream_lds_chunks" / "stream_reg_rounds" (NOS_STREAM_LDS_CHUNKS, NOS_STREAM_REG_ROUNDS; 0…3, default 3)
 *                 streamed one-launch loop: chunks every workgroup keeps in LDS / in spare vector registers after the
 *                 first iteration instead of reading them from HBM again (the register count is clamped to what the kernel
 *                 has room for: none for fp32 6-DoF NDT, 3 otherwise).  The results do not depend on either, bit for bit. */
int nos_ctx_set_option(nos_ctx* ctx, const char* key, int value);
int nos_ctx_get_option(const nos_ctx* ctx, const char* key, int* value);

/* ---- measurement / diagnostics ------------------------------------------------- */
/* Launch geometry override (0 = library default): blocks per CU of the assemble grid and
 * the index of the compiled kernel geometry.  Tuning knob, not needed for normal use. */
int nos_ctx_set_launch(nos_ctx* ctx, int blocks_per_cu, int variant);
/* Time `repeats` back-to-back assemble launches of shard 0 with HIP events recorded on
 * the stream the kernels are launched on; returns the mean per-launch duration of the
 * assemble kernel alone (kernel_ms) and of assemble + final reduce (total_ms). */
int nos_ndt6_time_kernel(nos_dataset* ds, const double R[9], const double t[3],
                         const nos_loss* loss, int repeats, double* kernel_ms,
                         double* total_ms);
int nos_reproj_time_kernel(nos_dataset* ds, const double R[9], const double t[3],
                           const double intr[4], const nos_loss* loss, double min_depth,
                           int repeats, double* kernel_ms, double* total_ms);
int nos_ndt3_time_kernel(nos_dataset* ds, const double R2[4], const double t2[2],
                         const nos_loss* loss, int repeats, double* kernel_ms,
                         double* total_ms);
/* Per-launch device timing inside a running loop: between _begin and _end every assemble
 * kernel launched through this context is bracketed by a HIP event pair recorded on the
 * stream it is launched on (every sample_every-th launch, up to max_launches timed launches per
 * device; the two event records cost about a microsecond of host time each).  _end synchronises
 * and returns the number of timed launches and their mean / min / max duration.
 * sample_every == 0 selects the bracket form for back-to-back launch trains (the device-resident
 * loop): ONE event is recorded at _begin and one at _end on the launch stream, nothing in between
 * (an event between two queued kernels would serialise their dispatch and show up in what it
 * measures); _end returns the launches in between and (t_end - t_begin) / launches as mean = min =
 * max — an upper bound of the kernel duration that includes whatever else ran in the train. */
int nos_ctx_profile_begin(nos_ctx* ctx, int max_launches, int sample_every);
int nos_ctx_profile_end(nos_ctx* ctx, int* n_launches, double* mean_ms, double* min_ms,
                        double* max_ms);
/* Demangled symbol of the hot-path kernel launched last on `shard` of this context ("" if none yet): the template
 * instantiation the library chose — problem, element type, loss, launch geometry or loop form — exactly as
 * rocprofv3 --kernel-trace lists it. */
int nos_ctx_last_kernel(const nos_ctx* ctx, int shard, char* buf, size_t capacity);
const char* nos_status_string(int status);
/* Thread-local description of the last failure in this thread ("" if none). */
const char* nos_last_error(void);
const char* nos_version(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* NOS_H_ */
