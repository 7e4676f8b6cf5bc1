// nos_score.hip — nos_ndt_score_batch (C ABI of include/nos.h) and the host path of nos_voxel_map_score_batch (whose
// entry point is in nos_voxelmap.hip; the store, struct nos_voxel_map, is voxel_store_host.hpp's, which only that unit includes).
//
// B (scan, pose) problems scored against one map — a snapshot (nos_ndt_map) or the LIVE voxel store — by
// nos::score_batch_kernel (score_kernels.hpp): matches, matched points and the cost Σ ρ per problem, nothing written in
// between.  One upload of descriptors, two launches on one stream (the chunks, then the per-problem sums), one copy back,
// one host wait; the memory of a call follows the scans and the batch, never the map.
#include "batch_host.hpp"
#include "score_kernels.hpp"

static_assert(sizeof(nos_pose_score) == 32 && sizeof(nos::ScoreRow) == sizeof(nos_pose_score), "nos_pose_score layout");
static_assert(offsetof(nos_pose_score, matched_points) == offsetof(nos::ScoreRow, matched_points) &&
                  offsetof(nos_pose_score, cost) == offsetof(nos::ScoreRow, cost),
              "nos_pose_score layout");

namespace nosd {
namespace {

struct ScoreCall {
  nos_ctx* ctx;  // the map's context; NULL: the map argument was NULL
  nos_scan* const* scans;
  int n;
  const double* R;  // [n][9]
  const double* t;  // [n][3]
  const nos_loss* loss;
  int max_neighbors;
  nos_pose_score* scores;
};

// Descriptors and the block list up through pinned memory, one pooled device block for them, the rows and the chunk
// partials, the two launches, the rows down in one copy, one synchronisation (BatchTrip), then the caller's array.
template <typename View>
int run_score(const ScoreCall& c, int loss_kind, const View& view, unsigned int* d_error) {
  DeviceSlot& slot = c.ctx->slots[0];
  hipStream_t stream = slot.stream;
  const size_t B = size_t(c.n);
  uint64_t total_blocks = 0;
  for (size_t i = 0; i < B; ++i) total_blocks += (uint64_t(c.scans[i]->n) + nos::kScoreChunkPoints - 1) / nos::kScoreChunkPoints;
  if (total_blocks >= (uint64_t(1) << 31)) return fail(NOS_ERR_UNSUPPORTED, "too many points for one score call");
  BatchTrip trip(slot);
  const auto descs = trip.section(BatchTrip::kUp, B * sizeof(nos::ScoreDesc));
  const auto blocks = trip.section(BatchTrip::kUp, size_t(total_blocks) * sizeof(uint2));
  const auto rows = trip.section(BatchTrip::kDown, (B + 1) * sizeof(nos::ScoreRow));
  const auto partials = trip.section(BatchTrip::kDeviceOnly, size_t(total_blocks) * sizeof(nos::ScorePartial));
  const int rc = trip.open();
  if (rc != NOS_OK) return rc;
  uint2* const h_blocks = trip.host<uint2>(blocks);
  uint32_t next_block = 0;
  for (size_t i = 0; i < B; ++i) {
    const nos_scan* scan = c.scans[i];
    nos::ScoreDesc& d = *new (trip.host<nos::ScoreDesc>(descs) + i) nos::ScoreDesc{};
    d.points = scan->d_planes;
    d.n_points = scan->n;
    set_pose(d, c.R + 9 * i, c.t + 3 * i);
    d.first_block = next_block;
    d.n_chunks = uint32_t((uint64_t(scan->n) + nos::kScoreChunkPoints - 1) / nos::kScoreChunkPoints);
    for (uint32_t k = 0; k < d.n_chunks; ++k) h_blocks[next_block + k] = make_uint2(uint32_t(i), k);
    next_block += d.n_chunks;
  }
  nos::ScoreLoss loss{};
  fill_loss(c.loss, loss.la, loss.lb, loss.lc);
  const nos::ScoreDesc* const d_descs = trip.dev<const nos::ScoreDesc>(descs);
  nos::ScorePartial* const d_partials = trip.dev<nos::ScorePartial>(partials);
  if (trip.send() && (d_error == nullptr || trip.check(hipMemsetAsync(d_error, 0, sizeof(unsigned int), stream)))) {
    if (next_block > 0) {
      slot.last_kernel = with_loss(loss_kind, [&](auto kind) {  // one loss for the whole call
        const auto kernel = nos::score_batch_kernel<View, decltype(kind)::value>;
        hipLaunchKernelGGL(kernel, dim3(next_block), dim3(nos::kScoreBlock), 0, stream, view, d_error, d_descs,
                           trip.dev<const uint2>(blocks), loss, c.max_neighbors, d_partials);
        return reinterpret_cast<const void*>(kernel);
      });
      if (slot.prof_on && slot.prof_every == 0) ++slot.prof_launches;  // SELF-REPORTED (bracket profiler)
    }
    hipLaunchKernelGGL(nos::score_finish_kernel, dim3(unsigned((B + nos::kScoreBlock - 1) / nos::kScoreBlock)),
                       dim3(nos::kScoreBlock), 0, stream, d_descs, uint32_t(B), d_partials, d_error, trip.dev<nos::ScoreRow>(rows));
    if (slot.prof_on && slot.prof_every == 0) ++slot.prof_launches;
    if (trip.launched()) trip.fetch();
  }
  const int status = trip.close("score batch");
  if (status != NOS_OK) return status;
  const nos::ScoreRow* const h_rows = trip.host<const nos::ScoreRow>(rows);
  if (h_rows[0].matches != 0)  // live store only; before anything of the caller's is written
    return fail(NOS_ERR_HIP, "scoring against the voxel store failed: a table probe ran through the whole table");
  memcpy(c.scores, h_rows + 1, B * sizeof(nos_pose_score));
  return NOS_OK;
}

// Validation first (nothing is launched and nothing written before every check has passed), then the launches.
// more_checks(): what the kind of map rejects beyond the common list, after it (→ a status).
template <typename View, typename Checks>
int score_batch(const ScoreCall& c, const Checks& more_checks, const View& view, unsigned int* d_error) {
  if (c.n < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_problems < 0");
  if (c.n == 0) return NOS_OK;
  if (!c.ctx || !c.scans || !c.R || !c.t || !c.scores) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL array");
  nos_ctx* ctx = c.ctx;
  CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  const int rc_scans = check_scans(ctx, c.scans, c.n);
  if (rc_scans != NOS_OK) return rc_scans;
  int loss_kind = 0;
  const int rc = check_loss(c.loss, &loss_kind);
  if (rc != NOS_OK) return rc;
  if (c.max_neighbors < 1 || c.max_neighbors > 2) return fail(NOS_ERR_UNSUPPORTED, "max_neighbors must be 1 or 2");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "scoring needs a single-device context");
  const int rc_more = more_checks();
  if (rc_more != NOS_OK) return rc_more;
  return run_score(c, loss_kind, view, d_error);
}

}  // namespace

int score_live(const LiveStore* store, nos_scan* const* scans, int32_t n_problems, const double* R, const double* t,
               const nos_loss* loss, int max_neighbors, nos_pose_score* scores) {
  static const LiveStore no_store{};  // never launched with: a NULL map is rejected first
  const LiveStore& s = store ? *store : no_store;
  auto more_checks = [&s] { return check_live_store(s); };  // what nos_voxel_map_match rejects, in its order
  return score_batch(ScoreCall{s.ctx, scans, n_problems, R, t, loss, max_neighbors, scores}, more_checks, s.view, s.d_error);
}

}  // namespace nosd

extern "C" {

int nos_ndt_score_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, const double* R, const double* t,
                        const nos_loss* loss, int max_neighbors, nos_pose_score* scores) {
  static const nos::MapView no_map{};  // never launched with: a NULL map is rejected first
  return nosd::score_batch(nosd::ScoreCall{map ? map->ctx : nullptr, scans, n_problems, R, t, loss, max_neighbors, scores},
                           [] { return NOS_OK; }, map ? map->view : no_map, static_cast<unsigned int*>(nullptr));
}

}  // extern "C"
