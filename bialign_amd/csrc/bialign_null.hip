// bialign_null.hip -- the kernels of the shuffled-null batches (bialign_null.hpp) and their launchers.
// A unit of its own: the sweeps' units do not see it.
#include "bialign_host.hpp"
#include "bialign_null.hpp"

namespace bialign {

// FEATURE-form null batch: one wave per virtual pair, the index array of the batch's longest B in LDS
static int launch_shuffle_features(bialign_batch* b, int first, int count) {
  if (b->null_max_m < 1 || b->null_max_m > NULL_FEAT_MAX_M)  // (bialign_batch_create_null_features refuses longer ones)
    return fail(BIALIGN_E_UNSUPPORTED, "feature shuffle: longest B molecule %d outside 1..%d", b->null_max_m, NULL_FEAT_MAX_M);
  const int64_t src_tot = (int64_t)b->d_null_seq.n;  // doubles per plane of the uploaded B features
  ShuffleFeatArgs a{};
  a.pairs = b->d_pairs.p;
  a.src_off = b->d_null_off.p;
  a.src_seq = b->d_null_seq.p;
  a.src_up = b->d_null_feat.p;
  a.src_down = b->d_null_feat.p + src_tot;
  a.src_unp = b->d_null_feat.p + 2 * src_tot;
  a.dst_seq = b->d_seq_b.p;
  a.dst_up = b->d_feat_b.p;
  a.dst_down = b->d_feat_b.p + b->feat_tot_b;
  a.dst_unp = b->d_feat_b.p + 2 * b->feat_tot_b;
  a.first = first;
  a.count = count;
  a.replicas = b->null_R;
  a.seed = b->null_seed;
  const size_t lds = ((size_t)b->null_max_m * sizeof(uint16_t) + 15) / 16 * 16;
  return launch(shuffle_features_kernel, dim3((unsigned)std::min(count, NULL_FEAT_MAX_GRID)), dim3(64), lds, b->eng->stream, a);
}

int launch_shuffle_null(bialign_batch* b, int first, int count) {
  if (!b->null_R || count < 1) return BIALIGN_OK;
  if (b->feat) return launch_shuffle_features(b, first, count);
  ShuffleArgs a{};
  a.pairs = b->d_pairs.p;
  a.src_off = b->d_null_off.p;
  a.src_seq = b->d_null_seq.p;
  a.src_cls = b->d_null_cls.p;
  a.dst_seq = b->d_seq_b.p;
  a.dst_cls = b->d_cls_b.p;
  a.first = first;
  a.count = count;
  a.replicas = b->null_R;
  a.seed = b->null_seed;
  return launch(shuffle_codes_kernel, dim3((unsigned)(((int64_t)count + NULL_BLOCK - 1) / NULL_BLOCK)), dim3(NULL_BLOCK), 0,
                b->eng->stream, a);
}

int launch_null_stats(bialign_batch* b, const int32_t* d_observed) {
  NullStatsArgs a{};
  a.scores = b->d_scores.p;
  a.observed = d_observed;
  a.out = b->d_null_stats.p;
  a.npairs = b->null_npairs;
  a.replicas = b->null_R;
  constexpr int WAVES = NULL_BLOCK / 64;
  return launch(null_stats_kernel, dim3((unsigned)((b->null_npairs + WAVES - 1) / WAVES)), dim3(NULL_BLOCK), 0, b->eng->stream, a);
}

}  // namespace bialign
