// bialign_null.hip -- the kernels of the shuffled-null batches (bialign_null.hpp) and their launchers.
// A unit of its own: the sweeps' units do not see it.
#include "bialign_host.hpp"
#include "bialign_null.hpp"

namespace bialign {

int launch_shuffle_null(bialign_batch* b, int first, int count) {
  if (!b->null_R || count < 1) return BIALIGN_OK;
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
