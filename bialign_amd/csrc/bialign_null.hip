// bialign_null.hip -- the kernels of the shuffled-null batches (bialign_null.hpp) and their launchers.
// A unit of its own: the sweeps' units do not see it.
#include "bialign_host.hpp"
#include "bialign_null.hpp"

namespace bialign {

// the fields the three shuffle kernels share
template <class Args>
static Args shuffle_args(const bialign_batch* b, int first, int count) {
  Args a{};
  a.pairs = b->d_pairs.p;
  a.src_off = b->d_null_off.p;
  a.first = first;
  a.count = count;
  a.replicas = b->null_R;
  a.seed = b->null_seed;
  return a;
}

// CAP of the dinucleotide model's step 2; BIALIGN_NULL_TREE_CAP: tests, a smaller one (0: every replica takes the fallback)
static int32_t null_tree_cap() {
  const char* e = getenv("BIALIGN_NULL_TREE_CAP");
  return e ? std::clamp(atoi(e), 0, NULL_TREE_CAP) : NULL_TREE_CAP;
}

// The two wave-per-pair kernels: one wave per virtual pair, the index array of the batch's longest B in LDS
// (bialign_batch_create_null_features / _dense refuse longer ones than NULL_FEAT_MAX_M); under the dinucleotide model the
// whole layout of null_dinuc_perm_to_lds (bialign_batch_set_null_model refuses longer ones than NULL_DINUC_MAX_M)
template <class Args>
static int launch_wave_shuffle(void (*kernel)(Args), const char* what, const bialign_batch* b, Args a) {
  const bool dinuc = b->null_model == BIALIGN_NULL_DINUCLEOTIDE;
  const int max_m = dinuc ? NULL_DINUC_MAX_M : NULL_FEAT_MAX_M;
  if (b->null_max_m < 1 || b->null_max_m > max_m)
    return fail(BIALIGN_E_UNSUPPORTED, "%s shuffle: longest B molecule %d outside 1..%d", what, b->null_max_m, max_m);
  a.model = b->null_model;
  a.tree_cap = null_tree_cap();
  const size_t bytes = dinuc ? (size_t)null_dinuc_lds(b->null_max_m) : (size_t)b->null_max_m * sizeof(uint16_t);
  return launch(kernel, dim3((unsigned)std::min(a.count, NULL_FEAT_MAX_GRID)), dim3(64), (bytes + 15) / 16 * 16, b->eng->stream, a);
}

// FEATURE-form null batch
static int launch_shuffle_features(bialign_batch* b, int first, int count) {
  const int64_t src_tot = (int64_t)b->d_null_seq.n;  // doubles per plane of the uploaded B features
  ShuffleFeatArgs a = shuffle_args<ShuffleFeatArgs>(b, first, count);
  a.src_seq = b->d_null_seq.p;
  a.src_up = b->d_null_feat.p;
  a.src_down = b->d_null_feat.p + src_tot;
  a.src_unp = b->d_null_feat.p + 2 * src_tot;
  a.dst_seq = b->d_seq_b.p;
  a.dst_up = b->d_feat_b.p;
  a.dst_down = b->d_feat_b.p + b->feat_tot_b;
  a.dst_unp = b->d_feat_b.p + 2 * b->feat_tot_b;
  return launch_wave_shuffle(shuffle_features_kernel, "feature", b, a);
}

// DENSE-form null batch: the finished permutations go to d_null_perm
// LOOKUP-form null batch under the dinucleotide model: the same kernel for the gathered codes alone, no permutations kept
static int launch_shuffle_index(bialign_batch* b, int first, int count) {
  ShuffleIndexArgs a = shuffle_args<ShuffleIndexArgs>(b, first, count);
  a.src_seq = b->dense1 ? nullptr : b->d_null_seq.p;
  a.src_cls = b->dense ? nullptr : b->d_null_cls.p;
  a.dst_seq = b->d_seq_b.p;
  a.dst_cls = b->d_cls_b.p;
  a.dst_perm = b->null_dense ? b->d_null_perm.p : nullptr;
  return launch_wave_shuffle(shuffle_index_kernel, "index", b, a);
}

int launch_permute_tables(bialign_batch* b, int first, int count) {
  if (!b->null_dense || count < 1) return BIALIGN_OK;
  PermuteArgs a{};
  a.pairs = b->d_pairs.p;
  a.order = b->d_order.p + first;
  a.perm = b->d_null_perm.p;
  a.src = b->d_null_tab.p;
  a.src_off = b->d_null_tab_off.p;
  a.tab = b->d_tab.p;
  a.replicas = b->null_R;
  a.forms = (b->dense ? 1 : 0) + (b->dense1 ? 1 : 0);
  int64_t groups = 1;  // workgroups per pair: one per tile of the launch's tallest stack of tables
  size_t lds = 0;      // ... with the launch's largest LDS tile
  for (int t = first; t < first + count; ++t) {
    const PairDesc& d = b->pairs[b->order[t]];
    const int32_t T = permute_tile_rows(d.m);
    const int64_t rows = (int64_t)d.n * a.forms, tr = T ? T : PERM_ROWS;
    groups = std::max(groups, (rows + tr - 1) / tr);
    lds = std::max(lds, (size_t)std::min<int64_t>(T, rows) * d.m * sizeof(int32_t));
  }
  return launch(permute_tables_kernel, dim3(count, (unsigned)std::min<int64_t>(groups, PERM_MAX_GRID_Y)), dim3(64 * PERM_WAVES), lds,
                b->eng->stream, a);
}

int launch_shuffle_null(bialign_batch* b, int first, int count) {
  if (!b->null_R || count < 1) return BIALIGN_OK;
  if (b->feat) return launch_shuffle_features(b, first, count);
  if (b->null_dense || b->null_model == BIALIGN_NULL_DINUCLEOTIDE) return launch_shuffle_index(b, first, count);
  ShuffleArgs a = shuffle_args<ShuffleArgs>(b, first, count);
  a.src_seq = b->d_null_seq.p;
  a.src_cls = b->d_null_cls.p;
  a.dst_seq = b->d_seq_b.p;
  a.dst_cls = b->d_cls_b.p;
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
