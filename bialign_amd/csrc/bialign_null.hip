// bialign_null.hip -- the kernels of the shuffled-null batches (bialign_null.hpp), their launchers and C entry points.
// A unit of its own: the sweeps' units do not see it.
#include "bialign_host.hpp"
#include "bialign_null.hpp"

namespace bialign {

// the fields the three shuffle kernels share
template <class Args>
static Args shuffle_args(const bialign_batch* b, int first, int count) {
  Args a{};
  a.pairs = b->d_pairs.p;
  a.src_off = b->null.d_off.p;
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
  const bool dinuc = b->null.model == BIALIGN_NULL_DINUCLEOTIDE;
  const int max_m = dinuc ? NULL_DINUC_MAX_M : NULL_FEAT_MAX_M;
  if (b->null_max_m < 1 || b->null_max_m > max_m)
    return fail(BIALIGN_E_UNSUPPORTED, "%s shuffle: longest B molecule %d outside 1..%d", what, b->null_max_m, max_m);
  a.model = b->null.model;
  a.tree_cap = null_tree_cap();
  const size_t bytes = dinuc ? (size_t)null_dinuc_lds(b->null_max_m) : (size_t)b->null_max_m * sizeof(uint16_t);
  return launch(kernel, dim3((unsigned)std::min(a.count, NULL_FEAT_MAX_GRID)), dim3(64), (bytes + 15) / 16 * 16, b->eng->stream, a);
}

// FEATURE-form null batch
static int launch_shuffle_features(bialign_batch* b, int first, int count) {
  const int64_t src_tot = (int64_t)b->null.d_seq.n;  // doubles per plane of the uploaded B features
  ShuffleFeatArgs a = shuffle_args<ShuffleFeatArgs>(b, first, count);
  a.src_seq = b->null.d_seq.p;
  a.src_up = b->null.d_feat.p;
  a.src_down = b->null.d_feat.p + src_tot;
  a.src_unp = b->null.d_feat.p + 2 * src_tot;
  a.dst_seq = b->d_seq_b.p;
  a.dst_up = b->tables.d_feat_b.p;
  a.dst_down = b->tables.d_feat_b.p + b->tables.feat_tot_b;
  a.dst_unp = b->tables.d_feat_b.p + 2 * b->tables.feat_tot_b;
  return launch_wave_shuffle(shuffle_features_kernel, "feature", b, a);
}

// DENSE-form null batch: the finished permutations go to null.d_perm
// LOOKUP-form null batch under the dinucleotide model: the same kernel for the gathered codes alone, no permutations kept
static int launch_shuffle_index(bialign_batch* b, int first, int count) {
  ShuffleIndexArgs a = shuffle_args<ShuffleIndexArgs>(b, first, count);
  a.src_seq = b->dense1 ? nullptr : b->null.d_seq.p;
  a.src_cls = b->dense ? nullptr : b->null.d_cls.p;
  a.dst_seq = b->d_seq_b.p;
  a.dst_cls = b->d_cls_b.p;
  a.dst_perm = b->null_dense ? b->null.d_perm.p : nullptr;
  return launch_wave_shuffle(shuffle_index_kernel, "index", b, a);
}

int launch_permute_tables(bialign_batch* b, int first, int count) {
  if (!b->null_dense || count < 1) return BIALIGN_OK;
  PermuteArgs a{};
  a.pairs = b->d_pairs.p;
  a.order = b->d_order.p + first;
  a.perm = b->null.d_perm.p;
  a.src = b->null.d_tab.p;
  a.src_off = b->null.d_tab_off.p;
  a.tab = b->tables.d_tab.p;
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
  if (b->null_dense || b->null.model == BIALIGN_NULL_DINUCLEOTIDE) return launch_shuffle_index(b, first, count);
  ShuffleArgs a = shuffle_args<ShuffleArgs>(b, first, count);
  a.src_seq = b->null.d_seq.p;
  a.src_cls = b->null.d_cls.p;
  a.dst_seq = b->d_seq_b.p;
  a.dst_cls = b->d_cls_b.p;
  return launch(shuffle_codes_kernel, dim3((unsigned)(((int64_t)count + NULL_BLOCK - 1) / NULL_BLOCK)), dim3(NULL_BLOCK), 0,
                b->eng->stream, a);
}

int launch_null_stats(bialign_batch* b, const int32_t* d_observed) {
  NullStatsArgs a{};
  a.scores = b->d_scores.p;
  a.observed = d_observed;
  a.out = b->null.d_stats.p;
  a.npairs = b->null_npairs;
  a.replicas = b->null_R;
  constexpr int WAVES = NULL_BLOCK / 64;
  return launch(null_stats_kernel, dim3((unsigned)((b->null_npairs + WAVES - 1) / WAVES)), dim3(NULL_BLOCK), 0, b->eng->stream, a);
}

}  // namespace bialign

using namespace bialign;

extern "C" {

int bialign_batch_get_null_scores(const bialign_batch* b, int32_t* out) {
  if (!b || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called");
  HIP_TRY(hipSetDevice(b->eng->device));
  HIP_TRY(hipMemcpy(out, b->d_scores.p, sizeof(int32_t) * b->npairs, hipMemcpyDeviceToHost));
  return BIALIGN_OK;
}

int bialign_batch_get_null_stats(const bialign_batch* cb, const int32_t* observed, bialign_null_stats* out) {
  if (!cb || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!cb->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  bialign_batch* b = const_cast<bialign_batch*>(cb);  // (the reduction's buffers and times are the batch's)
  if (int rc = bialign_batch_wait(b)) return rc;
  if (!b->ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called");
  HIP_TRY(hipSetDevice(b->eng->device));
  hipStream_t st = b->eng->stream;
  if (observed) HIP_TRY(b->null.d_obs.upload(observed, (size_t)b->null_npairs, st));
  StageClock& clk = b->null.stats_clock;
  clk.reset();
  HIP_TRY(clk.mark(st));
  if (int rc = launch_null_stats(b, observed ? b->null.d_obs.p : nullptr)) return rc;
  HIP_TRY(clk.mark(st, Stage::Stats));
  HIP_TRY(hipMemcpyAsync(out, b->null.d_stats.p, sizeof(bialign_null_stats) * b->null_npairs, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(clk.finish());
  return BIALIGN_OK;
}

int bialign_batch_get_null_info(const bialign_batch* b, bialign_null_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  info->shuffle_ms = b->clock.ms(Stage::Shuffle);
  info->stats_ms = b->null.stats_clock.ms(Stage::Stats);
  info->replica_bytes = (int64_t)(b->d_seq_b.n + b->d_cls_b.n + (b->feat ? b->tables.d_feat_b.n * sizeof(double) : 0) +
                                  b->null.d_perm.n * sizeof(uint16_t));
  return BIALIGN_OK;
}

int bialign_batch_set_null_model(bialign_batch* b, int32_t model) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  if (model != BIALIGN_NULL_MONO && model != BIALIGN_NULL_DINUCLEOTIDE)
    return fail(BIALIGN_E_INVALID, "unknown null model %d (BIALIGN_NULL_MONO, BIALIGN_NULL_DINUCLEOTIDE)", model);
  if (model == BIALIGN_NULL_DINUCLEOTIDE) {
    if (b->dense1)
      return fail(BIALIGN_E_UNSUPPORTED, "the dinucleotide model shuffles B's sequence letters: with mu1 in DENSE form B has none");
    if (b->null_max_m > BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN)  // (bialign_null.hpp checks the bound against its LDS layout)
      return fail(BIALIGN_E_UNSUPPORTED, "the dinucleotide model keeps a molecule's edge list in LDS: longest B molecule %d exceeds %d",
                  b->null_max_m, BIALIGN_NULL_DINUCLEOTIDE_MAX_LEN);
  }
  if (int rc = bialign_batch_wait(b)) return rc;
  b->null.model = model;
  return BIALIGN_OK;
}

int bialign_batch_get_null_model(const bialign_batch* b, int32_t* model) {
  if (!b || !model) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  *model = b->null.model;
  return BIALIGN_OK;
}

// What the three dumps below share once their own arguments are checked: the replica is in range, the batch idle and
// uploaded, and virtual pair *v = pair * R + replica shuffled anew on the engine's stream.
static int null_dump_begin(bialign_batch* b, int32_t pair, int32_t replica, int* v) {
  if (pair < 0 || pair >= b->null_npairs) return fail(BIALIGN_E_INVALID, "pair %d out of range", pair);
  if (replica < 0 || replica >= b->null_R) return fail(BIALIGN_E_INVALID, "replica %d out of range", replica);
  if (int rc = bialign_batch_wait(b)) return rc;
  HIP_TRY(hipSetDevice(b->eng->device));
  HIP_TRY(hipStreamWaitEvent(b->eng->stream, b->uploaded, 0));
  *v = pair * b->null_R + replica;
  return launch_shuffle_null(b, *v, 1);
}

int bialign_batch_dump_null_codes(bialign_batch* b, int32_t pair, int32_t replica, uint8_t* seq, uint8_t* cls) {
  if (!b || !seq || !cls) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  int v;
  if (int rc = null_dump_begin(b, pair, replica, &v)) return rc;
  hipStream_t st = b->eng->stream;
  const PairDesc& d = b->pairs[v];
  HIP_TRY(hipMemcpyAsync(seq, b->d_seq_b.p + d.seq_b, (size_t)d.m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(cls, b->d_cls_b.p + d.seq_b, (size_t)d.m, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

int bialign_batch_dump_null_features(bialign_batch* b, int32_t pair, int32_t replica, double* up, double* down, double* unp) {
  if (!b || !up || !down || !unp) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R || !b->feat) return fail(BIALIGN_E_INVALID, "not a FEATURE-form null batch (bialign_batch_create_null_features)");
  int v;
  if (int rc = null_dump_begin(b, pair, replica, &v)) return rc;
  hipStream_t st = b->eng->stream;
  const PairDesc& d = b->pairs[v];
  double* const out[3] = {up, down, unp};
  for (int f = 0; f < 3; ++f)
    HIP_TRY(hipMemcpyAsync(out[f], b->tables.d_feat_b.p + (size_t)f * b->tables.feat_tot_b + d.seq_b, (size_t)d.m * sizeof(double),
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

int bialign_batch_dump_null_tables(bialign_batch* b, int32_t pair, int32_t replica, int32_t* mu1_out, int32_t* mu2_out) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R || !b->null_dense) return fail(BIALIGN_E_INVALID, "not a DENSE-form null batch (bialign_batch_create_null_dense)");
  if (mu1_out && !b->dense1) return fail(BIALIGN_E_INVALID, "mu1_out given, but mu1 of this batch is in LOOKUP form");
  if (mu2_out && !b->dense) return fail(BIALIGN_E_INVALID, "mu2_out given, but mu2 of this batch is in LOOKUP form");
  // the replica's permutation, then its tables in their place in the chunk buffer (which may hold another chunk's by now;
  // results of a run live elsewhere)
  int v;
  if (int rc = null_dump_begin(b, pair, replica, &v)) return rc;
  hipStream_t st = b->eng->stream;
  const int pos = (int)(std::find(b->order.begin(), b->order.end(), v) - b->order.begin());
  if (int rc = launch_permute_tables(b, pos, 1)) return rc;
  const PairDesc& d = b->pairs[v];
  const size_t nm = (size_t)d.n * d.m;
  if (mu2_out) HIP_TRY(hipMemcpyAsync(mu2_out, b->tables.d_tab.p + d.tab_off, nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (mu1_out)
    HIP_TRY(hipMemcpyAsync(mu1_out, b->tables.d_tab.p + d.tab_off + (b->dense ? nm : 0), nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

}  // extern "C"
