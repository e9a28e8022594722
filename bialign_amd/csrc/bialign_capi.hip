// bialign_capi.hip -- C ABI (include/bialign.h) over the gfx950 kernels.
//
// Host-side responsibilities: allocate and upload what the planner (bialign_plan.hpp: validation, layout in HBM,
// HBM-budgeted chunks, team shapes) decided, launch fill + traceback per chunk on the engine's
// stream, time the kernels with HIP events, hand results back.  No CPU compute
// path exists here: if the device or a kernel is unavailable the call fails.
#include "bialign_hits.hpp"

using namespace bialign;

namespace bialign {

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// ---- cross-CU launches, one at a time per device (all engines of the process)
static std::mutex g_xcu_mu;
static hipEvent_t g_xcu_done[64] = {};  // per device: the last cross-CU launch (never destroyed: process lifetime)

int xcu_serial_begin(bialign_engine* e) {
  g_xcu_mu.lock();  // held until xcu_serial_end: wait, launch and record are one step
  if (getenv("BIALIGN_XCU_NOSERIAL")) return BIALIGN_OK;  // tests: provoke lost co-residency
  hipEvent_t& ev = g_xcu_done[e->device & 63];
  hipError_t err = hipSuccess;
  if (!ev) err = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  else err = hipStreamWaitEvent(e->stream, ev, 0);
  if (err != hipSuccess) {
    g_xcu_mu.unlock();
    return fail(BIALIGN_E_DEVICE, "cross-CU launch ordering: %s", hipGetErrorString(err));
  }
  return BIALIGN_OK;
}

int xcu_serial_end(bialign_engine* e) {
  hipError_t err = hipSuccess;
  if (!getenv("BIALIGN_XCU_NOSERIAL")) err = hipEventRecord(g_xcu_done[e->device & 63], e->stream);
  g_xcu_mu.unlock();
  if (err != hipSuccess) return fail(BIALIGN_E_DEVICE, "cross-CU launch ordering: %s", hipGetErrorString(err));
  return BIALIGN_OK;
}

}  // namespace bialign

namespace {

// The tiled kernels are templates on max_shift: fn(std::integral_constant<int, S>{}) for the batch's run-time S.
template <typename Fn>
int with_shift(const bialign_batch* b, const char* what, Fn&& fn) {
  switch (b->S) {
    case 0: return fn(std::integral_constant<int, 0>{});
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 3: return fn(std::integral_constant<int, 3>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 5: return fn(std::integral_constant<int, 5>{});
  }
  return fail(BIALIGN_E_UNSUPPORTED, "no %s kernel for affine=%d max_shift=%d", what, b->affine, b->S);
}

int launch_fill(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  if (b->wide) return launch_fill_wide(b, v, first, count);
  return with_shift(b, "fill", [&](auto s) {
    constexpr int S = decltype(s)::value;
    if (b->own_sweeps()) return b->affine ? launch_fill_affine_local<S>(b, v, first, count) : launch_fill_linear_local<S>(b, v, first, count);
    return b->affine ? launch_fill_affine<S>(b, v, first, count) : launch_fill_linear<S>(b, v, first, count);
  });
}

// Batches with an end key (BatchPlan::end_key: local, score-only overlap): behind a sweep, the pairs' keys become their
// scores and ends (bialign_free_ends.hpp)
int launch_end_key_finish(const bialign_batch* b, const DeviceBatch& v, int first, int count) {
  constexpr int BLOCK = 256;
  DeviceBatch w = v;
  w.order = v.order + first;
  return launch(end_key_finish_kernel<BLOCK>, dim3((count + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, b->eng->stream, w, count);
}

// Lean traceback of one chunk: as many (re-sweep, walk) rounds as its longest pair has strips.
int lean_traceback_rounds(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  hipStream_t st = b->eng->stream;
  HIP_TRY(hipMemsetAsync(b->d_tstate.p, 0, sizeof(TraceState) * b->npairs, st));
  int rounds = 0;
  for (int t = first; t < first + count; ++t) rounds = std::max(rounds, b->pairs[b->order[t]].NS);
  rounds = (rounds + b->resw_k - 1) / b->resw_k;
  return with_shift(b, "re-sweep", [&](auto s) {
    constexpr int S = decltype(s)::value;
    for (int r = 0; r < rounds; ++r) {
      int rc = b->affine ? launch_resweep_affine<S>(b, v, first, count) : launch_resweep_linear<S>(b, v, first, count);
      if (rc == BIALIGN_OK)
        rc = b->affine ? launch_traceback_affine_strip<S>(b, v, first, count) : launch_traceback_linear_strip<S>(b, v, first, count);
      if (rc) return rc;
    }
    return (int)BIALIGN_OK;
  });
}

// Level-checkpointed traceback of one chunk (bialign_wide.hpp): as many (segment sweep, walk) rounds as its longest pair
// has segments; every pair starts at its own top segment and drops out when its walk has ended.
int level_traceback_rounds(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  HIP_TRY(hipMemsetAsync(b->d_tstate.p, 0, sizeof(TraceState) * b->npairs, b->eng->stream));
  int rounds = 0;
  for (int t = first; t < first + count; ++t) {
    const PairDesc& d = b->pairs[b->order[t]];
    rounds = std::max(rounds, wide_segments(d.n, d.m, b->wide_seg));
  }
  for (int r = 0; r < rounds; ++r) {
    if (int rc = launch_segment_wide(b, v, first, count)) return rc;
    if (int rc = launch_traceback_level(b, v, first, count)) return rc;
  }
  return BIALIGN_OK;
}

int launch_traceback(const bialign_batch* b, const DeviceBatch& v, int first, int count, bool do_trace) {
  if (b->wide) return launch_traceback_wide(b, v, first, count, do_trace);
  return with_shift(b, "traceback", [&](auto s) {
    constexpr int S = decltype(s)::value;
    return b->affine ? launch_traceback_affine<S>(b, v, first, count, do_trace) : launch_traceback_linear<S>(b, v, first, count, do_trace);
  });
}

int launch_dump_any(const bialign_batch* b, const DeviceBatch& v, int pid, int32_t* d_out) {
  if (b->wide) return launch_dump_wide(b, v, pid, d_out);
  return with_shift(b, "dump", [&](auto s) {
    constexpr int S = decltype(s)::value;
    return b->affine ? launch_dump<S, 9>(b, v, pid, d_out) : launch_dump<S, 1>(b, v, pid, d_out);
  });
}

// A batch laid out for packed records has to continue with full ones (an offset did not fit): cut it into chunks
// again, now by the pairs' full-record sizes, within the layer buffer it already holds (a larger one only if a
// single pair needs it), and hand the new layout to the device.
int replan_full(bialign_batch* b) {
  if (!b->packed_sizing) return BIALIGN_OK;
  hipStream_t st = b->eng->stream;
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t need = *std::max_element(b->full_dwords.begin(), b->full_dwords.end());
  if ((int64_t)b->d_layers.n < need + 16) HIP_TRY(b->d_layers.alloc((size_t)need + 16));
  if (int rc = replan_full_layout(*b, (int64_t)b->d_layers.n - 16, (int64_t)b->d_tab.n)) return rc;
  HIP_TRY(hipMemcpy(b->d_pairs.p, b->pairs.data(), b->pairs.size() * sizeof(PairDesc), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_order.p, b->order.data(), b->order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return BIALIGN_OK;
}

int check_device_error(const bialign_batch* b) {
  int32_t err = 0;
  HIP_TRY(hipMemcpy(&err, b->d_err.p, sizeof err, hipMemcpyDeviceToHost));
  if (err) return fail(BIALIGN_E_DEVICE, "fill kernel: device error flag %d (1 = team hand-off timed out)", err);
  return BIALIGN_OK;
}

// streaming-write rate of a buffer in GB/s (second of two memset passes)
int probe_write_rate(bialign_engine* e, hipStream_t st, int32_t* p, size_t dwords, double* gbps) {
  float ms = 0;
  for (int rep = 0; rep < 2; ++rep) {
    HIP_TRY(hipEventRecord(e->ev[0], st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p, 0, dwords, st));
    HIP_TRY(hipEventRecord(e->ev[1], st));
    HIP_TRY(hipEventSynchronize(e->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms, e->ev[0], e->ev[1]));
  }
  *gbps = dwords * 4.0 / (ms * 1e6);
  return BIALIGN_OK;
}

// Null batch: the replicas' codes are input data like the uploaded codes -- outside the budget.  Allocated ahead of the
// budget's look at the free memory, which so has their size subtracted.
int alloc_replicas(bialign_batch* b) {
  HIP_TRY(b->d_seq_b.alloc((size_t)b->tot_b));
  HIP_TRY(b->d_cls_b.alloc((size_t)b->tot_b));
  if (b->feat) HIP_TRY(b->d_feat_b.alloc(3 * (size_t)b->tot_b));  // ... and so the replicas' three planes of features
  if (b->null_dense) {  // ... the replicas' permutations, and the real pairs' tables, which stay resident
    HIP_TRY(b->d_null_perm.alloc((size_t)b->tot_b));
    size_t real_dw = 0;
    for (int p = 0; p < b->npairs; p += b->null_R) real_dw += (size_t)b->tab_dwords[p];
    HIP_TRY(b->d_null_tab.alloc(real_dw));
  }
  return BIALIGN_OK;
}

// What the budget may count on: the free HBM, and the engine's cached buffers, which are reused or released below
int free_hbm(const bialign_batch* b, size_t* free_b) {
  const bialign_engine* eng = b->eng;
  size_t total_b = 0;
  HIP_TRY(hipMemGetInfo(free_b, &total_b));
  *free_b += (eng->layer_cache.n + eng->layer_cache2.n) * sizeof(int32_t);
  if (b->tab_scratch()) *free_b += eng->tab_cache.n * sizeof(int32_t);  // ... and so the cached table buffer
  return BIALIGN_OK;
}

// The layer buffer: a cached one if large enough, else a new one; if the device cannot provide a chunk of the
// planned size after all (fragmentation, another tenant), plan smaller chunks and try again
int alloc_layers(bialign_batch* b) {
  bialign_engine* eng = b->eng;
  for (int attempt = 0;; ++attempt) {
    // (slack: ghost tail pieces are read 16 B wide; behind the layers the wide-band affine sweep's ring, if the plan has one)
    const size_t layer_dw = (size_t)b->max_chunk_dwords + (size_t)b->max_chunk_ring_dwords + 16;
    DevBuf<int32_t>* slot = nullptr;  // the smallest cached buffer that is large enough
    for (DevBuf<int32_t>* c : {&eng->layer_cache, &eng->layer_cache2})
      if (c->p && c->n >= layer_dw && (!slot || c->n < slot->n)) slot = c;
    if (slot) {
      b->d_layers.swap(*slot);
      return BIALIGN_OK;
    }
    eng->layer_cache.release();
    eng->layer_cache2.release();
    hipError_t err = b->d_layers.alloc(layer_dw);
    if (err == hipSuccess && attempt == 0 && getenv("BIALIGN_TEST_FAIL_ALLOC")) {  // tests: pretend the first allocation failed
      b->d_layers.release();
      err = hipErrorOutOfMemory;
    }
    if (err == hipSuccess) return BIALIGN_OK;
    (void)hipGetLastError();
    b->d_layers.p = nullptr;
    b->d_layers.n = 0;
    const int64_t smaller = (int64_t)(b->max_chunk_dwords + b->max_chunk_tab_dwords + b->max_chunk_ring_dwords) * 3 / 4;
    if (attempt >= 3 || smaller < max_pair_need(*b))
      return fail(BIALIGN_E_DEVICE, "hipMalloc of %zu bytes of layer storage failed: %s", layer_dw * 4, hipGetErrorString(err));
    if (int rc = replan_smaller(*b, smaller)) return rc;
  }
}

// FEATURE form, DENSE-form null batch: the table buffer of the largest chunk, the engine's cached one if that is
// large enough
int alloc_tables(bialign_batch* b) {
  bialign_engine* eng = b->eng;
  if (!b->tab_scratch()) return BIALIGN_OK;
  const size_t tab_dw = (size_t)b->max_chunk_tab_dwords;
  if (eng->tab_cache.p && eng->tab_cache.n >= tab_dw) {
    b->d_tab.swap(eng->tab_cache);
  } else {
    eng->tab_cache.release();
    if (b->d_tab.alloc(tab_dw) != hipSuccess) {
      const hipError_t err = hipGetLastError();
      b->d_tab.p = nullptr;
      b->d_tab.n = 0;
      return fail(BIALIGN_E_DEVICE, "hipMalloc of %zu bytes of table storage failed: %s", tab_dw * 4, hipGetErrorString(err));
    }
  }
  return BIALIGN_OK;
}

// Upload (own stream: a batch can be prepared while another one sweeps), and the result buffers
int upload_inputs(bialign_batch* b, const bialign_scoring* sc, const bialign_pairs* pr, const bialign_features* ft, const NullPlan* nul) {
  bialign_engine* eng = b->eng;
  const int64_t tot_a = b->tot_a, tot_b = b->tot_b, tot_tab = b->tot_tab;
  hipStream_t st = eng->copy_stream;
  HIP_TRY(b->d_pairs.upload(b->pairs.data(), b->pairs.size(), st));
  HIP_TRY(b->d_order.upload(b->order.data(), b->order.size(), st));
  HIP_TRY(b->d_s1.upload(sc->s1, (size_t)sc->k1 * sc->k1, st));
  HIP_TRY(b->d_s2.upload(sc->s2, (size_t)sc->k2 * sc->k2, st));
  std::vector<uint8_t> zeros;
  if (b->dense || b->dense1) zeros.assign((size_t)(nul ? tot_a : std::max(tot_a, tot_b)), 0);  // codes a dense form replaces are unused
  HIP_TRY(b->d_seq_a.upload(b->dense1 ? zeros.data() : pr->seq_a, tot_a, st));
  HIP_TRY(b->d_cls_a.upload(b->dense ? zeros.data() : pr->cls_a, tot_a, st));
  if (nul) {  // B once, as the caller gave it: the shuffle kernel writes d_seq_b / d_cls_b from it ahead of every run's sweeps
    // (codes a dense form replaces are not uploaded: the replicas' codes of that kind are zero like those of any dense batch)
    if (b->dense1) HIP_TRY(hipMemsetAsync(b->d_seq_b.p, 0, std::max<size_t>((size_t)tot_b, 1), st));
    else HIP_TRY(b->d_null_seq.upload(nul->seq_b, (size_t)nul->tot_b, st));
    if (b->dense)  // (FEATURE form too: no classes)
      HIP_TRY(hipMemsetAsync(b->d_cls_b.p, 0, std::max<size_t>((size_t)tot_b, 1), st));
    else
      HIP_TRY(b->d_null_cls.upload(nul->cls_b, (size_t)nul->tot_b, st));
    HIP_TRY(b->d_null_off.upload(nul->off_b, (size_t)nul->npairs, st));
    HIP_TRY(b->d_null_stats.alloc((size_t)nul->npairs));
    for (hipEvent_t& e : b->null_evs) HIP_TRY(hipEventCreate(&e));
  } else {
    HIP_TRY(b->d_seq_b.upload(b->dense1 ? zeros.data() : pr->seq_b, tot_b, st));
    HIP_TRY(b->d_cls_b.upload(b->dense ? zeros.data() : pr->cls_b, tot_b, st));
  }
  std::vector<int32_t> tabs;
  std::vector<int64_t> mu1_offs;
  if (b->feat) {  // the molecules' features, three planes per side; a dense mu1's tables resident, pair after pair
    b->feat_tot_a = tot_a;
    b->feat_tot_b = tot_b;
    const double* src_a[3] = {ft->up_a, ft->down_a, ft->unp_a};
    const double* src_b[3] = {ft->up_b, ft->down_b, ft->unp_b};
    HIP_TRY(b->d_feat_a.alloc(3 * (size_t)tot_a));
    // null batch: d_feat_b is the replica planes (allocated above, filled by the shuffle kernel); B's own go beside d_null_seq
    DevBuf<double>& up_b = nul ? b->d_null_feat : b->d_feat_b;
    const int64_t src_tot_b = nul ? nul->tot_b : tot_b;
    HIP_TRY(up_b.alloc(3 * (size_t)src_tot_b));
    for (int f = 0; f < 3; ++f) {
      HIP_TRY(hipMemcpyAsync(b->d_feat_a.p + (size_t)f * tot_a, src_a[f], (size_t)tot_a * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(up_b.p + (size_t)f * src_tot_b, src_b[f], (size_t)src_tot_b * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (b->dense1) {
      mu1_offs.resize(pr->npairs);
      size_t tot1 = 0;
      for (int p = 0; p < pr->npairs; ++p) mu1_offs[p] = (int64_t)tot1, tot1 += (size_t)pr->len_a[p] * pr->len_b[p];
      tabs.resize(tot1);
      for (int p = 0; p < pr->npairs; ++p)
        std::memcpy(tabs.data() + mu1_offs[p], pr->mu1_dense + pr->mu1_off[p], (size_t)pr->len_a[p] * pr->len_b[p] * sizeof(int32_t));
      HIP_TRY(b->d_mu1.upload(tabs.data(), tabs.size(), st));
      HIP_TRY(b->d_mu1_off.upload(mu1_offs.data(), mu1_offs.size(), st));
    }
  } else if (b->null_dense) {  // the REAL pairs' tables end to end, mu2's, then mu1's; every replica's are made from them per chunk
    const int R = nul->replicas;
    std::vector<int64_t> offs((size_t)nul->npairs);
    tabs.resize(b->d_null_tab.n);
    int64_t at = 0;
    for (int p = 0; p < nul->npairs; ++p) {
      const size_t v = (size_t)p * R, nm = (size_t)pr->len_a[v] * pr->len_b[v];
      offs[p] = at;
      if (b->dense) std::memcpy(tabs.data() + at, pr->mu2_dense + pr->mu2_off[v], nm * sizeof(int32_t)), at += (int64_t)nm;
      if (b->dense1) std::memcpy(tabs.data() + at, pr->mu1_dense + pr->mu1_off[v], nm * sizeof(int32_t)), at += (int64_t)nm;
    }
    if (!tabs.empty()) HIP_TRY(hipMemcpyAsync(b->d_null_tab.p, tabs.data(), tabs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(b->d_null_tab_off.upload(offs.data(), offs.size(), st));
  } else if (b->dense || b->dense1) {  // the pairs' tables end to end (PairDesc::tab_off): mu2's, then mu1's
    tabs.resize((size_t)tot_tab);
    for (int p = 0; p < pr->npairs; ++p) {
      const size_t nm = (size_t)pr->len_a[p] * pr->len_b[p];
      int32_t* dst = tabs.data() + b->pairs[p].tab_off;
      if (b->dense) std::memcpy(dst, pr->mu2_dense + pr->mu2_off[p], nm * sizeof(int32_t)), dst += nm;
      if (b->dense1) std::memcpy(dst, pr->mu1_dense + pr->mu1_off[p], nm * sizeof(int32_t));
    }
    HIP_TRY(b->d_tab.upload(tabs.data(), tabs.size(), st));
  }
  if (getenv("BIALIGN_DEBUG")) {  // placement study: address and plain streaming-write rate of the layer buffer
    const size_t layer_dw = b->d_layers.n;
    double gbps = 0;
    if (int rc = probe_write_rate(eng, st, b->d_layers.p, layer_dw, &gbps)) return rc;
    fprintf(stderr, "[bialign] layers %p (%.1f GiB) memset %.0f GB/s\n", (void*)b->d_layers.p, layer_dw * 4.0 / (1 << 30), gbps);
  }
  HIP_TRY(b->d_scores.alloc(pr->npairs));
  if (b->free_ends()) HIP_TRY(b->d_span.alloc(4 * (size_t)pr->npairs));
  if (b->end_key()) HIP_TRY(b->d_end_key.alloc((size_t)pr->npairs));
  if (b->lean_trace || b->level_trace) HIP_TRY(b->d_tstate.alloc(pr->npairs));
  HIP_TRY(b->d_tlen.alloc(pr->npairs));
  HIP_TRY(b->d_complete.alloc(pr->npairs));
  HIP_TRY(b->d_err.alloc(1));
  HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), st));
  if (const char* e = getenv("BIALIGN_XCU_SPIN_LIMIT")) b->xcu_spin_limit = std::max(0, atoi(e));  // tests: force hand-off timeouts
  HIP_TRY(b->d_trace.alloc(b->trace_bytes));
  HIP_TRY(hipMemsetAsync(b->d_tlen.p, 0, sizeof(int32_t) * pr->npairs, st));
  HIP_TRY(hipMemsetAsync(b->d_complete.p, 0, sizeof(int32_t) * pr->npairs, st));
  HIP_TRY(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(b->uploaded, st));
  HIP_TRY(hipStreamSynchronize(st));  // the caller's host arrays may go away now
  return BIALIGN_OK;
}

// ---- hit search (bialign_hits.hpp): what a launch is given, and the state its results have ahead of a run
HitArgs hit_args(const bialign_batch* b, bool search) {
  HitArgs h{};
  h.max_hits = b->hit_spec.max_hits, h.max_walks = b->hit_spec.max_walks, h.min_score = b->hit_spec.min_score;
  h.search = search ? 1 : 0;
  h.lds_inputs = (int32_t)((b->lds_trace + 15) & ~size_t(15));
  h.mask_words = b->hit_mask_words;
  h.prof_off = b->d_hit_prof_off.p;
  h.profile = b->d_hit_profile.p;
  h.head = b->d_hit_head.p;
  h.hits = b->d_hit_rec.p;
  h.walks = b->d_hit_walks.p;
  h.trace = b->d_hit_trace.p;
  return h;
}

// profile: -infinity; status NOT_SEARCHED, no hits, no walks; records -1
int reset_hits(bialign_batch* b, hipStream_t st) {
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b->d_hit_profile.p, BIALIGN_NEG_INF, b->d_hit_profile.n, st));
  HIP_TRY(hipMemsetAsync(b->d_hit_head.p, 0, sizeof(int32_t) * b->d_hit_head.n, st));
  HIP_TRY(hipMemsetAsync(b->d_hit_rec.p, 0xff, sizeof(int32_t) * b->d_hit_rec.n, st));
  HIP_TRY(hipMemsetAsync(b->d_hit_walks.p, 0xff, sizeof(int32_t) * b->d_hit_walks.n, st));
  return BIALIGN_OK;
}

// the hit getters' common refusals, and the end of a pending run
int hits_ready(const bialign_batch* b) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->hits_on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  if (!b->ran || !b->hits_ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called since bialign_batch_set_hits");
  HIP_TRY(hipSetDevice(b->eng->device));
  return BIALIGN_OK;
}

}  // namespace

extern "C" {

int bialign_abi_version(void) { return BIALIGN_ABI_VERSION; }

int bialign_build_experiment(void) { return BIALIGN_EXP; }

const char* bialign_last_error(void) { return g_err.c_str(); }

int bialign_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(BIALIGN_E_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

int bialign_engine_create(int device, bialign_engine** out) {
  if (!out) return fail(BIALIGN_E_INVALID, "out is NULL");
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(BIALIGN_E_INVALID, "device %d out of range (0..%d)", device, n - 1);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(BIALIGN_E_UNSUPPORTED, "device %d is %s; this engine is built for gfx950 only", device,
                prop.gcnArchName);
  auto* e = new bialign_engine();
  e->device = device;
  e->num_cu = prop.multiProcessorCount;
  hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (err == hipSuccess) err = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
  for (int i = 0; i < 4 && err == hipSuccess; ++i) err = hipEventCreate(&e->ev[i]);
  if (err != hipSuccess) {
    bialign_engine_destroy(e);
    return fail(BIALIGN_E_DEVICE, "engine setup: %s", hipGetErrorString(err));
  }
  *out = e;
  return BIALIGN_OK;
}

void bialign_engine_destroy(bialign_engine* e) {
  if (!e) return;
  if (e->live_batches > 0) {  // destroy order is the caller's business (garbage collectors pick any): the
    e->closing = true;        // engine goes when its last batch goes
    return;
  }
  (void)hipSetDevice(e->device);
  for (auto& ev : e->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  delete e;
}

// bialign_batch_create (ft == nullptr), bialign_batch_create_features, and bialign_batch_create_null (nul != nullptr: pr
// describes the virtual pairs, whose off_b point into replica buffers that are allocated here and filled on the device);
// bialign_batch_create_null_features gives both: ft's B planes are then the real pairs' (NullPlan::off_b), the replica
// planes are allocated here.  The planner decides (bialign_plan.hpp), the steps between touch the device.
static int create_batch(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                        const bialign_pairs* pr, const bialign_features* ft, int64_t hbm_budget, bialign_batch** out,
                        const NullPlan* nul = nullptr) {
  if (!eng || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  *out = nullptr;
  std::unique_ptr<bialign_batch> b(new bialign_batch());
  b->eng = eng;
  if (int rc = check_inputs(prm, sc, pr, ft, nul, *b)) return rc;
  HIP_TRY(hipSetDevice(eng->device));
  int64_t colmax = 0;
  size_t free_b = 0;
  if (int rc = score_bound(prm, sc, pr, ft, nul, *b, &colmax)) return rc;
  if (int rc = plan_pairs(pr, nul, colmax, *b)) return rc;
  decide_pack(*b, colmax);
  if (nul)
    if (int rc = alloc_replicas(b.get())) return rc;
  if (int rc = free_hbm(b.get(), &free_b)) return rc;
  if (int rc = plan_storage(*b, budget_dwords(hbm_budget, free_b))) return rc;
  if (int rc = alloc_layers(b.get())) return rc;
  if (int rc = alloc_tables(b.get())) return rc;
  if (int rc = upload_inputs(b.get(), sc, pr, ft, nul)) return rc;
  ++eng->live_batches;
  *out = b.release();
  return BIALIGN_OK;
}

int bialign_batch_create(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                         const bialign_pairs* pr, int64_t hbm_budget, bialign_batch** out) {
  return create_batch(eng, prm, sc, pr, nullptr, hbm_budget, out);
}

int bialign_batch_create_features(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                                  const bialign_pairs* pr, const bialign_features* ft, int64_t hbm_budget,
                                  bialign_batch** out) {
  if (out) *out = nullptr;
  if (!ft) return fail(BIALIGN_E_INVALID, "feat is NULL");
  if (!ft->up_a || !ft->down_a || !ft->unp_a || !ft->up_b || !ft->down_b || !ft->unp_b)
    return fail(BIALIGN_E_INVALID, "a feature array is NULL");
  return create_batch(eng, prm, sc, pr, ft, hbm_budget, out);
}

// bialign_batch_create_null (ft == nullptr), bialign_batch_create_null_features, and bialign_batch_create_null_dense (dense)
static int create_null(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc, const bialign_pairs* pr,
                       const bialign_features* ft, const bialign_null_spec* spec, int64_t hbm_budget, bialign_batch** out,
                       bool dense = false) {
  if (out) *out = nullptr;
  if (!eng || !prm || !sc || !pr || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!spec) return fail(BIALIGN_E_INVALID, "spec is NULL");
  if (spec->replicas < 1 || spec->replicas > 65535)
    return fail(BIALIGN_E_INVALID, "replicas must be 1..65535, got %d", spec->replicas);
  if (pr->npairs < 1) return fail(BIALIGN_E_INVALID, "npairs must be >= 1");
  if ((int64_t)pr->npairs * spec->replicas > INT32_MAX)
    return fail(BIALIGN_E_INVALID, "npairs * replicas = %lld exceeds INT32_MAX", (long long)pr->npairs * spec->replicas);
  if (prm->flags & (BIALIGN_BATCH_LEAN_TRACE | BIALIGN_BATCH_LEVEL_TRACE))
    return fail(BIALIGN_E_INVALID, "a null batch is SCORE_ONLY: LEAN_TRACE / LEVEL_TRACE do not apply");
  if (dense && !pr->mu1_dense && !pr->mu2_dense)
    return fail(BIALIGN_E_INVALID, "neither mu1_dense nor mu2_dense is set: a null batch in LOOKUP form is bialign_batch_create_null's");
  if (dense && pr->mu1_dense && !pr->mu1_off) return fail(BIALIGN_E_INVALID, "mu1_dense given without mu1_off");
  if (dense && pr->mu2_dense && !pr->mu2_off) return fail(BIALIGN_E_INVALID, "mu2_dense given without mu2_off");
  if (!dense && !ft && (pr->mu1_dense || pr->mu2_dense))
    return fail(BIALIGN_E_UNSUPPORTED, "null batches take the LOOKUP form only (a dense table's columns would have to be permuted per replica)");
  if (ft && pr->mu1_dense)  // (mu2_dense is ignored in FEATURE form, as in bialign_batch_create_features)
    return fail(BIALIGN_E_UNSUPPORTED, "FEATURE-form null batches take mu1 in LOOKUP form only (a dense table's columns would have to be permuted per replica)");
  if (!pr->len_a || !pr->len_b || !pr->off_a || !pr->off_b) return fail(BIALIGN_E_INVALID, "len_a / len_b / off_a / off_b are NULL");
  // (DENSE form: the codes of whichever of mu1 / mu2 is in LOOKUP form)
  if (!(dense && pr->mu1_dense) && (!pr->seq_a || !pr->seq_b)) return fail(BIALIGN_E_INVALID, "seq_a / seq_b are NULL (LOOKUP form)");
  if (!ft && !(dense && pr->mu2_dense) && (!pr->cls_a || !pr->cls_b)) return fail(BIALIGN_E_INVALID, "cls_a / cls_b are NULL (LOOKUP form)");
  NullPlan plan{};
  if (int rc = expand_null_pairs(prm, pr, ft, spec->replicas, spec->seed, dense, plan)) return rc;
  return create_batch(eng, &plan.vprm, sc, &plan.vp, ft, hbm_budget, out, &plan);
}

int bialign_batch_create_null(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                              const bialign_pairs* pr, const bialign_null_spec* spec, int64_t hbm_budget, bialign_batch** out) {
  return create_null(eng, prm, sc, pr, nullptr, spec, hbm_budget, out);
}

int bialign_batch_create_null_features(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                                       const bialign_pairs* pr, const bialign_features* ft, const bialign_null_spec* spec,
                                       int64_t hbm_budget, bialign_batch** out) {
  if (out) *out = nullptr;
  if (!ft) return fail(BIALIGN_E_INVALID, "feat is NULL");
  if (!ft->up_a || !ft->down_a || !ft->unp_a || !ft->up_b || !ft->down_b || !ft->unp_b)
    return fail(BIALIGN_E_INVALID, "a feature array is NULL");
  return create_null(eng, prm, sc, pr, ft, spec, hbm_budget, out);
}

int bialign_batch_create_null_dense(bialign_engine* eng, const bialign_params* prm, const bialign_scoring* sc,
                                    const bialign_pairs* pr, const bialign_null_spec* spec, int64_t hbm_budget, bialign_batch** out) {
  return create_null(eng, prm, sc, pr, nullptr, spec, hbm_budget, out, true);
}

void bialign_batch_destroy(bialign_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->eng->device);
  bialign_engine* eng = b->eng;
  if (b->pending) (void)hipStreamSynchronize(b->eng->stream);  // its kernels still use the buffers freed below
  if (b->d_layers.p && !eng->closing) {  // keep the buffer for the next batch: a free slot, else in place of a smaller one
    (void)hipStreamSynchronize(eng->stream);
    DevBuf<int32_t>* slot = !eng->layer_cache.p ? &eng->layer_cache : (!eng->layer_cache2.p ? &eng->layer_cache2 : nullptr);
    if (!slot) slot = eng->layer_cache.n <= eng->layer_cache2.n ? &eng->layer_cache : &eng->layer_cache2;
    if (!slot->p || b->d_layers.n > slot->n) slot->swap(b->d_layers);
  }
  if (b->tab_scratch() && b->d_tab.p && !eng->closing) {  // ... and so the table buffer (the stream is idle here or was never used)
    (void)hipStreamSynchronize(eng->stream);
    if (!eng->tab_cache.p || b->d_tab.n > eng->tab_cache.n) eng->tab_cache.swap(b->d_tab);
  }
  delete b;
  if (--eng->live_batches == 0 && eng->closing) bialign_engine_destroy(eng);
}

int bialign_engine_reserve(bialign_engine* e, int64_t bytes, int tries, double* rate_gbps) {
  if (!e || bytes <= 0) return fail(BIALIGN_E_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(e->device));
  const size_t dwords = ((size_t)bytes + 3) / 4;
  DevBuf<int32_t> best;
  double best_rate = 0;
  if (e->layer_cache.n >= dwords) {  // what is cached is the first candidate
    best.swap(e->layer_cache);
  } else {
    e->layer_cache.release();
    HIP_TRY(best.alloc(dwords));
  }
  int rc = probe_write_rate(e, e->stream, best.p, dwords, &best_rate);
  for (int t = 1; t < tries && rc == BIALIGN_OK; ++t) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (free_b < (size_t)(dwords * 4 * 1.05)) break;  // no room for a second candidate next to the held one
    DevBuf<int32_t> cand;
    if (cand.alloc(dwords) != hipSuccess) { (void)hipGetLastError(); break; }
    double rate = 0;
    rc = probe_write_rate(e, e->stream, cand.p, dwords, &rate);
    if (rc == BIALIGN_OK && rate > best_rate * 1.005) {  // keep the better one; the other goes back
      best.swap(cand);
      best_rate = rate;
    }
  }
  if (rc == BIALIGN_OK) {
    e->layer_cache.swap(best);
    if (rate_gbps) *rate_gbps = best_rate;
  }
  return rc;
}

int bialign_engine_trim(bialign_engine* e) {
  if (!e) return fail(BIALIGN_E_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  e->layer_cache.release();
  e->layer_cache2.release();
  e->tab_cache.release();
  return BIALIGN_OK;
}

int bialign_batch_get_info(const bialign_batch* b, bialign_batch_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  info->npairs = b->null_R ? b->null_npairs : b->npairs;
  info->nchunks = (int)b->chunk_begin.size() - 1;
  info->affine = b->affine;
  info->max_shift = b->S;
  info->cells = b->cells;
  info->layer_bytes = b->cells * 4 * b->NL;
  info->hbm_layer_bytes = b->max_chunk_dwords * 4;
  info->trace_bytes = b->trace_bytes;
  info->storage = b->level_trace ? BIALIGN_BATCH_LEVEL_TRACE : (b->lean_trace ? BIALIGN_BATCH_LEAN_TRACE : (b->lean ? BIALIGN_BATCH_SCORE_ONLY : 0));
  info->reserved = 0;
  return BIALIGN_OK;
}

// Enqueue one run of the batch on the engine's stream (all chunks: fill, then traceback).
static int enqueue_run(bialign_batch* b, uint32_t flags) {
  HIP_TRY(hipSetDevice(b->eng->device));
  const bool do_trace = !(flags & BIALIGN_RUN_FILL_ONLY) && (!b->lean || b->lean_trace || b->level_trace);
  const DeviceBatch v = b->view();
  hipStream_t st = b->eng->stream;
  b->timing = bialign_timing{};
  b->ran = b->ran_trace = false;
  b->used_xcu = b->used_pack = false;
  const int nchunks = (int)b->chunk_begin.size() - 1;
  while ((int)b->evs.size() < 3 * nchunks) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    b->evs.push_back(e);
  }
  while (b->tab_scratch() && (int)b->build_evs.size() < 2 * nchunks) {
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    b->build_evs.push_back(e);
  }
  b->build_ms = 0;
  b->build_launches = 0;
  HIP_TRY(hipStreamWaitEvent(st, b->uploaded, 0));
  HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), st));  // the flag is per run
  if (b->free_ends()) HIP_TRY(hipMemsetAsync(b->d_span.p, 0xff, sizeof(int32_t) * b->d_span.n, st));  // spans: -1 until a kernel writes them
  if (b->end_key())  // keys: zero, below every key a sweep folds in
    HIP_TRY(hipMemsetAsync(b->d_end_key.p, 0, sizeof(unsigned long long) * b->npairs, st));
  b->hits_pending = false;
  if (b->hits_on) {  // hit search: its results are per run, like the spans
    while ((int)b->hit_evs.size() < 2 * nchunks) {
      hipEvent_t e = nullptr;
      HIP_TRY(hipEventCreate(&e));
      b->hit_evs.push_back(e);
    }
    if (int rc = reset_hits(b, st)) return rc;
  }
  if (b->null_R) {  // null batch: the replicas' B codes, all of them ahead of the first sweep (timed on its own, outside fill_ms)
    HIP_TRY(hipEventRecord(b->null_evs[0], st));
    if (int rc = launch_shuffle_null(b, 0, b->npairs)) return rc;
    HIP_TRY(hipEventRecord(b->null_evs[1], st));
  }
  for (int c = 0; c < nchunks; ++c) {  // stream order keeps chunk c's traceback ahead of chunk c+1's sweep
    const int first = b->chunk_begin[c], count = b->chunk_begin[c + 1] - first;
    if (b->tab_scratch()) {
      // FEATURE form: the chunk's mu2 tables, built into the table buffer ahead of the sweep (timed on its own, outside
      // fill_ms).  They stay until the next chunk's build, which stream order puts behind this chunk's tracebacks -- every
      // lean re-sweep round included -- so no round has to build them again.  DENSE-form null batch: the chunk's
      // replicas' tables, the real pairs' with their columns permuted, in the same slot.
      HIP_TRY(hipEventRecord(b->build_evs[2 * c], st));
      if (int rc = b->null_dense ? launch_permute_tables(b, first, count) : launch_build_mu2(b, first, count)) return rc;
      HIP_TRY(hipEventRecord(b->build_evs[2 * c + 1], st));
      ++b->build_launches;
    }
    HIP_TRY(hipEventRecord(b->evs[3 * c], st));
    int rc = launch_fill(b, v, first, count);
    if (rc == BIALIGN_OK && b->end_key()) rc = launch_end_key_finish(b, v, first, count);  // scores and ends (local: in every storage mode)
    if (rc) return rc;
    HIP_TRY(hipEventRecord(b->evs[3 * c + 1], st));
    if (!b->lean) {  // (with LEAN records the sweep itself wrote the scores)
      rc = launch_traceback(b, v, first, count, do_trace);
      if (rc) return rc;
    } else if (b->lean_trace && do_trace) {
      rc = lean_traceback_rounds(b, v, first, count);
      if (rc) return rc;
    } else if (b->level_trace && do_trace) {
      rc = level_traceback_rounds(b, v, first, count);
      if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(b->evs[3 * c + 2], st));
    if (b->hits_on) {  // behind the chunk's traceback, ahead of the next chunk's sweep: the layers are still the chunk's
      HIP_TRY(hipEventRecord(b->hit_evs[2 * c], st));
      if (int rc2 = launch_fit_hits(b, v, hit_args(b, do_trace), first, count)) return rc2;
      HIP_TRY(hipEventRecord(b->hit_evs[2 * c + 1], st));
      b->hits_pending = true;
    }
    b->timing.fill_launches += 1;
    b->timing.traceback_launches += 1;
    b->timing.waves_per_pair = std::abs(b->last_team);
    b->timing.cross_cu = b->last_team < 0;
  }
  b->pending = true;
  b->pending_trace = do_trace;
  b->pending_flags = flags;
  return BIALIGN_OK;
}

int bialign_batch_wait(bialign_batch* b) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  if (!b->pending) return BIALIGN_OK;
  HIP_TRY(hipSetDevice(b->eng->device));
  for (;;) {
    b->pending = false;
    const int nchunks = (int)b->chunk_begin.size() - 1;
    HIP_TRY(hipEventSynchronize(b->evs[3 * nchunks - 1]));  // (a re-planned batch may have fewer chunks than events)
    for (int c = 0; c < nchunks; ++c) {
      float f = 0, t = 0;
      HIP_TRY(hipEventElapsedTime(&f, b->evs[3 * c], b->evs[3 * c + 1]));
      HIP_TRY(hipEventElapsedTime(&t, b->evs[3 * c + 1], b->evs[3 * c + 2]));
      b->timing.fill_ms += f;
      b->timing.traceback_ms += t;
      if (b->tab_scratch()) {
        HIP_TRY(hipEventElapsedTime(&f, b->build_evs[2 * c], b->build_evs[2 * c + 1]));
        b->build_ms += f;
      }
    }
    if (b->null_R) {
      float f = 0;
      HIP_TRY(hipEventElapsedTime(&f, b->null_evs[0], b->null_evs[1]));
      b->shuffle_ms = f;
    }
    if (b->hits_pending) {  // the last chunk's search lies behind the event waited for above
      HIP_TRY(hipEventSynchronize(b->hit_evs[2 * nchunks - 1]));
      b->search_ms = 0;
      for (int c = 0; c < nchunks; ++c) {
        float f = 0;
        HIP_TRY(hipEventElapsedTime(&f, b->hit_evs[2 * c], b->hit_evs[2 * c + 1]));
        b->search_ms += f;
      }
    }
    int32_t err = 0;
    HIP_TRY(hipMemcpy(&err, b->d_err.p, sizeof err, hipMemcpyDeviceToHost));
    if (!err) break;
    // Bit 1: a cross-CU team lost co-residency (its waves spin on partners that were never scheduled:
    // another tenant holds wave slots) -- the run is repeated with in-workgroup teams, which depend on
    // nobody.  Bit 2: a packed record met a value that does not fit its 16-bit offset -- the run is
    // repeated with full records.  Either way the batch stays on the safe form.
    bool again = false;
    if (err & 1) {
      if (!b->used_xcu || b->no_xcu)
        return fail(BIALIGN_E_DEVICE, "fill kernel: team hand-off timed out (device error flag %d)", err);
      b->no_xcu = again = true;
    }
    if (err & 2) {
      if (!b->used_pack || b->pack_failed)
        return fail(BIALIGN_E_DEVICE, "fill kernel: device error flag %d", err);
      b->pack_failed = again = true;
      if (int rc = replan_full(b)) return rc;
    }
    if (!again) return fail(BIALIGN_E_DEVICE, "fill kernel: device error flag %d", err);
    ++b->recovered;
    if (int rc = enqueue_run(b, b->pending_flags)) return rc;
  }
  b->timing.recovered_runs = b->recovered;
  b->timing.packed_records = b->used_pack ? 1 : 0;
  b->ran = true;
  b->ran_trace = b->pending_trace;
  b->hits_ran = b->hits_pending;
  return BIALIGN_OK;
}

int bialign_batch_run(bialign_batch* b, uint32_t flags) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  int rc = bialign_batch_wait(b);  // one run of a batch at a time
  if (rc) return rc;
  rc = enqueue_run(b, flags);
  if (rc) return rc;
  return (flags & BIALIGN_RUN_ASYNC) ? BIALIGN_OK : bialign_batch_wait(b);
}

int bialign_batch_get_timing(const bialign_batch* b, bialign_timing* t) {
  if (!b || !t) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  *t = b->timing;
  return BIALIGN_OK;
}

int bialign_batch_get_scores(const bialign_batch* b, int32_t* scores) {
  if (!b || !scores) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (b->null_R) return fail(BIALIGN_E_INVALID, "a null batch has no observed scores: use bialign_batch_get_null_scores / _get_null_stats");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called");
  HIP_TRY(hipSetDevice(b->eng->device));
  HIP_TRY(hipMemcpy(scores, b->d_scores.p, sizeof(int32_t) * b->npairs, hipMemcpyDeviceToHost));
  return BIALIGN_OK;
}

// The spans of a batch of mode `mode`: the first `cols` columns of d_span's rows, scattered into out[0 .. cols)
static int read_spans(const bialign_batch* b, bialign::AlignMode mode, const char* no_mode, int cols, int32_t* const* out) {
  if (!b || std::count(out, out + cols, nullptr)) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (b->mode != mode) return fail(BIALIGN_E_INVALID, "%s", no_mode);
  if (b->null_R) return fail(BIALIGN_E_INVALID, "a null batch has no observed alignments: no spans");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called");
  HIP_TRY(hipSetDevice(b->eng->device));
  std::vector<int32_t> span((size_t)cols * b->npairs);
  HIP_TRY(hipMemcpy(span.data(), b->d_span.p, sizeof(int32_t) * span.size(), hipMemcpyDeviceToHost));
  for (size_t t = 0; t < span.size(); ++t) out[t % cols][t / cols] = span[t];
  return BIALIGN_OK;
}

int bialign_batch_get_fit_spans(const bialign_batch* b, int32_t* start_b, int32_t* end_b) {
  int32_t* const out[] = {start_b, end_b};
  return read_spans(b, bialign::AlignMode::Fit, "batch was created without BIALIGN_BATCH_FIT: it has no spans", 2, out);
}

int bialign_batch_get_local_spans(const bialign_batch* b, int32_t* start_a, int32_t* end_a, int32_t* start_b, int32_t* end_b) {
  int32_t* const out[] = {start_a, end_a, start_b, end_b};
  return read_spans(b, bialign::AlignMode::Local, "batch was created without BIALIGN_BATCH_LOCAL: it has no local spans", 4, out);
}

int bialign_batch_get_overlap_spans(const bialign_batch* b, int32_t* start_a, int32_t* end_a, int32_t* start_b, int32_t* end_b) {
  int32_t* const out[] = {start_a, end_a, start_b, end_b};
  return read_spans(b, bialign::AlignMode::Overlap, "batch was created without BIALIGN_BATCH_OVERLAP: it has no overlap spans", 4, out);
}

int bialign_batch_get_traces(const bialign_batch* b, uint8_t* trace, int64_t* trace_off, int32_t* trace_len,
                             int32_t* complete) {
  if (!b || !trace || !trace_off || !trace_len || !complete) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (b->lean && !b->lean_trace && !b->level_trace)
    return fail(BIALIGN_E_INVALID, "batch was created with BIALIGN_BATCH_SCORE_ONLY: it holds no layers to trace back");
  if (!b->ran || !b->ran_trace) return fail(BIALIGN_E_INVALID, "no traceback has been run on this batch");
  HIP_TRY(hipSetDevice(b->eng->device));
  HIP_TRY(hipMemcpy(trace, b->d_trace.p, b->trace_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(trace_len, b->d_tlen.p, sizeof(int32_t) * b->npairs, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(complete, b->d_complete.p, sizeof(int32_t) * b->npairs, hipMemcpyDeviceToHost));
  for (int p = 0; p < b->npairs; ++p) trace_off[p] = b->pairs[p].trace_off;
  return BIALIGN_OK;
}

int bialign_batch_set_hits(bialign_batch* b, const bialign_hit_spec* spec) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  if (int rc = bialign_batch_wait(b)) return rc;  // a pending run still writes the buffers released below
  HIP_TRY(hipSetDevice(b->eng->device));
  b->release_hits();
  if (!spec) return BIALIGN_OK;
  if (b->mode != bialign::AlignMode::Fit || b->lean || b->null_R)
    return fail(BIALIGN_E_UNSUPPORTED, "the hit search needs a FIT batch in full storage (not %s)",
                b->null_R ? "a null batch" : (b->mode != bialign::AlignMode::Fit ? "a batch without BIALIGN_BATCH_FIT" : "SCORE_ONLY"));
  if (spec->max_hits < 1 || spec->max_hits > 256) return fail(BIALIGN_E_INVALID, "max_hits must be 1..256, got %d", spec->max_hits);
  if (spec->min_score < 1) return fail(BIALIGN_E_INVALID, "min_score must be >= 1, got %d", spec->min_score);
  if (spec->max_walks != 0 && spec->max_walks < spec->max_hits)
    return fail(BIALIGN_E_INVALID, "max_walks must be 0 (4 * max_hits) or >= max_hits = %d, got %d", spec->max_hits, spec->max_walks);
  if (spec->reserved != 0) return fail(BIALIGN_E_INVALID, "bialign_hit_spec.reserved must be 0");
  bialign_hit_spec sp = *spec;
  if (sp.max_walks == 0) sp.max_walks = 4 * sp.max_hits;
  int max_m = 0;
  b->hit_prof_off.assign((size_t)b->npairs + 1, 0);
  for (int p = 0; p < b->npairs; ++p) {
    max_m = std::max(max_m, b->pairs[p].m);
    b->hit_prof_off[p + 1] = b->hit_prof_off[p] + b->pairs[p].m + 1;
  }
  b->hit_spec = sp;
  b->hit_mask_words = (max_m + 32) >> 5;
  const size_t lds = fit_hits_lds(hit_args(b, true));
  if (lds > 160 * 1024)
    return fail(BIALIGN_E_UNSUPPORTED, "the hit search's mask, spans and staged inputs need %zu bytes of LDS (160 KiB at most)", lds);
  const size_t prof = (size_t)b->hit_prof_off.back(), recs = (size_t)b->npairs * sp.max_hits * 4,
               walks = (size_t)b->npairs * sp.max_walks * 4, trace = (size_t)sp.max_hits * (size_t)b->trace_bytes;
  hipStream_t st = b->eng->stream;
  hipError_t err = b->d_hit_profile.alloc(prof);
  if (err == hipSuccess) err = b->d_hit_head.alloc(4 * (size_t)b->npairs);
  if (err == hipSuccess) err = b->d_hit_rec.alloc(recs);
  if (err == hipSuccess) err = b->d_hit_walks.alloc(walks);
  if (err == hipSuccess) err = b->d_hit_trace.alloc(trace);
  if (err == hipSuccess) err = b->d_hit_prof_off.upload(b->hit_prof_off.data(), (size_t)b->npairs, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err == hipSuccess && getenv("BIALIGN_TEST_FAIL_HITS_ALLOC")) err = hipErrorOutOfMemory;  // tests: pretend an allocation failed
  if (err != hipSuccess) {
    (void)hipGetLastError();
    b->release_hits();
    return fail(BIALIGN_E_NOMEM, "hit search: allocating %zu bytes of result buffers failed: %s",
                (prof + 4 * (size_t)b->npairs + recs + walks) * 4 + trace, hipGetErrorString(err));
  }
  b->hit_bytes = (int64_t)((prof + 4 * (size_t)b->npairs + recs + walks) * 4 + trace + (size_t)b->npairs * 8);
  b->hits_on = true;
  b->search_ms = 0;
  return BIALIGN_OK;
}

int bialign_batch_get_hit_profile(const bialign_batch* b, int32_t pair, int32_t* out) {
  if (!out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = hits_ready(b)) return rc;
  if (pair < 0 || pair >= b->npairs) return fail(BIALIGN_E_INVALID, "pair %d out of range", pair);
  HIP_TRY(hipMemcpy(out, b->d_hit_profile.p + b->hit_prof_off[pair], sizeof(int32_t) * (b->pairs[pair].m + 1), hipMemcpyDeviceToHost));
  return BIALIGN_OK;
}

int bialign_batch_get_hits(const bialign_batch* b, int32_t* nhits, int32_t* status, int32_t* start_b, int32_t* end_b,
                           int32_t* score, int32_t* trace_len, uint8_t* trace, int64_t* trace_off) {
  if (!nhits || !status || !start_b || !end_b || !score || !trace_len || !trace != !trace_off) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = hits_ready(b)) return rc;
  const int K = b->hit_spec.max_hits;
  std::vector<int32_t> head(4 * (size_t)b->npairs), rec((size_t)b->npairs * K * 4);
  HIP_TRY(hipMemcpy(head.data(), b->d_hit_head.p, sizeof(int32_t) * head.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rec.data(), b->d_hit_rec.p, sizeof(int32_t) * rec.size(), hipMemcpyDeviceToHost));
  if (trace) HIP_TRY(hipMemcpy(trace, b->d_hit_trace.p, (size_t)K * b->trace_bytes, hipMemcpyDeviceToHost));
  for (int p = 0; p < b->npairs; ++p) {
    nhits[p] = head[4 * (size_t)p], status[p] = head[4 * (size_t)p + 2];
    for (int h = 0; h < K; ++h) {
      const size_t t = (size_t)p * K + h;
      start_b[t] = rec[4 * t], end_b[t] = rec[4 * t + 1], score[t] = rec[4 * t + 2], trace_len[t] = rec[4 * t + 3];
      if (trace_off) trace_off[t] = (int64_t)K * b->pairs[p].trace_off + (int64_t)h * b->pairs[p].trace_cap;
    }
  }
  return BIALIGN_OK;
}

int bialign_batch_get_hit_walks(const bialign_batch* b, int32_t* nwalks, int32_t* end_b, int32_t* start_b, int32_t* score,
                                int32_t* accepted) {
  if (!nwalks || !end_b || !start_b || !score || !accepted) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = hits_ready(b)) return rc;
  const int K = b->hit_spec.max_walks;
  std::vector<int32_t> head(4 * (size_t)b->npairs), rec((size_t)b->npairs * K * 4);
  HIP_TRY(hipMemcpy(head.data(), b->d_hit_head.p, sizeof(int32_t) * head.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rec.data(), b->d_hit_walks.p, sizeof(int32_t) * rec.size(), hipMemcpyDeviceToHost));
  for (int p = 0; p < b->npairs; ++p) {
    nwalks[p] = head[4 * (size_t)p + 1];
    for (int h = 0; h < K; ++h) {
      const size_t t = (size_t)p * K + h;
      end_b[t] = rec[4 * t], start_b[t] = rec[4 * t + 1], score[t] = rec[4 * t + 2], accepted[t] = rec[4 * t + 3];
    }
  }
  return BIALIGN_OK;
}

int bialign_batch_get_hit_info(const bialign_batch* b, bialign_hit_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->hits_on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  info->spec = b->hit_spec;
  info->buffer_bytes = b->hit_bytes;
  info->search_ms = b->hits_ran ? b->search_ms : 0;
  return BIALIGN_OK;
}

int bialign_batch_dump_layers(bialign_batch* b, int32_t pair, int32_t* out) {
  if (!b || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (pair < 0 || pair >= b->npairs) return fail(BIALIGN_E_INVALID, "pair %d out of range", pair);
  if (int rc = bialign_batch_wait(b)) return rc;
  if (b->lean) return fail(BIALIGN_E_INVALID, "batch was created with reduced layer storage (SCORE_ONLY / LEAN_TRACE / LEVEL_TRACE): it holds no full layers");
  HIP_TRY(hipSetDevice(b->eng->device));
  hipStream_t st = b->eng->stream;
  // one-pair launch out of the regular launch order (team shape and layer offset are the pair's own)
  int pos = (int)(std::find(b->order.begin(), b->order.end(), pair) - b->order.begin());
  DeviceBatch v = b->view();
  HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), st));
  b->used_xcu = b->used_pack = false;
  int rc = launch_build_mu2(b, pos, 1);  // FEATURE form: the table buffer may hold another chunk's tables by now
  if (rc == BIALIGN_OK) rc = launch_fill(b, v, pos, 1);
  if (rc) return rc;
  if ((b->used_xcu && !b->no_xcu) || (b->used_pack && !b->pack_failed)) {  // forms a launch can fall back from, as in a run
    HIP_TRY(hipStreamSynchronize(st));
    int32_t err = 0;
    HIP_TRY(hipMemcpy(&err, b->d_err.p, sizeof err, hipMemcpyDeviceToHost));
    if (err) {
      if (err & 1) b->no_xcu = true;
      if (err & 2) {
        b->pack_failed = true;
        if (int rc2 = replan_full(b)) return rc2;
        // the re-plan sorts every chunk's launch order anew, moves every pair's layer_off and may have replaced
        // the layer buffer: the pair's launch position and the device view are the new ones from here on
        v = b->view();
        pos = (int)(std::find(b->order.begin(), b->order.end(), pair) - b->order.begin());
      }
      ++b->recovered;
      HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), st));
      rc = launch_build_mu2(b, pos, 1);  // (a re-plan moved the pair's table)
      if (rc == BIALIGN_OK) rc = launch_fill(b, v, pos, 1);
      if (rc) return rc;
    }
  }
  const PairDesc& d = b->pairs[pair];
  const int W = 2 * b->S + 1;
  const size_t elems = (size_t)b->NL * (d.n + 1) * (d.m + 1) * W * W;
  DevBuf<int32_t> d_out;
  HIP_TRY(d_out.alloc(elems));
  rc = launch_dump_any(b, v, pair, d_out.p);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out.p, elems * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // scores and traces live in their own buffers and stay valid; only the layer region was rewritten
  return check_device_error(b);
}

int bialign_batch_dump_mu2(bialign_batch* b, int32_t pair, int32_t* out) {
  if (!b || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (b->null_R)
    return fail(BIALIGN_E_INVALID, "a null batch has no table of a real pair to dump: its tables are those of the replicas "
                                   "(bialign_batch_dump_null_features shows what they are built from, "
                                   "bialign_batch_dump_null_tables a DENSE-form null batch's)");
  if (pair < 0 || pair >= b->npairs) return fail(BIALIGN_E_INVALID, "pair %d out of range", pair);
  if (!b->dense) return fail(BIALIGN_E_INVALID, "mu2 of this batch is in LOOKUP form: there is no table to dump");
  if (int rc = bialign_batch_wait(b)) return rc;
  HIP_TRY(hipSetDevice(b->eng->device));
  hipStream_t st = b->eng->stream;
  HIP_TRY(hipStreamWaitEvent(st, b->uploaded, 0));
  if (b->feat) {  // build the pair's table in its place in the chunk buffer (results of a run live elsewhere)
    const int pos = (int)(std::find(b->order.begin(), b->order.end(), pair) - b->order.begin());
    if (int rc = launch_build_mu2(b, pos, 1)) return rc;
  }
  const PairDesc& d = b->pairs[pair];
  HIP_TRY(hipMemcpyAsync(out, b->d_tab.p + d.tab_off, (size_t)d.n * d.m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

int bialign_batch_get_feature_info(const bialign_batch* b, bialign_feature_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  info->form = b->feat ? BIALIGN_MU2_FEATURE : (b->dense ? BIALIGN_MU2_DENSE : BIALIGN_MU2_LOOKUP);
  info->build_launches = b->build_launches;
  int64_t dense_dw = 0;  // DENSE: every pair's mu2 table is resident
  if (b->dense && !b->tab_scratch())
    for (const PairDesc& d : b->pairs) dense_dw += (int64_t)d.n * d.m;
  info->table_bytes = 4 * (b->tab_scratch() ? b->max_chunk_tab_dwords : dense_dw);
  info->build_ms = b->build_ms;
  return BIALIGN_OK;
}

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
  if (observed) HIP_TRY(b->d_null_obs.upload(observed, (size_t)b->null_npairs, st));
  HIP_TRY(hipEventRecord(b->null_evs[2], st));
  if (int rc = launch_null_stats(b, observed ? b->d_null_obs.p : nullptr)) return rc;
  HIP_TRY(hipEventRecord(b->null_evs[3], st));
  HIP_TRY(hipMemcpyAsync(out, b->d_null_stats.p, sizeof(bialign_null_stats) * b->null_npairs, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float f = 0;
  HIP_TRY(hipEventElapsedTime(&f, b->null_evs[2], b->null_evs[3]));
  b->stats_ms = f;
  return BIALIGN_OK;
}

int bialign_batch_get_null_info(const bialign_batch* b, bialign_null_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  info->shuffle_ms = b->shuffle_ms;
  info->stats_ms = b->stats_ms;
  info->replica_bytes = (int64_t)(b->d_seq_b.n + b->d_cls_b.n + (b->feat ? b->d_feat_b.n * sizeof(double) : 0) +
                                  b->d_null_perm.n * sizeof(uint16_t));
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
  b->null_model = model;
  return BIALIGN_OK;
}

int bialign_batch_get_null_model(const bialign_batch* b, int32_t* model) {
  if (!b || !model) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (!b->null_R) return fail(BIALIGN_E_INVALID, "not a null batch (bialign_batch_create_null)");
  *model = b->null_model;
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
    HIP_TRY(hipMemcpyAsync(out[f], b->d_feat_b.p + (size_t)f * b->feat_tot_b + d.seq_b, (size_t)d.m * sizeof(double),
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
  if (mu2_out) HIP_TRY(hipMemcpyAsync(mu2_out, b->d_tab.p + d.tab_off, nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (mu1_out)
    HIP_TRY(hipMemcpyAsync(mu1_out, b->d_tab.p + d.tab_off + (b->dense ? nm : 0), nm * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

}  // extern "C"
