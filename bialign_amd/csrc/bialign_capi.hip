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
  if (int rc = replan_full_layout(*b, (int64_t)b->d_layers.n - 16, (int64_t)b->tables.d_tab.n)) return rc;
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
  if (b->feat) HIP_TRY(b->tables.d_feat_b.alloc(3 * (size_t)b->tot_b));  // ... and so the replicas' three planes of features
  if (b->null_dense) {  // ... the replicas' permutations, and the real pairs' tables, which stay resident
    HIP_TRY(b->null.d_perm.alloc((size_t)b->tot_b));
    size_t real_dw = 0;
    for (int p = 0; p < b->npairs; p += b->null_R) real_dw += (size_t)b->tab_dwords[p];
    HIP_TRY(b->null.d_tab.alloc(real_dw));
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
    b->tables.d_tab.swap(eng->tab_cache);
  } else {
    eng->tab_cache.release();
    if (b->tables.d_tab.alloc(tab_dw) != hipSuccess) {
      const hipError_t err = hipGetLastError();
      b->tables.d_tab.p = nullptr;
      b->tables.d_tab.n = 0;
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
    else HIP_TRY(b->null.d_seq.upload(nul->seq_b, (size_t)nul->tot_b, st));
    if (b->dense)  // (FEATURE form too: no classes)
      HIP_TRY(hipMemsetAsync(b->d_cls_b.p, 0, std::max<size_t>((size_t)tot_b, 1), st));
    else
      HIP_TRY(b->null.d_cls.upload(nul->cls_b, (size_t)nul->tot_b, st));
    HIP_TRY(b->null.d_off.upload(nul->off_b, (size_t)nul->npairs, st));
    HIP_TRY(b->null.d_stats.alloc((size_t)nul->npairs));
  } else {
    HIP_TRY(b->d_seq_b.upload(b->dense1 ? zeros.data() : pr->seq_b, tot_b, st));
    HIP_TRY(b->d_cls_b.upload(b->dense ? zeros.data() : pr->cls_b, tot_b, st));
  }
  std::vector<int32_t> tabs;
  std::vector<int64_t> mu1_offs;
  if (b->feat) {  // the molecules' features, three planes per side; a dense mu1's tables resident, pair after pair
    b->tables.feat_tot_a = tot_a;
    b->tables.feat_tot_b = tot_b;
    const double* src_a[3] = {ft->up_a, ft->down_a, ft->unp_a};
    const double* src_b[3] = {ft->up_b, ft->down_b, ft->unp_b};
    HIP_TRY(b->tables.d_feat_a.alloc(3 * (size_t)tot_a));
    // null batch: d_feat_b is the replica planes (allocated above, filled by the shuffle kernel); B's own go beside null.d_seq
    DevBuf<double>& up_b = nul ? b->null.d_feat : b->tables.d_feat_b;
    const int64_t src_tot_b = nul ? nul->tot_b : tot_b;
    HIP_TRY(up_b.alloc(3 * (size_t)src_tot_b));
    for (int f = 0; f < 3; ++f) {
      HIP_TRY(hipMemcpyAsync(b->tables.d_feat_a.p + (size_t)f * tot_a, src_a[f], (size_t)tot_a * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(up_b.p + (size_t)f * src_tot_b, src_b[f], (size_t)src_tot_b * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (b->dense1) {
      mu1_offs.resize(pr->npairs);
      size_t tot1 = 0;
      for (int p = 0; p < pr->npairs; ++p) mu1_offs[p] = (int64_t)tot1, tot1 += (size_t)pr->len_a[p] * pr->len_b[p];
      tabs.resize(tot1);
      for (int p = 0; p < pr->npairs; ++p)
        std::memcpy(tabs.data() + mu1_offs[p], pr->mu1_dense + pr->mu1_off[p], (size_t)pr->len_a[p] * pr->len_b[p] * sizeof(int32_t));
      HIP_TRY(b->tables.d_mu1.upload(tabs.data(), tabs.size(), st));
      HIP_TRY(b->tables.d_mu1_off.upload(mu1_offs.data(), mu1_offs.size(), st));
    }
  } else if (b->null_dense) {  // the REAL pairs' tables end to end, mu2's, then mu1's; every replica's are made from them per chunk
    const int R = nul->replicas;
    std::vector<int64_t> offs((size_t)nul->npairs);
    tabs.resize(b->null.d_tab.n);
    int64_t at = 0;
    for (int p = 0; p < nul->npairs; ++p) {
      const size_t v = (size_t)p * R, nm = (size_t)pr->len_a[v] * pr->len_b[v];
      offs[p] = at;
      if (b->dense) std::memcpy(tabs.data() + at, pr->mu2_dense + pr->mu2_off[v], nm * sizeof(int32_t)), at += (int64_t)nm;
      if (b->dense1) std::memcpy(tabs.data() + at, pr->mu1_dense + pr->mu1_off[v], nm * sizeof(int32_t)), at += (int64_t)nm;
    }
    if (!tabs.empty()) HIP_TRY(hipMemcpyAsync(b->null.d_tab.p, tabs.data(), tabs.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(b->null.d_tab_off.upload(offs.data(), offs.size(), st));
  } else if (b->dense || b->dense1) {  // the pairs' tables end to end (PairDesc::tab_off): mu2's, then mu1's
    tabs.resize((size_t)tot_tab);
    for (int p = 0; p < pr->npairs; ++p) {
      const size_t nm = (size_t)pr->len_a[p] * pr->len_b[p];
      int32_t* dst = tabs.data() + b->pairs[p].tab_off;
      if (b->dense) std::memcpy(dst, pr->mu2_dense + pr->mu2_off[p], nm * sizeof(int32_t)), dst += nm;
      if (b->dense1) std::memcpy(dst, pr->mu1_dense + pr->mu1_off[p], nm * sizeof(int32_t));
    }
    HIP_TRY(b->tables.d_tab.upload(tabs.data(), tabs.size(), st));
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
  if (b->tab_scratch() && b->tables.d_tab.p && !eng->closing) {  // ... and so the table buffer (the stream is idle here or was never used)
    (void)hipStreamSynchronize(eng->stream);
    if (!eng->tab_cache.p || b->tables.d_tab.n > eng->tab_cache.n) eng->tab_cache.swap(b->tables.d_tab);
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

// How a run walks back, decided once per run.  Full records: the traceback kernel, which on a fill-only run reads the
// scores alone.  LEAN records: the sweep itself wrote the scores, and only the round forms walk.
enum class TraceForm { Kernel, LeanRounds, LevelRounds, None };
static TraceForm trace_form(const bialign_batch* b, uint32_t flags) {
  if (!b->lean) return TraceForm::Kernel;
  if (flags & BIALIGN_RUN_FILL_ONLY) return TraceForm::None;
  return b->lean_trace ? TraceForm::LeanRounds : (b->level_trace ? TraceForm::LevelRounds : TraceForm::None);
}

// One chunk of a run, stage by stage: tables, fill, traceback, hits.  Stream order keeps it ahead of the next chunk's.
static int run_chunk(bialign_batch* b, const DeviceBatch& v, int c, TraceForm form, bool do_trace) {
  const int first = b->chunk_begin[c], count = b->chunk_begin[c + 1] - first;
  hipStream_t st = b->eng->stream;
  StageClock& clk = b->clock;
  if (b->tab_scratch()) {
    // FEATURE form: the chunk's mu2 tables, built into the table buffer ahead of the sweep (timed on its own, outside
    // fill_ms).  They stay until the next chunk's build, which stream order puts behind this chunk's tracebacks -- every
    // lean re-sweep round included -- so no round has to build them again.  DENSE-form null batch: the chunk's
    // replicas' tables, the real pairs' with their columns permuted, in the same slot.
    HIP_TRY(clk.mark(st));
    if (int rc = b->null_dense ? launch_permute_tables(b, first, count) : launch_build_mu2(b, first, count)) return rc;
    HIP_TRY(clk.mark(st, Stage::Tables));
    ++b->tables.build_launches;
  }
  HIP_TRY(clk.mark(st));
  int rc = launch_fill(b, v, first, count);
  if (rc == BIALIGN_OK && b->end_key()) rc = launch_end_key_finish(b, v, first, count);  // scores and ends (local: in every storage mode)
  if (rc) return rc;
  HIP_TRY(clk.mark(st, Stage::Fill));
  switch (form) {
    case TraceForm::Kernel: rc = launch_traceback(b, v, first, count, do_trace); break;
    case TraceForm::LeanRounds: rc = lean_traceback_rounds(b, v, first, count); break;
    case TraceForm::LevelRounds: rc = level_traceback_rounds(b, v, first, count); break;
    case TraceForm::None: break;
  }
  if (rc) return rc;
  HIP_TRY(clk.mark(st, Stage::Traceback));  // (it began at the fill's end)
  if (b->hits.on) {  // behind the chunk's traceback, ahead of the next chunk's sweep: the layers are still the chunk's
    HIP_TRY(clk.mark(st));
    if (int rc2 = launch_fit_hits(b, v, hit_args(b, do_trace), first, count)) return rc2;
    HIP_TRY(clk.mark(st, Stage::Hits));
  }
  b->timing.fill_launches += 1;
  b->timing.traceback_launches += 1;
  b->timing.waves_per_pair = std::abs(b->last_team);
  b->timing.cross_cu = b->last_team < 0;
  return BIALIGN_OK;
}

// Enqueue one run of the batch on the engine's stream: what is per run, then every chunk.
static int enqueue_run(bialign_batch* b, uint32_t flags) {
  HIP_TRY(hipSetDevice(b->eng->device));
  const TraceForm form = trace_form(b, flags);
  const bool do_trace = !(flags & BIALIGN_RUN_FILL_ONLY) && form != TraceForm::None;  // a trace is walked and written
  const DeviceBatch v = b->view();
  hipStream_t st = b->eng->stream;
  b->timing = bialign_timing{};
  b->clock.reset();
  b->ran = b->ran_trace = false;
  b->used_xcu = b->used_pack = false;
  b->hits.pending = b->hits.on;  // every chunk's search follows its traceback
  b->tables.build_launches = 0;
  HIP_TRY(hipStreamWaitEvent(st, b->uploaded, 0));
  HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), st));  // the flag is per run
  if (b->free_ends()) HIP_TRY(hipMemsetAsync(b->d_span.p, 0xff, sizeof(int32_t) * b->d_span.n, st));  // spans: -1 until a kernel writes them
  if (b->end_key())  // keys: zero, below every key a sweep folds in
    HIP_TRY(hipMemsetAsync(b->d_end_key.p, 0, sizeof(unsigned long long) * b->npairs, st));
  if (b->hits.on)  // hit search: its results are per run, like the spans
    if (int rc = reset_hits(b, st)) return rc;
  if (b->null_R) {  // null batch: the replicas' B codes, all of them ahead of the first sweep (timed on its own, outside fill_ms)
    HIP_TRY(b->clock.mark(st));
    if (int rc = launch_shuffle_null(b, 0, b->npairs)) return rc;
    HIP_TRY(b->clock.mark(st, Stage::Shuffle));
  }
  for (int c = 0; c + 1 < (int)b->chunk_begin.size(); ++c)
    if (int rc = run_chunk(b, v, c, form, do_trace)) return rc;
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
    HIP_TRY(b->clock.finish());
    b->timing.fill_ms = b->clock.ms(Stage::Fill);
    b->timing.traceback_ms = b->clock.ms(Stage::Traceback);
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
  b->hits.ran = b->hits.pending;
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
  HIP_TRY(hipMemcpyAsync(out, b->tables.d_tab.p + d.tab_off, (size_t)d.n * d.m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return BIALIGN_OK;
}

int bialign_batch_get_feature_info(const bialign_batch* b, bialign_feature_info* info) {
  if (!b || !info) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  info->form = b->feat ? BIALIGN_MU2_FEATURE : (b->dense ? BIALIGN_MU2_DENSE : BIALIGN_MU2_LOOKUP);
  info->build_launches = b->tables.build_launches;
  int64_t dense_dw = 0;  // DENSE: every pair's mu2 table is resident
  if (b->dense && !b->tab_scratch())
    for (const PairDesc& d : b->pairs) dense_dw += (int64_t)d.n * d.m;
  info->table_bytes = 4 * (b->tab_scratch() ? b->max_chunk_tab_dwords : dense_dw);
  info->build_ms = b->clock.ms(Stage::Tables);
  return BIALIGN_OK;
}

}  // extern "C"
