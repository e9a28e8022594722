// bialign_hits.hip -- the hit-search kernels of FIT batches (bialign_hits.hpp), instantiated as the generic tracebacks
// are: max_shift 0..5, affine and one-layer, packed records (affine, max_shift 1..BIALIGN_MAX_SHIFT_PACKED), dense mu1;
// each without and with the search's options (OPT); and the search's C entry points (include/bialign.h).
#include "bialign_hits.hpp"

namespace bialign {

namespace {

template <int S, bool AFFINE, bool PACK, bool D1>
int launch_one(const bialign_batch* b, const DeviceBatch& v, const HitArgs& h, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  if (h.options())
    return launch(fit_hits_kernel<S, AFFINE, PACK, D1, true>, dim3(count), dim3(64), fit_hits_lds(h), b->eng->stream, w, h, count);
  return launch(fit_hits_kernel<S, AFFINE, PACK, D1, false>, dim3(count), dim3(64), fit_hits_lds(h), b->eng->stream, w, h, count);
}

template <int S>
int launch_s(const bialign_batch* b, const DeviceBatch& v, const HitArgs& h, int first, int count) {
  if (!b->affine)
    return b->dense1 ? launch_one<S, false, false, true>(b, v, h, first, count) : launch_one<S, false, false, false>(b, v, h, first, count);
  if (b->dense1) return launch_one<S, true, false, true>(b, v, h, first, count);
  if constexpr (S >= 1 && S <= BIALIGN_MAX_SHIFT_PACKED) {
    if (b->packed_layers) return launch_one<S, true, true, false>(b, v, h, first, count);
  }
  if (b->packed_layers) return fail(BIALIGN_E_UNSUPPORTED, "no hit search over packed records at max_shift %d", S);
  return launch_one<S, true, false, false>(b, v, h, first, count);
}

}  // namespace

int launch_fit_hits(const bialign_batch* b, const DeviceBatch& v, const HitArgs& h, int first, int count) {
  switch (b->S) {
#define BIALIGN_HITS_CASE(S, X) \
  case S: return launch_s<S>(b, v, h, first, count);
    BIALIGN_FOR_EACH_S(BIALIGN_HITS_CASE, )
#undef BIALIGN_HITS_CASE
  }
  return fail(BIALIGN_E_UNSUPPORTED, "no hit search kernel for max_shift %d", b->S);
}

// ---- hit search (bialign_hits.hpp): what a launch is given, and the state its results have ahead of a run
HitArgs hit_args(const bialign_batch* b, bool search) {
  HitArgs h{};
  h.max_hits = b->hits.spec.max_hits, h.max_walks = b->hits.spec.max_walks, h.min_score = b->hits.spec.min_score;
  h.search = search ? 1 : 0;
  h.lds_inputs = (int32_t)((b->lds_trace + 15) & ~size_t(15));
  h.mask_words = b->hits.mask_words;
  h.flags = b->hits.spec.flags;
  h.min_permille = b->hits.min_permille;
  h.min_scores = b->hits.d_min_scores.p;
  h.prof_off = b->hits.d_prof_off.p;
  h.profile = b->hits.d_profile.p;
  h.head = b->hits.d_head.p;
  h.hits = b->hits.d_rec.p;
  h.walks = b->hits.d_walks.p;
  h.trace = b->hits.d_trace.p;
  return h;
}

// profile: -infinity; status NOT_SEARCHED, no hits, no walks; records -1
int reset_hits(bialign_batch* b, hipStream_t st) {
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)b->hits.d_profile.p, BIALIGN_NEG_INF, b->hits.d_profile.n, st));
  HIP_TRY(hipMemsetAsync(b->hits.d_head.p, 0, sizeof(int32_t) * b->hits.d_head.n, st));
  HIP_TRY(hipMemsetAsync(b->hits.d_rec.p, 0xff, sizeof(int32_t) * b->hits.d_rec.n, st));
  HIP_TRY(hipMemsetAsync(b->hits.d_walks.p, 0xff, sizeof(int32_t) * b->hits.d_walks.n, st));
  return BIALIGN_OK;
}

// the hit getters' common refusals, and the end of a pending run
static int hits_ready(const bialign_batch* b) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->hits.on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  if (!b->ran || !b->hits.ran) return fail(BIALIGN_E_INVALID, "bialign_batch_run has not been called since bialign_batch_set_hits");
  HIP_TRY(hipSetDevice(b->eng->device));
  return BIALIGN_OK;
}

}  // namespace bialign

using namespace bialign;

extern "C" {

int bialign_batch_set_hits(bialign_batch* b, const bialign_hit_spec* spec) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  if (int rc = bialign_batch_wait(b)) return rc;  // a pending run still writes the buffers released below
  HIP_TRY(hipSetDevice(b->eng->device));
  b->hits.release();
  if (!spec) return BIALIGN_OK;
  if (b->mode != bialign::AlignMode::Fit || b->lean || b->null_R)
    return fail(BIALIGN_E_UNSUPPORTED, "the hit search needs a FIT batch in full storage (not %s)",
                b->null_R ? "a null batch" : (b->mode != bialign::AlignMode::Fit ? "a batch without BIALIGN_BATCH_FIT" : "SCORE_ONLY"));
  if (spec->max_hits < 1 || spec->max_hits > 256) return fail(BIALIGN_E_INVALID, "max_hits must be 1..256, got %d", spec->max_hits);
  if (spec->min_score < 1) return fail(BIALIGN_E_INVALID, "min_score must be >= 1, got %d", spec->min_score);
  if (spec->max_walks != 0 && spec->max_walks < spec->max_hits)
    return fail(BIALIGN_E_INVALID, "max_walks must be 0 (4 * max_hits) or >= max_hits = %d, got %d", spec->max_hits, spec->max_walks);
  if (spec->flags & ~BIALIGN_HITS_PEAKS) return fail(BIALIGN_E_INVALID, "bialign_hit_spec.flags: unknown bits 0x%x", spec->flags & ~BIALIGN_HITS_PEAKS);
  bialign_hit_spec sp = *spec;
  if (sp.max_walks == 0) sp.max_walks = 4 * sp.max_hits;
  int max_m = 0;
  b->hits.prof_off.assign((size_t)b->npairs + 1, 0);
  for (int p = 0; p < b->npairs; ++p) {
    max_m = std::max(max_m, b->pairs[p].m);
    b->hits.prof_off[p + 1] = b->hits.prof_off[p] + b->pairs[p].m + 1;
  }
  b->hits.spec = sp;
  b->hits.mask_words = (max_m + 32) >> 5;
  const size_t lds = fit_hits_lds(hit_args(b, true));
  if (lds > 160 * 1024)
    return fail(BIALIGN_E_UNSUPPORTED, "the hit search's mask, spans and staged inputs need %zu bytes of LDS (160 KiB at most)", lds);
  const size_t prof = (size_t)b->hits.prof_off.back(), recs = (size_t)b->npairs * sp.max_hits * 4,
               walks = (size_t)b->npairs * sp.max_walks * 4, trace = (size_t)sp.max_hits * (size_t)b->trace_bytes;
  hipStream_t st = b->eng->stream;
  hipError_t err = b->hits.d_profile.alloc(prof);
  if (err == hipSuccess) err = b->hits.d_head.alloc(4 * (size_t)b->npairs);
  if (err == hipSuccess) err = b->hits.d_rec.alloc(recs);
  if (err == hipSuccess) err = b->hits.d_walks.alloc(walks);
  if (err == hipSuccess) err = b->hits.d_trace.alloc(trace);
  if (err == hipSuccess) err = b->hits.d_prof_off.upload(b->hits.prof_off.data(), (size_t)b->npairs, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err == hipSuccess && getenv("BIALIGN_TEST_FAIL_HITS_ALLOC")) err = hipErrorOutOfMemory;  // tests: pretend an allocation failed
  if (err != hipSuccess) {
    (void)hipGetLastError();
    b->hits.release();
    return fail(BIALIGN_E_NOMEM, "hit search: allocating %zu bytes of result buffers failed: %s",
                (prof + 4 * (size_t)b->npairs + recs + walks) * 4 + trace, hipGetErrorString(err));
  }
  b->hits.bytes = (int64_t)((prof + 4 * (size_t)b->npairs + recs + walks) * 4 + trace + (size_t)b->npairs * 8);
  b->hits.on = true;
  return BIALIGN_OK;
}

int bialign_batch_set_hit_thresholds(bialign_batch* b, const int32_t* min_score, int32_t min_permille) {
  if (!b) return fail(BIALIGN_E_INVALID, "NULL batch");
  // (hits.on is host state that only bialign_batch_set_hits changes, and that call ends a pending run itself)
  if (!b->hits.on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  if (min_permille < 0 || min_permille > 1000) return fail(BIALIGN_E_INVALID, "min_permille must be 0..1000, got %d", min_permille);
  if (min_score)
    for (int p = 0; p < b->npairs; ++p)
      if (min_score[p] < 1) return fail(BIALIGN_E_INVALID, "min_score[%d] must be >= 1, got %d", p, min_score[p]);
  if (int rc = bialign_batch_wait(b)) return rc;  // the first device call: a pending run still reads the array released below
  HIP_TRY(hipSetDevice(b->eng->device));
  const int64_t had = (int64_t)b->hits.d_min_scores.n * 4;
  if (min_score) {
    DevBuf<int32_t> d;
    hipStream_t st = b->eng->stream;
    hipError_t err = d.upload(min_score, (size_t)b->npairs, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess && getenv("BIALIGN_TEST_FAIL_HITS_ALLOC")) err = hipErrorOutOfMemory;  // tests: pretend an allocation failed
    if (err != hipSuccess) {  // the thresholds stay what they were
      (void)hipGetLastError();
      return fail(BIALIGN_E_NOMEM, "hit thresholds: allocating %zu bytes failed: %s", (size_t)b->npairs * 4, hipGetErrorString(err));
    }
    b->hits.d_min_scores.swap(d);
  } else {
    b->hits.d_min_scores.release();
  }
  b->hits.bytes += (int64_t)b->hits.d_min_scores.n * 4 - had;
  b->hits.min_permille = min_permille;
  return BIALIGN_OK;
}

int bialign_batch_get_hit_thresholds(const bialign_batch* b, int32_t* out) {
  if (!b || !out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = bialign_batch_wait(const_cast<bialign_batch*>(b))) return rc;
  if (!b->hits.on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  std::fill(out, out + b->npairs, -1);
  if (!b->ran || !b->hits.ran) return BIALIGN_OK;  // no run yet
  HIP_TRY(hipSetDevice(b->eng->device));
  std::vector<int32_t> head(4 * (size_t)b->npairs);
  HIP_TRY(hipMemcpy(head.data(), b->hits.d_head.p, sizeof(int32_t) * head.size(), hipMemcpyDeviceToHost));
  for (int p = 0; p < b->npairs; ++p)  // NOT_SEARCHED: a fill-only run, which forms no threshold.  A search without
    if (head[4 * (size_t)p + 2] != BIALIGN_HITS_NOT_SEARCHED)  // options leaves the word 0 (a T_p is >= 1): min_score
      out[p] = head[4 * (size_t)p + 3] ? head[4 * (size_t)p + 3] : b->hits.spec.min_score;
  return BIALIGN_OK;
}

int bialign_batch_get_hit_profile(const bialign_batch* b, int32_t pair, int32_t* out) {
  if (!out) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = hits_ready(b)) return rc;
  if (pair < 0 || pair >= b->npairs) return fail(BIALIGN_E_INVALID, "pair %d out of range", pair);
  HIP_TRY(hipMemcpy(out, b->hits.d_profile.p + b->hits.prof_off[pair], sizeof(int32_t) * (b->pairs[pair].m + 1), hipMemcpyDeviceToHost));
  return BIALIGN_OK;
}

int bialign_batch_get_hits(const bialign_batch* b, int32_t* nhits, int32_t* status, int32_t* start_b, int32_t* end_b,
                           int32_t* score, int32_t* trace_len, uint8_t* trace, int64_t* trace_off) {
  if (!nhits || !status || !start_b || !end_b || !score || !trace_len || !trace != !trace_off) return fail(BIALIGN_E_INVALID, "NULL argument");
  if (int rc = hits_ready(b)) return rc;
  const int K = b->hits.spec.max_hits;
  std::vector<int32_t> head(4 * (size_t)b->npairs), rec((size_t)b->npairs * K * 4);
  HIP_TRY(hipMemcpy(head.data(), b->hits.d_head.p, sizeof(int32_t) * head.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rec.data(), b->hits.d_rec.p, sizeof(int32_t) * rec.size(), hipMemcpyDeviceToHost));
  if (trace) HIP_TRY(hipMemcpy(trace, b->hits.d_trace.p, (size_t)K * b->trace_bytes, hipMemcpyDeviceToHost));
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
  const int K = b->hits.spec.max_walks;
  std::vector<int32_t> head(4 * (size_t)b->npairs), rec((size_t)b->npairs * K * 4);
  HIP_TRY(hipMemcpy(head.data(), b->hits.d_head.p, sizeof(int32_t) * head.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rec.data(), b->hits.d_walks.p, sizeof(int32_t) * rec.size(), hipMemcpyDeviceToHost));
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
  if (!b->hits.on) return fail(BIALIGN_E_INVALID, "no hit search is set on this batch (bialign_batch_set_hits)");
  info->spec = b->hits.spec;
  info->buffer_bytes = b->hits.bytes;
  info->search_ms = b->hits.ran ? b->clock.ms(Stage::Hits) : 0;
  return BIALIGN_OK;
}

}  // extern "C"
