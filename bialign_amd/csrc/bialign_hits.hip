// bialign_hits.hip -- the hit-search kernels of FIT batches (bialign_hits.hpp), instantiated as the generic tracebacks
// are: max_shift 0..5, affine and one-layer, packed records (affine, max_shift 1..BIALIGN_MAX_SHIFT_PACKED), dense mu1.
#include "bialign_hits.hpp"

namespace bialign {

namespace {

template <int S, bool AFFINE, bool PACK, bool D1>
int launch_one(const bialign_batch* b, const DeviceBatch& v, const HitArgs& h, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  return launch(fit_hits_kernel<S, AFFINE, PACK, D1>, dim3(count), dim3(64), fit_hits_lds(h), b->eng->stream, w, h, count);
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

}  // namespace bialign
