// bialign_wide.hip -- launchers of the wide-band path (any max_shift; kernels in bialign_wide.hpp and the
// WIDE forms of the traceback kernels).  One translation unit: the band width is a runtime value.
#include "bialign_host.hpp"

namespace bialign {

// The sweep kernel of a batch, handed to fn: affine or one-layer, mu1 as LOOKUP or dense tables; MODE: all layers
// (or, affine, none: score only), or a pass of the level-checkpointed traceback.
template <int MODE, typename Fn>
int with_wide_fill_kernel(const bialign_batch* b, Fn&& fn) {
  if (b->affine) return b->dense1 ? fn(fill_wide_affine_kernel<1, MODE>) : fn(fill_wide_affine_kernel<0, MODE>);
  return b->dense1 ? fn(fill_wide_linear_kernel<1, MODE>) : fn(fill_wide_linear_kernel<0, MODE>);
}

template <int MODE>
static int launch_fill_wide_mode(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  DeviceBatch w = v;
  w.order = v.order + first;
  b->packed_layers = false;
  // Workgroups ("parts") per pair: as many as keep the device busy and can all be resident at once (they meet at a
  // counter after every level), no more than a level has work for; one after a lost-co-residency recovery.
  int parts = 1;
  if (!b->no_xcu) {
    const int resident = with_wide_fill_kernel<MODE>(b, [&](auto kern) { return xcu_resident(b, kern, WIDE_THREADS, 0); });
    int busiest = 1;  // points of the largest level, over the pairs of this launch: ~ min(n, m) rows x W x (W+1)/2
    for (int t = first; t < first + count; ++t) {
      const PairDesc& d = b->pairs[b->order[t]];
      const int W = 2 * b->S + 1;
      busiest = std::max<int64_t>(busiest, (int64_t)(std::min(d.n, d.m) + 1) * W * ((W + 1) / 2));
    }
    parts = std::max(1, std::min({resident / std::max(count, 1), (busiest + WIDE_THREADS - 1) / WIDE_THREADS, PROG_WORDS}));
    if (const char* e = getenv("BIALIGN_WIDE_PARTS")) parts = std::max(1, std::min(atoi(e), parts));  // tests
  }
  w.team = parts;
  // (WIDE_FULL, affine: the ring of derived values is chunk scratch of the plan -- DeviceBatch::wide_ring, a pair's at its
  //  PairDesc::scratch_off; bialign_batch::view() -- so a launch allocates and uploads nothing)
  b->last_team = parts * (WIDE_THREADS / 64) * (parts > 1 ? -1 : 1);
  return with_wide_fill_kernel<MODE>(b, [&](auto kern) {
    return launch_team(b, kern, dim3(count * parts), dim3(WIDE_THREADS), 0, w, count, parts > 1, b->S);
  });
}

int launch_fill_wide(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return b->level_trace ? launch_fill_wide_mode<WIDE_CKPT>(b, v, first, count) : launch_fill_wide_mode<WIDE_FULL>(b, v, first, count);
}

int launch_segment_wide(bialign_batch* b, const DeviceBatch& v, int first, int count) {
  return launch_fill_wide_mode<WIDE_SEG>(b, v, first, count);
}

int launch_traceback_level(const bialign_batch* b, const DeviceBatch& v, int first, int count) {
  constexpr unsigned F = T_TRACE | T_LEVEL;
  if (b->affine)
    return b->dense1 ? launch_traceback_kernel(b, traceback_affine_of<0, F | T_DENSE1>(), true, v, first, count)
                     : launch_traceback_kernel(b, traceback_affine_of<0, F>(), true, v, first, count);
  return b->dense1 ? launch_traceback_kernel(b, traceback_linear_of<0, F | T_DENSE1>(), true, v, first, count)
                   : launch_traceback_kernel(b, traceback_linear_of<0, F>(), true, v, first, count);
}

int launch_traceback_wide(const bialign_batch* b, const DeviceBatch& v, int first, int count, bool do_trace) {
  return with_flags<T_TRACE | T_DENSE1>(trace_flags(b, do_trace), [&](auto flags) -> int {
    constexpr unsigned F = decltype(flags)::value | T_WIDE;
    if constexpr (traceback_exists(true, 0, F))
      return b->affine ? launch_traceback_kernel(b, traceback_affine_of<0, F>(), do_trace, v, first, count)
                       : launch_traceback_kernel(b, traceback_linear_of<0, F>(), do_trace, v, first, count);
    else
      return fail(BIALIGN_E_UNSUPPORTED, "no wide-band traceback in form %u", F);
  });
}

int launch_dump_wide(const bialign_batch* b, const DeviceBatch& v, int pid, int32_t* d_out) {
  return b->affine ? launch(dump_wide_kernel<9>, dim3(256), dim3(256), 0, b->eng->stream, v, b->S, pid, d_out)
                   : launch(dump_wide_kernel<1>, dim3(256), dim3(256), 0, b->eng->stream, v, b->S, pid, d_out);
}

}  // namespace bialign
