// bialign_mu2_build.hip -- the table builder of the FEATURE form of mu2 (bialign_mu2_build.hpp) and its launcher.
// A unit of its own: compiled with contraction off, and the fill kernels' units do not see it.
#include "bialign_host.hpp"
#include "bialign_mu2_build.hpp"

namespace bialign {

int launch_build_mu2(bialign_batch* b, int first, int count) {
  if (!b->feat || count < 1) return BIALIGN_OK;
  Mu2BuildArgs a{};
  a.pairs = b->d_pairs.p;
  a.order = b->d_order.p + first;
  a.up_a = b->tables.d_feat_a.p;
  a.down_a = b->tables.d_feat_a.p + b->tables.feat_tot_a;
  a.unp_a = b->tables.d_feat_a.p + 2 * b->tables.feat_tot_a;
  a.up_b = b->tables.d_feat_b.p;
  a.down_b = b->tables.d_feat_b.p + b->tables.feat_tot_b;
  a.unp_b = b->tables.d_feat_b.p + 2 * b->tables.feat_tot_b;
  a.tab = b->tables.d_tab.p;
  a.mu1_src = b->dense1 ? b->tables.d_mu1.p : nullptr;
  a.mu1_off = b->dense1 ? b->tables.d_mu1_off.p : nullptr;
  a.sw = b->feat_sw;
  int64_t groups = 1;  // workgroups per pair: one per MU2_WAVES tiles of the launch's largest table
  for (int t = first; t < first + count; ++t) {
    const PairDesc& d = b->pairs[b->order[t]];
    const int64_t tiles = (int64_t)((d.m + 63) / 64) * ((d.n + MU2_ROWS - 1) / MU2_ROWS);
    groups = std::max(groups, (tiles + MU2_WAVES - 1) / MU2_WAVES);
  }
  return launch(build_mu2_kernel, dim3(count, (unsigned)std::min<int64_t>(groups, MU2_MAX_GRID_Y)), dim3(64 * MU2_WAVES), 0,
                b->eng->stream, a);
}

}  // namespace bialign
