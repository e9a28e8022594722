// bialign_mu2_build.hpp -- FEATURE form of mu2: the GPU builds the chunk's structure-score tables itself.
//
// The reference's RNA mode with predicted structures scores structure by (pyx:416-423)
//     mu2(k,l) = int(sw * (sqrt(upA[k] upB[l]) + sqrt(dnA[k] dnB[l]) + sqrt(unpA[k] unpB[l])))
// of three doubles per residue.  build_mu2_kernel writes, for every pair of the chunk about to be swept, the
// int32 n x m table the DENSE consumers read (entry (k,l) at [(k-1)*m + (l-1)] of dense_tab + tab_off) from the
// per-residue features in HBM; nothing of size n x m ever exists on the host.  The table buffer is per-chunk
// scratch (PairDesc::tab_off is chunk-relative for such a batch) and part of the HBM chunk plan.
//
// Bit-exactness: the same IEEE double operations in the reference's order -- three products, three square roots,
// two additions left to right, the product with (double)sw, truncation toward zero.  Contraction is off for this
// unit (no product may fuse into an addition); f64 subnormals are kept (the hipcc default for gfx950 kernels).
//
// Mapping: lanes run along l (one 256-byte row segment per wave store), a wave keeps its three B features in
// registers for a tile of MU2_ROWS rows, the row's three A features are wave-uniform loads.  A workgroup of four
// waves takes four consecutive tiles, i.e. 1 KiB of the same rows where the pair is that wide.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "bialign_types.hpp"

#pragma clang fp contract(off)

namespace bialign {

constexpr int MU2_ROWS = 16;     // rows per tile
constexpr int MU2_WAVES = 4;     // waves per workgroup
constexpr int MU2_MAX_GRID_Y = 4096;  // tile groups per pair in the grid; longer pairs loop

struct Mu2BuildArgs {
  const PairDesc* pairs;
  const int32_t* order;  // launch order of the pairs to build (block x -> pair id)
  // per-residue features, indexed like the code arrays: PairDesc::seq_a / seq_b + residue
  const double *up_a, *down_a, *unp_a, *up_b, *down_b, *unp_b;
  int32_t* tab;  // the chunk's table buffer
  // a dense mu1 riding along: its resident tables (pair p's at mu1_src + mu1_off[p]) are copied behind mu2's,
  // where the DENSE1 consumers expect them (mu1_table()); nullptr otherwise
  const int32_t* mu1_src;
  const int64_t* mu1_off;
  int32_t sw;  // structure_weight
};

// One table entry, the reference's expression operation by operation (pyx:416-423).
__host__ __device__ inline int32_t mu2_entry(double sw, double ua, double da, double pa, double ub, double db, double pb) {
  const double t = (sqrt(ua * ub) + sqrt(da * db)) + sqrt(pa * pb);
  return (int32_t)(sw * t);  // int(): toward zero; the host's range check keeps |sw * t| below 2^28
}

__global__ __launch_bounds__(64 * MU2_WAVES) void build_mu2_kernel(Mu2BuildArgs A) {
  const int pid = A.order[blockIdx.x];
  const PairDesc& pd = A.pairs[pid];
  const int n = pd.n, m = pd.m;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ctiles = (m + 63) / 64, rtiles = (n + MU2_ROWS - 1) / MU2_ROWS;
  const int64_t ntiles = (int64_t)ctiles * rtiles;
  int32_t* const dst = A.tab + pd.tab_off;
  const double sw = (double)A.sw;
  const double* const ua_p = A.up_a + pd.seq_a;
  const double* const da_p = A.down_a + pd.seq_a;
  const double* const pa_p = A.unp_a + pd.seq_a;
  for (int64_t t = (int64_t)blockIdx.y * MU2_WAVES + wave; t < ntiles; t += (int64_t)gridDim.y * MU2_WAVES) {
    const int rt = (int)(t / ctiles), ct = (int)(t - (int64_t)rt * ctiles);
    const int l = ct * 64 + lane;  // 0-based column
    const bool in = l < m;
    double ub = 0.0, db = 0.0, pb = 0.0;
    if (in) {
      ub = A.up_b[pd.seq_b + l];
      db = A.down_b[pd.seq_b + l];
      pb = A.unp_b[pd.seq_b + l];
    }
    const int k0 = rt * MU2_ROWS, k1 = k0 + MU2_ROWS < n ? k0 + MU2_ROWS : n;
    for (int k = k0; k < k1; ++k) {  // 0-based row, wave-uniform
      const int32_t v = mu2_entry(sw, ua_p[k], da_p[k], pa_p[k], ub, db, pb);
      if (in) dst[(int64_t)k * m + l] = v;
    }
  }
  if (A.mu1_src) {
    const int64_t nm = (int64_t)n * m;
    const int32_t* const src = A.mu1_src + A.mu1_off[pid];
    for (int64_t t = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; t < nm; t += (int64_t)gridDim.y * blockDim.x)
      dst[nm + t] = src[t];
  }
}

}  // namespace bialign
