// bialign_affine_point.hpp -- what the affine sweeps share per lattice point: the fifteen cases of the recurrence over
// the delay lines, and the register hand-over from lane L-1.  Part of bialign_kernels.hpp (include that, not this).
// fill_affine_kernel and fill_affine_slim_kernel differ in how rows i-1 reach a lane (LDS exchange array against
// ds_bpermute) and in how records leave it; the recurrence itself is stated here, once.
#pragma once

namespace bialign {

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
// f_T for the three target halves; arguments are the values for source half Y, X, M.
__device__ __forceinline__ int fM(int y, int x, int m) { return imax(imax(y, x), m); }
__device__ __forceinline__ int fX(int y, int x, int m, int beta) { return imax(x, beta + imax(y, m)); }
__device__ __forceinline__ int fY(int y, int x, int m, int beta) { return imax(y, beta + imax(x, m)); }

// Can target state (hU,hV) at band column bb end up with no guard-valid case for
// some band row a when all four lattice coordinates are >= 1?  (Then only the
// band decides validity and the answer is static per (state, bb).)
template <int W>
__host__ __device__ constexpr bool can_be_empty(int hU, int hV, int bb) {
  const int u0 = hU >= 1, u1 = hU != 1, v0 = hV >= 1, v1 = hV != 1;
  for (int aa = 0; aa < W; ++aa) {
    const int a1 = aa + u0 - v0, b1 = bb + u1 - v1;  // group 1, offset (U,V)
    const int a2 = aa - v0, b2 = bb - v1;            // group 2, offset (0,0,V)
    const int a3 = aa + u0, b3 = bb + u1;            // group 3, offset (U,0,0)
    const bool g1 = a1 >= 0 && a1 < W && b1 >= 0 && b1 < W;
    const bool g2 = a2 >= 0 && a2 < W && b2 >= 0 && b2 < W;
    const bool g3 = a3 >= 0 && a3 < W && b3 >= 0 && b3 < W;
    if (!g1 && !g2 && !g3) return true;
  }
  return false;
}

template <bool V>
struct BoolTag {
  static constexpr bool value = V;
};

// The fifteen cases (pyx:474-509) of the nine states of one lattice point: band column bb of this lane's (i, j, a), read
// off the delay lines (see the sweeps for who fills them and when):
//   dA2  GMM, GMX from (i-1,a), age 3            dAx    GXM, GXX from (i-1,a), age 2
//   dB   GMY, H3M[0..2] from (i-1,a+1), age 2    dC     GYM, GYX from (i,a-1), age 2
//   inB  what (i-1,a+1) derived one step ago     inC    what lane L-1 handed over (dpp_from_left)
//   selfv  GYY, H3Y[0..2] of this lane's previous column     h2y  H2[U][Y] of point bb-1 (same step, same lane)
// and the addends: c_MM = mu1 + mu2, c_Mg = mu1 + gamma + Delta, c_gM = mu2 + gamma + Delta, gg = 2 gamma,
// ggdd = 2 gamma + 2 Delta (group 1);  c2M = mu2 + 2 Delta (group 2, V = M);  c3M = mu1 + 2 Delta (group 3, U = M);
// gD = gamma + Delta (every other group-2 and group-3 case).  A case whose source would leave the band (bb - 1 < 0,
// bb + 1 >= W) does not exist; Tv[3 hU + hV] is the maximum over those that do, in the sentinel window if none is valid.
// bb is a constant wherever a point is evaluated (an unrolled loop): every branch on it folds.
//   A sweep binds the point's inputs once --  const AffineCases<W> cases{dA2, bb, ...};  -- and evaluates with cases(Tv).
// A struct of references, its members in the order the body first names them, and not a function with seventeen
// parameters: this is the object the sweeps' own `cases` lambdas were, and hipcc's register allocation follows it.  As a
// function template the same body left every kernel with gap_opening_cost <= 0 as it was and made the general-beta
// sweeps 2.5 % (max_shift 1) to 5 % (max_shift 5) longer, with 7-19 more AGPRs at max_shift 2 and 3 and 32-92 bytes
// more scratch per lane at max_shift 4 and 5 (profiles/r08a_one_form); in this form all of them compile to what they
// were.  Keep the member order when adding to it.
template <int W>
struct AffineCases {
  const int (&dA2)[2][W];
  const int& bb;
  const int (&dB)[4][W];
  const int (&dAx)[2][W];
  const int (&inB)[W][8];
  const int (&dC)[2][W];
  const int (&selfv)[4][W];
  const int &c_MM, &c_Mg, &c_gM, &gg, &ggdd;
  const int (&inC)[W][8];
  const int (&h2y)[3];
  const int &c2M, &gD, &c3M;

  __device__ __forceinline__ void operator()(int (&Tv)[9]) const {
#pragma unroll
    for (int hU = 0; hU < 3; ++hU) {
#pragma unroll
      for (int hV = 0; hV < 3; ++hV) {
        // group 1: offset (U,V)
        int gin = SENT;
        bool ok1 = true;
        if (hU == 2 && hV == 2) gin = dA2[0][bb];
        if (hU == 2 && hV == 1) { ok1 = bb + 1 < W; if (ok1) gin = dA2[1][bb + 1 < W ? bb + 1 : 0]; }
        if (hU == 2 && hV == 0) gin = dB[0][bb];
        if (hU == 1 && hV == 2) { ok1 = bb >= 1; if (ok1) gin = dAx[0][bb >= 1 ? bb - 1 : 0]; }
        if (hU == 1 && hV == 1) gin = dAx[1][bb];
        if (hU == 1 && hV == 0) { ok1 = bb >= 1; if (ok1) gin = inB[bb >= 1 ? bb - 1 : 0][1]; }
        if (hU == 0 && hV == 2) gin = dC[0][bb];
        if (hU == 0 && hV == 1) { ok1 = bb + 1 < W; if (ok1) gin = dC[1][bb + 1 < W ? bb + 1 : 0]; }
        if (hU == 0 && hV == 0) gin = selfv[0][bb];
        const int c1 = (hU == 2 && hV == 2) ? c_MM
                       : (hU == 2)          ? c_Mg
                       : (hV == 2)          ? c_gM
                       : (hU == hV)         ? gg
                                            : ggdd;
        // group 2: offset (0,0,V)
        int h2in = SENT;
        bool ok2 = true;
        if (hV == 2) { ok2 = bb >= 1; if (ok2) h2in = inC[bb >= 1 ? bb - 1 : 0][2 + hU]; }
        if (hV == 1) h2in = inC[bb][5 + hU];
        if (hV == 0) { ok2 = bb >= 1; if (ok2) h2in = h2y[hU]; }
        const int c2 = (hV == 2) ? c2M : gD;
        // group 3: offset (U,0,0)
        int h3in = SENT;
        bool ok3 = true;
        if (hU == 2) { ok3 = bb + 1 < W; if (ok3) h3in = dB[1 + hV][bb + 1 < W ? bb + 1 : 0]; }
        if (hU == 1) h3in = inB[bb][5 + hV];
        if (hU == 0) { ok3 = bb + 1 < W; if (ok3) h3in = selfv[1 + hV][bb + 1 < W ? bb + 1 : 0]; }
        const int c3 = (hU == 2) ? c3M : gD;

        int t = SENT;
        bool any = false;
        if (hU < 2 && hV < 2 && ok2 && ok3) {
          // both gap-gap groups cost gamma + Delta: max(c1 + g, gD + h2, gD + h3) = gD + max(g + (c1 - gD), h2, h3),
          // exact in integers, one add less (c1 - gD is wave-uniform: gamma - Delta or gamma + Delta)
          const int inner = ok1 ? imax(imax(gin + (c1 - gD), h2in), h3in) : imax(h2in, h3in);
          t = gD + inner;
        } else {
          if (ok1) { t = c1 + gin; any = true; }
          if (ok2) { t = any ? imax(t, c2 + h2in) : c2 + h2in; any = true; }
          if (ok3) { t = any ? imax(t, c3 + h3in) : c3 + h3in; any = true; }
        }
        Tv[3 * hU + hV] = t;
      }
    }
  }
};

// Lane L-1 = (i, a-1) hands what it published for band column r (pubC[r]: GYM, GYX, H2M[0..2], H2X[0..2] of its
// previous column) over in registers: one DPP wave shift fused with a min against the lane's cap (the sentinel where
// a-1 leaves the band, INT_MAX elsewhere).  One asm block per band column: the compiler's own DPP folding gives up once
// the consumers are sunk behind the store branches.  s_nop 1 = the two wait states a DPP read needs after a VALU write
// of its source (the hazard recogniser does not look inside asm; dropping it "because the sources are a step old" broke
// the dense s=2,3 kernels in round 3); lane 0 reads out of range -> 0 with bound_ctrl, it is an a_first lane anyway.
// H2[.][M] (x = 2..4) of the last band column has no consumer: offset (0,0,M) from there would leave the band.
template <int W>
__device__ __forceinline__ void dpp_from_left(const int r, int (&inC)[W][8], const int (&pubC)[W][8], const int lane_cap) {
  if (r + 1 < W) {
    asm("s_nop 1\n\t"
        "v_min_i32_dpp %0, %8, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %1, %9, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %2, %10, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %3, %11, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %4, %12, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %5, %13, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %6, %14, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %7, %15, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(inC[r][0]), "=&v"(inC[r][1]), "=&v"(inC[r][2]), "=&v"(inC[r][3]), "=&v"(inC[r][4]),
          "=&v"(inC[r][5]), "=&v"(inC[r][6]), "=&v"(inC[r][7])
        : "v"(pubC[r][0]), "v"(pubC[r][1]), "v"(pubC[r][2]), "v"(pubC[r][3]), "v"(pubC[r][4]),
          "v"(pubC[r][5]), "v"(pubC[r][6]), "v"(pubC[r][7]), "v"(lane_cap));
  } else {
    asm("s_nop 1\n\t"
        "v_min_i32_dpp %0, %5, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %1, %6, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %2, %7, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %3, %8, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_min_i32_dpp %4, %9, %10 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(inC[r][0]), "=&v"(inC[r][1]), "=&v"(inC[r][5]), "=&v"(inC[r][6]), "=&v"(inC[r][7])
        : "v"(pubC[r][0]), "v"(pubC[r][1]), "v"(pubC[r][5]), "v"(pubC[r][6]), "v"(pubC[r][7]), "v"(lane_cap));
    inC[r][2] = inC[r][3] = inC[r][4] = SENT;
  }
}

}  // namespace bialign
