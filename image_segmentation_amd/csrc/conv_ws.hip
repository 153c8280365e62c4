// Weight-stationary 3x3 convolution for the narrow, high-resolution layers (Cin <= 2 chunks, 64 output channels per
// tile: the 3->64 stem, the 64->64 convs of down1/up4 and the 64->128 concat gradient) where conv_rs.hip does not serve
// (images at most 16 pixels wide, a bias): these are HBM-bound (K = 9*Cin is tiny), so the structure is built around keeping
// the memory pipes busy instead of the matrix cores.  All 9*Cin*64 weights of the workgroup's channel tile are loaded into
// LDS ONCE; a persistent workgroup (8 waves, 256-pixel tiles) then streams pixel tiles: the next tile's patch is
// fetched into registers before the current tile's barrier-free MFMA loop (36 k-steps), so its HBM
// latency hides under the matrix work, and the only barriers left are the four around the epilogue.
// Shared pieces (layout, walk, piece map, transform, fragment loop, epilogue): conv_tile.hpp.
#include "conv_tile.hpp"

namespace {

template <typename T, int TWL, bool PRO>
__global__ __launch_bounds__(512, 2) void conv_ws_kernel(const ConvArgs a) {
  using E = ET<T>;
  using L = WsLayout<T, TWL>;
  constexpr int WM = 4, WN = 2, MF = 2, NF = 1, NTHR = L::NTHR, BM = L::BM, BN = L::BN, MAXCH = L::MAXCH;
  constexpr int TW = L::TW, TH = L::TH, ROWP = L::ROWP, PB = L::PB, WTAP = L::WTAP, WOFF = L::WOFF, MAINB = L::MAINB;
  constexpr int NPL = (L::NP + NTHR - 1) / NTHR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int H = a.H, W = a.W;
  const int nchunks = (a.CA + a.CB) / E::CH;       // 1 or 2 (checked by the launcher)
  const int nchA = a.CA / E::CH;

  // units: the channel tile is fixed per workgroup (its weights stay resident)
  const int tpi = a.tiles_x * a.tiles_y;
  const TileWalk tw = tile_walk(a.B * tpi, a.Ntot / BN);
  const int nt = tw.nt, GW = tw.GW, mt_end = tw.mt_end;
  int mt = tw.mt;
  if (mt >= mt_end) return;
  const int n0 = nt * BN;

  const int trash = MAINB + tid * 16;
  const int pc = tid & 3;
  int plds[NPL], prel[NPL];
  unsigned pint = 0;                               // bit i: piece i is an interior (non-halo) pixel of the tile
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int q = tid + i * NTHR;
    int py, px;
    prel[i] = patch_piece<L>(q, py, px);
    plds[i] = (q < L::NP) ? py * ROWP + px * PIXB + pc * 16 : trash;
    pint |= (patch_interior<L>(q, py, px) ? 1u : 0u) << i;
  }
  int laneA[MF], laneB[NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = (wm * MF + mf) * 32 + lr;
    laneA[mf] = (m >> TWL) * ROWP + (m & (TW - 1)) * PIXB + lh * 16;
  }
  laneB[0] = WOFF + (wn * 32 + lr) * PIXB + lh * 16;

  // ---- resident weights: [chunk][tap][64 rows][80 B]
  {
    const int total = nchunks * 9 * BN * 4;
    for (int q = tid; q < total; q += NTHR) {
      const int r = q & (BN * 4 - 1), ct = q / (BN * 4);     // ct = chunk*9 + tap
      const u32x4 v = *(const u32x4*)((const char*)a.w + ((size_t)ct * a.Ntot + n0) * 64 + r * 16);
      *(u32x4*)(smem + WOFF + ct * WTAP + (r >> 2) * PIXB + (r & 3) * 16) = v;
    }
  }

  u32x4 preg[MAXCH][NPL];
  unsigned pvalid = 0;
  float psc[MAXCH][E::VEC], psh[MAXCH][E::VEC];
  if (PRO) {
#pragma unroll
    for (int kc = 0; kc < MAXCH; ++kc)
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) {
        const int c = (kc < nchunks ? kc : 0) * E::CH + pc * E::VEC + j;
        psc[kc][j] = a.scale[c];
        psh[kc][j] = a.shift[c];
      }
  }
  int plin[NPL];                                   // pixel index of each fetched piece (for the act_out side output)
  auto load_patch = [&](int b, int y0, int x0) {
    pvalid = 0;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const PatchPixel px = patch_pixel<1>(prel[i], y0, x0, H, W);
      const size_t lin = (size_t)(b * H + px.cy) * W + px.cx;
      plin[i] = (int)lin;
      pvalid |= (px.ok ? 1u : 0u) << i;
#pragma unroll
      for (int kc = 0; kc < MAXCH; ++kc) {
        const int k = kc < nchunks ? kc : 0;                  // unused second chunk: harmless duplicate load
        const T* src = (k < nchA) ? (const T*)a.srcA + lin * a.CA + k * E::CH
                                  : (const T*)a.srcB + lin * a.CB + (k - nchA) * E::CH;
        preg[kc][i] = *(const u32x4*)(src + pc * E::VEC);
      }
    }
  };
  auto store_patch = [&]() {
#pragma unroll
    for (int kc = 0; kc < MAXCH; ++kc)
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const bool ok = (pvalid >> i) & 1;
        const u32x4 v = patch_transform<T, PRO>(preg[kc][i], psc[kc], psh[kc], ok);
        const int off = plds[i] + ((plds[i] < MAINB) ? kc * PB : 0);
        *(u32x4*)(smem + off) = v;
        if (PRO) {   // side output: the transformed activation itself, interior pixels, once per pixel and chunk
          if (a.act_out && nt == 0 && kc < nchunks && ok && ((pint >> i) & 1))
            *(u32x4*)((T*)a.act_out + (size_t)(unsigned)plin[i] * a.CA + kc * E::CH + pc * E::VEC) = v;
        }
      }
  };

  f32x16 acc[MF][NF];
  int ub, uy0, ux0;
  auto epilogue_t = [&](auto FULLc) {
    constexpr bool FULL = decltype(FULLc)::value;
    stage_wave32<T, TWL, BN, MF, NF, FULL, false>(a, acc, smem, (float*)(smem + L::RED), wm, wn, lane, n0, uy0, ux0);
    __syncthreads();
    reduce_stat_rows<WM, BN>(a, (const float*)(smem + L::RED), tid, mt, n0);
    store_staged_tile<T, TWL, BM, BN, NTHR, FULL, false>(a, smem, tid, ub, uy0, ux0, n0);
  };

  decode_tile<TW, TH>(a, tpi, mt, ub, uy0, ux0);
  load_patch(ub, uy0, ux0);
  store_patch();
  __syncthreads();
  for (;;) {
    const int mnext = mt + GW;
    const bool has_next = mnext < mt_end;
    int nb = ub, ny0 = uy0, nx0 = ux0;
    if (has_next) {
      decode_tile<TW, TH>(a, tpi, mnext, nb, ny0, nx0);
      load_patch(nb, ny0, nx0);            // flies under the MFMA loop below
    }
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mf][0][r] = 0.f;
    // per chunk 18 sub-steps (9 taps x 2 k-steps); fragment reads run one sub-step ahead of the MFMAs
    for (int kc = 0; kc < nchunks; ++kc) mma_taps<T, 9, ROWP, WTAP>(smem + kc * PB, smem + kc * 9 * WTAP, laneA, laneB, acc);
    __syncthreads();                       // patch fully consumed: its LDS becomes the output staging tile
    if ((uy0 + TH <= H) && (ux0 + TW <= W)) epilogue_t(std::true_type{});
    else epilogue_t(std::false_type{});
    if (!has_next) break;
    __syncthreads();
    store_patch();
    mt = mnext; ub = nb; uy0 = ny0; ux0 = nx0;
    __syncthreads();
  }
}

template <typename T, int TWL, bool PRO>
int launch_ws(ConvArgs a, const ConvPlan& p, hipStream_t st) {
  using L = WsLayout<T, TWL>;
  static_assert(L::LDS <= 160 * 1024, "conv_ws: LDS exceeds 160 KiB");
  SEGK_REQUIRE_PLAN_TILE("conv_ws", p, L::BM, TWL);
  int gw, GW;                                              // one workgroup per CU
  segk_conv_rs_grid(conv_set_tiles<L>(a, TWL), a.Ntot / L::BN, &gw, &GW);
  return segk_launch_lds<conv_ws_kernel<T, TWL, PRO>>("conv_ws", 160 * 1024, dim3(8 * gw), dim3(L::NTHR), L::LDS, st, a);
}

}  // namespace

int segk_conv_ws_launch(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
  auto by_pro = [&](auto TWLc) {
    constexpr int TWL = decltype(TWLc)::value;
    return a.scale ? launch_ws<bf16_t, TWL, true>(a, p, st) : launch_ws<bf16_t, TWL, false>(a, p, st);
  };
  return p.twl == 5 ? by_pro(std::integral_constant<int, 5>{}) : by_pro(std::integral_constant<int, 4>{});
}
