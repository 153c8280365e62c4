// Implicit-GEMM convolution for NHWC activations on CDNA4 matrix cores (gfx950).
//
// One kernel family serves, by geometry/flags:
//   GEO 0 : Conv2d 3x3 pad 1 stride 1   -- forward (reference unet/unet.py:16,19; clip/clipunet.py:87,90)
//                                          and data-gradient (same kernel, flipped+transposed weights)
//   GEO 1 : 1x1 "conv"                  -- ConvTranspose2d(k=2,s=2) forward as GEMM + pixel-shuffle store
//                                          (unet.py:59, clipunet.py:83), its data-gradient as a 2x2
//                                          un-shuffle gather GEMM, and the CLIP 1x1 projections (clipunet.py:84,122)
//
// GEMM view: M = BM output pixels of one spatial tile (TH x TW), N = BN output channels, K = taps x Cin.
// The input patch (tile + halo) of one 64-byte channel chunk is staged ONCE into LDS and reused by all 9
// taps as shifted row addresses (the 3x3 im2col never exists); weight tiles stream through a second,
// double-buffered LDS region.  Staging is register-staged (global -> VGPR -> LDS, issue-early /
// write-late) so the previous layer's BatchNorm+ReLU can be applied on the fly (prologue fusion) and so
// out-of-image halo pixels become exact zeros.  MFMA: bf16 32x32x16 or exact fp32 32x32x2 with a
// byte-identical LDS image (a 16-byte fragment read is 8 bf16 k-values or 4 fp32).
//
// The kernel is PERSISTENT over work units (pixel tile x channel tile): every XCD owns a contiguous range
// of units (neighbouring tiles share halos and weights through that XCD's L2), each workgroup walks its
// XCD's range with a fixed stride, and the loads of the next unit's first patch chunk / weight step are
// issued under the current unit's last MFMA steps, so the HBM latency of a tile start hides behind the
// previous tile's tail and the per-thread addressing set-up is paid once per workgroup, not per tile.
//
// Epilogue: optional bias, per-channel sum / sum-of-squares partials for training-mode BatchNorm taken
// from the fp32 accumulators (deterministic per-tile partials, no atomics), LDS transpose, 16-byte
// coalesced NHWC stores (optionally split over two destinations, or pixel-shuffled for ConvTranspose).
// This unit keeps the dispatch plan, the entry checks and the generic kernel; the other forms have units of their own
// (conv_pipe.hip, conv_ws.hip, conv_rs.hip) and what they share is conv_tile.hpp.
#include "conv_tile.hpp"

// ---- the dispatch, stated once: which kernel form serves a call, with which tile (segk_internal.h: ConvPlan)
// weight-stationary kernel: at most two 64-byte input chunks and N a multiple of 64 (but not a 128-wide layer
// with a long K, which the MFMA-bound streaming kernel serves better)
static bool use_ws(int cin_p, int n_p, int dtype) {
  return dtype == SEGK_DT_BF16 && cin_p <= 64 && n_p % 64 == 0;   // bf16 performance mode only
}
// producer/consumer kernel (bf16 3x3, at least two 64-byte input chunks, not a weight-stationary layer): returns
// its channel tile, 128 (256-pixel tiles) or 64 (512-pixel tiles, Cin >= 128: with K = 576 the unit boundary
// dominates and the weight-stationary kernel wins), or 0
static int use_pipe(int cin_p, int n_p, int dtype) {
  if (dtype != SEGK_DT_BF16 || use_ws(cin_p, n_p, dtype) || cin_p < 64) return 0;
  if (n_p % 128 == 0) return 128;
  if (n_p % 64 == 0 && cin_p >= 128) return 64;
  return 0;
}
// Tile of the generic kernel for a layer whose N is a multiple of `unit` (128 | 64 | 32, the largest that divides it), on an
// image wider than 16 pixels or not: BM = wm * mf * 32 pixels by BN = wn * nf * 32 channels (BN must divide N; with the
// pixel-shuffle store a tile may span taps: each thread derives its own tap).  constexpr: the plan reads it at run time and
// launch_geo takes its template arguments from it, so no shape is compiled that the plan cannot name.  wm == 0: no generic
// kernel -- a bf16 3x3 layer with N % 128 == 0 is weight-stationary (Cin <= 64) or producer/consumer (Cin >= 96).
struct GenericTile { int twl, wm, wn, mf, nf, pbuf; };
static constexpr GenericTile generic_tile(int geo, bool bf16, int unit, bool wide) {
  const int twl = wide ? 5 : 4;                    // 8x32 tiles unless the image is at most 16 wide
  // bf16 1x1 / ConvTranspose GEMMs have a short K (Cin) and are bound by their output epilogue: 128-pixel tiles on
  // 4-wave workgroups, two per CU, so one workgroup's epilogue overlaps the other's loads and MFMAs
  if (geo == 1 && bf16 && unit >= 64) return {4, 2, 2, 2, unit == 128 ? 2 : 1, 2};
  if (unit == 128) return geo == 0 && bf16 ? GenericTile{0, 0, 0, 0, 0, 0} : GenericTile{twl, 4, 2, 2, 2, 2};   // 256 px x 128 ch, 8 waves
  if (geo == 0) return unit == 64 ? GenericTile{4, 2, 2, 2, 1, 1}           // 128 px x 64 ch, 4 waves
                                  : GenericTile{4, 4, 1, 1, 1, 1};          // 128 px x 32 ch, 4 waves
  return unit == 64 ? GenericTile{twl, 4, 2, 2, 1, 2} : GenericTile{twl, 8, 1, 1, 1, 2};
}

ConvPlan segk_conv_plan(int geo, int dtype, int cin_p, int n_p, int W, bool has_bias, bool gemm_dma) {
  ConvPlan p{};
  p.wide = W > 16;
  p.twl = p.wide ? 5 : 4;                            // 8x32 | 16x16 (16x32 | 32x16 at 512 pixels) tiles
  p.bm = 256;
  if (geo == 0 && segk_conv_use_rs(cin_p, n_p, dtype, W) && !has_bias) {
    // narrow high-resolution layers, images wider than 16 pixels: register-stationary streaming kernel (conv_rs.hip); it
    // carries no bias, a biased layer goes on to the weight-stationary kernel
    p.form = CONV_RS; p.bn = 64; p.rs_rows = true;
  } else if (geo == 0 && use_ws(cin_p, n_p, dtype)) {      // narrow high-resolution layers (64-channel tiles)
    p.form = CONV_WS; p.bn = 64;
  } else if (geo == 0 && use_pipe(cin_p, n_p, dtype)) {    // MFMA-bound bf16 layers
    p.form = CONV_PIPE; p.bn = use_pipe(cin_p, n_p, dtype); p.bm = 32768 / p.bn;
  } else if (gemm_dma) {                            // long-K GEMMs (ViT projections, ConvTranspose up-sampling and its data gradient)
    p.form = CONV_GEMM_DMA; p.bn = 128; p.twl = 0;  // rows, not pixel tiles: gemm.hip picks 256 or 320 of them
  } else {
    p.form = CONV_GENERIC;
    p.unit = n_p % 128 == 0 ? 128 : n_p % 64 == 0 ? 64 : 32;
    const GenericTile g = generic_tile(geo, dtype == SEGK_DT_BF16, p.unit, p.wide);
    p.twl = g.twl; p.wm = g.wm; p.wn = g.wn; p.mf = g.mf; p.nf = g.nf; p.pbuf = g.pbuf;
    p.bm = g.wm * g.mf * 32; p.bn = g.wn * g.nf * 32;
  }
  return p;
}
// conv_rs, conv_ws and the producer/consumer kernel can; the width only chooses between the first two
int segk_conv_writes_act(int cin_p, int n_p, int dtype) {
  return segk_conv_plan(0, dtype, cin_p, n_p, /*W=*/17, false, false).form != CONV_GENERIC;
}

namespace {

// Tile: BM = WM*MF*32 output pixels (TH x TW, TW = 1 << TWL) by BN = WN*NF*32 output channels, WM*WN waves.
// PBUF: patch buffers (2 = next chunk staged under the current chunk's MFMAs; 1 = smaller LDS footprint so
// that two or three 4-wave workgroups share a CU and overlap each other's load / MFMA / store phases).
template <typename T, int GEO, int TWL, int WM, int WN, int MF, int NF, int PBUF, bool PRO>
__global__ __launch_bounds__(WM * WN * 64, 2) void conv_igemm_kernel(const ConvArgs a) {
  using E = ET<T>;
  using L = IgemmLayout<T, GEO, TWL, WM, WN, MF, NF, PBUF>;
  constexpr int NTHR = L::NTHR, BM = L::BM, BN = L::BN;
  constexpr int NTAPS = (GEO == 0) ? 9 : 1;
  constexpr int TPS = L::TPS;               // taps per pipeline step (one kernel row)
  constexpr int SPC = (GEO == 0) ? 3 : 1;   // steps per channel chunk
  constexpr int HALO = (GEO == 0) ? 1 : 0;
  constexpr int TW = L::TW, TH = L::TH, ROWP = L::ROWP, PB = L::PB, WB = L::WB, NP = L::NP;
  constexpr int NPL = (NP + NTHR - 1) / NTHR;
  constexpr int NWP = TPS * BN * 4;                // weight 16-byte pieces per step
  constexpr int NWL = (NWP + NTHR - 1) / NTHR;
  static_assert(BM == 256 || BM == 128, "pixel tile is 256 or 128");
  static_assert(NTHR % 4 == 0, "a thread keeps one 16-byte slot of the 64-byte chunk");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave - wm * WN;
  const int lr = lane & 31, lh = lane >> 5;
  const int H = a.H, W = a.W;

  // ---- work units
  const int NT = a.Ntot / BN;
  const int tpi = a.tiles_x * a.tiles_y;
  const UnitWalk uw = unit_walk(a.B * tpi * NT);
  const int GW = uw.GW, u_end = uw.u_end;
  int u = uw.u;
  if (u >= u_end) return;

  // ---- unit-invariant staging assignment.  Straight-line staging: every thread always moves NPL patch
  // pieces and NWL weight pieces; pieces past the tile's count read a valid dummy address and land in a
  // per-thread trash slot behind the staging buffers, so there is no divergent control flow around
  // loads or LDS stores.
  constexpr int MAINB = L::MAINB;
  const int trash = MAINB + tid * 16;
  const int pc = tid & 3;  // 16-byte slot inside the 64-byte chunk (NTHR % 4 == 0: same for every piece)
  int plds[NPL], prel[NPL];   // LDS byte offset and packed patch-relative coordinates (py << 8 | px)
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int q = tid + i * NTHR;
    int py, px;
    prel[i] = patch_piece<L>(q, py, px);
    plds[i] = (q < NP) ? py * ROWP + px * PIXB + pc * 16 : trash;
  }
  int wsrc[NWL], wlds[NWL];
#pragma unroll
  for (int i = 0; i < NWL; ++i) {
    const int q = tid + i * NTHR;
    const int t = q / (BN * 4), r = q - t * (BN * 4);
    wsrc[i] = (q < NWP) ? t * a.Ntot * 64 + r * 16 : 0;    // byte offset from the step's weight base
    wlds[i] = (q < NWP) ? PBUF * PB + t * (BN * PIXB) + (r >> 2) * PIXB + (r & 3) * 16 : trash;
  }
  const int nchA = a.CA / E::CH;
  const int nchunks = a.unshuf ? 4 * nchA : (a.CA + a.CB) / E::CH;
  const int nsteps = nchunks * SPC;

  // per-lane fragment addresses
  int laneA[MF], laneB[NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = (wm * MF + mf) * 32 + lr;
    laneA[mf] = (m >> TWL) * ROWP + (m & (TW - 1)) * PIXB + lh * 16;
  }
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) laneB[nf] = ((wn * NF + nf) * 32 + lr) * PIXB + lh * 16;

  char* const patch0 = smem;
  char* const wbuf0 = smem + PBUF * PB;

  // ---- unit state
  int ub, uy0, ux0, un0, umt;       // current unit
  auto decode = [&](int uu, int& mt, int& b, int& y0, int& x0, int& n0) { decode_unit<TW, TH, BN>(a, NT, tpi, uu, mt, b, y0, x0, n0); };
  u32x4 preg[NPL], wreg[NWL];
  unsigned pvalid = 0;              // bit i: preg[i] holds an in-image pixel
  float psc[E::VEC], psh[E::VEC];

  auto load_patch = [&](int kc, int b, int y0, int x0) {
    const T* src;
    int C, coff, tapadd = 0;
    if (a.unshuf) {
      const int tap = kc / nchA, cc = kc - tap * nchA;
      src = (const T*)a.srcA; C = a.CA; coff = cc * E::CH;
      tapadd = (tap >> 1) * 2 * W + (tap & 1);
    } else if (kc < nchA) {
      src = (const T*)a.srcA; C = a.CA; coff = kc * E::CH;
    } else {
      src = (const T*)a.srcB; C = a.CB; coff = (kc - nchA) * E::CH;
    }
    const T* const base = src + coff + pc * E::VEC;
    pvalid = 0;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      // patch_pixel<HALO> in this kernel's own text: through the helper <float,1,4,4,2,2,1,2,false> takes 171 registers
      // instead of 167 and loses its third wave
      const int gy = y0 + (prel[i] >> 8) - HALO, gx = x0 + (prel[i] & 255) - HALO;
      const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
      const int cy = ok ? gy : y0, cx = ok ? gx : x0;      // clamp to the tile origin: always a valid pixel
      const int lin = a.unshuf ? ((b * 2 * H + 2 * cy) * 2 * W + 2 * cx) : ((b * H + cy) * W + cx);
      preg[i] = *(const u32x4*)(base + (size_t)(lin + tapadd) * C);
      pvalid |= (ok ? 1u : 0u) << i;
    }
    if (PRO) {
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) {
        psc[j] = a.scale[coff + pc * E::VEC + j];
        psh[j] = a.shift[coff + pc * E::VEC + j];
      }
    }
  };
  auto store_patch = [&](int pboff) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const u32x4 v = patch_transform<T, PRO>(preg[i], psc, psh, (pvalid >> i) & 1);
      const int off = plds[i] + ((plds[i] < MAINB) ? pboff : 0);
      *(u32x4*)(smem + off) = v;
    }
  };
  auto load_w = [&](int s, int n0) {
    const int kc = s / SPC, tg = s - kc * SPC;
    const char* wb = (const char*)a.w + ((size_t)(kc * NTAPS + tg * TPS) * a.Ntot + n0) * 64;
#pragma unroll
    for (int i = 0; i < NWL; ++i) wreg[i] = *(const u32x4*)(wb + wsrc[i]);
  };
  auto store_w = [&](int par) {
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
      const int off = wlds[i] + ((wlds[i] < MAINB) ? par * WB : 0);
      *(u32x4*)(smem + off) = wreg[i];
    }
  };

  f32x16 acc[MF][NF];
  auto zero_acc = [&]() {
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mf][nf][r] = 0.f;
  };

  // ---- epilogue (entered right after a barrier: nobody reads the staging LDS any more).
  // FULL = the whole tile lies inside the image (the common case): no per-element bounds tests.
  auto epilogue_t = [&](auto FULLc) {
    constexpr bool FULL = decltype(FULLc)::value;
    stage_wave32<T, TWL, BN, MF, NF, FULL, GEO == 1>(a, acc, smem, (float*)(smem + L::RED), wm, wn, lane, un0, uy0, ux0);
    __syncthreads();
    reduce_stat_rows<WM, BN>(a, (const float*)(smem + L::RED), tid, umt, un0);
    store_staged_tile<T, TWL, BM, BN, NTHR, FULL, true>(a, smem, tid, ub, uy0, ux0, un0);
  };
  auto epilogue = [&]() {
    if ((uy0 + TH <= H) && (ux0 + TW <= W)) epilogue_t(std::true_type{});
    else epilogue_t(std::false_type{});
  };

  // ---- first unit: stage chunk 0 / step 0
  decode(u, umt, ub, uy0, ux0, un0);
  zero_acc();
  load_patch(0, ub, uy0, ux0);
  load_w(0, un0);
  store_patch(0);
  store_w(0);
  __syncthreads();

  for (;;) {
    const int un = u + GW;
    const bool has_next = un < u_end;
    int nmt = 0, nb = 0, ny0 = 0, nx0 = 0, nn0 = 0;
    if (has_next) decode(un, nmt, nb, ny0, nx0, nn0);

    int kc = 0, tg = 0;
    for (int s = 0; s < nsteps; ++s) {
      const bool last_step = (s + 1 == nsteps);
      const bool more_chunks = (kc + 1 < nchunks);
      // issue-early: next weight step (wrapping into the next unit) and, at a chunk's first step, the next
      // patch chunk (the next unit's chunk 0 during the last chunk)
      if (!last_step) load_w(s + 1, un0);
      else if (has_next) load_w(0, nn0);
      if (tg == 0) {
        if (more_chunks) load_patch(kc + 1, ub, uy0, ux0);
        else if (has_next) load_patch(0, nb, ny0, nx0);
      }
      const char* pb = patch0 + (PBUF == 2 ? (kc & 1) * PB : 0) + (GEO == 0 ? tg * ROWP : 0);
      const char* wb = wbuf0 + (s & 1) * WB;
      mma_taps<T, TPS, ROWP, BN * PIXB>(pb, wb, laneA, laneB, acc);   // fragment reads one sub-step ahead of the MFMAs
      // write-late: the data issued above (or a step / chunk earlier) lands in the other LDS buffers
      if (!last_step) store_w((s + 1) & 1);
      if (tg == SPC - 1 && more_chunks && PBUF == 2) store_patch(((kc + 1) & 1) * PB);
      __syncthreads();
      if (tg == SPC - 1 && more_chunks && PBUF == 1) {
        store_patch(0);
        __syncthreads();
      }
      if (++tg == SPC) { tg = 0; ++kc; }
    }
    epilogue();
    if (!has_next) break;
    __syncthreads();                 // the epilogue's LDS reads are done: staging LDS may be rewritten
    store_w(0);                      // next unit's step 0 (buffer parity restarts at 0)
    store_patch(0);                  // next unit's chunk 0
    zero_acc();
    u = un; umt = nmt; ub = nb; uy0 = ny0; ux0 = nx0; un0 = nn0;
    __syncthreads();
  }
}

template <typename T, int GEO, int TWL, int WM, int WN, int MF, int NF, int PBUF, bool PRO>
int launch_pro(ConvArgs a, const ConvPlan& p, hipStream_t st) {
  using L = IgemmLayout<T, GEO, TWL, WM, WN, MF, NF, PBUF>;
  constexpr size_t lds = L::LDS;
  static_assert(lds <= 160 * 1024, "conv_igemm: LDS exceeds 160 KiB");
  SEGK_REQUIRE_PLAN_TILE("conv_igemm", p, L::BM, TWL);
  // persistent grid: as many workgroups per CU as LDS allows (the register budget allows 2 x 8 waves)
  int wg_per_cu = (int)((160 * 1024) / lds);
  const int wg_cap = (L::NTHR == 512) ? 1 : 2;
  if (wg_per_cu > wg_cap) wg_per_cu = wg_cap;
  const int gw = conv_unit_grid(conv_set_tiles<L>(a, TWL) * (a.Ntot / L::BN), wg_per_cu);
  return segk_launch_lds<conv_igemm_kernel<T, GEO, TWL, WM, WN, MF, NF, PBUF, PRO>>("conv_igemm", 160 * 1024, dim3(8 * gw),
                                                                                     dim3(L::NTHR), lds, st, a);
}

template <typename T, int GEO>
int launch_geo(const ConvArgs& a, hipStream_t st) {
  constexpr bool BF = sizeof(T) == 2;
  const int dtype = BF ? SEGK_DT_BF16 : SEGK_DT_F32, cin = a.CA + a.CB;
  GemmArgs g{};
  const int mode = a.shuffle ? 1 : (a.unshuf ? 2 : 0);
  bool gemm_dma = false;
  if constexpr (GEO == 1 && BF) {
    g.A = a.srcA; g.w = (const char*)a.w; g.bias = a.bias; g.out = a.out;
    g.M = (long)a.B * a.H * a.W; g.N = a.Ntot; g.nchA = a.CA / 32; g.nchunks = a.unshuf ? 4 * g.nchA : g.nchA; g.lda = a.CA;
    g.H = a.H; g.W = a.W; g.Cout = a.CO1; g.act = a.act;
    gemm_dma = !a.srcB && !a.out2 && !a.stats && segk_gemm_dma_ok(g.M, g.nchunks, g.nchA, g.N, g.Cout, g.lda, mode);
  }
  const ConvPlan p = segk_conv_plan(GEO, dtype, cin, a.Ntot, a.W, a.bias != nullptr, gemm_dma);
  // segk_conv_tiles() does not know the bias.  A biased conv_rs shape is served by the weight-stationary kernel, whose
  // statistics rows are per tile while the query sized the buffer for conv_rs: the combination is refused instead of
  // overrunning it
  SEGK_REQUIRE(!a.stats || p.rs_rows == segk_conv_plan(GEO, dtype, cin, a.Ntot, a.W, false, gemm_dma).rs_rows,
               "conv3x3: bias together with BatchNorm statistics is not served for this layer shape");
  // run-time fields of the plan (and the prologue flag of the call) -> template arguments
  auto by_wide = [&](auto f) { return p.wide ? f(std::true_type{}) : f(std::false_type{}); };
  auto by_pro = [&](auto f) {
    if constexpr (GEO == 0) {                     // the BatchNorm prologue is a 3x3 feature
      if (a.scale) return f(std::true_type{});
    }
    return f(std::false_type{});
  };
  switch (p.form) {
    case CONV_RS:
      if constexpr (GEO == 0 && BF) return segk_conv_rs_launch(a, p, st);
      break;
    case CONV_WS:
      if constexpr (GEO == 0 && BF) return segk_conv_ws_launch(a, p, st);
      break;
    case CONV_PIPE:
      if constexpr (GEO == 0 && BF) return segk_conv_pipe_launch(a, p, st);
      break;
    case CONV_GEMM_DMA:
      if constexpr (GEO == 1 && BF) return segk_gemm_dma_launch(g, mode, st);
      break;
    case CONV_GENERIC: {
      // the template arguments are generic_tile's at the plan's (unit, wide), evaluated at compile time
      auto by_unit = [&](auto UNITc) {
        return by_wide([&](auto WIDEc) {
          return by_pro([&](auto PROc) {
            constexpr GenericTile G = generic_tile(GEO, BF, decltype(UNITc)::value, decltype(WIDEc)::value);
            if constexpr (G.wm != 0)
              return launch_pro<T, GEO, G.twl, G.wm, G.wn, G.mf, G.nf, G.pbuf, decltype(PROc)::value>(a, p, st);
            else
              SEGK_FAIL(-2, "conv_igemm: no generic kernel for a bf16 3x3 layer with N %% 128 == 0");
          });
        });
      };
      return p.unit == 128 ? by_unit(std::integral_constant<int, 128>{})
           : p.unit == 64 ? by_unit(std::integral_constant<int, 64>{})
                          : by_unit(std::integral_constant<int, 32>{});
    }
  }
  SEGK_FAIL(-2, "conv_igemm: the plan names a kernel form (%d) that this geometry and dtype do not compile", (int)p.form);
}

}  // namespace

int segk_conv_igemm_launch(const ConvArgs& a, int geo, int dtype, hipStream_t st) {
  using F = ET<float>;
  using H = ET<bf16_t>;
  const int CH = (dtype == SEGK_DT_BF16) ? H::CH : F::CH;
  SEGK_REQUIRE_DTYPE("conv_igemm", dtype);
  SEGK_REQUIRE(geo == 0 || geo == 1, "conv_igemm: bad geometry %d", geo);
  SEGK_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0, "conv_igemm: bad shape B=%d H=%d W=%d", a.B, a.H, a.W);
  SEGK_REQUIRE(a.srcA && a.w && a.out, "conv_igemm: null pointer");
  SEGK_REQUIRE(a.CA > 0 && a.CA % CH == 0, "conv_igemm: CA=%d must be a positive multiple of %d", a.CA, CH);
  SEGK_REQUIRE(a.CB >= 0 && a.CB % CH == 0 && (a.CB == 0) == (a.srcB == nullptr), "conv_igemm: bad second source");
  SEGK_REQUIRE(!(a.unshuf && (a.CB || geo != 1)), "conv_igemm: un-shuffle gather needs geo 1, single source");
  SEGK_REQUIRE(!(a.scale && (a.CB || geo != 0)), "conv_igemm: BN prologue needs the 3x3 geometry and one source");
  SEGK_REQUIRE((a.scale == nullptr) == (a.shift == nullptr), "conv_igemm: scale/shift must come together");
  SEGK_REQUIRE(!a.act_out || (a.scale && geo == 0 && segk_conv_writes_act(a.CA + a.CB, a.Ntot, dtype)),
               "conv_igemm: act_out needs the BN prologue and a layer served by the producer/consumer or weight-stationary kernel");
  SEGK_REQUIRE(a.Ntot > 0 && a.Ntot % 32 == 0, "conv_igemm: N=%d must be a multiple of 32", a.Ntot);
  SEGK_REQUIRE(a.CO1 > 0 && a.CO1 % 32 == 0 && a.CO2 >= 0 && a.CO2 % 32 == 0, "conv_igemm: bad output channels");
  if (a.shuffle) SEGK_REQUIRE(a.Ntot == 4 * a.CO1 && !a.out2 && geo == 1, "conv_igemm: pixel-shuffle needs N=4*Cout");
  else SEGK_REQUIRE(a.Ntot == a.CO1 + a.CO2 && (a.CO2 == 0) == (a.out2 == nullptr), "conv_igemm: N != CO1+CO2");
  SEGK_REQUIRE((long long)a.B * a.H * a.W * 4 < 2147483647LL, "conv_igemm: pixel index overflows int32");
  if (dtype == SEGK_DT_BF16) return geo == 0 ? launch_geo<bf16_t, 0>(a, st) : launch_geo<bf16_t, 1>(a, st);
  return geo == 0 ? launch_geo<float, 0>(a, st) : launch_geo<float, 1>(a, st);
}
