// What the convolution kernels share, stated once: conv_igemm_kernel (conv_igemm.hip), conv3x3_pipe_kernel
// (conv_pipe.hip), conv_ws_kernel (conv_ws.hip) and conv_rs_kernel (conv_rs.hip); gemm.hip takes the weight-row swizzle and
// the address-space typedefs.  Everything here is address arithmetic or a barrier-free pass: barriers, counted waits,
// sched_barrier placement and the roles of the waves stay in each kernel's own text.
// Internal linkage throughout: every unit gets its own copy, and its kernels keep their anonymous-namespace names.
#pragma once
#include <type_traits>
#include "common.hpp"
#include "segk_internal.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

constexpr int PIXB = 80;  // LDS pitch of one pixel's 64-byte K-chunk: +16 B pad -> conflict-free ds_read_b128

// out-of-image pixels of the LDS-DMA forms are fetched from here (a device array of the code object: nothing is allocated)
__device__ __attribute__((aligned(256), unused)) unsigned char g_conv_zero_page[256];

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                  acc, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  // lane (r, h) supplies k-slot h of each of the four 32x32x2 products: floats [4h + j] of the 8-float block
  static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
};

// ---- LDS layouts: the kernel addresses with the record its launcher sizes the launch with ---------------------------------------
// pixel tile of BM pixels, 1 << TWL wide, with its halo; ROWP: patch row pitch at PPIX bytes per pixel, a multiple of 256 B
// (two-row fragments stay conflict-free)
template <int BM_, int TWL, int HALO, int PPIX = PIXB> struct PatchTile {
  static constexpr int BM = BM_, TW = 1 << TWL, TH = BM >> TWL, PW = TW + 2 * HALO, PH = TH + 2 * HALO;
  static constexpr int ROWP = (PW * PPIX + 255) & ~255, PB = PH * ROWP;
  static constexpr int NP = PH * PW * 4;             // 16-byte pieces of one chunk of the patch
};
// the staged epilogue: [BM pixels][BN channels + 16 B] output tile, then WM rows of per-channel (sum, sum of squares)
template <typename T, int BM, int BN, int WM> struct EpiTile {
  static constexpr int OP = BN * ET<T>::ES + 16, RED = BM * OP, BYTES = RED + WM * BN * 8;
};
// conv_igemm_kernel: [PBUF patch chunks | 2 weight steps | one 16-byte trash slot per thread], overlaid by the epilogue tile
template <typename T, int GEO, int TWL, int WM, int WN, int MF, int NF, int PBUF>
struct IgemmLayout : PatchTile<WM * MF * 32, TWL, GEO == 0 ? 1 : 0>, EpiTile<T, WM * MF * 32, WN * NF * 32, WM> {
  using P = PatchTile<WM * MF * 32, TWL, GEO == 0 ? 1 : 0>;
  static constexpr int BN = WN * NF * 32, NTHR = WM * WN * 64;
  static constexpr int TPS = GEO == 0 ? 3 : 1;       // taps per pipeline step (one kernel row)
  static constexpr int WB = TPS * BN * PIXB, MAINB = PBUF * P::PB + 2 * WB;
  static constexpr size_t LDS = MAINB + NTHR * 16 > IgemmLayout::BYTES ? MAINB + NTHR * 16 : IgemmLayout::BYTES;
};
// conv_ws_kernel: [2 patch chunks | 2 x 9 weight taps | trash slots]; the epilogue tile overlays the patch
template <typename T, int TWL> struct WsLayout : PatchTile<256, TWL, 1>, EpiTile<T, 256, 64, 4> {
  using P = PatchTile<256, TWL, 1>;
  static constexpr int BN = 64, NTHR = 512, MAXCH = 2, WTAP = BN * PIXB;
  static constexpr int WOFF = MAXCH * P::PB, MAINB = WOFF + MAXCH * 9 * WTAP;
  static constexpr size_t LDS = MAINB + NTHR * 16;
  static_assert(WsLayout::BYTES <= WOFF, "output staging tile fits in the patch region");
};
// conv3x3_pipe_kernel: [W0 | W1 | P0 | P1 | W2], then the producers' trash slots (staged form; the epilogue tile overlays
// [P0 | P1 | W2]) or one trash KiB and the statistics exchange [4 waves][64 ch][2] floats + one flag per wave (DMA form)
template <int TWL, int BN_, bool DMA> struct PipeLayout : PatchTile<32768 / BN_, TWL, 1, 96>, EpiTile<bf16_t, 32768 / BN_, BN_, 4 / (BN_ / 64)> {
  using P = PatchTile<32768 / BN_, TWL, 1, 96>;
  static constexpr int BN = BN_, NTHR = 512, NPT = 256, WPIX = 64, PPIX = DMA ? 64 : 96;
  static constexpr int RPX = (P::PW + 7) & ~7;       // DMA image: pixel slots per patch row (whole 8-pixel blocks)
  static constexpr int ROWP = DMA ? RPX * 64 : P::ROWP, PB = P::PH * ROWP;
  static constexpr int WB = 3 * BN * WPIX;           // one step of weights: 3 taps x BN rows
  static constexpr int POFF = 2 * WB, W2OFF = POFF + 2 * PB, MAINB = W2OFF + WB;
  static constexpr int STOFF = MAINB + 1024;
  static constexpr size_t LDS = DMA ? STOFF + 4 * 64 * 8 + 64 : MAINB + NPT * 16;
  static_assert(DMA || PipeLayout::BYTES <= MAINB - POFF, "epilogue tile fits behind the live ring slots");
};

// ---- the unit walk: every XCD owns a contiguous range, walked by its workgroups with a fixed stride ---------------------------
// (unit) variant: U units of (pixel tile x channel tile); this workgroup takes u, u + GW, ... below u_end
struct UnitWalk { int u, u_end, GW; };
__device__ __forceinline__ UnitWalk unit_walk(int U) {
  const int xcd = blockIdx.x & 7, upx = (U + 7) >> 3;
  return {xcd * upx + (int)(blockIdx.x >> 3), min(U, (xcd + 1) * upx), (int)(gridDim.x >> 3)};
}
// (pixel tile, fixed channel tile) variant: the workgroup keeps channel tile nt and takes pixel tiles mt, mt + GW, ...
// below mt_end; (xcd, slot) number the workgroups of one channel tile
struct TileWalk { int mt, mt_end, GW, nt, xcd, slot; };
__device__ __forceinline__ TileWalk tile_walk(int MT, int NT) {
  const int xcd = blockIdx.x & 7, wgi = blockIdx.x >> 3, GWX = gridDim.x >> 3;
  const int slot = wgi / NT, mpx = (MT + 7) >> 3;
  return {xcd * mpx + slot, min(MT, (xcd + 1) * mpx), GWX / NT, wgi % NT, xcd, slot};
}
// pixel tile m -> image and tile origin
template <int TW, int TH> __device__ __forceinline__ void decode_tile(const ConvArgs& a, int tpi, int m, int& b, int& y0, int& x0) {
  b = m / tpi;
  const int trem = m - b * tpi;
  const int tyi = trem / a.tiles_x;
  y0 = tyi * TH;
  x0 = (trem - tyi * a.tiles_x) * TW;
}
// unit uu -> pixel tile mt (decoded) and channel origin n0
template <int TW, int TH, int BN>
__device__ __forceinline__ void decode_unit(const ConvArgs& a, int NT, int tpi, int uu, int& mt, int& b, int& y0, int& x0, int& n0) {
  mt = uu / NT;
  n0 = (uu - mt * NT) * BN;
  decode_tile<TW, TH>(a, tpi, mt, b, y0, x0);
}

// ---- the register-staged patch --------------------------------------------------------------------------------------------------
// 16-byte piece q of a chunk: pixel q >> 2 of the patch, row-major.  Returns (py << 8) | px, or row 32767 -- outside every
// image, never valid -- for a piece past the patch, which its thread moves into a trash slot (no divergent staging)
constexpr int PREL_NEVER = 0x7fff << 8;
template <typename P> __device__ __forceinline__ int patch_piece(int q, int& py, int& px) {
  const int pix = q >> 2;
  py = pix / P::PW;
  px = pix - py * P::PW;
  return (q < P::NP) ? ((py << 8) | px) : PREL_NEVER;
}
// ... and whether it is an interior (non-halo) pixel of the tile
template <typename P> __device__ __forceinline__ bool patch_interior(int q, int py, int px) {
  return q < P::NP && py >= 1 && py <= P::TH && px >= 1 && px <= P::TW;
}
// the image pixel of a piece: in the image?  If not, (cy, cx) is the tile origin, always a valid pixel to load
struct PatchPixel { bool ok; int cy, cx; };
template <int HALO> __device__ __forceinline__ PatchPixel patch_pixel(int prel, int y0, int x0, int H, int W) {
  const int gy = y0 + (prel >> 8) - HALO, gx = x0 + (prel & 255) - HALO;
  const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
  return {ok, ok ? gy : y0, ok ? gx : x0};
}
// one piece on its way to LDS: BatchNorm(scale, shift) + ReLU of the producer layer (PRO), then exact zeros for an
// out-of-image halo pixel (after the transform)
template <typename T, bool PRO>
__device__ __forceinline__ u32x4 patch_transform(u32x4 v, const float (&psc)[ET<T>::VEC], const float (&psh)[ET<T>::VEC], bool ok) {
  if (PRO) {
    float f[ET<T>::VEC];
    unpack16<T>(make_uint4(v.x, v.y, v.z, v.w), f);
#pragma unroll
    for (int j = 0; j < ET<T>::VEC; ++j) f[j] = fmaxf(fmaf(f[j], psc[j], psh[j]), 0.f);
    const uint4 t = pack16<T>(f);
    v = (u32x4){t.x, t.y, t.z, t.w};
  }
  return ok ? v : (u32x4){0u, 0u, 0u, 0u};
}

// ---- conflict-free unpadded LDS images ------------------------------------------------------------------------------------------
// 64-byte weight rows: the 16-byte piece index is XOR-ed by [0,3,2,1][(row >> 2) & 3]
__host__ __device__ __forceinline__ constexpr int wswz(int row) { return (0x1230 >> (4 * ((row >> 2) & 3))) & 3; }
// LDS-DMA patch: rows of 8-pixel blocks of 512 B, piece q of pixel p (conflict-free for a 16-pixel operand read at any shift)
__device__ __forceinline__ int dma_slot(int p, int q) { return (p >> 3) * 512 + (q >> 1) * 256 + ((6 * p + q) & 15) * 16; }
// ... and its inverse for the DMA instruction, whose lane l writes slot l of a 16-pixel KiB: l -> (pixel of the 16, piece)
__device__ __forceinline__ void dma_slot_lane(int l, int& q, int& p) {
  const int lb = l >> 5, lh = (l >> 4) & 1, ls = l & 15;
  q = 2 * lh + (ls & 1);
  p = 8 * lb + ((3 * ((ls >> 1) - lh)) & 7);
}

// ---- the 32x32 kernels: fragment loop and staged epilogue ---------------------------------------------------------------------
// NTAP taps x two MFMA k-steps against LDS, the fragment reads of sub-step i + 1 issued BEFORE the MFMAs of sub-step i
// (register double buffer), so LDS latency hides under the matrix pipe.  pb / wb: the patch row and weight tap of sub-step 0;
// tap t sits t % 3 pixels and t / 3 patch rows further, its weights WTAP bytes per tap further.
template <typename T, int NTAP, int ROWP, int WTAP, int MF, int NF>
__device__ __forceinline__ void mma_taps(const char* pb, const char* wb, const int (&laneA)[MF], const int (&laneB)[NF],
                                         f32x16 (&acc)[MF][NF]) {
  constexpr int NSUB = NTAP * 2;
  uint4 fa[2][MF], fb[2][NF];
  auto rd = [&](int i, uint4 (&A)[MF], uint4 (&Bf)[NF]) {
    const int t = i >> 1, kk = i & 1;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) A[mf] = *(const uint4*)(pb + laneA[mf] + (t / 3) * ROWP + (t % 3) * PIXB + kk * 32);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) Bf[nf] = *(const uint4*)(wb + laneB[nf] + t * WTAP + kk * 32);
  };
  rd(0, fa[0], fb[0]);
#pragma unroll
  for (int i = 0; i < NSUB; ++i) {
    if (i + 1 < NSUB) rd(i + 1, fa[(i + 1) & 1], fb[(i + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);   // keep the prefetch reads ahead of this sub-step's MFMAs
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) Mma<T>::run(fa[i & 1][mf], fb[i & 1][nf], acc[mf][nf]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// one wave's MF x NF fragments -> the staging tile `ot`, with the bias (and, ACT, the quick_gelu of the CLIP MLP); pixels
// past the image edge (!FULL) are never stored and must not enter the statistics: they are staged as zeros.  The wave's
// per-channel partial sums go to row wm of `red` when the call takes statistics.  (wm, wn): the wave; tile origin (uy0, ux0).
template <typename T, int TWL, int BN, int MF, int NF, bool FULL, bool ACT>
__device__ __forceinline__ void stage_wave32(const ConvArgs& a, const f32x16 (&acc)[MF][NF], char* ot, float* red, int wm, int wn,
                                             int lane, int n0, int uy0, int ux0) {
  constexpr int OP = BN * ET<T>::ES + 16, TW = 1 << TWL;
  const int lr = lane & 31, lh = lane >> 5;
  const bool do_stats = (a.stats != nullptr);
  float s1[NF], s2[NF];
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    s1[nf] = 0.f;
    s2[nf] = 0.f;
    const int n = (wn * NF + nf) * 32 + lr;
    const float bv = a.bias ? a.bias[n0 + n] : 0.f;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      const int mb = (wm * MF + mf) * 32 + 4 * lh;
      char* const obase = ot + mb * OP + n * ET<T>::ES;
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        v[r] = acc[mf][nf][r] + bv;
        if constexpr (ACT) {   // quick_gelu(x) = x * sigmoid(1.702 x) fused behind fc1 (segk_linear)
          if (a.act) v[r] = v[r] / (1.f + __expf(-1.702f * v[r]));
        }
        if (!FULL) {
          const int m = mb + (r & 3) + 8 * (r >> 2);
          v[r] = ((uy0 + (m >> TWL) < a.H) && (ux0 + (m & (TW - 1)) < a.W)) ? v[r] : 0.f;
        }
      }
      stage_frag<T>(v, obase, OP, s1[nf], s2[nf]);
    }
  }
  if (do_stats) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      s1[nf] += __shfl_xor(s1[nf], 32);
      s2[nf] += __shfl_xor(s2[nf], 32);
      if (lh == 0) {
        const int n = (wn * NF + nf) * 32 + lr;
        red[(wm * BN + n) * 2 + 0] = s1[nf];
        red[(wm * BN + n) * 2 + 1] = s2[nf];
      }
    }
  }
}
// behind the barrier that publishes the staged tile: the unit's statistics row, the WM partial rows added in fixed order
// (bit-stable) ...
template <int WM, int BN>
__device__ __forceinline__ void reduce_stat_rows(const ConvArgs& a, const float* red, int tid, int mt, int n0) {
  if (a.stats != nullptr && tid < BN) {
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int w = 0; w < WM; ++w) {
      t1 += red[(w * BN + tid) * 2 + 0];
      t2 += red[(w * BN + tid) * 2 + 1];
    }
    float2* dst = (float2*)a.stats + (size_t)mt * a.Ntot + n0 + tid;
    *dst = make_float2(t1, t2);
  }
}
// ... and the tile itself in 16-byte pieces, coalesced along the channels: NHWC with the channels split over out (CO1) and
// out2 (CO2), or (SHUF and a.shuffle) pixel-shuffled for ConvTranspose2d(k=2,s=2): N = (a*2+c)*Cout + co -> pixel (2y+a, 2x+c)
template <typename T, int TWL, int BM, int BN, int NTHR, bool FULL, bool SHUF>
__device__ __forceinline__ void store_staged_tile(const ConvArgs& a, const char* ot, int tid, int ub, int uy0, int ux0, int un0) {
  using E = ET<T>;
  constexpr int OP = BN * E::ES + 16, TW = 1 << TWL;
  constexpr int CPR = BN * E::ES / 16;   // 16-byte chunks per pixel row of the tile
  constexpr int NST = BM * CPR / NTHR;
  static_assert(BM * CPR % NTHR == 0 && (CPR & (CPR - 1)) == 0, "store loop is exact");
  const int H = a.H, W = a.W;
  const int cc = tid & (CPR - 1);
  const int n = un0 + cc * E::VEC;
  // destination of this thread's channel slice at the tile origin, and the element strides per pixel step in x / row step in y
  T* dbase;
  size_t pstride, rstride;
  if (SHUF && a.shuffle) {
    const int tq = n / a.CO1, co = n - tq * a.CO1;   // per thread: a channel tile may span several taps
    dbase = (T*)a.out + (((size_t)(ub * 2 * H + 2 * uy0 + (tq >> 1))) * (2 * W) + 2 * ux0 + (tq & 1)) * a.CO1 + co;
    pstride = 2 * (size_t)a.CO1;
    rstride = 4 * (size_t)W * a.CO1;
  } else {
    const size_t pix0 = ((size_t)(ub * H + uy0)) * W + ux0;
    if (n < a.CO1) { dbase = (T*)a.out + pix0 * a.CO1 + n; pstride = a.CO1; }
    else { dbase = (T*)a.out2 + pix0 * a.CO2 + (n - a.CO1); pstride = a.CO2; }
    rstride = (size_t)W * pstride;
  }
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const int m = (tid + i * NTHR) / CPR;
    const int ty = m >> TWL, tx = m & (TW - 1);
    const uint4 v = *(const uint4*)(ot + m * OP + cc * 16);
    if (FULL || (uy0 + ty < H && ux0 + tx < W)) *(uint4*)(dbase + ty * rstride + tx * pstride) = v;
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
// the tile a launcher was instantiated for is the plan's, which sized the caller's statistics buffer
#define SEGK_REQUIRE_PLAN_TILE(name, p, BM, TWL) \
  SEGK_REQUIRE((p).bm == (BM) && (p).twl == (TWL), name ": instantiated for a %d-pixel tile (twl %d), the plan says %d (twl %d)", BM, TWL, (p).bm, (p).twl)
// tiles of the image -> pixel tiles of the call
template <typename P> inline int conv_set_tiles(ConvArgs& a, int twl) {
  a.twl = twl;
  a.tiles_x = cdiv(a.W, P::TW);
  a.tiles_y = cdiv(a.H, P::TH);
  return a.B * a.tiles_x * a.tiles_y;
}
// workgroups per XCD of a unit-walk kernel: wg_per_cu per CU, capped by the units an XCD owns
inline int conv_unit_grid(int units, int wg_per_cu) {
  const int per_xcd = (units + 7) / 8;
  const int gw = (segk_num_cus() / 8) * wg_per_cu;
  return gw > per_xcd ? per_xcd : gw;
}

}  // namespace
