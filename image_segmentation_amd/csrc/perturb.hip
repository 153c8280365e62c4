// Robustness perturbations on the device (report section 4.1, figure 6: eight perturbation types at ten severity levels; the
// reference holds no code for them, the arithmetic is this project's definition: DESIGN.md section 3).
//
// Images stay 8-bit interleaved [H][W][3] at their own sizes -- what a decoder hands out and segk_resize_pad_u8 consumes next.
// Every value that decides a result is an INTEGER: the host builds the tables (value LUT, Gaussian inverse CDF) and draws the
// per-image seeds and occlusion corners; the kernels combine them with integer arithmetic only, so the bytes do not depend on
// the tiling and equal the NumPy restatement of tests/perturb_reference.py.
//
//  perturb_point_kernel<KIND>  the four pointwise kinds; an image is a run of H W 3 bytes, a tile is 4096 of them, a lane
//                              owns 16 consecutive bytes: one 16-byte load and store when the pointers allow, bytes otherwise
//                              (4-channel or misaligned sources, the last lanes of an image).
//  perturb_blur_kernel         k passes of [1 2 1; 2 4 2; 1 2 1] / 16 in LDS: a 32 x 64 pixel tile with a halo of k, reflected
//                              once at load (a lane loads one byte column, all its rows in flight together); in a pass a lane
//                              owns four consecutive bytes of a row (one LDS dword, the sums as two 16-bit fields per
//                              register) and walks down a band of rows with a sliding window of three unrounded horizontal
//                              sums; the region shrinks by one pixel per pass; the centre leaves as aligned dwords.
//
// One launch serves a ragged batch: a workgroup finds its image by a binary search of tile0 in the descriptor table.  The table
// is device data the entry points cannot see: sizes and tile ranges are checked before they become addresses.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int K_LUT = SEGK_PERTURB_LUT, K_GAUSS = SEGK_PERTURB_GAUSS_NOISE, K_SP = SEGK_PERTURB_SALT_PEPPER,
              K_OCC = SEGK_PERTURB_OCCLUDE;
constexpr int GAUSS_N = SEGK_PERTURB_GAUSS_ENTRIES;
constexpr int PT_TILE = SEGK_PERTURB_POINT_TILE;              // 256 lanes x 16 bytes
constexpr int BK = SEGK_PERTURB_BLUR_MAX, BTH = SEGK_PERTURB_BLUR_TH, BTW = SEGK_PERTURB_BLUR_TW;
constexpr int BR = BTH + 2 * BK;                               // 50 rows
constexpr int BC = (BTW + 2 * BK) * 3;                         // 246 byte columns: one lane each
constexpr int BQ = 64;                                         // row pitch in dwords: a pad dword, 246 bytes, pad
static_assert(PT_TILE == 256 * 16 && BC <= 256 && 4 + BC + 4 <= BQ * 4 && (BC + 3) / 4 + 1 < BQ, "tile geometry");

// the last entry whose first tile is <= tile (entries are sorted by tile0); block-uniform
__device__ __forceinline__ int find_desc(const segk_perturb_desc* __restrict__ descs, int n, int tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------ pointwise kinds
template <int KIND>
__global__ __launch_bounds__(256) void perturb_point_kernel(const segk_perturb_desc* __restrict__ descs, int n,
                                                            const void* __restrict__ table) {
  __shared__ unsigned s_tab[KIND == K_GAUSS ? GAUSS_N / 2 : KIND == K_LUT ? 64 : 1];
  const int tid = threadIdx.x;
  if constexpr (KIND == K_GAUSS) {
    const unsigned* t = (const unsigned*)table;
    unsigned w[GAUSS_N / 512];
#pragma unroll
    for (int u = 0; u < GAUSS_N / 512; ++u) w[u] = t[u * 256 + tid];
#pragma unroll
    for (int u = 0; u < GAUSS_N / 512; ++u) s_tab[u * 256 + tid] = w[u];
    __syncthreads();
  } else if constexpr (KIND == K_LUT) {
    ((uint8_t*)s_tab)[tid] = ((const uint8_t*)table)[tid];
    __syncthreads();
  }
  const segk_perturb_desc& d = descs[find_desc(descs, n, blockIdx.x)];
  const int H = d.H, W = d.W;
  const uint8_t* __restrict__ src = d.src;
  uint8_t* __restrict__ dst = d.dst;
  if (H < 1 || W < 1 || !src || !dst) return;
  const long long N = (long long)H * W * 3;
  const long long t_loc = (long long)blockIdx.x - d.tile0;
  if (N >= (1LL << 31) || t_loc < 0 || t_loc * PT_TILE >= N) return;
  const unsigned Nu = (unsigned)N, base = (unsigned)t_loc * PT_TILE + tid * 16;
  if (base >= Nu) return;
  const int sc = d.src_c == 4 ? 4 : 3;
  const bool full = base + 16 <= Nu;

  int v[16];
  if (full && sc == 3 && ((uintptr_t)src & 15) == 0) {
    const uint4 q = *(const uint4*)(src + base);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (w[j >> 2] >> (8 * (j & 3))) & 255;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {                         // clamped addresses: 16 loads in flight together
      const unsigned e = base + j < Nu ? base + j : Nu - 1;
      v[j] = src[sc == 3 ? (size_t)e : (size_t)(e / 3) * 4 + e % 3];
    }
  }

  if constexpr (KIND == K_LUT) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = ((const uint8_t*)s_tab)[v[j]];
  } else if constexpr (KIND == K_GAUSS) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = clampi(v[j] + ((const short*)s_tab)[splitmix(d.seed, base + j) >> 52], 0, 255);
  } else if constexpr (KIND == K_SP) {
    const unsigned thr = (unsigned)d.p0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned long long h = splitmix(d.seed, base + j);
      v[j] = (unsigned)(h >> 40) < thr ? (((h >> 39) & 1) ? 255 : 0) : v[j];
    }
  } else {
    const int y0 = d.p0, x0 = d.p1, e = d.p2;
    const unsigned pix = base / 3;
    int c = (int)(base - pix * 3), y = (int)(pix / (unsigned)W), x = (int)(pix - (unsigned)y * (unsigned)W);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (y >= y0 && y - y0 < e && x >= x0 && x - x0 < e) v[j] = 0;
      if (++c == 3) {
        c = 0;
        if (++x == W) { x = 0; ++y; }
      }
    }
  }

  if (full && ((uintptr_t)dst & 15) == 0) {
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= (unsigned)v[j] << (8 * (j & 3));
    *(uint4*)(dst + base) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (base + j < Nu) dst[base + j] = (uint8_t)v[j];
  }
}

// ------------------------------------------------------------------------------------------------ blur
// even / odd bytes of a dword as two 16-bit fields each: four bytes are summed with two adds (no field passes 4088)
__device__ __forceinline__ void hsum4(unsigned l, unsigned c, unsigned r, unsigned& he, unsigned& ho) {
  const unsigned left = __builtin_amdgcn_alignbyte(c, l, 1);    // bytes -3 .. 0 of the lane's dword
  const unsigned right = __builtin_amdgcn_alignbyte(r, c, 3);   // bytes +3 .. +6
  const unsigned m = 0x00ff00ffu;
  he = (left & m) + 2 * (c & m) + (right & m);
  ho = ((left >> 8) & m) + 2 * ((c >> 8) & m) + ((right >> 8) & m);
}

__global__ __launch_bounds__(256) void perturb_blur_kernel(const segk_perturb_desc* __restrict__ descs, int n, int k) {
  // [buffer][row][dword]: the tile's byte column j lives at byte 4 + j of its row, so that every dword that holds data has
  // both neighbours in the row (dwords 0 and 63 are never written: what is read from them stays in the shrinking margin)
  __shared__ unsigned s_px[2][BR][BQ];
  __shared__ int s_row[BR];
  const int tid = threadIdx.x;
  const segk_perturb_desc& d = descs[find_desc(descs, n, blockIdx.x)];
  const int H = d.H, W = d.W;
  const uint8_t* __restrict__ src = d.src;
  uint8_t* __restrict__ dst = d.dst;
  if (H < 1 || W < 1 || !src || !dst || (long long)H * W * 3 >= (1LL << 31)) return;
  const int tiles_x = (W + BTW - 1) / BTW, tiles_y = (H + BTH - 1) / BTH;
  const long long t_loc = (long long)blockIdx.x - d.tile0;
  if (t_loc < 0 || t_loc >= (long long)tiles_x * tiles_y) return;
  const int ty = (int)t_loc / tiles_x, tx = (int)t_loc - ty * tiles_x;
  const int sc = d.src_c == 4 ? 4 : 3;
  const int R = BTH + 2 * k, CB = (BTW + 2 * k) * 3;           // rows and byte columns of the tile with its halo
  const int y0 = ty * BTH - k, x0 = tx * BTW - k;

  if (tid < BR) s_row[tid] = reflect101(y0 + (tid < R ? tid : R - 1), H);
  __syncthreads();
  if (tid < CB) {                                              // a lane loads one byte column: all rows in flight together
    const int c = tid / 3, ch = tid - c * 3;
    const uint8_t* col = src + (size_t)reflect101(x0 + c, W) * sc + ch;
    const size_t pitch = (size_t)W * sc;
    uint8_t v[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) v[r] = col[(size_t)s_row[r] * pitch];   // rows past R repeat row R - 1
#pragma unroll
    for (int r = 0; r < BR; ++r)
      if (r < R) ((uint8_t*)s_px[0][r])[4 + tid] = v[r];
  }
  __syncthreads();

  // a pass: wave w owns a band of the rows [p, R - p), lane q the dword 1 + q; three unrounded horizontal sums slide down
  const int q = 1 + (tid & 63), wv = tid >> 6;
  const bool lane_on = q <= (CB + 3) / 4;
  int cur = 0;
  for (int p = 1; p <= k; ++p) {                               // rows [p, R - p) x byte columns [3p, CB - 3p) stay exact
    const int rows = R - 2 * p, band = (rows + 3) >> 2;
    const int ra = p + wv * band, rb = ra + band < R - p ? ra + band : R - p;
    if (lane_on && ra < rb) {
      const unsigned(*in)[BQ] = s_px[cur];
      unsigned(*out)[BQ] = s_px[cur ^ 1];
      unsigned e0, o0, e1, o1, e2, o2;
      hsum4(in[ra - 1][q - 1], in[ra - 1][q], in[ra - 1][q + 1], e0, o0);
      hsum4(in[ra][q - 1], in[ra][q], in[ra][q + 1], e1, o1);
      for (int r = ra; r < rb; ++r) {
        hsum4(in[r + 1][q - 1], in[r + 1][q], in[r + 1][q + 1], e2, o2);
        const unsigned ve = ((e0 + 2 * e1 + e2 + 0x00080008u) >> 4) & 0x00ff00ffu;
        const unsigned vo = ((o0 + 2 * o1 + o2 + 0x00080008u) >> 4) & 0x00ff00ffu;
        out[r][q] = ve | (vo << 8);
        e0 = e1; o0 = o1; e1 = e2; o1 = o2;
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // the centre, as aligned dwords of the destination row where all four bytes belong to this tile, else byte by byte
  const int rowb = W * 3, xb0 = tx * BTW * 3;
  const int xb1 = xb0 + BTW * 3 < rowb ? xb0 + BTW * 3 : rowb;
  constexpr int SQ = BTW * 3 / 4 + 1;                          // aligned dwords that can touch 192 bytes
  for (int i = tid; i < BTH * SQ; i += 256) {
    const int ly = i / SQ, l = i - ly * SQ;
    const int y = ty * BTH + ly;
    if (y >= H) break;
    uint8_t* row = dst + (size_t)y * rowb;
    const int g0 = xb0 - (int)((uintptr_t)(row + xb0) & 3) + 4 * l;     // first byte column of an aligned dword
    const uint8_t* px = (const uint8_t*)s_px[cur][k + ly];
    const int o = 4 + 3 * k - xb0 + g0;                        // LDS byte of column g0
    if (g0 >= xb0 && g0 + 4 <= xb1) {
      const unsigned w = px[o] | (px[o + 1] << 8) | (px[o + 2] << 16) | ((unsigned)px[o + 3] << 24);
      *(unsigned*)(row + g0) = w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (g0 + j >= xb0 && g0 + j < xb1) row[g0 + j] = px[o + j];
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
static_assert(sizeof(segk_perturb_desc) == 56, "segk_perturb_desc is 56 bytes");

static int check_table(const char* what, const void* descs, int n, int total_tiles) {
  SEGK_REQUIRE(descs, "%s: NULL descriptor table", what);
  SEGK_REQUIRE(((uintptr_t)descs & 7) == 0, "%s: misaligned descriptor table", what);
  SEGK_REQUIRE(n >= 1 && n <= 65535, "%s: %d images (1..65535)", what, n);
  SEGK_REQUIRE(total_tiles >= 0 && total_tiles <= (1 << 30), "%s: total_tiles=%d (0..2^30)", what, total_tiles);
  return 0;
}

extern "C" int segk_perturb_point(const segk_perturb_desc* descs, int n, int total_tiles, int kind, const void* table,
                                  segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (int rc = check_table("perturb_point", descs, n, total_tiles)) return rc;
  SEGK_REQUIRE(kind == K_LUT || kind == K_GAUSS || kind == K_SP || kind == K_OCC, "perturb_point: unknown kind %d (0..3)", kind);
  const bool needs = kind == K_LUT || kind == K_GAUSS;
  SEGK_REQUIRE(!needs || table, "perturb_point: kind %d needs its table", kind);
  SEGK_REQUIRE(kind != K_GAUSS || ((uintptr_t)table & 3) == 0, "perturb_point: misaligned noise table");
  if (total_tiles == 0) return 0;
  const dim3 grid(total_tiles), block(256);
  if (kind == K_LUT) hipLaunchKernelGGL(perturb_point_kernel<K_LUT>, grid, block, 0, st, descs, n, table);
  else if (kind == K_GAUSS) hipLaunchKernelGGL(perturb_point_kernel<K_GAUSS>, grid, block, 0, st, descs, n, table);
  else if (kind == K_SP) hipLaunchKernelGGL(perturb_point_kernel<K_SP>, grid, block, 0, st, descs, n, table);
  else hipLaunchKernelGGL(perturb_point_kernel<K_OCC>, grid, block, 0, st, descs, n, table);
  SEGK_CHECK_LAUNCH("perturb_point");
  return 0;
}

extern "C" int segk_perturb_blur(const segk_perturb_desc* descs, int n, int total_tiles, int k, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (int rc = check_table("perturb_blur", descs, n, total_tiles)) return rc;
  SEGK_REQUIRE(k >= 0 && k <= BK, "perturb_blur: %d passes (0..%d: the halo one tile holds)", k, BK);
  if (total_tiles == 0) return 0;
  hipLaunchKernelGGL(perturb_blur_kernel, dim3(total_tiles), dim3(256), 0, st, descs, n, k);
  SEGK_CHECK_LAUNCH("perturb_blur");
  return 0;
}
