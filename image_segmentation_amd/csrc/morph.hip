// Mask morphology on the device: erode, dilate, open, close, the void band around label changes and
// the capped distance to the nearest different label are ONE integer primitive with a per-pixel write rule, segk_morph; hole
// filling is a byte table pass (segk_byte_lut), the labelling of components.hip and a small fill pass (segk_fill_holes).  The
// reference holds no code for this; the arithmetic is this project's definition, every value is an integer and the result is
// unique, so the device equals the restatement of tests/morph_reference.py bit for bit.
//
//  segk_morph       morph_kernel<METRIC>: one workgroup per tile of 64 rows x 128 columns
//                     stage    keys (16 bits, key[] of the pixel's byte; the wild key outside the image) of the tile and a halo
//                              of r cells on every side, in LDS
//                     columns  one thread per staged column, down then up: g = the vertical distance to the nearest live key
//                              that differs from the cell's own, saturating at r + 1 (a wild cell: to the nearest live key)
//                     rows     per pixel the minimum over dx in [-r, r] of dist(dx, 0) where the key at x + dx differs, else
//                              dist(dx, g(x + dx)); a wild cell inside the image is the one case the recurrence cannot serve
//                              (its g is not relative to p's key): its column is walked from g to r.  The pixel's own byte
//                              for the write rule comes from LDS too; only a pixel that fires under a paint source loads
//                   every output byte is written once; no atomics, no workgroup waits for another, all loops bounded by r and
//                   the tile
//  segk_byte_lut    dst[i] = lut[src[i]]
//  segk_fill_holes  a pixel of a reported component whose box stays off the image border and whose area is small enough takes
//                   `value`; the filled components are counted at their first pixel, one atomic per workgroup
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int TH = SEGK_MORPH_TILE_H, TW = SEGK_MORPH_TILE_W, RMAX = SEGK_MORPH_MAX_RADIUS;
constexpr unsigned WILD = SEGK_MORPH_WILD;
static_assert(TW == 128 && TH == 64, "the row pass splits a pixel index by a shift of 7");
static_assert(SEGK_MORPH_LDS_BYTES(RMAX) + 1024 <= 80 * 1024, "two workgroups of the largest radius fit a CU's 160 KiB of LDS");

template <int METRIC>
__device__ __forceinline__ int metric_of(int adx, int v) {
  if (METRIC == SEGK_MORPH_SQUARE) return adx > v ? adx : v;
  if (METRIC == SEGK_MORPH_DIAMOND) return adx + v;
  return adx * adx + v * v;
}

template <int METRIC>
__global__ __launch_bounds__(256) void morph_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ paint, uint8_t* __restrict__ out,
                                                    uint16_t* __restrict__ dist, const uint16_t* __restrict__ key,
                                                    const uint8_t* __restrict__ fire, int value, int r, int H, int W, int tiles_x) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ uint16_t s_tab[256];
  __shared__ uint8_t s_fire[256];
  const int SW = TW + 2 * r, SH = TH + 2 * r;              // staged columns and rows: cell (ly, lx) of the tile at [ly + r][lx + r]
  uint16_t* s_key = (uint16_t*)smem;
  uint8_t* s_g = smem + (size_t)SH * SW * 2;               // [TH][SW]: the tile's rows, every staged column
  uint8_t* s_val = s_g + TH * SW;                          // [TH][TW]: the tile's own bytes, for the write rule
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;

  s_tab[tid] = key[tid];
  s_fire[tid] = fire[tid];
  __syncthreads();
  // stage: a wave takes every fourth staged row, its lanes consecutive columns; twelve loads in flight per thread
  for (int s0 = wv; s0 < SH; s0 += 16) {
    unsigned v[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int s = s0 + 4 * a, gy = ty0 + s - r;
      const bool row_in = s < SH && gy >= 0 && gy < H;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int c = lane + 64 * b, gx = tx0 + c - r;
        v[a][b] = (row_in && c < SW && gx >= 0 && gx < W) ? (unsigned)mask[(size_t)gy * W + gx] : 256u;
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int s = s0 + 4 * a;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int c = lane + 64 * b;
        if (s < SH && c < SW) {
          s_key[s * SW + c] = (uint16_t)(v[a][b] < 256u ? (unsigned)s_tab[v[a][b]] : WILD);
          if (s >= r && s < TH + r && c >= r && c < TW + r) s_val[(s - r) * TW + c - r] = (uint8_t)v[a][b];
        }
      }
    }
  }
  __syncthreads();
  // columns: a = the last live key met, da the distance to it, db the distance to the nearest live key before it that is not a;
  // eight cells are read before they are walked, so the reads do not wait for the stores between them
  if (tid < SW) {
    const int sat = r + 1;
    unsigned a = WILD;
    int da = sat, db = sat;
    auto walk = [&](unsigned k) {                          // -> the distance from this cell; then one step on
      int d = da;
      if (k != WILD) {
        if (a != k) { db = da; a = k; } else d = db;
        da = 0;
      }
      da = da < sat ? da + 1 : sat;
      db = db < sat ? db + 1 : sat;
      return d;
    };
    for (int s0 = 0; s0 < TH + r; s0 += 8) {               // down: the rows below TH + r serve no row of the tile from above
      unsigned k[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) k[u] = s0 + u < TH + r ? (unsigned)s_key[(s0 + u) * SW + tid] : WILD;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int s = s0 + u, up = walk(k[u]);
        if (s >= r && s < TH + r) s_g[(s - r) * SW + tid] = (uint8_t)up;
      }
    }
    a = WILD; da = sat; db = sat;
    for (int s0 = SH - 1; s0 >= r; s0 -= 8) {              // up
      unsigned k[8], g[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int s = s0 - u;
        k[u] = s >= r ? (unsigned)s_key[s * SW + tid] : WILD;
        g[u] = (s >= r && s < TH + r) ? (unsigned)s_g[(s - r) * SW + tid] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int s = s0 - u, dn = walk(k[u]);
        if (s >= r && s < TH + r && (unsigned)dn < g[u]) s_g[(s - r) * SW + tid] = (uint8_t)dn;
      }
    }
  }
  __syncthreads();
  // rows: a wave takes 64 consecutive pixels of one row.  A cell is flagged when its g is in range or its key is not its left
  // neighbour's; a pixel with no flagged cell in its window has nothing that differs within the radius, and a wave of such
  // pixels (the inside of an object) does not walk at all.  Others walk from one left of their first flagged cell to the last.
  const int cap = METRIC == SEGK_MORPH_DISK ? r * r : r;
  for (int i = tid; i < TH * TW; i += 256) {
    const int ly = i >> 7, lx = i & (TW - 1);
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gy >= H || tx0 + lx - lane >= W) continue;         // wave-uniform: the row, or all 64 pixels, outside the image
    const uint16_t* krow = s_key + (ly + r) * SW + lx;     // cell (ly, lx + dx) at krow[dx + r]
    const uint8_t* grow = s_g + ly * SW + lx;
    u64 flags[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                          // cell c of the wave's window: krow[c - lane], c in [0, 64 + 2r)
      const int c = lane + 64 * h;
      bool f = false;
      if (c <= 63 + 2 * r) f = grow[c - lane] <= r || (c > 0 && krow[c - lane] != krow[c - lane - 1]);
      flags[h] = __ballot(f);
    }
    // the window of this lane: cells lane .. lane + 2r, bit j = cell lane + j (bit 64, r = 32 only, apart)
    const u64 w = ((flags[0] >> lane) | (lane ? flags[1] << (64 - lane) : 0ull)) & (2 * r + 1 >= 64 ? ~0ull : (1ull << (2 * r + 1)) - 1ull);
    const bool last = 2 * r == 64 && ((flags[1] >> lane) & 1ull);
    const unsigned kp = krow[r];
    int best = 0xFFFF;
    if (kp != WILD && gx < W && (w || last)) {
      const int first = w ? __ffsll((long long)w) - 1 : 64;
      const int j0 = first > 0 ? first - 1 : 0, j1 = last ? 64 : 63 - __clzll((long long)w);
      for (int j = j0; j <= j1; ++j) {
        const unsigned kq = krow[j];
        int v = grow[j];
        if (kq == WILD) {                                  // g: the nearest live key of the column, whatever it is
          const uint16_t* col = krow + j;
          int dy = v;
          for (; dy <= r; ++dy) {
            const unsigned u = col[-dy * SW], d = col[dy * SW];
            if ((u != WILD && u != kp) || (d != WILD && d != kp)) break;
          }
          v = dy;
        } else if (kq != kp) {
          v = 0;
        }
        const int dx = j - r;
        const int m = metric_of<METRIC>(dx < 0 ? -dx : dx, v);
        best = m < best ? m : best;
      }
    }
    if (gx >= W) continue;
    const bool fires = best <= cap;
    const size_t p = (size_t)gy * W + gx;
    if (out) {
      const unsigned m = s_val[i];
      unsigned o = m;
      if (fires && s_fire[m]) {
        if (paint) {
          const unsigned pv = paint[p];
          if (s_tab[pv] != kp) o = pv;
        } else {
          o = (unsigned)value;
        }
      }
      out[p] = (uint8_t)o;
    }
    if (dist) dist[p] = (uint16_t)(fires ? best : 0xFFFF);
  }
}

// ------------------------------------------------------------------------------------------------ byte table
__global__ __launch_bounds__(256) void byte_lut_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ lut,
                                                       long n, int words) {
  __shared__ uint8_t s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  if (words) {                                             // both pointers 4-byte aligned: four bytes per thread and trip
    const long n4 = n >> 2;
    for (long i = thread_of(); i < n4; i += stride_of()) {
      const unsigned v = ((const unsigned*)src)[i];
      ((unsigned*)dst)[i] = (unsigned)s_lut[v & 255u] | ((unsigned)s_lut[(v >> 8) & 255u] << 8) | ((unsigned)s_lut[(v >> 16) & 255u] << 16) |
                            ((unsigned)s_lut[v >> 24] << 24);
    }
    for (long i = (n4 << 2) + thread_of(); i < n; i += stride_of()) dst[i] = s_lut[src[i]];
  } else {
    for (long i = thread_of(); i < n; i += stride_of()) dst[i] = s_lut[src[i]];
  }
}

// ------------------------------------------------------------------------------------------------ hole fill
__global__ __launch_bounds__(256) void fill_holes_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ num, const int32_t* __restrict__ area,
                                                         const int32_t* __restrict__ box, const int32_t* __restrict__ first,
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ filled, int value, int max_area, int H,
                                                         int W, int cap) {
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int K = *num, rows = K < cap ? K : cap;
  const long total = (long)H * W;
  int mine = 0;
  for (long p = thread_of(); p < total; p += stride_of()) {
    const int id = labels[p];
    unsigned o = mask[p];
    if (id >= 1 && id <= rows) {
      const int4 b = *(const int4*)(box + 4 * (size_t)(id - 1));
      if (b.x > 0 && b.y > 0 && b.z < H && b.w < W && area[id - 1] <= max_area) {
        o = (unsigned)value;
        mine += first[id - 1] == (int)p;
      }
    }
    out[p] = (uint8_t)o;
  }
  const u64 any = __ballot(mine != 0);
  if (any) {                                               // wave-uniform
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_n, mine);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(filled, s_n);
}

int flat_grid(long items) {
  long g = (items + 255) / 256;
  const long cap = 8L * segk_num_cus();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

extern "C" int segk_morph(const uint8_t* mask, const uint8_t* paint, uint8_t* out, uint16_t* dist, const uint16_t* key,
                          const uint8_t* fire, int value, int metric, int radius, int H, int W, segk_stream_t s) {
  SEGK_REQUIRE(mask && key && fire, "morph: NULL pointer");
  SEGK_REQUIRE(out || dist, "morph: at least one of out and dist");
  SEGK_REQUIRE(metric == SEGK_MORPH_SQUARE || metric == SEGK_MORPH_DIAMOND || metric == SEGK_MORPH_DISK, "morph: metric %d (0 square, 1 diamond, 2 disk)",
               metric);
  SEGK_REQUIRE(radius >= 1 && radius <= SEGK_MORPH_MAX_RADIUS, "morph: radius %d (1..%d)", radius, SEGK_MORPH_MAX_RADIUS);
  SEGK_REQUIRE(H >= 1 && W >= 1, "morph: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "morph: %d x %d pixels, at most 2^28", H, W);
  SEGK_REQUIRE(value >= 0 && value <= 255, "morph: value %d (0..255)", value);
  SEGK_REQUIRE(((uintptr_t)key & 1) == 0 && ((uintptr_t)dist & 1) == 0, "morph: key and dist must be 2-byte aligned");
  SEGK_REQUIRE(!out || (out != mask && out != paint), "morph: the mask and paint are read while the output is written: not in place");
  SEGK_REQUIRE((const void*)dist != (const void*)mask, "morph: the mask is read while dist is written: not in place");
  SEGK_REQUIRE(!paint || out, "morph: paint without out");
  hipStream_t st = (hipStream_t)s;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;          // at most 2^28 / 64 tiles
  const dim3 grid((unsigned)((long)tiles_x * tiles_y));
  const size_t lds = (size_t)SEGK_MORPH_LDS_BYTES(radius);
  const int limit = SEGK_MORPH_LDS_BYTES(SEGK_MORPH_MAX_RADIUS);   // above the default 64 KiB from radius 30 on
  if (metric == SEGK_MORPH_SQUARE)
    return segk_launch_lds<morph_kernel<SEGK_MORPH_SQUARE>>("morph", limit, grid, dim3(256), lds, st, mask, paint, out, dist, key, fire, value,
                                                            radius, H, W, tiles_x);
  if (metric == SEGK_MORPH_DIAMOND)
    return segk_launch_lds<morph_kernel<SEGK_MORPH_DIAMOND>>("morph", limit, grid, dim3(256), lds, st, mask, paint, out, dist, key, fire, value,
                                                             radius, H, W, tiles_x);
  return segk_launch_lds<morph_kernel<SEGK_MORPH_DISK>>("morph", limit, grid, dim3(256), lds, st, mask, paint, out, dist, key, fire, value, radius,
                                                        H, W, tiles_x);
}

extern "C" int segk_byte_lut(const uint8_t* src, uint8_t* dst, const uint8_t* lut, long n, segk_stream_t s) {
  SEGK_REQUIRE(src && dst && lut, "byte_lut: NULL pointer");
  SEGK_REQUIRE(n >= 1 && n <= SEGK_CC_MAX_PIXELS, "byte_lut: %ld bytes (1..2^28)", n);
  SEGK_REQUIRE(src != dst, "byte_lut: not in place");
  const int words = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
  hipLaunchKernelGGL(byte_lut_kernel, dim3(flat_grid(words ? (n + 3) / 4 : n)), dim3(256), 0, (hipStream_t)s, src, dst, lut, n, words);
  SEGK_CHECK_LAUNCH("byte_lut");
  return 0;
}

extern "C" int segk_fill_holes(const uint8_t* mask, const int32_t* labels, const int32_t* num, const int32_t* area, const int32_t* box,
                               const int32_t* first, uint8_t* out, int32_t* filled, int value, int max_area, int H, int W,
                               int max_components, segk_stream_t s) {
  SEGK_REQUIRE(mask && labels && num && area && box && first && out && filled, "fill_holes: NULL pointer");
  SEGK_REQUIRE(H >= 1 && W >= 1, "fill_holes: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "fill_holes: %d x %d pixels, at most 2^28", H, W);
  SEGK_REQUIRE(max_components >= 1 && max_components <= (1 << 24), "fill_holes: max_components=%d (1..2^24)", max_components);
  SEGK_REQUIRE(value >= 0 && value <= 255, "fill_holes: value %d (0..255)", value);
  SEGK_REQUIRE(max_area >= 0, "fill_holes: max_area %d is negative", max_area);
  SEGK_REQUIRE(((uintptr_t)box & 15) == 0, "fill_holes: box must be 16-byte aligned");
  SEGK_REQUIRE(out != mask, "fill_holes: the mask is read while the output is written: not in place");
  hipLaunchKernelGGL(fill_holes_kernel, dim3(flat_grid((long)H * W)), dim3(256), 0, (hipStream_t)s, mask, labels, num, area, box, first, out,
                     filled, value, max_area, H, W, max_components);
  SEGK_CHECK_LAUNCH("fill_holes");
  return 0;
}
