// Boundary quality on the device: the band counts of Boundary IoU / trimap IoU and the histogram of
// contour-to-contour distances for one predicted and one label map, on the primitive of section 3.21 (the capped distance to
// the nearest non-void pixel of another class) and nothing wider.  The reference holds no code for this; every quantity is an
// integer count, so the device equals the restatement of tests/boundary_reference.py bit for bit.
//
//  segk_boundary_stats   boundary_kernel: one workgroup per tile of 64 rows x 128 columns
//                          stage     both byte maps of the tile and a halo of max(width, max_distance) + 1 cells become BIT PLANES
//                                    in LDS: per map and class one 64-bit word per 64 staged columns (a wave's ballot of
//                                    "class == c"), and the plane of non-void pixels.  Cells outside the image are in no plane.
//                          band      a wave takes 64 pixels of a row (one word) and each class present in it: its lanes fetch
//                                    the 2 width + 1 rows of "non-void and not c" once and flag the rows that hold a bit inside
//                                    the wave's box -- none: the wave leaves at once; else the flagged rows are walked, the
//                                    window of half-width hw(dy) (a small table: the metric) tested per lane by shifts
//                          counts    the band planes AND-ed with the class planes, popcounts, an LDS table
//                          contours  per class that occurs: K = the class plane AND the shifted "other" planes, both maps; a lane
//                                    that is a contour pixel walks the rows of the other map's K by increasing |dy|, takes the
//                                    nearest set bit of the row's window with clz / ffs and stops when dy^2 >= best
//                          flush     the non-zero entries of the LDS tables are added with 64-bit integer atomics
//  segk_boundary_finish  one workgroup: the per-image HD95 of every class from the image's histogram, which is then added to
//                        the running one and cleared -- so an update needs no synchronisation with the host
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int TH = SEGK_BOUNDARY_TILE_H, TW = SEGK_BOUNDARY_TILE_W, RMAX = SEGK_BOUNDARY_MAX_WIDTH, BINS = SEGK_BOUNDARY_BINS;
constexpr int MAXC = SEGK_MAX_CLASSES, HIST = SEGK_BOUNDARY_HIST_WORDS, CNT = SEGK_BOUNDARY_HD_SUM;
constexpr int PW = 4;                                      // words per staged row: columns tx0 - 64 .. tx0 + 191
constexpr unsigned VOID = 0xFFu;
static_assert(TW == 128 && TH == 64 && RMAX == 32, "a wave is one word of a tile row; windows are 65 bits at most");
static_assert(RMAX + 1 <= 64, "the halo lies inside the words beside the tile");
static_assert(SEGK_BOUNDARY_LDS_BYTES(MAXC, RMAX + 1) + 8192 <= 160 * 1024, "the largest launch fits a CU's LDS");
static_assert(SEGK_BOUNDARY_LDS_BYTES(MAXC - 2, RMAX + 1) + 8192 <= 80 * 1024, "two workgroups of up to six classes fit a CU");

__device__ __forceinline__ u64 uniform64(u64 v) {          // a value every lane of the wave holds -> scalar registers
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// bits sc - 32 .. sc + 31 of the row whose words wj - 1, wj, wj + 1 are o0, o1, o2 (sc = 64 wj + lane): bit 32 is the pixel
__device__ __forceinline__ u64 window_of(u64 o0, u64 o1, u64 o2, int lane) {
  const int start = lane + 32;                             // in the 192 bits o0 : o1 : o2
  if (start < 64) return (o0 >> start) | (o1 << (64 - start));
  const int s2 = start - 64;
  return s2 ? (o1 >> s2) | (o2 << (64 - s2)) : o1;
}
// ... and bit sc + 32
__device__ __forceinline__ bool far_bit(u64 o1, u64 o2, int lane) { return ((lane < 32 ? o1 >> (lane + 32) : o2 >> (lane - 32)) & 1ull) != 0; }

__global__ __launch_bounds__(256) void boundary_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ label,
                                                       u64* __restrict__ stats, u64* __restrict__ image_hist, int C, int ign, int metric,
                                                       int width, int maxd, int border, int H, int W, int tiles_x) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ u64 s_band[2][TH][2];                         // per map: the tile's pixels with D <= width
  __shared__ int s_cnt[CNT];                               // band_g, band_p, band_i, conf
  __shared__ int s_hist[HIST];
  __shared__ int s_hw[2 * RMAX + 1];                       // half-width of the element's row dy at [dy + width]
  __shared__ int s_present, s_kflag[MAXC];
  const int h = SEGK_BOUNDARY_HALO(width, maxd), SH = TH + 2 * h;
  u64* planes = (u64*)smem;                                // plane k, staged row s, word j at planes[(k * SH + s) * PW + j]
  auto plane = [&](int k) { return planes + (size_t)k * SH * PW; };
  // planes: class c of the label at c, of the prediction at C + c, non-void at 2C (label) and 2C + 1, contours at 2C + 2, 2C + 3
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;

  for (int i = tid; i < CNT; i += 256) s_cnt[i] = 0;
  for (int i = tid; i < HIST; i += 256) s_hist[i] = 0;
  for (int i = tid; i < 2 * TH * 2; i += 256) (&s_band[0][0][0])[i] = 0ull;
  if (tid < MAXC) s_kflag[tid] = 0;
  if (tid == 0) s_present = 0;
  if (tid <= 2 * width) {
    const int dy = tid - width, ady = dy < 0 ? -dy : dy;
    int hw = width;
    if (metric == SEGK_MORPH_DIAMOND) hw = width - ady;
    if (metric == SEGK_MORPH_DISK) {
      hw = 0;
      for (int k = 1; k <= width; ++k) hw = (k * k + ady * ady <= width * width) ? k : hw;
    }
    s_hw[tid] = hw;
  }
  __syncthreads();

  // stage: a wave takes every fourth staged row and its four words; sixteen loads in flight per thread (two rows at a time)
  int seen = 0;
  for (int s0 = wv; s0 < SH; s0 += 8) {
    unsigned g[2][PW], p[2][PW];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int s = s0 + 4 * a, gy = ty0 + s - h;
      const bool row_in = s < SH && gy >= 0 && gy < H;
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        const int off = 64 * j + lane - 64, gx = tx0 + off;        // off: the column relative to the tile
        const bool in = row_in && off >= -h && off < TW + h && gx >= 0 && gx < W;
        g[a][j] = in ? (unsigned)label[(size_t)gy * W + gx] : VOID;
        p[a][j] = in ? (unsigned)pred[(size_t)gy * W + gx] : VOID;
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int s = s0 + 4 * a;
      if (s >= SH) continue;                                        // wave-uniform
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        const unsigned gb = g[a][j], pb = p[a][j];
        const unsigned cg = (gb < (unsigned)C && !((ign >> gb) & 1)) ? gb : VOID;
        const unsigned cp = (cg != VOID && pb < (unsigned)C) ? pb : VOID;
        const size_t at = (size_t)s * PW + j;
        for (int c = 0; c < C; ++c) {
          const u64 bg = __ballot(cg == (unsigned)c), bp = __ballot(cp == (unsigned)c);
          if (lane == 0) {
            plane(c)[at] = bg;
            plane(C + c)[at] = bp;
          }
          seen |= (bg | bp) ? 1 << c : 0;
        }
        const u64 ng = __ballot(cg != VOID), np = __ballot(cp != VOID);
        if (lane == 0) {
          plane(2 * C)[at] = ng;
          plane(2 * C + 1)[at] = np;
        }
      }
    }
  }
  if (lane == 0 && seen) atomicOr(&s_present, seen);
  __syncthreads();

  // band: a wave per (row, word) of the tile
  for (int step = wv; step < TH * 2; step += 4) {
    const int ly = step >> 1, wj = 1 + (step & 1), row = ly + h;
    const int gy = ty0 + ly, gx = tx0 + 64 * (wj - 1) + lane;
    if (gy >= H || gx - lane >= W) continue;                        // wave-uniform: the row, or all 64 pixels, outside the image
    bool edge = false;
    if (border && gx < W) {
      int b = gy + 1 < gx + 1 ? gy + 1 : gx + 1;
      b = H - gy < b ? H - gy : b;
      b = W - gx < b ? W - gx : b;
      edge = b <= width;
    }
#pragma unroll 1
    for (int m = 0; m < 2; ++m) {
      const u64* nv = plane(2 * C + m);
      u64 todo = uniform64(nv[row * PW + wj]);                      // the non-void pixels of this word
      u64 band = 0ull;
#pragma unroll 1
      for (int c = 0; c < C && todo; ++c) {
        const u64* cls = plane(m * C + c);
        const u64 cw = uniform64(cls[row * PW + wj]);
        if (!cw) continue;
        todo &= ~cw;
        // lane l fetches row dy = l - width; the wave's box is the columns 64 wj - width .. 64 wj + 63 + width
        bool f = false;
        if (lane <= 2 * width) {
          const int at = (row - width + lane) * PW + wj;
          const u64 o0 = (nv[at - 1] & ~cls[at - 1]) & (~0ull << (64 - width));
          const u64 o1 = nv[at] & ~cls[at];
          const u64 o2 = (nv[at + 1] & ~cls[at + 1]) & ((1ull << width) - 1ull);
          f = (o0 | o1 | o2) != 0ull;
        }
        u64 rows = __ballot(f);
        bool last = false;                                          // the 65th row of width 32, which has no lane
        if (2 * width == 64) {
          const int at = (row + width) * PW + wj;
          last = uniform64(((nv[at - 1] & ~cls[at - 1]) >> 32) | (nv[at] & ~cls[at]) | ((nv[at + 1] & ~cls[at + 1]) << 32)) != 0ull;
        }
        bool in = edge;
        const int n_rows = __popcll(rows) + (last ? 1 : 0);
        for (int k = 0; k < n_rows; ++k) {                          // wave-uniform trip count, at most 2 width + 1
          int l = 64;
          if (rows) {
            l = __ffsll((long long)rows) - 1;
            rows &= rows - 1ull;
          }
          const int at = (row - width + l) * PW + wj, hw = s_hw[l];
          const u64 o0 = nv[at - 1] & ~cls[at - 1], o1 = nv[at] & ~cls[at], o2 = nv[at + 1] & ~cls[at + 1];
          const u64 v = window_of(o0, o1, o2, lane);
          if (hw >= 32) in = in || v != 0ull || far_bit(o1, o2, lane);
          else if (hw >= 0) in = in || (v & (((1ull << (2 * hw + 1)) - 1ull) << (32 - hw))) != 0ull;
          if (!(cw & ~__ballot(in))) break;                         // every pixel of the class is in the band already
        }
        band |= __ballot(in) & cw;
      }
      if (lane == 0) s_band[m][ly][wj - 1] = band;
    }
  }
  __syncthreads();

  // counts: one thread per word of the tile
  if (tid < TH * 2) {
    const int ly = tid >> 1, j = tid & 1, at = (ly + h) * PW + 1 + j;
    const u64 bg = s_band[0][ly][j], bp = s_band[1][ly][j];
    if (bg | bp) {
      for (int c = 0; c < C; ++c) {
        const u64 gc = plane(c)[at] & bg, pc = plane(C + c)[at] & bp;
        if (gc) atomicAdd(&s_cnt[SEGK_BOUNDARY_BAND_G + c], __popcll(gc));
        if (pc) atomicAdd(&s_cnt[SEGK_BOUNDARY_BAND_P + c], __popcll(pc));
        if (gc & pc) atomicAdd(&s_cnt[SEGK_BOUNDARY_BAND_I + c], __popcll(gc & pc));
        if (gc) {
          for (int q = 0; q < C; ++q) {
            const u64 both = gc & plane(C + q)[at];
            if (both) atomicAdd(&s_cnt[SEGK_BOUNDARY_CONF + MAXC * c + q], __popcll(both));
          }
        }
      }
    }
  }

  // contours, class by class
  const int present = __builtin_amdgcn_readfirstlane(s_present);
  u64* kpl = plane(2 * C + 2);                                      // K of the label, then K of the prediction
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    if (!((present >> c) & 1)) continue;                            // uniform over the workgroup
    __syncthreads();                                                // the last class's searches are over
    for (int i = tid; i < SH * PW * 2; i += 256) {
      const int m = i >= SH * PW, at = i - m * SH * PW, s = at >> 2, j = at & 3;
      const u64 *nv = plane(2 * C + m), *cls = plane(m * C + c);
      const u64 cw = cls[at];
      u64 k = 0ull;
      if (cw) {
        const u64 o = nv[at] & ~cls[at];
        u64 near = (o << 1) | (o >> 1);
        if (j > 0) near |= (nv[at - 1] & ~cls[at - 1]) >> 63;
        if (j < PW - 1) near |= (nv[at + 1] & ~cls[at + 1]) << 63;
        if (s > 0) near |= nv[at - PW] & ~cls[at - PW];
        if (s < SH - 1) near |= nv[at + PW] & ~cls[at + PW];
        k = cw & near;
      }
      kpl[i] = k;
      if (k && s >= h && s < h + TH && (j == 1 || j == 2)) atomicOr(&s_kflag[c], 1 << m);
    }
    __syncthreads();
    const int kf = __builtin_amdgcn_readfirstlane(s_kflag[c]);
    if (!kf) continue;
    for (int step = wv; step < TH * 2; step += 4) {
      const int ly = step >> 1, wj = 1 + (step & 1), row = ly + h;
#pragma unroll 1
      for (int m = 0; m < 2; ++m) {                                 // m: the map whose contour pixels look for the other's
        if (!((kf >> m) & 1)) continue;
        const u64 mine = uniform64(kpl[(m * SH + row) * PW + wj]);
        if (!((mine >> lane) & 1ull)) continue;
        const u64* other = kpl + (size_t)(1 - m) * SH * PW;
        int best = 1 << 20;
        for (int ady = 0; ady <= maxd && ady * ady < best; ++ady) {
          for (int sg = 0; sg < (ady ? 2 : 1); ++sg) {
            const int at = (row + (sg ? ady : -ady)) * PW + wj;
            const u64 o0 = other[at - 1], o1 = other[at], o2 = other[at + 1];
            const u64 v = window_of(o0, o1, o2, lane);
            const u64 left = v & ((1ull << 33) - 1ull), right = v >> 33;      // offsets -32..0 and 1..31
            int adx = 64;
            if (left) adx = __clzll((long long)left) - 31;
            if (right) {
              const int r = __ffsll((long long)right);
              adx = r < adx ? r : adx;
            } else if (adx > 32 && far_bit(o1, o2, lane)) {
              adx = 32;
            }
            if (adx <= 32) {
              const int d2 = adx * adx + ady * ady;
              best = d2 < best ? d2 : best;
            }
          }
        }
        int bin = maxd + 1;
        if (best <= maxd * maxd) {
          bin = 0;
          for (int t = 0; t < maxd; ++t) bin += t * t < best ? 1 : 0;         // the smallest t with t^2 >= best
        }
        atomicAdd(&s_hist[((1 - m) * MAXC + c) * BINS + bin], 1);   // hist[0]: pred -> label (m == 1), hist[1]: label -> pred
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < CNT; i += 256)
    if (s_cnt[i]) atomicAdd(stats + i, (u64)s_cnt[i]);
  for (int i = tid; i < HIST; i += 256)
    if (s_hist[i]) atomicAdd(image_hist + i, (u64)s_hist[i]);
}

__global__ __launch_bounds__(64) void boundary_finish_kernel(u64* __restrict__ stats, u64* __restrict__ image_hist, int C, int maxd) {
  const int tid = threadIdx.x;
  if (tid < C) {
    const u64 *a = image_hist + (size_t)tid * BINS, *b = image_hist + (size_t)(MAXC + tid) * BINS;
    u64 n = 0ull;
    for (int t = 0; t <= maxd + 1; ++t) n += a[t] + b[t];
    if (n) {
      u64 cum = 0ull;
      int hd = maxd + 1;
      for (int t = 0; t <= maxd + 1; ++t) {
        cum += a[t] + b[t];
        if (20ull * cum >= 19ull * n) {
          hd = t;
          break;
        }
      }
      if (hd == maxd + 1) {
        stats[SEGK_BOUNDARY_HD_CAPPED + tid] += 1ull;
      } else {
        stats[SEGK_BOUNDARY_HD_SUM + tid] += (u64)hd;
        stats[SEGK_BOUNDARY_HD_IMAGES + tid] += 1ull;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < HIST; i += 64) {
    const u64 v = image_hist[i];
    if (v) {
      stats[SEGK_BOUNDARY_HIST + i] += v;
      image_hist[i] = 0ull;
    }
  }
}

}  // namespace

extern "C" int segk_boundary_stats(const uint8_t* pred, const uint8_t* label, int64_t* stats, int64_t* image_hist, int num_classes,
                                   int ignore_mask, int metric, int width, int max_distance, int image_border, int H, int W,
                                   segk_stream_t s) {
  SEGK_REQUIRE(pred && label && stats && image_hist, "boundary_stats: NULL pointer");
  SEGK_REQUIRE(num_classes >= 1 && num_classes <= SEGK_MAX_CLASSES, "boundary_stats: num_classes %d (1..%d)", num_classes, SEGK_MAX_CLASSES);
  SEGK_REQUIRE(ignore_mask >= 0 && ignore_mask <= 255, "boundary_stats: ignore_mask %d (bits 0..7)", ignore_mask);
  SEGK_REQUIRE(metric == SEGK_MORPH_SQUARE || metric == SEGK_MORPH_DIAMOND || metric == SEGK_MORPH_DISK,
               "boundary_stats: metric %d (0 square, 1 diamond, 2 disk)", metric);
  SEGK_REQUIRE(width >= 1 && width <= SEGK_BOUNDARY_MAX_WIDTH, "boundary_stats: width %d (1..%d)", width, SEGK_BOUNDARY_MAX_WIDTH);
  SEGK_REQUIRE(max_distance >= 1 && max_distance <= SEGK_BOUNDARY_MAX_WIDTH, "boundary_stats: max_distance %d (1..%d)", max_distance,
               SEGK_BOUNDARY_MAX_WIDTH);
  SEGK_REQUIRE(image_border == 0 || image_border == 1, "boundary_stats: image_border %d (0 | 1)", image_border);
  SEGK_REQUIRE(H >= 1 && W >= 1, "boundary_stats: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "boundary_stats: %d x %d pixels, at most 2^28", H, W);
  SEGK_REQUIRE((((uintptr_t)stats | (uintptr_t)image_hist) & 7) == 0, "boundary_stats: stats and image_hist must be 8-byte aligned");
  SEGK_REQUIRE(stats != image_hist, "boundary_stats: stats and image_hist are distinct buffers");
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int halo = SEGK_BOUNDARY_HALO(width, max_distance);
  const size_t lds = (size_t)SEGK_BOUNDARY_LDS_BYTES(num_classes, halo);
  return segk_launch_lds<boundary_kernel>("boundary_stats", SEGK_BOUNDARY_LDS_BYTES(SEGK_MAX_CLASSES, SEGK_BOUNDARY_MAX_WIDTH + 1),
                                          dim3((unsigned)((long)tiles_x * tiles_y)), dim3(256), lds, (hipStream_t)s, pred, label, (u64*)stats,
                                          (u64*)image_hist, num_classes, ignore_mask, metric, width, max_distance, image_border, H, W,
                                          tiles_x);
}

extern "C" int segk_boundary_finish(int64_t* stats, int64_t* image_hist, int num_classes, int max_distance, segk_stream_t s) {
  SEGK_REQUIRE(stats && image_hist, "boundary_finish: NULL pointer");
  SEGK_REQUIRE(num_classes >= 1 && num_classes <= SEGK_MAX_CLASSES, "boundary_finish: num_classes %d (1..%d)", num_classes, SEGK_MAX_CLASSES);
  SEGK_REQUIRE(max_distance >= 1 && max_distance <= SEGK_BOUNDARY_MAX_WIDTH, "boundary_finish: max_distance %d (1..%d)", max_distance,
               SEGK_BOUNDARY_MAX_WIDTH);
  SEGK_REQUIRE((((uintptr_t)stats | (uintptr_t)image_hist) & 7) == 0, "boundary_finish: stats and image_hist must be 8-byte aligned");
  SEGK_REQUIRE(stats != image_hist, "boundary_finish: stats and image_hist are distinct buffers");
  hipLaunchKernelGGL(boundary_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (u64*)stats, (u64*)image_hist, num_classes, max_distance);
  SEGK_CHECK_LAUNCH("boundary_finish");
  return 0;
}
