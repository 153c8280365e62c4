// Superpixels on the device: SLIC in the pixel-centric (gSLIC) formulation, and snapping a mask to a
// segmentation by a per-segment vote.  The reference holds no code for this; every quantity is an integer, ties go to the
// lowest index and the sums are order-free, so the device equals the restatement of tests/slic_reference.py bit for bit.
//
//  segk_slic_start   slic_start_kernel: K threads set the start centres and zero the sums
//  segk_slic_assign  slic_assign_kernel: one workgroup of 256 per tile of tile_rows (4, 16 or 64) x 64 pixels
//                      stage    the centres of the cells the tile and its one-cell ring touch (at most 18 x 18) go to LDS, eight
//                               words per cell; the tile's table of sums is cleared
//                      rows     a wave takes every fourth row of the tile, 64 pixels: the row's bytes are read as dwords where the row address is
//                               4-byte aligned (byte by byte where not, and for a ragged last dword), a pixel's bytes come from
//                               two lanes' dwords; nine distances (two 64-bit multiply-adds each), strict < in index order
//                      sums     adjacent lanes with one label are a run (run_length, scan.hpp): the head lane adds the run's
//                               count, its position sums in closed form and its colour sums from a wave prefix to the LDS table
//                      flush    the non-zero words of the table are added with 32-bit integer atomics
//  segk_slic_update  slic_update_kernel: K threads: the division, the keep-on-empty rule, the counts, the re-zeroing
//  segk_snap_vote    snap_vote_kernel: the same tile and run rule; (label, class) -> weight in an open LDS table (tab_slot,
//                    scan.hpp), flushed with 64-bit integer atomics
//  segk_snap_paint   snap_winner_kernel (K threads: winner and the share test) and snap_paint_kernel (four pixels per thread)
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int TS = SEGK_SLIC_TILE, MAXC = SEGK_SLIC_MAX_CELLS, CENW = SEGK_SLIC_CENTRE_WORDS, SUMW = SEGK_SLIC_SUM_WORDS;
constexpr int LCW = 8;                                     // words per staged centre: Y X C0 C1 | C2 and three unused
constexpr int LSW = 6;                                     // words per cell of the tile's sums: n, y, x, c0, c1, c2
constexpr int VOTE_SLOTS = 2048;
static_assert(TS == 64, "a wave is one row of the tile");
static_assert((TS - 1) / SEGK_SLIC_MIN_STEP + 1 + 2 <= MAXC, "a tile's cells and their ring fit the staged table at step 4");
static_assert((TS - 1) / (SEGK_SLIC_MIN_STEP + 1) + 2 + 2 <= MAXC, "... and at every step that does not divide the tile");
// the sums fit 32 bits: a cluster owns at most 9 S^2 pixels, an offset is below 3 S, a colour below 256, and update forms 32 sum + n
static_assert(32L * 9 * SEGK_SLIC_MAX_STEP * SEGK_SLIC_MAX_STEP * (3 * SEGK_SLIC_MAX_STEP) + 9 * SEGK_SLIC_MAX_STEP * SEGK_SLIC_MAX_STEP < (1L << 31),
              "32 sum + n of a position fits an int");
static_assert(32L * 9 * SEGK_SLIC_MAX_STEP * SEGK_SLIC_MAX_STEP * 255 + 9 * SEGK_SLIC_MAX_STEP * SEGK_SLIC_MAX_STEP < (1L << 31), "... and of a colour");

__device__ __forceinline__ int clamp_byte(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the features of the pixel whose bytes are px = b0 | b1 << 8 | b2 << 16 (DESIGN.md 3.24 "features")
__device__ __forceinline__ void features_of(unsigned px, int C, int space, int& c0, int& c1, int& c2) {
  const int r = (int)(px & 255u), g = (int)((px >> 8) & 255u), b = (int)((px >> 16) & 255u);
  c0 = r;
  c1 = C == 1 ? 0 : g;
  c2 = C == 1 ? 0 : b;
  if (C != 1 && space == SEGK_SLIC_YCC) {
    c0 = clamp_byte((77 * r + 150 * g + 29 * b + 128) >> 8);
    c1 = clamp_byte(((-43 * r - 85 * g + 128 * b + 128) >> 8) + 128);
    c2 = clamp_byte(((128 * r - 107 * g - 21 * b + 128) >> 8) + 128);
  }
}

__global__ __launch_bounds__(256) void slic_start_kernel(const uint8_t* __restrict__ img, int* __restrict__ centres, int* __restrict__ sums,
                                                         int C, int space, int S, int H, int W, int nx, int K) {
  const long k = thread_of();
  if (k >= K) return;
  const int i = (int)(k / nx), j = (int)(k - (long)i * nx);
  const int y = i * S + S / 2 < H - 1 ? i * S + S / 2 : H - 1, x = j * S + S / 2 < W - 1 ? j * S + S / 2 : W - 1;
  const uint8_t* p = img + ((size_t)y * W + x) * C;
  unsigned px = p[0];
  if (C >= 3) px |= ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
  int c0, c1, c2;
  features_of(px, C, space, c0, c1, c2);
  int* c = centres + k * CENW;
  c[0] = 16 * y;
  c[1] = 16 * x;
  c[2] = 16 * c0;
  c[3] = 16 * c1;
  c[4] = 16 * c2;
  int4* z = (int4*)(sums + k * SUMW);
  z[0] = make_int4(0, 0, 0, 0);
  z[1] = make_int4(0, 0, 0, 0);
}

// dword d of the nb bytes at `row`: one load where the row is 4-byte aligned and the dword lies inside, else byte by byte
__device__ __forceinline__ unsigned row_dword(const uint8_t* __restrict__ row, int d, int nb, bool wide) {
  const int at = 4 * d;
  unsigned v = 0u;
  if (at < nb) {
    if (wide && at + 4 <= nb) {
      v = *(const unsigned*)(row + at);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (at + b < nb) v |= (unsigned)row[at + b] << (8 * b);
    }
  }
  return v;
}

// inclusive prefix over the wave
__device__ __forceinline__ unsigned wave_prefix(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}
// the sum over the run of `len` lanes that starts at this (head) lane, from the inclusive prefix `inc` of `own`; the halves of
// a packed word do not borrow: each half's prefix only grows
__device__ __forceinline__ unsigned run_sum(unsigned inc, unsigned own, int len, int lane) {
  return __shfl(inc, (lane + len - 1) & 63) - (inc - own);
}

__global__ __launch_bounds__(256) void slic_assign_kernel(const uint8_t* __restrict__ img, const int* __restrict__ centres,
                                                          int* __restrict__ sums, int* __restrict__ labels, int C, int space, int S,
                                                          int m2, int H, int W, int ny, int nx, int tiles_x, int rows, int write_labels) {
  __shared__ __align__(16) int s_cen[MAXC * MAXC * LCW];
  __shared__ int s_sum[MAXC * MAXC * LSW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty0 = (int)(blockIdx.x / tiles_x) * rows, tx0 = (int)(blockIdx.x % tiles_x) * TS;
  const int ty1 = (ty0 + rows < H ? ty0 + rows : H) - 1, tx1 = (tx0 + TS < W ? tx0 + TS : W) - 1;      // the tile's last row and column
  const int cy0 = ty0 / S - 1, cx0 = tx0 / S - 1;                                                  // first staged cell: the ring
  int ncy = ty1 / S + 1 - cy0 + 1, ncx = tx1 / S + 1 - cx0 + 1;
  ncy = ncy < MAXC ? ncy : MAXC;                           // never more (the static_asserts above): the tables are this large
  ncx = ncx < MAXC ? ncx : MAXC;
  const int cells = ncy * ncx;

  for (int i = tid; i < cells; i += 256) {
    const int ly = i / ncx, lx = i - ly * ncx, gy = cy0 + ly, gx = cx0 + lx;
    int4 a = make_int4(0, 0, 0, 0);
    int c2 = 0;
    if ((unsigned)gy < (unsigned)ny && (unsigned)gx < (unsigned)nx) {
      const int* c = centres + ((size_t)gy * nx + gx) * CENW;
      a = make_int4(c[0], c[1], c[2], c[3]);
      c2 = c[4];
    }
    *(int4*)(s_cen + i * LCW) = a;
    s_cen[i * LCW + 4] = c2;
  }
  for (int i = tid; i < cells * LSW; i += 256) s_sum[i] = 0;
  __syncthreads();

  const int x = tx0 + lane;
  const bool in_x = x <= tx1;
  const int xe = in_x ? x : tx1;                           // a lane past the image computes on the last column and adds nothing
  const int cxp = xe / S, lcx = cxp - cx0;                 // the pixel's own cell: lcx in 1 .. ncx - 2
  const int off = C * lane, src = off >> 2, sh = (off & 3) * 8;
  const int nb = (tx1 - tx0 + 1) * C;                      // bytes of a tile row, at most 256: a dword per lane
  const unsigned S2 = (unsigned)(S * S), M2 = (unsigned)m2;

  for (int r = wv; r < rows; r += 4) {
    const int y = ty0 + r;
    if (y > ty1) break;                                    // wave-uniform
    const uint8_t* row = img + ((size_t)y * W + tx0) * C;
    const unsigned dw = row_dword(row, lane, nb, (((uintptr_t)row) & 3) == 0);
    const unsigned lo = __shfl(dw, src), hi = __shfl(dw, (src + 1) & 63);
    const unsigned px = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    int c0, c1, c2;
    features_of(px, C, space, c0, c1, c2);
    const int cyp = y / S, lcy = cyp - cy0;

    u64 best = ~0ull;
    int bq = 4;                                            // the own cell is always a candidate
#pragma unroll
    for (int di = -1; di <= 1; ++di) {
      if ((unsigned)(cyp + di) >= (unsigned)ny) continue;  // wave-uniform
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const bool valid = (unsigned)(cxp + dj) < (unsigned)nx;
        const int* c = s_cen + ((lcy + di) * ncx + lcx + dj) * LCW;
        const int4 a = *(const int4*)c;
        const int a4 = c[4];
        const unsigned dy = (unsigned)(16 * y - a.x), dx = (unsigned)(16 * xe - a.y);
        const unsigned e0 = (unsigned)(16 * c0 - a.z), e1 = (unsigned)(16 * c1 - a.w), e2 = (unsigned)(16 * c2 - a4);
        const unsigned dp = dy * dy + dx * dx, dc = e0 * e0 + e1 * e1 + e2 * e2;
        const u64 D = (u64)dc * S2 + (u64)dp * M2;
        if (valid && D < best) {                           // index order and a strict <: the lowest k of a tie
          best = D;
          bq = (di + 1) * 3 + dj + 1;
        }
      }
    }
    const int bdi = (bq * 11) >> 5, bdj = bq - 3 * bdi;    // bq / 3 and bq % 3 for 0..8
    const int gy = cyp + bdi - 1, gx = cxp + bdj - 1;
    const int cell = (lcy + bdi - 1) * ncx + lcx + bdj - 1;
    if (write_labels && in_x) labels[(size_t)y * W + x] = gy * nx + gx;

    const int key = in_x ? cell : -1;
    const int len = run_length(key, lane);
    const unsigned own01 = in_x ? (unsigned)c0 | ((unsigned)c1 << 16) : 0u, own2 = in_x ? (unsigned)c2 : 0u;
    const unsigned inc01 = wave_prefix(own01, lane), inc2 = wave_prefix(own2, lane);
    const unsigned t01 = run_sum(inc01, own01, len, lane), t2 = run_sum(inc2, own2, len, lane);
    if (len && key >= 0) {
      int* t = s_sum + cell * LSW;
      atomicAdd(t + 0, len);
      atomicAdd(t + 1, len * (y - (gy - 1) * S));
      atomicAdd(t + 2, len * (x - (gx - 1) * S) + len * (len - 1) / 2);
      atomicAdd(t + 3, (int)(t01 & 0xFFFFu));
      if (C != 1) {
        atomicAdd(t + 4, (int)(t01 >> 16));
        atomicAdd(t + 5, (int)t2);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < cells * LSW; i += 256) {
    const int v = s_sum[i];
    if (!v) continue;
    const int cell = i / LSW, w = i - cell * LSW, ly = cell / ncx, lx = cell - ly * ncx, gy = cy0 + ly, gx = cx0 + lx;
    if ((unsigned)gy < (unsigned)ny && (unsigned)gx < (unsigned)nx) atomicAdd(sums + ((size_t)gy * nx + gx) * SUMW + w, v);
  }
}

__global__ __launch_bounds__(256) void slic_update_kernel(int* __restrict__ centres, int* __restrict__ sums, int* __restrict__ counts, int S,
                                                          int nx, int K) {
  const long k = thread_of();
  if (k >= K) return;
  int4* sp = (int4*)(sums + k * SUMW);
  const int4 a = sp[0], b = sp[1];
  const int n = a.x > 0 ? a.x : 0;
  counts[k] = n;
  if (n > 0) {
    const int i = (int)(k / nx), j = (int)(k - (long)i * nx);
    const unsigned un = (unsigned)n;
    auto mean16 = [&](int sum) { return (int)((32u * (unsigned)sum + un) / (2u * un)); };        // round(16 mean), half up
    int* c = centres + k * CENW;
    c[0] = 16 * (i - 1) * S + mean16(a.y);                 // the position sums are offsets from the cell before the home cell
    c[1] = 16 * (j - 1) * S + mean16(a.z);
    c[2] = mean16(a.w);
    c[3] = mean16(b.x);
    c[4] = mean16(b.y);
  }
  sp[0] = make_int4(0, 0, 0, 0);
  sp[1] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void snap_vote_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ mask,
                                                        const uint8_t* __restrict__ weights, u64* __restrict__ hist, int classes, int H,
                                                        int W, int K, int tiles_x, int rows) {
  __shared__ int s_key[VOTE_SLOTS], s_val[VOTE_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ty0 = (int)(blockIdx.x / tiles_x) * rows, x = (int)(blockIdx.x % tiles_x) * TS + lane;
  for (int i = tid; i < VOTE_SLOTS; i += 256) {
    s_key[i] = -1;
    s_val[i] = 0;
  }
  __syncthreads();
  for (int r = wv; r < rows; r += 4) {
    const int y = ty0 + r;
    if (y >= H) break;                                     // wave-uniform
    int key = -1;
    unsigned w = 0u;
    if (x < W) {
      const size_t p = (size_t)y * W + x;
      const int k = labels[p];
      const unsigned c = mask[p];
      if ((unsigned)k < (unsigned)K && c < 8u && ((classes >> c) & 1)) {
        key = k * 8 + (int)c;                              // K <= 2^28: fits
        w = weights ? (unsigned)weights[p] : 1u;
      }
    }
    const int len = run_length(key, lane);
    const unsigned tot = run_sum(wave_prefix(w, lane), w, len, lane);
    if (len && key >= 0 && tot) {
      const int h = tab_slot<VOTE_SLOTS>(s_key, key);
      if (h >= 0) atomicAdd(s_val + h, (int)tot);          // at most 255 * 4096 per tile
      else atomicAdd(hist + key, (u64)tot);
    }
  }
  __syncthreads();
  for (int i = tid; i < VOTE_SLOTS; i += 256)
    if (s_key[i] >= 0 && s_val[i]) atomicAdd(hist + s_key[i], (u64)(unsigned)s_val[i]);
}

__global__ __launch_bounds__(256) void snap_winner_kernel(const u64* __restrict__ hist, int* __restrict__ winner, uint8_t* __restrict__ paint,
                                                          int min_share, int K) {
  const long k = thread_of();
  if (k >= K) return;
  const u64* h = hist + k * 8;
  u64 best = 0ull, total = 0ull;
  int w = -1;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const u64 v = h[c];
    total += v;
    if (v > best) {                                        // strict: the lowest class of a tie; a row of zeros has no winner
      best = v;
      w = c;
    }
  }
  winner[k] = w;
  paint[k] = (uint8_t)((w >= 0 && 256ull * best >= (u64)min_share * total) ? w : SEGK_SNAP_NONE);
}

__device__ __forceinline__ unsigned snap_one(int k, unsigned m, const uint8_t* __restrict__ paint, u64 a0, u64 a1, u64 a2, u64 a3, int K) {
  if ((unsigned)k >= (unsigned)K) return m;
  const unsigned pv = paint[k];
  const u64 word = m < 128u ? (m < 64u ? a0 : a1) : (m < 192u ? a2 : a3);
  return (pv != (unsigned)SEGK_SNAP_NONE && ((word >> (m & 63u)) & 1ull)) ? pv : m;
}

__global__ __launch_bounds__(256) void snap_paint_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ mask,
                                                         const uint8_t* __restrict__ paint, uint8_t* __restrict__ out, u64 a0, u64 a1, u64 a2,
                                                         u64 a3, long n, int K, int wide) {
  for (long g = thread_of(); 4 * g < n; g += stride_of()) {
    const long p = 4 * g;
    if (wide && p + 4 <= n) {
      const int4 k4 = *(const int4*)(labels + p);
      const unsigned m4 = *(const unsigned*)(mask + p);
      const unsigned o = snap_one(k4.x, m4 & 255u, paint, a0, a1, a2, a3, K) | (snap_one(k4.y, (m4 >> 8) & 255u, paint, a0, a1, a2, a3, K) << 8) |
                         (snap_one(k4.z, (m4 >> 16) & 255u, paint, a0, a1, a2, a3, K) << 16) | (snap_one(k4.w, m4 >> 24, paint, a0, a1, a2, a3, K) << 24);
      *(unsigned*)(out + p) = o;
    } else {
      for (long q = p; q < p + 4 && q < n; ++q) out[q] = (uint8_t)snap_one(labels[q], mask[q], paint, a0, a1, a2, a3, K);
    }
  }
}

// the checks the three SLIC entries share; nx_out: cells per row
int slic_check(const char* who, int step, int H, int W, int K, int* nx_out) {
  SEGK_REQUIRE(step >= SEGK_SLIC_MIN_STEP && step <= SEGK_SLIC_MAX_STEP, "%s: step %d (%d..%d)", who, step, SEGK_SLIC_MIN_STEP, SEGK_SLIC_MAX_STEP);
  SEGK_REQUIRE(H >= 1 && W >= 1 && H <= SEGK_SLIC_MAX_SIDE && W <= SEGK_SLIC_MAX_SIDE, "%s: bad shape %d x %d (sides 1..2^27)", who, H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "%s: %d x %d pixels, at most 2^28", who, H, W);
  const long ny = ((long)H + step - 1) / step, nx = ((long)W + step - 1) / step;
  SEGK_REQUIRE((long)K == ny * nx, "%s: K %d is not the grid %ld x %ld of step %d", who, K, ny, nx, step);
  *nx_out = (int)nx;
  return 0;
}

int image_check(const char* who, const uint8_t* image, int C, int space) {
  SEGK_REQUIRE(C == 1 || C == 3 || C == 4, "%s: C %d (1, 3 or 4)", who, C);
  SEGK_REQUIRE(space == SEGK_SLIC_RGB || space == SEGK_SLIC_YCC, "%s: space %d (0 rgb, 1 ycc)", who, space);
  SEGK_REQUIRE(image != nullptr, "%s: NULL pointer", who);
  return 0;
}

// rows of a tile: the result does not depend on it; the host layer takes fewer for a small image, to fill the device
int rows_check(const char* who, int tile_rows) {
  SEGK_REQUIRE(tile_rows == 4 || tile_rows == 16 || tile_rows == SEGK_SLIC_TILE, "%s: tile_rows %d (4, 16 or %d)", who, tile_rows, SEGK_SLIC_TILE);
  return 0;
}

inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int segk_slic_start(const uint8_t* image, int32_t* centres, int32_t* sums, int C, int space, int step, int H, int W, int K,
                               segk_stream_t s) {
  SEGK_REQUIRE(centres && sums, "slic_start: NULL pointer");
  if (const int rc = image_check("slic_start", image, C, space)) return rc;
  int nx;
  if (const int rc = slic_check("slic_start", step, H, W, K, &nx)) return rc;
  SEGK_REQUIRE((((uintptr_t)centres) & 3) == 0 && (((uintptr_t)sums) & 15) == 0, "slic_start: centres 4-byte, sums 16-byte aligned");
  hipLaunchKernelGGL(slic_start_kernel, dim3(blocks_of(K)), dim3(256), 0, (hipStream_t)s, image, centres, sums, C, space, step, H, W, nx, K);
  SEGK_CHECK_LAUNCH("slic_start");
  return 0;
}

extern "C" int segk_slic_assign(const uint8_t* image, const int32_t* centres, int32_t* sums, int32_t* labels, int C, int space, int step,
                                int compactness, int round, int iterations, int tile_rows, int H, int W, int K, segk_stream_t s) {
  SEGK_REQUIRE(centres && sums && labels, "slic_assign: NULL pointer");
  if (const int rc = image_check("slic_assign", image, C, space)) return rc;
  int nx;
  if (const int rc = slic_check("slic_assign", step, H, W, K, &nx)) return rc;
  SEGK_REQUIRE(compactness >= 1 && compactness <= SEGK_SLIC_MAX_COMPACTNESS, "slic_assign: compactness %d (1..%d)", compactness,
               SEGK_SLIC_MAX_COMPACTNESS);
  SEGK_REQUIRE(iterations >= 1 && iterations <= SEGK_SLIC_MAX_ITERATIONS, "slic_assign: iterations %d (1..%d)", iterations,
               SEGK_SLIC_MAX_ITERATIONS);
  SEGK_REQUIRE(round >= 0 && round < iterations, "slic_assign: round %d of %d", round, iterations);
  if (const int rc = rows_check("slic_assign", tile_rows)) return rc;
  SEGK_REQUIRE(((((uintptr_t)centres) | ((uintptr_t)labels)) & 3) == 0 && (((uintptr_t)sums) & 15) == 0,
               "slic_assign: centres and labels 4-byte, sums 16-byte aligned");
  SEGK_REQUIRE((const void*)labels != (const void*)centres && (const void*)labels != (const void*)sums && (const void*)centres != (const void*)sums,
               "slic_assign: centres, sums and labels are distinct buffers");
  const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + tile_rows - 1) / tile_rows, ny = K / nx;
  hipLaunchKernelGGL(slic_assign_kernel, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)s, image, centres, sums, labels, C,
                     space, step, compactness * compactness, H, W, ny, nx, tiles_x, tile_rows, round == iterations - 1 ? 1 : 0);
  SEGK_CHECK_LAUNCH("slic_assign");
  return 0;
}

extern "C" int segk_slic_update(int32_t* centres, int32_t* sums, int32_t* counts, int step, int H, int W, int K, segk_stream_t s) {
  SEGK_REQUIRE(centres && sums && counts, "slic_update: NULL pointer");
  int nx;
  if (const int rc = slic_check("slic_update", step, H, W, K, &nx)) return rc;
  SEGK_REQUIRE(((((uintptr_t)centres) | ((uintptr_t)counts)) & 3) == 0 && (((uintptr_t)sums) & 15) == 0,
               "slic_update: centres and counts 4-byte, sums 16-byte aligned");
  SEGK_REQUIRE(counts != centres && counts != sums && centres != sums, "slic_update: centres, sums and counts are distinct buffers");
  hipLaunchKernelGGL(slic_update_kernel, dim3(blocks_of(K)), dim3(256), 0, (hipStream_t)s, centres, sums, counts, step, nx, K);
  SEGK_CHECK_LAUNCH("slic_update");
  return 0;
}

extern "C" int segk_snap_vote(const int32_t* labels, const uint8_t* mask, const uint8_t* weights, int64_t* hist, int classes_mask, int tile_rows,
                              int H, int W, int K, segk_stream_t s) {
  SEGK_REQUIRE(labels && mask && hist, "snap_vote: NULL pointer");
  SEGK_REQUIRE(classes_mask >= 1 && classes_mask <= 255, "snap_vote: classes_mask %d (bits 0..7, at least one)", classes_mask);
  if (const int rc = rows_check("snap_vote", tile_rows)) return rc;
  SEGK_REQUIRE(H >= 1 && W >= 1, "snap_vote: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "snap_vote: %d x %d pixels, at most 2^28", H, W);
  SEGK_REQUIRE(K >= 1 && K <= SEGK_CC_MAX_PIXELS, "snap_vote: K %d (1..2^28)", K);
  SEGK_REQUIRE((((uintptr_t)labels) & 3) == 0 && (((uintptr_t)hist) & 7) == 0, "snap_vote: labels 4-byte, hist 8-byte aligned");
  const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + tile_rows - 1) / tile_rows;
  hipLaunchKernelGGL(snap_vote_kernel, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)s, labels, mask, weights, (u64*)hist,
                     classes_mask, H, W, K, tiles_x, tile_rows);
  SEGK_CHECK_LAUNCH("snap_vote");
  return 0;
}

extern "C" int segk_snap_paint(const int32_t* labels, const uint8_t* mask, const int64_t* hist, int32_t* winner, uint8_t* paint, uint8_t* out,
                               long allow0, long allow1, long allow2, long allow3, int min_share, int H, int W, int K, segk_stream_t s) {
  SEGK_REQUIRE(labels && mask && hist && winner && paint && out, "snap_paint: NULL pointer");
  SEGK_REQUIRE(min_share >= 0 && min_share <= 256, "snap_paint: min_share %d (0..256 of 256)", min_share);
  SEGK_REQUIRE(H >= 1 && W >= 1, "snap_paint: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "snap_paint: %d x %d pixels, at most 2^28", H, W);
  SEGK_REQUIRE(K >= 1 && K <= SEGK_CC_MAX_PIXELS, "snap_paint: K %d (1..2^28)", K);
  SEGK_REQUIRE(((((uintptr_t)labels) | ((uintptr_t)winner)) & 3) == 0 && (((uintptr_t)hist) & 7) == 0,
               "snap_paint: labels and winner 4-byte, hist 8-byte aligned");
  SEGK_REQUIRE(out != mask && out != paint && paint != mask, "snap_paint: out is neither mask nor paint");
  const long n = (long)H * W;
  const int wide = ((((uintptr_t)labels) & 15) == 0 && ((((uintptr_t)mask) | ((uintptr_t)out)) & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(snap_winner_kernel, dim3(blocks_of(K)), dim3(256), 0, (hipStream_t)s, (const u64*)hist, winner, paint, min_share, K);
  SEGK_CHECK_LAUNCH("snap_paint (winner)");
  const long groups = (n + 3) / 4;
  const unsigned blocks = blocks_of(groups) < 4096u ? blocks_of(groups) : 4096u;
  hipLaunchKernelGGL(snap_paint_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)s, labels, mask, (const uint8_t*)paint, out, (u64)allow0, (u64)allow1,
                     (u64)allow2, (u64)allow3, n, K, wide);
  SEGK_CHECK_LAUNCH("snap_paint");
  return 0;
}
