// Label rasterisation on the device: COCO-style polygons and uncompressed run-length codes of a
// ragged batch of images -> uint8 label maps, one launch.  The reference holds no code for this; the arithmetic is this
// project's definition, every value is an integer and the result is unique, so the device equals the restatement of
// tests/raster_reference.py bit for bit.
//
// One workgroup per tile of 64 rows x 256 columns.  The host builds every table (image_segmentation_amd/raster.py): the
// fixed-point edges of all rings, the cumulative run starts, a record per shape, per tile the list of the shapes whose
// bounding box meets it (in paint order) and a record per tile.  The tile lives in LDS from the fill to the store, so every
// output byte is written exactly once; no workgroup waits for another and nothing is an atomic on global memory.
//
//  polygon  a 64 x 256-bit plane in LDS.  A lane takes an edge; for every tile row the edge crosses it toggles (LDS XOR: the
//           order does not matter) the bit of the first column whose centre counts the crossing -- column 0 for a crossing
//           left of the tile, nothing for one at or right of its end.  The crossing column steps from row to row by quotient
//           and remainder.  Then lane (row, quarter) takes its two words of the plane (and leaves them zero for the next
//           polygon), a prefix XOR -- inside the 32-bit words, then across the 8 words of the row -- turns the toggles into
//           the even-odd parity, and the lane paints the value into its own 64 pixels where the bit is set.
//  RLE      a lane per pixel searches run_start[begin:end) for t = x*H + y (upper bound, so empty runs are stepped over); an
//           odd run index paints the value.  The 64 lanes of a wave hold 64 consecutive t: they walk the same search path.
//
// A tile's list is taken 64 shapes at a time: the lanes of one wave read their records into LDS, so the dependent pair of
// loads (list entry, record) is paid per round and not per shape.
//
// The tables live in device memory where the entry cannot see them: every index read from a table is clamped to its
// argument (n_shapes, n_edges, n_runs, list_len) and a tile whose record does not fit out_bytes writes nothing.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int TH = SEGK_RAST_TILE_H, TW = SEGK_RAST_TILE_W;
constexpr int ROW_WORDS = TW / 32;          // words of the bit plane per tile row
constexpr int LAB_WORDS = TW / 4;           // words of the label tile per row
constexpr int ROUND = 64;                   // shapes of a tile's list taken at a time
static_assert(TH == 64 && TW == 256, "256 lanes: two plane words and 64 pixels each, a wave stores one tile row");
static_assert(sizeof(segk_rast_shape) == 32 && sizeof(segk_rast_tile) == 32, "table records are 32 bytes");

struct Rec { int kind, value, begin, end, H; };             // a shape record with its range clamped; kind -1: skipped

// the toggles of one edge in the rows [y0, y1) and columns [x0, x1) of the image
__device__ __forceinline__ void edge_toggles(const int4 e, int y0, int y1, int x0, int x1, uint32_t* __restrict__ s_bits) {
  int X0 = e.x, Y0 = e.y, X1 = e.z, Y1 = e.w;
  if (Y0 == Y1) return;                                        // horizontal edges never cross
  if (Y0 > Y1) { int t = X0; X0 = X1; X1 = t; t = Y0; Y0 = Y1; Y1 = t; }
  // rows whose centre 256 y + 128 lies in [Y0, Y1)
  int ya = (Y0 + 127) >> 8, yb = (Y1 + 127) >> 8;
  ya = ya < y0 ? y0 : ya;
  yb = yb > y1 ? y1 : yb;
  if (ya >= yb) return;
  const int xmin = X0 < X1 ? X0 : X1;
  if (((xmin + 127) >> 8) >= x1) return;                       // every crossing lies right of the last centre of the tile
  // first counting centre of row y: Xc >= X0 + ceil(dx (Yc - Y0) / dy); N = dx (Yc - Y0) = q dy + r, 0 <= r < dy.
  // |dx|, dy <= 2^23, |q| <= |dx| + 1 and r < dy: 32-bit words hold everything but N
  const int dy = Y1 - Y0, dx = X1 - X0;
  int q = 0, r = 0, sq = 0, sr = 0;
  if (dx != 0) {
    // The ONE 64-bit division of this edge and tile, as a float64 division: |N| < 2^46 and dy are exact doubles and the
    // quotient is rounded correctly, so its floor is the true floor or one above it; the remainder tells which
    const long long N = (long long)dx * (long long)(256 * ya + 128 - Y0);
    q = (int)floor((double)N / (double)dy);
    long long r64 = N - (long long)q * dy;
    if (r64 < 0) { r64 += dy; --q; }
    else if (r64 >= dy) { r64 -= dy; ++q; }
    r = (int)r64;
    if (yb - ya > 1) {
      // N steps by 256 dx from row to row: floor division of the magnitudes, |256 dx| <= 2^31, in 32 bits.  More than one
      // row means dy > 256, so |sq| < 2^23
      const uint32_t mag = (uint32_t)(dx < 0 ? -dx : dx) << 8, udy = (uint32_t)dy;
      const uint32_t mq = mag / udy, mr = mag - mq * udy;
      if (dx > 0) { sq = (int)mq; sr = (int)mr; }
      else if (mr == 0) { sq = -(int)mq; sr = 0; }
      else { sq = -(int)mq - 1; sr = (int)(udy - mr); }
    }
  }
  for (int y = ya; y < yb; ++y) {
    const int xm = X0 + q + (r > 0 ? 1 : 0);
    int col = (xm + 127) >> 8;
    if (col < x1) {
      col = col < x0 ? 0 : col - x0;
      atomicXor(&s_bits[(y - y0) * ROW_WORDS + (col >> 5)], 1u << (col & 31));
    }
    q += sq;
    r += sr;
    if (r >= dy) { r -= dy; ++q; }
  }
}

__global__ __launch_bounds__(256) void raster_labels_kernel(const segk_rast_tile* __restrict__ tiles, int n_tiles,
                                                            const segk_rast_shape* __restrict__ shapes, int n_shapes,
                                                            const int32_t* __restrict__ shape_list, int list_len,
                                                            const int4* __restrict__ edges, int n_edges,
                                                            const int32_t* __restrict__ run_start, int n_runs,
                                                            uint8_t* __restrict__ out, long out_bytes, int fill) {
  __shared__ uint32_t s_lab[TH * LAB_WORDS];
  __shared__ uint32_t s_bits[TH * ROW_WORDS];
  __shared__ Rec s_rec[ROUND];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= n_tiles) return;
  const segk_rast_tile T = tiles[blockIdx.x];
  const int H = T.H, W = T.W, y0 = T.y0, x0 = T.x0;
  // a record that does not describe a tile inside out[0, out_bytes) writes nothing (the same words for every lane)
  if (H < 1 || W < 1 || H > SEGK_RAST_MAX_SIDE || W > SEGK_RAST_MAX_SIDE || y0 < 0 || x0 < 0 || y0 >= H || x0 >= W) return;
  if (T.out_off < 0 || T.out_off > out_bytes || (long)H * W > out_bytes - T.out_off) return;
  const int y1 = y0 + TH < H ? y0 + TH : H, x1 = x0 + TW < W ? x0 + TW : W;
  const int l0 = clampi(T.list0, 0, list_len), l1 = clampi(T.list1, l0, list_len);

  const uint32_t fill4 = (uint32_t)(fill & 255) * 0x01010101u;
  for (int i = tid; i < TH * LAB_WORDS; i += 256) s_lab[i] = fill4;
  s_bits[tid] = 0;                                             // the plane is zero between polygons: who reads a word clears it
  s_bits[tid + 256] = 0;

  for (int c0 = l0; c0 < l1; c0 += ROUND) {
    const int n = l1 - c0 < ROUND ? l1 - c0 : ROUND;
    __syncthreads();                                           // the round before has been read (first round: the fill is done)
    if (tid < n) {
      Rec rec = {-1, 0, 0, 0, 1};
      const int si = shape_list[c0 + tid];
      if ((unsigned)si < (unsigned)n_shapes) {
        const segk_rast_shape S = shapes[si];
        const int cap = S.kind == SEGK_RAST_POLYGON ? n_edges : n_runs;
        rec.kind = S.kind == SEGK_RAST_POLYGON ? SEGK_RAST_POLYGON : SEGK_RAST_RLE;
        rec.value = S.value & 255;
        rec.begin = clampi(S.begin, 0, cap);
        rec.end = clampi(S.end, rec.begin, cap);
        rec.H = S.H;
      }
      s_rec[tid] = rec;
    }
    __syncthreads();
    for (int li = 0; li < n; ++li) {
      const Rec S = s_rec[li];                                 // the same words for every lane: the branches are uniform
      if (S.kind < 0) continue;
      if (S.kind == SEGK_RAST_POLYGON) {
        for (int e = S.begin + tid; e < S.end; e += 256) edge_toggles(edges[e], y0, y1, x0, x1, s_bits);
        __syncthreads();
        // lane = (row tid / 4, quarter tid % 4): its two words of the plane, columns 64 (tid % 4) .. + 63
        uint32_t a = s_bits[2 * tid], b = s_bits[2 * tid + 1];
        if (a | b) {
          s_bits[2 * tid] = 0;
          s_bits[2 * tid + 1] = 0;
        }
        // prefix XOR inside the words, then across the four lanes of the row
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          a ^= a << o;
          b ^= b << o;
        }
        const uint32_t mine = (a ^ b) >> 31;
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 4; o <<= 1) {
          const uint32_t u = __shfl_up(inc, o, 4);
          if ((tid & 3) >= o) inc ^= u;
        }
        const uint32_t carry = inc ^ mine;                     // parity of the words left of this pair
        a ^= 0u - carry;
        b ^= 0u - (a >> 31);                                   // a's last bit now is the parity up to its end
        if (a | b) {
          // paint the lane's own 64 pixels, four per LDS word; the word order is rotated by the lane so that the lanes of
          // a wave spread over the banks (the words of two lanes lie 16 apart)
          const uint32_t val4 = (uint32_t)S.value * 0x01010101u;
          uint32_t* mine16 = s_lab + (tid >> 2) * LAB_WORDS + (tid & 3) * 16;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int jj = (j + tid) & 15;
            const uint32_t four = ((jj < 8 ? a : b) >> ((jj & 7) * 4)) & 15u;
            if (four) {
              const uint32_t m = ((four * 0x00204081u) & 0x01010101u) * 0xffu;         // bit i of `four` -> byte i
              mine16[jj] = (mine16[jj] & ~m) | (val4 & m);
            }
          }
        }
        __syncthreads();
      } else {
        uint8_t* lab8 = (uint8_t*)s_lab;
        const int row = tid & 63, y = y0 + row;
        for (int c = tid >> 6; c < TW; c += 4) {
          const int x = x0 + c;
          if (y < y1 && x < x1) {
            const int t = x * S.H + y;
            int lo = S.begin, hi = S.end;                      // the number of run starts <= t, less one, is the run of t
            for (int it = 0; it < 32 && lo < hi; ++it) {       // at most log2(n_runs) + 1 halvings
              const int mid = (lo + hi) >> 1;
              if (run_start[mid] <= t) lo = mid + 1;
              else hi = mid;
            }
            if (lo > S.begin && ((lo - S.begin - 1) & 1)) lab8[row * TW + c] = (uint8_t)S.value;
          }
        }
        __syncthreads();
      }
    }
  }
  __syncthreads();

  // store: a wave per row, lane = one 4-byte-aligned word of the output row; the row starts `a` bytes into its first word
  const int lane = tid & 63, ncols = x1 - x0;
  for (int row = tid >> 6; row < y1 - y0; row += 4) {
    const long base = T.out_off + (long)(y0 + row) * W + x0;
    const int a = (int)(((uintptr_t)out + (uintptr_t)base) & 3);
    for (int w = lane; w <= LAB_WORDS; w += 64) {
      const int c0 = 4 * w - a;                                // tile column of the word's first byte
      if (c0 >= ncols) continue;
      if (c0 >= 0 && c0 + 3 < ncols) {
        const int k = c0 >> 2, sh = (c0 & 3) * 8;
        const uint32_t lo = s_lab[row * LAB_WORDS + k];
        const uint32_t hi = sh ? s_lab[row * LAB_WORDS + k + 1] : 0u;      // k + 1 <= 63: c0 + 3 < 256 and c0 % 4 != 0
        *(uint32_t*)(out + base + c0) = (uint32_t)((((unsigned long long)hi << 32) | lo) >> sh);
      } else {
        const uint8_t* lab8 = (const uint8_t*)s_lab;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j >= 0 && c0 + j < ncols) out[base + c0 + j] = lab8[row * TW + c0 + j];
      }
    }
  }
}

}  // namespace

extern "C" int segk_raster_labels(const segk_rast_tile* tiles, int n_tiles, const segk_rast_shape* shapes, int n_shapes,
                                  const int32_t* shape_list, int list_len, const int32_t* edges, int n_edges,
                                  const int32_t* run_start, int n_runs, uint8_t* out, long out_bytes, int fill, segk_stream_t s) {
  SEGK_REQUIRE(tiles && shapes && shape_list && edges && run_start && out, "raster_labels: NULL pointer");
  SEGK_REQUIRE(n_tiles >= 1 && n_tiles <= (1 << 30), "raster_labels: n_tiles=%d (1..2^30)", n_tiles);
  SEGK_REQUIRE(n_shapes >= 0 && list_len >= 0 && n_edges >= 0 && n_runs >= 0,
               "raster_labels: negative table length (n_shapes=%d list_len=%d n_edges=%d n_runs=%d)", n_shapes, list_len, n_edges,
               n_runs);
  SEGK_REQUIRE(out_bytes >= n_tiles, "raster_labels: out_bytes=%ld cannot hold %d tiles", out_bytes, n_tiles);
  SEGK_REQUIRE(fill >= 0 && fill <= 255, "raster_labels: fill=%d (0..255)", fill);
  SEGK_REQUIRE(((uintptr_t)tiles & 7) == 0 && ((uintptr_t)shapes & 3) == 0 && ((uintptr_t)shape_list & 3) == 0 &&
                   ((uintptr_t)edges & 15) == 0 && ((uintptr_t)run_start & 3) == 0,
               "raster_labels: misaligned table (tiles 8, edges 16, the others 4 bytes)");
  hipLaunchKernelGGL(raster_labels_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)s, tiles, n_tiles, shapes, n_shapes,
                     shape_list, list_len, (const int4*)edges, n_edges, run_start, n_runs, out, out_bytes, fill);
  SEGK_CHECK_LAUNCH("raster_labels");
  return 0;
}
