// Mask vectorisation on the device: the column-major run table of an object map, the directed unit
// boundary edges of its objects, their rings (cycles of the successor rule) and the corner vertices of every ring.  The
// reference holds no code for this; the arithmetic is this project's definition, every value is an integer and the result is
// unique, so the device equals the restatement of tests/vector_reference.py bit for bit.
//
// The host knows neither the object count nor any of the totals: grids are sized from H, W and the capacities, a kernel reads
// the counts it needs from device memory (totals[], written by an earlier launch of the same call) and grid-strides over them.
// Every loop is bounded by an argument; no workgroup waits for another (every prefix sum is reduce, then scan of the block
// partials by ONE workgroup, then scan again with the block's base); order between the launches is stream order.  The prefix
// inside a workgroup (block_scan) and the scan of the partials (wg_scan) are the object kernels' shared ones: scan.hpp
// (DESIGN.md 3.20).
//
//  segk_vec_runs
//   vec_runs_kernel<false>  one workgroup per tile of 128 rows x 32 columns: rows read whole (coalesced) into LDS, 8 lanes walk one
//                           column segment: run starts per (column, tile row) in t-order
//   vec_scan_kernel         wg_scan of those counts, totals[0]
//   vec_runs_kernel<true>   the same walk with the segment's base: run_start / run_obj
//  segk_vec_rings           E edges, R rings, V vertices; J = ceil(log2(max_edges)) + 1 rounds
//   vec_sides_kernel        side mask of every pixel (4 bits: the sides that carry an edge), edges per block of 2048 pixels
//   vec_scan_kernel         totals[1] = E
//   vec_edges_kernel        edge base of every pixel, the edge keys in ascending order (edge index = rank of its key)
//   vec_succ_kernel         successor of every edge from the four pixels at its end vertex; the successor's corner flag
//   vec_jump_kernel<MIN>    J rounds, double-buffered: (next, min) -> the ring's smallest edge index = its head
//   vec_cut_kernel          the edge before the head ends the list
//   vec_jump_kernel<SUM>    J rounds: (next, distance to the end of the list)
//   vec_heads_kernel<false> per block of 2048 edges: (heads, their ring lengths) as one 64-bit word
//   vec_scan_kernel         totals[2] = R
//   vec_heads_kernel<true>  ring index and first slot of every ring (ascending head), ring_obj / ring_head / ring_len
//   vec_order_kernel        every edge to slot first + distance from the head; ring_area2 by 64-bit integer atomics
//   vec_verts_kernel<false> corners and ring starts per block of 2048 slots
//   vec_scan_kernel         totals[3] = V
//   vec_verts_kernel<true>  xy of the corners, ring_offset, ring_area2
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int CH = SEGK_VEC_CHUNK;          // items a workgroup scans
constexpr int RY = SEGK_VEC_RUN_ROWS;       // rows and columns of a run-table tile
constexpr int RX = 32;
static_assert(CH == 8 * 256 && RY == 128, "a workgroup scans 8 items per thread; 8 lanes x 16 rows walk a column segment");

// workspace layout in 32-bit words (SEGK_VEC_WS_INTS of the header): the 64-bit arrays come first
struct Ws {
  u64 *area, *bpart;
  int2 *ja, *jb;
  int *key, *succ, *head, *pixbase, *ppart;
  uint8_t *corner, *sides;
};
__host__ __device__ inline Ws ws_split(int32_t* ws, long hw, long me) {
  Ws w;
  int32_t* p = ws + 16;
  w.area = (u64*)p;      p += r4(2 * (me / 4 + 1));
  w.bpart = (u64*)p;     p += r4(2 * ((me + CH - 1) / CH));
  w.ja = (int2*)p;       p += 2 * r4(me);
  w.jb = (int2*)p;       p += 2 * r4(me);
  w.key = p;             p += r4(me);
  w.succ = p;            p += r4(me);
  w.head = p;            p += r4(me);
  w.pixbase = p;         p += r4(hw);
  w.ppart = p;           p += r4((hw + CH - 1) / CH);
  w.corner = (uint8_t*)p; p += r4((me + 3) / 4);
  w.sides = (uint8_t*)p;
  return w;
}

template <typename T> __device__ __forceinline__ int scan_count(T v);
template <> __device__ __forceinline__ int scan_count<int>(int v) { return v; }
template <> __device__ __forceinline__ int scan_count<u64>(u64 v) { return (int)(v >> 32); }

// ONE workgroup: d[0..n) -> its exclusive prefix sums, in place; the count of the sum -> *out (the high word of a 64-bit pair).
// guard: skipped when guard[1] (the edge count) exceeds cap.
template <typename T>
__global__ __launch_bounds__(256) void vec_scan_kernel(T* d, long n, int32_t* __restrict__ out, const int32_t* __restrict__ guard, int cap) {
  if (guard && guard[1] > cap) return;
  const T total = wg_scan(d, d, n);
  if (threadIdx.x == 0) *out = scan_count(total);
}

// ------------------------------------------------------------------------------------------------ run table
// workgroup b: tile row j = b % nj, tile column b / nj.  seg[x * nj + j]: the run starts of column x inside tile row j --
// ascending in t = x*H + y.  Lanes 8c .. 8c+7 walk column c of the tile, 16 rows each.
template <bool SCATTER>
__global__ __launch_bounds__(256) void vec_runs_kernel(const int32_t* __restrict__ obj, int32_t* __restrict__ seg, int32_t* __restrict__ run_start,
                                                       int32_t* __restrict__ run_obj, int H, int W, int nj, int max_runs) {
  __shared__ int s_o[RY][RX + 1];
  __shared__ int s_prev[RX];
  const int tid = threadIdx.x, j = blockIdx.x % nj, y0 = j * RY, x0 = (blockIdx.x / nj) * RX;
  for (int r = tid >> 5; r < RY; r += 8) {
    const int y = y0 + r, x = x0 + (tid & 31);
    s_o[r][tid & 31] = (y < H && x < W) ? obj[(size_t)y * W + x] : 0;
  }
  if (tid < RX) {                           // the element before the segment: above it, or the foot of the column to the left
    const int x = x0 + tid;
    int v = -1;                             // t = 0 always starts a run (ids are >= 0)
    if (x < W) {
      if (y0 > 0) v = obj[(size_t)(y0 - 1) * W + x];
      else if (x > 0) v = obj[(size_t)(H - 1) * W + x - 1];
    }
    s_prev[tid] = v;
  }
  __syncthreads();
  const int c = tid >> 3, part = tid & 7, x = x0 + c, r0 = part * 16;
  int prev = part == 0 ? s_prev[c] : s_o[r0 - 1][c];
  const int first = prev;
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int v = s_o[r0 + k][c];
    cnt += (x < W && y0 + r0 + k < H && v != prev) ? 1 : 0;
    prev = v;
  }
  int inc = cnt;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    const int u = __shfl_up(inc, o, 8);
    if (part >= o) inc += u;
  }
  if (x >= W) return;
  if (!SCATTER) {
    if (part == 7) seg[(size_t)x * nj + j] = inc;
    return;
  }
  int r = seg[(size_t)x * nj + j] + inc - cnt;
  prev = first;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int v = s_o[r0 + k][c], y = y0 + r0 + k;
    if (y < H && v != prev) {
      if (r < max_runs) { run_start[r] = x * H + y; run_obj[r] = v; }
      ++r;
    }
    prev = v;
  }
}

// ------------------------------------------------------------------------------------------------ edges
__device__ __forceinline__ int obj_at(const int32_t* __restrict__ obj, int H, int W, int y, int x) {
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? obj[(size_t)y * W + x] : 0;
}

// one pixel per lane, consecutive lanes consecutive pixels: the five loads of a wave are each whole lines of the map
__global__ __launch_bounds__(256) void vec_sides_kernel(const int32_t* __restrict__ obj, int32_t* __restrict__ wsp, int H, int W, long me) {
  __shared__ int s_w[4];
  const long hw = (long)H * W;
  const Ws ws = ws_split(wsp, hw, me);
  for (long i = thread_of(); i < me / 4 + 1; i += stride_of()) ws.area[i] = 0;
  int sum = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long p = (long)blockIdx.x * CH + k * 256 + threadIdx.x;
    if (p < hw) {
      const int y = (int)(p / W), x = (int)(p - (long)y * W);
      const int v = obj[p];
      unsigned m = 0;
      if (v != 0) {
        m = (obj_at(obj, H, W, y - 1, x) != v ? 1u : 0u) | (obj_at(obj, H, W, y, x + 1) != v ? 2u : 0u) |
            (obj_at(obj, H, W, y + 1, x) != v ? 4u : 0u) | (obj_at(obj, H, W, y, x - 1) != v ? 8u : 0u);
      }
      ws.sides[p] = (uint8_t)m;
      sum += (int)__popc(m);
    }
  }
  int total;
  block_scan<4>(sum, s_w, total);
  if (threadIdx.x == 0) ws.ppart[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void vec_edges_kernel(int32_t* __restrict__ wsp, int32_t* __restrict__ totals, int H, int W, int max_edges) {
  __shared__ int s_w[4];
  const long hw = (long)H * W;
  const Ws ws = ws_split(wsp, hw, max_edges);
  if (totals[1] > max_edges) {               // the same word for every workgroup: all of them leave here
    if (blockIdx.x == 0 && threadIdx.x == 0) { totals[2] = -1; totals[3] = -1; }
    return;
  }
  int carry = ws.ppart[blockIdx.x];
  for (int k = 0; k < 8; ++k) {
    const long p = (long)blockIdx.x * CH + k * 256 + threadIdx.x;
    const unsigned m = p < hw ? ws.sides[p] : 0u;
    int total;
    int e = carry + block_scan<4>((int)__popc(m), s_w, total);
    carry += total;
    if (p < hw) ws.pixbase[p] = e;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if ((m >> s) & 1u) {
        if (e < max_edges) ws.key[e] = 4 * (int)p + s;
        ++e;
      }
  }
}

// Edge loops count in int: E <= max_edges <= 2^30 and the grid stride (flat_grid: at most 8 workgroups per CU) is far below
// 2^30, so an index plus one stride still fits; thread_of and stride_of themselves are long (scan.hpp).
// successor of edge e = (pixel, side d): of the edges that leave its end vertex (vx, vy) with the object on their right --
// E: top of the pixel SE of the vertex, S: right of SW, W: bottom of NW, N: left of NE -- the first that exists of right turn,
// straight, left turn (connectivity 4) or left turn, straight, right turn (connectivity 8).
__global__ __launch_bounds__(256) void vec_succ_kernel(const int32_t* __restrict__ obj, int32_t* __restrict__ wsp, const int32_t* __restrict__ totals,
                                                       int H, int W, int conn8, int max_edges) {
  const Ws ws = ws_split(wsp, (long)H * W, max_edges);
  const int E = totals[1];
  if (E > max_edges) return;
  for (int e = (int)thread_of(); e < E; e += (int)stride_of()) {
    const int key = ws.key[e], p = key >> 2, d = key & 3;
    const int y = p / W, x = p - y * W, k = obj[p];
    const int vx = x + ((d == 0 || d == 1) ? 1 : 0), vy = y + ((d == 1 || d == 2) ? 1 : 0);
    const bool nw = obj_at(obj, H, W, vy - 1, vx - 1) == k, ne = obj_at(obj, H, W, vy - 1, vx) == k;
    const bool sw = obj_at(obj, H, W, vy, vx - 1) == k, se = obj_at(obj, H, W, vy, vx) == k;
    const unsigned exists = (se && !ne ? 1u : 0u) | (sw && !se ? 2u : 0u) | (nw && !sw ? 4u : 0u) | (ne && !nw ? 8u : 0u);
    const int right = (d + 1) & 3, left = (d + 3) & 3;
    const int c0 = conn8 ? left : right, c2 = conn8 ? right : left;
    int nd = -1;
    if ((exists >> c0) & 1u) nd = c0;
    else if ((exists >> d) & 1u) nd = d;
    else if ((exists >> c2) & 1u) nd = c2;
    int s = e;
    if (nd >= 0) {
      const int py = vy - ((nd == 2 || nd == 3) ? 1 : 0), px = vx - ((nd == 1 || nd == 2) ? 1 : 0);
      const int q = py * W + px;
      s = ws.pixbase[q] + __popc((unsigned)ws.sides[q] & ((1u << nd) - 1u));
      if ((unsigned)s >= (unsigned)E) s = e;                 // cannot happen: every edge has a successor among the E
    }
    ws.succ[e] = s;
    ws.ja[e] = make_int2(s, e);
    if (s != e) ws.corner[s] = (uint8_t)(nd != d);           // s has this one predecessor
  }
}

// one round of pointer jumping, src -> dst: .x the edge 2^round steps ahead, .y the minimum (MIN) or the sum of what lies between
template <bool MIN>
__global__ __launch_bounds__(256) void vec_jump_kernel(const int2* __restrict__ src, int2* __restrict__ dst, const int32_t* __restrict__ totals,
                                                       int max_edges) {
  const int E = totals[1];
  if (E > max_edges) return;
  for (int e = (int)thread_of(); e < E; e += (int)stride_of()) {
    const int2 a = src[e];
    const int2 b = src[a.x];
    dst[e] = make_int2(b.x, MIN ? (a.y < b.y ? a.y : b.y) : a.y + b.y);
  }
}

// src: (., head) of every edge.  dst: the list that starts at the head -- the edge whose successor is the head ends it
__global__ __launch_bounds__(256) void vec_cut_kernel(const int2* __restrict__ src, int2* __restrict__ dst, const int* __restrict__ succ,
                                                      int* __restrict__ head, const int32_t* __restrict__ totals, int max_edges) {
  const int E = totals[1];
  if (E > max_edges) return;
  for (int e = (int)thread_of(); e < E; e += (int)stride_of()) {
    const int h = src[e].y, s = succ[e];
    head[e] = h;
    dst[e] = s == h ? make_int2(e, 0) : make_int2(s, 1);
  }
}

// dist: (., edges from here to the end of the list).  A head's ring has dist + 1 edges.  rec (SCATTER): (ring, first slot) at
// the head.  The scanned word: heads << 32 | ring lengths.
template <bool SCATTER>
__global__ __launch_bounds__(256) void vec_heads_kernel(const int32_t* __restrict__ obj, int32_t* __restrict__ wsp, const int2* __restrict__ dist,
                                                        int2* __restrict__ rec, const int32_t* __restrict__ totals, int32_t* __restrict__ ring_obj,
                                                        int32_t* __restrict__ ring_head, int32_t* __restrict__ ring_len, int H, int W,
                                                        int max_edges, int max_rings) {
  __shared__ u64 s_w[4];
  const Ws ws = ws_split(wsp, (long)H * W, max_edges);
  const int E = totals[1];
  if (E > max_edges) return;
  u64 carry = SCATTER ? ws.bpart[blockIdx.x] : 0;
  for (int k = 0; k < 8; ++k) {
    const long e = (long)blockIdx.x * CH + k * 256 + threadIdx.x;
    const bool is_head = e < E && ws.head[e] == (int)e;
    const int len = is_head ? dist[e].y + 1 : 0;
    u64 total;
    const u64 ex = carry + block_scan<4>(is_head ? ((1ull << 32) | (u64)(unsigned)len) : 0ull, s_w, total);
    carry += total;
    if (SCATTER && is_head) {
      const int ring = (int)(ex >> 32), first = (int)(ex & 0xffffffffu);
      rec[e] = make_int2(ring, first);
      if (ring < max_rings) {
        const int key = ws.key[e];
        ring_obj[ring] = obj[key >> 2];
        ring_head[ring] = key;
        ring_len[ring] = len;
      }
    }
  }
  if (!SCATTER && threadIdx.x == 0) ws.bpart[blockIdx.x] = carry;
}

// twice the signed area an edge adds: x0*y1 - x1*y0 over its two ends
__device__ __forceinline__ long long edge_area2(int key, int W) {
  const int p = key >> 2, d = key & 3, y = p / W, x = p - y * W;
  return d == 0 ? -(long long)y : d == 1 ? (long long)(x + 1) : d == 2 ? (long long)(y + 1) : -(long long)x;
}

// ord[slot] = key | corner << 30 | ring start << 31 with slot = the ring's first + distance from its head (ord is the
// successor array: not needed any more).  A wave whose edges all lie on one ring adds their areas as one atomic.
__global__ __launch_bounds__(256) void vec_order_kernel(int32_t* __restrict__ wsp, const int2* __restrict__ dist, const int2* __restrict__ rec,
                                                        const int32_t* __restrict__ totals, int H, int W, int max_edges) {
  const Ws ws = ws_split(wsp, (long)H * W, max_edges);
  const int E = totals[1];
  if (E > max_edges) return;
  const int lane = threadIdx.x & 63, nslot = max_edges / 4 + 1;
  const int stride = (int)stride_of(), rounds = (E + stride - 1) / stride;
  for (int it = 0; it < rounds; ++it) {                       // whole waves stay together for the ballots
    const int e = it * stride + (int)thread_of();
    bool valid = e < E;
    int ring = -1;
    long long a2 = 0;
    if (valid) {
      const int h = ws.head[e], key = ws.key[e];
      const int2 r = rec[h];
      const int slot = r.y + dist[h].y - dist[e].y;
      ring = r.x;
      valid = (unsigned)slot < (unsigned)E && (unsigned)ring < (unsigned)nslot;      // cannot fail
      if (valid) {
        ws.succ[slot] = (int)((unsigned)key | ((unsigned)ws.corner[e] << 30) | (e == h ? 0x80000000u : 0u));
        a2 = edge_area2(key, W);
      }
    }
    const u64 vm = __ballot(valid);
    if (!vm) continue;
    const int lead = __ffsll((long long)vm) - 1, ring0 = __shfl(ring, lead);
    if (__ballot(valid && ring != ring0) == 0) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) a2 += __shfl_xor(a2, o);
      if (lane == lead) atomicAdd(ws.area + ring0, (u64)a2);
    } else if (valid) {
      atomicAdd(ws.area + ring, (u64)a2);
    }
  }
}

// the scanned word: corners << 32 | ring starts
template <bool SCATTER>
__global__ __launch_bounds__(256) void vec_verts_kernel(int32_t* __restrict__ wsp, const int32_t* __restrict__ totals, int64_t* __restrict__ ring_area2,
                                                        int32_t* __restrict__ ring_offset, int32_t* __restrict__ xy, int H, int W, int max_edges,
                                                        int max_rings, int max_vertices) {
  __shared__ u64 s_w[4];
  const Ws ws = ws_split(wsp, (long)H * W, max_edges);
  const int E = totals[1];
  if (E > max_edges) return;
  if (SCATTER && blockIdx.x == 0 && threadIdx.x == 0 && totals[2] <= max_rings) ring_offset[totals[2]] = totals[3];
  u64 carry = SCATTER ? ws.bpart[blockIdx.x] : 0;
  for (int k = 0; k < 8; ++k) {
    const long q = (long)blockIdx.x * CH + k * 256 + threadIdx.x;
    const unsigned o = q < E ? (unsigned)ws.succ[q] : 0u;
    u64 total;
    const u64 ex = carry + block_scan<4>(((u64)((o >> 30) & 1u) << 32) | (u64)(o >> 31), s_w, total);
    carry += total;
    if (!SCATTER) continue;
    const int v = (int)(ex >> 32), ring = (int)(ex & 0xffffffffu);
    if ((o >> 31) && ring <= max_rings) {
      ring_offset[ring] = v;
      if (ring < max_rings) ring_area2[ring] = (int64_t)ws.area[ring];
    }
    if (((o >> 30) & 1u) && v < max_vertices) {
      const int key = (int)(o & 0x3fffffffu), p = key >> 2, d = key & 3, y = p / W, x = p - y * W;
      xy[2 * (size_t)v] = x + ((d == 1 || d == 2) ? 1 : 0);
      xy[2 * (size_t)v + 1] = y + ((d == 2 || d == 3) ? 1 : 0);
    }
  }
  if (!SCATTER && threadIdx.x == 0) ws.bpart[blockIdx.x] = carry;
}

int flat_grid(long items) {
  long g = (items + 255) / 256;
  const long cap = 8L * segk_num_cus();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

int check_map(const char* what, int H, int W) {
  SEGK_REQUIRE(H >= 1 && W >= 1, "%s: bad shape %d x %d", what, H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "%s: %d x %d pixels, at most 2^28", what, H, W);
  return 0;
}

}  // namespace

extern "C" int segk_vec_runs(const int32_t* obj, int32_t* run_start, int32_t* run_obj, int32_t* totals, int32_t* ws, int H, int W,
                             int max_runs, segk_stream_t s) {
  SEGK_REQUIRE(obj && run_start && run_obj && totals && ws, "vec_runs: NULL pointer");
  if (int rc = check_map("vec_runs", H, W)) return rc;
  SEGK_REQUIRE(max_runs >= 1 && max_runs <= SEGK_VEC_MAX_CAP, "vec_runs: max_runs=%d (1..2^30)", max_runs);
  SEGK_REQUIRE(((uintptr_t)ws & 15) == 0, "vec_runs: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const int nj = (H + RY - 1) / RY, ntx = (W + RX - 1) / RX;
  const dim3 tiles((unsigned)((long)nj * ntx));
  hipLaunchKernelGGL(vec_runs_kernel<false>, tiles, dim3(256), 0, st, obj, ws, run_start, run_obj, H, W, nj, max_runs);
  SEGK_CHECK_LAUNCH("vec_runs (count)");
  hipLaunchKernelGGL(vec_scan_kernel<int>, dim3(1), dim3(256), 0, st, ws, (long)W * nj, totals, (const int32_t*)nullptr, 0);
  hipLaunchKernelGGL(vec_runs_kernel<true>, tiles, dim3(256), 0, st, obj, ws, run_start, run_obj, H, W, nj, max_runs);
  SEGK_CHECK_LAUNCH("vec_runs");
  return 0;
}

extern "C" int segk_vec_rings(const int32_t* obj, int32_t* ring_obj, int32_t* ring_head, int32_t* ring_len, int64_t* ring_area2,
                              int32_t* ring_offset, int32_t* xy, int32_t* totals, int32_t* ws, int H, int W, int connectivity,
                              int max_edges, int max_rings, int max_vertices, segk_stream_t s) {
  SEGK_REQUIRE(obj && ring_obj && ring_head && ring_len && ring_area2 && ring_offset && xy && totals && ws, "vec_rings: NULL pointer");
  if (int rc = check_map("vec_rings", H, W)) return rc;
  SEGK_REQUIRE(connectivity == 4 || connectivity == 8, "vec_rings: connectivity %d (4 or 8)", connectivity);
  SEGK_REQUIRE(max_edges >= 1 && max_edges <= SEGK_VEC_MAX_CAP, "vec_rings: max_edges=%d (1..2^30)", max_edges);
  SEGK_REQUIRE(max_rings >= 1 && max_rings <= SEGK_VEC_MAX_CAP, "vec_rings: max_rings=%d (1..2^30)", max_rings);
  SEGK_REQUIRE(max_vertices >= 1 && max_vertices <= SEGK_VEC_MAX_CAP, "vec_rings: max_vertices=%d (1..2^30)", max_vertices);
  SEGK_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)ring_area2 & 7) == 0, "vec_rings: ws must be 16-byte, ring_area2 8-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const long hw = (long)H * W;
  const Ws w = ws_split(ws, hw, max_edges);
  const int conn8 = connectivity == 8;
  const unsigned nbp = (unsigned)((hw + CH - 1) / CH), nbe = (unsigned)(((long)max_edges + CH - 1) / CH);
  const dim3 ge(flat_grid(max_edges)), blk(256);
  int rounds = 1;                                                    // ceil(log2(max_edges)) + 1
  while ((1L << (rounds - 1)) < max_edges) ++rounds;

  hipLaunchKernelGGL(vec_sides_kernel, dim3(nbp), blk, 0, st, obj, ws, H, W, (long)max_edges);
  SEGK_CHECK_LAUNCH("vec_rings (sides)");
  hipLaunchKernelGGL(vec_scan_kernel<int>, dim3(1), blk, 0, st, w.ppart, (long)nbp, totals + 1, (const int32_t*)nullptr, 0);
  hipLaunchKernelGGL(vec_edges_kernel, dim3(nbp), blk, 0, st, ws, totals, H, W, max_edges);
  hipLaunchKernelGGL(vec_succ_kernel, ge, blk, 0, st, obj, ws, (const int32_t*)totals, H, W, conn8, max_edges);
  int2 *src = w.ja, *dst = w.jb;
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(vec_jump_kernel<true>, ge, blk, 0, st, (const int2*)src, dst, (const int32_t*)totals, max_edges);
    int2* t = src; src = dst; dst = t;
  }
  hipLaunchKernelGGL(vec_cut_kernel, ge, blk, 0, st, (const int2*)src, dst, (const int*)w.succ, w.head, (const int32_t*)totals, max_edges);
  { int2* t = src; src = dst; dst = t; }
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(vec_jump_kernel<false>, ge, blk, 0, st, (const int2*)src, dst, (const int32_t*)totals, max_edges);
    int2* t = src; src = dst; dst = t;
  }
  SEGK_CHECK_LAUNCH("vec_rings (jumps)");
  // src: the distances; dst: free, takes (ring, first slot) at the heads
  hipLaunchKernelGGL(vec_heads_kernel<false>, dim3(nbe), blk, 0, st, obj, ws, (const int2*)src, dst, (const int32_t*)totals, ring_obj, ring_head,
                     ring_len, H, W, max_edges, max_rings);
  hipLaunchKernelGGL(vec_scan_kernel<u64>, dim3(1), blk, 0, st, w.bpart, (long)nbe, totals + 2, (const int32_t*)totals, max_edges);
  hipLaunchKernelGGL(vec_heads_kernel<true>, dim3(nbe), blk, 0, st, obj, ws, (const int2*)src, dst, (const int32_t*)totals, ring_obj, ring_head,
                     ring_len, H, W, max_edges, max_rings);
  hipLaunchKernelGGL(vec_order_kernel, ge, blk, 0, st, ws, (const int2*)src, (const int2*)dst, (const int32_t*)totals, H, W, max_edges);
  hipLaunchKernelGGL(vec_verts_kernel<false>, dim3(nbe), blk, 0, st, ws, (const int32_t*)totals, ring_area2, ring_offset, xy, H, W, max_edges,
                     max_rings, max_vertices);
  hipLaunchKernelGGL(vec_scan_kernel<u64>, dim3(1), blk, 0, st, w.bpart, (long)nbe, totals + 3, (const int32_t*)totals, max_edges);
  hipLaunchKernelGGL(vec_verts_kernel<true>, dim3(nbe), blk, 0, st, ws, (const int32_t*)totals, ring_area2, ring_offset, xy, H, W, max_edges,
                     max_rings, max_vertices);
  SEGK_CHECK_LAUNCH("vec_rings");
  return 0;
}
