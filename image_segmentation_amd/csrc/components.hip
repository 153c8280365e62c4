// Mask clean-up on the device: connected components of a uint8 class mask, their statistics and
// boxes, and removal of small / non-largest components by a one-pass neighbour vote (the colour / count / confusion
// outputs of the finished mask are segk_mask_finish, predict.hip).  The reference holds no code for this; the arithmetic
// is this project's definition, every value is an integer and the result is unique, so the device equals the restatement
// of tests/components_reference.py bit for bit whatever the tiling and the arrival order of the atomics.
//
// A component's name while it is built is its ROOT: the smallest linear index y*W + x among its pixels.  parent[p] <= p
// always holds and parents only fall, which bounds every loop below (a walk up a chain strictly decreases, a union's
// larger index strictly decreases).  No workgroup waits for another: order between the phases is stream order.
//
//  segk_cc_label
//   cc_tile_kernel     one workgroup per tile of 32 rows x 64 columns: values in LDS, a pixel links to its lowest equal backward neighbour,
//                      chains are shortened, the remaining equal neighbours are united with LDS atomicMin, and every pixel's
//                      tile root leaves as a global linear index (-1: unlabelled).  Also zeroes the accumulators.
//   cc_border_kernel   one thread per pixel on a tile border: lock-free union with its backward neighbours in other tiles
//   cc_flatten_kernel  parent[p] = root(p); area at the root (+ run_length per run head, summed per workgroup in scan.hpp's
//                      AddTable before the atomic); roots per row
//   cc_scan_kernel     one workgroup: scan.hpp's wg_scan of the H row counts, K
//   cc_rank_kernel     one wave per row: ids 1..K in raster order of the roots, the reported rows, the largest component
//                      per class (key = area << 32 | ~id: a tie goes to the lowest id)
//   cc_ids_kernel      labels[p] = id, boxes of the reported components (min / max of runs per workgroup in LDS cells found
//                      by the same tab_slot, then global atomics filtered by a coherent read)
//  segk_cc_clean
//   cc_clean_init_kernel, cc_vote_kernel, cc_apply_kernel
// The run heads, the LDS table, the scan and dev_load are the object kernels' shared ones: scan.hpp.
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int TS = SEGK_CC_TILE_W, TH = SEGK_CC_TILE_H, TP = TS * TH;     // tile width and height, pixels per tile
constexpr int RW = 8;                                    // rows a wave walks down in the flatten / ids kernels
constexpr int NC = SEGK_MAX_CLASSES;
static_assert(TS == 64 && TH == 32, "a tile row is one wave wide; local indices use shifts by 6, tile rows shifts by 5");

// workspace layout in 32-bit words (SEGK_CC_WS_INTS of the header): best[8] as 64-bit words come first (8-byte aligned)
struct Ws {
  u64* best;
  int *parent, *area, *rid, *rowcnt, *rowbase, *votes;
};
__host__ __device__ inline Ws ws_split(int32_t* ws, int H, int W) {
  const size_t hw = (size_t)H * W;
  Ws w;
  w.best = (u64*)ws;
  w.votes = ws + 16;                 // 8 per pixel, read and zeroed as two 16-byte vectors at a root
  w.parent = w.votes + 8 * hw;
  w.area = w.parent + hw;
  w.rid = w.area + hw;
  w.rowcnt = w.rid + hw;
  w.rowbase = w.rowcnt + H;
  return w;
}

__device__ __forceinline__ int wg_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- union-find on the tile (LDS) and on the image (global).  find: the chain strictly decreases.  unite: needs no
// roots -- if a (the larger) was not a root, its former parent `old` still has to meet b, and max(a, b) fell.
__device__ __forceinline__ int lds_find(const int* lab, int i) {
  int r = wg_load(lab + i);
  for (;;) {
    const int n = wg_load(lab + r);
    if (n == r) return r;
    r = n;
  }
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
  a = lds_find(lab, a);
  b = lds_find(lab, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);
    if (old == a) break;
    a = old;
  }
}
__device__ __forceinline__ int glb_find(const int* parent, int i) {
  int r = dev_load(parent + i);
  for (;;) {
    const int n = dev_load(parent + r);
    if (n == r) return r;
    r = n;
  }
}
__device__ __forceinline__ void glb_unite(int* parent, int a, int b) {
  a = glb_find(parent, a);
  b = glb_find(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    a = old;
  }
}

// ------------------------------------------------------------------------------------------------ tile labelling
__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ wsp, int32_t* __restrict__ num,
                                                      int32_t* __restrict__ cls, int32_t* __restrict__ oarea, int32_t* __restrict__ box,
                                                      int32_t* __restrict__ first, int H, int W, int conn8, unsigned cmask, int cap) {
  __shared__ uint8_t s_val[TP];       // the class of a labelled pixel, 255 otherwise (unlabelled or outside the image)
  __shared__ int s_lab[TP];
  const Ws ws = ws_split(wsp, H, W);
  const int tid = threadIdx.x, ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TS;

  // accumulators and the reported rows: zeroed here, read by later launches
  const int bid = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.x * gridDim.y;
  for (long i = (long)bid * 256 + tid; i < cap; i += (long)nb * 256) {
    cls[i] = 0; oarea[i] = 0; first[i] = 0;
    *(int4*)(box + 4 * i) = make_int4(0, 0, 0, 0);
  }
  if (bid == 0 && tid < NC) ws.best[tid] = 0;
  if (bid == 0 && tid == NC) *num = 0;
  if (blockIdx.x == 0 && tid < TH && ty0 + tid < H) ws.rowcnt[ty0 + tid] = 0;

  for (int i = tid; i < TP; i += 256) {
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    unsigned v = 255;
    if (y < H && x < W) {
      v = mask[(size_t)y * W + x];
      v = (v < NC && ((cmask >> v) & 1u)) ? v : 255u;
    }
    s_val[i] = (uint8_t)v;
  }
  __syncthreads();
  // a tile row is one wave: a pixel links to the head of its run of equal values in the row (no chain to walk)
  const int lane = tid & 63;
  for (int i = tid; i < TP; i += 256) {
    const unsigned v = s_val[i];
    const bool head = lane == 0 || s_val[i - 1] != v;
    const u64 heads = __ballot(head);
    s_lab[i] = (i & ~63) + 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  }
  __syncthreads();
  // unite the runs of neighbouring rows.  A vertical pair is redundant unless one of the two pixels heads its run (the
  // pair one column to the left joins the same two runs); a diagonal pair is redundant where a pixel between the two
  // (above, or beside) has the value: those are joined to both by pairs of their own.
  for (int i = tid; i < TP; i += 256) {
    const int ly = i >> 6;
    const unsigned v = s_val[i];
    if (v == 255 || ly == 0) continue;
    const bool up = s_val[i - TS] == v;
    if (up && (lane == 0 || s_val[i - 1] != v || s_val[i - TS - 1] != v)) lds_unite(s_lab, i, i - TS);
    if (conn8 && !up) {
      if (lane > 0 && s_val[i - TS - 1] == v && s_val[i - 1] != v) lds_unite(s_lab, i, i - TS - 1);
      if (lane < TS - 1 && s_val[i - TS + 1] == v && s_val[i + 1] != v) lds_unite(s_lab, i, i - TS + 1);
    }
  }
  __syncthreads();
  // the run heads find their roots first (few, and only they have chains); then every pixel is two steps from its root
  for (int i = tid; i < TP; i += 256)
    if (s_val[i] != 255 && (lane == 0 || s_val[i - 1] != s_val[i])) {
      const int r = lds_find(s_lab, i);
      __hip_atomic_store(s_lab + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  __syncthreads();
  for (int i = tid; i < TP; i += 256) {
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    if (y >= H || x >= W) continue;
    int g = -1;
    if (s_val[i] != 255) {
      const int r = lds_find(s_lab, i);
      g = (ty0 + (r >> 6)) * W + tx0 + (r & 63);
    }
    const size_t p = (size_t)y * W + x;
    ws.parent[p] = g;
    ws.area[p] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ border merge
// threads [0, nbr*W): the pixels of the rows y = 32, 64, ...; then per border column c two runs of H pixels: x = 64(c+1)
// (its left and upper-left neighbours lie in the tile to the left) and, connectivity 8, x = 64(c+1) - 1 (upper right)
__global__ __launch_bounds__(256) void cc_border_kernel(const uint8_t* __restrict__ mask, int* __restrict__ parent, int H, int W, int conn8,
                                                        int nbr, int nbc) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long rows = (long)nbr * W, sides = conn8 ? 2 : 1;
  int y, x;
  if (t < rows) {
    y = ((int)(t / W) + 1) * TH;
    x = (int)(t % W);
  } else {
    const long u = t - rows;
    if (u >= (long)nbc * sides * H) return;
    const int c = (int)(u / (sides * H)), rem = (int)(u % (sides * H));
    y = rem % H;
    x = (c + 1) * TS - rem / H;
  }
  const int p = y * W + x, pp = dev_load(parent + p);
  if (pp < 0) return;
  const unsigned v = mask[p];
  auto inside = [&](int qy, int qx) { return qy >= 0 && qy < H && qx >= 0 && qx < W; };
  auto has = [&](int qy, int qx) { return inside(qy, qx) && mask[qy * W + qx] == v; };      // equal to a labelled pixel: labelled too
  auto other_tile = [&](int qy, int qx) { return (qy >> 5) != (y >> 5) || (qx >> 6) != (x >> 6); };
  // a straight pair (p, q) is left to the pair one step back along the border (p', q') where that pair lies in the same
  // two tiles and shows the same two parents: equal parents mean equal sets, and the first pair of such a run has no
  // predecessor, so it is always made
  auto straight = [&](int dy, int dx) {
    const int qy = y + dy, qx = x + dx;
    if (!has(qy, qx) || !other_tile(qy, qx)) return;
    const int q = qy * W + qx;
    const int by = dy ? y : y - 1, bx = dy ? x - 1 : x;              // p': left of p for a vertical pair, above p for a horizontal one
    if (inside(by, bx) && !other_tile(by, bx) && has(by, bx) && has(by + dy, bx + dx) &&
        dev_load(parent + by * W + bx) == pp && dev_load(parent + (by + dy) * W + bx + dx) == dev_load(parent + q))
      return;
    glb_unite(parent, p, q);
  };
  straight(0, -1);
  straight(-1, 0);
  if (conn8) {                                                       // a diagonal pair only where neither pixel between has the value
    if (has(y - 1, x - 1) && other_tile(y - 1, x - 1) && !has(y - 1, x) && !has(y, x - 1)) glb_unite(parent, p, (y - 1) * W + x - 1);
    if (has(y - 1, x + 1) && other_tile(y - 1, x + 1) && !has(y - 1, x) && !has(y, x + 1)) glb_unite(parent, p, (y - 1) * W + x + 1);
  }
}

constexpr int TAB = 128;                 // slots of a workgroup's LDS table (scan.hpp): areas here, boxes in cc_ids_kernel

// ------------------------------------------------------------------------------------------------ flatten + area
// a workgroup owns 32 rows x 64 columns, a wave 8 rows of them; per row the run heads add their run's length
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int* __restrict__ area, int* __restrict__ rowcnt, int H,
                                                         int W) {
  __shared__ AddTable<TAB> tab;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * (4 * RW) + wv * RW;
  tab.clear();
  int r[RW], n[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) r[k] = (x < W && y0 + k < H) ? parent[(size_t)(y0 + k) * W + x] : -1;
#pragma unroll
  for (int k = 0; k < RW; ++k) n[k] = r[k] >= 0 ? parent[r[k]] : -1;
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    while (n[k] != r[k]) {                                         // strictly decreasing
      r[k] = n[k];
      n[k] = parent[r[k]];
    }
    if (r[k] >= 0) parent[(size_t)(y0 + k) * W + x] = r[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const int y = y0 + k;
    if (y >= H) break;                                             // wave-uniform
    const u64 roots = __ballot(r[k] >= 0 && r[k] == y * W + x);
    if (lane == 0 && roots) atomicAdd(rowcnt + y, __popcll(roots));
    const int len = run_length(r[k], lane);
    if (len && r[k] >= 0) tab.add(r[k], len, area + r[k]);
  }
  __syncthreads();
  tab.flush([&](int root) { return area + root; });
}

// ------------------------------------------------------------------------------------------------ ranking
// ONE workgroup: rowbase = the exclusive scan of the H row counts, *num = K
__global__ __launch_bounds__(256) void cc_scan_kernel(const int* __restrict__ rowcnt, int* __restrict__ rowbase, int32_t* __restrict__ num,
                                                      int H) {
  const int total = wg_scan(rowcnt, rowbase, (long)H);
  if (threadIdx.x == 0) *num = total;
}

__device__ __forceinline__ u64 cc_key(int area, int id) { return ((u64)(unsigned)area << 32) | (u64)(0xffffffffu - (unsigned)id); }

__global__ __launch_bounds__(256) void cc_rank_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ wsp, int32_t* __restrict__ cls,
                                                      int32_t* __restrict__ oarea, int32_t* __restrict__ box, int32_t* __restrict__ first,
                                                      int H, int W, int cap) {
  __shared__ u64 s_best[NC];
  const Ws ws = ws_split(wsp, H, W);
  const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (threadIdx.x < NC) s_best[threadIdx.x] = 0;
  __syncthreads();
  if (y < H) {
    int run = ws.rowbase[y];
    for (int x0 = 0; x0 < W; x0 += 256) {                          // four chunks of the row in flight together
      bool root[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + 64 * j + lane;
        root[j] = x < W && ws.parent[y * W + x] == y * W + x;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = y * W + x0 + 64 * j + lane;
        const u64 m = __ballot(root[j]);
        if (root[j]) {
          const int id = run + __popcll(m & ((1ull << lane) - 1ull)) + 1;
          const int v = mask[p], a = ws.area[p];
          ws.rid[p] = id;
          atomicMax(&s_best[v], cc_key(a, id));
          if (id <= cap) {
            cls[id - 1] = v; oarea[id - 1] = a; first[id - 1] = p;
            *(int4*)(box + 4 * (size_t)(id - 1)) = make_int4(H, W, 0, 0);
          }
        }
        run += __popcll(m);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < NC && s_best[threadIdx.x]) atomicMax(ws.best + threadIdx.x, s_best[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ ids + boxes
__global__ __launch_bounds__(256) void cc_ids_kernel(const int* __restrict__ parent, const int* __restrict__ rid, int32_t* __restrict__ labels,
                                                     int32_t* __restrict__ box, int H, int W, int cap) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * (4 * RW) + wv * RW;
  __shared__ int t_key[TAB], t_box[TAB][4];
  if (threadIdx.x < TAB) {
    t_key[threadIdx.x] = -1;
    t_box[threadIdx.x][0] = H; t_box[threadIdx.x][1] = W; t_box[threadIdx.x][2] = 0; t_box[threadIdx.x][3] = 0;
  }
  __syncthreads();
  int id[RW];
#pragma unroll
  for (int k = 0; k < RW; ++k) id[k] = (x < W && y0 + k < H) ? parent[(size_t)(y0 + k) * W + x] : -1;
#pragma unroll
  for (int k = 0; k < RW; ++k) id[k] = id[k] >= 0 ? rid[id[k]] : 0;
#pragma unroll
  for (int k = 0; k < RW; ++k)
    if (x < W && y0 + k < H) labels[(size_t)(y0 + k) * W + x] = id[k];
  // an atomic that cannot change the word is skipped on a coherent read: the word only moves towards the final value
  auto to_global = [&](int c, int ylo, int xlo, int yhi, int xhi) {
    int* b = box + 4 * (size_t)(c - 1);
    if (dev_load(b) > ylo) atomicMin(b, ylo);
    if (dev_load(b + 1) > xlo) atomicMin(b + 1, xlo);
    if (dev_load(b + 2) < yhi) atomicMax(b + 2, yhi);
    if (dev_load(b + 3) < xhi) atomicMax(b + 3, xhi);
  };
#pragma unroll
  for (int k = 0; k < RW; ++k) {
    const int y = y0 + k;
    if (y >= H) break;                                             // wave-uniform
    const int len = run_length(id[k], lane);
    if (len && id[k] >= 1 && id[k] <= cap) {
      const int h = tab_slot<TAB>(t_key, id[k]);
      if (h >= 0) {
        atomicMin(&t_box[h][0], y); atomicMin(&t_box[h][1], x); atomicMax(&t_box[h][2], y + 1); atomicMax(&t_box[h][3], x + len);
      } else to_global(id[k], y, x, y + 1, x + len);
    }
  }
  __syncthreads();
  if (threadIdx.x < TAB && t_key[threadIdx.x] >= 1) {
    const int* t = t_box[threadIdx.x];
    to_global(t_key[threadIdx.x], t[0], t[1], t[2], t[3]);
  }
}

// ------------------------------------------------------------------------------------------------ cleaning
__device__ __forceinline__ bool cc_removed(const Ws& ws, int r, int v, int min_area, unsigned keep) {
  const int a = ws.area[r];
  if (a < min_area) return true;
  return ((keep >> v) & 1u) && cc_key(a, ws.rid[r]) != ws.best[v];
}

__global__ __launch_bounds__(256) void cc_clean_init_kernel(int32_t* __restrict__ wsp, int32_t* __restrict__ kept, int32_t* __restrict__ new_cls,
                                                            int H, int W, int cap) {
  const Ws ws = ws_split(wsp, H, W);
  const long total = (long)H * W, stride = (long)gridDim.x * 256;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += stride)
    if (ws.parent[p] == (int)p) {
      int4* v = (int4*)(ws.votes + 8 * (size_t)p);
      v[0] = make_int4(0, 0, 0, 0);
      v[1] = make_int4(0, 0, 0, 0);
    }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) { kept[i] = 0; new_cls[i] = 0; }
}

__global__ __launch_bounds__(256) void cc_vote_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ wsp, int H, int W, int min_area,
                                                      unsigned keep) {
  const Ws ws = ws_split(wsp, H, W);
  const long total = (long)H * W;
  for (long pl = (long)blockIdx.x * 256 + threadIdx.x; pl < total; pl += (long)gridDim.x * 256) {
    const int p = (int)pl, r = ws.parent[p];
    if (r < 0 || !cc_removed(ws, r, mask[p], min_area, keep)) continue;
    const int y = p / W, x = p - y * W;
    auto vote = [&](bool inside, int q) {
      if (!inside) return;
      const int rq = ws.parent[q], vq = mask[q];
      if (rq == r) return;
      const bool stands = rq < 0 ? vq < NC : !cc_removed(ws, rq, vq, min_area, keep);
      if (stands) atomicAdd(ws.votes + 8 * (size_t)r + vq, 1);
    };
    vote(y > 0, p - W);
    vote(x > 0, p - 1);
    vote(x + 1 < W, p + 1);
    vote(y + 1 < H, p + W);
  }
}

__global__ __launch_bounds__(256) void cc_apply_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int32_t* __restrict__ wsp,
                                                       int32_t* __restrict__ kept, int32_t* __restrict__ new_cls, int H, int W, int min_area,
                                                       unsigned keep, int cap) {
  const Ws ws = ws_split(wsp, H, W);
  const long total = (long)H * W;
  for (long pl = (long)blockIdx.x * 256 + threadIdx.x; pl < total; pl += (long)gridDim.x * 256) {
    const int p = (int)pl, r = ws.parent[p];
    const int v = mask[p];
    int o = v;
    bool gone = false;
    if (r >= 0 && cc_removed(ws, r, v, min_area, keep)) {
      gone = true;
      const int4* vt = (const int4*)(ws.votes + 8 * (size_t)r);
      const int4 a = vt[0], b = vt[1];
      const int c[NC] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      int bestv = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (c[k] > bestv) { bestv = c[k]; o = k; }                 // strict: the lowest class on a tie, v with no votes
    }
    out[p] = (uint8_t)o;
    if (r == p) {
      const int id = ws.rid[p];
      if (id <= cap) { kept[id - 1] = gone ? 0 : 1; new_cls[id - 1] = o; }
    }
  }
}

int flat_grid(long items) {
  long g = (items + 255) / 256;
  const long cap = 8L * segk_num_cus();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

static int cc_check_shape(const char* what, int H, int W, int cap) {
  SEGK_REQUIRE(H >= 1 && W >= 1, "%s: bad shape %d x %d", what, H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "%s: %d x %d pixels, at most 2^28", what, H, W);
  SEGK_REQUIRE(cap >= 1 && cap <= (1 << 24), "%s: max_components=%d (1..2^24)", what, cap);
  return 0;
}

extern "C" int segk_cc_label(const uint8_t* mask, int32_t* labels, int32_t* num, int32_t* cls, int32_t* area, int32_t* box,
                             int32_t* first, int32_t* ws, int H, int W, int connectivity, int class_mask, int max_components,
                             segk_stream_t s) {
  SEGK_REQUIRE(mask && labels && num && cls && area && box && first && ws, "cc_label: NULL pointer");
  if (int rc = cc_check_shape("cc_label", H, W, max_components)) return rc;
  SEGK_REQUIRE(connectivity == 4 || connectivity == 8, "cc_label: connectivity %d (4 or 8)", connectivity);
  SEGK_REQUIRE(class_mask >= 0 && class_mask < (1 << SEGK_MAX_CLASSES), "cc_label: class_mask %d (8 bits)", class_mask);
  SEGK_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)box & 15) == 0, "cc_label: ws and box must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const int conn8 = connectivity == 8, cap = max_components;
  const Ws w = ws_split(ws, H, W);
  const dim3 tiles((W + TS - 1) / TS, (H + TH - 1) / TH), strips((W + 63) / 64, (H + 4 * RW - 1) / (4 * RW));
  hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, st, mask, ws, num, cls, area, box, first, H, W, conn8, (unsigned)class_mask, cap);
  SEGK_CHECK_LAUNCH("cc_label (tiles)");
  const int nbr = (H - 1) / TH, nbc = (W - 1) / TS;
  const long border = (long)nbr * W + (long)nbc * (conn8 ? 2 : 1) * H;
  if (border > 0)
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, st, mask, w.parent, H, W, conn8, nbr, nbc);
  hipLaunchKernelGGL(cc_flatten_kernel, strips, dim3(256), 0, st, w.parent, w.area, w.rowcnt, H, W);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(256), 0, st, w.rowcnt, w.rowbase, num, H);
  hipLaunchKernelGGL(cc_rank_kernel, dim3((H + 3) / 4), dim3(256), 0, st, mask, ws, cls, area, box, first, H, W, cap);
  hipLaunchKernelGGL(cc_ids_kernel, strips, dim3(256), 0, st, w.parent, w.rid, labels, box, H, W, cap);
  SEGK_CHECK_LAUNCH("cc_label");
  return 0;
}

extern "C" int segk_cc_clean(const uint8_t* mask, uint8_t* out, int32_t* ws, int32_t* kept, int32_t* new_cls, int H, int W,
                             int min_area, int keep_mask, int max_components, segk_stream_t s) {
  SEGK_REQUIRE(mask && out && ws && kept && new_cls, "cc_clean: NULL pointer");
  if (int rc = cc_check_shape("cc_clean", H, W, max_components)) return rc;
  SEGK_REQUIRE(min_area >= 0, "cc_clean: min_area %d is negative", min_area);
  SEGK_REQUIRE(keep_mask >= 0 && keep_mask < (1 << SEGK_MAX_CLASSES), "cc_clean: keep_mask %d (8 bits)", keep_mask);
  SEGK_REQUIRE(((uintptr_t)ws & 15) == 0, "cc_clean: ws must be 16-byte aligned");
  SEGK_REQUIRE(mask != out, "cc_clean: the mask is read while the output is written: not in place");
  hipStream_t st = (hipStream_t)s;
  const int g = flat_grid((long)H * W);
  hipLaunchKernelGGL(cc_clean_init_kernel, dim3(g), dim3(256), 0, st, ws, kept, new_cls, H, W, max_components);
  SEGK_CHECK_LAUNCH("cc_clean (init)");
  if (min_area > 1 || keep_mask)                                   // otherwise nothing can be removed: no votes
    hipLaunchKernelGGL(cc_vote_kernel, dim3(g), dim3(256), 0, st, mask, ws, H, W, min_area, (unsigned)keep_mask);
  hipLaunchKernelGGL(cc_apply_kernel, dim3(g), dim3(256), 0, st, mask, out, ws, kept, new_cls, H, W, min_area, (unsigned)keep_mask,
                     max_components);
  SEGK_CHECK_LAUNCH("cc_clean");
  return 0;
}
