// Object-level evaluation on the device: the overlap (contingency) table of two segmentations, the
// unique IoU > 0.5 matching of their segments and the per-class Panoptic Quality statistics.  The reference holds no code for
// this; the arithmetic is this project's definition, every value is an integer and the result is unique, so the device equals
// the restatement of tests/panoptic_reference.py bit for bit whatever the arrival order of the atomics.  No float anywhere.
//
// The host knows no count: grids are sized from H, W and the capacities, a kernel reads the counts it needs from device
// memory and grid-strides over them.  Every loop is bounded by an argument (the probe loop by the slot count), no workgroup
// waits for another, order between the launches is stream order.  Slot positions of the hash table depend on arrival order;
// no output depends on them: a pair's row is the rank of its FIRST pixel among the first pixels of all pairs.
//
//  segk_pq_pairs
//   pq_init_kernel     table keys empty, counts 0, first pixels +inf, the leader bitmap 0, the overflow flag 0
//   pq_insert_kernel   one workgroup per 2048 pixels: segment pair of every pixel, equal keys of consecutive pixels collapsed
//                      by scan.hpp's run_length, the runs collapsed in an LDS table of 256 slots of its own (64-bit keys, two
//                      payloads; a key that finds its slot taken goes to the global table directly), then ONE global insert
//                      per LDS slot: atomicCAS on the 64-bit key, integer atomicAdd of the count, atomicMin of the first pixel
//   pq_mark_kernel     one thread per slot: bit `first pixel` of the leader bitmap
//   pq_words_kernel<false>  leaders per chunk of 1024 bitmap words (block_scan)
//   pq_scan_kernel     ONE workgroup: wg_scan of the chunk counts, P; decides overflow and writes totals
//   pq_words_kernel<true>   the same chunk again with its base: leaders before every bitmap word
//   pq_emit_kernel     one thread per slot: row = leaders before its first pixel -> pair_g / pair_p / pair_n
//  segk_pq_match
//   pq_zero_kernel     the per-segment rows in use, totals[1..3]
//   pq_area_kernel     one thread per pair: area_g, area_p, void_p, through LDS cells for the stuff rows and scan.hpp's
//                      AddTable for the others (a segment that meets thousands of others is one address)
//   pq_test_kernel     one thread per pair: 2 n > union -> the match records (a unique writer per row: DESIGN.md 3.19)
//   pq_classify_kernel one thread per segment row: TP / FP / FN and the IoU sums into an LDS copy of the 8 x 16 cells, then one
//                      64-bit integer atomic per non-zero cell
// block_scan, wg_scan, run_length, AddTable and the load / index helpers are the object kernels' shared ones: scan.hpp
// (DESIGN.md 3.20).
#include "scan.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int BP = SEGK_PQ_BLOCK_PIXELS;    // pixels a workgroup inserts
constexpr int LT = SEGK_PQ_LDS_SLOTS;       // slots of its LDS table, and of the area pass's: one per thread
constexpr int CH = SEGK_PQ_CHUNK;           // bitmap words a workgroup counts and scans
constexpr int NC = SEGK_MAX_CLASSES;
constexpr int NS = SEGK_PQ_STAT_COLS;
constexpr u64 EMPTY = ~0ull;
constexpr int NOPIX = 0x7fffffff;
static_assert(BP == 8 * 256 && LT == 256 && CH == 4 * 256, "8 pixels, one LDS slot and 4 bitmap words per thread of a workgroup");
static_assert(NC * NS == 128, "the statistics are 128 cells: one per thread of half a workgroup");

// workspace layout in 32-bit words (SEGK_PQ_WS_INTS of the header).  head[0]: the overflow flag
struct Ws {
  int* head;
  u64* key;
  int *cnt, *first;
  unsigned* bits;
  int *wbase, *part;
  long slots, words, chunks;
};
__host__ __device__ inline Ws ws_split(int32_t* ws, long hw, long max_pairs) {
  Ws w;
  w.slots = SEGK_PQ_SLOTS(max_pairs);
  w.words = (hw + 31) / 32;
  w.chunks = (w.words + CH - 1) / CH;
  w.head = ws;
  w.key = (u64*)(ws + 16);
  w.cnt = ws + 16 + 2 * w.slots;
  w.first = w.cnt + w.slots;
  w.bits = (unsigned*)(w.first + w.slots);
  w.wbase = (int*)w.bits + r4(w.words);
  w.part = w.wbase + r4(w.words);
  return w;
}

__device__ __forceinline__ unsigned pq_hash(u64 k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return (unsigned)k;
}

// segment of a pixel with label L and value v (DESIGN.md 3.19 "segments"); a label outside 1..num counts as 0
__device__ __forceinline__ int seg_of(int L, unsigned v, int num, unsigned stuff, int cap) {
  if (L >= 1 && L <= num) return L;
  return (v < (unsigned)NC && ((stuff >> v) & 1u)) ? cap + 1 + (int)v : 0;
}

// ------------------------------------------------------------------------------------------------ pair table
__global__ __launch_bounds__(256) void pq_init_kernel(int32_t* __restrict__ wsp, long hw, long max_pairs) {
  const Ws w = ws_split(wsp, hw, max_pairs);
  for (long i = thread_of(); i < w.slots; i += stride_of()) { w.key[i] = EMPTY; w.cnt[i] = 0; w.first[i] = NOPIX; }
  for (long i = thread_of(); i < w.words; i += stride_of()) w.bits[i] = 0u;
  if (thread_of() == 0) w.head[0] = 0;
}

// the key's slot gets n more pixels and the first pixel pix.  Linear probing from the hashed slot, at most `slots` steps; a
// full table raises the flag, and once it is up nobody probes any more (the call's result is "overflow" whatever follows).
__device__ __forceinline__ void glb_insert(const Ws& w, u64 key, int n, int pix) {
  if (dev_load(w.head) != 0) return;
  long s = (long)(((u64)pq_hash(key) * (u64)w.slots) >> 32);
  for (long i = 0; i < w.slots; ++i) {
    u64 old = dev_load64(w.key + s);
    if (old == EMPTY) old = atomicCAS(w.key + s, EMPTY, key);
    if (old == EMPTY || old == key) {
      atomicAdd(w.cnt + s, n);
      if (dev_load(w.first + s) > pix) atomicMin(w.first + s, pix);      // the word only falls: an atomic that cannot change it is skipped
      return;
    }
    if (++s == w.slots) s = 0;
  }
  atomicOr(w.head, 1);
}

__global__ __launch_bounds__(256) void pq_insert_kernel(const uint8_t* __restrict__ mp, const int32_t* __restrict__ lp,
                                                        const int32_t* __restrict__ nump, const uint8_t* __restrict__ mg,
                                                        const int32_t* __restrict__ lg, const int32_t* __restrict__ numg,
                                                        int32_t* __restrict__ wsp, long hw, unsigned stuff, int ignore, int cap,
                                                        long max_pairs) {
  __shared__ u64 t_key[LT];
  __shared__ int t_cnt[LT], t_first[LT];
  const Ws w = ws_split(wsp, hw, max_pairs);
  const int tid = threadIdx.x, lane = tid & 63;
  t_key[tid] = EMPTY; t_cnt[tid] = 0; t_first[tid] = NOPIX;
  const int np = *nump, ng = *numg;
  __syncthreads();
  const long p0 = (long)blockIdx.x * BP + tid;
  u64 key[BP / 256];
#pragma unroll
  for (int k = 0; k < BP / 256; ++k) {                            // all loads of the workgroup are in flight together
    const long p = p0 + k * 256;
    key[k] = EMPTY;
    if (p < hw) {
      const unsigned vg = mg[p], vp = mp[p];
      const int sp = seg_of(lp[p], vp, np, stuff, cap);
      const int sg = (vg >= (unsigned)NC || (int)vg == ignore) ? -1 : seg_of(lg[p], vg, ng, stuff, cap);
      key[k] = ((u64)(unsigned)(sg + 1) << 32) | (u64)(unsigned)sp;
    }
  }
#pragma unroll
  for (int k = 0; k < BP / 256; ++k) {
    // run heads of the wave's 64 consecutive pixels: a head adds its run's length once (its own pixel is the run's first)
    const int len = run_length(key[k], lane);
    if (len && key[k] != EMPTY) {
      const int p = (int)(p0 + k * 256);
      const int h = (int)(pq_hash(key[k]) & (unsigned)(LT - 1));
      const u64 old = atomicCAS(&t_key[h], EMPTY, key[k]);
      if (old == EMPTY || old == key[k]) {
        atomicAdd(&t_cnt[h], len);
        atomicMin(&t_first[h], p);
      } else {
        glb_insert(w, key[k], len, p);
      }
    }
  }
  __syncthreads();
  if (t_key[tid] != EMPTY) glb_insert(w, t_key[tid], t_cnt[tid], t_first[tid]);
}

__global__ __launch_bounds__(256) void pq_mark_kernel(int32_t* __restrict__ wsp, long hw, long max_pairs) {
  const Ws w = ws_split(wsp, hw, max_pairs);
  for (long s = thread_of(); s < w.slots; s += stride_of())
    if (w.key[s] != EMPTY) {
      const int f = w.first[s];
      if ((long)f < hw) atomicOr(w.bits + (f >> 5), 1u << (f & 31));
    }
}

// chunk blockIdx.x of the bitmap: SCATTER false -> its leader count; true -> the leaders before each of its words
template <bool SCATTER>
__global__ __launch_bounds__(256) void pq_words_kernel(int32_t* __restrict__ wsp, const int32_t* __restrict__ totals, long hw, long max_pairs) {
  __shared__ int s_w[4];
  const Ws w = ws_split(wsp, hw, max_pairs);
  if (SCATTER && totals[0] < 0) return;         // the same word for every workgroup: all of them leave here
  const long i = (long)blockIdx.x * CH + 4 * threadIdx.x;
  int c[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c[k] = i + k < w.words ? (int)__popc(w.bits[i + k]) : 0;
    sum += c[k];
  }
  int total;
  int ex = block_scan<4>(sum, s_w, total);
  if (!SCATTER) {
    if (threadIdx.x == 0) w.part[blockIdx.x] = total;
    return;
  }
  ex += w.part[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (i + k < w.words) w.wbase[i + k] = ex;
    ex += c[k];
  }
}

// ONE workgroup: part[0..chunks) -> its exclusive prefix sums, in place; P; the overflow decision; totals
__global__ __launch_bounds__(256) void pq_scan_kernel(int32_t* __restrict__ wsp, int32_t* __restrict__ totals, const int32_t* __restrict__ nump,
                                                      const int32_t* __restrict__ numg, long hw, long max_pairs, int cap) {
  const Ws w = ws_split(wsp, hw, max_pairs);
  const int total = wg_scan(w.part, w.part, w.chunks);
  if (threadIdx.x == 0) {
    const bool over = w.head[0] != 0 || (long)total > max_pairs || *nump > cap || *numg > cap || *nump < 0 || *numg < 0;
    totals[0] = over ? -1 : total;
    if (over) { totals[1] = -1; totals[2] = -1; totals[3] = -1; }
  }
}

__global__ __launch_bounds__(256) void pq_emit_kernel(int32_t* __restrict__ wsp, const int32_t* __restrict__ totals, int32_t* __restrict__ pair_g,
                                                      int32_t* __restrict__ pair_p, int32_t* __restrict__ pair_n, long hw, long max_pairs) {
  const Ws w = ws_split(wsp, hw, max_pairs);
  const int P = totals[0];
  if (P < 0) return;
  for (long s = thread_of(); s < w.slots; s += stride_of()) {
    const u64 key = w.key[s];
    if (key == EMPTY) continue;
    const int f = w.first[s];
    if ((long)f >= hw) continue;
    const int r = w.wbase[f >> 5] + (int)__popc(w.bits[f >> 5] & ((1u << (f & 31)) - 1u));
    if (r < P && (long)r < max_pairs) {
      pair_g[r] = (int)(unsigned)(key >> 32) - 1;
      pair_p[r] = (int)(unsigned)key;
      pair_n[r] = w.cnt[s];
    }
  }
}

// ------------------------------------------------------------------------------------------------ matching
// the rows in use: things 0..num-1, stuff cap..cap+7 (rows num..cap-1 are never read or written)
__device__ __forceinline__ bool row_ok(int r, int num, int cap) { return (r >= 0 && r < num && r < cap) || (r >= cap && r < cap + NC); }
__device__ __forceinline__ int row_class(const int32_t* __restrict__ cls, int r, int cap) { return r < cap ? cls[r] : r - cap; }

struct Seg {               // the per-segment arrays of one call
  int32_t *area_g, *match_g, *inter_g, *union_g, *area_p, *void_p, *match_p;
};

__global__ __launch_bounds__(256) void pq_zero_kernel(Seg a, int32_t* __restrict__ totals, const int32_t* __restrict__ nump,
                                                      const int32_t* __restrict__ numg, int cap) {
  if (totals[0] < 0) return;
  const int np = *nump, ng = *numg;
  for (long i = thread_of(); i < cap + NC; i += stride_of()) {
    if (row_ok((int)i, ng, cap)) { a.area_g[i] = 0; a.match_g[i] = 0; a.inter_g[i] = 0; a.union_g[i] = 0; }
    if (row_ok((int)i, np, cap)) { a.area_p[i] = 0; a.void_p[i] = 0; a.match_p[i] = 0; }
  }
  if (thread_of() == 0) { totals[1] = 0; totals[2] = 0; totals[3] = 0; }
}

// A segment that meets many others (a stuff class, a background component) is one address for thousands of pairs: what a
// workgroup adds to one row leaves as ONE global atomic per word.  The eight stuff rows have cells of their own; the other rows
// share scan.hpp's AddTable under the key 3 * row + t.  t: 0 area_g, 1 area_p, 2 void_p.
__device__ __forceinline__ void area_add(int (*s_stuff)[NC], AddTable<LT>& tab, int32_t* __restrict__ dst, int t, int r, int n, int cap) {
  if (r >= cap) atomicAdd(&s_stuff[t][r - cap], n);
  else tab.add(3 * r + t, n, dst + r);
}

__global__ __launch_bounds__(256) void pq_area_kernel(const int32_t* __restrict__ pair_g, const int32_t* __restrict__ pair_p,
                                                      const int32_t* __restrict__ pair_n, Seg a, const int32_t* __restrict__ totals,
                                                      const int32_t* __restrict__ nump, const int32_t* __restrict__ numg, int cap,
                                                      int max_pairs) {
  __shared__ int s_stuff[3][NC];
  __shared__ AddTable<LT> tab;
  int P = totals[0];
  if (P < 0) return;
  P = P < max_pairs ? P : max_pairs;
  tab.clear();
  if (threadIdx.x < 3 * NC) s_stuff[threadIdx.x / NC][threadIdx.x % NC] = 0;
  __syncthreads();
  const int np = *nump, ng = *numg;
  int32_t* const dst[3] = {a.area_g, a.area_p, a.void_p};
  for (long i = thread_of(); i < P; i += stride_of()) {
    const int g = pair_g[i], p = pair_p[i], n = pair_n[i];
    if (row_ok(g - 1, ng, cap)) area_add(s_stuff, tab, dst[0], 0, g - 1, n, cap);
    if (row_ok(p - 1, np, cap)) {
      area_add(s_stuff, tab, dst[1], 1, p - 1, n, cap);
      if (g == -1) area_add(s_stuff, tab, dst[2], 2, p - 1, n, cap);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * NC) {
    const int v = s_stuff[threadIdx.x / NC][threadIdx.x % NC];
    if (v) atomicAdd(dst[threadIdx.x / NC] + cap + threadIdx.x % NC, v);
  }
  tab.flush([&](int key) { return dst[key % 3] + key / 3; });
}

__global__ __launch_bounds__(256) void pq_test_kernel(const int32_t* __restrict__ pair_g, const int32_t* __restrict__ pair_p,
                                                      const int32_t* __restrict__ pair_n, Seg a, const int32_t* __restrict__ totals,
                                                      const int32_t* __restrict__ clsp, const int32_t* __restrict__ nump,
                                                      const int32_t* __restrict__ clsg, const int32_t* __restrict__ numg, int cap,
                                                      int max_pairs) {
  int P = totals[0];
  if (P < 0) return;
  P = P < max_pairs ? P : max_pairs;
  const int np = *nump, ng = *numg;
  for (long i = thread_of(); i < P; i += stride_of()) {
    const int g = pair_g[i], p = pair_p[i], n = pair_n[i];
    if (!row_ok(g - 1, ng, cap) || !row_ok(p - 1, np, cap)) continue;
    const int cg = row_class(clsg, g - 1, cap), cp = row_class(clsp, p - 1, cap);
    if (cg != cp || (unsigned)cg >= (unsigned)NC) continue;
    const long uni = (long)a.area_g[g - 1] + a.area_p[p - 1] - n - a.void_p[p - 1];
    if (2L * n > uni) {
      a.match_g[g - 1] = p; a.inter_g[g - 1] = n; a.union_g[g - 1] = (int)uni;
      a.match_p[p - 1] = g;
    }
  }
}

// item i < cap + 8: target row i; else predicted row i - (cap + 8)
__global__ __launch_bounds__(256) void pq_classify_kernel(Seg a, int32_t* __restrict__ totals, const int32_t* __restrict__ clsp,
                                                          const int32_t* __restrict__ nump, const int32_t* __restrict__ clsg,
                                                          const int32_t* __restrict__ numg, u64* __restrict__ stats, int cap) {
  __shared__ u64 s_cell[NC * NS];
  __shared__ int s_tot[3];
  if (totals[0] < 0) return;
  if (threadIdx.x < NC * NS) s_cell[threadIdx.x] = 0;
  if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
  __syncthreads();
  const int np = *nump, ng = *numg, rows = cap + NC;
  for (long i = thread_of(); i < 2L * rows; i += stride_of()) {
    const bool pred = i >= rows;
    const int r = (int)(pred ? i - rows : i);
    if (!row_ok(r, pred ? np : ng, cap)) continue;
    const int c = row_class(pred ? clsp : clsg, r, cap);
    if ((unsigned)c >= (unsigned)NC) continue;
    u64* cell = s_cell + c * NS;
    if (pred) {
      const int ar = a.area_p[r];
      if (ar <= 0) continue;
      atomicAdd(cell + 15, 1ull);
      atomicAdd(&s_tot[1], 1);
      if (a.match_p[r] == 0 && !(2L * a.void_p[r] > (long)ar)) atomicAdd(cell + 1, 1ull);
    } else {
      if (a.area_g[r] <= 0) continue;
      atomicAdd(cell + 14, 1ull);
      atomicAdd(&s_tot[0], 1);
      if (a.match_g[r] == 0) {
        atomicAdd(cell + 2, 1ull);
        continue;
      }
      const u64 n = (u64)a.inter_g[r], uni = (u64)a.union_g[r];
      atomicAdd(cell + 0, 1ull);
      atomicAdd(&s_tot[2], 1);
      atomicAdd(cell + 3, (n << 32) / uni);
#pragma unroll
      for (int k = 0; k < 10; ++k)
        if (20ull * n >= (u64)(10 + k) * uni) atomicAdd(cell + 4 + k, 1ull);
    }
  }
  __syncthreads();
  if (threadIdx.x < NC * NS && s_cell[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_cell[threadIdx.x]);
  if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(totals + 1 + threadIdx.x, s_tot[threadIdx.x]);
}

int flat_grid(long items) {
  long g = (items + 255) / 256;
  const long cap = 8L * segk_num_cus();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace

static int pq_check_caps(const char* what, int max_components, int max_pairs) {
  SEGK_REQUIRE(max_components >= 1 && max_components <= (1 << 24), "%s: max_components=%d (1..2^24)", what, max_components);
  SEGK_REQUIRE(max_pairs >= 1 && max_pairs <= SEGK_PQ_MAX_PAIRS, "%s: max_pairs=%d (1..2^28)", what, max_pairs);
  return 0;
}

extern "C" int segk_pq_pairs(const uint8_t* pred, const int32_t* pred_labels, const int32_t* pred_num, const uint8_t* target,
                             const int32_t* target_labels, const int32_t* target_num, int32_t* pair_g, int32_t* pair_p,
                             int32_t* pair_n, int32_t* totals, int32_t* ws, int H, int W, int stuff_mask, int ignore_index,
                             int max_components, int max_pairs, segk_stream_t s) {
  SEGK_REQUIRE(pred && pred_labels && pred_num && target && target_labels && target_num && pair_g && pair_p && pair_n && totals && ws,
               "pq_pairs: NULL pointer");
  SEGK_REQUIRE(H >= 1 && W >= 1, "pq_pairs: bad shape %d x %d", H, W);
  SEGK_REQUIRE((long)H * W <= SEGK_CC_MAX_PIXELS, "pq_pairs: %d x %d pixels, at most 2^28", H, W);
  if (int rc = pq_check_caps("pq_pairs", max_components, max_pairs)) return rc;
  SEGK_REQUIRE(stuff_mask >= 0 && stuff_mask < (1 << SEGK_MAX_CLASSES), "pq_pairs: stuff_mask %d (8 bits)", stuff_mask);
  SEGK_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "pq_pairs: ignore_index %d (-1: none, or 0..255)", ignore_index);
  SEGK_REQUIRE(((uintptr_t)ws & 15) == 0, "pq_pairs: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const long hw = (long)H * W;
  const Ws w = ws_split(ws, hw, max_pairs);
  const long init = w.slots > w.words ? w.slots : w.words;
  hipLaunchKernelGGL(pq_init_kernel, dim3(flat_grid(init)), dim3(256), 0, st, ws, hw, (long)max_pairs);
  SEGK_CHECK_LAUNCH("pq_pairs (init)");
  hipLaunchKernelGGL(pq_insert_kernel, dim3((unsigned)((hw + BP - 1) / BP)), dim3(256), 0, st, pred, pred_labels, pred_num, target,
                     target_labels, target_num, ws, hw, (unsigned)stuff_mask, ignore_index, max_components, (long)max_pairs);
  hipLaunchKernelGGL(pq_mark_kernel, dim3(flat_grid(w.slots)), dim3(256), 0, st, ws, hw, (long)max_pairs);
  hipLaunchKernelGGL(pq_words_kernel<false>, dim3((unsigned)w.chunks), dim3(256), 0, st, ws, totals, hw, (long)max_pairs);
  hipLaunchKernelGGL(pq_scan_kernel, dim3(1), dim3(256), 0, st, ws, totals, pred_num, target_num, hw, (long)max_pairs, max_components);
  hipLaunchKernelGGL(pq_words_kernel<true>, dim3((unsigned)w.chunks), dim3(256), 0, st, ws, totals, hw, (long)max_pairs);
  hipLaunchKernelGGL(pq_emit_kernel, dim3(flat_grid(w.slots)), dim3(256), 0, st, ws, totals, pair_g, pair_p, pair_n, hw, (long)max_pairs);
  SEGK_CHECK_LAUNCH("pq_pairs");
  return 0;
}

extern "C" int segk_pq_match(const int32_t* pair_g, const int32_t* pair_p, const int32_t* pair_n, int32_t* totals,
                             const int32_t* pred_cls, const int32_t* pred_num, const int32_t* target_cls, const int32_t* target_num,
                             int32_t* area_g, int32_t* match_g, int32_t* inter_g, int32_t* union_g, int32_t* area_p, int32_t* void_p,
                             int32_t* match_p, int64_t* stats, int max_components, int max_pairs, segk_stream_t s) {
  SEGK_REQUIRE(pair_g && pair_p && pair_n && totals && pred_cls && pred_num && target_cls && target_num && area_g && match_g && inter_g &&
                   union_g && area_p && void_p && match_p && stats,
               "pq_match: NULL pointer");
  if (int rc = pq_check_caps("pq_match", max_components, max_pairs)) return rc;
  SEGK_REQUIRE(((uintptr_t)stats & 7) == 0, "pq_match: stats must be 8-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const Seg a = {area_g, match_g, inter_g, union_g, area_p, void_p, match_p};
  const int cap = max_components, gp = flat_grid(max_pairs);
  hipLaunchKernelGGL(pq_zero_kernel, dim3(flat_grid(cap + NC)), dim3(256), 0, st, a, totals, pred_num, target_num, cap);
  SEGK_CHECK_LAUNCH("pq_match (zero)");
  hipLaunchKernelGGL(pq_area_kernel, dim3(gp), dim3(256), 0, st, pair_g, pair_p, pair_n, a, totals, pred_num, target_num, cap, max_pairs);
  hipLaunchKernelGGL(pq_test_kernel, dim3(gp), dim3(256), 0, st, pair_g, pair_p, pair_n, a, totals, pred_cls, pred_num, target_cls,
                     target_num, cap, max_pairs);
  hipLaunchKernelGGL(pq_classify_kernel, dim3(flat_grid(2L * (cap + NC))), dim3(256), 0, st, a, totals, pred_cls, pred_num, target_cls,
                     target_num, (u64*)stats, cap);
  SEGK_CHECK_LAUNCH("pq_match");
  return 0;
}
