// Mixed-sample augmentation on the device: CutMix, ClassMix and object copy-paste are ONE write rule
// driven by a paste bit m(y, x) per output pixel.  The reference only puts two images side by side (utils/augmentation.ipynb
// cell 17); the arithmetic here is this project's definition.  Every output value is a copy of one input value and m is defined
// in integers, so the device equals the restatement of tests/mix_reference.py bit for bit.
//
//  segk_mix_select  mix_bytes_kernel    the partner's int64 labels as bytes (outside 0..255 -> 255) for segk_cc_label
//                   mix_select_kernel   one workgroup of 1024 per sample, CLASS / OBJECT samples only
//                     CLASS   stride over the partner's labels, presence flags in LDS; thread v < 256 forms key(v) and counts the
//                             candidates with a smaller key (its rank); the k lowest ranks are selected -> 256 bytes
//                     OBJECT  count the candidate ids of the partner's num / cls / area rows, then k <= 32 rounds of a workgroup
//                             minimum over the keys above the last one; a last pass writes every byte of the table once
//                   no atomics on global memory, no workgroup waits for another, loops bounded by H W and max_components
//  segk_mix_apply   mix_apply_kernel<E, NHWC, L>: one workgroup per tile of 16 rows x 64 columns and sample
//                     stage    m of the tile and a one-pixel halo in LDS: the deciding label or id of a thread's five cells is
//                              read at the source pixels with all loads in flight, the class table comes from LDS
//                     write    a thread takes four pixels of a row: the bits of m and of the seam, then per plane four values
//                              from the partner or the sample itself.  A group whose four bits agree is one vector load when
//                              the source allows it (the partner side is misaligned by dx and reversed under flip: scalar loads
//                              there); the four values leave as one vector store when the output address allows it
//                     count    popcount of m, wave sum, LDS, one integer add to pasted[b] per workgroup
//                   every output element is written once, nothing else is written
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

typedef unsigned long long u64;
constexpr int TH = SEGK_MIX_TILE_H, TW = SEGK_MIX_TILE_W;
constexpr int SEL_THREADS = 1024;
static_assert(TH == 16 && TW == 64, "256 threads: thread t takes row t >> 4 and the columns 4 (t & 15) .. + 3");
static_assert(SEGK_MIX_MAX_COMPONENTS < (1 << 24), "an id fits the low 24 bits of a key");
static_assert(sizeof(segk_mix_desc) == 64, "segk_mix_desc is 64 bytes");

// a label as a byte, -1 when it lies outside 0..255
__device__ __forceinline__ int label_byte(uint8_t v) { return v; }
__device__ __forceinline__ int label_byte(long long v) { return v < 0 || v > 255 ? -1 : (int)v; }

__device__ __forceinline__ u64 key_of(u64 seed, unsigned i) { return (splitmix(seed, i) & ~0xFFFFFFull) | i; }

// ------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(256) void mix_bytes_kernel(const segk_mix_desc* __restrict__ descs, int n, const long long* __restrict__ y,
                                                        long HW, int n_slots, uint8_t* __restrict__ bytes) {
  const segk_mix_desc& d = descs[blockIdx.y];
  if (d.mode != SEGK_MIX_OBJECT) return;
  const long long* lab = y + (size_t)clampi(d.partner, 0, n - 1) * HW;
  uint8_t* dst = bytes + (size_t)clampi(d.slot, 0, n_slots - 1) * HW;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long)gridDim.x * 256) {
    const int v = label_byte(lab[i]);
    dst[i] = (uint8_t)(v < 0 ? 255 : v);
  }
}

template <typename L>
__global__ __launch_bounds__(SEL_THREADS) void mix_select_kernel(const segk_mix_desc* __restrict__ descs, int n, const L* __restrict__ y,
                                                                 long HW, const uint8_t* __restrict__ exclude, int n_classes,
                                                                 const int32_t* __restrict__ cc_rows, int n_slots, int things, int min_area,
                                                                 int max_area, int max_objects, int cap, uint8_t* __restrict__ select,
                                                                 int stride) {
  __shared__ unsigned s_present[256];
  __shared__ u64 s_key[256];
  __shared__ u64 s_wave[SEL_THREADS / 64];
  __shared__ int s_chosen[SEGK_MIX_MAX_OBJECTS];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const segk_mix_desc& d = descs[blockIdx.x];
  const int mode = d.mode;                                 // workgroup-uniform
  const u64 seed = d.seed;
  uint8_t* sel = select + (size_t)blockIdx.x * stride;
  if (mode == SEGK_MIX_CLASS) {
    const L* lab = y + (size_t)clampi(d.partner, 0, n - 1) * HW;
    if (tid < 256) s_present[tid] = 0u;
    __syncthreads();
    for (long i0 = tid; i0 < HW; i0 += SEL_THREADS * 8) {  // eight loads in flight per thread
      L v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long i = i0 + (long)u * SEL_THREADS;
        v[u] = lab[i < HW ? i : HW - 1];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = label_byte(v[u]);
        if (b >= 0) s_present[b] = 1u;                     // every writer stores the same word
      }
    }
    __syncthreads();
    const bool cand = tid < 256 && s_present[tid & 255] && !exclude[tid & 255];
    const u64 key = key_of(seed, (unsigned)tid);
    if (tid < 256) s_key[tid] = cand ? key : ~0ull;        // a candidate's low 24 bits are below 256: never all ones
    const int count = __syncthreads_count(cand);
    const int k = n_classes > 0 ? (count < n_classes ? count : n_classes) : (count + 1) / 2;
    if (tid < 256) {
      int rank = 0;
      for (int j = 0; j < 256; ++j) rank += s_key[j] < key;
      sel[tid] = (uint8_t)(cand && rank < k);
    }
    return;
  }
  if (mode != SEGK_MIX_OBJECT || n_slots < 1 || !cc_rows) return;
  const int32_t* row = cc_rows + (size_t)clampi(d.slot, 0, n_slots - 1) * SEGK_MIX_ROW_INTS(cap);
  const int K = row[0], rows = K < 0 ? 0 : K < cap ? K : cap;
  const int32_t* cls = row + 4;
  const int32_t* area = row + 4 + cap;
  auto candidate = [&](int i) {                            // of row i, the component id i + 1
    const int c = cls[i], a = area[i];
    return c >= 0 && c < SEGK_MAX_CLASSES && ((things >> c) & 1) && a >= min_area && a <= max_area;
  };
  if (tid == 0) s_n = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < rows; i += SEL_THREADS) mine += candidate(i);
  if (mine) atomicAdd(&s_n, mine);                         // LDS
  __syncthreads();
  const int count = s_n, k = count < max_objects ? count : max_objects;
  u64 last = 0;                                            // keys carry an id >= 1: none is zero
  for (int r = 0; r < k; ++r) {
    u64 best = ~0ull;
    for (int i = tid; i < rows; i += SEL_THREADS) {
      if (!candidate(i)) continue;
      const u64 key = key_of(seed, (unsigned)(i + 1));
      if (key > last && key < best) best = key;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const u64 other = __shfl_xor(best, o);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) s_wave[tid >> 6] = best;
    __syncthreads();
    best = s_wave[0];
#pragma unroll
    for (int w = 1; w < SEL_THREADS / 64; ++w) best = s_wave[w] < best ? s_wave[w] : best;
    last = best;                                           // the r-th smallest key, the same in every thread
    if (tid == 0) s_chosen[r] = (int)(best & 0xFFFFFFull) - 1;
    __syncthreads();                                       // s_wave is free again
  }
  for (int i = tid; i < cap; i += SEL_THREADS) {
    bool on = false;
    for (int r = 0; r < k; ++r) on |= s_chosen[r] == i;
    sel[i] = (uint8_t)on;
  }
}

// ------------------------------------------------------------------------------------------------ apply
// four values of T as one vector: 4, 8 or 16 bytes, and two 16-byte halves for 8-byte labels
template <typename T> struct Four {
  typedef T vec __attribute__((ext_vector_type(4)));
  static constexpr int ALIGN = sizeof(T) * 4 > 16 ? 16 : (int)sizeof(T) * 4;
  typedef vec avec __attribute__((aligned(ALIGN)));
};
template <typename T> __device__ __forceinline__ bool aligned4(const T* p) { return ((uintptr_t)p & (Four<T>::ALIGN - 1)) == 0; }
template <typename T> __device__ __forceinline__ void load4(const T* p, T (&v)[4]) {
  const typename Four<T>::vec q = *(const typename Four<T>::avec*)p;
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}
template <typename T> __device__ __forceinline__ void store4(T* p, const T (&v)[4]) {
  typename Four<T>::vec q;
  q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
  *(typename Four<T>::avec*)p = q;
}

// what one thread knows about its four pixels (y, x .. x + 3): npx of them are inside the image
struct Group {
  int npx, mbits, ys, xs0, step;       // pixel j reads the partner at (ys, xs0 + j step) where bit j of mbits is set
};

// four values of one plane: `own` points at the sample's (y, x), `part` at the partner's row ys
template <typename T>
__device__ __forceinline__ void gather4(const T* __restrict__ own, const T* __restrict__ part_row, const Group& g, T (&v)[4]) {
  const bool full = g.npx == 4;
  if (full && g.mbits == 0 && aligned4(own)) {
    load4(own, v);
  } else if (full && g.mbits == 15 && g.step == 1 && aligned4(part_row + g.xs0)) {
    load4(part_row + g.xs0, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (T)0;
      if (j < g.npx) v[j] = ((g.mbits >> j) & 1) ? part_row[g.xs0 + j * g.step] : own[j];
    }
  }
}
template <typename T>
__device__ __forceinline__ void scatter4(T* __restrict__ out, const Group& g, const T (&v)[4]) {
  if (g.npx == 4 && aligned4(out)) {
    store4(out, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < g.npx) out[j] = v[j];
  }
}

template <typename E, bool NHWC, typename L>
__global__ __launch_bounds__(256) void mix_apply_kernel(const segk_mix_desc* __restrict__ descs, int n, const E* __restrict__ X,
                                                        const L* __restrict__ Y, E* __restrict__ Xo, L* __restrict__ Yo,
                                                        int32_t* __restrict__ pasted, int C, int H, int W,
                                                        const uint8_t* __restrict__ select, int stride, const int32_t* __restrict__ ids,
                                                        int n_slots, int cap, int has_seam, long long seam, int tiles_x) {
  __shared__ uint8_t s_m[TH + 2][TW + 4];                  // cell (ly, lx) of the tile at [ly + 1][lx + 1]
  __shared__ uint8_t s_sel[256];                            // CLASS: the sample's select table
  __shared__ int s_cnt;
  const int tid = threadIdx.x, b = blockIdx.y;
  const segk_mix_desc& d = descs[b];
  int mode = d.mode;                                       // workgroup-uniform
  if (mode < SEGK_MIX_NONE || mode > SEGK_MIX_OBJECT || (mode == SEGK_MIX_OBJECT && (n_slots < 1 || !ids))) mode = SEGK_MIX_NONE;
  const int p = clampi(d.partner, 0, n - 1);
  const bool flip = d.flip != 0;
  const int dy = clampi(d.dy, -H, H), dx = clampi(d.dx, -W, W);      // a shift of a whole side already leaves nothing inside
  const size_t HW = (size_t)H * W;
  const L* __restrict__ own_lab = Y + (size_t)b * HW;
  const L* __restrict__ part_lab = Y + (size_t)p * HW;
  const uint8_t* __restrict__ sel = select + (size_t)b * stride;
  const int32_t* __restrict__ idmap = mode == SEGK_MIX_OBJECT ? ids + (size_t)clampi(d.slot, 0, n_slots - 1) * HW : nullptr;
  const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;
  if (tid == 0) s_cnt = 0;
  if (mode != SEGK_MIX_NONE) {
    // the deciding values of the thread's cells first, every load in flight together (clamped addresses, unconditional), then
    // the bits; the class table is read from LDS
    constexpr int CELLS = (TH + 2) * (TW + 2), TRIPS = (CELLS + 255) / 256;
    size_t q[TRIPS];
    int key[TRIPS];
    bool in[TRIPS];
#pragma unroll
    for (int u = 0; u < TRIPS; ++u) {
      const int e = tid + 256 * u, r = e / (TW + 2), c = e - r * (TW + 2);
      const int gy = ty0 + r - 1, gx = tx0 + c - 1;
      const int ys = gy - dy, xr = gx - dx, xs = flip ? W - 1 - xr : xr;
      in[u] = e < CELLS && gy >= 0 && gy < H && gx >= 0 && gx < W && ys >= 0 && ys < H && xs >= 0 && xs < W;
      q[u] = in[u] ? (size_t)ys * W + xs : 0;
      key[u] = 0;
    }
    if (mode == SEGK_MIX_CLASS) {
      const unsigned mine = sel[tid];
#pragma unroll
      for (int u = 0; u < TRIPS; ++u) key[u] = label_byte(part_lab[q[u]]);
      s_sel[tid] = (uint8_t)mine;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < TRIPS; ++u) key[u] = key[u] >= 0 && s_sel[key[u] & 255];
    } else if (mode == SEGK_MIX_OBJECT) {
#pragma unroll
      for (int u = 0; u < TRIPS; ++u) key[u] = idmap[q[u]];
      unsigned on[TRIPS];
#pragma unroll
      for (int u = 0; u < TRIPS; ++u) on[u] = sel[key[u] >= 1 && key[u] <= cap ? key[u] - 1 : 0];
#pragma unroll
      for (int u = 0; u < TRIPS; ++u) key[u] = key[u] >= 1 && key[u] <= cap && on[u];
    }
#pragma unroll
    for (int u = 0; u < TRIPS; ++u) {
      const int e = tid + 256 * u, r = e / (TW + 2), c = e - r * (TW + 2);
      const int gy = ty0 + r - 1, gx = tx0 + c - 1;
      const bool rule = mode == SEGK_MIX_BOX ? gy >= d.y0 && gy < d.y1 && gx >= d.x0 && gx < d.x1 : key[u] != 0;
      if (e < CELLS) s_m[r][c] = (uint8_t)(in[u] && rule);
    }
  }
  __syncthreads();
  const int ly = tid >> 4, lx = (tid & 15) * 4;
  const int gy = ty0 + ly, gx = tx0 + lx;
  int cnt = 0;
  if (gy < H && gx < W) {
    Group g;
    g.npx = W - gx < 4 ? W - gx : 4;
    g.mbits = 0;
    int seams = 0;
    if (mode != SEGK_MIX_NONE) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j >= g.npx) continue;
        const int m = s_m[ly + 1][lx + 1 + j];
        g.mbits |= m << j;
        if (has_seam) {
          const bool edge = (gy > 0 && s_m[ly][lx + 1 + j] != m) || (gy + 1 < H && s_m[ly + 2][lx + 1 + j] != m) ||
                            (gx + j > 0 && s_m[ly + 1][lx + j] != m) || (gx + j + 1 < W && s_m[ly + 1][lx + 2 + j] != m);
          seams |= (int)edge << j;
        }
      }
    }
    cnt = __popc((unsigned)g.mbits);
    g.ys = clampi(gy - dy, 0, H - 1);                      // used where a bit of mbits is set: then already inside
    g.step = flip ? -1 : 1;
    g.xs0 = flip ? W - 1 - (gx - dx) : gx - dx;
    const size_t at = (size_t)gy * W + gx, srow = (size_t)g.ys * W;
    {                                                      // label
      L v[4];
      gather4(own_lab + at, part_lab + srow, g, v);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((seams >> j) & 1) v[j] = (L)seam;
      scatter4(Yo + (size_t)b * HW + at, g, v);
    }
    if constexpr (!NHWC) {
      for (int c = 0; c < C; ++c) {
        E v[4];
        gather4(X + ((size_t)b * C + c) * HW + at, X + ((size_t)p * C + c) * HW + srow, g, v);
        scatter4(Xo + ((size_t)b * C + c) * HW + at, g, v);
      }
    } else {                                               // uint8 [H][W][C]: the four pixels are 4 C bytes, C words
      const uint8_t* own = (const uint8_t*)X + ((size_t)b * HW + at) * C;
      const uint8_t* prow = (const uint8_t*)X + ((size_t)p * HW + srow) * C;
      uint8_t* out = (uint8_t*)Xo + ((size_t)b * HW + at) * C;
      const bool full = g.npx == 4, out_words = full && ((uintptr_t)out & 3) == 0;
      const uint8_t* run = nullptr;                        // the 4 C source bytes where they are one run
      if (full && g.mbits == 0) run = own;
      else if (full && g.mbits == 15 && !flip) run = prow + (size_t)g.xs0 * C;
      if (run && out_words && ((uintptr_t)run & 3) == 0) {
        for (int w = 0; w < C; ++w) ((unsigned*)out)[w] = ((const unsigned*)run)[w];
      } else {
        for (int w = 0; w < C; ++w) {
          unsigned word = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = 4 * w + i, j = C == 1 ? k : C == 2 ? k >> 1 : C == 4 ? k >> 2 : k / 3, c = k - j * C;
            unsigned byte = 0;
            if (j < g.npx) byte = ((g.mbits >> j) & 1) ? prow[(size_t)(g.xs0 + j * g.step) * C + c] : own[k];
            word |= byte << (8 * i);
          }
          if (out_words) {
            ((unsigned*)out)[w] = word;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (4 * w + i < g.npx * C) out[4 * w + i] = (uint8_t)(word >> (8 * i));
          }
        }
      }
    }
  }
  if (mode == SEGK_MIX_NONE) return;                       // workgroup-uniform: nothing was pasted
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((tid & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);      // LDS
  __syncthreads();
  if (tid == 0 && s_cnt) atomicAdd(pasted + b, s_cnt);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int segk_mix_select(const segk_mix_desc* descs, int n_desc, int n, const void* y, int label_bytes, int H, int W,
                               const uint8_t* exclude, int n_classes, const int32_t* cc_rows, int n_slots, int things_mask,
                               int min_area, int max_area, int max_objects, int max_components, uint8_t* bytes, uint8_t* select,
                               int select_stride, int stage, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(descs && ((uintptr_t)descs & 7) == 0, "mix_select: NULL or misaligned descriptor table");
  SEGK_REQUIRE(n >= 1 && n <= 65535 && n_desc >= 1 && n_desc <= n, "mix_select: %d descriptors of %d samples (1..n, n <= 65535)", n_desc, n);
  SEGK_REQUIRE(y, "mix_select: NULL labels");
  SEGK_REQUIRE(label_bytes == 1 || label_bytes == 8, "mix_select: labels of %d bytes (uint8: 1, int64: 8)", label_bytes);
  SEGK_REQUIRE(((uintptr_t)y & (label_bytes - 1)) == 0, "mix_select: misaligned labels");
  SEGK_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= SEGK_CC_MAX_PIXELS, "mix_select: bad shape %d x %d (at most 2^28 pixels)", H, W);
  SEGK_REQUIRE(n_slots >= 0 && n_slots <= n, "mix_select: %d slots (0..n)", n_slots);
  SEGK_REQUIRE(max_components >= 1 && max_components <= SEGK_MIX_MAX_COMPONENTS, "mix_select: max_components=%d (1..%d)", max_components,
               SEGK_MIX_MAX_COMPONENTS);
  const long HW = (long)H * W;
  if (stage == SEGK_MIX_STAGE_BYTES) {
    SEGK_REQUIRE(label_bytes == 8, "mix_select: the byte stage is for int64 labels (uint8 labels are bytes already)");
    SEGK_REQUIRE(bytes && n_slots >= 1 && n_desc <= n_slots, "mix_select: the byte stage needs a byte buffer and a descriptor per slot");
    SEGK_REQUIRE(!overlap(bytes, (size_t)n_slots * HW, y, (size_t)n * HW * 8), "mix_select: the byte buffer overlaps the labels");
    const long want = (HW + 2047) / 2048;
    hipLaunchKernelGGL(mix_bytes_kernel, dim3((unsigned)(want < 256 ? want : 256), n_desc), dim3(256), 0, st, descs, n, (const long long*)y, HW,
                       n_slots, bytes);
    SEGK_CHECK_LAUNCH("mix_select");
    return 0;
  }
  SEGK_REQUIRE(stage == SEGK_MIX_STAGE_SELECT, "mix_select: stage %d (0 bytes, 1 select)", stage);
  SEGK_REQUIRE(n_desc == n, "mix_select: the select stage takes one descriptor per sample (%d of %d)", n_desc, n);
  SEGK_REQUIRE(select && exclude, "mix_select: NULL select or exclude table");
  SEGK_REQUIRE(n_classes >= 0 && n_classes <= 256, "mix_select: n_classes=%d (0: half of the candidates, else 1..256)", n_classes);
  SEGK_REQUIRE(select_stride >= 256 && (n_slots == 0 || select_stride >= max_components), "mix_select: select_stride=%d (>= 256 and >= max_components)",
               select_stride);
  SEGK_REQUIRE(!overlap(select, (size_t)n * select_stride, y, (size_t)n * HW * label_bytes), "mix_select: the select table overlaps the labels");
  if (n_slots > 0) {
    SEGK_REQUIRE(cc_rows && ((uintptr_t)cc_rows & 3) == 0, "mix_select: NULL or misaligned component rows");
    SEGK_REQUIRE(things_mask >= 0 && things_mask < (1 << SEGK_MAX_CLASSES), "mix_select: things_mask=%d (bits 0..7)", things_mask);
    SEGK_REQUIRE(min_area >= 0 && max_area >= min_area, "mix_select: areas %d..%d", min_area, max_area);
    SEGK_REQUIRE(max_objects >= 1 && max_objects <= SEGK_MIX_MAX_OBJECTS, "mix_select: max_objects=%d (1..%d)", max_objects, SEGK_MIX_MAX_OBJECTS);
  }
  const int mo = n_slots > 0 ? max_objects : 1;
  if (label_bytes == 1)
    hipLaunchKernelGGL(mix_select_kernel<uint8_t>, dim3(n), dim3(SEL_THREADS), 0, st, descs, n, (const uint8_t*)y, HW, exclude, n_classes, cc_rows,
                       n_slots, things_mask, min_area, max_area, mo, max_components, select, select_stride);
  else
    hipLaunchKernelGGL(mix_select_kernel<long long>, dim3(n), dim3(SEL_THREADS), 0, st, descs, n, (const long long*)y, HW, exclude, n_classes,
                       cc_rows, n_slots, things_mask, min_area, max_area, mo, max_components, select, select_stride);
  SEGK_CHECK_LAUNCH("mix_select");
  return 0;
}

extern "C" int segk_mix_apply(const segk_mix_desc* descs, int n, const void* X, const void* y, void* X_out, void* y_out, int32_t* pasted,
                              int C, int H, int W, int elem_bytes, int label_bytes, const uint8_t* select, int select_stride,
                              const int32_t* ids, int n_slots, int max_components, int has_seam, long seam_value, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(descs && ((uintptr_t)descs & 7) == 0, "mix_apply: NULL or misaligned descriptor table");
  SEGK_REQUIRE(n >= 1 && n <= 65535, "mix_apply: %d samples (1..65535)", n);
  SEGK_REQUIRE(X && y && X_out && y_out && pasted && select, "mix_apply: NULL pointer");
  SEGK_REQUIRE(C >= 1 && C <= 4, "mix_apply: %d channels (1..4)", C);
  SEGK_REQUIRE(H >= 1 && W >= 1 && (long)H * W <= SEGK_CC_MAX_PIXELS, "mix_apply: bad shape %d x %d (at most 2^28 pixels)", H, W);
  SEGK_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4, "mix_apply: image elements of %d bytes (1 uint8 NHWC, 2 or 4 NCHW)", elem_bytes);
  SEGK_REQUIRE(label_bytes == 1 || label_bytes == 8, "mix_apply: labels of %d bytes (uint8: 1, int64: 8)", label_bytes);
  SEGK_REQUIRE(n_slots >= 0 && n_slots <= n, "mix_apply: %d slots (0..n)", n_slots);
  SEGK_REQUIRE(max_components >= 1 && max_components <= SEGK_MIX_MAX_COMPONENTS, "mix_apply: max_components=%d (1..%d)", max_components,
               SEGK_MIX_MAX_COMPONENTS);
  SEGK_REQUIRE(select_stride >= 256 && (n_slots == 0 || select_stride >= max_components), "mix_apply: select_stride=%d (>= 256 and >= max_components)",
               select_stride);
  SEGK_REQUIRE(n_slots == 0 || ids, "mix_apply: %d slots without an id map", n_slots);
  SEGK_REQUIRE(has_seam == 0 || has_seam == 1, "mix_apply: has_seam=%d (0 | 1)", has_seam);
  SEGK_REQUIRE(!has_seam || label_bytes == 8 || (seam_value >= 0 && seam_value <= 255), "mix_apply: seam_value %ld does not fit a uint8 label",
               seam_value);
  SEGK_REQUIRE((((uintptr_t)X | (uintptr_t)X_out) & (elem_bytes - 1)) == 0 && (((uintptr_t)y | (uintptr_t)y_out) & (label_bytes - 1)) == 0 &&
               (((uintptr_t)pasted | (uintptr_t)ids) & 3) == 0, "mix_apply: misaligned buffer");
  const size_t HW = (size_t)H * W, xb = (size_t)n * C * HW * elem_bytes, yb = (size_t)n * HW * label_bytes, pb = (size_t)n * 4;
  // partners are read while outputs are written
  SEGK_REQUIRE(!overlap(X_out, xb, X, xb) && !overlap(X_out, xb, y, yb) && !overlap(y_out, yb, X, xb) && !overlap(y_out, yb, y, yb) &&
               !overlap(pasted, pb, X, xb) && !overlap(pasted, pb, y, yb), "mix_apply: an output overlaps an input");
  SEGK_REQUIRE(!overlap(X_out, xb, y_out, yb) && !overlap(pasted, pb, X_out, xb) && !overlap(pasted, pb, y_out, yb), "mix_apply: the outputs overlap");
  SEGK_REQUIRE(!overlap(select, (size_t)n * select_stride, X_out, xb) && !overlap(select, (size_t)n * select_stride, y_out, yb) &&
               !overlap(select, (size_t)n * select_stride, pasted, pb), "mix_apply: an output overlaps the select table");
  SEGK_REQUIRE(!ids || (!overlap(ids, (size_t)n_slots * HW * 4, X_out, xb) && !overlap(ids, (size_t)n_slots * HW * 4, y_out, yb) &&
                        !overlap(ids, (size_t)n_slots * HW * 4, pasted, pb)), "mix_apply: an output overlaps the id maps");
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;            // at most 2^28 / 16 tiles
  const dim3 grid((unsigned)((long)tiles_x * tiles_y), n), block(256);
  const long long seam = seam_value;
#define SEGK_MIX_LAUNCH(E, NHWC, L)                                                                                                     \
  hipLaunchKernelGGL((mix_apply_kernel<E, NHWC, L>), grid, block, 0, st, descs, n, (const E*)X, (const L*)y, (E*)X_out, (L*)y_out, pasted, C, \
                     H, W, select, select_stride, ids, n_slots, max_components, has_seam, seam, tiles_x)
  if (label_bytes == 1) {
    if (elem_bytes == 4) SEGK_MIX_LAUNCH(uint32_t, false, uint8_t);
    else if (elem_bytes == 2) SEGK_MIX_LAUNCH(uint16_t, false, uint8_t);
    else SEGK_MIX_LAUNCH(uint8_t, true, uint8_t);
  } else {
    if (elem_bytes == 4) SEGK_MIX_LAUNCH(uint32_t, false, long long);
    else if (elem_bytes == 2) SEGK_MIX_LAUNCH(uint16_t, false, long long);
    else SEGK_MIX_LAUNCH(uint8_t, true, long long);
  }
#undef SEGK_MIX_LAUNCH
  SEGK_CHECK_LAUNCH("mix_apply");
  return 0;
}
