// What the channel-vector streaming kernels share, each stated once: NHWC tensors, a thread owns one channel
// vector (its per-channel constants live in registers) and walks pixels, a block reduces its threads' channel sums in one fixed
// order, and a 1024-thread block adds the partial rows in float64.  With -ffp-contract=off one source expression gives one bit
// pattern and every sum below has ONE order of additions, so the agreements the tests pin (tests/golden/bn_pool_bits.json,
// tests/golden/loss_bits.json) hold because the kernels call the code below instead of restating it.
//   bn_pool.hip   bn_relu_apply, bn_bwd_reduce, bn_bwd_apply, channel_sum        lane map, pixel walk (not bn_bwd_apply), row reduce,
//                                                                                 constants
//                 bn_stats_finalize_small, bn_bwd_finalize, channel_sum_finalize  partial-row sum (+ the statistics finish)
//                 bn_relu_apply_pool, maxpool_bwd (both loops)                    the 2x2 window
//   head.hip      head_bwd, head_bn_bwd_apply                                    lane map, row reduce, constants, pixel walk (apply)
// Deliberately NOT here: bn_bwd_apply_kernel's walk (through walk_pixels the bf16 instance took 78 registers and six waves instead
// of 100 and four and ran 2 to 3 us slower: see the kernel), head_bwd_kernel's pixel loop (two pixels in flight, each stream carrying its own (image, offset) pair
// that is advanced after the use: walk_pixels' load sees a pixel index, not the stream it belongs to), its dW / db reduce (sums NC
// of the MAXC columns of a row, and the bias column in one lane only), maxpool_bwd_kernel<STAT>'s reduce (the 256 threads of a
// block share channels by thread index, not by lane row), maxpool_fwd_kernel's window (the even part of the image only: nothing
// to clamp), the eval branch and the ticket kernel's two-stage sum of finalize_channels, pack.hip's colsum_block (eight
// accumulators, another order of additions), the conv epilogues and stem.hip.
// Measured against the parent on one box: profiles/channel_refactor_kbench.txt; registers: profiles/channel_refactor_registers.txt.
// Everything is __forceinline__ and every register array is indexed by unrolled constants only.
#pragma once
#include <type_traits>

#include "common.hpp"

// ---- lane map: a block of 256 threads = cvb channel vectors x rows pixel lanes (cvb * rows <= 256, the rest idle); grid.y covers
// the channel blocks.  The cap is 128 vectors for the 16-byte vectors of bn_pool.hip and 64 for the head's (four channels each) ----
struct LaneGeometry { int cvb, rows, gy; };
static inline LaneGeometry lane_geometry(int cvec, int cap) {
  LaneGeometry g;
  g.cvb = cvec < cap ? cvec : cap;
  g.rows = 256 / g.cvb;
  g.gy = cdiv(cvec, g.cvb);
  return g;
}
constexpr int BN_LANE_CAP = 128, HEAD_LANE_CAP = 64;
// blocks (grid.x) of an apply pass: one per `rows` pixels, at most 4096 (the walk takes the rest in further trips)
static inline int apply_blocks(long P, int rows) {
  const long g = (P + rows - 1) / rows;
  return (int)(g > 4096 ? 4096 : g);
}

struct ChannelLanes {
  int cx, ry, cv;
  bool in_c, in_r;         // the thread's channel vector exists; its pixel lane exists
  __device__ __forceinline__ bool active() const { return in_c && in_r; }
};
__device__ __forceinline__ ChannelLanes channel_lanes(int cvb, int rows, int cvec) {
  ChannelLanes l;
  l.cx = threadIdx.x % cvb;
  l.ry = threadIdx.x / cvb;
  l.cv = blockIdx.y * cvb + l.cx;
  l.in_c = l.cv < cvec;
  l.in_r = l.ry < rows;
  return l;
}

// ---- pixel walk of lane (blockIdx.x, ry): p = first, first + step, ... < P.  PIF pixels per trip: all their loads are issued
// before the first is used (v = load(p), then use(p, v) in pixel order), then a one-pixel tail.  The barrier keeps the scheduler
// from sinking the loads back to two in flight.  Pixels in flight, measured at B = 32 on one box:
//   read-only passes (bn_bwd_reduce, channel_sum)   4   the grid is only two blocks per CU (short finalize), and left to itself the
//                                                       compiler keeps one pixel in flight
//   passes that write as much as they read          1   bn_bwd_apply (its own walk, this count): reduce + finalize + apply 250 / 274 / 278 us at 1 / 2 / 4
//                                                       pixels, 64 ch x 256^2 (122 / 125 / 132 at 128 x 128^2); head_bn_bwd_apply: 253
//                                                       against 256 us with two (profiles/end_fusion_kbench.txt); such a stream runs
//                                                       best with one pixel per thread and the occupancy that leaves
constexpr int REDUCE_FLIGHT = 4, APPLY_FLIGHT = 1;
template <int PIF, typename L, typename U>
__device__ __forceinline__ void walk_pixels(long first, long step, long P, L&& load, U&& use) {
  long p = first;
  if constexpr (PIF > 1) {
    for (; p + (PIF - 1) * step < P; p += PIF * step) {
      decltype(load(p)) v[PIF];
#pragma unroll
      for (int u = 0; u < PIF; ++u) v[u] = load(p + u * step);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < PIF; ++u) use(p + u * step, v[u]);
    }
  }
  for (; p < P; p += step) use(p, load(p));
}

// ---- block row reduce: every pixel lane puts its NW channel sums into LDS red[rows][cvb][pitch], lane row 0 adds the rows in row
// order from 0.f (bit-stable) and hands the NW totals of its channel vector to write(tot): one partial row per block ----------------
template <int NW, typename W>
__device__ __forceinline__ void reduce_lane_rows(float* __restrict__ red, const ChannelLanes& l, int cvb, int rows, int pitch,
                                                 const float (&sums)[NW], W&& write) {
  if (l.in_r) {
    float* q = red + ((size_t)l.ry * cvb + l.cx) * pitch;
#pragma unroll
    for (int i = 0; i < NW; ++i) q[i] = sums[i];
  }
  __syncthreads();
  if (l.ry == 0 && l.in_c) {
    float tot[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) tot[i] = 0.f;
    for (int r = 0; r < rows; ++r) {  // fixed order
      const float* q = red + ((size_t)r * cvb + l.cx) * pitch;
#pragma unroll
      for (int i = 0; i < NW; ++i) tot[i] += q[i];
    }
    write(tot);
  }
}

// ---- partial-row sum: a block of 1024 threads = 32 channels (c = blockIdx.x * 32 + cx) x 32 row lanes adds the NB rows of
// part[NB][C][NV] in float64.  Sixteen rows in flight per lane and ONE accumulator per word (the registers hold loads, not partial
// sums: 1024 threads leave 128 per lane), so NB <= 512 is a single memory round trip; unconditional loads of a clamped row (a
// conditional load compiles to branch + wait); the 32 lane sums are added in lane order.  Fixed order of additions: bit-stable.
// Returns true in the thread (row lane 0) that holds the channel's sums in s ----------------------------------------------------
template <int NV>
__device__ __forceinline__ bool sum_rows16(const float* __restrict__ part, int NB, int C, double (&s)[NV]) {
  static_assert(NV == 1 || NV == 2, "rows of floats or of float2");
  using Row = std::conditional_t<NV == 2, float2, float>;
  __shared__ double sh[32][32][NV];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  auto word = [](const Row& v, int i) {
    if constexpr (NV == 2) return i == 0 ? v.x : v.y;
    else return v;
  };
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = 0.0;
#pragma unroll 1
  for (int m = ry; m < NB; m += 512) {
    Row v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int r = m + 32 * u < NB ? m + 32 * u : NB - 1;
      v[u] = ((const Row*)part)[(unsigned)r * (unsigned)C + (unsigned)c];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const bool ok = m + 32 * u < NB;
#pragma unroll
      for (int i = 0; i < NV; ++i) s[i] += ok ? (double)word(v[u], i) : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) sh[ry][cx][i] = s[i];
  __syncthreads();
  if (ry != 0) return false;
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = 0.0;
#pragma unroll 8
  for (int r = 0; r < 32; ++r) {   // (32 reads in flight would spill)
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] += sh[r][cx][i];
  }
  return true;
}

// ---- training-mode BatchNorm of channel c (gamma g, beta be, conv bias cb) from its sums (s1, s2) = (sum x, sum x^2) over `count`
// values of the bias-free conv output: scale, shift, mean, rstd and the running statistics (biased variance to normalise,
// unbiased into running_var; the conv bias cancels in the normalisation and only moves the running mean).  A padded channel stays
// identically zero: bn_channel_zero ------------------------------------------------------------------------------------------
__device__ __forceinline__ void bn_channel_zero(int c, float* scale, float* shift, float* mean_out, float* rstd_out) {
  scale[c] = 0.f; shift[c] = 0.f;
  if (mean_out) { mean_out[c] = 0.f; rstd_out[c] = 0.f; }
}
__device__ __forceinline__ void bn_channel_finish(double s1, double s2, double count, int c, float g, float be, float cb,
                                                  float* rmean, float* rvar, float momentum, float eps, float* scale, float* shift,
                                                  float* mean_out, float* rstd_out) {
  const double mean = s1 / count;
  double var = s2 / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = g * rstd;
  scale[c] = sc;
  shift[c] = be - (float)mean * sc;      // applied to the bias-free conv output: the bias cancels
  mean_out[c] = (float)mean;
  rstd_out[c] = rstd;
  if (rmean) {
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    rmean[c] = (1.f - momentum) * rmean[c] + momentum * ((float)mean + cb);
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
  }
}

// ---- the BatchNorm constants of a thread's V channels from c0 on; COEF: also (c1, c2) = coef[c][0..1] -----------------------------
template <int V, bool COEF = false>
struct BnConsts {
  float sc[V], sh[V], mu[V], rs[V], c1[COEF ? V : 1], c2[COEF ? V : 1];
  __device__ __forceinline__ BnConsts(const float* __restrict__ scale, const float* __restrict__ shift,
                                      const float* __restrict__ mean, const float* __restrict__ rstd, int c0,
                                      const float* __restrict__ coef = nullptr) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = c0 + j;
      sc[j] = scale[c]; sh[j] = shift[c]; mu[j] = mean[c]; rs[j] = rstd[c];
      if constexpr (COEF) { c1[j] = coef[2 * c]; c2[j] = coef[2 * c + 1]; }
    }
  }
};

// ---- the 2x2 window (yo, xo) of image b, channel vector cv, of an NHWC tensor of T: the offsets of its four pixels from
// coordinates clamped into the image, so that all four loads are issued together, unconditionally (a load under a per-lane
// condition compiles to branch + load + wait: four serial round trips per window); inside(k) tells the pixels that exist.
// Windows also cover the odd border of the image -------------------------------------------------------------------------------
template <typename T>
struct Window2x2 {
  size_t off[4];
  int b, cv, y0, x0, H, W, C;
  __device__ __forceinline__ Window2x2(int b_, int yo, int xo, int cv_, int H_, int W_, int C_, bool offsets = true)
      : b(b_), cv(cv_), y0(2 * yo), x0(2 * xo), H(H_), W(W_), C(C_) {
    if (offsets) {
#pragma unroll
      for (int k = 0; k < 4; ++k) off[k] = at(k);
    }
  }
  // offset of pixel k (for a loop over k that is not unrolled: off[] is for unrolled ones)
  __device__ __forceinline__ size_t at(int k) const {
    const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
    return (((size_t)(b * H + (yy < H ? yy : H - 1))) * W + (xx < W ? xx : W - 1)) * C + cv * ET<T>::VEC;
  }
  __device__ __forceinline__ bool inside(int k) const { return y0 + (k >> 1) < H && x0 + (k & 1) < W; }
  __device__ __forceinline__ void load(const T* __restrict__ x, uint4 (&raw)[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = *(const uint4*)(x + off[k]);
  }
};

// ---- host: blocks of 256 threads for B x (H/2) x (W/2) windows x channel vectors (odd_border: the windows also cover an odd last
// row / column), at most cap; 0 when the items do not fit the kernels' 32-bit index ----------------------------------------------
static inline int window_grid(int B, int H, int W, int C, int dtype, bool odd_border, int cap) {
  const int vec = dtype == SEGK_DT_BF16 ? 8 : 4, odd = odd_border ? 1 : 0;
  const long total = (long)B * ((H + odd) / 2) * ((W + odd) / 2) * (C / vec);
  if (total >= (1L << 31)) return 0;
  const long g = (total + 255) / 256;
  return (int)(g > cap ? cap : g);
}
