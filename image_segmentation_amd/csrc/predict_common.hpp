// What the prediction finishers share, each stated once: the source index / blend helpers of F.interpolate,
// the slot-window sampler, the first-maximum argmax, the class softmax, the mask sink (everything a kernel does once a
// pixel's class is known) and the host-side launch helpers.  With -ffp-contract=off one source expression gives one bit
// pattern: the exact agreements the tests pin (fused mask == crop_resize + argmax, the temperature sweep at inv_T = 1 ==
// predict_merge, tiles == views) hold because every kernel calls the expressions below instead of restating them.
//   resize.hip   bilinear, resize_pad, crop_resize      index and blend helpers
//   predict.hip  predict_mask, predict_merge            sampler, argmax, softmax, sink
//                mask_finish                            sink
//   tiles.hip    predict_tiles                          argmax, softmax, sink
//   calib.hip    calib_temps                            sampler, argmax
// Everything is __forceinline__ and every register array (pal, cnt, c4, cf, best, lab) is indexed by unrolled constants
// only, so the arrays stay in registers: callers pass j from a `#pragma unroll` loop.
#pragma once
#include <type_traits>

#include "class_pixels.hpp"
#include "segk_internal.h"

// ---- index and blend: ATen's area_pixel_compute_source_index (align_corners=False), its two-tap blend, and "nearest" --------
__device__ __forceinline__ void src_index(int o, float scale, int in_size, int& i0, int& i1, float& lam) {
  float s = scale * ((float)o + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  lam = s - (float)i0;
}
__device__ __forceinline__ float bilerp(float a, float b, float d, float e, float ly, float lx) {
  // ATen: (1-ly)*((1-lx)*a + lx*b) + ly*((1-lx)*d + lx*e)
  return (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * d + lx * e);
}
__device__ __forceinline__ int nearest_index(int o, float scale, int in_size) {
  const int s = (int)floorf((float)o * scale);
  return s > in_size - 1 ? in_size - 1 : s;
}

// ---- window sampler: the NC class values of one output pixel of crop_resize (MODE 0 bilinear, 1 nearest) --------------------
// Per-class window origins are uniform (scalar registers); a tap is origin + a 32-bit BYTE offset, the addressing form that
// costs no 64-bit vector arithmetic per load.  Classes past C repeat class C - 1: they can never win argmax_first's strict
// comparison, and sums over classes skip them.  Loads are unconditional at clamped indices and all 4 * NC taps are issued
// before the blends, so they are in flight together.
__device__ __forceinline__ float tap(const char* origin, unsigned byte_off) { return *(const float*)(origin + byte_off); }

template <int NC>
__device__ __forceinline__ void window_origins(const float* slot, int C, int T, int pt, int pl, const char* (&wk)[NC]) {
#pragma unroll
  for (int k = 0; k < NC; ++k) wk[k] = (const char*)(slot + ((size_t)(k < C ? k : C - 1) * T + pt) * T + pl);
}

// the y half of a pixel's taps: a thread that walks along a row recomputes it only where it steps over the row end
struct RowTaps {
  int y0, y1;
  float ly;
};
template <int MODE>
__device__ __forceinline__ RowTaps row_taps(int sy, float sh, int nh) {
  RowTaps r;
  r.ly = 0.f;
  if (MODE == 1) r.y0 = r.y1 = nearest_index(sy, sh, nh);
  else src_index(sy, sh, nh, r.y0, r.y1, r.ly);
  return r;
}
template <int NC, int MODE>
__device__ __forceinline__ void sample_window(const char* const (&wk)[NC], unsigned pitch, const RowTaps& r, int sx, float sw, int nw,
                                              float (&v)[NC]) {
  if (MODE == 1) {
    const unsigned o = (unsigned)r.y0 * pitch + 4u * (unsigned)nearest_index(sx, sw, nw);
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] = tap(wk[k], o);
  } else {
    int x0, x1;
    float lx;
    src_index(sx, sw, nw, x0, x1, lx);
    const unsigned r0 = (unsigned)r.y0 * pitch, r1 = (unsigned)r.y1 * pitch, c0 = 4u * (unsigned)x0, c1 = 4u * (unsigned)x1;
    float a[NC], b[NC], d[NC], e[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      a[k] = tap(wk[k], r0 + c0); b[k] = tap(wk[k], r0 + c1); d[k] = tap(wk[k], r1 + c0); e[k] = tap(wk[k], r1 + c1);
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) v[k] = bilerp(a[k], b[k], d[k], e[k], r.ly, lx);
  }
}
template <int NC, int MODE>
__device__ __forceinline__ void sample_window(const char* const (&wk)[NC], unsigned pitch, int sy, int sx, float sh, float sw, int nh,
                                              int nw, float (&v)[NC]) {
  sample_window<NC, MODE>(wk, pitch, row_taps<MODE>(sy, sh, nh), sx, sw, nw, v);
}

// ---- argmax and softmax over the classes --------------------------------------------------------------------------------
// first maximum, NaN maximal (confusion_kernel / torch.argmax); selects, not branches
template <int NC>
__device__ __forceinline__ int argmax_first(const float (&v)[NC]) {
  int bi = 0;
  float bv = v[0];
#pragma unroll
  for (int k = 1; k < NC; ++k) {
    const bool take = (v[k] > bv) | ((v[k] != v[k]) & (bv == bv));
    bv = take ? v[k] : bv;
    bi = take ? k : bi;
  }
  return bi;
}

// m = max z, e_k = expf(z_k - m), p_k = e_k / sum_k e_k, the sum in class order
template <int NC>
__device__ __forceinline__ void softmax_classes(float (&z)[NC], int C) {
  float m = z[0];
#pragma unroll
  for (int k = 1; k < NC; ++k) m = z[k] > m ? z[k] : m;
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    z[k] = expf(z[k] - m);
    sum = sum + ((NC <= 4 || k < C) ? z[k] : 0.f);
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) z[k] = z[k] / sum;
}

// ---- the thread's four pixels -------------------------------------------------------------------------------------------
// A thread owns four consecutive FLAT pixels p .. p + 3 of a W-wide image, p % 4 == 0 (the mask leaves as one aligned dword,
// the colour as three); one past the end repeats the last, and a thread may straddle a row end.
__device__ __forceinline__ void four_pixels(int p, int total, int W, int (&oy)[4], int (&ox)[4]) {
  oy[0] = p / W; ox[0] = p - oy[0] * W;
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    oy[j] = oy[j - 1]; ox[j] = ox[j - 1];
    if (p + j < total && ++ox[j] == W) { ox[j] = 0; ++oy[j]; }
  }
}

// ---- mask sink: everything after "pixel j of this thread has class bi" --------------------------------------------------
// Class counts live in registers over the grid-stride loop and are summed per wave, confusion counts go to an LDS histogram
// [64 confusion bins | 8 class counts] the kernel declares (`__shared__ unsigned int hist[Sink::HIST]`); a block ends with
// one 64-bit atomic per non-zero bin (integers: order-independent, bit-stable).  Outputs that are NULL are not written; a
// kernel that has no confidence or scores passes a literal nullptr and the code folds away, and MASK = false (mask_finish,
// whose mask is its input) stores no mask.
// A pixel counts only where the caller calls it `live`, and a class outside 0 .. NC - 1 matches no palette entry and is
// coloured black.  The argmax kernels can never choose a class >= C and their only dead pixels lie past the image's end;
// mask_finish, which alone can meet a mask value >= C, hands it over as not live and as class NC.
// The register arrays are an object of their own (Regs), which the kernel declares beside the histogram: an array is
// indexed by a loop counter until the loops are unrolled, and scalars that shared its object would sit in memory with it
// until then -- enough to cost predict_merge<8, 1, false> its fourth wave.
// Use:  Sink::Regs regs;  Sink sink(regs, hist, ...);
//       for each quad { sink.begin(p); account(j, ..) or merged(j, ..) for j = 0..3; sink.store(); }   sink.finish();
template <int NC, bool LAB, bool MASK = true>
struct MaskSink {
  static constexpr int NB = SEGK_MAX_CLASSES * SEGK_MAX_CLASSES, HIST = NB + SEGK_MAX_CLASSES;
  struct Regs {
    unsigned int pal[NC], cnt[NC], c4[4], cf[4];
    int best[4];
    long long lab[4];
  };
  unsigned int* hist;
  uint8_t *mask, *color, *conf;
  float* scores;
  unsigned long long *counts, *M;
  const long long* labels;
  int C, total, p;
  unsigned int (&pal)[NC], (&cnt)[NC], (&c4)[4], (&cf)[4];
  int (&best)[4];
  long long (&lab)[4];

  __device__ __forceinline__ MaskSink(Regs& r, unsigned int* hist_, uint8_t* mask_, uint8_t* color_, const uint8_t* palette,
                                      unsigned long long* counts_, const long long* labels_, unsigned long long* M_, uint8_t* conf_,
                                      float* scores_, int C_, int total_)
      : hist(hist_), mask(mask_), color(color_), conf(conf_), scores(scores_), counts(counts_), M(M_), labels(labels_), C(C_),
        total(total_), p(0), pal(r.pal), cnt(r.cnt), c4(r.c4), cf(r.cf), best(r.best), lab(r.lab) {
    if (threadIdx.x < HIST) hist[threadIdx.x] = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      pal[k] = 0; cnt[k] = 0;
      if (color) {                                        // unconditional loads: entries past C repeat entry C - 1
        const uint8_t* q = palette + 3 * (k < C ? k : C - 1);
        pal[k] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
      }
    }
    __syncthreads();
  }

  // the quad at flat pixel p_: its labels, at clamped indices
  __device__ __forceinline__ void begin(int p_) {
    p = p_;
    if (LAB) {
#pragma unroll
      for (int j = 0; j < 4; ++j) lab[j] = labels[(unsigned)(p + j < total ? p + j : total - 1)];
    }
  }
  __device__ __forceinline__ unsigned live(int j) const { return p + j < total ? 1u : 0u; }

  // class count, palette pick, confusion bin
  __device__ __forceinline__ void account(int j, int bi, unsigned lv) {
    best[j] = bi;
    c4[j] = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      cnt[k] += bi == k ? lv : 0u;
      c4[j] = bi == k ? pal[k] : c4[j];
    }
    if (LAB && lv && lab[j] >= 0 && lab[j] < C) atomicAdd(&hist[bi * SEGK_MAX_CLASSES + (int)lab[j]], 1u);
  }

  // a merged accumulator (views, tiles): its class, and p = acc / sum acc (prob merge) or softmax(acc) (logit merge) for the
  // confidence byte round(255 p_best) and the scores
  __device__ __forceinline__ void merged(int j, const float (&acc)[NC], int merge) {
    const int bi = argmax_first<NC>(acc);
    account(j, bi, live(j));
    cf[j] = 0;
    if (conf || scores) {
      float pr[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) pr[k] = acc[k];
      if (merge == SEGK_MERGE_PROB) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) sum = sum + ((NC <= 4 || k < C) ? pr[k] : 0.f);
#pragma unroll
        for (int k = 0; k < NC; ++k) pr[k] = pr[k] / sum;
      } else {
        softmax_classes<NC>(pr, C);
      }
      float pb = pr[0];
#pragma unroll
      for (int k = 1; k < NC; ++k) pb = bi == k ? pr[k] : pb;
      const float c = 255.f * pb + 0.5f;
      cf[j] = c >= 0.f ? (unsigned)(c > 255.f ? 255.f : c) : 0u;     // a NaN confidence is stored as 0
      if (scores && live(j)) {
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (NC <= 4 || k < C) scores[(size_t)k * total + (unsigned)(p + j)] = pr[k];
      }
    }
  }

  // the quad's packed store: one mask dword, one confidence dword, three colour dwords; bytes for the image's last pixels
  __device__ __forceinline__ void store() {
    if (p + 3 < total) {
      if (MASK) *(uint32_t*)(mask + (unsigned)p) = (unsigned)best[0] | ((unsigned)best[1] << 8) | ((unsigned)best[2] << 16) | ((unsigned)best[3] << 24);
      if (conf) *(uint32_t*)(conf + (unsigned)p) = cf[0] | (cf[1] << 8) | (cf[2] << 16) | (cf[3] << 24);
      if (color)
        *(uint3*)(color + (size_t)p * 3) = make_uint3(c4[0] | (c4[1] << 24), (c4[1] >> 8) | (c4[2] << 16), (c4[2] >> 16) | (c4[3] << 8));
    } else {
      for (int j = 0; j < 4; ++j)
        if (p + j < total) {
          if (MASK) mask[p + j] = (uint8_t)best[j];
          if (conf) conf[p + j] = (uint8_t)cf[j];
          if (color)
            for (int b = 0; b < 3; ++b) color[(size_t)(p + j) * 3 + b] = (uint8_t)(c4[j] >> (8 * b));
        }
    }
  }

  // the block's sums: wave sums first (64 lanes adding to one LDS word serialise), then one 64-bit atomic per non-zero bin
  __device__ __forceinline__ void finish() {
    if (counts) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        unsigned int c = cnt[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(&hist[NB + k], c);
      }
    }
    __syncthreads();
    if (LAB && threadIdx.x < NB && hist[threadIdx.x]) atomicAdd(&M[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
    if (counts && threadIdx.x >= NB && threadIdx.x < HIST && hist[threadIdx.x])
      atomicAdd(&counts[threadIdx.x - NB], (unsigned long long)hist[threadIdx.x]);
  }
};

// ---- host side ------------------------------------------------------------------------------------------------------------
// Blocks of a finisher over `pixels` pixels (256 threads x 4 pixels).  The neighbours' 16384-block cap for the mask / colour
// alone.  With counts or labels every block ends in 64-bit atomics on the same few words, and those serialise in L2 at
// ~12 ns per block (measured: 11719 blocks at 3000x4000 took 150 us against 30 us without the counts), so the grid becomes
// persistent: three blocks per CU, one resident round for every instance (the 8-class bilinear one fits three), 17 us at
// 1200x1600 and 36-42 us at 3000x4000.
inline int finisher_grid(long pixels, bool counting) {
  const long g = ((pixels + 3) / 4 + 255) / 256, cap = counting ? 3L * segk_num_cus() : 16384;
  return (int)(g > cap ? cap : g);
}

// The checks of a finisher's output pointers, in two steps because each entry has checks of its own between them and the
// first failing check names the error.  conf and scores: NULL for an entry that has neither.
inline int check_output_pairs(const char* name, const void* color, const void* palette, const void* labels, const void* M) {
  SEGK_REQUIRE((color == nullptr) == (palette == nullptr), "%s: color and palette come together", name);
  SEGK_REQUIRE((labels == nullptr) == (M == nullptr), "%s: labels and M come together", name);
  return 0;
}
inline int check_output_alignment(const char* name, bool merged, const void* mask, const void* color, const void* conf,
                                  const void* scores) {
  SEGK_REQUIRE((((uintptr_t)mask | (uintptr_t)color | (uintptr_t)conf | (uintptr_t)scores) & 3) == 0,
               "%s: mask%s must be 4-byte aligned", name, merged ? ", color, conf and scores" : " and color");
  return 0;
}

// The kernels are compiled for 1, 2, 3, 4 and SEGK_MAX_CLASSES classes: f(integral_constant<smallest that holds C>)
template <typename F>
inline auto dispatch_classes(int C, F f) { return dispatch_each_nc(C, f); }
