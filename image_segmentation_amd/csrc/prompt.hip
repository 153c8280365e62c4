// Point prompts of the prompt model (reference utils/augmentation.ipynb, cell "Prompt Augmentation": create_gaussian_heatmap,
// select_dominant_class and the retry loop around them; prompt_based/prompt.py reads the results as heat-map / label files).
//
// Every value that decides a result is LOOKED UP, never computed here: the host builds w[d2] = exp(-d2 / (2 sigma^2)) in
// float64 and q[d2] = (uint8)(255 w[d2]) with the reference's own expression, indexed by the integer squared distance
// d2 = dy^2 + dx^2.  So the heat-map is the reference's 8-bit file bit for bit and the score terms are the reference's terms.
//
//  prompt_scores_kernel   one wave per (image, candidate centre): per-class float64 sums of w over the (2R+1)^2 window around
//                         the centre clipped to the image (lane = column, loop over rows), per-lane accumulators for the 8
//                         classes, then a fixed shuffle tree -- no atomics, two runs give the same bits -- and the
//                         reference's choice (largest sum among classes 1..7, lowest class on a tie, 0 below 1e-9).
//  prompt_make_kernel     per image: the first `per_image` distinct non-zero classes in candidate order (the reference's
//                         while loop as a parallel "first index per class" minimum), then one pass over the image: label in,
//                         per taken candidate heat = q[d2] / 255 and target = (label == class ? class : 0) out.
//  prompt_heatmap_kernel  P points -> heat = q[min over the points of d2] / 255 (prediction side).
//
// Centres, classes and points are device data the entry points cannot see: a centre outside the image contributes nothing
// (class 0, never taken, zero heat), a class outside 1..7 is ignored, and every table index is bounded by the table length.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int NC = SEGK_MAX_CLASSES;
constexpr int MAXPI = NC - 1;             // distinct non-zero classes an image can yield
constexpr int MAXPTS = 1024;              // points of one prediction heat-map (staged in LDS)
constexpr unsigned long long NOT_FOUND = ~0ULL;

// label -> class through the 256-entry table in LDS; labels outside 0..255 are class 0
__device__ __forceinline__ int class_of(long long v, const uint8_t* s_lut) {
  const int c = s_lut[(int)(v & 255)];
  return (v & ~255LL) ? 0 : c;
}

// the table a block works with: lut[i] (results >= NC count as class 0), or the identity on 0..NC-1 without a table.
// `any` is a valid address that is read (and ignored) when there is no table, so the load is unconditional.
__device__ __forceinline__ void stage_lut(const uint8_t* __restrict__ lut, const void* any, uint8_t* s_lut) {
  const int t = threadIdx.x;
  const uint8_t* src = lut ? lut : (const uint8_t*)any;
  const int raw = src[lut ? t : 0];
  const int c = lut ? raw : t;
  s_lut[t] = (uint8_t)(c < NC ? c : 0);
}

__global__ __launch_bounds__(256) void prompt_scores_kernel(const long long* __restrict__ labels, const uint8_t* __restrict__ lut,
                                                            const int2* __restrict__ centers, const double* __restrict__ w,
                                                            int nw, int R, double* __restrict__ scores, int* __restrict__ cls,
                                                            int K, int H, int W) {
  __shared__ uint8_t s_lut[256];
  stage_lut(lut, w, s_lut);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  if (k >= K) return;
  const size_t ck = (size_t)b * K + k;
  const int2 c2 = centers[ck];
  const int cy = c2.x, cx = c2.y;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  if (cy >= 0 && cy < H && cx >= 0 && cx < W) {                  // wave-uniform
    const int ylo = cy - R < 0 ? 0 : cy - R, yhi = cy + R > H - 1 ? H - 1 : cy + R;
    const int xlo = cx - R < 0 ? 0 : cx - R, xhi = cx + R > W - 1 ? W - 1 : cx + R;
    const long long* lb = labels + (size_t)b * H * W;
    for (int x0 = xlo; x0 <= xhi; x0 += 64) {
      const bool okx = x0 + lane <= xhi;
      const int x = okx ? x0 + lane : xhi;                        // clamped: the load is unconditional, the term is dropped
      const int dx2 = (x - cx) * (x - cx);
#pragma unroll 4
      for (int y = ylo; y <= yhi; ++y) {
        const long long v = lb[(size_t)y * W + x];
        const int d2 = (y - cy) * (y - cy) + dx2;
        const bool in = okx && d2 < nw;
        const double t = w[d2 < nw ? d2 : 0];
        const double term = in ? t : 0.0;
        const int c = class_of(v, s_lut);
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] += c == q ? term : 0.0;      // adding +0.0 leaves a non-negative sum unchanged
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] += __shfl_down(acc[c], off, 64);
  }
  if (lane == 0) {
    int best = 0;
    double top = -1.0;
#pragma unroll
    for (int c = 1; c < NC; ++c)
      if (acc[c] > top) {
        top = acc[c];
        best = c;
      }
    if (top < 1e-9) best = 0;
    double2* so = (double2*)(scores + ck * NC);
#pragma unroll
    for (int c = 0; c < NC; c += 2) so[c / 2] = make_double2(acc[c], acc[c + 1]);
    cls[ck] = best;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void prompt_make_kernel(const long long* __restrict__ labels, const uint8_t* __restrict__ lut,
                                                          const int2* __restrict__ centers, const int* __restrict__ cls,
                                                          const uint8_t* __restrict__ q, int nq, float* __restrict__ heat,
                                                          long long* __restrict__ target, int* __restrict__ classes,
                                                          int2* __restrict__ out_centers, uint8_t* __restrict__ valid, int K,
                                                          int PI, int H, int W, unsigned HW) {
  constexpr int PX = VEC ? 4 : 1;
  __shared__ uint8_t s_lut[256];
  __shared__ unsigned long long s_first[NC];           // per class: (first candidate << 30) | (cy << 15) | cx
  __shared__ int s_cy[NC], s_cx[NC];
  __shared__ int s_sel[MAXPI];                          // taken classes in candidate order (0: none)
  const int tid = threadIdx.x, b = blockIdx.y;
  // this thread's pixels: the loads are issued before the selection, which does not depend on them
  const unsigned p0r = (blockIdx.x * 256u + tid) * PX;
  const bool live = p0r < HW;
  const unsigned p0 = live ? p0r : HW - PX;
  const long long* lb = labels + (size_t)b * HW;
  long long lv[PX];
  if constexpr (VEC) {
    const longlong2 a0 = *(const longlong2*)(lb + p0), a1 = *(const longlong2*)(lb + p0 + 2);
    lv[0] = a0.x; lv[1] = a0.y; lv[2] = a1.x; lv[3] = a1.y;
  } else {
    lv[0] = lb[p0];
  }
  stage_lut(lut, q, s_lut);
  if (tid < NC) s_first[tid] = NOT_FOUND;
  __syncthreads();
  // first candidate of every class 1..7 whose centre lies inside the image (H, W <= 32768: a centre fits 2 x 15 bits)
  for (int k0 = 0; k0 < K; k0 += 1024) {
    int c[4];
    int2 ce[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * 256 + tid;
      const size_t i = (size_t)b * K + (k < K ? k : K - 1);
      c[u] = cls[i];
      ce[u] = centers[i];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * 256 + tid;
      const bool ok = k < K && c[u] >= 1 && c[u] < NC && ce[u].x >= 0 && ce[u].x < H && ce[u].y >= 0 && ce[u].y < W;
      if (ok) atomicMin(&s_first[c[u]], ((unsigned long long)k << 30) | ((unsigned long long)ce[u].x << 15) | (unsigned)ce[u].y);
    }
  }
  __syncthreads();
  if (tid == 0) {                                       // the PI classes with the smallest first index, in that order
    int used = 0, n = 0;
    for (int j = 0; j < MAXPI; ++j) {
      int best = 0;
      unsigned long long bk = NOT_FOUND;
      for (int cc = 1; cc < NC; ++cc)
        if (!((used >> cc) & 1) && s_first[cc] < bk) {
          bk = s_first[cc];
          best = cc;
        }
      if (j < PI && best) {
        used |= 1 << best;
        ++n;
        s_cy[best] = (int)((bk >> 15) & 32767);
        s_cx[best] = (int)(bk & 32767);
      }
      s_sel[j] = j < PI ? best : 0;
    }
    if (n < PI)
      for (int j = 0; j < MAXPI; ++j) s_sel[j] = 0;     // fewer distinct classes than asked for: the image is skipped
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < PI) {
    const int cj = s_sel[tid];
    classes[(size_t)b * PI + tid] = cj;
    out_centers[(size_t)b * PI + tid] = cj ? make_int2(s_cy[cj], s_cx[cj]) : make_int2(0, 0);
    if (tid == 0) valid[b] = cj ? 1 : 0;
  }
  if (!live) return;
  int cl[PX], y[PX], x[PX];
  y[0] = (int)(p0 / (unsigned)W);
  x[0] = (int)(p0 - (unsigned)y[0] * (unsigned)W);
#pragma unroll
  for (int e = 1; e < PX; ++e) {
    const bool wrap = x[e - 1] + 1 == W;
    x[e] = wrap ? 0 : x[e - 1] + 1;
    y[e] = wrap ? y[e - 1] + 1 : y[e - 1];
  }
#pragma unroll
  for (int e = 0; e < PX; ++e) cl[e] = class_of(lv[e], s_lut);
  for (int j = 0; j < PI; ++j) {
    const int cj = s_sel[j];
    const int cy = cj ? s_cy[cj] : 0, cx = cj ? s_cx[cj] : 0;     // inside the image: |dy|, |dx| < 32768, d2 < 2^31
    unsigned qv[PX];
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      const unsigned d2 = (unsigned)((y[e] - cy) * (y[e] - cy)) + (unsigned)((x[e] - cx) * (x[e] - cx));
      const bool in = cj && d2 < (unsigned)nq;
      const unsigned v = q[d2 < (unsigned)nq ? d2 : 0];
      qv[e] = in ? v : 0u;
    }
    const size_t o = ((size_t)b * PI + j) * HW + p0;
    if constexpr (VEC) {
      *(float4*)(heat + o) = make_float4((float)qv[0] / 255.0f, (float)qv[1] / 255.0f, (float)qv[2] / 255.0f,
                                         (float)qv[3] / 255.0f);
      longlong2 t0, t1;
      t0.x = cj && cl[0] == cj ? cj : 0; t0.y = cj && cl[1] == cj ? cj : 0;
      t1.x = cj && cl[2] == cj ? cj : 0; t1.y = cj && cl[3] == cj ? cj : 0;
      *(longlong2*)(target + o) = t0;
      *(longlong2*)(target + o + 2) = t1;
    } else {
      heat[o] = (float)qv[0] / 255.0f;
      target[o] = cj && cl[0] == cj ? cj : 0;
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void prompt_heatmap_kernel(const int2* __restrict__ points, int P, const uint8_t* __restrict__ q,
                                                             int nq, float* __restrict__ heat, int H, int W, unsigned HW) {
  constexpr int PX = VEC ? 4 : 1;
  __shared__ int2 s_pt[MAXPTS];
  const int tid = threadIdx.x;
  int2 pt[MAXPTS / 256];
#pragma unroll
  for (int u = 0; u < MAXPTS / 256; ++u) {              // P <= MAXPTS: clamped loads, all in flight together
    const int i = u * 256 + tid;
    pt[u] = points[i < P ? i : P - 1];
  }
#pragma unroll
  for (int u = 0; u < MAXPTS / 256; ++u) {
    const int i = u * 256 + tid;
    const bool in = pt[u].x >= 0 && pt[u].x < H && pt[u].y >= 0 && pt[u].y < W;
    if (i < P) s_pt[i] = in ? pt[u] : make_int2(-1, -1);     // a point outside the image contributes nothing
  }
  __syncthreads();
  const unsigned p0 = (blockIdx.x * 256u + tid) * PX;
  if (p0 >= HW) return;
  int y[PX], x[PX];
  unsigned best[PX];
  y[0] = (int)(p0 / (unsigned)W);
  x[0] = (int)(p0 - (unsigned)y[0] * (unsigned)W);
#pragma unroll
  for (int e = 1; e < PX; ++e) {
    const bool wrap = x[e - 1] + 1 == W;
    x[e] = wrap ? 0 : x[e - 1] + 1;
    y[e] = wrap ? y[e - 1] + 1 : y[e - 1];
  }
#pragma unroll
  for (int e = 0; e < PX; ++e) best[e] = 0xffffffffu;
  for (int i = 0; i < P; ++i) {
    const int2 p = s_pt[i];                             // wave-uniform address: a broadcast read
#pragma unroll
    for (int e = 0; e < PX; ++e) {
      const unsigned d2 = (unsigned)((y[e] - p.x) * (y[e] - p.x)) + (unsigned)((x[e] - p.y) * (x[e] - p.y));
      const unsigned d = p.x < 0 ? 0xffffffffu : d2;
      best[e] = d < best[e] ? d : best[e];
    }
  }
  float hv[PX];
#pragma unroll
  for (int e = 0; e < PX; ++e) {
    const bool in = best[e] < (unsigned)nq;
    const unsigned v = q[in ? best[e] : 0];
    hv[e] = (float)(in ? v : 0u) / 255.0f;
  }
  if constexpr (VEC)
    *(float4*)(heat + p0) = make_float4(hv[0], hv[1], hv[2], hv[3]);
  else
    heat[p0] = hv[0];
}

}  // namespace

// ------------------------------------------------------------------------------------------------
static int check_image(const char* what, int H, int W) {
  SEGK_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "%s: image %d x %d (sides 1..32768)", what, H, W);
  return 0;
}

extern "C" int segk_prompt_scores(const int64_t* labels, const uint8_t* lut, const int* centers, const double* w, int nw, int R,
                                  double* scores, int* cls, int B, int K, int H, int W, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(labels && centers && w && scores && cls, "prompt_scores: NULL pointer");
  SEGK_REQUIRE(B > 0 && B < 65536 && K > 0 && K <= (1 << 20), "prompt_scores: B=%d (1..65535), K=%d (1..2^20)", B, K);
  if (int rc = check_image("prompt_scores", H, W)) return rc;
  SEGK_REQUIRE(R >= 0 && R <= 4096 && nw > 0, "prompt_scores: R=%d (0..4096), nw=%d (> 0)", R, nw);
  SEGK_REQUIRE(((uintptr_t)labels & 7) == 0 && ((uintptr_t)centers & 7) == 0 && ((uintptr_t)w & 7) == 0 &&
               ((uintptr_t)scores & 15) == 0 && ((uintptr_t)cls & 3) == 0, "prompt_scores: misaligned buffer");
  hipLaunchKernelGGL(prompt_scores_kernel, dim3(cdiv(K, 4), B), dim3(256), 0, st, (const long long*)labels, lut, (const int2*)centers, w, nw, R,
                     scores, cls, K, H, W);
  SEGK_CHECK_LAUNCH("prompt_scores");
  return 0;
}

extern "C" int segk_prompt_make(const int64_t* labels, const uint8_t* lut, const int* centers, const int* cls, const uint8_t* q,
                                int nq, float* heat, int64_t* target, int* classes, int* out_centers, uint8_t* valid, int B,
                                int K, int per_image, int H, int W, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(labels && centers && cls && q && heat && target && classes && out_centers && valid, "prompt_make: NULL pointer");
  SEGK_REQUIRE(B > 0 && B < 65536 && K > 0 && K <= (1 << 20), "prompt_make: B=%d (1..65535), K=%d (1..2^20)", B, K);
  SEGK_REQUIRE(per_image >= 1 && per_image <= MAXPI, "prompt_make: per_image=%d (1..%d)", per_image, MAXPI);
  if (int rc = check_image("prompt_make", H, W)) return rc;
  SEGK_REQUIRE(nq > 0 && nq <= (1 << 30), "prompt_make: nq=%d", nq);
  const unsigned HW = (unsigned)H * (unsigned)W;
  const bool vec = HW % 4 == 0;
  SEGK_REQUIRE(((uintptr_t)labels & (vec ? 15 : 7)) == 0 && ((uintptr_t)target & (vec ? 15 : 7)) == 0 &&
               ((uintptr_t)heat & (vec ? 15 : 3)) == 0 && ((uintptr_t)centers & 7) == 0 && ((uintptr_t)out_centers & 7) == 0 &&
               ((uintptr_t)cls & 3) == 0 && ((uintptr_t)classes & 3) == 0, "prompt_make: misaligned buffer");
  const dim3 grid((HW / (vec ? 4 : 1) + 255) / 256, B);
  if (vec)
    hipLaunchKernelGGL(prompt_make_kernel<true>, grid, dim3(256), 0, st, (const long long*)labels, lut, (const int2*)centers, cls, q, nq, heat,
                       (long long*)target, classes, (int2*)out_centers, valid, K, per_image, H, W, HW);
  else
    hipLaunchKernelGGL(prompt_make_kernel<false>, grid, dim3(256), 0, st, (const long long*)labels, lut, (const int2*)centers, cls, q, nq, heat,
                       (long long*)target, classes, (int2*)out_centers, valid, K, per_image, H, W, HW);
  SEGK_CHECK_LAUNCH("prompt_make");
  return 0;
}

extern "C" int segk_prompt_heatmap(const int* points, int P, const uint8_t* q, int nq, float* heat, int H, int W,
                                   segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(points && q && heat, "prompt_heatmap: NULL pointer");
  SEGK_REQUIRE(P >= 1 && P <= MAXPTS, "prompt_heatmap: %d points (1..%d)", P, MAXPTS);
  if (int rc = check_image("prompt_heatmap", H, W)) return rc;
  SEGK_REQUIRE(nq > 0 && nq <= (1 << 30), "prompt_heatmap: nq=%d", nq);
  const unsigned HW = (unsigned)H * (unsigned)W;
  const bool vec = HW % 4 == 0;
  SEGK_REQUIRE(((uintptr_t)points & 7) == 0 && ((uintptr_t)heat & (vec ? 15 : 3)) == 0, "prompt_heatmap: misaligned buffer");
  const dim3 grid((HW / (vec ? 4 : 1) + 255) / 256);
  if (vec)
    hipLaunchKernelGGL(prompt_heatmap_kernel<true>, grid, dim3(256), 0, st, (const int2*)points, P, q, nq, heat, H, W, HW);
  else
    hipLaunchKernelGGL(prompt_heatmap_kernel<false>, grid, dim3(256), 0, st, (const int2*)points, P, q, nq, heat, H, W, HW);
  SEGK_CHECK_LAUNCH("prompt_heatmap");
  return 0;
}
