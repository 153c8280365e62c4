// Training augmentation and dataset preparation on the device (reference utils/augmentation.ipynb: the eight imgaug
// augmenters each followed by "pad to square, resize to 256", the pair merge of cell 17 and convert_rgb_label_to_classes;
// utils/utils.py:117-198 calculate_class_weights, utils/utils.py:201-250 convert_rgb_label_to_classes).
//
// Every value that decides a result is an INTEGER: the host builds the tables (cubic taps and 11-bit coefficients, contrast
// LUT, Laplace inverse CDF, Q16 rotation matrix, PIL-NEAREST index tables) and the kernels combine them with integer
// arithmetic only, so two runs -- and the NumPy restatement of tests/augment_reference.py -- give the same bytes.
//
//  aug_prefilter_kernel   stage A of the samples that need one, a 16x16 output tile per workgroup: rotation (bilinear gather
//                         of the image with 8-bit fractions, nearest gather of the label) or the 12x12 box blur (a 27x27 input
//                         tile in LDS, a horizontal 12-sum, then a vertical 12-sum: 24 LDS reads per pixel and channel).
//  aug_resample_kernel    stage B of every sample: window -> pointwise op on each tap -> pad to square -> separable cubic
//                         resize of the image / nearest resize of the label to T x T; one thread per output pixel, the 16 taps
//                         of a pixel are loaded before any is used.
//  aug_merge_kernel       cell 17 for a batch of pairs: four per-axis index tables per pair say which source pixel, if any,
//                         lands on a canvas pixel.
//  label_hist_kernel      class counts: LDS histogram per workgroup, then one 64-bit atomic add per class and workgroup.
//  rgb_label_kernel       convert_rgb_label_to_classes.
//
// The descriptor tables are device data the entry points cannot see: every coordinate is clamped to its buffer and every table
// row to the table length before it is used as an address, and an unknown op code is treated as a plain resize.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int OP_ROTATION = SEGK_AUG_ROTATION, OP_MASKING = SEGK_AUG_MASKING, OP_GRAYSCALE = SEGK_AUG_GRAYSCALE,
              OP_LAPLACE = SEGK_AUG_LAPLACE, OP_BLUR = SEGK_AUG_BLUR, OP_CONTRAST = SEGK_AUG_CONTRAST;
constexpr int LAP_N = SEGK_AUG_LAPLACE_ENTRIES;
constexpr unsigned DROP_BELOW = 2516582u;          // floor(0.15 * 2^24)

// utils/utils.py:201-250: black or white -> 0, (128,0,0) -> 1, (0,128,0) -> 2, else 255
__device__ __forceinline__ int rgb_class(int r, int g, int b) {
  const int p = (r << 16) | (g << 8) | b;
  return p == 0 || p == 0xffffff ? 0 : p == 0x800000 ? 1 : p == 0x008000 ? 2 : 255;
}

// one label pixel as a class id / trimap value: lc == 3 colour labels go through rgb_class
__device__ __forceinline__ int label_at(const uint8_t* __restrict__ lab, size_t pix, int lc) {
  if (lc == 3) {
    const uint8_t* p = lab + pix * 3;
    return rgb_class(p[0], p[1], p[2]);
  }
  return lab[pix];
}

// CoarseDropout cell of a source pixel: dropped iff the top 24 bits of the cell's hash are below 0.15 * 2^24
__device__ __forceinline__ bool dropped(const segk_aug_desc& d, int y, int x) {
  const int cy = (int)(((long long)y * d.gh) / d.H), cx = (int)(((long long)x * d.gw) / d.W);
  return (unsigned)(splitmix(d.seed, (unsigned long long)((long long)cy * d.gw + cx)) >> 40) < DROP_BELOW;
}

// ------------------------------------------------------------------------------------------------ stage A
__global__ __launch_bounds__(256) void aug_prefilter_kernel(const segk_aug_desc* __restrict__ descs) {
  __shared__ uint8_t s_in[27][84];
  __shared__ uint16_t s_h[27][48];
  const segk_aug_desc& d = descs[blockIdx.y];
  const int Ha = d.Ha, Wa = d.Wa, H = d.H, W = d.W;
  if (Ha < 1 || Wa < 1 || H < 1 || W < 1 || !d.img || !d.a_img) return;
  const int tiles_x = (Wa + 15) >> 4, tiles_y = (Ha + 15) >> 4;
  if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
  const int x = tx * 16 + lx, y = ty * 16 + ly;
  const bool live = x < Wa && y < Ha;
  const int ic = d.img_c == 4 ? 4 : 3;
  const uint8_t* __restrict__ img = d.img;
  uint8_t* __restrict__ out = d.a_img;
  if (d.op == OP_BLUR) {                                  // block-uniform; Ha == H, Wa == W
    const int y0 = ty * 16 - 6, x0 = tx * 16 - 6;
    int v[3][3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {                         // 729 input pixels: clamped loads, all in flight together
      const int e = u * 256 + tid, ec = e < 729 ? e : 728;
      const int r = ec / 27, c = ec - r * 27;
      const uint8_t* p = img + ((size_t)reflect101(y0 + r, H) * W + reflect101(x0 + c, W)) * ic;
      v[u][0] = p[0]; v[u][1] = p[1]; v[u][2] = p[2];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int e = u * 256 + tid;
      if (e < 729) {
        const int r = e / 27, c = e - r * 27;
        s_in[r][c * 3] = (uint8_t)v[u][0]; s_in[r][c * 3 + 1] = (uint8_t)v[u][1]; s_in[r][c * 3 + 2] = (uint8_t)v[u][2];
      }
    }
    __syncthreads();
    for (int e = tid; e < 27 * 48; e += 256) {            // horizontal 12-sums of the 16 columns x 3 channels
      const int r = e / 48, q = e - r * 48;
      int s = 0;
#pragma unroll
      for (int k = 0; k < 12; ++k) s += s_in[r][q + 3 * k];
      s_h[r][q] = (uint16_t)s;
    }
    __syncthreads();
    if (live) {
      uint8_t* o = out + ((size_t)y * Wa + x) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) s += s_h[ly + k][lx * 3 + ch];
        o[ch] = (uint8_t)((s + 72) / 144);
      }
    }
    return;
  }
  if (d.op != OP_ROTATION || !live) return;
  const long long SX = d.A[0] * x + d.A[1] * y + d.A[2], SY = d.A[3] * x + d.A[4] * y + d.A[5];
  const long long ixl = SX >> 16, iyl = SY >> 16;
  const int ix = (int)(ixl < -2 ? -2 : ixl > W ? W : ixl), iy = (int)(iyl < -2 ? -2 : iyl > H ? H : iyl);
  const int fx = (int)((SX >> 8) & 255), fy = (int)((SY >> 8) & 255);
  const int wgt[4] = {(256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy};   // sum 65536
  int pix[4][3];
#pragma unroll
  for (int t = 0; t < 4; ++t) {                           // clamped addresses: the loads are unconditional
    const int yy = iy + (t >> 1), xx = ix + (t & 1);
    const uint8_t* p = img + ((size_t)clampi(yy, 0, H - 1) * W + clampi(xx, 0, W - 1)) * ic;
    pix[t][0] = p[0]; pix[t][1] = p[1]; pix[t][2] = p[2];
  }
  int acc[3] = {32768, 32768, 32768};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int yy = iy + (t >> 1), xx = ix + (t & 1);
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;             // a tap outside the source reads 0
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += in ? wgt[t] * pix[t][ch] : 0;
  }
  uint8_t* o = out + ((size_t)y * Wa + x) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = (uint8_t)(acc[ch] >> 16);
  if (d.lab && d.a_lab) {
    const long long nxl = (SX + 32768) >> 16, nyl = (SY + 32768) >> 16;
    const bool in = nxl >= 0 && nxl < W && nyl >= 0 && nyl < H;
    const int nx = (int)(nxl < 0 ? 0 : nxl > W - 1 ? W - 1 : nxl), ny = (int)(nyl < 0 ? 0 : nyl > H - 1 ? H - 1 : nyl);
    const int v = label_at(d.lab, (size_t)ny * W + nx, d.lab_c);
    d.a_lab[(size_t)y * Wa + x] = (uint8_t)(in ? v : d.label_fill);
  }
}

// ------------------------------------------------------------------------------------------------ stage B
__global__ __launch_bounds__(256) void aug_resample_kernel(const segk_aug_desc* __restrict__ descs, int T,
                                                           const int* __restrict__ cidx, const short* __restrict__ ccoef,
                                                           int n_cub, const uint8_t* __restrict__ contrast, int n_con,
                                                           const short* __restrict__ laplace, int n_lap,
                                                           const uint8_t* __restrict__ lut, float* __restrict__ X,
                                                           uint8_t* __restrict__ X8, long long* __restrict__ Y) {
  __shared__ uint8_t s_con[256];
  __shared__ short s_lap[LAP_N];
  const segk_aug_desc& d = descs[blockIdx.y];
  const int tid = threadIdx.x;
  const int op = d.op;
  const bool has_a = d.a_img != nullptr;
  const uint8_t* __restrict__ img = has_a ? d.a_img : d.img;
  const int ic = has_a ? 3 : (d.img_c == 4 ? 4 : 3);
  const bool lab_a = d.a_lab != nullptr;
  const uint8_t* __restrict__ lab = lab_a ? d.a_lab : d.lab;
  const int lc = lab_a ? 1 : (d.lab_c == 3 ? 3 : 1);
  const int Hb = has_a || lab_a ? d.Ha : d.H, Wb = has_a || lab_a ? d.Wa : d.W;      // the stage-B input
  if (Hb < 1 || Wb < 1 || !img) return;
  const int wh = clampi(d.wh, 1, Hb), ww = clampi(d.ww, 1, Wb);
  const int wy = clampi(d.wy, 0, Hb - wh), wx = clampi(d.wx, 0, Wb - ww);
  const int S = wh > ww ? wh : ww, py = (S - wh) / 2, px = (S - ww) / 2;
  const bool use_con = op == OP_CONTRAST && n_con > 0, use_lap = op == OP_LAPLACE && n_lap > 0;
  const bool use_mask = op == OP_MASKING && d.gh > 0 && d.gw > 0 && d.H == Hb && d.W == Wb;
  if (use_con) s_con[tid] = contrast[(size_t)clampi(d.aux, 0, n_con - 1) * 256 + tid];
  if (use_lap) {
    const unsigned* src = (const unsigned*)(laplace + (size_t)clampi(d.aux, 0, n_lap - 1) * LAP_N);
    unsigned w[LAP_N / 512];
#pragma unroll
    for (int u = 0; u < LAP_N / 512; ++u) w[u] = src[u * 256 + tid];
#pragma unroll
    for (int u = 0; u < LAP_N / 512; ++u) ((unsigned*)s_lap)[u * 256 + tid] = w[u];
  }
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p >= T * T) return;
  const int oy = p / T, ox = p - oy * T;
  const size_t TT = (size_t)T * T, b = blockIdx.y;

  if (Y && lab) {                                        // label: nearest, src = (dst * S) / T in the padded square
    const int sy = (int)(((long long)oy * S) / T) - py, sx = (int)(((long long)ox * S) / T) - px;
    const bool in = sy >= 0 && sy < wh && sx >= 0 && sx < ww;
    const int yy = wy + clampi(sy, 0, wh - 1), xx = wx + clampi(sx, 0, ww - 1);
    int v = label_at(lab, (size_t)yy * Wb + xx, lc);
    if (use_mask) v = dropped(d, yy, xx) ? 0 : v;
    v = in ? v : 0;
    const int m = lut ? lut[v] : v;
    Y[b * TT + p] = m;
  }

  const int t = clampi(d.tab, 0, n_cub - 1);
  const int iy = cidx[(size_t)t * T + oy], ix = cidx[(size_t)t * T + ox];
  const short4 cy4 = *(const short4*)(ccoef + ((size_t)t * T + oy) * 4), cx4 = *(const short4*)(ccoef + ((size_t)t * T + ox) * 4);
  const int cy[4] = {cy4.x, cy4.y, cy4.z, cy4.w}, cx[4] = {cx4.x, cx4.y, cx4.z, cx4.w};
  int yy[4], xx[4];
  bool iny[4], inx[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int sy = clampi(iy - 1 + r, 0, S - 1) - py, sx = clampi(ix - 1 + r, 0, S - 1) - px;
    iny[r] = sy >= 0 && sy < wh;
    inx[r] = sx >= 0 && sx < ww;
    yy[r] = wy + clampi(sy, 0, wh - 1);
    xx[r] = wx + clampi(sx, 0, ww - 1);
  }
  int v[4][4][3];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {                        // 16 taps, clamped addresses, all in flight together
      const uint8_t* q = img + ((size_t)yy[r] * Wb + xx[c]) * ic;
      v[r][c][0] = q[0]; v[r][c][1] = q[1]; v[r][c][2] = q[2];
    }
  long long acc[3] = {0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int h[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int R = v[r][c][0], G = v[r][c][1], B = v[r][c][2];
      if (op == OP_GRAYSCALE) {
        R = G = B = (4899 * R + 9617 * G + 1868 * B + 8192) >> 14;
      } else if (use_con) {
        R = s_con[R]; G = s_con[G]; B = s_con[B];
      } else if (use_lap) {
        const unsigned long long i0 = ((unsigned long long)yy[r] * (unsigned)Wb + (unsigned)xx[c]) * 3ULL;
        R = clampi(R + s_lap[splitmix(d.seed, i0) >> 52], 0, 255);
        G = clampi(G + s_lap[splitmix(d.seed, i0 + 1) >> 52], 0, 255);
        B = clampi(B + s_lap[splitmix(d.seed, i0 + 2) >> 52], 0, 255);
      } else if (use_mask) {
        if (dropped(d, yy[r], xx[c])) R = G = B = 0;
      }
      const bool in = iny[r] && inx[c];                  // the pad is added after the augmenter: it stays 0
      h[0] += in ? cx[c] * R : 0;
      h[1] += in ? cx[c] * G : 0;
      h[2] += in ? cx[c] * B : 0;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += (long long)cy[r] * h[ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long long s = (acc[ch] + (1LL << 21)) >> 22;
    const int o = (int)(s < 0 ? 0 : s > 255 ? 255 : s);
    if (X) X[(b * 3 + ch) * TT + p] = (float)o / 255.0f;            // utils/dataset.py:39
    if (X8) X8[(b * TT + p) * 3 + ch] = (uint8_t)o;
  }
}

// ------------------------------------------------------------------------------------------------ merge (cell 17)
__global__ __launch_bounds__(256) void aug_merge_kernel(const segk_merge_desc* __restrict__ descs, const int* __restrict__ tab,
                                                        int T, const uint8_t* __restrict__ lut, float* __restrict__ X,
                                                        uint8_t* __restrict__ X8, long long* __restrict__ Y) {
  const segk_merge_desc& d = descs[blockIdx.y];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= T * T || !d.img[0] || !d.img[1] || d.H[0] < 1 || d.W[0] < 1 || d.H[1] < 1 || d.W[1] < 1) return;
  const int oy = p / T, ox = p - oy * T;
  const size_t TT = (size_t)T * T, b = blockIdx.y;
  const int* tb = tab + b * 4 * (size_t)T;
  int sy[2], sx[2];
  sy[0] = tb[oy]; sx[0] = tb[T + ox]; sy[1] = tb[2 * T + oy]; sx[1] = tb[3 * T + ox];
  int rgb[2][3], lv[2][3];
  bool hit[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {                          // both sources are read (clamped); the later paste wins
    const int H = d.H[k], W = d.W[k];
    hit[k] = sy[k] >= 0 && sy[k] < H && sx[k] >= 0 && sx[k] < W && d.img[k] != nullptr;
    const size_t pix = (size_t)clampi(sy[k], 0, H - 1) * W + clampi(sx[k], 0, W - 1);
    const uint8_t* q = d.img[k] + pix * (d.img_c[k] == 4 ? 4 : 3);
    rgb[k][0] = q[0]; rgb[k][1] = q[1]; rgb[k][2] = q[2];
    lv[k][0] = lv[k][1] = lv[k][2] = 0;
    if (Y && d.lab[k]) {
      if (d.lab_c[k] == 3) {
        const uint8_t* l = d.lab[k] + pix * 3;
        lv[k][0] = l[0]; lv[k][1] = l[1]; lv[k][2] = l[2];
      } else {
        lv[k][0] = lv[k][1] = lv[k][2] = d.lab[k][pix];   // a one-channel file is loaded as grey RGB
      }
    }
  }
  const int k = hit[1] ? 1 : 0;
  const bool any = hit[0] || hit[1];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int o = any ? rgb[k][ch] : 0;
    if (X) X[(b * 3 + ch) * TT + p] = (float)o / 255.0f;
    if (X8) X8[(b * TT + p) * 3 + ch] = (uint8_t)o;
  }
  if (Y) {
    const int c = any ? rgb_class(lv[k][0], lv[k][1], lv[k][2]) : 0;
    Y[b * TT + p] = lut ? lut[c] : c;
  }
}

// ------------------------------------------------------------------------------------------------ class counts
template <typename L>
__global__ __launch_bounds__(256) void label_hist_kernel(const L* __restrict__ labels, long long n, int C, int has_ignore,
                                                         long long ignore, unsigned long long* __restrict__ counts) {
  __shared__ unsigned s_hist[256];
  const int tid = threadIdx.x;
  s_hist[tid] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i0 = ((long long)blockIdx.x * 256 + tid) * 4; i0 < n; i0 += stride) {
    long long v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (long long)labels[i0 + e < n ? i0 + e : n - 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = i0 + e < n && !(has_ignore && v[e] == ignore);    // utils.py:168-173: drop, then clamp
      const int c = (int)(v[e] < 0 ? 0 : v[e] > C - 1 ? C - 1 : v[e]);
      if (ok) atomicAdd(&s_hist[c], 1u);
    }
  }
  __syncthreads();
  if (tid < C && s_hist[tid]) atomicAdd(&counts[tid], (unsigned long long)s_hist[tid]);
}

__global__ __launch_bounds__(256) void rgb_label_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = rgb + i * 3;
  out[i] = (uint8_t)rgb_class(p[0], p[1], p[2]);
}

}  // namespace

// ------------------------------------------------------------------------------------------------
static_assert(sizeof(segk_aug_desc) == 160, "segk_aug_desc is 160 bytes");
static_assert(sizeof(segk_merge_desc) == 64, "segk_merge_desc is 64 bytes");

static int check_batch(const char* what, const void* descs, int n, int T) {
  SEGK_REQUIRE(descs, "%s: NULL descriptor table", what);
  SEGK_REQUIRE(((uintptr_t)descs & 7) == 0, "%s: misaligned descriptor table", what);
  SEGK_REQUIRE(n >= 1 && n <= 65535, "%s: %d samples (1..65535)", what, n);
  SEGK_REQUIRE(T >= 1 && T <= 4096, "%s: target size %d (1..4096)", what, T);
  return 0;
}

extern "C" int segk_aug_prefilter(const segk_aug_desc* descs, int n, int max_tiles, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (int rc = check_batch("aug_prefilter", descs, n, 1)) return rc;
  // a rotated 8192 x 8192 image has sides of at most 11586: 725^2 tiles of 16 x 16
  SEGK_REQUIRE(max_tiles >= 1 && max_tiles <= 725 * 725, "aug_prefilter: max_tiles=%d (1..%d)", max_tiles, 725 * 725);
  hipLaunchKernelGGL(aug_prefilter_kernel, dim3(max_tiles, n), dim3(256), 0, st, descs);
  SEGK_CHECK_LAUNCH("aug_prefilter");
  return 0;
}

extern "C" int segk_aug_resample(const segk_aug_desc* descs, int n, int T, const int32_t* cub_idx, const int16_t* cub_coef,
                                 int n_cub, const uint8_t* contrast, int n_contrast, const int16_t* laplace, int n_laplace,
                                 const uint8_t* label_lut, float* X, uint8_t* X8, int64_t* y, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (int rc = check_batch("aug_resample", descs, n, T)) return rc;
  SEGK_REQUIRE(cub_idx && cub_coef && n_cub >= 1 && n_cub <= 65535, "aug_resample: cubic tables (NULL, or %d rows: 1..65535)", n_cub);
  SEGK_REQUIRE(n_contrast >= 0 && n_contrast <= 65535 && (n_contrast == 0 || contrast),
               "aug_resample: %d contrast tables (0..65535) need a table pointer", n_contrast);
  SEGK_REQUIRE(n_laplace >= 0 && n_laplace <= 65535 && (n_laplace == 0 || laplace),
               "aug_resample: %d Laplace tables (0..65535) need a table pointer", n_laplace);
  SEGK_REQUIRE(X || X8, "aug_resample: no image output (X and X8 are NULL)");
  SEGK_REQUIRE(((uintptr_t)cub_idx & 3) == 0 && ((uintptr_t)cub_coef & 7) == 0 && ((uintptr_t)laplace & 3) == 0 &&
               ((uintptr_t)X & 3) == 0 && ((uintptr_t)y & 7) == 0, "aug_resample: misaligned buffer");
  hipLaunchKernelGGL(aug_resample_kernel, dim3(cdiv(T * T, 256), n), dim3(256), 0, st, descs, T, cub_idx, cub_coef, n_cub,
                     contrast, n_contrast, laplace, n_laplace, label_lut, X, X8, (long long*)y);
  SEGK_CHECK_LAUNCH("aug_resample");
  return 0;
}

extern "C" int segk_aug_merge(const segk_merge_desc* descs, const int32_t* tables, int n, int T, const uint8_t* label_lut,
                              float* X, uint8_t* X8, int64_t* y, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (int rc = check_batch("aug_merge", descs, n, T)) return rc;
  SEGK_REQUIRE(tables && ((uintptr_t)tables & 3) == 0, "aug_merge: NULL or misaligned index tables");
  SEGK_REQUIRE(X || X8, "aug_merge: no image output (X and X8 are NULL)");
  SEGK_REQUIRE(((uintptr_t)X & 3) == 0 && ((uintptr_t)y & 7) == 0, "aug_merge: misaligned buffer");
  hipLaunchKernelGGL(aug_merge_kernel, dim3(cdiv(T * T, 256), n), dim3(256), 0, st, descs, tables, T, label_lut, X, X8, (long long*)y);
  SEGK_CHECK_LAUNCH("aug_merge");
  return 0;
}

extern "C" int segk_label_hist(const void* labels, long n, int elem_bytes, int num_classes, int has_ignore, long ignore_index,
                               uint64_t* counts, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(labels && counts, "label_hist: NULL pointer");
  SEGK_REQUIRE(n >= 1 && n <= (1L << 40), "label_hist: n=%ld (1..2^40)", n);
  SEGK_REQUIRE(elem_bytes == 1 || elem_bytes == 8, "label_hist: labels of %d bytes (uint8: 1, int64: 8)", elem_bytes);
  SEGK_REQUIRE(num_classes >= 1 && num_classes <= 256, "label_hist: %d classes (1..256)", num_classes);
  SEGK_REQUIRE(has_ignore == 0 || has_ignore == 1, "label_hist: has_ignore=%d (0 | 1)", has_ignore);
  SEGK_REQUIRE(((uintptr_t)counts & 7) == 0 && ((uintptr_t)labels & (elem_bytes - 1)) == 0, "label_hist: misaligned buffer");
  const long want = (n + 4095) / 4096;                   // 16 labels per thread and pass; at most 2^30 labels per workgroup
  const int blocks = (int)(want < 1024 ? want : 1024);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(label_hist_kernel<uint8_t>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)labels, (long long)n,
                       num_classes, has_ignore, (long long)ignore_index, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(label_hist_kernel<long long>, dim3(blocks), dim3(256), 0, st, (const long long*)labels, (long long)n,
                       num_classes, has_ignore, (long long)ignore_index, (unsigned long long*)counts);
  SEGK_CHECK_LAUNCH("label_hist");
  return 0;
}

extern "C" int segk_rgb_label_to_classes(const uint8_t* rgb, uint8_t* out, long n, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(rgb && out, "rgb_label_to_classes: NULL pointer");
  SEGK_REQUIRE(n >= 1 && n <= (1L << 38), "rgb_label_to_classes: n=%ld pixels (1..2^38)", n);
  hipLaunchKernelGGL(rgb_label_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rgb, out, (long long)n);
  SEGK_CHECK_LAUNCH("rgb_label_to_classes");
  return 0;
}
