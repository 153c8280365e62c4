// BatchNorm2d (train/eval) finalisation, BN+ReLU apply, BN backward reductions, MaxPool2d(2,2) forward/backward on NHWC
// tensors.  HBM-bound streaming kernels: every thread owns one 16-byte channel vector (fixed channels -> per-channel constants
// live in registers) and walks pixels, so a row of threads reads/writes whole contiguous pixel rows (coalesced 16 B per lane).
// The lane map, the pixel walk, the block row reduce, the float64 sum of partial rows, the statistics finish and the 2x2 window
// are stated once, in channel_lanes.hpp.
//
// Reference semantics: torch.nn.BatchNorm2d as instantiated at unet/unet.py:17,20 and
// clip/clipunet.py:88,91 (eps 1e-5, momentum 0.1, biased variance to normalise, unbiased variance into
// running_var), nn.ReLU, nn.MaxPool2d(2,2) at unet.py:40 (backward routes to the first maximum in
// row-major window order).
#include <atomic>
#include "channel_lanes.hpp"
#include "segk_internal.h"
#include "ticket.hpp"
#include "../../include/segk.h"

namespace {
__device__ unsigned g_tickets[TICKET_SLOTS * TICKET_GROUPS];     // zeroed per launch by the host (ticket.hpp)

// ---------------------------------------------------------------------------------------------
constexpr int NCH = 32;   // first-stage chunks of the per-tile statistics reduction
// stage A: per-tile partials [MT][C][2] float -> [NCH][C][2] double (fixed order inside a chunk: bit-stable)
__device__ __forceinline__ void stats_chunk(const float* __restrict__ part, int MT, int C, double* __restrict__ out,
                                            double (&sh)[8][32][2]) {
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  const int chunk = (MT + NCH - 1) / NCH;
  const int m0 = blockIdx.y * chunk, m1 = min(MT, m0 + chunk);
  double s1 = 0.0, s2 = 0.0;
  for (int m = m0 + ry; m < m1; m += 8) {
    const float2 v = ((const float2*)part)[(size_t)m * C + c];
    s1 += (double)v.x;
    s2 += (double)v.y;
  }
  sh[ry][cx][0] = s1;
  sh[ry][cx][1] = s2;
  __syncthreads();
  if (ry == 0) {
    s1 = 0.0; s2 = 0.0;
    for (int r = 0; r < 8; ++r) { s1 += sh[r][cx][0]; s2 += sh[r][cx][1]; }
    out[((size_t)blockIdx.y * C + c) * 2 + 0] = s1;
    out[((size_t)blockIdx.y * C + c) * 2 + 1] = s2;
  }
}

// stage B: [MT][C][2] double partials -> scale/shift (+ running stats) for the 32 channels of blockIdx.x
__device__ __forceinline__ void finalize_channels(const double* __restrict__ part, int MT, int C, int C_real,
                                                  double count, const float* conv_bias,
                                                  const float* gamma, const float* beta, float* rmean,
                                                  float* rvar, float momentum, float eps, int training,
                                                  float* scale, float* shift, float* mean_out,
                                                  float* rstd_out, double (&sh)[8][32][2]) {
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx;
  double s1 = 0.0, s2 = 0.0;
  if (training && c < C)
    for (int m = ry; m < MT; m += 8) {
      s1 += part[((size_t)m * C + c) * 2 + 0];
      s2 += part[((size_t)m * C + c) * 2 + 1];
    }
  sh[ry][cx][0] = s1;
  sh[ry][cx][1] = s2;
  __syncthreads();
  if (ry != 0 || c >= C) return;
  if (c >= C_real) return bn_channel_zero(c, scale, shift, mean_out, rstd_out);
  const float g = gamma[c], be = beta[c];
  const float cb = conv_bias ? conv_bias[c] : 0.f;
  if (training) {
    s1 = 0.0; s2 = 0.0;
    for (int r = 0; r < 8; ++r) { s1 += sh[r][cx][0]; s2 += sh[r][cx][1]; }
    return bn_channel_finish(s1, s2, count, c, g, be, cb, rmean, rvar, momentum, eps, scale, shift, mean_out, rstd_out);
  }
  const float rstd = 1.f / sqrtf(rvar[c] + eps);
  const float sc = g * rstd;
  scale[c] = sc;
  shift[c] = be + (cb - rmean[c]) * sc;
  if (mean_out) { mean_out[c] = rmean[c] - cb; rstd_out[c] = rstd; }
}

// eval mode (no statistics to reduce): stage B alone
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ part, int MT, int C, int C_real,
                                                          double count, const float* conv_bias,
                                                          const float* gamma, const float* beta, float* rmean,
                                                          float* rvar, float momentum, float eps, int training,
                                                          float* scale, float* shift, float* mean_out,
                                                          float* rstd_out) {
  __shared__ double sh[8][32][2];
  finalize_channels(part, MT, C, C_real, count, conv_bias, gamma, beta, rmean, rvar, momentum, eps, training, scale, shift,
                    mean_out, rstd_out, sh);
}

// training mode, few partial rows (MT <= 1024: every layer but the 128-channel ones at 128x128 and above): one block of
// 32 row lanes x 32 channels walks all rows itself (sum_rows16) and finishes -- no second stage at all
__global__ __launch_bounds__(1024) void bn_stats_finalize_small_kernel(const float* __restrict__ part, int MT, int C,
                                                                       int C_real, double count, const float* conv_bias,
                                                                       const float* gamma, const float* beta, float* rmean,
                                                                       float* rvar, float momentum, float eps, float* scale,
                                                                       float* shift, float* mean_out, float* rstd_out) {
  double s[2];
  if (!sum_rows16<2>(part, MT, C, s)) return;
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  if (c >= C_real) return bn_channel_zero(c, scale, shift, mean_out, rstd_out);
  bn_channel_finish(s[0], s[1], count, c, gamma[c], beta[c], conv_bias ? conv_bias[c] : 0.f, rmean, rvar, momentum, eps, scale, shift,
                    mean_out, rstd_out);
}

// training mode, ONE launch: grid (C/32, NCH) blocks reduce their chunk of the per-tile partials (stage A); the block that
// arrives last for a channel group finishes it (stage B over the NCH chunk sums, in chunk order: bit-stable)
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const float* __restrict__ part, int MT, int C, int C_real,
                                                                double count, const float* conv_bias,
                                                                const float* gamma, const float* beta, float* rmean,
                                                                float* rvar, float momentum, float eps,
                                                                float* scale, float* shift, float* mean_out,
                                                                float* rstd_out, double* __restrict__ scratch,
                                                                unsigned* __restrict__ tickets) {
  __shared__ double sh[8][32][2];
  __shared__ int last;
  stats_chunk(part, MT, C, scratch, sh);
  if (!last_arriver(tickets + blockIdx.x, gridDim.y, &last)) return;
  finalize_channels(scratch, (int)gridDim.y, C, C_real, count, conv_bias, gamma, beta, rmean, rvar, momentum, eps, 1, scale,
                    shift, mean_out, rstd_out, sh);
}

// ---------------------------------------------------------------------------------------------
// y = relu(z*scale + shift)
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const T* __restrict__ z, T* __restrict__ y,
                                                            const float* scale, const float* shift, long P, int C,
                                                            int cvb, int rows) {
  using E = ET<T>;
  const ChannelLanes l = channel_lanes(cvb, rows, C / E::VEC);
  if (!l.active()) return;
  float sc[E::VEC], sh[E::VEC];
#pragma unroll
  for (int j = 0; j < E::VEC; ++j) { sc[j] = scale[l.cv * E::VEC + j]; sh[j] = shift[l.cv * E::VEC + j]; }
  const size_t cofs = (size_t)l.cv * E::VEC;
  walk_pixels<APPLY_FLIGHT>((long)blockIdx.x * rows + l.ry, (long)gridDim.x * rows, P,
                            [&](long p) { return *(const uint4*)(z + (size_t)p * C + cofs); },
                            [&](long p, const uint4 raw) {
                              float f[E::VEC];
                              unpack16<T>(raw, f);
#pragma unroll
                              for (int j = 0; j < E::VEC; ++j) f[j] = fmaxf(fmaf(f[j], sc[j], sh[j]), 0.f);
                              *(uint4*)(y + (size_t)p * C + cofs) = pack16<T>(f);
                            });
}

// ---------------------------------------------------------------------------------------------
struct ZD { uint4 z, d; };   // one pixel of the backward passes: the channel vectors of z and dy
// BN backward pass 1: g = dy * [z*scale+shift > 0];  partial sums of g and g*xhat per channel.
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ z,
                                                            const float* scale, const float* shift,
                                                            const float* mean, const float* rstd, long P, int C,
                                                            int cvb, int rows, float* part) {
  using E = ET<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [rows][cvb][2*VEC]
  const ChannelLanes l = channel_lanes(cvb, rows, C / E::VEC);
  float s[2 * E::VEC];                                          // sum g, then sum g * xhat
#pragma unroll
  for (int j = 0; j < 2 * E::VEC; ++j) s[j] = 0.f;
  if (l.active()) {
    const BnConsts<E::VEC> k(scale, shift, mean, rstd, l.cv * E::VEC);
    const size_t cofs = (size_t)l.cv * E::VEC;
    // pixels are consumed in the order of a one-pixel walk: bit-identical sums
    walk_pixels<REDUCE_FLIGHT>((long)blockIdx.x * rows + l.ry, (long)gridDim.x * rows, P,
                               [&](long p) {
                                 const size_t off = (size_t)p * C + cofs;
                                 return ZD{*(const uint4*)(z + off), *(const uint4*)(dy + off)};
                               },
                               [&](long, const ZD& v) {
                                 float fz[E::VEC], fd[E::VEC];
                                 unpack16<T>(v.z, fz);
                                 unpack16<T>(v.d, fd);
#pragma unroll
                                 for (int j = 0; j < E::VEC; ++j) {
                                   const float g = (fmaf(fz[j], k.sc[j], k.sh[j]) > 0.f) ? fd[j] : 0.f;
                                   s[j] += g;
                                   s[E::VEC + j] = fmaf(g, (fz[j] - k.mu[j]) * k.rs[j], s[E::VEC + j]);
                                 }
                               });
  }
  reduce_lane_rows(reinterpret_cast<float*>(smem), l, cvb, rows, 2 * E::VEC, s, [&](const float (&tot)[2 * E::VEC]) {
    float2* dst = (float2*)part + (size_t)blockIdx.x * C + l.cv * E::VEC;
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) dst[j] = make_float2(tot[j], tot[E::VEC + j]);
  });
}

// partials [NB][C][2] -> dgamma, dbeta, coef = (sum_g/N, sum_gx/N); NB <= 512 (segk_bn_bwd_blocks) is ONE memory round trip
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ part, int NB, int C,
                                                               int C_real, double count, float* dgamma, float* dbeta,
                                                               float* coef) {
  double s[2];
  if (!sum_rows16<2>(part, NB, C, s)) return;
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  if (c < C_real) { dbeta[c] = (float)s[0]; dgamma[c] = (float)s[1]; }
  coef[2 * c] = (float)(s[0] / count);
  coef[2 * c + 1] = (float)(s[1] / count);
}

// BN backward pass 2 (in place allowed): dz = scale * (g - c1 - xhat*c2)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ z,
                                                           T* __restrict__ dz, const float* scale,
                                                           const float* shift, const float* mean, const float* rstd,
                                                           const float* coef, long P, int C, int cvb, int rows) {
  using E = ET<T>;
  const ChannelLanes l = channel_lanes(cvb, rows, C / E::VEC);
  if (!l.active()) return;
  const BnConsts<E::VEC, true> k(scale, shift, mean, rstd, l.cv * E::VEC, coef);
  const size_t cofs = (size_t)l.cv * E::VEC;
  auto one = [&](const uint4 rz, const uint4 rd, const size_t off) {
    float fz[E::VEC], fd[E::VEC];
    unpack16<T>(rz, fz);
    unpack16<T>(rd, fd);
#pragma unroll
    for (int j = 0; j < E::VEC; ++j)
      fd[j] = bn_relu_bwd_dz(fz[j], fd[j], k.sc[j], k.sh[j], k.mu[j], k.rs[j], k.c1[j], k.c2[j]);
    *(uint4*)(dz + off) = pack16<T>(fd);
  };
  // Not walk_pixels: through it (one loop) the bf16 instance takes 78 registers instead of 100 and six waves instead of four, and
  // ran 2 to 3 us slower at 128 ch x 128^2 and 64 ch x 256^2 (profiles/channel_refactor_kbench.txt) -- this pass, which writes as
  // much as it reads, streams best at the occupancy the two-loop form leaves.  APPLY_FLIGHT pixels (2 loads each) per thread in
  // flight, all issued before the first store (dz may be dy or z: in place allowed, a thread only ever reads the elements it
  // writes)
  constexpr int APF = APPLY_FLIGHT;
  const long step = (long)gridDim.x * rows;
  long p = (long)blockIdx.x * rows + l.ry;
  for (; p + (APF - 1) * step < P; p += APF * step) {
    size_t o[APF];
    uint4 rz[APF], rd[APF];
#pragma unroll
    for (int u = 0; u < APF; ++u) {
      o[u] = (size_t)(p + u * step) * C + cofs;
      rz[u] = *(const uint4*)(z + o[u]);
      rd[u] = *(const uint4*)(dy + o[u]);
    }
#pragma unroll
    for (int u = 0; u < APF; ++u) one(rz[u], rd[u], o[u]);
  }
  for (; p < P; p += step) {
    const size_t o0 = (size_t)p * C + cofs;
    one(*(const uint4*)(z + o0), *(const uint4*)(dy + o0), o0);
  }
}

// y = relu(z*scale + shift) AND its MaxPool2d(2,2) in one pass (a DoubleConv block whose output feeds a Down block):
// one thread per 2x2 window x channel vector; the pooled value is the maximum of the ROUNDED y values, i.e. exactly what
// maxpool_fwd_kernel reads back, so fused and unfused paths agree bit for bit.
template <typename T>
__global__ __launch_bounds__(256) void bn_relu_apply_pool_kernel(const T* __restrict__ z, T* __restrict__ y,
                                                                 T* __restrict__ pooled, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, int B, int H, int W, int C) {
  using E = ET<T>;
  const int Ho = H >> 1, Wo = W >> 1, CV = C / E::VEC;
  const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;   // also visit the odd border (no pooled output there)
  const long total = (long)B * Hc * Wc * CV;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)total; i += gridDim.x * 256u) {
    const Idx4 ix = split4(i, (unsigned)CV, (unsigned)Wc, (unsigned)Hc);
    const int cv = ix.cv, xo = ix.x, yo = ix.y, b = ix.b;
    float sc[E::VEC], sh[E::VEC], mx[E::VEC];
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) { sc[j] = scale[cv * E::VEC + j]; sh[j] = shift[cv * E::VEC + j]; mx[j] = 0.f; }
    const Window2x2<T> win(b, yo, xo, cv, H, W, C);
    uint4 raw[4];
    win.load(z, raw);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!win.inside(k)) continue;
      float f[E::VEC];
      unpack16<T>(raw[k], f);
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) f[j] = fmaxf(fmaf(f[j], sc[j], sh[j]), 0.f);
      const uint4 pk = pack16<T>(f);
      *(uint4*)(y + win.off[k]) = pk;
      unpack16<T>(pk, f);                           // the rounded values the pooling would read back
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) mx[j] = fmaxf(mx[j], f[j]);   // y >= 0: 0 is a neutral start
    }
    if (yo < Ho && xo < Wo) *(uint4*)(pooled + (((size_t)(b * Ho + yo)) * Wo + xo) * C + cv * E::VEC) = pack16<T>(mx);
  }
}

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int H,
                                                          int W, int C) {
  using E = ET<T>;
  const int Ho = H >> 1, Wo = W >> 1, CV = C / E::VEC;
  const long total = (long)B * Ho * Wo * CV;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)total; i += gridDim.x * 256u) {
    const Idx4 ix = split4(i, (unsigned)CV, (unsigned)Wo, (unsigned)Ho);
    const int cv = ix.cv, xo = ix.x, yo = ix.y, b = ix.b;
    const T* src = x + (((size_t)(b * H + 2 * yo)) * W + 2 * xo) * C + cv * E::VEC;
    float f0[E::VEC], f1[E::VEC], f2[E::VEC], f3[E::VEC];
    unpack16<T>(*(const uint4*)src, f0);
    unpack16<T>(*(const uint4*)(src + C), f1);
    unpack16<T>(*(const uint4*)(src + (size_t)W * C), f2);
    unpack16<T>(*(const uint4*)(src + (size_t)W * C + C), f3);
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) f0[j] = fmaxf(fmaxf(f0[j], f1[j]), fmaxf(f2[j], f3[j]));
    *(uint4*)(y + (((size_t)(b * Ho + yo)) * Wo + xo) * C + cv * E::VEC) = pack16<T>(f0);
  }
}

// dx (+)= route(dy) ; one thread per 2x2 window x channel vector (windows tile the even part of the image).
// STAT: x is the output y = relu(bn(z)) of a DoubleConv block and dx its complete gradient (skip gradient + routed
// pool gradient): the kernel also accumulates that BatchNorm's backward reductions sum(g), sum(g * xhat) with
// g = dx where y > 0 -- xhat is recovered from y itself where the ReLU is active (xhat_from_y), and pixels with y == 0
// contribute nothing -- so the block's bn_bwd_reduce pass (a read of dx and z) disappears.
// Needs a power-of-two number of channel vectors (a thread then keeps its channels); channels with scale == 0 or
// |scale| < |shift| / 16 take xhat from z instead (see from_z below; without z they would get xhat = -mean * rstd).
template <typename T, bool STAT>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          T* __restrict__ dx, int B, int H, int W, int C,
                                                          int accumulate, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, float* __restrict__ part,
                                                          const T* __restrict__ z) {
  using E = ET<T>;
  const int Ho = H >> 1, Wo = W >> 1, CV = C / E::VEC;
  const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;  // also visit the odd border (gradient zero there)
  const long total = (long)B * Hc * Wc * CV;
  float xa[E::VEC], xb[E::VEC], sg[E::VEC], sgx[E::VEC];
  // xhat cannot be recovered from y where scale == 0 (y = relu(shift) is constant), and only badly where |scale| << |shift|
  // (the rounding of y is amplified by 1 / scale).  A thread whose channels include such a one reads z (when the caller
  // passed it) and takes xhat = (z - mean) * rstd like the stand-alone reduction, in a second pass of its own after the
  // main loop; every other thread never touches z.
  bool from_z = false;
  if (STAT) {
    const int cv0 = threadIdx.x % CV;              // fixed for the thread: 256 and the grid stride are multiples of CV
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) {
      const int c = cv0 * E::VEC + j;
      const float sc = scale[c], sh = shift[c];
      from_z = from_z || (z != nullptr && (sc == 0.f || fabsf(sc) * 16.f < fabsf(sh)));
      xhat_from_y(sc, sh, mean[c], rstd[c], xa[j], xb[j]);
      sg[j] = 0.f; sgx[j] = 0.f;
    }
  }
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)total; i += gridDim.x * 256u) {
    const Idx4 ix = split4(i, (unsigned)CV, (unsigned)Wc, (unsigned)Hc);
    const int cv = ix.cv, xo = ix.x, yo = ix.y, b = ix.b;
    const bool inwin = (yo < Ho) && (xo < Wo);
    // every load of the window is issued before any is used (nine serial memory round trips per window otherwise); the pooled
    // gradient too comes from a clamped window
    const int yoc = yo < Ho ? yo : Ho - 1, xoc = xo < Wo ? xo : Wo - 1;
    const uint4 rg = *(const uint4*)(dy + (((size_t)(b * Ho + yoc)) * Wo + xoc) * C + cv * E::VEC);
    const Window2x2<T> win(b, yo, xo, cv, H, W, C);
    uint4 rv[4], ro[4];
    win.load(x, rv);
    if (accumulate) win.load(dx, ro);
    float g[E::VEC];
    float v[4][E::VEC];
    unpack16<T>(rg, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) unpack16<T>(rv[k], v[k]);
    int sel[E::VEC];
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) {
      sel[j] = 0;
      float m = v[0][j];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (v[k][j] > m) { m = v[k][j]; sel[j] = k; }  // strict '>' keeps the FIRST maximum
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!win.inside(k)) continue;
      float o[E::VEC];
      if (accumulate) unpack16<T>(ro[k], o);
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) {
        const float r = (inwin && sel[j] == k) ? g[j] : 0.f;
        o[j] = accumulate ? o[j] + r : r;
        if (STAT) {
          const float gg = v[k][j] > 0.f ? o[j] : 0.f;
          sg[j] += gg;
          sgx[j] = fmaf(gg, fmaf(v[k][j], xa[j], xb[j]), sgx[j]);
        }
      }
      *(uint4*)(dx + win.off[k]) = pack16<T>(o);
    }
  }
  if (STAT) {
    __shared__ float red[256][2 * E::VEC + 1];
    if (from_z) {
      // Rare second pass of this thread over ITS OWN items (a separate loop: the main loop above keeps its registers):
      // sum(g * xhat) again with xhat = (z - mean) * rstd, from the dx values the thread itself wrote (program order makes
      // them visible to it), y for the ReLU mask, and z
#pragma unroll
      for (int j = 0; j < E::VEC; ++j) sgx[j] = 0.f;
      for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)total; i += gridDim.x * 256u) {
        const Idx4 ix = split4(i, (unsigned)CV, (unsigned)Wc, (unsigned)Hc);
        const int cv = ix.cv;
        const Window2x2<T> win(ix.b, ix.y, ix.x, cv, H, W, C, false);
        for (int k = 0; k < 4; ++k) {
          if (!win.inside(k)) continue;
          const size_t off = win.at(k);
          float fy[E::VEC], fd[E::VEC], fz[E::VEC];
          unpack16<T>(*(const uint4*)(x + off), fy);
          unpack16<T>(*(const uint4*)(dx + off), fd);
          unpack16<T>(*(const uint4*)(z + off), fz);
#pragma unroll
          for (int j = 0; j < E::VEC; ++j) {
            const int c = cv * E::VEC + j;
            const float gg = fy[j] > 0.f ? fd[j] : 0.f;
            sgx[j] = fmaf(gg, (fz[j] - mean[c]) * rstd[c], sgx[j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) { red[threadIdx.x][j] = sg[j]; red[threadIdx.x][E::VEC + j] = sgx[j]; }
    __syncthreads();
    for (int q = threadIdx.x; q < CV * E::VEC; q += 256) {
      const int cv = q / E::VEC, j = q - cv * E::VEC;
      float a = 0.f, bsum = 0.f;
      for (int t = cv; t < 256; t += CV) {          // fixed order
        a += red[t][j];
        bsum += red[t][E::VEC + j];
      }
      ((float2*)part)[(size_t)blockIdx.x * C + q] = make_float2(a, bsum);
    }
  }
}

// per-channel sum over pixels (bias gradient of ConvTranspose2d / 1x1 Conv2d): partials [gridDim.x][C]
template <typename T>
__global__ __launch_bounds__(256) void channel_sum_kernel(const T* __restrict__ x, long P, int C, int cvb, int rows,
                                                          float* part) {
  using E = ET<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [rows][cvb][VEC]
  const ChannelLanes l = channel_lanes(cvb, rows, C / E::VEC);
  float s[E::VEC];
#pragma unroll
  for (int j = 0; j < E::VEC; ++j) s[j] = 0.f;
  if (l.active()) {
    const size_t cofs = (size_t)l.cv * E::VEC;
    walk_pixels<REDUCE_FLIGHT>((long)blockIdx.x * rows + l.ry, (long)gridDim.x * rows, P,
                               [&](long p) { return *(const uint4*)(x + (size_t)p * C + cofs); },
                               [&](long, const uint4 raw) {
                                 float f[E::VEC];
                                 unpack16<T>(raw, f);
#pragma unroll
                                 for (int j = 0; j < E::VEC; ++j) s[j] += f[j];
                               });
  }
  reduce_lane_rows(reinterpret_cast<float*>(smem), l, cvb, rows, E::VEC, s, [&](const float (&tot)[E::VEC]) {
    float* dst = part + (size_t)blockIdx.x * C + l.cv * E::VEC;
#pragma unroll
    for (int j = 0; j < E::VEC; ++j) dst[j] = tot[j];
  });
}
// partials [NB][C] -> out; NB <= 512 (segk_bn_bwd_blocks) is one memory round trip
__global__ __launch_bounds__(1024) void channel_sum_finalize_kernel(const float* __restrict__ part, int NB, int C,
                                                                    int C_real, float* out) {
  double s[1];
  if (!sum_rows16<1>(part, NB, C, s)) return;
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  if (c < C_real) out[c] = (float)s[0];
}

template <typename T> constexpr int dtype_of() { return sizeof(T) == 2 ? SEGK_DT_BF16 : SEGK_DT_F32; }
template <typename T> LaneGeometry bn_lanes(int C) { return lane_geometry(C / ET<T>::VEC, BN_LANE_CAP); }

}  // namespace

// ------------------------------------------------------------------------------------------------
unsigned* segk_ticket_slot(int groups, hipStream_t st) {
  static std::atomic<unsigned> n{0};
  static unsigned* base[SEGK_MAX_DEVICES] = {};      // per device: the symbol lives in that device's module image
  const int dev = segk_device_index();
  if (groups < 1 || groups > TICKET_GROUPS) return nullptr;
  if (!base[dev] && hipGetSymbolAddress((void**)&base[dev], HIP_SYMBOL(g_tickets)) != hipSuccess) return nullptr;
  unsigned* const p = base[dev] + (size_t)(n.fetch_add(1, std::memory_order_relaxed) % TICKET_SLOTS) * TICKET_GROUPS;
  // zero what this launch will count in, in stream order right before it (graph-capture safe: a memset node)
  if (hipMemsetAsync(p, 0, (size_t)groups * sizeof(unsigned), st) != hipSuccess) return nullptr;
  return p;
}

// diagnostics / tests: overwrite every ticket counter of the current device with the low 32 bits of `pattern` (what an
// aborted launch, or a stray store, would leave behind); every launch that draws a ticket afterwards must still elect
// exactly one finisher
extern "C" int segk_debug_poison_tickets(uint64_t pattern, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  unsigned* base = nullptr;
  SEGK_REQUIRE(hipGetSymbolAddress((void**)&base, HIP_SYMBOL(g_tickets)) == hipSuccess, "poison_tickets: no ticket array");
  static unsigned host[TICKET_SLOTS * TICKET_GROUPS];
  for (int i = 0; i < TICKET_SLOTS * TICKET_GROUPS; ++i) host[i] = (unsigned)pattern;
  SEGK_REQUIRE(hipMemcpyAsync(base, host, sizeof(host), hipMemcpyHostToDevice, st) == hipSuccess, "poison_tickets: copy failed");
  SEGK_REQUIRE(hipStreamSynchronize(st) == hipSuccess, "poison_tickets: sync failed");
  return 0;
}

extern "C" int segk_bn_finalize(const float* part, int MT, int C, int C_real, double count, const float* conv_bias,
                                const float* gamma, const float* beta, float* rmean, float* rvar, float momentum, float eps,
                                int training, float* scale, float* shift, float* mean, float* rstd, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(C > 0 && C % 32 == 0 && C_real > 0 && C_real <= C, "bn_finalize: bad channels C=%d real=%d", C, C_real);
  SEGK_REQUIRE(gamma && beta && scale && shift, "bn_finalize: null pointer");
  if (training) SEGK_REQUIRE(part && MT > 0 && count > 0 && mean && rstd, "bn_finalize: training needs partials");
  else SEGK_REQUIRE(rmean && rvar, "bn_finalize: eval needs running statistics");
  // the stats buffer carries NCH*C*2 doubles of scratch behind the [MT][C][2] float partials
  double* scratch = part ? (double*)(const_cast<float*>(part) + (size_t)MT * C * 2) : nullptr;
  if (training && MT <= 1024) {
    hipLaunchKernelGGL(bn_stats_finalize_small_kernel, dim3(C / 32), dim3(1024), 0, st, part, MT, C, C_real, count, conv_bias,
                       gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean, rstd);
    SEGK_CHECK_LAUNCH("bn_stats_finalize_small");
    return 0;
  }
  if (training) {
    SEGK_REQUIRE(C / 32 <= TICKET_GROUPS, "bn_finalize: at most %d channels", 32 * TICKET_GROUPS);
    unsigned* const tickets = segk_ticket_slot(C / 32, st);
    SEGK_REQUIRE(tickets != nullptr, "bn_finalize: no ticket array");
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C / 32, NCH), dim3(256), 0, st, part, MT, C, C_real, count, conv_bias,
                       gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean, rstd, scratch, tickets);
    SEGK_CHECK_LAUNCH("bn_stats_finalize");
    return 0;
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C / 32), dim3(256), 0, st, scratch, NCH, C, C_real, count, conv_bias,
                     gamma, beta, rmean, rvar, momentum, eps, training, scale, shift, mean, rstd);
  SEGK_CHECK_LAUNCH("bn_finalize");
  return 0;
}
int segk_bn_stats_floats(int tiles, int Cp) {
  if (tiles <= 0 || Cp <= 0) return 0;
  const long long n = (long long)tiles * Cp * 2 + (long long)NCH * Cp * 4;
  return n > 0x7fffffffLL ? 0 : (int)n;     // sizes that do not fit an int are not served (the launch entries refuse them)
}

extern "C" int segk_bn_relu_apply(const void* z, void* y, const float* scale, const float* shift, long P, int C, int dtype,
                                  segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("bn_relu_apply", dtype);
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(z && y && scale && shift && P > 0 && C > 0 && C % 32 == 0, "bn_relu_apply: bad arguments");
  return by_dtype(dtype, [&](auto Tc) {
    using T = decltype(Tc);
    const LaneGeometry g = bn_lanes<T>(C);
    hipLaunchKernelGGL(bn_relu_apply_kernel<T>, dim3(apply_blocks(P, g.rows), g.gy), dim3(256), 0, st, (const T*)z, (T*)y, scale,
                       shift, P, C, g.cvb, g.rows);
    SEGK_CHECK_LAUNCH("bn_relu_apply");
    return 0;
  });
}

extern "C" int segk_bn_relu_apply_pool(const void* z, void* y, void* pooled, const float* scale, const float* shift, int B,
                                       int H, int W, int C, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("bn_relu_apply_pool", dtype);
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(z && y && pooled && scale && shift && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 32 == 0,
               "bn_relu_apply_pool: bad arguments");
  const int g = window_grid(B, H, W, C, dtype, true, 8192);
  SEGK_REQUIRE(g > 0, "bn_relu_apply_pool: more than 2^31 windows x channel vectors");
  by_dtype(dtype, [&](auto Tc) {
    using T = decltype(Tc);
    hipLaunchKernelGGL(bn_relu_apply_pool_kernel<T>, dim3(g), dim3(256), 0, st, (const T*)z, (T*)y, (T*)pooled, scale, shift, B, H,
                       W, C);
    return 0;
  });
  SEGK_CHECK_LAUNCH("bn_relu_apply_pool");
  return 0;
}

// partial rows [nb][C][2] -> dgamma, dbeta, coef: the finalize step of every BatchNorm backward form
int segk_bn_bwd_finalize_launch(const float* part, int nb, int C, int C_real, long P, float* dgamma, float* dbeta, float* coef,
                                hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C / 32), dim3(1024), 0, st, part, nb, C, C_real, (double)P, dgamma, dbeta,
                     coef);
  SEGK_CHECK_LAUNCH("bn_bwd_finalize");
  return 0;
}

int segk_bn_bwd_blocks(long P, int C, int dtype) {
  if (P <= 0 || C <= 0 || C % 32 != 0) return 0;      // nonsense input: no blocks (the launch entries refuse it)
  const int rows = lane_geometry(C / (dtype == SEGK_DT_BF16 ? 8 : 4), BN_LANE_CAP).rows;
  const long gx = (P + rows - 1) / rows;
  return (int)(gx > 512 ? 512 : gx);      // enough blocks to fill the chip; keeps the finalize pass short
}

// The BatchNorm + ReLU backward: reduce (partials of nb = segk_bn_bwd_blocks rows into `part`; without it `part` holds nb rows
// another kernel produced), finalize, apply (without it the consumer of dz forms it in registers: segk_stem3x3_wgrad_bn)
template <typename T>
static int bn_bwd_launch(bool reduce, bool apply, const void* dy, const void* z, void* dz, const float* scale, const float* shift,
                         const float* mean, const float* rstd, long P, int C, int C_real, float* part, int nb, float* dgamma,
                         float* dbeta, float* coef, hipStream_t st) {
  const LaneGeometry g = bn_lanes<T>(C);
  if (reduce) {
    nb = segk_bn_bwd_blocks(P, C, dtype_of<T>());
    const size_t lds = (size_t)g.rows * g.cvb * 2 * ET<T>::VEC * sizeof(float);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(nb, g.gy), dim3(256), lds, st, (const T*)dy, (const T*)z, scale, shift, mean,
                       rstd, P, C, g.cvb, g.rows, part);
    SEGK_CHECK_LAUNCH("bn_bwd_reduce");
  }
  if (const int rc = segk_bn_bwd_finalize_launch(part, nb, C, C_real, P, dgamma, dbeta, coef, st)) return rc;
  if (apply) {
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(apply_blocks(P, g.rows), g.gy), dim3(256), 0, st, (const T*)dy, (const T*)z,
                       (T*)dz, scale, shift, mean, rstd, coef, P, C, g.cvb, g.rows);
    SEGK_CHECK_LAUNCH("bn_bwd_apply");
  }
  return 0;
}
extern "C" int segk_bn_relu_bwd_from_part(const void* dy, const void* z, void* dz, const float* scale, const float* shift,
                                          const float* mean, const float* rstd, long P, int C, int C_real, const float* part,
                                          int nb, float* dgamma, float* dbeta, float* coef, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("bn_relu_bwd_from_part", dtype);
  SEGK_REQUIRE(dy && z && dz && scale && shift && mean && rstd && part && dgamma && dbeta && coef && nb > 0,
               "bn_bwd_from_part: bad arguments");
  SEGK_REQUIRE(P > 0 && C > 0 && C % 32 == 0 && C_real > 0 && C_real <= C, "bn_bwd_from_part: bad shape");
  return by_dtype(dtype, [&](auto Tc) {
    return bn_bwd_launch<decltype(Tc)>(false, true, dy, z, dz, scale, shift, mean, rstd, P, C, C_real, const_cast<float*>(part), nb,
                                       dgamma, dbeta, coef, (hipStream_t)s);
  });
}

extern "C" int segk_bn_relu_bwd_stats(const void* dy, const void* z, const float* scale, const float* shift, const float* mean,
                                      const float* rstd, long P, int C, int C_real, float* part, float* dgamma, float* dbeta,
                                      float* coef, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("bn_relu_bwd_stats", dtype);
  SEGK_REQUIRE(dy && z && scale && shift && mean && rstd && part && dgamma && dbeta && coef, "bn_bwd_stats: null pointer");
  SEGK_REQUIRE(P > 0 && C > 0 && C % 32 == 0 && C_real > 0 && C_real <= C, "bn_bwd_stats: bad shape");
  return by_dtype(dtype, [&](auto Tc) {
    return bn_bwd_launch<decltype(Tc)>(true, false, dy, z, nullptr, scale, shift, mean, rstd, P, C, C_real, part, 0, dgamma, dbeta,
                                       coef, (hipStream_t)s);
  });
}

extern "C" int segk_bn_relu_bwd(const void* dy, const void* z, void* dz, const float* scale, const float* shift,
                                const float* mean, const float* rstd, long P, int C, int C_real, float* part, float* dgamma,
                                float* dbeta, float* coef, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("bn_relu_bwd", dtype);
  SEGK_REQUIRE(dy && z && dz && scale && shift && mean && rstd && part && dgamma && dbeta && coef,
               "bn_bwd: null pointer");
  SEGK_REQUIRE(P > 0 && C > 0 && C % 32 == 0 && C_real > 0 && C_real <= C, "bn_bwd: bad shape");
  return by_dtype(dtype, [&](auto Tc) {
    return bn_bwd_launch<decltype(Tc)>(true, true, dy, z, dz, scale, shift, mean, rstd, P, C, C_real, part, 0, dgamma, dbeta, coef,
                                       (hipStream_t)s);
  });
}

extern "C" int segk_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int C, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("maxpool2x2_fwd", dtype);
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(x && y && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 32 == 0, "maxpool_fwd: bad arguments");
  const int g = window_grid(B, H, W, C, dtype, false, 8192);
  SEGK_REQUIRE(g > 0, "maxpool_fwd: more than 2^31 windows x channel vectors");
  by_dtype(dtype, [&](auto Tc) {
    using T = decltype(Tc);
    hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(g), dim3(256), 0, st, (const T*)x, (T*)y, B, H, W, C);
    return 0;
  });
  SEGK_CHECK_LAUNCH("maxpool_fwd");
  return 0;
}

// the two forms of the pooling backward on a grid of g blocks (bn, part, z: the statistics form's operands)
template <bool STAT>
static void maxpool_bwd_launch(int g, const void* x, const void* dy, void* dx, int B, int H, int W, int C, int accumulate,
                               const float* const* bn, float* part, const void* z, int dtype, hipStream_t st) {
  by_dtype(dtype, [&](auto Tc) {
    using T = decltype(Tc);
    hipLaunchKernelGGL((maxpool_bwd_kernel<T, STAT>), dim3(g), dim3(256), 0, st, (const T*)x, (const T*)dy, (T*)dx, B, H, W, C,
                       accumulate, bn[0], bn[1], bn[2], bn[3], part, (const T*)z);
    return 0;
  });
}

extern "C" int segk_maxpool2x2_bwd(const void* x, const void* dy, void* dx, int B, int H, int W, int C, int accumulate,
                                   int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("maxpool2x2_bwd", dtype);
  SEGK_REQUIRE(x && dy && dx && B > 0 && H >= 2 && W >= 2 && C > 0 && C % 32 == 0, "maxpool_bwd: bad arguments");
  const int g = window_grid(B, H, W, C, dtype, true, 8192);
  SEGK_REQUIRE(g > 0, "maxpool_bwd: more than 2^31 windows x channel vectors");
  const float* const none[4] = {nullptr, nullptr, nullptr, nullptr};
  maxpool_bwd_launch<false>(g, x, dy, dx, B, H, W, C, accumulate, none, nullptr, nullptr, dtype, (hipStream_t)s);
  SEGK_CHECK_LAUNCH("maxpool_bwd");
  return 0;
}

// blocks (= partial rows) of the fused pooling-backward + BatchNorm-reduce kernel, or 0 when the shape is not served
int segk_maxpool_bwd_stat_blocks(int B, int H, int W, int C, int dtype) {
  if (B <= 0 || H < 2 || W < 2 || C <= 0 || C % 32 != 0) return 0;
  const int cv = C / (dtype == SEGK_DT_BF16 ? 8 : 4);
  if ((cv & (cv - 1)) != 0 || cv > 256) return 0;
  return window_grid(B, H, W, C, dtype, true, 1024);    // (0: the kernels index windows x channel vectors with 32 bits)
}

extern "C" int segk_maxpool2x2_bwd_bnstat(const void* x, const void* dy, void* dx, int B, int H, int W, int C, int accumulate,
                                          const float* scale, const float* shift, const float* mean, const float* rstd,
                                          float* part, const void* z, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("maxpool2x2_bwd_bnstat", dtype);
  SEGK_REQUIRE(x && dy && dx && scale && shift && mean && rstd && part, "maxpool_bwd_bnstat: null pointer");
  const int g = segk_maxpool_bwd_stat_blocks(B, H, W, C, dtype);
  SEGK_REQUIRE(g > 0, "maxpool_bwd_bnstat: shape not served (channel vectors must be a power of two)");
  const float* const bn[4] = {scale, shift, mean, rstd};
  maxpool_bwd_launch<true>(g, x, dy, dx, B, H, W, C, accumulate, bn, part, z, dtype, (hipStream_t)s);
  SEGK_CHECK_LAUNCH("maxpool_bwd_bnstat");
  return 0;
}

extern "C" int segk_channel_sum(const void* x, long P, int C, int C_real, float* part, float* out, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("channel_sum", dtype);
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(x && part && out && P > 0 && C > 0 && C % 32 == 0 && C_real > 0 && C_real <= C, "channel_sum: bad arguments");
  const int gx = segk_bn_bwd_blocks(P, C, dtype);
  by_dtype(dtype, [&](auto Tc) {
    using T = decltype(Tc);
    const LaneGeometry g = bn_lanes<T>(C);
    const size_t lds = (size_t)g.rows * g.cvb * ET<T>::VEC * sizeof(float);
    hipLaunchKernelGGL(channel_sum_kernel<T>, dim3(gx, g.gy), dim3(256), lds, st, (const T*)x, P, C, g.cvb, g.rows, part);
    return 0;
  });
  SEGK_CHECK_LAUNCH("channel_sum");
  hipLaunchKernelGGL(channel_sum_finalize_kernel, dim3(C / 32), dim3(1024), 0, st, part, gx, C, C_real, out);
  SEGK_CHECK_LAUNCH("channel_sum_finalize");
  return 0;
}
