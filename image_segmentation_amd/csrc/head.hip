// Output head: the 1x1 Conv2d to a handful of classes, forward and backward, and the BatchNorm + ReLU backward apply pass of the
// block in front of it without a stored gradient.  All HBM-bound; logits are fp32 NCHW exactly like the reference returns
// them (unet/unet.py:91,105; clip/clipunet.py:181,187).  The losses and the metric on those logits: loss.hip.  The backward
// kernels are channel-vector streaming kernels like bn_pool.hip's: lane map, row reduce, constants and walk of channel_lanes.hpp.
#include "channel_lanes.hpp"
#include "class_pixels.hpp"
#include "segk_internal.h"

namespace {
static_assert(MAXC == 8, "the staged weights ws[MAXC * HCH] and the partial layout [block][MAXC][Cp + 1] are sized for 8 classes");
constexpr int HT = 256;    // pixels per head tile (one per thread)
constexpr int HCH = 64;    // channels staged per pass

// kernels are compiled for 2, 3, 4 and MAXC classes (the smallest that holds ncls).  The forward, the backward and the apply
// pass without a stored dy all come through here: the sums over k of the last two run over the same terms
template <typename F> auto dispatch_head_nc(int ncls, F&& f) { return dispatch_nc<2, 3, 4, MAXC>(ncls, f); }

// ------------------------------------------------------------------------------------------------
// logits[b][k][y][x] = bias[k] + sum_c y[p][c] * Wt[k][c]
// NC = compiled class count (>= ncls): the per-class loops are unrolled to it, not to MAXC
template <typename T, int NC>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ y, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ logits,
                                                       long P, long HW, int Cp, int C, int ncls,
                                                       const float* __restrict__ zsc, const float* __restrict__ zsh) {
  // zsc != NULL: the input is the pre-activation z of the last DoubleConv block and y = relu(z * zsc + zsh), rounded to T
  // as segk_bn_relu_apply would have stored it, is formed on the way into LDS (the block's output is never written)
  using E = ET<T>;
  constexpr int PITCH = HCH * E::ES + 16;
  extern __shared__ __attribute__((aligned(16))) char tile[];   // HT * PITCH bytes
  __shared__ float ws[MAXC * HCH + 2 * HCH];
  float* const zs = ws + MAXC * HCH;                            // [2][HCH] scale, shift of this pass
  const int tid = threadIdx.x;
  for (long p0 = (long)blockIdx.x * HT; p0 < P; p0 += (long)gridDim.x * HT) {
    float acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = (k < ncls) ? bias[k] : 0.f;
    for (int c0 = 0; c0 < Cp; c0 += HCH) {
      __syncthreads();
      constexpr int VPR = HCH / E::VEC;  // 16-byte vectors per pixel row of this pass
      if (zsc != nullptr) {
        if (tid < 2 * HCH) {
          const int c = c0 + (tid & (HCH - 1));
          zs[tid] = c < Cp ? (tid < HCH ? zsc[c] : zsh[c]) : 0.f;
        }
        __syncthreads();
      }
      // all of the thread's vectors of this pass are fetched before the first is used, unconditionally, from a pixel /
      // channel index clamped into the tensor (left as a loop of conditional loads the compiler keeps ONE in flight)
      constexpr int NQ = HT * VPR / 256;
      uint4 raw[NQ];
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int q = tid + 256 * u, px = q / VPR, v = q - px * VPR;
        const long pp = p0 + px < P ? p0 + px : P - 1;
        const int cc = c0 + v * E::VEC < Cp ? c0 + v * E::VEC : 0;
        raw[u] = *(const uint4*)(y + (size_t)pp * Cp + cc);
      }
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int q = tid + 256 * u, px = q / VPR, v = q - px * VPR;
        uint4 d = make_uint4(0, 0, 0, 0);
        if (p0 + px < P && c0 + v * E::VEC < Cp) {
          d = raw[u];
          if (zsc != nullptr) {
            float f[E::VEC];
            unpack16<T>(d, f);
#pragma unroll
            for (int j = 0; j < E::VEC; ++j) f[j] = fmaxf(fmaf(f[j], zs[v * E::VEC + j], zs[HCH + v * E::VEC + j]), 0.f);
            d = pack16<T>(f);
          }
        }
        *(uint4*)(tile + px * PITCH + v * 16) = d;
      }
      for (int q = tid; q < MAXC * HCH; q += 256) {
        const int k = q / HCH, c = c0 + (q - k * HCH);
        ws[q] = (k < ncls && c < C) ? w[(size_t)k * C + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int v = 0; v < VPR; ++v) {
        float f[E::VEC];
        unpack16<T>(*(const uint4*)(tile + tid * PITCH + v * 16), f);
#pragma unroll
        for (int j = 0; j < E::VEC; ++j)
#pragma unroll
          for (int k = 0; k < NC; ++k) acc[k] = fmaf(f[j], ws[k * HCH + v * E::VEC + j], acc[k]);
      }
    }
    const long p = p0 + tid;
    if (p < P) {
      long b, r; split_hw(p, HW, b, r);
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < ncls) logits[(b * ncls + k) * HW + r] = acc[k];
    }
  }
}

// dy[p][c] = sum_k dl[p][k] * W[k][c];  partial dW[k][c] = sum_p dl[p][k]*y[p][c], db[k] = sum_p dl[p][k].
// Pure streaming: a thread owns one 16-byte channel vector (its weights W[k][c..c+VEC) and its dW partials
// live in registers) and walks pixels; a row of threads covers whole contiguous pixel rows of y / dy.
// ZIN: `y` holds the pre-activation z of the last DoubleConv block: y = relu(z * scale + shift) is re-formed per value
// (rounded to T like the stored tensor would be) and the BatchNorm reductions take xhat = (z - mean) * rstd from z itself.
// Vector width of the head's backward pass.  bf16 threads own FOUR channels (an 8-byte vector) instead of the eight of a
// 16-byte one: the per-thread weight / gradient / BatchNorm arrays halve (176 -> ~100 registers), twice the waves fit a CU, and
// the pass -- whose arithmetic (~73 us) and traffic (~100 us) added up at 8 waves per CU -- overlaps them.
#ifndef HEAD_BWD_VEC
#define HEAD_BWD_VEC 4
#endif
template <typename T> struct HeadVec;
template <> struct HeadVec<float> {
  static constexpr int HV = 4;
  using Raw = uint4;
  static __device__ __forceinline__ void unpack(const Raw& v, float* f) { unpack16<float>(v, f); }
  static __device__ __forceinline__ Raw pack(const float* f) { return pack16<float>(f); }
};
template <> struct HeadVec<bf16_t> {
  static constexpr int HV = HEAD_BWD_VEC;
  static_assert(HV == 4 || HV == 8, "head backward: 4 or 8 bf16 channels per thread");
  using Raw = std::conditional_t<HV == 8, uint4, uint2>;
  static __device__ __forceinline__ void unpack(const uint4& v, float* f) { unpack16<bf16_t>(v, f); }
  static __device__ __forceinline__ void unpack(const uint2& v, float* f) {
    f[0] = bf2f(v.x & 0xffffu); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = bf2f(v.y & 0xffffu); f[3] = __uint_as_float(v.y & 0xffff0000u);
  }
  static __device__ __forceinline__ uint4 pack_n(const float* f, std::integral_constant<int, 8>) { return pack16<bf16_t>(f); }
  static __device__ __forceinline__ uint2 pack_n(const float* f, std::integral_constant<int, 4>) {
    return make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
  }
  static __device__ __forceinline__ Raw pack(const float* f) { return pack_n(f, std::integral_constant<int, HV>{}); }
};

// STORE = false: everything but the store of dy (segk_head_bwd_bn_stats: head_bn_bwd_apply_kernel below re-forms dy per element)
template <typename T, int NC, bool ZIN, bool STORE = true>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dlog, const T* __restrict__ y,
                                                       const float* __restrict__ w, T* __restrict__ dy,
                                                       float* __restrict__ part, long P, long HW, int Cp, int C,
                                                       int ncls, int cvb, int rows, const float* __restrict__ bn_scale,
                                                       const float* __restrict__ bn_shift, const float* __restrict__ bn_mean,
                                                       const float* __restrict__ bn_rstd, float* __restrict__ bnpart) {
  constexpr int HV = HeadVec<T>::HV;                   // channels per thread (bf16: 4 = an 8-byte vector)
  using Raw = typename HeadVec<T>::Raw;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = (float*)smem_raw;                       // [rows][cvb][MAXC*VEC + MAXC]
  // bnpart != NULL: y is the output relu(bn(z)) of the last DoubleConv block and dy its complete gradient: also accumulate
  // that BatchNorm's backward reductions sum(g), sum(g*xhat) (xhat recovered from y where the ReLU is active), like
  // maxpool_bwd_kernel<STAT> does for the Down blocks
  const bool stat = bnpart != nullptr;
  float xa[HV], xb[HV], sg[2 * HV];               // sg: sum g, then sum g * xhat
#pragma unroll
  for (int j = 0; j < HV; ++j) { xa[j] = 0.f; xb[j] = 0.f; sg[j] = 0.f; sg[HV + j] = 0.f; }
  constexpr int RW = MAXC * HV + MAXC;
  const ChannelLanes l = channel_lanes(cvb, rows, Cp / HV);
  const int cx = l.cx, ry = l.ry, cv = l.cv;
  const bool active = l.active();
  float wr[NC][HV], aw[NC][HV], ab[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    ab[k] = 0.f;
#pragma unroll
    for (int j = 0; j < HV; ++j) {
      const int c = cv * HV + j;
      wr[k][j] = (active && k < ncls && c < C) ? w[(size_t)k * C + c] : 0.f;
      aw[k][j] = 0.f;
    }
  }
  float zc[ZIN ? HV : 1], zh[ZIN ? HV : 1];     // ZIN: scale, shift (xa = rstd, xb = -mean * rstd)
  if (active && (stat || ZIN)) {
#pragma unroll
    for (int j = 0; j < HV; ++j) {
      const int c = cv * HV + j;
      const float sc = bn_scale[c], rs = bn_rstd[c];
      if constexpr (ZIN) {
        zc[j] = sc; zh[j] = bn_shift[c];
        xa[j] = rs; xb[j] = -bn_mean[c] * rs;
      } else {
        xhat_from_y(sc, bn_shift[c], bn_mean[c], rs, xa[j], xb[j]);
      }
    }
  }
  if (active) {
    // one pixel: dy, the dW / db partials and (stat) the BatchNorm reductions from the raw input vector `raw`
    auto pixel = [&](long p, const float (&dl)[NC], const Raw raw) {
      float f[HV], z[HV], o[HV];
      HeadVec<T>::unpack(raw, f);
      if constexpr (ZIN) {
#pragma unroll
        for (int j = 0; j < HV; ++j) { z[j] = f[j]; f[j] = fmaxf(fmaf(f[j], zc[j], zh[j]), 0.f); }
        HeadVec<T>::unpack(HeadVec<T>::pack(f), f);               // the value segk_bn_relu_apply would have stored
      }
#pragma unroll
      for (int j = 0; j < HV; ++j) o[j] = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        ab[k] += dl[k];
#pragma unroll
        for (int j = 0; j < HV; ++j) {
          o[j] = fmaf(dl[k], wr[k][j], o[j]);
          aw[k][j] = fmaf(dl[k], f[j], aw[k][j]);
        }
      }
      if constexpr (STORE) *(Raw*)(dy + (size_t)p * Cp + cv * HV) = HeadVec<T>::pack(o);
      if (stat) {
#pragma unroll
        for (int j = 0; j < HV; ++j) {
          const float gg = f[j] > 0.f ? o[j] : 0.f;
          sg[j] += gg;
          sg[HV + j] = fmaf(gg, fmaf(ZIN ? z[j] : f[j], xa[j], xb[j]), sg[HV + j]);
        }
      }
    };
    // (image, offset) of a pixel stream is carried along instead of divided out per pixel: no division in the loop
    auto advance = [&](long& b, long& r, long d) {
      r += d;
      while (r >= HW) { r -= HW; ++b; }
    };
    // PIF pixels per iteration: all their loads are in flight before the first is used (the loop is latency-bound otherwise);
    // every pixel stream carries its own (image, offset), which is why this is not walk_pixels (channel_lanes.hpp): its load
    // sees a pixel index, not the stream the pixel belongs to
    constexpr int PIF = 2;
    const long step = (long)gridDim.x * rows;
    long p = (long)blockIdx.x * rows + ry;
    long bS[PIF], rS[PIF];
    bS[0] = 0; rS[0] = 0;
    if (p < P) split_hw(p, HW, bS[0], rS[0]);
#pragma unroll
    for (int u = 1; u < PIF; ++u) { bS[u] = bS[u - 1]; rS[u] = rS[u - 1]; advance(bS[u], rS[u], step); }
    for (; p + (PIF - 1) * step < P; p += PIF * step) {
      float dl[PIF][NC];
      Raw rw[PIF];
#pragma unroll
      for (int u = 0; u < PIF; ++u) rw[u] = *(const Raw*)(y + (size_t)(p + u * step) * Cp + cv * HV);
#pragma unroll
      for (int u = 0; u < PIF; ++u) load_classes<NC>(dlog, bS[u], rS[u], ncls, HW, dl[u], 0.f);
#pragma unroll
      for (int u = 0; u < PIF; ++u) pixel(p + u * step, dl[u], rw[u]);
#pragma unroll
      for (int u = 0; u < PIF; ++u) advance(bS[u], rS[u], PIF * step);
    }
    for (; p < P; p += step) {                      // tail: one pixel at a time, stream 0 walks on by one step
      float dl0[NC];
      const Raw r0 = *(const Raw*)(y + (size_t)p * Cp + cv * HV);
      load_classes<NC>(dlog, bS[0], rS[0], ncls, HW, dl0, 0.f);
      pixel(p, dl0, r0);
      advance(bS[0], rS[0], step);
    }
  }
  if (ry < rows) {
    float* q = red + ((size_t)ry * cvb + cx) * RW;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int j = 0; j < HV; ++j) q[k * HV + j] = aw[k][j];
      q[MAXC * HV + k] = ab[k];
    }
  }
  __syncthreads();
  if (ry == 0 && cv < Cp / HV) {
    // part layout: [block][MAXC][Cp + 1]  (last column = bias gradient, written by channel vector 0)
    float* dst = part + (size_t)blockIdx.x * MAXC * (Cp + 1);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
      for (int j = 0; j < HV; ++j) {
        float s = 0.f;
        for (int r2 = 0; r2 < rows; ++r2) s += red[((size_t)r2 * cvb + cx) * RW + k * HV + j];   // fixed order
        dst[k * (Cp + 1) + cv * HV + j] = s;
      }
      if (cv == 0) {
        float s = 0.f;
        for (int r2 = 0; r2 < rows; ++r2) s += red[((size_t)r2 * cvb + cx) * RW + MAXC * HV + k];
        dst[k * (Cp + 1) + Cp] = s;
      }
    }
  }
  if (stat) {
    __syncthreads();
    reduce_lane_rows(red, l, cvb, rows, RW, sg, [&](const float (&tot)[2 * HV]) {
      float2* dst = (float2*)bnpart + (size_t)blockIdx.x * Cp + cv * HV;
#pragma unroll
      for (int j = 0; j < HV; ++j) dst[j] = make_float2(tot[j], tot[HV + j]);
    });
  }
}

// one 64-lane wave per output element: lanes stride the NB block partials, fixed-order tree reduce
__global__ __launch_bounds__(256) void head_bwd_finalize_kernel(const float* __restrict__ part, int NB, int Cp, int C,
                                                                int ncls, float* __restrict__ dw,
                                                                float* __restrict__ db) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= ncls * (C + 1)) return;
  const int k = i / (C + 1), c = i - k * (C + 1);
  const int col = (c == C) ? Cp : c;
  double s = 0.0;
  for (int b = lane; b < NB; b += 64) s += (double)part[(size_t)b * MAXC * (Cp + 1) + k * (Cp + 1) + col];
  s = wave_sum(s);
  if (lane != 0) return;
  if (c == C) db[k] = (float)s;
  else dw[(size_t)k * C + c] = (float)s;
}

// BatchNorm + ReLU backward apply pass of the block in front of the head WITHOUT a stored dy (the 64-channel gradient at full
// resolution is larger than the Infinity Cache: written, read back once, dropped).  dy[p][c] = sum_k dl[p][k] * W[k][c] is
// re-formed per element exactly as head_bwd_kernel forms it (k ascending from 0.f, the same compiled class count, rounded to T
// like the stored tensor), then bn_relu_bwd_dz: dz is bit-identical to segk_head_bwd_bn + segk_bn_relu_bwd_from_part.
// A thread owns one channel vector and walks pixels; the vector is head_bwd_kernel's (bf16: four channels, 8 bytes), not the
// 16 bytes of bn_bwd_apply_kernel: beside six BatchNorm constants per channel the NC weights per channel make 8 channels
// 138 registers (3 waves per SIMD; 268 MB took 173 us, no faster than the stored apply pass), 4 channels about 80.
// One pixel in flight per thread (APPLY_FLIGHT, channel_lanes.hpp).
template <typename T, int NC>
__global__ __launch_bounds__(256) void head_bn_bwd_apply_kernel(const float* __restrict__ dlog, const T* __restrict__ z,
                                                                const float* __restrict__ w, T* __restrict__ dz,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ coef, long P, long HW, int Cp, int C,
                                                                int ncls, int cvb, int rows) {
  constexpr int V = HeadVec<T>::HV;
  using Raw = typename HeadVec<T>::Raw;
  const ChannelLanes l = channel_lanes(cvb, rows, Cp / V);
  if (!l.active()) return;
  const int cv = l.cv;
  const BnConsts<V, true> bn(scale, shift, mean, rstd, cv * V, coef);
  float wr[NC][V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = cv * V + j;
#pragma unroll
    for (int k = 0; k < NC; ++k) wr[k][j] = (k < ncls && c < C) ? w[(size_t)k * C + c] : 0.f;
  }
  struct Pixel { Raw z; float dl[NC]; };
  // the (image, offset) of the thread's pixel is carried along instead of divided out per pixel, as in head_bwd_kernel
  const long step = (long)gridDim.x * rows, first = (long)blockIdx.x * rows + l.ry;
  long b = 0, r = 0;
  if (first < P) split_hw(first, HW, b, r);
  auto load = [&](long p) {
    Pixel v;
    v.z = *(const Raw*)(z + (size_t)p * Cp + cv * V);
    load_classes<NC>(dlog, b, r, ncls, HW, v.dl, 0.f);      // head_bwd_kernel's load
    r += step;
    while (r >= HW) { r -= HW; ++b; }
    return v;
  };
  auto pixel = [&](long p, const Pixel& v) {
    const float (&dl)[NC] = v.dl;
    float fz[V], o[V];
    HeadVec<T>::unpack(v.z, fz);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = fmaf(dl[k], wr[k][j], o[j]);
    HeadVec<T>::unpack(HeadVec<T>::pack(o), o);      // the value the stored dy would have held
#pragma unroll
    for (int j = 0; j < V; ++j)
      o[j] = bn_relu_bwd_dz(fz[j], o[j], bn.sc[j], bn.sh[j], bn.mu[j], bn.rs[j], bn.c1[j], bn.c2[j]);
    *(Raw*)(dz + (size_t)p * Cp + cv * V) = HeadVec<T>::pack(o);
  };
  walk_pixels<APPLY_FLIGHT>(first, step, P, load, pixel);
}
}  // namespace

template <typename T> static size_t head_lds() { return (size_t)HT * (HCH * ET<T>::ES + 16); }

// ------------------------------------------------------------------------------------------------
int segk_head_blocks(long P) {
  if (P <= 0) return 0;
  const long g = (P + 31) / 32;
  return (int)(g > 1024 ? 1024 : g);
}
int segk_head_part_floats(long P, int Cp) {
  if (P <= 0 || Cp <= 0) return 0;
  const long long n = (long long)segk_head_blocks(P) * MAXC * ((long long)Cp + 1);
  return n > 0x7fffffffLL ? 0 : (int)n;
}

// zsc, zsh: BatchNorm scale / shift applied (with the ReLU) to a pre-activation input, or null for an activation
static int head_fwd(const void* y, const float* w, const float* bias, float* logits, int B, int H, int W, int Cp, int C, int ncls,
                    const float* zsc, const float* zsh, int dtype, hipStream_t st) {
  SEGK_REQUIRE(y && w && bias && logits && B > 0 && H > 0 && W > 0, "head_fwd: bad arguments");
  SEGK_REQUIRE((zsc == nullptr) == (zsh == nullptr), "head_fwd: scale and shift come together");
  SEGK_REQUIRE_DTYPE("head_fwd", dtype);
  SEGK_REQUIRE(ncls >= 1 && ncls <= MAXC, "head_fwd: 1..%d classes supported, got %d", MAXC, ncls);
  SEGK_REQUIRE(Cp % 32 == 0 && C > 0 && C <= Cp, "head_fwd: bad channels");
  const long P = (long)B * H * W, HW = (long)H * W;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  long g = (P + HT - 1) / HT;
  if (g > 4096) g = 4096;
  auto launch = [&](auto Tc, auto NCc) {
    using T = decltype(Tc);
    constexpr int NC = decltype(NCc)::value;
    return segk_launch_lds<head_fwd_kernel<T, NC>>("head_fwd", 96 * 1024, dim3((int)g), dim3(256), head_lds<T>(), st, (const T*)y, w,
                                                   bias, logits, P, HW, Cp, C, ncls, zsc, zsh);
  };
  auto by_nc = [&](auto Tc) { return dispatch_head_nc(ncls, [&](auto NCc) { return launch(Tc, NCc); }); };
  return by_dtype(dtype, by_nc);
}
extern "C" int segk_head_fwd(const void* y, const float* w, const float* bias, float* logits, int B, int H, int W, int Cp, int C,
                             int ncls, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("head_fwd", dtype);
  return head_fwd(y, w, bias, logits, B, H, W, Cp, C, ncls, nullptr, nullptr, dtype, (hipStream_t)s);
}
extern "C" int segk_head_fwd_bn(const void* z, const float* scale, const float* shift, const float* w, const float* bias,
                                float* logits, int B, int H, int W, int Cp, int C, int ncls, int dtype, segk_stream_t s) {
  SEGK_REQUIRE(scale && shift, "head_fwd_bn: null scale/shift");
  return head_fwd(z, w, bias, logits, B, H, W, Cp, C, ncls, scale, shift, dtype, (hipStream_t)s);
}

template <typename T>
static int head_bwd_t(const float* dlog, const void* y, const float* w, void* dy, float* part, float* dw, float* db,
                      long P, long HW, int Cp, int C, int ncls, const float* const* bn, float* bnpart, bool zin, bool store,
                      hipStream_t st) {
  constexpr int HV = HeadVec<T>::HV;
  const LaneGeometry g = lane_geometry(Cp / HV, HEAD_LANE_CAP);
  const int nb = segk_head_blocks(P);
  const size_t lds = (size_t)g.rows * g.cvb * (MAXC * HV + MAXC) * sizeof(float);
  // gy > 1 (more than 64 channel vectors: above 256 channels): blockIdx.y slices the channels; every slice walks the
  // block's pixels and writes its own columns of the partial rows (tests/test_gpu_kernels.py at 288 and 512 channels)
  auto launch_z = [&](auto NCc, auto ZINc, auto STOREc) {
    constexpr int NC = decltype(NCc)::value;
    return segk_launch_lds<head_bwd_kernel<T, NC, decltype(ZINc)::value, decltype(STOREc)::value>>(
        "head_bwd", 96 * 1024, dim3(nb, g.gy), dim3(256), lds, st, dlog, (const T*)y, w, (T*)dy, part, P, HW, Cp, C, ncls, g.cvb, g.rows,
        bn ? bn[0] : nullptr, bn ? bn[1] : nullptr, bn ? bn[2] : nullptr, bn ? bn[3] : nullptr, bnpart);
  };
  auto launch = [&](auto NCc) {      // the form without the store exists on the pre-activation input only
    if (!store) return launch_z(NCc, std::true_type{}, std::false_type{});
    return zin ? launch_z(NCc, std::true_type{}, std::true_type{}) : launch_z(NCc, std::false_type{}, std::true_type{});
  };
  if (const int rc = dispatch_head_nc(ncls, launch)) return rc;
  hipLaunchKernelGGL(head_bwd_finalize_kernel, dim3(cdiv(ncls * (C + 1), 4)), dim3(256), 0, st, part, nb, Cp, C, ncls, dw, db);
  SEGK_CHECK_LAUNCH("head_bwd_finalize");
  return 0;
}

// bnpart: also reduce the BatchNorm backward partials of the layer in front; zin: y is that layer's pre-activation;
// store = 0 (zin only): dy is not written (null)
static int head_bwd(const float* dlog, const void* y, const float* w, void* dy, float* part, float* dw, float* db, int B, int H,
                    int W, int Cp, int C, int ncls, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                    const float* bn_rstd, float* bnpart, int zin, int store, int dtype, hipStream_t st) {
  SEGK_REQUIRE(dlog && y && w && (dy || !store) && part && dw && db && B > 0 && H > 0 && W > 0, "head_bwd: bad arguments");
  SEGK_REQUIRE(store || zin, "head_bwd: the form without dy reads the pre-activation");
  SEGK_REQUIRE(ncls >= 1 && ncls <= MAXC && Cp % 32 == 0 && C > 0 && C <= Cp, "head_bwd: bad channels/classes");
  SEGK_REQUIRE_DTYPE("head_bwd", dtype);
  SEGK_REQUIRE(!(bnpart || zin) || (bn_scale && bn_shift && bn_mean && bn_rstd),
               "head_bwd: BatchNorm reductions / a pre-activation input need scale, shift, mean and rstd");
  const long P = (long)B * H * W, HW = (long)H * W;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  const float* bn[4] = {bn_scale, bn_shift, bn_mean, bn_rstd};
  const float* const* bnp = (bnpart || zin) ? bn : nullptr;
  return by_dtype(dtype, [&](auto Tc) {
    return head_bwd_t<decltype(Tc)>(dlog, y, w, dy, part, dw, db, P, HW, Cp, C, ncls, bnp, bnpart, zin != 0, store != 0, st);
  });
}
extern "C" int segk_head_bwd(const float* dlogits, const void* y, const float* w, void* dy, float* part, float* dw, float* db,
                             int B, int H, int W, int Cp, int C, int ncls, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("head_bwd", dtype);
  return head_bwd(dlogits, y, w, dy, part, dw, db, B, H, W, Cp, C, ncls, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, dtype,
                  (hipStream_t)s);
}
extern "C" int segk_head_bwd_blocks(long P) { return segk_head_blocks(P); }
extern "C" int segk_head_bwd_bnstat(const float* dlogits, const void* y, const float* w, void* dy, float* part, float* dw,
                                    float* db, int B, int H, int W, int Cp, int C, int ncls, const float* scale,
                                    const float* shift, const float* mean, const float* rstd, float* bnpart, int dtype,
                                    segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("head_bwd_bnstat", dtype);
  SEGK_REQUIRE(bnpart, "head_bwd_bnstat: null partials");
  return head_bwd(dlogits, y, w, dy, part, dw, db, B, H, W, Cp, C, ncls, scale, shift, mean, rstd, bnpart, 0, 1, dtype,
                  (hipStream_t)s);
}
extern "C" int segk_head_bwd_bn(const float* dlogits, const void* z, const float* w, void* dy, float* part, float* dw, float* db,
                                int B, int H, int W, int Cp, int C, int ncls, const float* scale, const float* shift,
                                const float* mean, const float* rstd, float* bnpart, int dtype, segk_stream_t s) {
  SEGK_REQUIRE(scale && shift && mean && rstd, "head_bwd_bn: null BatchNorm vectors");
  return head_bwd(dlogits, z, w, dy, part, dw, db, B, H, W, Cp, C, ncls, scale, shift, mean, rstd, bnpart, 1, 1, dtype,
                  (hipStream_t)s);
}
extern "C" int segk_head_bwd_bn_stats(const float* dlogits, const void* z, const float* w, float* part, float* dw, float* db, int B,
                                      int H, int W, int Cp, int C, int ncls, const float* scale, const float* shift,
                                      const float* mean, const float* rstd, float* bnpart, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("head_bwd_bn_stats", dtype);
  SEGK_REQUIRE(scale && shift && mean && rstd && bnpart, "head_bwd_bn_stats: null BatchNorm vectors / partials");
  return head_bwd(dlogits, z, w, nullptr, part, dw, db, B, H, W, Cp, C, ncls, scale, shift, mean, rstd, bnpart, 1, 0, dtype,
                  (hipStream_t)s);
}

template <typename T>
static int head_bn_bwd_apply_t(const float* dlog, const void* z, const float* w, void* dz, const float* const* bn,
                               const float* coef, long P, long HW, int Cp, int C, int ncls, hipStream_t st) {
  const LaneGeometry g = lane_geometry(Cp / HeadVec<T>::HV, HEAD_LANE_CAP);       // head_bwd_t's
  dispatch_head_nc(ncls, [&](auto NCc) {
    hipLaunchKernelGGL((head_bn_bwd_apply_kernel<T, decltype(NCc)::value>), dim3(apply_blocks(P, g.rows), g.gy), dim3(256), 0, st, dlog,
                       (const T*)z, w, (T*)dz, bn[0], bn[1], bn[2], bn[3], coef, P, HW, Cp, C, ncls, g.cvb, g.rows);
  });
  SEGK_CHECK_LAUNCH("head_bn_bwd_apply");
  return 0;
}
extern "C" int segk_head_bn_bwd_apply(const float* dlogits, const void* z, const float* w, void* dz, const float* scale,
                                      const float* shift, const float* mean, const float* rstd, int B, int H, int W, int Cp,
                                      int C, int ncls, const float* bnpart, int nb, float* dgamma, float* dbeta, float* coef,
                                      int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("head_bn_bwd_apply", dtype);
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(dlogits && z && w && dz && dz != z && scale && shift && mean && rstd && bnpart && dgamma && dbeta && coef &&
                   B > 0 && H > 0 && W > 0 && nb > 0,
               "head_bn_bwd_apply: bad arguments");
  SEGK_REQUIRE(ncls >= 1 && ncls <= MAXC && Cp % 32 == 0 && C > 0 && C <= Cp, "head_bn_bwd_apply: bad channels/classes");
  const long P = (long)B * H * W, HW = (long)H * W;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  if (const int rc = segk_bn_bwd_finalize_launch(bnpart, nb, Cp, C, P, dgamma, dbeta, coef, st)) return rc;
  const float* bn[4] = {scale, shift, mean, rstd};
  return by_dtype(dtype, [&](auto Tc) { return head_bn_bwd_apply_t<decltype(Tc)>(dlogits, z, w, dz, bn, coef, P, HW, Cp, C, ncls, st); });
}
