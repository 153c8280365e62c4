// Shared device/host helpers for the segk kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // native vector: stays in registers (SSA)

#define SEGK_DT_F32 0
#define SEGK_DT_BF16 1

// ---- error plumbing (thread-local message, negative return codes; no exceptions cross the ABI)
extern thread_local char g_segk_err[512];
#define SEGK_FAIL(code, ...)                                   \
  do {                                                         \
    snprintf(g_segk_err, sizeof(g_segk_err), __VA_ARGS__);     \
    return (code);                                             \
  } while (0)
#define SEGK_REQUIRE(cond, ...)                                \
  do {                                                         \
    if (!(cond)) SEGK_FAIL(-2, __VA_ARGS__);                   \
  } while (0)
#define SEGK_REQUIRE_DTYPE(name, dtype) \
  SEGK_REQUIRE((dtype) == SEGK_DT_F32 || (dtype) == SEGK_DT_BF16, name ": bad dtype %d", dtype)
#define SEGK_CHECK_LAUNCH(name)                                                        \
  do {                                                                                 \
    hipError_t e_ = hipGetLastError();                                                 \
    if (e_ != hipSuccess) SEGK_FAIL(-3, "%s: launch failed: %s", name, hipGetErrorString(e_)); \
  } while (0)

// ---- element traits: one 16-byte LDS/global vector holds VEC elements
template <typename T> struct ET;
template <> struct ET<float> {
  static constexpr int VEC = 4;     // elements per 16 B
  static constexpr int ES = 4;      // element size
  static constexpr int CH = 16;     // channels per 64-byte K-chunk
};
template <> struct ET<bf16_t> {
  static constexpr int VEC = 8;
  static constexpr int ES = 2;
  static constexpr int CH = 32;
};

__device__ __forceinline__ float bf2f(uint32_t lo16) { return __uint_as_float(lo16 << 16); }

// unpack a 16-byte vector of T into floats
template <typename T> __device__ __forceinline__ void unpack16(const uint4& v, float* f);
template <> __device__ __forceinline__ void unpack16<float>(const uint4& v, float* f) {
  f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
  f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
}
template <> __device__ __forceinline__ void unpack16<bf16_t>(const uint4& v, float* f) {
  f[0] = bf2f(v.x & 0xffffu); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = bf2f(v.y & 0xffffu); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = bf2f(v.z & 0xffffu); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = bf2f(v.w & 0xffffu); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
// Two floats -> one packed bf16 pair (round to nearest even, NaN-preserving): ONE v_cvt_pk_bf16_f32, emitted by the compiler
// from a vector conversion.  Never write this instruction as inline asm on accumulator values: the compiler inserts the
// wait states an MFMA result needs before a VALU read only for instructions it knows -- an asm statement placed right behind
// the MFMA reads the register before the matrix pipe has written it (round 3: the ConvTranspose streaming kernel produced
// garbage as soon as the 64-bit index arithmetic that used to sit between the two was shortened).
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2v){lo, hi}, bf16x2v));
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) { return cvt_pk_bf16(lo, hi); }
template <typename T> __device__ __forceinline__ uint4 pack16(const float* f);
template <> __device__ __forceinline__ uint4 pack16<float>(const float* f) {
  return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
}
template <> __device__ __forceinline__ uint4 pack16<bf16_t>(const float* f) {
  return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                    pack_bf16x2(f[6], f[7]));
}
template <typename T> __device__ __forceinline__ T from_float(float f);
template <> __device__ __forceinline__ float from_float<float>(float f) { return f; }
template <> __device__ __forceinline__ bf16_t from_float<bf16_t>(float f) { return (bf16_t)f; }
template <typename T> __device__ __forceinline__ float to_float(T v);
template <> __device__ __forceinline__ float to_float<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_float<bf16_t>(bf16_t v) { return (float)v; }

// BatchNorm + ReLU backward, one element: dz = scale * (g - c1 - xhat * c2) with g = d where the ReLU was active,
// xhat = (z - mean) * rstd and (c1, c2) = (sum g, sum g * xhat) / N.  Stated ONCE: bn_bwd_apply_kernel and the kernels that
// form dz in registers (head_bn_bwd_apply_kernel, stem_wgrad_kernel<BN>) must agree bit for bit.
__device__ __forceinline__ float bn_relu_bwd_dz(float z, float d, float sc, float sh, float mu, float rs, float c1, float c2) {
  const float g = (fmaf(z, sc, sh) > 0.f) ? d : 0.f;
  const float xh = (z - mu) * rs;
  return sc * (g - c1 - xh * c2);
}
// xhat recovered from y = relu(z * scale + shift) where the ReLU is active: xhat = y * xa + xb = (y - shift) * rstd / scale -
// mean * rstd (a channel with scale == 0 gets xa = 0).  Stated ONCE: the kernels that reduce sum(g * xhat) from the block output
// (maxpool_bwd_kernel<STAT>, head_bwd_kernel) must agree bit for bit.
__device__ __forceinline__ void xhat_from_y(float sc, float sh, float mu, float rs, float& xa, float& xb) {
  xa = sc != 0.f ? rs / sc : 0.f;
  xb = -sh * xa - mu * rs;
}

// Conv epilogue helper: the 16 fp32 results one lane holds of a 32x32 accumulator fragment (one output channel,
// pixel rows (r & 3) + 8 (r >> 2) of the fragment) -> running per-channel (sum, sum of squares) for
// training-mode BatchNorm, and stores into the [pixel][channel] LDS staging tile (row pitch OP bytes).
// Packed fp32 math (v_pk_add_f32 / v_pk_fma_f32) and paired bf16 conversion halve the VALU count; the
// pairwise summation order is fixed, so the statistics stay bit-stable run to run.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ void stage_frag(const float (&v)[16], char* obase, int OP, float& s1, float& s2) {
  f32x2_t p1 = {0.f, 0.f}, p2 = {0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int dm = (r & 3) + 8 * (r >> 2);          // r even: rows dm and dm + 1
    const f32x2_t x = {v[r], v[r + 1]};
    p1 += x;
    p2 = __builtin_elementwise_fma(x, x, p2);
    if constexpr (sizeof(T) == 2) {
      const uint32_t pk = cvt_pk_bf16(x.x, x.y);   // ONE conversion for the pair
      *(uint16_t*)(obase + dm * OP) = (uint16_t)(pk & 0xffffu);
      *(uint16_t*)(obase + (dm + 1) * OP) = (uint16_t)(pk >> 16);
    } else {
      *(float*)(obase + dm * OP) = x.x;
      *(float*)(obase + (dm + 1) * OP) = x.y;
    }
  }
  s1 += p1.x + p1.y;
  s2 += p2.x + p2.y;
}

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1 (inline-asm immediates need constants)
template <int I, int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
  const int x = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
  return v + __int_as_float(x);
}
// sum over the 16 lanes of a DPP row, result in every lane: xor 1, xor 2 (quad permutes), half mirror, mirror -- a fixed tree
__device__ __forceinline__ float row16_sum(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x141>(v);
  v = dpp_add<0x140>(v);
  return v;
}

// XCD-aware block remap: blocks b and b+8 share an XCD (observed round-robin dispatch; speed only).
// Gives each XCD a contiguous range of logical ids so neighbouring tiles share one L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, x = bid & 7, i = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Item index -> (channel vector, x, y, image) in 32-bit arithmetic.  A 64-bit division by a run-time value is a ~130-
// instruction loop on this ISA, and a streaming kernel that decomposes a `long` index per item (five div/mod) spends more
// VALU time on that than on its data; every launcher that uses this checks that its item count is below 2^31.
struct Idx4 { int cv, x, y, b; };
__device__ __forceinline__ Idx4 split4(unsigned i, unsigned CV, unsigned Wc, unsigned Hc) {
  const unsigned p = i / CV, q = p / Wc, b = q / Hc;
  Idx4 r;
  r.cv = (int)(i - p * CV); r.x = (int)(p - q * Wc); r.y = (int)(q - b * Hc); r.b = (int)b;
  return r;
}
// ---- shared by the 8-bit image kernels (augment.hip, perturb.hip)
// splitmix64 finaliser of i + seed * 0x9E3779B97F4A7C15
__device__ __forceinline__ unsigned long long splitmix(unsigned long long seed, unsigned long long i) {
  unsigned long long z = i + seed * 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int m = i % p;
  m = m < 0 ? m + p : m;
  return m < n ? m : p - m;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
