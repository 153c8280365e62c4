// Reconstruction head and MSE loss of the autoencoder pretraining stage (reference autoencoder/autoencoder.py:188-191,
// nn.MSELoss as autoencoder.ipynb constructs it and utils/training.py:141,234 calls it).
//
//  recon_head_fwd_kernel   rec[B,Cout,H,W] fp32 = sigmoid(bias + conv3x3_pad1(x)), x an act tensor [B,H,W,Cp].  A 32x32
//                          output tile per block; its 34x34 input window is staged through LDS one channel chunk at a time
//                          (each input byte is read once from memory, neighbours come from LDS), the next chunk's loads are
//                          in flight while the current one is consumed.  bf16: packed dot products (v_dot2_f32_bf16) of
//                          channel pairs against the bf16-rounded weights; fp32: fp32 FMAs on the unrounded operands.
//  sigmoid_bwd_act_kernel  dz[B,H,W,Cp] (compute dtype, padding channels zero) = drec * (1 - rec) * rec, ATen's order.
//  mse_part_kernel +       scale * sum((a - b)^2): fixed per-block fp64 partials, then one block sums them in fixed order.
//  mse_final_kernel        The block count depends on n only, so the value is the same on every run and every device.
//  mse_bwd_kernel          da = (norm * (a - b)) * g (norm = 2 scale as ATen rounds it; g read on the device), db = -da.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

namespace {

constexpr int RT = 32;                 // output tile: RT x RT pixels, 256 threads of RPT rows each
constexpr int RPT = 4;
constexpr int HALO = RT + 2;           // staged input window
constexpr int NPIX = HALO * HALO;
constexpr int PW = 8;                  // dwords of one pixel's channel chunk (8 fp32 / 16 bf16 channels)
constexpr int PP = PW + 4;             // LDS pitch per pixel: 48 bytes keep a wave's 16-byte reads on disjoint banks
constexpr int NV = (NPIX * 2 + 255) / 256;     // 16-byte loads per thread per chunk
constexpr int NW = PW * 9 * 4;         // weight dwords per chunk: [pair or channel][tap][4 output channels]

template <typename T>
__global__ __launch_bounds__(256) void recon_head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ rec,
                                                             int H, int W, int Cp, int Cin, int Cout, int COG, int tiles_x) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int CK = BF ? 16 : 8;      // channels per chunk
  __shared__ uint4 s_x[NPIX * PP / 4];
  __shared__ uint4 s_w[NW / 4];
  const int tid = threadIdx.x;
  const int tx0 = (blockIdx.x % tiles_x) * RT, ty0 = (blockIdx.x / tiles_x) * RT;
  const int b = blockIdx.y, co0 = blockIdx.z * COG;
  const int lx = tid & 31, ly = (tid >> 5) * RPT;
  const char* xb = (const char*)x + (size_t)b * H * W * Cp * sizeof(T);
  const int nchunks = (Cin + CK - 1) / CK;

  uint4 v[NV];
  uint32_t wv[2];
  // issue the loads of chunk q: out-of-image pixels and absent weights read a valid address and are zeroed on store
  auto fetch = [&](int q) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int e = tid + k * 256;
      const int p = (e >> 1) < NPIX ? (e >> 1) : NPIX - 1;
      int gy = ty0 - 1 + p / HALO, gx = tx0 - 1 + p % HALO;
      gy = gy < 0 ? 0 : (gy >= H ? H - 1 : gy);
      gx = gx < 0 ? 0 : (gx >= W ? W - 1 : gx);
      v[k] = *(const uint4*)(xb + ((size_t)gy * W + gx) * Cp * sizeof(T) + (size_t)q * 32 + (e & 1) * 16);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = tid + k * 256;              // e = (j * 9 + tap) * 4 + c
      const int c = e & 3, tap = (e >> 2) % 9, j = (e >> 2) / 9;
      const int co = co0 + c;
      const int ci = q * CK + (BF ? 2 * j : j);
      const bool ok0 = e < NW && c < COG && co < Cout && ci < Cin;
      const bool ok1 = BF && e < NW && c < COG && co < Cout && ci + 1 < Cin;
      const float w0 = w[ok0 ? ((size_t)co * Cin + ci) * 9 + tap : 0];
      const float w1 = w[ok1 ? ((size_t)co * Cin + ci + 1) * 9 + tap : 0];
      if (BF)
        wv[k] = cvt_pk_bf16(ok0 ? w0 : 0.f, ok1 ? w1 : 0.f);
      else
        wv[k] = __float_as_uint(ok0 ? w0 : 0.f);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int e = tid + k * 256;
      const int p = e >> 1;
      if (p < NPIX) {
        const int gy = ty0 - 1 + p / HALO, gx = tx0 - 1 + p % HALO;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        s_x[p * (PP / 4) + (e & 1)] = in ? v[k] : make_uint4(0, 0, 0, 0);   // exact-zero halo
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (tid + k * 256 < NW) ((uint32_t*)s_w)[tid + k * 256] = wv[k];
  };

  float acc[RPT][4];
#pragma unroll
  for (int i = 0; i < RPT; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;

  fetch(0);
  for (int q = 0; q < nchunks; ++q) {
    __syncthreads();                   // the previous chunk's LDS reads are done
    stage();
    __syncthreads();
    if (q + 1 < nchunks) fetch(q + 1);
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      uint4 xv[RPT + 2][2];
#pragma unroll
      for (int r = 0; r < RPT + 2; ++r) {
        const int p = (ly + r) * HALO + lx + dx;
        xv[r][0] = s_x[p * (PP / 4)];
        xv[r][1] = s_x[p * (PP / 4) + 1];
      }
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int tap = dy * 3 + dx;
        uint4 wq[PW];
#pragma unroll
        for (int j = 0; j < PW; ++j) wq[j] = s_w[j * 9 + tap];      // wave-uniform address: a broadcast read
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
          const uint32_t* xr = (const uint32_t*)&xv[i + dy][0];
#pragma unroll
          for (int j = 0; j < PW; ++j) {
            const uint32_t wc[4] = {wq[j].x, wq[j].y, wq[j].z, wq[j].w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if constexpr (BF) {
                acc[i][c] = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2v, xr[j]),
                                                            __builtin_bit_cast(bf16x2v, wc[c]), acc[i][c], false);
              } else {
                acc[i][c] = __builtin_fmaf(__uint_as_float(xr[j]), __uint_as_float(wc[c]), acc[i][c]);
              }
            }
          }
        }
      }
    }
  }

  const int gx = tx0 + lx;
  if (gx >= W) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int co = co0 + c;
    if (c >= COG || co >= Cout) break;
    const float bc = bias ? bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
      const int gy = ty0 + ly + i;
      if (gy < H) {
        const float z = bc + acc[i][c];
        rec[(((size_t)b * Cout + co) * H + gy) * W + gx] = 1.f / (1.f + expf(-z));
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sigmoid_bwd_act_kernel(const float* __restrict__ drec, const float* __restrict__ rec,
                                                              T* __restrict__ dz, unsigned P, unsigned HW, int C, int Cp) {
  constexpr int VEC = ET<T>::VEC;
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= P) return;
  const unsigned b = p / HW, hw = p - b * HW;
  const size_t base = (size_t)b * C * HW + hw;
  T* out = dz + (size_t)p * Cp;
  const int nvl = (C + VEC - 1) / VEC;
  for (int vq = 0; vq < nvl; ++vq) {
    float g[VEC], r[VEC], f[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {                 // all loads first (clamped channel), then the arithmetic
      const int c = vq * VEC + e;
      const size_t off = base + (size_t)(c < C ? c : C - 1) * HW;
      g[e] = drec[off];
      r[e] = rec[off];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = vq * VEC + e < C ? g[e] * (1.f - r[e]) * r[e] : 0.f;
    *(uint4*)(out + vq * VEC) = pack16<T>(f);
  }
  for (int vq = nvl; vq < Cp / VEC; ++vq) *(uint4*)(out + vq * VEC) = make_uint4(0, 0, 0, 0);
}

constexpr int MSE_MAX_BLOCKS = SEGK_MSE_PART_FLOATS / 2;     // fp64 partials
constexpr int MSE_UNROLL = 8;

__device__ __forceinline__ double block_sum_f64(double s, double* sh) {
  sh[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void mse_part_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       double* __restrict__ part, long n) {
  __shared__ double sh[256];
  const long stride = (long)gridDim.x * 256;
  double s = 0.0;
  for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += stride * MSE_UNROLL) {
    float d[MSE_UNROLL];
#pragma unroll
    for (int k = 0; k < MSE_UNROLL; ++k) {          // clamped loads stay in flight together
      const long i = i0 + k * stride;
      const long j = i < n ? i : n - 1;
      d[k] = a[j] - b[j];
    }
#pragma unroll
    for (int k = 0; k < MSE_UNROLL; ++k)
      if (i0 + k * stride < n) s += (double)(d[k] * d[k]);
  }
  const double t = block_sum_f64(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void mse_final_kernel(const double* __restrict__ part, int nb, double scale,
                                                        float* __restrict__ out) {
  __shared__ double sh[256];
  const int i0 = threadIdx.x, i1 = threadIdx.x + 256;          // nb <= 512: two partials per thread, fixed order
  const double p0 = part[i0 < nb ? i0 : 0], p1 = part[i1 < nb ? i1 : 0];
  const double s = (i0 < nb ? p0 : 0.0) + (i1 < nb ? p1 : 0.0);
  const double t = block_sum_f64(s, sh);
  if (threadIdx.x == 0) out[0] = (float)(t * scale);
}

__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ gout, float* __restrict__ da,
                                                      float* __restrict__ db, long n, float norm) {
  const float g = gout[0];
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float v = (norm * (a[i] - b[i])) * g;
    da[i] = v;
    if (db) db[i] = -v;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
int segk_mse_blocks(long n) {
  const long g = (n + 256L * MSE_UNROLL * 2 - 1) / (256L * MSE_UNROLL * 2);
  return (int)(g < 1 ? 1 : (g > MSE_MAX_BLOCKS ? MSE_MAX_BLOCKS : g));
}

extern "C" int segk_recon_head_fwd(const void* x, const float* w, const float* bias, float* rec, int B, int H, int W, int Cp,
                                   int Cin, int Cout, int dtype, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE_DTYPE("recon_head_fwd", dtype);
  SEGK_REQUIRE(x && w && rec && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "recon_head_fwd: bad arguments");
  SEGK_REQUIRE(Cp % 32 == 0 && Cin <= Cp, "recon_head_fwd: Cp=%d must be a multiple of 32 holding Cin=%d", Cp, Cin);
  SEGK_REQUIRE(((uintptr_t)x & 15) == 0, "recon_head_fwd: the act tensor must be 16-byte aligned");
  SEGK_REQUIRE(B < 65536 && (long long)B * H * W * Cp < (1LL << 40) && (long long)Cout * Cin * 9 < (1LL << 31),
               "recon_head_fwd: shape too large");
  const int COG = Cout < 4 ? Cout : 4;
  const int tiles_x = cdiv(W, RT), tiles_y = cdiv(H, RT), groups = cdiv(Cout, COG);
  SEGK_REQUIRE((long long)tiles_x * tiles_y < (1LL << 31) && groups < 65536, "recon_head_fwd: grid too large");
  const dim3 grid(tiles_x * tiles_y, B, groups);
  if (dtype == SEGK_DT_BF16)
    hipLaunchKernelGGL(recon_head_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, w, bias, rec, H, W, Cp, Cin,
                       Cout, COG, tiles_x);
  else
    hipLaunchKernelGGL(recon_head_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)x, w, bias, rec, H, W, Cp, Cin,
                       Cout, COG, tiles_x);
  SEGK_CHECK_LAUNCH("recon_head_fwd");
  return 0;
}

extern "C" int segk_recon_sigmoid_bwd(const float* drec, const float* rec, void* dz, int B, int H, int W, int C, int Cp,
                                      int dtype, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE_DTYPE("recon_sigmoid_bwd", dtype);
  SEGK_REQUIRE(drec && rec && dz && B > 0 && H > 0 && W > 0 && C > 0, "recon_sigmoid_bwd: bad arguments");
  SEGK_REQUIRE(Cp % 32 == 0 && C <= Cp, "recon_sigmoid_bwd: Cp=%d must be a multiple of 32 holding C=%d", Cp, C);
  SEGK_REQUIRE(((uintptr_t)dz & 15) == 0, "recon_sigmoid_bwd: dz must be 16-byte aligned");
  const long long P = (long long)B * H * W;
  SEGK_REQUIRE(P < (1LL << 31), "recon_sigmoid_bwd: pixels are indexed with 32 bits: %lld pixels", P);
  const dim3 grid((unsigned)((P + 255) / 256));
  if (dtype == SEGK_DT_BF16)
    hipLaunchKernelGGL(sigmoid_bwd_act_kernel<bf16_t>, grid, dim3(256), 0, st, drec, rec, (bf16_t*)dz, (unsigned)P,
                       (unsigned)((long long)H * W), C, Cp);
  else
    hipLaunchKernelGGL(sigmoid_bwd_act_kernel<float>, grid, dim3(256), 0, st, drec, rec, (float*)dz, (unsigned)P,
                       (unsigned)((long long)H * W), C, Cp);
  SEGK_CHECK_LAUNCH("recon_sigmoid_bwd");
  return 0;
}

extern "C" int segk_mse_fwd(const float* a, const float* b, float* part, int part_floats, float* out, long n, int mean,
                            segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(a && b && part && out && n > 0 && part_floats > 0, "mse_fwd: bad arguments");
  SEGK_REQUIRE(mean == 0 || mean == 1, "mse_fwd: mean must be 0 (sum) or 1 (mean), got %d", mean);
  SEGK_REQUIRE(((uintptr_t)part & 7) == 0, "mse_fwd: part must be 8-byte aligned (it holds fp64 partials)");
  const int nb = segk_mse_blocks(n);
  SEGK_REQUIRE(part_floats >= 2 * nb, "mse_fwd: part holds %d floats, %d needed", part_floats, 2 * nb);
  hipLaunchKernelGGL(mse_part_kernel, dim3(nb), dim3(256), 0, st, a, b, (double*)part, n);
  SEGK_CHECK_LAUNCH("mse_part");
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nb, mean ? 1.0 / (double)n : 1.0, out);
  SEGK_CHECK_LAUNCH("mse_final");
  return 0;
}

extern "C" int segk_mse_bwd(const float* a, const float* b, const float* gout, float* da, float* db, long n, int mean,
                            segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(a && b && gout && da && n > 0, "mse_bwd: bad arguments");
  SEGK_REQUIRE(mean == 0 || mean == 1, "mse_bwd: mean must be 0 (sum) or 1 (mean), got %d", mean);
  const float norm = mean ? (float)(2.0 / (double)n) : 2.0f;      // aten mse_loss_backward: 2/numel (mean) or 2 (sum)
  long g = (n + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)g), dim3(256), 0, st, a, b, gout, da, db, n, norm);
  SEGK_CHECK_LAUNCH("mse_bwd");
  return 0;
}
