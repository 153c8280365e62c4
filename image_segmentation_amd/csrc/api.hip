// Process state (error text, device index, CU count), the version / build-id entries, and the extern "C" entries of
// include/segk.h that assemble ConvArgs, WgradArgs or GemmArgs.  Every other entry is defined in its kernels' file.
#include "common.hpp"
#include "segk_internal.h"
#include "../../include/segk.h"

thread_local char g_segk_err[512] = "";

int segk_device_index() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
  return dev < SEGK_MAX_DEVICES ? dev : SEGK_MAX_DEVICES - 1;
}
int segk_num_cus() {
  static int n[SEGK_MAX_DEVICES] = {};    // racing first calls write the same value
  const int dev = segk_device_index();
  if (n[dev] == 0) {
    hipDeviceProp_t p;
    int v = 0;
    if (hipGetDeviceProperties(&p, dev) == hipSuccess) v = p.multiProcessorCount;
    n[dev] = v >= 8 ? v : 256;
  }
  return n[dev];
}

extern "C" {

#ifndef SEGK_BUILD_ID
#define SEGK_BUILD_ID "unknown"
#endif
int segk_version(void) { return SEGK_ABI_VERSION; }
int segk_entry_count(void) { return SEGK_ENTRY_COUNT; }
const char* segk_build_id(void) { return SEGK_BUILD_ID; }
const char* segk_last_error(void) { return g_segk_err; }

int segk_conv_tiles(int B, int H, int W, int Cin, int Cout, int dtype) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (long long)B * H * W > 0x1fffffffLL) return 0;
  const ConvPlan p = segk_conv_plan(0, dtype, Cin, Cout, W, /*has_bias=*/false, /*gemm_dma=*/false);   // the query does not know the bias
  if (p.rs_rows) return segk_conv_rs_rows(B, H, W, Cout);   // one row per wave slab
  return B * cdiv(W, 1 << p.twl) * cdiv(H, p.bm >> p.twl);
}

int segk_conv3x3(const void* srcA, const void* srcB, const void* wpacked, const float* bias, const float* scale,
                 const float* shift, void* out, void* out2, float* stats, int B, int H, int W, int CA, int CB, int CO1,
                 int CO2, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("conv3x3", dtype);
  ConvArgs a{};
  a.srcA = srcA; a.srcB = srcB; a.w = wpacked; a.bias = bias; a.scale = scale; a.shift = shift;
  a.out = out; a.out2 = out2; a.stats = stats;
  a.B = B; a.H = H; a.W = W; a.CA = CA; a.CB = CB; a.Ntot = CO1 + CO2; a.CO1 = CO1; a.CO2 = CO2;
  return segk_conv_igemm_launch(a, 0, dtype, (hipStream_t)s);
}

int segk_conv_writes_act_q(int Cin, int Cout, int dtype) { return segk_conv_writes_act(Cin, Cout, dtype); }

int segk_stem3x3_rows(int B, int H, int W, int Cin, int Cout, int dtype) { return segk_stem_rows(B, H, W, Cin, Cout, dtype); }
int segk_stem3x3_wgrad_slabs(int B, int H, int W, int Cin, int Cout, int dtype) {
  return segk_stem_wgrad_slabs(B, H, W, Cin, Cout, dtype);
}
int segk_stem3x3_wgrad(const float* x_nchw, const void* dz, float* slabs, int B, int H, int W, int Cin, int Cout, int dtype,
                       segk_stream_t s) {
  SEGK_REQUIRE(dtype == SEGK_DT_BF16, "stem3x3_wgrad: bf16 only (dtype %d)", dtype);
  return segk_stem_wgrad_launch(x_nchw, dz, slabs, B, H, W, Cin, Cout, (hipStream_t)s);
}
int segk_stem3x3_wgrad_bn(const float* x_nchw, const void* da, const void* z, const float* scale, const float* shift,
                          const float* mean, const float* rstd, const float* coef, float* slabs, int B, int H, int W, int Cin,
                          int Cout, int dtype, segk_stream_t s) {
  SEGK_REQUIRE(dtype == SEGK_DT_BF16, "stem3x3_wgrad_bn: bf16 only (dtype %d)", dtype);
  const float* bn[4] = {scale, shift, mean, rstd};
  return segk_stem_wgrad_bn_launch(x_nchw, da, z, bn, coef, slabs, B, H, W, Cin, Cout, (hipStream_t)s);
}
int segk_stem3x3(const float* x_nchw, const float* w_oihw, void* z, void* x_nhwc, float* stats, int B, int H, int W, int Cin,
                 int Cout, int dtype, segk_stream_t s) {
  SEGK_REQUIRE(dtype == SEGK_DT_BF16, "stem3x3: bf16 only (dtype %d)", dtype);
  return segk_stem_launch(x_nchw, w_oihw, z, x_nhwc, stats, B, H, W, Cin, Cout, (hipStream_t)s);
}

int segk_conv3x3_act(const void* srcA, const void* wpacked, const float* scale, const float* shift, void* out,
                     void* act_out, float* stats, int B, int H, int W, int CA, int CO, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("conv3x3_act", dtype);
  ConvArgs a{};
  a.srcA = srcA; a.w = wpacked; a.scale = scale; a.shift = shift; a.out = out; a.act_out = act_out; a.stats = stats;
  a.B = B; a.H = H; a.W = W; a.CA = CA; a.Ntot = CO; a.CO1 = CO;
  return segk_conv_igemm_launch(a, 0, dtype, (hipStream_t)s);
}

int segk_conv1x1(const void* srcA, const void* wpacked, const float* bias, void* out, int B, int H, int W, int CA,
                 int CO, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("conv1x1", dtype);
  ConvArgs a{};
  a.srcA = srcA; a.w = wpacked; a.bias = bias; a.out = out;
  a.B = B; a.H = H; a.W = W; a.CA = CA; a.Ntot = CO; a.CO1 = CO;
  return segk_conv_igemm_launch(a, 1, dtype, (hipStream_t)s);
}

int segk_linear(const void* rows, const void* wpacked, const float* bias, void* out, long M, int K, int N, int act,
                int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("linear", dtype);
  // [M][K] x [K][N] (+ bias, optional quick_gelu): the 1x1-convolution GEMM over a 16-pixel-wide strip of M/16 rows
  SEGK_REQUIRE(M > 0 && M % 16 == 0 && M / 16 < (1 << 24), "linear: M=%ld must be a positive multiple of 16", M);
  SEGK_REQUIRE(act == 0 || act == 1, "linear: bad activation %d", act);
  ConvArgs a{};
  a.srcA = rows; a.w = wpacked; a.bias = bias; a.out = out;
  a.B = 1; a.H = (int)(M / 16); a.W = 16; a.CA = K; a.Ntot = N; a.CO1 = N; a.act = act;
  return segk_conv_igemm_launch(a, 1, dtype, (hipStream_t)s);
}

int segk_linear_splitk(const void* rows, const void* wpacked, const float* bias, void* out_parts, long M, int K, int N,
                       int ksplit, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("linear_splitk", dtype);
  // bf16 only: `ksplit` partial products [ksplit][M][N] (the consumer sums them: segk_add_layernorm_parts)
  SEGK_REQUIRE(dtype == SEGK_DT_BF16, "linear_splitk: bf16 only");
  SEGK_REQUIRE(M > 0 && M % 16 == 0 && K > 0 && K % 64 == 0 && N > 0 && ksplit >= 1, "linear_splitk: bad shape");
  SEGK_REQUIRE(segk_gemm_dma_ok(M, K / 32, K / 32, N, N, K, 0) && (K / 64) % ksplit == 0 && K / 64 / ksplit >= 1,
               "linear_splitk: K=%d does not split %d ways into 64-element stages (or the shape is not served)", K, ksplit);
  GemmArgs g{};
  g.A = rows; g.w = (const char*)wpacked; g.bias = bias; g.out = out_parts;
  g.M = M; g.N = N; g.nchunks = K / 32; g.nchA = K / 32; g.lda = K; g.H = 1; g.W = 1; g.Cout = N;
  g.ksplit = ksplit; g.split_stride = M * (long)N;
  return segk_gemm_dma_launch(g, 0, (hipStream_t)s);
}

int segk_convt2x2_fwd(const void* in, const void* wpacked, const float* bias4, void* out, int B, int H, int W, int Cin,
                      int Cout, int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("convt2x2_fwd", dtype);
  // bias4: per-N bias of length 4*Cout (the layer bias repeated for the four taps) or NULL
  SEGK_REQUIRE(in && wpacked && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "convt2x2_fwd: bad arguments");
  if (segk_convt_stream_ok(B, H, W, Cin, Cout, dtype))      // short K: weights in registers, no LDS, no unit boundary
    return segk_convt_stream_launch(in, wpacked, bias4, out, B, H, W, Cin, Cout, (hipStream_t)s);
  ConvArgs a{};
  a.srcA = in; a.w = wpacked; a.bias = bias4; a.out = out;
  a.B = B; a.H = H; a.W = W; a.CA = Cin; a.Ntot = 4 * Cout; a.CO1 = Cout; a.shuffle = 1;
  return segk_conv_igemm_launch(a, 1, dtype, (hipStream_t)s);
}

int segk_convt2x2_dgrad(const void* dout, const void* wpacked, void* din, int B, int H, int W, int Cin, int Cout,
                        int dtype, segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("convt2x2_dgrad", dtype);
  SEGK_REQUIRE(dout && wpacked && din && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "convt2x2_dgrad: bad arguments");
  if (segk_convt_stream_dgrad_ok(B, H, W, Cin, Cout, dtype))
    return segk_convt_stream_dgrad_launch(dout, wpacked, din, B, H, W, Cin, Cout, (hipStream_t)s);
  ConvArgs a{};
  a.srcA = dout; a.w = wpacked; a.out = din;
  a.B = B; a.H = H; a.W = W; a.CA = Cout; a.Ntot = Cin; a.CO1 = Cin; a.unshuf = 1;
  return segk_conv_igemm_launch(a, 1, dtype, (hipStream_t)s);
}

int segk_wgrad(const void* dz, const void* srcA, const void* srcB, const float* scale, const float* shift, float* slabs,
               const void* zeros, int S, int B, int H, int W, int CD, int CA, int CB, int geo, int dtype,
               segk_stream_t s) {
  SEGK_REQUIRE_DTYPE("wgrad", dtype);
  WgradArgs a{};
  a.dz = dz; a.srcA = srcA; a.srcB = srcB; a.scale = scale; a.shift = shift; a.slabs = slabs; a.zeros = zeros;
  a.B = B; a.H = H; a.W = W; a.CD = CD; a.CA = CA; a.CB = CB; a.S = S;
  return segk_wgrad_launch(a, geo, dtype, (hipStream_t)s);
}

}  // extern "C"
