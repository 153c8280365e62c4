// The prediction finishers over network-output slots and finished masks (reference segmentation_webapp/app.py:250-326 for the
// single view).  Each turns its input into a uint8 class mask [oh,ow] with optional RGB
// [oh,ow,3], class counts and confusion counts without ever storing full-size logits; they differ only in how a pixel's
// class is produced, and everything after that is the MaskSink of predict_common.hpp:
//   predict_mask    one slot window, crop + resize (the arithmetic of crop_resize_kernel) -> argmax
//   predict_merge   V views with flips, weighted sum of logits or probabilities -> argmax (+ confidence, scores)
//   mask_finish     a mask dword read back (after the clean-up of components.hip)
// predict_tiles, the fourth, sits in tiles.hip beside the axis arithmetic it needs.
#include "predict_common.hpp"

namespace {

// 1 + 3 bytes leave per pixel where crop_resize + argmax + palette index move ~50, and the source is a C*T*T*4-byte slot that
// stays in L2.  A thread's four pixels are consecutive in a row until it steps over a row end, so (oy, ox) advance per pixel
// and the row's taps are recomputed only there.
template <int NC, int MODE, bool LAB>
__global__ __launch_bounds__(256) void predict_mask_kernel(const float* __restrict__ slot, uint8_t* __restrict__ mask,
                                                           uint8_t* __restrict__ color, const uint8_t* __restrict__ palette,
                                                           unsigned long long* __restrict__ counts,
                                                           const long long* __restrict__ labels, unsigned long long* __restrict__ M,
                                                           int C, int T, int pt, int pl, int nh, int nw, int oh, int ow) {
  using Sink = MaskSink<NC, LAB>;
  __shared__ unsigned int hist[Sink::HIST];
  typename Sink::Regs regs;
  const int total = oh * ow;
  Sink sink(regs, hist, mask, color, palette, counts, labels, M, nullptr, nullptr, C, total);
  const float sh = (float)nh / (float)oh, sw = (float)nw / (float)ow;
  const char* wk[NC];
  window_origins<NC>(slot, C, T, pt, pl, wk);
  const unsigned pitch = 4u * (unsigned)T;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 4 < total; q += (long)gridDim.x * 256) {
    const int p = (int)(q * 4);
    sink.begin(p);
    int oy = p / ow, ox = p - oy * ow;
    RowTaps row = row_taps<MODE>(oy, sh, nh);
    int best[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[NC];
      sample_window<NC, MODE>(wk, pitch, row, ox, sw, nw, v);
      best[j] = argmax_first<NC>(v);
      if (p + j + 1 < total && ++ox == ow) { ox = 0; ++oy; row = row_taps<MODE>(oy, sh, nh); }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sink.account(j, best[j], sink.live(j));
    sink.store();
  }
  sink.finish();
}

// Multi-view prediction: predict_mask_kernel with an accumulator.  A thread walks the views in table order
// over acc[4][NC]; per view it samples the view's window at the FLIPPED pixel, turns logits into probabilities where the
// merge asks for it, and adds weight * s.  A view's descriptor is indexed by the loop counter alone, so it is read with
// uniform loads into scalar registers, and its per-class window origins are scalar too.  The slots (V*C*T*T*4 bytes) stay
// in L2; 1 + 3 + 1 bytes leave per pixel.
template <int NC, int MODE, bool LAB>
__global__ __launch_bounds__(256) void predict_merge_kernel(const segk_view_desc* __restrict__ views, int V, int C, int merge,
                                                            int oh, int ow, uint8_t* __restrict__ mask, uint8_t* __restrict__ color,
                                                            const uint8_t* __restrict__ palette,
                                                            unsigned long long* __restrict__ counts,
                                                            const long long* __restrict__ labels, unsigned long long* __restrict__ M,
                                                            uint8_t* __restrict__ conf, float* __restrict__ scores) {
  using Sink = MaskSink<NC, LAB>;
  __shared__ unsigned int hist[Sink::HIST];
  typename Sink::Regs regs;
  const int total = oh * ow;
  Sink sink(regs, hist, mask, color, palette, counts, labels, M, conf, scores, C, total);
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 4 < total; q += (long)gridDim.x * 256) {
    const int p = (int)(q * 4);
    sink.begin(p);
    int oy[4], ox[4];
    four_pixels(p, total, ow, oy, ox);
    float acc[4][NC];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[j][k] = 0.f;
    for (int v = 0; v < V; ++v) {                                  // fixed order: the order is part of the result
      const segk_view_desc d = views[v];                           // uniform: scalar loads
      const float sh = (float)d.nh / (float)oh, sw = (float)d.nw / (float)ow;
      const char* wk[NC];
      window_origins<NC>((const float*)d.slot, C, d.T, d.pad_top, d.pad_left, wk);
      const unsigned pitch = 4u * (unsigned)d.T;
      const bool soft = merge == SEGK_MERGE_PROB && d.kind == 0;
      const float wt = d.weight;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sy = (d.flip & 2) ? oh - 1 - oy[j] : oy[j], sx = (d.flip & 1) ? ow - 1 - ox[j] : ox[j];
        float z[NC];
        sample_window<NC, MODE>(wk, pitch, sy, sx, sh, sw, d.nh, d.nw, z);
        if (soft) softmax_classes<NC>(z, C);
#pragma unroll
        for (int k = 0; k < NC; ++k) acc[j][k] = acc[j][k] + wt * z[k];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sink.merged(j, acc[j], merge);
    sink.store();
  }
  sink.finish();
}

// The colour / counts / confusion outputs of a finished mask: one mask dword in, three colour dwords out.  A
// mask value >= C is coloured black and counted nowhere: for the sink it is class NC (no palette entry) and not live.
template <bool LAB>
__global__ __launch_bounds__(256) void mask_finish_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ color,
                                                          const uint8_t* __restrict__ palette, unsigned long long* __restrict__ counts,
                                                          const long long* __restrict__ labels, unsigned long long* __restrict__ M,
                                                          int C, int total) {
  using Sink = MaskSink<SEGK_MAX_CLASSES, LAB, false>;
  __shared__ unsigned int hist[Sink::HIST];
  typename Sink::Regs regs;
  Sink sink(regs, hist, nullptr, color, palette, counts, labels, M, nullptr, nullptr, C, total);
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q * 4 < total; q += (long)gridDim.x * 256) {
    const int p = (int)(q * 4);
    unsigned w;
    if (p + 3 < total) w = *(const uint32_t*)(mask + (unsigned)p);
    else {
      w = 0;
      for (int j = 0; j < 4; ++j)
        if (p + j < total) w |= (unsigned)mask[p + j] << (8 * j);
    }
    sink.begin(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = (w >> (8 * j)) & 255;
      sink.account(j, v < C ? v : SEGK_MAX_CLASSES, (sink.live(j) && v < C) ? 1u : 0u);
    }
    sink.store();
  }
  sink.finish();
}

}  // namespace

static_assert(sizeof(segk_view_desc) == 48, "segk_view_desc is 48 bytes (image_segmentation_amd/tta.py: VIEW_DESC)");

extern "C" int segk_predict_mask(const float* slot, uint8_t* mask, uint8_t* color, const uint8_t* palette, uint64_t* counts,
                                 const int64_t* labels, uint64_t* M, int C, int T, int pad_top, int pad_left, int nh, int nw,
                                 int oh, int ow, int mode, segk_stream_t s) {
  SEGK_REQUIRE(slot && mask && T > 0 && nh > 0 && nw > 0 && oh > 0 && ow > 0, "predict_mask: bad shape");
  SEGK_REQUIRE(C >= 1 && C <= SEGK_MAX_CLASSES, "predict_mask: 1..%d classes supported, got %d", SEGK_MAX_CLASSES, C);
  if (int rc = check_output_pairs("predict_mask", color, palette, labels, M)) return rc;
  SEGK_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_top + nh <= T && pad_left + nw <= T, "predict_mask: window outside the slot");
  SEGK_REQUIRE(mode == 0 || mode == 1, "predict_mask: bad mode %d", mode);
  SEGK_REQUIRE((long)T * T < (1L << 30) && (long)oh * ow < (1L << 31) - 4, "predict_mask: slot or output too large for 32-bit offsets");
  if (int rc = check_output_alignment("predict_mask", false, mask, color, nullptr, nullptr)) return rc;
  const int g = finisher_grid((long)oh * ow, counts || labels);
  hipStream_t st = (hipStream_t)s;
  auto launch = [&](auto nc, auto md, auto lab) {
    hipLaunchKernelGGL((predict_mask_kernel<decltype(nc)::value, decltype(md)::value, decltype(lab)::value>), dim3(g), dim3(256), 0, st,
                       slot, mask, color, palette, (unsigned long long*)counts, (const long long*)labels, (unsigned long long*)M, C, T,
                       pad_top, pad_left, nh, nw, oh, ow);
  };
  auto by_lab = [&](auto nc, auto md) {
    if (labels) launch(nc, md, std::true_type{});
    else launch(nc, md, std::false_type{});
  };
  dispatch_classes(C, [&](auto nc) {
    if (mode == 0) by_lab(nc, std::integral_constant<int, 0>{});
    else by_lab(nc, std::integral_constant<int, 1>{});
  });
  SEGK_CHECK_LAUNCH("predict_mask");
  return 0;
}

extern "C" int segk_predict_merge(const void* views_dev, int V, int C, int merge, int mode, int oh, int ow, uint8_t* mask,
                                  uint8_t* color, const uint8_t* palette, uint64_t* counts, const int64_t* labels, uint64_t* M,
                                  uint8_t* conf, float* scores, segk_stream_t s) {
  SEGK_REQUIRE(views_dev && mask && oh > 0 && ow > 0, "predict_merge: bad shape");
  SEGK_REQUIRE(V >= 1 && V <= SEGK_MAX_VIEWS, "predict_merge: 1..%d views supported, got %d", SEGK_MAX_VIEWS, V);
  SEGK_REQUIRE(C >= 1 && C <= SEGK_MAX_CLASSES, "predict_merge: 1..%d classes supported, got %d", SEGK_MAX_CLASSES, C);
  SEGK_REQUIRE(merge == SEGK_MERGE_PROB || merge == SEGK_MERGE_LOGIT, "predict_merge: bad merge %d", merge);
  SEGK_REQUIRE(mode == 0 || mode == 1, "predict_merge: bad mode %d", mode);
  if (int rc = check_output_pairs("predict_merge", color, palette, labels, M)) return rc;
  SEGK_REQUIRE((long)oh * ow < (1L << 31) - 4, "predict_merge: output too large for 32-bit offsets");
  SEGK_REQUIRE(((uintptr_t)views_dev & 15) == 0, "predict_merge: the view table must be 16-byte aligned");
  if (int rc = check_output_alignment("predict_merge", true, mask, color, conf, scores)) return rc;
  const int g = finisher_grid((long)oh * ow, counts || labels);
  hipStream_t st = (hipStream_t)s;
  auto launch = [&](auto nc, auto md, auto lab) {
    hipLaunchKernelGGL((predict_merge_kernel<decltype(nc)::value, decltype(md)::value, decltype(lab)::value>), dim3(g), dim3(256), 0, st,
                       (const segk_view_desc*)views_dev, V, C, merge, oh, ow, mask, color, palette, (unsigned long long*)counts,
                       (const long long*)labels, (unsigned long long*)M, conf, scores);
  };
  auto by_lab = [&](auto nc, auto md) {
    if (labels) launch(nc, md, std::true_type{});
    else launch(nc, md, std::false_type{});
  };
  dispatch_classes(C, [&](auto nc) {
    if (mode == 0) by_lab(nc, std::integral_constant<int, 0>{});
    else by_lab(nc, std::integral_constant<int, 1>{});
  });
  SEGK_CHECK_LAUNCH("predict_merge");
  return 0;
}

extern "C" int segk_mask_finish(const uint8_t* mask, uint8_t* color, const uint8_t* palette, uint64_t* counts, const int64_t* labels,
                                uint64_t* M, int C, int H, int W, segk_stream_t s) {
  SEGK_REQUIRE(mask && H >= 1 && W >= 1, "mask_finish: bad shape");
  SEGK_REQUIRE(C >= 1 && C <= SEGK_MAX_CLASSES, "mask_finish: 1..%d classes supported, got %d", SEGK_MAX_CLASSES, C);
  if (int rc = check_output_pairs("mask_finish", color, palette, labels, M)) return rc;
  SEGK_REQUIRE(color || counts || M, "mask_finish: no output asked for");
  SEGK_REQUIRE((long)H * W < (1L << 31) - 4, "mask_finish: mask too large for 32-bit offsets");
  if (int rc = check_output_alignment("mask_finish", false, mask, color, nullptr, nullptr)) return rc;
  const int g = finisher_grid((long)H * W, counts || labels);
  hipStream_t st = (hipStream_t)s;
  auto launch = [&](auto lab) {
    hipLaunchKernelGGL(mask_finish_kernel<decltype(lab)::value>, dim3(g), dim3(256), 0, st, mask, color, palette,
                       (unsigned long long*)counts, (const long long*)labels, (unsigned long long*)M, C, H * W);
  };
  if (labels) launch(std::true_type{});
  else launch(std::false_type{});
  SEGK_CHECK_LAUNCH("mask_finish");
  return 0;
}
