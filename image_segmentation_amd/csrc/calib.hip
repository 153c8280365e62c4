// Confidence calibration (the reference holds no code for it): reliability histograms of an 8-bit
// confidence map, and the temperature sweep -- from one view's network output slot to the reliability statistics and the
// negative log-likelihood of K temperatures at the image's own size, in one pass.  Integer sums only: no float atomics, no
// ticket, no finalize pass; every output is order-independent and bit-stable.
//
// Both kernels follow predict_mask_kernel / predict_merge_kernel (predict.hip): a thread owns four consecutive flat pixels,
// loads are unconditional with clamped indices, histograms live in LDS as 32-bit counters and a block ends with one 64-bit
// global atomic per NON-ZERO bin.  A trained network puts most pixels into q = 255, and 64 lanes adding to one LDS word
// serialise, so the top bin is aggregated per wave before the LDS add: a ballot and a population count, added by one lane.
// The grid-stride loops are wave-uniform (dead pixels are masked, not skipped) so that every ballot sees the whole wave.
// A (count, correct) pair is ONE 64-bit LDS word (count in the low half: the layout of the uint32 [..][256][2] view), so
// a pixel costs one ds_add_u64; no count can carry into the other half because a launch holds fewer than 2^31 pixels.
#include "predict_common.hpp"

namespace {

__device__ __forceinline__ bool label_valid(long long l, int C, int ignore_index) {
  return l >= 0 && l < C && !(ignore_index >= 0 && l == ignore_index);
}

// one lane adds the wave's count of `hit` lanes (and of those that are also `correct`) to a (count, correct) word
__device__ __forceinline__ void add_top(unsigned long long* word, bool hit, bool correct) {
  const unsigned long long n = (unsigned long long)__popcll(__ballot(hit));
  const unsigned long long c = (unsigned long long)__popcll(__ballot(hit && correct));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(word, n | (c << 32));
}

// ---- reliability histogram of (confidence, mask, labels) per predicted class -------------------------------------------
__global__ __launch_bounds__(256) void calib_hist_kernel(const uint8_t* __restrict__ conf, const uint8_t* __restrict__ mask,
                                                         const long long* __restrict__ labels, int total, int C,
                                                         int ignore_index, unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long h[SEGK_MAX_CLASSES * 256];       // [class][q] -> (count, correct)
  for (int i = threadIdx.x; i < C * 256; i += 256) h[i] = 0;
  __syncthreads();
  for (long base = (long)blockIdx.x * 256; base * 4 < total; base += (long)gridDim.x * 256) {
    const long p = (base + threadIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = p + j < total;
      const unsigned i = (unsigned)(live ? p + j : total - 1);
      const long long l = labels[i];
      const unsigned q = conf[i], m = mask[i];
      const bool valid = live && label_valid(l, C, ignore_index);
      const bool correct = (long long)m == l;
      const unsigned cls = m < (unsigned)C ? m : (unsigned)C - 1;     // a mask value past the classes counts under C-1
      const bool top = valid && q == 255;
      for (int k = 0; k < C; ++k) add_top(&h[k * 256 + 255], top && cls == (unsigned)k, correct);
      if (valid && !top) atomicAdd(&h[cls * 256 + q], 1ull | ((unsigned long long)(correct ? 1u : 0u) << 32));
    }
  }
  __syncthreads();
  const unsigned int* w = (const unsigned int*)h;
  for (int i = threadIdx.x; i < C * 512; i += 256)
    if (w[i]) atomicAdd(&hist[i], (unsigned long long)w[i]);
}

// ---- temperature sweep ---------------------------------------------------------------------------------------------------
// z of the thread's four pixels is sampled once with predict_merge_kernel's sampler and argmax (predict_common.hpp: the
// sweep at inv_T = 1 agrees with segk_predict_merge exactly, tests/test_gpu_calibration.py); the K loop then runs over
// registers only, inv_T[j] indexed by the loop counter alone (uniform loads).
// K is a run-time count, so per-temperature sums cannot sit in a register array over the grid-stride loop (an array
// indexed by j would live in scratch).  Per temperature the four pixels' fixed-point NLL (< 2^36) and their non-finite
// count (bits 48..) are one 64-bit word per thread, summed over the wave with shuffles and added by one lane to the
// block's LDS accumulators; a block ends with one global atomic per temperature and counter.
template <int NC, int MODE>
__global__ __launch_bounds__(256) void calib_temps_kernel(const float* __restrict__ slot, int C, int T, int pt, int pl, int nh,
                                                          int nw, int oh, int ow, const long long* __restrict__ labels,
                                                          int ignore_index, const float* __restrict__ inv_T, int K,
                                                          unsigned long long* __restrict__ hist,
                                                          unsigned long long* __restrict__ nll_fx,
                                                          unsigned long long* __restrict__ nonfinite,
                                                          unsigned long long* __restrict__ valid_out) {
  extern __shared__ unsigned long long lds[];
  unsigned long long* h = lds;                       // [K][256] -> (count, correct)
  unsigned long long* nl = lds + K * 256;            // [K] fixed-point NLL
  unsigned long long* nf = nl + K;                   // [K] non-finite NLL count
  for (int i = threadIdx.x; i < K * 258; i += 256) lds[i] = 0;
  __syncthreads();
  const int total = oh * ow;
  const float sh = (float)nh / (float)oh, sw = (float)nw / (float)ow;
  const char* wk[NC];
  window_origins<NC>(slot, C, T, pt, pl, wk);
  const unsigned pitch = 4u * (unsigned)T;
  unsigned int nvalid = 0;
  for (long base = (long)blockIdx.x * 256; base * 4 < total; base += (long)gridDim.x * 256) {
    const long p = (base + threadIdx.x) * 4;
    float z[4][NC];
    int best[4], lab[4];
    bool valid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = p + j < total;
      const int i = (int)(live ? p + j : total - 1);
      const long long l = labels[(unsigned)i];
      valid[j] = live && label_valid(l, C, ignore_index);
      lab[j] = valid[j] ? (int)l : 0;
      nvalid += valid[j] ? 1u : 0u;
      const int oy = i / ow, ox = i - oy * ow;
      sample_window<NC, MODE>(wk, pitch, oy, ox, sh, sw, nh, nw, z[j]);
      best[j] = argmax_first<NC>(z[j]);
    }
    for (int t = 0; t < K; ++t) {
      const float it = inv_T[t];                          // uniform
      unsigned long long* ht = h + t * 256;
      unsigned long long sums = 0;                        // fixed-point NLL | non-finite count << 48
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float s[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) s[k] = z[j][k] * it;
        float mx = s[0];
#pragma unroll
        for (int k = 1; k < NC; ++k) mx = s[k] > mx ? s[k] : mx;
        float sl = s[0];
#pragma unroll
        for (int k = 1; k < NC; ++k) sl = lab[j] == k ? s[k] : sl;
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          s[k] = expf(s[k] - mx);
          S = S + ((NC <= 4 || k < C) ? s[k] : 0.f);
        }
        float ps = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          s[k] = s[k] / S;
          ps = ps + ((NC <= 4 || k < C) ? s[k] : 0.f);
        }
        float pb = s[0];
#pragma unroll
        for (int k = 1; k < NC; ++k) pb = best[j] == k ? s[k] : pb;
        pb = pb / ps;
        const float c = 255.f * pb + 0.5f;
        const unsigned q = c >= 0.f ? (unsigned)(c > 255.f ? 255.f : c) : 0u;      // a NaN confidence is stored as 0
        const float nll = logf(S) - (sl - mx);
        const bool fin = nll < SEGK_CALIB_NLL_MAX;        // false for NaN and +inf too
        const float nn = nll > 0.f ? nll : 0.f;
        const unsigned long long fx = fin ? (unsigned long long)((double)nn * 65536.0 + 0.5) : (1ull << 48);
        sums += valid[j] ? fx : 0ull;
        const bool correct = best[j] == lab[j];
        const bool top = valid[j] && q == 255;
        add_top(&ht[255], top, correct);
        if (valid[j] && !top) atomicAdd(&ht[q], 1ull | ((unsigned long long)(correct ? 1u : 0u) << 32));
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sums += __shfl_xor(sums, o);
      if ((threadIdx.x & 63) == 0 && sums) {
        if (sums & ((1ull << 48) - 1)) atomicAdd(&nl[t], sums & ((1ull << 48) - 1));
        if (sums >> 48) atomicAdd(&nf[t], sums >> 48);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o);
  __shared__ unsigned int vsum;
  if (threadIdx.x == 0) vsum = 0;
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && nvalid) atomicAdd(&vsum, nvalid);
  __syncthreads();
  const unsigned int* w = (const unsigned int*)h;
  for (int i = threadIdx.x; i < K * 512; i += 256)
    if (w[i]) atomicAdd(&hist[i], (unsigned long long)w[i]);
  for (int t = threadIdx.x; t < K; t += 256) {
    if (nl[t]) atomicAdd(&nll_fx[t], nl[t]);
    if (nf[t]) atomicAdd(&nonfinite[t], nf[t]);
  }
  if (threadIdx.x == 0 && vsum) atomicAdd(valid_out, (unsigned long long)vsum);
}

}  // namespace

extern "C" int segk_calib_hist(const uint8_t* conf, const uint8_t* mask, const int64_t* labels, int H, int W, int C,
                               int ignore_index, uint64_t* hist, segk_stream_t s) {
  SEGK_REQUIRE(conf && mask && labels && hist, "calib_hist: NULL confidence, mask, labels or histogram");
  SEGK_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31) - 4, "calib_hist: image of %d x %d (sides positive, H W < 2^31 - 4)", H, W);
  SEGK_REQUIRE(C >= 1 && C <= SEGK_MAX_CLASSES, "calib_hist: 1..%d classes supported, got %d", SEGK_MAX_CLASSES, C);
  SEGK_REQUIRE(ignore_index >= -1, "calib_hist: ignore_index is a class index or -1 (none), got %d", ignore_index);
  SEGK_REQUIRE(((uintptr_t)labels & 7) == 0 && ((uintptr_t)hist & 7) == 0, "calib_hist: labels and hist must be 8-byte aligned");
  long g = (((long)H * W + 3) / 4 + 255) / 256;
  const long cap = 3L * segk_num_cus();                   // as segk_predict_mask: every block ends in atomics on few words
  if (g > cap) g = cap;
  hipLaunchKernelGGL(calib_hist_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)s, conf, mask, (const long long*)labels, H * W, C,
                     ignore_index, (unsigned long long*)hist);
  SEGK_CHECK_LAUNCH("calib_hist");
  return 0;
}

extern "C" int segk_calib_temps(const float* slot, int C, int T, int pad_top, int pad_left, int nh, int nw, int oh, int ow, int mode,
                                const int64_t* labels, int ignore_index, const float* inv_T_dev, int K, uint64_t* hist,
                                uint64_t* nll_fx, uint64_t* nonfinite, uint64_t* valid, segk_stream_t s) {
  SEGK_REQUIRE(slot && labels && inv_T_dev && hist && nll_fx && nonfinite && valid, "calib_temps: NULL slot, labels, table or output");
  SEGK_REQUIRE(T > 0 && nh > 0 && nw > 0 && oh > 0 && ow > 0, "calib_temps: bad shape");
  SEGK_REQUIRE(C >= 1 && C <= SEGK_MAX_CLASSES, "calib_temps: 1..%d classes supported, got %d", SEGK_MAX_CLASSES, C);
  SEGK_REQUIRE(K >= 1 && K <= SEGK_MAX_TEMPS, "calib_temps: 1..%d temperatures supported, got %d", SEGK_MAX_TEMPS, K);
  SEGK_REQUIRE(pad_top >= 0 && pad_left >= 0 && pad_top + nh <= T && pad_left + nw <= T, "calib_temps: window outside the slot");
  SEGK_REQUIRE(mode == 0 || mode == 1, "calib_temps: bad mode %d", mode);
  SEGK_REQUIRE(ignore_index >= -1, "calib_temps: ignore_index is a class index or -1 (none), got %d", ignore_index);
  SEGK_REQUIRE((long)T * T < (1L << 30) && (long)oh * ow < (1L << 31) - 4, "calib_temps: slot or image too large for 32-bit offsets");
  SEGK_REQUIRE(((uintptr_t)slot & 3) == 0 && ((uintptr_t)inv_T_dev & 3) == 0, "calib_temps: slot and table must be 4-byte aligned");
  SEGK_REQUIRE(((uintptr_t)labels & 7) == 0 && ((uintptr_t)hist & 7) == 0 && ((uintptr_t)nll_fx & 7) == 0 &&
                   ((uintptr_t)nonfinite & 7) == 0 && ((uintptr_t)valid & 7) == 0,
               "calib_temps: labels and the outputs must be 8-byte aligned");
  const size_t lds = (size_t)K * 258 * sizeof(unsigned long long);     // K 2 KB histograms + the K NLL and non-finite sums
  long g = (((long)oh * ow + 3) / 4 + 255) / 256;
  // persistent grid as segk_predict_mask's counting form; at most three blocks per CU, fewer where the LDS holds fewer
  long per_cu = (160L * 1024) / (long)(lds + 64);
  if (per_cu > 3) per_cu = 3;
  const long cap = per_cu * segk_num_cus();
  if (g > cap) g = cap;
  hipStream_t st = (hipStream_t)s;
  auto launch = [&](auto nc, auto md) {
    return segk_launch_lds<calib_temps_kernel<decltype(nc)::value, decltype(md)::value>>(
        "calib_temps", 96 * 1024, dim3((int)g), dim3(256), lds, st, slot, C, T, pad_top, pad_left, nh, nw, oh, ow,
        (const long long*)labels, ignore_index, inv_T_dev, K, (unsigned long long*)hist, (unsigned long long*)nll_fx,
        (unsigned long long*)nonfinite, (unsigned long long*)valid);
  };
  return dispatch_classes(C, [&](auto nc) {
    return mode == 0 ? launch(nc, std::integral_constant<int, 0>{}) : launch(nc, std::integral_constant<int, 1>{});
  });
}
