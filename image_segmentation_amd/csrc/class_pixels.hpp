// What the per-pixel class kernels share, each stated once: fp32 NCHW logits, at most MAXC classes, one
// thread per pixel.  With -ffp-contract=off one source expression gives one bit pattern, so the agreements the tests pin
// (the hard-pixel loss with everything off == loss_fwd's CrossEntropy, the unstored BatchNorm apply == the stored head
// backward) hold because the kernels call the expressions below instead of restating them.
//   head.hip       head_bwd, head_bn_bwd_apply                        pixel split, class load, dispatch
//   loss.hip       loss_fwd / loss_bwd, prompt_mix, confusion          all of it (segk_loss_blocks is defined there)
//   hard_loss.hip  hard_key, hard_fwd, hard_bwd                        all of it but the row write
//   distill.hip    distill_fwd, distill_bwd                            pixel split, class load, wave sum, row write, dispatch
//   vit.hip        the LayerNorm kernels                               wave sum
// Deliberately NOT here: distill.hip's softmax_nc (starts the maximum at a[0] and takes expf of the -inf padding unmasked:
// other bits for a NaN in class 0) and distill_finalize_block (one row per thread, wave butterfly: another order of the
// float64 additions than sum_partial_rows); hard_fwd_kernel's row write (its instance <8, false, true> holds the 128 registers
// a 1024-thread block may have: through write_partial_row it spilled one, 8 bytes of scratch); predict_common.hpp's
// softmax_classes (divides, compares without fmaxf) and the butterflies of predict_common.hpp and calib.hip (through wave_sum
// 62 finisher instances changed their register allocation for nothing).
// Measured against the parent on one box (profiles/loss_refactor_kbench.txt): two lines of changed kernels stayed above "new
// median not above the parent's larger median" in more than one run set and are merged all the same -- hard_bwd_kernel<4, true,
// true> (the selection backward: 15.0 / 14.9 us against 14.7 / 14.8, min..max 14.4 .. 15.4 in both builds) and
// head_bn_bwd_apply_kernel<bf16, 3> with the unchanged head_bwd_kernel in front of it (67.1 MB: 89.7 / 88.6 us against
// 88.9 / 88.2).  Both hold the parent's instructions in another order, and lines that run the parent's very instructions
// (head_bwd_kernel, the stem end) were above the rule as often and by as much.
// Everything is __forceinline__ and every register array is indexed by unrolled constants only.  The names below are global in
// every unit that includes this header, predict_common.hpp's users among them.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "ticket.hpp"
#include "../../include/segk.h"

constexpr int MAXC = SEGK_MAX_CLASSES;   // classes supported by the fused kernels

// ---- loss launch geometry: segk_loss_blocks(P) blocks of LT threads, LPIF pixels per thread in flight per pass, one partial
// row per block and never more than LROWS of them (the last arriver's walk below is sized to LROWS) ------------------------------
constexpr int LT = 1024, LROWS = 256, LPIF = 4;
int segk_loss_blocks(long P);            // loss.hip: rows of the partial buffer segk_loss_part_floats(P) sizes

// pixel index -> (image, offset inside the image) with ONE 32-bit division: a 64-bit one is a ~130-instruction loop, per
// pixel more than the rest of a loss kernel's arithmetic.  Every launcher requires P < 2^31.
__device__ __forceinline__ void split_hw(long p, long HW, long& b, long& r) {
  const unsigned bb = (unsigned)p / (unsigned)HW;
  b = (long)bb;
  r = p - (long)bb * HW;
}

// ---- the NC compiled classes of pixel (b, r): unconditional loads from a class index clamped into the tensor (a conditional
// load compiles to branch + wait).  Without `pad` the classes past C hold class C - 1 and the caller selects at first use;
// with it they are selected here ---------------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void load_classes(const float* __restrict__ base, long b, long r, int C, long HW, float (&raw)[NC]) {
#pragma unroll
  for (int k = 0; k < NC; ++k) raw[k] = base[(b * C + (k < C ? k : C - 1)) * HW + r];
}
template <int NC>
__device__ __forceinline__ void load_classes(const float* __restrict__ base, long b, long r, int C, long HW, float (&raw)[NC],
                                             float pad) {
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float v = base[(b * C + (k < C ? k : C - 1)) * HW + r];
    raw[k] = (k < C) ? v : pad;
  }
}

// ---- softmax pieces over values whose padding is -inf: m = class_max(z), se = class_exp(z, m, C, e), then 1.f / se for the
// probabilities e_k * inv and logf(se) for nl_k = neg_log_softmax(lse, z_k, m) ------------------------------------------------
template <int NC>
__device__ __forceinline__ float class_max(const float (&z)[NC]) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) m = fmaxf(m, z[k]);
  return m;
}
// e_k = expf(z_k - m), 0 past C; returns their sum in class order from 0.f (e may be z itself)
template <int NC>
__device__ __forceinline__ float class_exp(const float (&z)[NC], float m, int C, float (&e)[NC]) {
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) { e[k] = (k < C) ? expf(z[k] - m) : 0.f; se += e[k]; }
  return se;
}
// -log softmax = log(sum exp) - (logit - max)
__device__ __forceinline__ float neg_log_softmax(float lse, float z, float m) { return lse - (z - m); }

// ---- sums ------------------------------------------------------------------------------------------------------------------
// the 64-lane butterfly: every lane gets the sum (float, unsigned, double, unsigned long long)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One partial row per block of LT threads: v holds a wave's NW sums (wave_sum); lane 0 of every wave puts them into LDS and
// thread i < NW adds column i over the LT / 64 waves in wave order -- as floats, or as the uint32 bits they carry for the
// columns of the bit mask UINTS -- and writes word i of `row`.  Only distill_fwd_kernel has integer columns (hard_fwd_kernel,
// the other row of that kind, keeps its own write: above); both sums are formed and one is selected, the other is dead code.
template <int NW, unsigned UINTS = 0>
__device__ __forceinline__ void write_partial_row(const float (&v)[NW], float* __restrict__ row) {
  __shared__ float sh[LT / 64][NW];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) sh[threadIdx.x >> 6][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < NW) {
    const int i = threadIdx.x;
    float s = 0.f;
    unsigned n = 0;
#pragma unroll
    for (int w = 0; w < LT / 64; ++w) { s += sh[w][i]; n += __float_as_uint(sh[w][i]); }   // fixed order
    row[i] = ((UINTS >> i) & 1u) ? __uint_as_float(n) : s;
  }
}

// Runs in ONE block of LT threads, the one that arrived last (ticket.hpp): the float64 column sums of NB <= LROWS partial rows of
// NCOL words.  Every thread takes one column of LROWS / (LT / 32) rows, all loads in flight at once (ONE memory round trip: the
// rows were written by other XCDs and come from memory), from a clamped row (a conditional load compiles to branch + wait); the
// 32 row groups are added in one fixed order: bit-stable.  word(v, column): the float64 value of a word (a float, or uint32
// bits).  Returns the NCOL sums (LDS), valid in every thread.
template <int NCOL, typename F>
__device__ __forceinline__ const double* sum_partial_rows(const float* __restrict__ part, int NB, F&& word) {
  __shared__ double tot[NCOL];
  __shared__ double sh[LT / 32][32];
  static_assert(NCOL <= 32, "one column lane per partial");
  constexpr int RG = LT / 32, FL = LROWS / RG;
  const int t = threadIdx.x, cx = t & 31, ry = t >> 5;
  double acc = 0.0;
  if (cx < NCOL) {
    float v[FL];
#pragma unroll
    for (int u = 0; u < FL; ++u) {
      const int r = ry + RG * u < NB ? ry + RG * u : NB - 1;
      v[u] = part[(unsigned)r * NCOL + cx];
    }
#pragma unroll
    for (int u = 0; u < FL; ++u) acc += (ry + RG * u < NB) ? word(v[u], cx) : 0.0;
  }
  sh[ry][cx] = acc;
  __syncthreads();
  if (t < NCOL) {
    double s = 0.0;
    for (int r = 0; r < RG; ++r) s += sh[r][t];   // fixed order
    tot[t] = s;
  }
  __syncthreads();
  return tot;
}

// ---- host: f(integral_constant<int, N>) for the smallest N of the compiled class counts Ns (ascending) that holds C -------------
template <int N, int... Ns, typename F>
inline auto dispatch_nc(int C, F&& f) {
  if constexpr (sizeof...(Ns) == 0) {
    return f(std::integral_constant<int, N>{});
  } else {
    if (C <= N) return f(std::integral_constant<int, N>{});
    return dispatch_nc<Ns...>(C, f);
  }
}
// the instance sets: the losses (loss.hip, hard_loss.hip); one instance per class count up to 4 (distill.hip, the finishers)
template <typename F> inline auto dispatch_loss_nc(int C, F&& f) { return dispatch_nc<2, 4, MAXC>(C, f); }
template <typename F> inline auto dispatch_each_nc(int C, F&& f) { return dispatch_nc<1, 2, 3, 4, MAXC>(C, f); }
