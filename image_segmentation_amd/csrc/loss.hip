// What is computed on the head's fp32 NCHW logits: the per-pixel CrossEntropy + soft-Dice loss and its probability form, the
// prompt model's remix and the argmax / confusion-count metric kernel.  All HBM-bound.  The shared pieces (pixel split, class
// load, softmax, wave sum, partial rows, dispatch): class_pixels.hpp.
//
// Loss semantics (one fused pass over logits + labels):
//   CE   : nn.CrossEntropyLoss(mean, optional weight / ignore_index)  -- utils/training.py:47,
//          utils/weighted_loss.py:132-138,163:  sum_p w[y_p] * nll_p / sum_p w[y_p] over non-ignored pixels
//   Dice : utils/weighted_loss.py:31-98: p = softmax; per class I = sum p*onehot, Sp = sum p, Sg = sum onehot
//          over N,H,W; dc = (2I+s)/clip(Sp+Sg+s, 1e-8); (weighted) mean over non-ignored classes; loss = -mean
//   combined = dice_weight * dice + ce_weight * ce   (weighted_loss.py:165)
// Metric: utils/MetricsHistory.py:65-75 (argmax -> first maximum, per-class TP/FP/FN/TN).
#include "class_pixels.hpp"
#include "segk_internal.h"

namespace {
// loss partials per block: [0]=sum w*nll, [1]=sum w, then I[MAXC], Sp[MAXC], Sg[MAXC]
constexpr int LP = 2 + 3 * MAXC;

// state: [0]=loss [1]=ce [2]=dice(-mean dc) [3]=ce_den, [4..4+MAXC) dc, [.. ) den_raw(Sp+Sg+smooth), [..) a_k
constexpr int LS = 4 + 3 * MAXC;
// runs in the block of loss_fwd_kernel that finished last: NB <= LROWS partial rows -> state, loss_out
__device__ __forceinline__ void loss_finalize_block(const float* __restrict__ part, int NB, int C, const float* cw,
                                                    int ignore_index, float smooth, float dice_weight, float ce_weight,
                                                    float* __restrict__ state, float* __restrict__ loss_out) {
  const double* tot = sum_partial_rows<LP>(part, NB, [](float v, int) { return (double)v; });
  if (threadIdx.x != 0) return;
  const double ce = tot[1] > 0.0 ? tot[0] / tot[1] : NAN;   // all pixels ignored -> NaN like torch
  double wsum = 0.0, dsum = 0.0;
  for (int k = 0; k < C; ++k) {
    const double den_raw = tot[2 + MAXC + k] + tot[2 + 2 * MAXC + k] + (double)smooth;
    const double den = den_raw < 1e-8 ? 1e-8 : den_raw;
    const double dc = (2.0 * tot[2 + k] + (double)smooth) / den;
    state[4 + k] = (float)dc;
    state[4 + MAXC + k] = (float)den_raw;
    const bool valid = !(ignore_index >= 0 && ignore_index < C && k == ignore_index);
    if (valid) {
      const double wk = cw ? (double)cw[k] : 1.0;
      wsum += wk; dsum += dc * wk;
    }
  }
  if (cw && wsum < 1e-8) wsum = 1e-8;
  const double dice = -(dsum / wsum);
  for (int k = 0; k < C; ++k) {
    const bool valid = !(ignore_index >= 0 && ignore_index < C && k == ignore_index);
    state[4 + 2 * MAXC + k] = valid ? (float)((cw ? (double)cw[k] : 1.0) / wsum) : 0.f;
  }
  // ce_weight == 0: the Dice-only losses, which have no CrossEntropy term -- a NaN ce (no pixel counts: every label is the
  // ignored class, or every class weight present is zero) must not reach them through 0 * NaN
  state[0] = (float)((double)dice_weight * dice + (ce_weight != 0.f ? (double)ce_weight * ce : 0.0));
  if (loss_out) *loss_out = state[0];
  state[1] = (float)ce;
  state[2] = (float)dice;
  state[3] = (float)tot[1];
}

// PROB: the input already holds class probabilities (prompt model, prompt_based/prompt.py:33-56): Dice on the values
// themselves (weighted_loss.py:206-209 with apply_softmax=False) and NLLLoss on nll_nonlin(x) = log(x + eps)
// (nll_log, prompt.ipynb's stable_log) or on x itself (weighted_loss.py:338-340)
// NC = compiled class count (>= C): the per-class work and the accumulators are sized to it, not to MAXC.  LPIF pixels per
// thread are in flight per pass (the walk is latency-bound otherwise); additions stay in one fixed order: bit-stable.
template <bool PROB, int NC>
__global__ __launch_bounds__(LT) void loss_fwd_kernel(const float* __restrict__ logits,
                                                       const long long* __restrict__ labels,
                                                       const float* __restrict__ cw, long P, long HW, int C,
                                                       int ignore_index, float* __restrict__ part, int nll_log, float eps,
                                                       float smooth, float dice_weight, float ce_weight,
                                                       float* __restrict__ state, float* __restrict__ loss_out,
                                                       unsigned* __restrict__ ticket) {
  __shared__ int last;
  float a0 = 0.f, a1 = 0.f, aI[NC], aP[NC], aG[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) { aI[k] = 0.f; aP[k] = 0.f; aG[k] = 0.f; }
  auto fetch = [&](long p, float (&raw)[NC], long long& y) {
    long b, r; split_hw(p, HW, b, r);
    load_classes<NC>(logits, b, r, C, HW, raw, -INFINITY);
    y = labels[p];
  };
  auto pixel = [&](const float (&raw)[NC], const long long y) {
    float l[NC], m = 0.f, se = 0.f;
    if constexpr (PROB) {
#pragma unroll
      for (int k = 0; k < NC; ++k) l[k] = (k < C) ? raw[k] : 0.f;
    } else {
      m = class_max(raw);
      se = class_exp(raw, m, C, l);
    }
    const float inv = PROB ? 1.f : 1.f / se, lse = PROB ? 0.f : logf(se);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float pk = l[k] * inv;
      const float oh = (y == k) ? 1.f : 0.f;
      aI[k] += pk * oh;
      aP[k] += pk;
      aG[k] += oh;
      if (y == k && k < C && y != ignore_index) {
        const float wy = cw ? cw[k] : 1.f;
        if constexpr (PROB) a0 += wy * (nll_log ? -logf(raw[k] + eps) : -raw[k]);
        else a0 += wy * neg_log_softmax(lse, raw[k], m);
        a1 += wy;
      }
    }
  };
  // LPIF pixels per thread in flight per pass (the walk is latency-bound otherwise); one fixed order of additions
  static_assert(LPIF == 4, "the main loop below is written out for four pixels");
  const long step = (long)gridDim.x * LT;
  long p = (long)blockIdx.x * LT + threadIdx.x;
  for (; p + 3 * step < P; p += 4 * step) {
    float r0[NC], r1[NC], r2[NC], r3[NC];
    long long y0, y1, y2, y3;
    fetch(p, r0, y0);
    fetch(p + step, r1, y1);
    fetch(p + 2 * step, r2, y2);
    fetch(p + 3 * step, r3, y3);
    pixel(r0, y0);
    pixel(r1, y1);
    pixel(r2, y2);
    pixel(r3, y3);
  }
  for (; p < P; p += step) {
    float r0[NC];
    long long y0;
    fetch(p, r0, y0);
    pixel(r0, y0);
  }
  // wave sums, then one row of LP partials per block (unused class slots = 0)
  float v[LP];
#pragma unroll
  for (int i = 0; i < LP; ++i) v[i] = 0.f;
  v[0] = wave_sum(a0); v[1] = wave_sum(a1);
#pragma unroll
  for (int k = 0; k < NC; ++k) { v[2 + k] = wave_sum(aI[k]); v[2 + MAXC + k] = wave_sum(aP[k]); v[2 + 2 * MAXC + k] = wave_sum(aG[k]); }
  write_partial_row<LP>(v, part + (size_t)blockIdx.x * LP);
  // the block that finishes last turns the partial rows into the loss (no second launch, nobody waits)
  if (last_arriver(ticket, gridDim.x, &last))
    loss_finalize_block(part, (int)gridDim.x, C, cw, ignore_index, smooth, dice_weight, ce_weight, state, loss_out);
}


template <bool PROB, int NC>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ logits,
                                                       const long long* __restrict__ labels,
                                                       const float* __restrict__ cw, const float* __restrict__ state,
                                                       const float* __restrict__ gout, long P, long HW, int C,
                                                       int ignore_index, float dice_weight, float ce_weight,
                                                       float* __restrict__ dlogits, int nll_log, float eps) {
  const float go = gout[0];
  const float ce_den = state[3];
  float G0[NC], G1[NC];   // dL_dice/dp_k = G0 + onehot*G1
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    G0[k] = 0.f; G1[k] = 0.f;
    if (k < C) {
      const float dc = state[4 + k], den_raw = state[4 + MAXC + k], ak = state[4 + 2 * MAXC + k];
      if (den_raw < 1e-8f) { G1[k] = -ak * 2.f / 1e-8f; }           // clip active: denominator constant
      else { G0[k] = ak * dc / den_raw; G1[k] = -ak * 2.f / den_raw; }
    }
  }
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    float l[NC];
    load_classes<NC>(logits, b, r, C, HW, l, -INFINITY);
    const float m = class_max(l);
    const long long y = labels[p];
    const bool ce_valid = (ce_weight != 0.f && y >= 0 && y < C && y != ignore_index);   // no term, no 0 / 0 weight
    float wy = 0.f;
    if (ce_valid) wy = (cw ? cw[y] : 1.f) / ce_den;
    if constexpr (PROB) {   // d/dx of  dice(x) + nll(log(x + eps) | x)
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (k < C) {
          const bool hit = (y == k);
          const float dd = G0[k] + (hit ? G1[k] : 0.f);
          const float dn = hit ? (nll_log ? -wy / (l[k] + eps) : -wy) : 0.f;
          dlogits[(b * C + k) * HW + r] = go * (dice_weight * dd + ce_weight * dn);
        }
      continue;
    }
    const float inv = 1.f / class_exp(l, m, C, l);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      l[k] *= inv;
      dot += l[k] * (G0[k] + ((y == k) ? G1[k] : 0.f));
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < C) {
        const float gk = G0[k] + ((y == k) ? G1[k] : 0.f);
        const float dd = l[k] * (gk - dot);
        const float dce = wy * (l[k] - ((y == k) ? 1.f : 0.f));
        dlogits[(b * C + k) * HW + r] = go * (dice_weight * dd + ce_weight * dce);
      }
  }
}

// confusion matrix M[pred][label] (uint64) over [N][C][HW] logits; argmax = FIRST maximum (torch.argmax)
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ logits,
                                                        const long long* __restrict__ labels, long P, long HW, int C,
                                                        unsigned long long* __restrict__ M) {
  __shared__ unsigned int hist[MAXC * MAXC];
  if (threadIdx.x < MAXC * MAXC) hist[threadIdx.x] = 0;
  __syncthreads();
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    int best = 0;
    float bv = logits[(b * C) * HW + r];
    for (int k = 1; k < C; ++k) {
      const float v = logits[(b * C + k) * HW + r];
      if (v > bv || (v != v && bv == bv)) { bv = v; best = k; }   // NaN counts as maximal, like torch
    }
    const long long y = labels[p];
    if (y >= 0 && y < C) atomicAdd(&hist[best * MAXC + (int)y], 1u);
  }
  __syncthreads();
  if (threadIdx.x < MAXC * MAXC && hist[threadIdx.x])
    atomicAdd(&M[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

}  // namespace

// ---- prompt model remix (prompt_based/prompt.py:33-56), 4 CLIP classes x 1 mask channel, fp32 NCHW ----
//   p = softmax(clip_logits), m = sigmoid(mask_logit)
//   final[0] = 1 - m;  final[1] = m*p0 + m*p3;  final[2] = m*p1;  final[3] = m*p2
__global__ __launch_bounds__(256) void prompt_mix_fwd_kernel(const float* __restrict__ clip, const float* __restrict__ mask,
                                                             float* __restrict__ out, long P, long HW) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    float l[4];
    load_classes<4>(clip, b, r, 4, HW, l);
    const float inv = 1.f / class_exp(l, class_max(l), 4, l);
    const float m = 1.f / (1.f + expf(-mask[p]));
    float sel[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sel[k] = m * (l[k] * inv);
    out[(b * 4 + 0) * HW + r] = 1.0f - m;
    out[(b * 4 + 1) * HW + r] = sel[0] + sel[3];
    out[(b * 4 + 2) * HW + r] = sel[1];
    out[(b * 4 + 3) * HW + r] = sel[2];
  }
}
// gradient w.r.t. the mask logit (the CLIP branch is frozen, prompt.py:30-31)
__global__ __launch_bounds__(256) void prompt_mix_bwd_kernel(const float* __restrict__ clip, const float* __restrict__ mask,
                                                             const float* __restrict__ dout, float* __restrict__ dmask,
                                                             long P, long HW) {
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    float l[4];
    load_classes<4>(clip, b, r, 4, HW, l);
    const float inv = 1.f / class_exp(l, class_max(l), 4, l);
    const float m = 1.f / (1.f + expf(-mask[p]));
    const float d0 = dout[(b * 4 + 0) * HW + r], d1 = dout[(b * 4 + 1) * HW + r];
    const float d2 = dout[(b * 4 + 2) * HW + r], d3 = dout[(b * 4 + 3) * HW + r];
    const float dm = -d0 + d1 * ((l[0] + l[3]) * inv) + d2 * (l[1] * inv) + d3 * (l[2] * inv);
    dmask[p] = dm * m * (1.f - m);
  }
}

// dout null: forward, out = final probabilities; else backward, out = gradient of the mask logit
static int prompt_mix(const float* clip, const float* mask, const float* dout, float* out, int N, long HW, hipStream_t st) {
  SEGK_REQUIRE(clip && mask && out && N > 0 && HW > 0, "prompt_mix: bad arguments");
  const long P = (long)N * HW;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  long g = (P + 255) / 256;
  if (g > 4096) g = 4096;
  if (dout) hipLaunchKernelGGL(prompt_mix_bwd_kernel, dim3((int)g), dim3(256), 0, st, clip, mask, dout, out, P, HW);
  else hipLaunchKernelGGL(prompt_mix_fwd_kernel, dim3((int)g), dim3(256), 0, st, clip, mask, out, P, HW);
  SEGK_CHECK_LAUNCH("prompt_mix");
  return 0;
}
extern "C" int segk_prompt_mix_fwd(const float* clip_logits, const float* mask_logit, float* final_probs, int N, long HW,
                                   segk_stream_t s) {
  return prompt_mix(clip_logits, mask_logit, nullptr, final_probs, N, HW, (hipStream_t)s);
}
extern "C" int segk_prompt_mix_bwd(const float* clip_logits, const float* mask_logit, const float* dfinal, float* dmask_logit,
                                   int N, long HW, segk_stream_t s) {
  SEGK_REQUIRE(dfinal, "prompt_mix_bwd: null gradient");
  return prompt_mix(clip_logits, mask_logit, dfinal, dmask_logit, N, HW, (hipStream_t)s);
}

int segk_loss_blocks(long P) {
  if (P <= 0) return 0;
  long g = (P + LPIF * LT - 1) / (LPIF * LT);     // LPIF pixels per thread per pass, at most LROWS partial rows
  return (int)(g > LROWS ? LROWS : g < 1 ? 1 : g);
}
int segk_loss_part_floats(long P) { return segk_loss_blocks(P) * LP; }
int segk_loss_state_floats(void) { return LS; }

// prob: the input holds probabilities (NLL with or without the logarithm, nll_log / eps), not logits (cross-entropy)
static int loss_fwd(const float* logits, const int64_t* labels64, const float* cw, int N, int C, long HW, int ignore_index,
                    float smooth, float dice_weight, float ce_weight, float* part, float* state, float* loss_out, int prob,
                    int nll_log, float eps, segk_stream_t s) {
  const long long* labels = (const long long*)labels64;
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(logits && labels && part && state && N > 0 && HW > 0, "loss_fwd: bad arguments");
  SEGK_REQUIRE(C >= 1 && C <= MAXC, "loss_fwd: 1..%d classes supported, got %d", MAXC, C);
  const long P = (long)N * HW;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  const int nb = segk_loss_blocks(P);
  unsigned* const ticket = segk_ticket_slot(1, st);
  SEGK_REQUIRE(ticket != nullptr, "loss_fwd: no ticket array");
  auto launch = [&](auto PROBc, auto NCc) {
    constexpr bool PR = decltype(PROBc)::value;
    constexpr int NC = decltype(NCc)::value;
    hipLaunchKernelGGL((loss_fwd_kernel<PR, NC>), dim3(nb), dim3(LT), 0, st, logits, labels, cw, P, HW, C, ignore_index, part,
                       PR ? nll_log : 0, PR ? eps : 0.f, smooth, dice_weight, ce_weight, state, loss_out, ticket);
  };
  auto by_nc = [&](auto PROBc) { dispatch_loss_nc(C, [&](auto NCc) { launch(PROBc, NCc); }); };
  if (prob) by_nc(std::true_type{});
  else by_nc(std::false_type{});
  SEGK_CHECK_LAUNCH("loss_fwd");
  return 0;
}
extern "C" int segk_loss_fwd(const float* logits, const int64_t* labels, const float* cw, int N, int C, long HW, int ignore_index,
                             float smooth, float dice_weight, float ce_weight, float* part, float* state, float* loss_out,
                             segk_stream_t s) {
  return loss_fwd(logits, labels, cw, N, C, HW, ignore_index, smooth, dice_weight, ce_weight, part, state, loss_out, 0, 0, 0.f, s);
}
extern "C" int segk_prob_loss_fwd(const float* probs, const int64_t* labels, const float* cw, int N, int C, long HW,
                                  int ignore_index, float smooth, float dice_weight, float nll_weight, int nll_log, float eps,
                                  float* part, float* state, float* loss_out, segk_stream_t s) {
  return loss_fwd(probs, labels, cw, N, C, HW, ignore_index, smooth, dice_weight, nll_weight, part, state, loss_out, 1, nll_log,
                  eps, s);
}

static int loss_bwd(const float* logits, const int64_t* labels64, const float* cw, const float* state, const float* gout, int N,
                    int C, long HW, int ignore_index, float dice_weight, float ce_weight, float* dlogits, int prob, int nll_log,
                    float eps, segk_stream_t s) {
  const long long* labels = (const long long*)labels64;
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(logits && labels && state && gout && dlogits && N > 0 && HW > 0 && C >= 1 && C <= MAXC, "loss_bwd: bad arguments");
  const long P = (long)N * HW;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  long g = (P + 255) / 256;
  if (g > 4096) g = 4096;
  auto launch = [&](auto PROBc, auto NCc) {
    constexpr bool PR = decltype(PROBc)::value;
    constexpr int NC = decltype(NCc)::value;
    hipLaunchKernelGGL((loss_bwd_kernel<PR, NC>), dim3((int)g), dim3(256), 0, st, logits, labels, cw, state, gout, P, HW, C,
                       ignore_index, dice_weight, ce_weight, dlogits, PR ? nll_log : 0, PR ? eps : 0.f);
  };
  auto by_nc = [&](auto PROBc) { dispatch_loss_nc(C, [&](auto NCc) { launch(PROBc, NCc); }); };
  if (prob) by_nc(std::true_type{});
  else by_nc(std::false_type{});
  SEGK_CHECK_LAUNCH("loss_bwd");
  return 0;
}
extern "C" int segk_loss_bwd(const float* logits, const int64_t* labels, const float* cw, const float* state, const float* gout,
                             int N, int C, long HW, int ignore_index, float dice_weight, float ce_weight, float* dlogits,
                             segk_stream_t s) {
  return loss_bwd(logits, labels, cw, state, gout, N, C, HW, ignore_index, dice_weight, ce_weight, dlogits, 0, 0, 0.f, s);
}
extern "C" int segk_prob_loss_bwd(const float* probs, const int64_t* labels, const float* cw, const float* state,
                                  const float* gout, int N, int C, long HW, int ignore_index, float dice_weight,
                                  float nll_weight, int nll_log, float eps, float* dprobs, segk_stream_t s) {
  return loss_bwd(probs, labels, cw, state, gout, N, C, HW, ignore_index, dice_weight, nll_weight, dprobs, 1, nll_log, eps, s);
}

extern "C" int segk_confusion(const float* logits, const int64_t* labels, int N, int C, long HW, uint64_t* M, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(logits && labels && M && N > 0 && HW > 0 && C >= 1 && C <= MAXC, "confusion: bad arguments");
  const long P = (long)N * HW;
  SEGK_REQUIRE(P < (1L << 31), "head / loss kernels index pixels with 32 bits: %ld pixels", P);
  long g = (P + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(confusion_kernel, dim3((int)g), dim3(256), 0, st, logits, (const long long*)labels, P, HW, C, (unsigned long long*)M);
  SEGK_CHECK_LAUNCH("confusion");
  return 0;
}
