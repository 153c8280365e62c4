// Hard-pixel losses (the reference reaches label smoothing through nn.CrossEntropyLoss kwargs,
// utils/weighted_loss.py:132-138, and holds no focal or bootstrapped loss): label-smoothed, class-weighted CrossEntropy with an
// optional focal modulation and an optional selection of the hardest pixels (OHEM), mean over the kept pixels.
//
// Per counted pixel, in fp32 and in this order (pixel_terms below; forward, key pass and backward all come through it):
//   m = max_k z_k, e_k = expf(z_k - m), se = sum_k e_k, lse = logf(se), nl_k = lse - (z_k - m), p_k = e_k * (1 / se)
//   key    kappa = nl_t, clamped to >= 0 (a NaN stays)
//   ce     = w_t * nl_t                                  (label_smoothing == 0)
//          = sum_k a_k * nl_k,  a_k = [k = t] * ((1 - eps) * w_t) + (eps / C) * w_k        (class order, from 0.f)
//   u      = sum_{k != t} p_k (class order), mod = powf(u, gamma) (1 and no powf when gamma == 0), l = mod * ce
// Selection: an exact k-th largest key by a three-level radix select (11 + 11 + 10 bits) over one 32-bit word per pixel
// (bits(kappa) + 1, 0x7FC00001 for a NaN key, 0 for a pixel that does not count): histograms in LDS, one integer atomic per
// non-zero bin and block, the block that arrives last (ticket.hpp) scans from the top bin down.  No sort, no host sync, no float
// atomics; the loss sums take loss_fwd_kernel's order (loss.hip) through the same code (class_pixels.hpp) and are finished in
// float64 by the last arriver.
#include "class_pixels.hpp"
#include "segk_internal.h"

namespace {
constexpr int HP = 4;                  // words per partial row: [0] sum l, [1] sum w_t (float), [2] n, [3] n_kept (uint32 bits)
constexpr int L0 = 2048, L1 = 2048, L2 = 1024;   // bins of the three levels: word >> 21, (word >> 10) & 2047, word & 1023
constexpr int CTRL = L0 + L1 + L2;     // control words behind the histograms:
enum { C_PRE0 = 0,                     //   level-0 bin of the k-th word
       C_REM0,                         //   its rank inside that bin, from the top (>= 1)
       C_DONE,                         //   1: k == 0, the threshold is theta's word and levels 1, 2 have nothing to do
       C_TAU,                          //   word of tau
       C_PRE1,                         //   top 22 bits of the k-th word
       C_REM1,                         //   its rank inside that level-1 bin
       C_N };                          //   n
static_assert(CTRL + 16 == SEGK_HARD_HIST_WORDS, "histogram scratch of include/segk.h");
constexpr unsigned NAN_WORD = 0x7FC00001u;

template <int NC>
__device__ __forceinline__ void fetch(const float* __restrict__ logits, const long long* __restrict__ labels, long p, long HW,
                                      int C, float (&raw)[NC], long long& y) {
  long b, r; split_hw(p, HW, b, r);
  load_classes<NC>(logits, b, r, C, HW, raw);     // selected at first use (pixel_terms)
  y = labels[p];
}
// between the loads of the pixels in flight and their first use: the scheduler otherwise pairs each load with the select that
// consumes it (load, wait, select, next address) in the instances with few live values, one memory round trip per class
__device__ __forceinline__ void loads_issued() { __builtin_amdgcn_sched_barrier(0); }

// what one pixel contributes; register arrays are only ever indexed by unrolled loop counters
template <int NC>
struct Px {
  float p[NC], nl[NC];   // softmax, -log softmax
  float nlt, wt, pt;     // at the label (0 when the pixel does not count)
  bool counted;
};
template <int NC>
__device__ __forceinline__ void pixel_terms(const float (&raw)[NC], long long y, int C, int ignore_index, const float (&w)[NC],
                                            Px<NC>& o) {
  float z[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) z[k] = (k < C) ? raw[k] : -INFINITY;
  const float m = class_max(z), se = class_exp(z, m, C, o.p);
  const float inv = 1.f / se, lse = logf(se);
  o.counted = y >= 0 && y < C && y != ignore_index;
  o.nlt = 0.f; o.wt = 0.f; o.pt = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    o.p[k] *= inv;
    o.nl[k] = neg_log_softmax(lse, z[k], m);
    if (o.counted && y == k) { o.nlt = o.nl[k]; o.wt = w[k]; o.pt = o.p[k]; }
  }
}
__device__ __forceinline__ unsigned key_word(float nlt, bool counted) {
  const float kappa = nlt < 0.f ? 0.f : nlt;
  return !counted ? 0u : (kappa != kappa ? NAN_WORD : __float_as_uint(kappa) + 1u);
}
// smoothing coefficients a_k, their sum A and ce (PLAIN: ce = w_t * nl_t, a and A unused)
template <int NC, bool PLAIN>
__device__ __forceinline__ float ce_terms(const Px<NC>& x, long long y, int C, const float (&w)[NC], float eps, float c1,
                                          float c2, float (&a)[NC], float& A) {
  A = 0.f;
  if constexpr (PLAIN) return x.wt * x.nlt;
  const float c1w = c1 * x.wt;
  float ce = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    a[k] = (k < C) ? ((y == k) ? c1w : 0.f) + c2 * w[k] : 0.f;
    A += a[k];
    ce += (k < C) ? a[k] * x.nl[k] : 0.f;
  }
  return eps != 0.f ? ce : x.wt * x.nlt;   // uniform: without smoothing no other class's term exists (0 * inf)
}
template <int NC>
__device__ __forceinline__ float others(const Px<NC>& x, long long y, int C) {   // u = sum_{k != t} p_k, never 1 - p_t
  float u = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) u += (k < C && y != k) ? x.p[k] : 0.f;
  return u;
}
// the class weights (1 when absent) go through LDS once per block: a read of `cw` itself under the label's condition compiles
// to branch + load + wait per class and pixel (the pointer may be null, so the load cannot be hoisted)
template <int NC>
__device__ __forceinline__ void load_weights(const float* __restrict__ cw, int C, float (&w)[NC]) {
  __shared__ float sw[MAXC];
  if (threadIdx.x < MAXC) sw[threadIdx.x] = (cw != nullptr && (int)threadIdx.x < C) ? cw[threadIdx.x] : 1.f;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NC; ++k) w[k] = sw[k];
}

// ---- the block that arrived last: bin of the k-th largest word ----------------------------------------------------------
// hist: NB (<= 2048) counters other blocks added to (read past this CU's L1).  Every thread of the LT-thread block calls;
// k = rank(total of the counters) says which word is wanted (0: none; else 1 <= k <= total); returns the bin of the k-th
// largest word and its rank inside that bin, counted from the bin's top (>= 1), and the total.
template <typename F>
__device__ __forceinline__ void select_bin(unsigned* hist, int NB, F&& rank, unsigned& bin, unsigned& rem, unsigned& total) {
  __shared__ unsigned wtot[LT / 64], res[2];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // thread t owns bins 2t, 2t + 1; a suffix sum over the threads (wave shuffles, then the 16 wave totals)
  const int i0 = 2 * t < NB ? 2 * t : 0;
  const unsigned long long both =
      __hip_atomic_load((unsigned long long*)(hist + i0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned h0 = 2 * t < NB ? (unsigned)both : 0u, h1 = 2 * t < NB ? (unsigned)(both >> 32) : 0u;
  const unsigned v = h0 + h1;
  unsigned s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = __shfl_down(s, o);
    s += (lane + o < 64) ? x : 0u;
  }
  if (lane == 0) wtot[wv] = s;
  if (t < 2) res[t] = 0;
  __syncthreads();
  unsigned above_waves = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < LT / 64; ++q) {
    const unsigned x = wtot[q];
    tot += x;
    above_waves += q > wv ? x : 0u;
  }
  const unsigned k = rank(tot);
  s += above_waves;                    // words in bins >= 2t
  const unsigned above = s - v;        // words in bins >= 2t + 2
  if (k > 0 && s >= k && above < k) {  // exactly one thread
    const bool hi = above + h1 >= k;
    res[0] = (unsigned)(2 * t) + (hi ? 1u : 0u);
    res[1] = hi ? k - above : k - above - h1;
  }
  __syncthreads();
  bin = res[0]; rem = res[1]; total = tot;
}

// LDS histogram -> one integer atomic per non-zero bin
__device__ __forceinline__ void flush_hist(const unsigned* lh, unsigned* gh, int NB) {
  __syncthreads();
  for (int i = threadIdx.x; i < NB; i += LT)
    if (lh[i]) atomicAdd(gh + i, lh[i]);
}

// pass 1 of the selection: the words, the level-0 histogram, then (last arriver) n, k and the level-0 bin
template <int NC>
__global__ __launch_bounds__(LT) void hard_key_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                      long P, long HW, int C, int ignore_index, unsigned theta_word,
                                                      unsigned min_kept, unsigned q16, unsigned* __restrict__ keys,
                                                      unsigned* hist, unsigned* __restrict__ ticket) {
  __shared__ unsigned lh[L0];
  __shared__ int last;
  for (int i = threadIdx.x; i < L0; i += LT) lh[i] = 0;
  __syncthreads();
  float w[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) w[k] = 1.f;
  auto pixel = [&](long p, const float (&raw)[NC], long long y) {
    Px<NC> x;
    pixel_terms<NC>(raw, y, C, ignore_index, w, x);
    const unsigned word = key_word(x.nlt, x.counted);
    if (p < P) {
      keys[p] = word;
      if (word) atomicAdd(&lh[word >> 21], 1u);
    }
  };
  // four pixels in flight in every pass: past the end the loads are clamped to the last pixel and the result is dropped (no
  // float sum depends on the order here, so the tail needs no loop of its own)
  const long step = (long)gridDim.x * LT;
  for (long p = (long)blockIdx.x * LT + threadIdx.x; p < P; p += 4 * step) {
    float r0[NC], r1[NC], r2[NC], r3[NC];
    long long y0, y1, y2, y3;
    const long last_p = P - 1;
    fetch<NC>(logits, labels, p, HW, C, r0, y0);
    fetch<NC>(logits, labels, p + step < P ? p + step : last_p, HW, C, r1, y1);
    fetch<NC>(logits, labels, p + 2 * step < P ? p + 2 * step : last_p, HW, C, r2, y2);
    fetch<NC>(logits, labels, p + 3 * step < P ? p + 3 * step : last_p, HW, C, r3, y3);
    loads_issued();
    pixel(p, r0, y0);
    pixel(p + step, r1, y1);
    pixel(p + 2 * step, r2, y2);
    pixel(p + 3 * step, r3, y3);
  }
  flush_hist(lh, hist, L0);
  if (!last_arriver(ticket, gridDim.x, &last)) return;
  // n = every counted word; k = min(n, max(min_kept, ceil(f n))) with the ceiling in 64-bit integers
  auto rank = [&](unsigned n) {
    const unsigned long long kf = ((unsigned long long)n * q16 + 65535ull) >> 16;
    unsigned long long k = kf > min_kept ? kf : min_kept;
    return (unsigned)(k > n ? n : k);
  };
  unsigned bin, rem, n;
  select_bin(hist, L0, rank, bin, rem, n);
  const unsigned k = rank(n);
  if (threadIdx.x == 0) {
    unsigned* c = hist + CTRL;
    c[C_N] = n;
    c[C_DONE] = k == 0 ? 1u : 0u;
    c[C_TAU] = theta_word;
    c[C_PRE0] = k == 0 ? 0u : bin;
    c[C_REM0] = k == 0 ? 0u : rem;
  }
}

// passes 2 and 3: histogram of the next bits over the words that share the prefix found so far
template <int LEVEL>
__global__ __launch_bounds__(LT) void hard_refine_kernel(const unsigned* __restrict__ keys, long P, unsigned theta_word,
                                                         unsigned* hist, unsigned* __restrict__ ticket) {
  constexpr int NB = LEVEL == 1 ? L1 : L2;
  constexpr int SH = LEVEL == 1 ? 21 : 10;          // the bits above this level's
  __shared__ unsigned lh[NB];
  __shared__ int last;
  unsigned* const ctrl = hist + CTRL;
  // written by the launch in front (plain loads: nothing of this launch writes them before its last block has read them)
  if (ctrl[C_DONE]) return;
  const unsigned prefix = ctrl[LEVEL == 1 ? C_PRE0 : C_PRE1], k = ctrl[LEVEL == 1 ? C_REM0 : C_REM1];
  unsigned* const gh = hist + (LEVEL == 1 ? L0 : L0 + L1);
  for (int i = threadIdx.x; i < NB; i += LT) lh[i] = 0;
  __syncthreads();
  auto word = [&](unsigned v) {
    if (v != 0u && (v >> SH) == prefix) atomicAdd(&lh[LEVEL == 1 ? (v >> 10) & 2047u : v & 1023u], 1u);
  };
  const long step = (long)gridDim.x * LT;
  long p = (long)blockIdx.x * LT + threadIdx.x;
  for (; p + 3 * step < P; p += 4 * step) {
    const unsigned v0 = keys[p], v1 = keys[p + step], v2 = keys[p + 2 * step], v3 = keys[p + 3 * step];
    word(v0); word(v1); word(v2); word(v3);
  }
  for (; p < P; p += step) word(keys[p]);
  flush_hist(lh, gh, NB);
  if (!last_arriver(ticket, gridDim.x, &last)) return;
  unsigned bin, rem, tot;
  select_bin(gh, NB, [&](unsigned) { return k; }, bin, rem, tot);
  if (threadIdx.x == 0) {
    if constexpr (LEVEL == 1) {
      ctrl[C_PRE1] = (prefix << 11) | bin;
      ctrl[C_REM1] = rem;
    } else {
      const unsigned wk = (prefix << 10) | bin;     // the k-th largest word, exactly
      ctrl[C_TAU] = wk < theta_word ? wk : theta_word;
    }
  }
}

// runs in the block that arrived last: NB <= LROWS rows of [sum l, sum w_t, n, n_kept] -> state, loss_out.  The walk over the
// rows is loss_finalize_block's (sum_partial_rows): with everything off, the same bits
__device__ __forceinline__ void hard_finalize_block(const float* __restrict__ part, int NB, unsigned tau_word, int nstate,
                                                    float* __restrict__ state, float* __restrict__ loss_out) {
  const double* tot = sum_partial_rows<HP>(part, NB, [](float v, int cx) { return cx < 2 ? (double)v : (double)__float_as_uint(v); });
  if (threadIdx.x != 0) return;
  const double S = tot[0], D = tot[1];
  const unsigned n = (unsigned)tot[2], nk = (unsigned)tot[3];
  // no weight kept: NaN when no pixel counts at all (torch's rule), else exactly 0 (an empty kept set, zero weights)
  const float loss = D > 0.0 ? (float)(S / D) : (n == 0 ? NAN : 0.f);
  state[0] = loss;
  state[1] = (float)S;
  state[2] = 0.f;
  state[3] = (float)D;
  state[4] = tau_word == NAN_WORD ? NAN : __uint_as_float(tau_word - 1u);
  state[5] = __uint_as_float(tau_word);
  state[6] = __uint_as_float(n);
  state[7] = __uint_as_float(nk);
  for (int i = 8; i < nstate; ++i) state[i] = 0.f;
  if (loss_out) *loss_out = loss;
}

// the loss sums, loss_fwd_kernel's launch arithmetic: segk_loss_blocks(P) blocks of 1024 threads, four pixels in flight,
// unconditional clamped loads, wave butterfly, LDS rows, one partial row per block, the last arriver finishes.
// PLAIN: gamma == 0 and label_smoothing == 0.  SEL: a pixel is kept when its word >= the word of tau (hist's control block)
template <int NC, bool PLAIN, bool SEL>
__global__ __launch_bounds__(LT) void hard_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                      const float* __restrict__ cw, long P, long HW, int C, int ignore_index,
                                                      float eps, float gamma, const unsigned* __restrict__ keys,
                                                      const unsigned* __restrict__ hist, float* __restrict__ part, int nstate,
                                                      float* __restrict__ state, float* __restrict__ loss_out,
                                                      unsigned* __restrict__ ticket) {
  __shared__ int last;
  unsigned tau_word = 1u;              // every counted pixel
  if constexpr (SEL) tau_word = hist[CTRL + C_TAU];
  float w[NC];
  load_weights<NC>(cw, C, w);
  const float c1 = 1.f - eps, c2 = eps / (float)C;
  float a0 = 0.f, a1 = 0.f;
  unsigned cnt = 0, kept = 0;
  auto pixel = [&](const float (&raw)[NC], const long long y, const unsigned word) {
    Px<NC> x;
    pixel_terms<NC>(raw, y, C, ignore_index, w, x);
    bool keep = x.counted;
    if constexpr (SEL) keep = word >= tau_word;      // the word of a pixel that does not count is 0, tau's is >= 1
    float a[NC], A;
    float l = ce_terms<NC, PLAIN>(x, y, C, w, eps, c1, c2, a, A);
    if constexpr (!PLAIN)
      if (gamma != 0.f) l = powf(others<NC>(x, y, C), gamma) * l;
    cnt += x.counted ? 1u : 0u;
    if (keep) {
      a0 += l;
      a1 += x.wt;
      kept += 1u;
    }
  };
  const long step = (long)gridDim.x * LT;
  long p = (long)blockIdx.x * LT + threadIdx.x;
  for (; p + 3 * step < P; p += 4 * step) {
    float r0[NC], r1[NC], r2[NC], r3[NC];
    long long y0, y1, y2, y3;
    unsigned k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    fetch<NC>(logits, labels, p, HW, C, r0, y0);
    fetch<NC>(logits, labels, p + step, HW, C, r1, y1);
    fetch<NC>(logits, labels, p + 2 * step, HW, C, r2, y2);
    fetch<NC>(logits, labels, p + 3 * step, HW, C, r3, y3);
    if constexpr (SEL) { k0 = keys[p]; k1 = keys[p + step]; k2 = keys[p + 2 * step]; k3 = keys[p + 3 * step]; }
    loads_issued();
    pixel(r0, y0, k0);
    pixel(r1, y1, k1);
    pixel(r2, y2, k2);
    pixel(r3, y3, k3);
  }
  for (; p < P; p += step) {
    float r0[NC];
    long long y0;
    unsigned k0 = 0;
    fetch<NC>(logits, labels, p, HW, C, r0, y0);
    if constexpr (SEL) k0 = keys[p];
    loads_issued();
    pixel(r0, y0, k0);
  }
  // wave sums, the wave rows through LDS, one partial row per block.  Not write_partial_row (class_pixels.hpp): the instance
  // <8, false, true> sits at the 128 registers a 1024-thread block may have and spilled one of them through it
  __shared__ float shs[LT / 64], shd[LT / 64];
  __shared__ unsigned shn[LT / 64], shk[LT / 64];
  a0 = wave_sum(a0); a1 = wave_sum(a1); cnt = wave_sum(cnt); kept = wave_sum(kept);
  if ((threadIdx.x & 63) == 0) {
    shs[threadIdx.x >> 6] = a0; shd[threadIdx.x >> 6] = a1; shn[threadIdx.x >> 6] = cnt; shk[threadIdx.x >> 6] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s2 = 0.f, d2 = 0.f;
    unsigned n2 = 0, k2 = 0;
#pragma unroll
    for (int q = 0; q < LT / 64; ++q) { s2 += shs[q]; d2 += shd[q]; n2 += shn[q]; k2 += shk[q]; }   // fixed order
    float* row = part + (size_t)blockIdx.x * HP;
    row[0] = s2;
    row[1] = d2;
    row[2] = __uint_as_float(n2);
    row[3] = __uint_as_float(k2);
  }
  if (last_arriver(ticket, gridDim.x, &last)) hard_finalize_block(part, (int)gridDim.x, tau_word, nstate, state, loss_out);
}

// dlogits_j = (grad_out / D) * g_j at kept pixels, g_j = mod (A p_j - a_j) - gamma powf(u, gamma - 1) p_t ([j = t] - p_j) ce;
// PLAIN: loss_bwd_kernel's expression go * ((w_t / D) * (p_j - [j = t])).  Exactly 0 off the kept set and when D == 0.
template <int NC, bool PLAIN, bool SEL>
__global__ __launch_bounds__(256) void hard_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                       const float* __restrict__ cw, const unsigned* __restrict__ keys,
                                                       const float* __restrict__ state, const float* __restrict__ gout, long P,
                                                       long HW, int C, int ignore_index, float eps, float gamma,
                                                       float* __restrict__ dlogits) {
  const float go = gout[0], D = state[3];
  const unsigned tau_word = __float_as_uint(state[5]);
  const bool live = D > 0.f;
  const float gs = live ? go / D : 0.f;
  float w[NC];
  load_weights<NC>(cw, C, w);
  const float c1 = 1.f - eps, c2 = eps / (float)C;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    float raw[NC];
    load_classes<NC>(logits, b, r, C, HW, raw);     // selected at first use (pixel_terms)
    const long long y = labels[p];
    unsigned word = 0;
    if constexpr (SEL) word = keys[p];
    Px<NC> x;
    pixel_terms<NC>(raw, y, C, ignore_index, w, x);
    bool keep = x.counted && live;
    if constexpr (SEL) keep = keep && word >= tau_word;
    float g[NC];
    if constexpr (PLAIN) {
      const float wy = x.wt / D;
#pragma unroll
      for (int k = 0; k < NC; ++k) g[k] = go * (wy * (x.p[k] - ((y == k) ? 1.f : 0.f)));
    } else {
      float a[NC], A;
      const float ce = ce_terms<NC, false>(x, y, C, w, eps, c1, c2, a, A);
      if (eps == 0.f) {              // uniform: a_k = [k = t] w_t exactly, A = w_t
        A = x.wt;
#pragma unroll
        for (int k = 0; k < NC; ++k) a[k] = (y == k) ? x.wt : 0.f;
      }
      float mod = 1.f, fc = 0.f;
      if (gamma != 0.f) {
        const float u = others<NC>(x, y, C);
        mod = powf(u, gamma);
        fc = ((gamma * powf(u, gamma - 1.f)) * x.pt) * ce;
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const float t1 = mod * (A * x.p[k] - a[k]);
        const float t2 = fc * (((y == k) ? 1.f : 0.f) - x.p[k]);
        g[k] = gs * (gamma != 0.f ? t1 - t2 : t1);
      }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < C) dlogits[(b * C + k) * HW + r] = keep ? g[k] : 0.f;
  }
}

template <typename F>
void by_mode(bool plain, bool sel, F&& launch) {
  if (plain) { if (sel) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
  else { if (sel) launch(std::false_type{}, std::true_type{}); else launch(std::false_type{}, std::false_type{}); }
}

int check_common(const char* name, const void* logits, const void* labels, const void* cw, int N, int C, long HW,
                 float label_smoothing, float gamma, int select, const void* keys) {
  SEGK_REQUIRE(logits != nullptr, "%s: null logits", name);
  SEGK_REQUIRE(labels != nullptr, "%s: null labels", name);
  SEGK_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)cw & 3) == 0 &&
               ((uintptr_t)keys & 3) == 0, "%s: misaligned buffer", name);
  SEGK_REQUIRE(C >= 1 && C <= MAXC, "%s: 1..%d classes supported, got %d", name, MAXC, C);
  SEGK_REQUIRE(N > 0 && HW > 0 && HW < (1L << 31), "%s: bad shape N=%d HW=%ld", name, N, HW);
  SEGK_REQUIRE((long)N * HW < (1L << 31), "%s: pixels are indexed with 32 bits: %ld pixels", name, (long)N * HW);
  SEGK_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, "%s: label_smoothing must lie in [0, 1), got %g", name,
               (double)label_smoothing);
  SEGK_REQUIRE(gamma == 0.f || (gamma >= 1.f && gamma <= 8.f), "%s: gamma must be 0 or lie in [1, 8], got %g", name,
               (double)gamma);
  SEGK_REQUIRE(select == 0 || select == 1, "%s: select must be 0 or 1, got %d", name, select);
  SEGK_REQUIRE(select == 0 || keys != nullptr, "%s: the selection needs the key buffer", name);
  return 0;
}
}  // namespace

extern "C" int segk_hard_loss_fwd(const float* logits, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                                  int ignore_index, float label_smoothing, float gamma, int select, float theta, int min_kept,
                                  int min_frac_q16, uint32_t* keys, uint32_t* hist, float* part, float* state, float* loss_out,
                                  segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (const int rc = check_common("hard_loss_fwd", logits, labels, class_weights, N, C, HW, label_smoothing, gamma, select, keys))
    return rc;
  SEGK_REQUIRE(part != nullptr, "hard_loss_fwd: null partial buffer");
  SEGK_REQUIRE(state != nullptr, "hard_loss_fwd: null state");
  SEGK_REQUIRE(((uintptr_t)part & 3) == 0 && ((uintptr_t)state & 3) == 0 && ((uintptr_t)loss_out & 3) == 0 &&
               ((uintptr_t)hist & 15) == 0, "hard_loss_fwd: misaligned buffer");
  SEGK_REQUIRE(select == 0 || hist != nullptr, "hard_loss_fwd: the selection needs SEGK_HARD_HIST_WORDS words of scratch");
  SEGK_REQUIRE(select == 0 || theta >= 0.f, "hard_loss_fwd: theta = -log(thresh) must be >= 0 (+inf: no threshold), got %g",
               (double)theta);
  SEGK_REQUIRE(min_kept >= 0, "hard_loss_fwd: min_kept must be >= 0, got %d", min_kept);
  SEGK_REQUIRE(min_frac_q16 >= 0 && min_frac_q16 <= 65536, "hard_loss_fwd: min_fraction is a 16-bit fraction in [0, 65536], got %d",
               min_frac_q16);
  const long P = (long)N * HW;
  const int nb = segk_loss_blocks(P);                            // nb * HP <= segk_loss_part_floats(P)
  SEGK_REQUIRE(nb >= 1 && nb <= LROWS, "hard_loss_fwd: bad block count %d", nb);
  const int nstate = segk_loss_state_floats();
  const bool plain = gamma == 0.f && label_smoothing == 0.f, sel = select != 0;
  unsigned* const tickets = segk_ticket_slot(sel ? 4 : 1, st);
  SEGK_REQUIRE(tickets != nullptr, "hard_loss_fwd: no ticket array");
  const long long* lab = (const long long*)labels;
  if (sel) {
    // the histograms and their control block are zeroed on the stream like the ticket counters: whatever an earlier call left
    if (hipMemsetAsync(hist, 0, (size_t)SEGK_HARD_HIST_WORDS * sizeof(uint32_t), st) != hipSuccess)
      SEGK_FAIL(-3, "hard_loss_fwd: cannot zero the histogram scratch");
    const float th = theta + 0.f;                                // -0 -> +0
    const unsigned theta_word = __builtin_bit_cast(unsigned, th) + 1u;
    dispatch_loss_nc(C, [&](auto NCc) {
      hipLaunchKernelGGL((hard_key_kernel<decltype(NCc)::value>), dim3(nb), dim3(LT), 0, st, logits, lab, P, HW, C, ignore_index,
                         theta_word, (unsigned)min_kept, (unsigned)min_frac_q16, keys, hist, tickets);
    });
    SEGK_CHECK_LAUNCH("hard_loss_fwd (keys)");
    hipLaunchKernelGGL(hard_refine_kernel<1>, dim3(nb), dim3(LT), 0, st, keys, P, theta_word, hist, tickets + 1);
    hipLaunchKernelGGL(hard_refine_kernel<2>, dim3(nb), dim3(LT), 0, st, keys, P, theta_word, hist, tickets + 2);
    SEGK_CHECK_LAUNCH("hard_loss_fwd (select)");
  }
  dispatch_loss_nc(C, [&](auto NCc) {
    by_mode(plain, sel, [&](auto PLAINc, auto SELc) {
      hipLaunchKernelGGL((hard_fwd_kernel<decltype(NCc)::value, decltype(PLAINc)::value, decltype(SELc)::value>), dim3(nb),
                         dim3(LT), 0, st, logits, lab, class_weights, P, HW, C, ignore_index, label_smoothing, gamma, keys, hist,
                         part, nstate, state, loss_out, tickets + (sel ? 3 : 0));
    });
  });
  SEGK_CHECK_LAUNCH("hard_loss_fwd");
  return 0;
}

extern "C" int segk_hard_loss_bwd(const float* logits, const int64_t* labels, const float* class_weights, const uint32_t* keys,
                                  const float* state, const float* grad_out, int N, int C, long HW, int ignore_index,
                                  float label_smoothing, float gamma, int select, float* dlogits, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (const int rc = check_common("hard_loss_bwd", logits, labels, class_weights, N, C, HW, label_smoothing, gamma, select, keys))
    return rc;
  SEGK_REQUIRE(state != nullptr, "hard_loss_bwd: null state");
  SEGK_REQUIRE(grad_out != nullptr, "hard_loss_bwd: null upstream gradient");
  SEGK_REQUIRE(dlogits != nullptr, "hard_loss_bwd: null gradient buffer");
  SEGK_REQUIRE(((uintptr_t)state & 3) == 0 && ((uintptr_t)grad_out & 3) == 0 && ((uintptr_t)dlogits & 3) == 0,
               "hard_loss_bwd: misaligned buffer");
  const long P = (long)N * HW;
  long g = (P + 255) / 256;
  if (g > 4096) g = 4096;
  const bool plain = gamma == 0.f && label_smoothing == 0.f, sel = select != 0;
  dispatch_loss_nc(C, [&](auto NCc) {
    by_mode(plain, sel, [&](auto PLAINc, auto SELc) {
      hipLaunchKernelGGL((hard_bwd_kernel<decltype(NCc)::value, decltype(PLAINc)::value, decltype(SELc)::value>), dim3((int)g),
                         dim3(256), 0, st, logits, (const long long*)labels, class_weights, keys, state, grad_out, P, HW, C,
                         ignore_index, label_smoothing, gamma, dlogits);
    });
  });
  SEGK_CHECK_LAUNCH("hard_loss_bwd");
  return 0;
}
