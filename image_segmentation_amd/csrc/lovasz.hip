// Lovasz-Softmax loss (Berman, Triki, Blaschko 2018; the reference holds no set loss): for every (segment s,
// class c) the per-pixel errors err_c = fg ? sum_{k != c} p_k : p_c are sorted descending and weighted by the discrete
// gradient of the Jaccard index along that order.  Everything but the softmax is integer or float64 arithmetic in a fixed order:
//   keys      one thread per pixel (hard_key's launch geometry and loads): C words bits(err_c) + 1 (NAN_WORD for a NaN, 0 for a
//             pixel that does not count) and payloads (fg << 31) | index-in-segment into class-major scratch; segment
//             q = c * S + s starts at slot q * L
//   sort      a stable LSD radix sort of the S * C segments, PASSES passes of 8 bits over the 30 key bits, descending (the digit
//             is inverted).  Every pass: hist (digit counts of one tile of TILE slots), scan (per segment and digit, exclusive
//             over the tiles; the digit totals), scatter (the tile's slots ranked in input order by wave ballots, then stored)
//   count     fg slots and counted slots per tile of the sorted order; fgscan: exclusive over the tiles, the totals are G and n
//             (the prefix over a workgroup, here and for the scatter's digit bases, is scan.hpp's block_scan: DESIGN.md 3.20)
//   terms     F_i by ballots, g_i = J_i - J_{i-1} in float64 from integers, coef scattered back to pixel order, one float64
//             partial per tile; the block that arrives last (ticket.hpp) adds the partials per segment in a fixed order and
//             writes the state and the loss
// No workgroup waits for another: every scan across tiles is a launch of its own, the finish is a last-arriver ticket.  No
// atomics on global memory but that ticket, nothing to zero, no host sync, no allocation.
#include "class_pixels.hpp"
#include "scan.hpp"
#include "segk_internal.h"

namespace {
constexpr int TILE = SEGK_LOVASZ_TILE;
constexpr int ST = 256, NW = ST / 64, ROUNDS = TILE / ST;   // a wave owns ROUNDS * 64 consecutive slots of its tile
constexpr int RADIX = 256, PASSES = 4;
constexpr int SCAN_T = 1024, SCAN_W = SCAN_T / 64;
constexpr unsigned NAN_WORD = 0x3FFFFFFFu;
static_assert(TILE == ST * ROUNDS && ST == RADIX, "one thread per digit, ROUNDS slots per thread");

// where everything lies in the caller's scratch (uint32 words; the float64 partials first: 8-byte aligned)
struct Lay {
  double* part;                         // [NT]        float64 term sum of a tile
  unsigned *wa, *pa, *wb, *pb;          // [C P] each  words and payloads, ping and pong
  unsigned* hist;                       // [NT][256]   digit counts of a tile, then their exclusive scan over the segment's tiles
  unsigned* dtot;                       // [Q][256]    digit totals of a segment
  unsigned *tf, *tn;                    // [NT] each   fg slots / counted slots of a tile (tf: then exclusive over the tiles)
  unsigned* gn;                         // [2 Q]       G of a segment, then its counted slots
};
__host__ __device__ inline Lay lay_of(void* scratch, long CP, long NT, long Q) {
  Lay l;
  unsigned* u = (unsigned*)scratch;
  l.part = (double*)u; u += 2 * NT;
  l.wa = u; u += CP;
  l.pa = u; u += CP;
  l.wb = u; u += CP;
  l.pb = u; u += CP;
  l.hist = u; u += (long)RADIX * NT;
  l.dtot = u; u += (long)RADIX * Q;
  l.tf = u; u += NT;
  l.tn = u; u += NT;
  l.gn = u;
  return l;
}

__device__ __forceinline__ unsigned digit_of(unsigned word, int shift) { return 255u - ((word >> shift) & 255u); }

// ---- keys: the C words and payloads of every pixel ---------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void fetch(const float* __restrict__ logits, const long long* __restrict__ labels, long p, long HW,
                                      int C, float (&raw)[NC], long long& y) {
  long b, r; split_hw(p, HW, b, r);
  load_classes<NC>(logits, b, r, C, HW, raw);
  y = labels[p];
}
// p_k of one pixel by class_pixels.hpp's expressions
template <int NC>
__device__ __forceinline__ void softmax_of(const float (&raw)[NC], int C, float (&pr)[NC]) {
  float z[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) z[k] = (k < C) ? raw[k] : -INFINITY;
  const float m = class_max(z), se = class_exp(z, m, C, pr);
  const float inv = 1.f / se;
#pragma unroll
  for (int k = 0; k < NC; ++k) pr[k] *= inv;
}

template <int NC>
__global__ __launch_bounds__(LT) void lovasz_keys_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                         long P, long HW, int C, int ignore_index, int per_image,
                                                         unsigned* __restrict__ words, unsigned* __restrict__ pays) {
  auto pixel = [&](long p, const float (&raw)[NC], long long y) {
    if (p >= P) return;
    float pr[NC];
    softmax_of<NC>(raw, C, pr);
    const bool counted = y >= 0 && y < C && y != ignore_index;
    float u = 0.f;                       // sum_{k != y} p_k in class order from 0.f, never 1 - p_y
#pragma unroll
    for (int k = 0; k < NC; ++k) u += (k < C && y != k) ? pr[k] : 0.f;
    long b, r; split_hw(p, HW, b, r);
    const unsigned idx = (unsigned)(per_image ? r : p);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (k < C) {
        const bool fg = counted && y == k;
        const float err = fg ? u : pr[k];
        const unsigned word = !counted ? 0u : (err != err ? NAN_WORD : __float_as_uint(err) + 1u);
        words[(long)k * P + p] = word;
        pays[(long)k * P + p] = (fg ? 0x80000000u : 0u) | idx;
      }
    }
  };
  // PIF pixels in flight in every pass (hard_key's four; two for the eight-class instance, which would spill with four): past
  // the end the loads are clamped to the last pixel and the result is dropped
  constexpr int PIF = NC <= 4 ? 4 : 2;
  const long step = (long)gridDim.x * LT;
  for (long p = (long)blockIdx.x * LT + threadIdx.x; p < P; p += PIF * step) {
    float raw[PIF][NC];
    long long y[PIF];
#pragma unroll
    for (int j = 0; j < PIF; ++j) fetch<NC>(logits, labels, p + j * step < P ? p + j * step : P - 1, HW, C, raw[j], y[j]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < PIF; ++j) pixel(p + j * step, raw[j], y[j]);
  }
}

// ---- sort ----------------------------------------------------------------------------------------------------------------------
// block = tile t of segment q (blockIdx.x = q * TS + t): digit counts of its slots
__global__ __launch_bounds__(ST) void lovasz_hist_kernel(const unsigned* __restrict__ words, long L, unsigned TS, int shift,
                                                         unsigned* __restrict__ hist) {
  __shared__ unsigned lh[RADIX];
  const unsigned blk = blockIdx.x, q = blk / TS, t = blk - q * TS;
  lh[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* w = words + (long)q * L;
  const long i0 = (long)t * TILE + threadIdx.x;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long i = i0 + r * ST;
    if (i < L) atomicAdd(&lh[digit_of(w[i], shift)], 1u);
  }
  __syncthreads();
  hist[(size_t)blk * RADIX + threadIdx.x] = lh[threadIdx.x];
}

// block = 64 digits of segment q (blockIdx.x = 4 q + digit group), lane = digit, wave = a run of tiles: the counts become
// the exclusive sum over the tiles in front, the totals go to dtot
__global__ __launch_bounds__(SCAN_T) void lovasz_scan_kernel(unsigned* __restrict__ hist, unsigned TS, unsigned* __restrict__ dtot) {
  __shared__ unsigned wt[SCAN_W][64];
  const unsigned q = blockIdx.x >> 2, d = (blockIdx.x & 3) * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;
  unsigned* const col = hist + (size_t)q * TS * RADIX + d;
  const unsigned ch = (TS + SCAN_W - 1) / SCAN_W, t0 = w * ch, t1 = t0 + ch < TS ? t0 + ch : TS;
  unsigned s = 0;
  for (unsigned t = t0; t < t1; ++t) s += col[(size_t)t * RADIX];
  wt[w][threadIdx.x & 63] = s;
  __syncthreads();
  unsigned run = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < SCAN_W; ++j) {
    const unsigned x = wt[j][threadIdx.x & 63];
    run += j < (int)w ? x : 0u;
    tot += x;
  }
  if (w == 0) dtot[q * RADIX + d] = tot;
  for (unsigned t = t0; t < t1; ++t) {
    const unsigned x = col[(size_t)t * RADIX];
    col[(size_t)t * RADIX] = run;
    run += x;
  }
}

// block = tile t of segment q: every slot goes to (start of its digit in the segment) + (slots of that digit in the tiles in
// front) + (slots of that digit in front of it inside the tile).  The last is formed in input order: wave w owns slots
// [w * ROUNDS * 64, (w + 1) * ROUNDS * 64) of the tile, a round is 64 consecutive slots, the lanes of one digit find each
// other by eight ballots, and cnt[w][digit] carries the wave's count from round to round (LDS operations of one wave complete
// in order: every lane reads before the group's first lane writes).
__global__ __launch_bounds__(ST) void lovasz_scatter_kernel(const unsigned* __restrict__ win, const unsigned* __restrict__ pin,
                                                            unsigned* __restrict__ wout, unsigned* __restrict__ pout, long L,
                                                            unsigned TS, int shift, const unsigned* __restrict__ off,
                                                            const unsigned* __restrict__ dtot) {
  __shared__ volatile unsigned cnt[NW][RADIX];
  __shared__ unsigned base[RADIX];
  __shared__ unsigned wsum[NW];
  const unsigned blk = blockIdx.x, q = blk / TS, t = blk - q * TS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int j = 0; j < NW; ++j) cnt[j][tid] = 0;
  // thread = digit: start of the digit in the segment (exclusive sum of the totals) + the tiles in front
  unsigned all;
  base[tid] = block_scan<NW>(dtot[q * RADIX + tid], wsum, all) + off[(size_t)blk * RADIX + tid];

  const long sb = (long)q * L;
  const long i0 = (long)t * TILE + w * (ROUNDS * 64) + lane;
  unsigned word[ROUNDS], pay[ROUNDS], rk[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long i = i0 + r * 64, ic = i < L ? i : L - 1;   // clamped: an unconditional load, dropped below
    word[r] = win[sb + ic];
    pay[r] = pin[sb + ic];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const bool ok = i0 + r * 64 < L;
    const unsigned d = digit_of(word[r], shift);
    unsigned long long peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned rank = (unsigned)__popcll(peers & below), n = (unsigned)__popcll(peers);
    const unsigned pre = cnt[w][d];
    if (ok && rank == 0) cnt[w][d] = pre + n;
    rk[r] = pre + rank;
  }
  __syncthreads();
  {                                      // thread = digit: a wave's count -> the count of the waves in front
    unsigned run = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const unsigned x = cnt[j][tid];
      cnt[j][tid] = run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const bool ok = i0 + r * 64 < L;
    const unsigned d = digit_of(word[r], shift);
    const unsigned pos = base[d] + cnt[w][d] + rk[r];
    if (ok && (long)pos < L) {           // pos < L by construction; the comparison keeps a wrong count inside the segment
      wout[sb + pos] = word[r];
      pout[sb + pos] = pay[r];
    }
  }
}

// ---- scan of the fg bit and the terms ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST) void lovasz_count_kernel(const unsigned* __restrict__ words, const unsigned* __restrict__ pays,
                                                          long L, unsigned TS, unsigned* __restrict__ tf,
                                                          unsigned* __restrict__ tn) {
  __shared__ unsigned sf[NW], sn[NW];
  const unsigned blk = blockIdx.x, q = blk / TS, t = blk - q * TS;
  const long sb = (long)q * L, i0 = (long)t * TILE + threadIdx.x;
  unsigned f = 0, n = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long i = i0 + r * ST;
    if (i < L) {
      f += pays[sb + i] >> 31;
      n += words[sb + i] != 0u ? 1u : 0u;
    }
  }
  f = wave_sum(f); n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) { sf[threadIdx.x >> 6] = f; sn[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = 0, b = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) { a += sf[j]; b += sn[j]; }
    tf[blk] = a;
    tn[blk] = b;
  }
}

// block = segment q: tf becomes the exclusive sum over the tiles in front; gn[q] = G, gn[Q + q] = the counted slots
__global__ __launch_bounds__(SCAN_T) void lovasz_fgscan_kernel(unsigned* __restrict__ tf, const unsigned* __restrict__ tn,
                                                               unsigned TS, unsigned Q, unsigned* __restrict__ gn) {
  __shared__ unsigned ws[SCAN_W], wn[SCAN_W];
  const unsigned q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned* const f = tf + (size_t)q * TS;
  const unsigned* const n = tn + (size_t)q * TS;
  unsigned carry = 0, nacc = 0;
  for (unsigned base = 0; base < TS; base += SCAN_T) {
    const unsigned i = base + tid;
    const unsigned v = i < TS ? f[i] : 0u;
    nacc += i < TS ? n[i] : 0u;
    unsigned tot;
    const unsigned ex = carry + block_scan<SCAN_W>(v, ws, tot);
    if (i < TS) f[i] = ex;
    carry += tot;
  }
  nacc = wave_sum(nacc);
  if (lane == 0) wn[w] = nacc;
  __syncthreads();
  if (tid == 0) {
    unsigned tot = 0;
#pragma unroll
    for (int j = 0; j < SCAN_W; ++j) tot += wn[j];
    gn[q] = carry;
    gn[Q + q] = tot;
  }
}

// J_i = 1 - (G - F) / (G + i - F) from integers (i >= 1, so the divisor is >= 1)
__device__ __forceinline__ double jaccard(unsigned G, unsigned F, unsigned i) {
  return 1.0 - (double)(G - F) / (double)((G - F) + i);
}

// the block that arrived last.  Wave w takes the segments s = w, w + NW, ...: per class the tile partials in one fixed order
// (lane l adds tiles l, l + 64, ..., then the butterfly), the entering classes, a_{s,c}, loss_s; then the waves' sums in order.
// state (float64): [0] loss, [1] n, then [S][C] each: L, a, G, enters; then n_s [S]
__device__ __forceinline__ void lovasz_finalize_block(const double* __restrict__ part, const unsigned* __restrict__ gn,
                                                      const float* __restrict__ cw, unsigned S, int C, unsigned TS, int all,
                                                      double* __restrict__ state, float* __restrict__ loss_out) {
  __shared__ double wl[NW], wc[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t Q = (size_t)S * C;
  double lsum = 0.0, nsum = 0.0;
  for (unsigned s = w; s < S; s += NW) {
    const unsigned ns = gn[Q + s];       // the counted slots of class 0's segment: the counted pixels of s
    double num = 0.0, den = 0.0;
    for (int c = 0; c < C; ++c) {
      const size_t q = (size_t)c * S + s;
      double acc = 0.0;
      for (unsigned t = lane; t < TS; t += 64) acc += part[q * TS + t];
      acc = wave_sum(acc);
      const unsigned G = gn[q];
      const double wt = cw != nullptr ? (double)cw[c] : 1.0;
      const bool enters = ns > 0 && (all != 0 || G > 0);
      if (enters) { num += wt * acc; den += wt; }
      if (lane == 0) {
        state[2 + (size_t)s * C + c] = acc;
        state[2 + 2 * Q + (size_t)s * C + c] = (double)G;
        state[2 + 3 * Q + (size_t)s * C + c] = enters ? 1.0 : 0.0;
      }
    }
    for (int c = 0; c < C; ++c) {
      const unsigned G = gn[(size_t)c * S + s];
      const double wt = cw != nullptr ? (double)cw[c] : 1.0;
      const bool enters = ns > 0 && (all != 0 || G > 0);
      const float a = (enters && den > 0.0) ? (float)(wt / ((double)S * den)) : 0.f;
      if (lane == 0) state[2 + Q + (size_t)s * C + c] = (double)a;
    }
    lsum += den > 0.0 ? num / den : 0.0;
    nsum += (double)ns;
    if (lane == 0) state[2 + 4 * Q + s] = (double)ns;
  }
  if (lane == 0) { wl[w] = lsum; wc[w] = nsum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0, n = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) { tot += wl[j]; n += wc[j]; }
    const float loss = (float)(tot / (double)S);
    state[0] = (double)loss;
    state[1] = n;
    if (loss_out) *loss_out = loss;
  }
}

// block = tile t of segment q of the sorted order (the scatter's slot map: wave w owns ROUNDS * 64 consecutive slots)
__global__ __launch_bounds__(ST) void lovasz_terms_kernel(const unsigned* __restrict__ words, const unsigned* __restrict__ pays,
                                                          long L, unsigned TS, unsigned S, int C, int all,
                                                          const unsigned* __restrict__ tf, const unsigned* __restrict__ gn,
                                                          const float* __restrict__ cw, float* __restrict__ coef,
                                                          double* __restrict__ part, double* __restrict__ state,
                                                          float* __restrict__ loss_out, unsigned* __restrict__ ticket) {
  __shared__ unsigned wf[NW];
  __shared__ double wp[NW];
  __shared__ int last;
  const unsigned blk = blockIdx.x, q = blk / TS, t = blk - q * TS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long sb = (long)q * L;
  const long i0 = (long)t * TILE + w * (ROUNDS * 64) + lane;
  const unsigned G = gn[q], F0 = tf[blk];
  unsigned word[ROUNDS], pay[ROUNDS];
  unsigned long long bal[ROUNDS];
  unsigned wtot = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long i = i0 + r * 64;
    const bool ok = i < L;
    const long ic = ok ? i : L - 1;
    word[r] = words[sb + ic];
    pay[r] = pays[sb + ic];
    bal[r] = __ballot(ok && (pay[r] >> 31) != 0u);
    wtot += (unsigned)__popcll(bal[r]);
  }
  if (lane == 0) wf[w] = wtot;
  __syncthreads();
  unsigned run = F0;
#pragma unroll
  for (int j = 0; j < NW; ++j) run += j < w ? wf[j] : 0u;
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const long i = i0 + r * 64;
    const bool ok = i < L;
    const unsigned fg = pay[r] >> 31;
    const unsigned F = run + (unsigned)__popcll(bal[r] & upto);   // fg slots among the sorted positions 1 .. i + 1
    run += (unsigned)__popcll(bal[r]);
    const unsigned pos = (unsigned)i + 1u;
    const double Ji = jaccard(G, F, pos);
    const double Jp = pos == 1u ? 0.0 : jaccard(G, F - fg, pos - 1u);
    const double g = Ji - Jp;
    const bool counted = ok && word[r] != 0u;
    const float err = word[r] == NAN_WORD ? NAN : __uint_as_float(word[r] - 1u);
    acc += counted ? (double)err * g : 0.0;
    const unsigned idx = pay[r] & 0x7FFFFFFFu;
    if (ok && (long)idx < L) coef[sb + idx] = counted ? (fg ? -(float)g : (float)g) : 0.f;
  }
  acc = wave_sum(acc);
  if (lane == 0) wp[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) s += wp[j];   // fixed order
    part[blk] = s;
  }
  if (last_arriver(ticket, gridDim.x, &last)) lovasz_finalize_block(part, gn, cw, S, C, TS, all, state, loss_out);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// t_c = (a_{s,c} * coef_c) * p_c, A = sum_c t_c (class order from 0.f), dlogits_j = grad_out * (t_j - p_j * A)
template <int NC>
__global__ __launch_bounds__(256) void lovasz_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                         const float* __restrict__ coef, const double* __restrict__ state,
                                                         const float* __restrict__ gout, long P, long HW, int C, unsigned S,
                                                         int ignore_index, int per_image, float* __restrict__ dlogits) {
  const float go = gout[0];
  const double* const a = state + 2 + (size_t)S * C;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    long b, r; split_hw(p, HW, b, r);
    float raw[NC], pr[NC], t[NC];
    load_classes<NC>(logits, b, r, C, HW, raw);
    const long long y = labels[p];
    const long s = per_image ? b : 0;
    softmax_of<NC>(raw, C, pr);
    const bool counted = y >= 0 && y < C && y != ignore_index;
    float A = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int kc = k < C ? k : C - 1;
      const float ak = (float)a[s * C + kc], ck = coef[(long)kc * P + p];
      t[k] = (k < C) ? (ak * ck) * pr[k] : 0.f;
      A += t[k];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < C) dlogits[(b * C + k) * HW + r] = counted ? go * (t[k] - pr[k] * A) : 0.f;
  }
}

int check_shape(const char* name, const void* logits, const void* labels, int N, int C, long HW, int per_image) {
  SEGK_REQUIRE(logits != nullptr, "%s: null logits", name);
  SEGK_REQUIRE(labels != nullptr, "%s: null labels", name);
  SEGK_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)labels & 7) == 0, "%s: misaligned buffer", name);
  SEGK_REQUIRE(C >= 1 && C <= MAXC, "%s: 1..%d classes supported, got %d", name, MAXC, C);
  SEGK_REQUIRE(N > 0 && HW > 0 && HW < (1L << 31), "%s: bad shape N=%d HW=%ld", name, N, HW);
  SEGK_REQUIRE((long)N * HW < (1L << 31), "%s: pixels are indexed with 32 bits: %ld pixels", name, (long)N * HW);
  SEGK_REQUIRE(per_image == 0 || per_image == 1, "%s: per_image must be 0 or 1, got %d", name, per_image);
  return 0;
}
}  // namespace

extern "C" int segk_lovasz_fwd(const float* logits, const int64_t* labels, const float* class_weights, int N, int C, long HW,
                               int ignore_index, int per_image, int classes, void* scratch, long scratch_bytes, float* coef,
                               double* state, float* loss_out, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (const int rc = check_shape("lovasz_fwd", logits, labels, N, C, HW, per_image)) return rc;
  SEGK_REQUIRE(classes == SEGK_LOVASZ_PRESENT || classes == SEGK_LOVASZ_ALL, "lovasz_fwd: classes must be 0 (present) or 1 (all), got %d",
               classes);
  SEGK_REQUIRE(scratch != nullptr, "lovasz_fwd: null scratch");
  SEGK_REQUIRE(coef != nullptr, "lovasz_fwd: null coefficient buffer");
  SEGK_REQUIRE(state != nullptr, "lovasz_fwd: null state");
  SEGK_REQUIRE(((uintptr_t)class_weights & 3) == 0 && ((uintptr_t)scratch & 15) == 0 && ((uintptr_t)coef & 3) == 0 &&
               ((uintptr_t)state & 7) == 0 && ((uintptr_t)loss_out & 3) == 0, "lovasz_fwd: misaligned buffer");
  const long P = (long)N * HW, S = per_image ? N : 1, L = P / S, Q = S * C;
  const long need = SEGK_LOVASZ_SCRATCH_BYTES((long)C, P, S);
  SEGK_REQUIRE(scratch_bytes >= need, "lovasz_fwd: %ld bytes of scratch, SEGK_LOVASZ_SCRATCH_BYTES(%d, %ld, %ld) = %ld needed",
               scratch_bytes, C, P, S, need);
  const long TS = (L + TILE - 1) / TILE, NT = Q * TS;
  SEGK_REQUIRE(NT < (1L << 31) && Q * 4 < (1L << 31), "lovasz_fwd: %ld tiles", NT);
  const Lay l = lay_of(scratch, (long)C * P, NT, Q);
  unsigned* const ticket = segk_ticket_slot(1, st);
  SEGK_REQUIRE(ticket != nullptr, "lovasz_fwd: no ticket array");
  const int nb = segk_loss_blocks(P);
  SEGK_REQUIRE(nb >= 1 && nb <= LROWS, "lovasz_fwd: bad block count %d", nb);
  dispatch_loss_nc(C, [&](auto NCc) {
    hipLaunchKernelGGL((lovasz_keys_kernel<decltype(NCc)::value>), dim3(nb), dim3(LT), 0, st, logits, (const long long*)labels, P,
                       HW, C, ignore_index, per_image, l.wa, l.pa);
  });
  SEGK_CHECK_LAUNCH("lovasz_fwd (keys)");
  unsigned *wi = l.wa, *pi = l.pa, *wo = l.wb, *po = l.pb;
  for (int pass = 0; pass < PASSES; ++pass) {                  // an even count: the sorted order ends where the keys began
    const int shift = 8 * pass;
    hipLaunchKernelGGL(lovasz_hist_kernel, dim3((unsigned)NT), dim3(ST), 0, st, wi, L, (unsigned)TS, shift, l.hist);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3((unsigned)(Q * 4)), dim3(SCAN_T), 0, st, l.hist, (unsigned)TS, l.dtot);
    hipLaunchKernelGGL(lovasz_scatter_kernel, dim3((unsigned)NT), dim3(ST), 0, st, wi, pi, wo, po, L, (unsigned)TS, shift, l.hist,
                       l.dtot);
    SEGK_CHECK_LAUNCH("lovasz_fwd (sort)");
    unsigned* x = wi; wi = wo; wo = x;
    x = pi; pi = po; po = x;
  }
  static_assert(PASSES % 2 == 0, "the header says where the sorted order lies");
  hipLaunchKernelGGL(lovasz_count_kernel, dim3((unsigned)NT), dim3(ST), 0, st, wi, pi, L, (unsigned)TS, l.tf, l.tn);
  hipLaunchKernelGGL(lovasz_fgscan_kernel, dim3((unsigned)Q), dim3(SCAN_T), 0, st, l.tf, l.tn, (unsigned)TS, (unsigned)Q, l.gn);
  hipLaunchKernelGGL(lovasz_terms_kernel, dim3((unsigned)NT), dim3(ST), 0, st, wi, pi, L, (unsigned)TS, (unsigned)S, C,
                     classes == SEGK_LOVASZ_ALL ? 1 : 0, l.tf, l.gn, class_weights, coef, l.part, state, loss_out, ticket);
  SEGK_CHECK_LAUNCH("lovasz_fwd (terms)");
  return 0;
}

extern "C" int segk_lovasz_bwd(const float* logits, const int64_t* labels, const float* coef, const double* state,
                               const float* grad_out, int N, int C, long HW, int ignore_index, int per_image, float* dlogits,
                               segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  if (const int rc = check_shape("lovasz_bwd", logits, labels, N, C, HW, per_image)) return rc;
  SEGK_REQUIRE(coef != nullptr, "lovasz_bwd: null coefficient buffer");
  SEGK_REQUIRE(state != nullptr, "lovasz_bwd: null state");
  SEGK_REQUIRE(grad_out != nullptr, "lovasz_bwd: null upstream gradient");
  SEGK_REQUIRE(dlogits != nullptr, "lovasz_bwd: null gradient buffer");
  SEGK_REQUIRE(((uintptr_t)coef & 3) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)grad_out & 3) == 0 &&
               ((uintptr_t)dlogits & 3) == 0, "lovasz_bwd: misaligned buffer");
  const long P = (long)N * HW;
  long g = (P + 255) / 256;
  if (g > 4096) g = 4096;
  dispatch_loss_nc(C, [&](auto NCc) {
    hipLaunchKernelGGL((lovasz_bwd_kernel<decltype(NCc)::value>), dim3((int)g), dim3(256), 0, st, logits, (const long long*)labels,
                       coef, state, grad_out, P, HW, C, (unsigned)(per_image ? N : 1), ignore_index, per_image, dlogits);
  });
  SEGK_CHECK_LAUNCH("lovasz_bwd");
  return 0;
}
