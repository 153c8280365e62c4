// The optimizer step of the train loop: global-norm gradient clipping, AdamW and a weight EMA as ONE streaming pass over
// every parameter (segk_optim_adamw), behind one deterministic norm pass (segk_optim_grad_norm) when clipping or the
// non-finite skip is on.  Replaces the notebooks' `AdamW(weight_decay=0.01)` cell (torch.optim.AdamW,
// the one layer of the train step that was still stock) and what users compose around it (clip_grad_norm_, a _foreach_lerp_
// EMA).  The arithmetic is DEFINED in DESIGN section 3.13 and restated in tests/optim_reference.py; this file is held to it
// bit for bit (-ffp-contract=off: every operation below rounds once).
//
// Both entries walk one device table (segk_optim_rec, sorted by block0): a tensor owns ceil(numel / SEGK_OPTIM_CHUNK)
// consecutive blocks, a block finds its record by a binary search over block0 (uniform: scalar loads) and works on one chunk.
//
// Device step state (`state`, 32 + 2 * (8 + 16 * ngroups) bytes, caller-owned, persists across steps):
//   head   { double norm; float clip; int32 finite; int32 skipped; int32 pad[3] }
//   slot k { int32 t; int32 pad; double pow[ngroups][2] }      k = 0, 1: pow = (beta1^t, beta2^t) as RUNNING products
// A step reads slot `parity` and writes slot `parity ^ 1`; the host flips parity with every step it launches.  Nobody reads
// the slot that is written in the same launch, so the block that advances the state needs no ordering against the others:
//   - with the norm pass, its finishing block writes the next slot (advanced, or copied when the step is skipped) and the
//     update kernel reads that slot;
//   - without it, every block of the update kernel derives t + 1 and pow * beta from the current slot in registers (one
//     multiplication: the same bits in every block) and block 0 also stores them to the next slot.
#include "common.hpp"
#include "segk_internal.h"
#include "ticket.hpp"
#include "../../include/segk.h"
#include <math.h>

namespace {

constexpr int CHUNK = SEGK_OPTIM_CHUNK, NT = 256, SWEEPS = CHUNK / (4 * NT), NORM_CHUNKS = 8;
static_assert(CHUNK == 4 * NT * SWEEPS && SWEEPS == 4, "a chunk is four float4 sweeps of the block");
static_assert(sizeof(segk_optim_rec) == 64 && sizeof(segk_optim_group) == 64, "table records are 64 bytes");

struct OptimHead { double norm; float clip; int finite; int skipped; int pad_[3]; };
static_assert(sizeof(OptimHead) == 32, "state head is 32 bytes");
struct OptimSlot { int t; int pad_; double pow[2]; };     // pow[2 * ngroups] really

__device__ __forceinline__ OptimSlot* optim_slot(char* state, int k, int G) {
  return (OptimSlot*)(state + sizeof(OptimHead) + (size_t)k * (8 + 16 * (size_t)G));
}

// Pointers read from the table are generic to the compiler (flat loads); they are device memory: say so
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) double gf64;
__device__ __forceinline__ gf32* gl(const float* p) { return (gf32*)p; }
__device__ __forceinline__ gf32x4* gl4(const float* p) { return (gf32x4*)p; }

// the record whose chunks contain chunk `c`: table[lo].block0 <= c < table[lo + 1].block0
__device__ __forceinline__ int find_idx(const segk_optim_rec* __restrict__ table, int n, int c) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c >= table[mid].block0) lo = mid; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ const segk_optim_rec& find_rec(const segk_optim_rec* __restrict__ table, int n) {
  return table[find_idx(table, n, (int)blockIdx.x)];
}

// elements of this block's chunk: >= 1 when the host gave the tensor ceil(numel / CHUNK) blocks; a table that lies gets 0
__device__ __forceinline__ int chunk_count(long long left) { return left < CHUNK ? (left > 0 ? (int)left : 0) : CHUNK; }

__device__ __forceinline__ double wave_sum_f64(double v) {       // xor butterfly: a fixed tree, the same bits in every lane
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// every thread's value -> the block's sum in thread 0 (waves in order)
__device__ __forceinline__ double block_sum_f64(double v, double* wsum) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// ---- 1. sum of squares of every gradient of the table, float64, fixed order ------------------------------------------------
// A block takes NORM_CHUNKS consecutive chunks (one arrival at the ticket per 32 K elements: 7 635 arrivals at one word cost
// the U-Net's norm 280 us, profiles/optim_kbench.txt).  Element j of a chunk belongs to thread (j / 4) % 256, which adds its
// elements' squares chunk after chunk, in increasing j (a float32 squared is exact in float64); then the butterfly, the four
// waves in order: one partial per block.  The last block to arrive sums the partials -- thread i takes partials i, i + 256, ... in that order, then the same tree -- and finishes the step state.
__global__ __launch_bounds__(NT) void optim_grad_norm_kernel(const segk_optim_rec* __restrict__ table, int n,
                                                             int total_chunks, const segk_optim_group* __restrict__ groups,
                                                             int G, char* state, double* part, double max_norm, int flags,
                                                             int parity, unsigned* ticket) {
  __shared__ double wsum[4];
  __shared__ int last;
  const int tid = threadIdx.x;
  const int c0 = (int)blockIdx.x * NORM_CHUNKS, c1 = c0 + NORM_CHUNKS < total_chunks ? c0 + NORM_CHUNKS : total_chunks;
  double acc = 0.0;
  int lo = 0, next0 = c0;                                            // the first chunk searches; its successors mostly stay
  for (int c = c0; c < c1; ++c) {
    if (c >= next0) {
      lo = find_idx(table, n, c);
      next0 = lo + 1 < n ? table[lo + 1].block0 : 0x7fffffff;
    }
    const segk_optim_rec& r = table[lo];
    const long long i0 = (long long)(c - r.block0) * CHUNK;
    const int cnt = chunk_count(r.numel - i0);
    const float* g = r.g + i0;
    const int nfull = (((uintptr_t)r.g & 15) == 0) ? (cnt >> 2) : 0;   // whole 16-byte vectors of this chunk
    if (nfull > 0) {                                                   // uniform
      f32x4 x[SWEEPS];
#pragma unroll
      for (int k = 0; k < SWEEPS; ++k) {                               // unconditional loads of a clamped vector
        const int vi = k * NT + tid;
        x[k] = gl4(g)[vi < nfull ? vi : nfull - 1];
      }
#pragma unroll
      for (int k = 0; k < SWEEPS; ++k) {
        const bool in = k * NT + tid < nfull;
        acc += in ? (double)x[k].x * (double)x[k].x : 0.0;
        acc += in ? (double)x[k].y * (double)x[k].y : 0.0;
        acc += in ? (double)x[k].z * (double)x[k].z : 0.0;
        acc += in ? (double)x[k].w * (double)x[k].w : 0.0;
      }
    }
    if (nfull * 4 < cnt) {                                             // uniform: a tail, or a record that is not 16-byte aligned
      float y[4 * SWEEPS];
#pragma unroll
      for (int q = 0; q < 4 * SWEEPS; ++q) {
        const int j = (q >> 2) * (4 * NT) + tid * 4 + (q & 3);
        y[q] = gl(g)[j < cnt ? j : cnt - 1];
      }
#pragma unroll
      for (int q = 0; q < 4 * SWEEPS; ++q) {
        const int j = (q >> 2) * (4 * NT) + tid * 4 + (q & 3);
        acc += (j >= nfull * 4 && j < cnt) ? (double)y[q] * (double)y[q] : 0.0;
      }
    }
  }
  const double b = block_sum_f64(acc, wsum);
  if (tid == 0) part[blockIdx.x] = b;
  if (!last_arriver(ticket, gridDim.x, &last)) return;

  const int NB = (int)gridDim.x;
  OptimHead* h = (OptimHead*)state;
  const OptimSlot* cur = optim_slot(state, parity, G);
  OptimSlot* nxt = optim_slot(state, parity ^ 1, G);
  const int t_cur = cur->t, skipped = h->skipped;                    // issued ahead of the walk, not behind it
  double s = 0.0;
  for (int m0 = tid; m0 < NB; m0 += 8 * NT) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ((gf64*)part)[m0 + u * NT < NB ? m0 + u * NT : NB - 1];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (m0 + u * NT < NB) ? v[u] : 0.0;
  }
  __syncthreads();                                                   // wsum is reused
  const double sumsq = block_sum_f64(s, wsum);
  const bool finite = sumsq - sumsq == 0.0;                          // inf and NaN both fail
  const bool apply = finite || !(flags & SEGK_OPTIM_SKIP_NONFINITE);
  for (int i = tid; i < G; i += NT) {                                // the running products: one multiplication per step
    const double p1 = cur->pow[2 * i], p2 = cur->pow[2 * i + 1];
    nxt->pow[2 * i] = apply ? p1 * groups[i].beta1 : p1;
    nxt->pow[2 * i + 1] = apply ? p2 * groups[i].beta2 : p2;
  }
  if (tid != 0) return;
  const double norm = sqrt(sumsq);
  float c = 1.0f;
  if (flags & SEGK_OPTIM_CLIP) {
    const double q = max_norm / (norm + 1e-6);
    c = (q < 1.0 || q != q) ? (float)q : 1.0f;                       // min(1, q), a NaN norm stays NaN as in clip_grad_norm_
  }
  h->norm = norm;
  h->clip = c;
  h->finite = finite ? 1 : 0;
  h->skipped = skipped + (apply ? 0 : 1);
  nxt->t = t_cur + (apply ? 1 : 0);
}

// ---- 2. the update ---------------------------------------------------------------------------------------------------------
struct StepK { float c, decay, omb1, b2, omb2, eps, step, bc2s, omd; };

// DESIGN 3.13, in torch.optim.AdamW's order; every operation rounds once
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }
__device__ __forceinline__ f32x4 sqrt_rn(f32x4 x) { return (f32x4){sqrtf(x.x), sqrtf(x.y), sqrtf(x.z), sqrtf(x.w)}; }
template <typename T>      // float, or four of them: the same operations lane by lane
__device__ __forceinline__ void adamw_elem(T g, T& p, T& m, T& v, const StepK& k) {
  const T gc = g * k.c;
  const T pd = p * k.decay;
  const T mn = m + (gc - m) * k.omb1;
  const T vn = v * k.b2 + (gc * gc) * k.omb2;
  const T den = sqrt_rn(vn) / k.bc2s + k.eps;
  p = pd - (mn / den) * k.step;
  m = mn;
  v = vn;
}
template <typename T>
__device__ __forceinline__ T ema_elem(T s, T p, const StepK& k) { return s + (p - s) * k.omd; }

template <bool EMA>
__device__ __forceinline__ void adamw_chunk(const segk_optim_rec& r, long long i0, int cnt, const StepK& k) {
  gf32 *g = gl(r.g + i0), *p = gl(r.p + i0), *m = gl(r.m + i0), *v = gl(r.v + i0), *s = EMA ? gl(r.shadow + i0) : nullptr;
  const int tid = threadIdx.x;
  const uintptr_t bits = (uintptr_t)r.g | (uintptr_t)r.p | (uintptr_t)r.m | (uintptr_t)r.v | (EMA ? (uintptr_t)r.shadow : 0);
  const int nfull = ((bits & 15) == 0) ? (cnt >> 2) : 0;
  if (nfull > 0) {                                                   // uniform
    f32x4 xg[SWEEPS], xp[SWEEPS], xm[SWEEPS], xv[SWEEPS], xs[EMA ? SWEEPS : 1];
#pragma unroll
    for (int q = 0; q < SWEEPS; ++q) {                               // unconditional loads of a clamped vector
      const int vi = q * NT + tid, vc = vi < nfull ? vi : nfull - 1;
      xg[q] = ((gf32x4*)g)[vc]; xp[q] = ((gf32x4*)p)[vc];
      xm[q] = ((gf32x4*)m)[vc]; xv[q] = ((gf32x4*)v)[vc];
      if constexpr (EMA) xs[q] = ((gf32x4*)s)[vc];
    }
#pragma unroll
    for (int q = 0; q < SWEEPS; ++q) {
      const int vi = q * NT + tid;
      adamw_elem(xg[q], xp[q], xm[q], xv[q], k);
      if constexpr (EMA) xs[q] = ema_elem(xs[q], xp[q], k);
      if (vi < nfull) {
        ((gf32x4*)p)[vi] = xp[q]; ((gf32x4*)m)[vi] = xm[q]; ((gf32x4*)v)[vi] = xv[q];
        if constexpr (EMA) ((gf32x4*)s)[vi] = xs[q];
      }
    }
  }
#pragma unroll 1
  for (int j = nfull * 4 + tid; j < cnt; j += NT) {                  // tensor tails; records that are not 16-byte aligned
    float pj = p[j], mj = m[j], vj = v[j];
    adamw_elem((float)g[j], pj, mj, vj, k);
    if constexpr (EMA) s[j] = ema_elem((float)s[j], pj, k);
    p[j] = pj; m[j] = mj; v[j] = vj;
  }
}

__global__ __launch_bounds__(NT) void optim_adamw_kernel(const segk_optim_rec* __restrict__ table, int n,
                                                         const segk_optim_group* __restrict__ groups, int G, char* state,
                                                         int flags, int parity) {
  const bool normed = flags & SEGK_OPTIM_NORMED;
  const OptimHead* h = (const OptimHead*)state;
  if (normed && (flags & SEGK_OPTIM_SKIP_NONFINITE) && !h->finite) return;     // uniform: the step is skipped, nothing is written
  // after the norm pass the next slot already holds this step's state; otherwise it is derived here from the current one
  const OptimSlot* rd = optim_slot(state, normed ? parity ^ 1 : parity, G);
  if (!normed && blockIdx.x == 0) {
    OptimSlot* nxt = optim_slot(state, parity ^ 1, G);
    for (int i = threadIdx.x; i < G; i += NT) {
      nxt->pow[2 * i] = rd->pow[2 * i] * groups[i].beta1;
      nxt->pow[2 * i + 1] = rd->pow[2 * i + 1] * groups[i].beta2;
    }
    if (threadIdx.x == 0) nxt->t = rd->t + 1;
  }
  const segk_optim_rec& r = find_rec(table, n);
  const int gi = r.group < 0 ? 0 : (r.group < G ? r.group : G - 1);
  const segk_optim_group gr = groups[gi];
  const int t = normed ? rd->t : rd->t + 1;
  const double p1 = normed ? rd->pow[2 * gi] : rd->pow[2 * gi] * gr.beta1;
  const double p2 = normed ? rd->pow[2 * gi + 1] : rd->pow[2 * gi + 1] * gr.beta2;
  StepK k;
  k.c = normed ? h->clip : 1.0f;
  k.decay = gr.decay; k.omb1 = gr.omb1; k.b2 = gr.b2; k.omb2 = gr.omb2; k.eps = gr.eps;
  const float bc1 = (float)(1.0 - p1), bc2 = (float)(1.0 - p2);      // the bias corrections, rounded to float32 once
  k.step = gr.lr / bc1;
  k.bc2s = sqrtf(bc2);
  k.omd = gr.omd;
  if (flags & SEGK_OPTIM_EMA_WARMUP) {
    const float tf = (float)t;
    k.omd = 1.0f - fminf(gr.ema_decay, (1.0f + tf) / (10.0f + tf));
  }
  const long long i0 = (long long)((int)blockIdx.x - r.block0) * CHUNK;
  const long long left = r.numel - i0;
  const int cnt = chunk_count(left);
  if (r.shadow) adamw_chunk<true>(r, i0, cnt, k);
  else adamw_chunk<false>(r, i0, cnt, k);
}

// ---- 3. parameters <-> shadow, in place (ema_weights()) --------------------------------------------------------------------
__global__ __launch_bounds__(NT) void optim_swap_kernel(const segk_optim_rec* __restrict__ table, int n) {
  const segk_optim_rec& r = find_rec(table, n);
  if (!r.shadow) return;
  const long long i0 = (long long)((int)blockIdx.x - r.block0) * CHUNK;
  const long long left = r.numel - i0;
  const int cnt = chunk_count(left);
  gf32 *p = gl(r.p + i0), *s = gl(r.shadow + i0);
  const int tid = threadIdx.x;
  const int nfull = ((((uintptr_t)r.p | (uintptr_t)r.shadow) & 15) == 0) ? (cnt >> 2) : 0;
  if (nfull > 0) {
    f32x4 xp[SWEEPS], xs[SWEEPS];
#pragma unroll
    for (int q = 0; q < SWEEPS; ++q) {
      const int vi = q * NT + tid, vc = vi < nfull ? vi : nfull - 1;
      xp[q] = ((gf32x4*)p)[vc]; xs[q] = ((gf32x4*)s)[vc];
    }
#pragma unroll
    for (int q = 0; q < SWEEPS; ++q) {
      const int vi = q * NT + tid;
      if (vi < nfull) { ((gf32x4*)p)[vi] = xs[q]; ((gf32x4*)s)[vi] = xp[q]; }
    }
  }
#pragma unroll 1
  for (int j = nfull * 4 + tid; j < cnt; j += NT) {
    const float a = p[j], b = s[j];
    p[j] = b; s[j] = a;
  }
}

}  // namespace

extern "C" int segk_optim_grad_norm(const segk_optim_rec* table, int n, int total_blocks, const segk_optim_group* groups,
                                    int ngroups, void* state, double* part, double max_norm, int flags, int parity,
                                    segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  SEGK_REQUIRE(table && groups && state && part, "optim_grad_norm: null pointer");
  SEGK_REQUIRE(n > 0 && total_blocks >= n && ngroups > 0 && ngroups <= SEGK_OPTIM_MAX_GROUPS,
               "optim_grad_norm: bad counts n=%d blocks=%d groups=%d", n, total_blocks, ngroups);
  SEGK_REQUIRE((flags & ~(SEGK_OPTIM_CLIP | SEGK_OPTIM_SKIP_NONFINITE)) == 0 && (parity == 0 || parity == 1),
               "optim_grad_norm: bad flags %d or parity %d", flags, parity);
  SEGK_REQUIRE(!(flags & SEGK_OPTIM_CLIP) || max_norm > 0.0, "optim_grad_norm: max_norm must be positive");
  unsigned* const ticket = segk_ticket_slot(1, st);
  SEGK_REQUIRE(ticket != nullptr, "optim_grad_norm: no ticket array");
  hipLaunchKernelGGL(optim_grad_norm_kernel, dim3(cdiv(total_blocks, NORM_CHUNKS)), dim3(NT), 0, st, table, n, total_blocks, groups,
                     ngroups, (char*)state, part, max_norm, flags, parity, ticket);
  SEGK_CHECK_LAUNCH("optim_grad_norm");
  return 0;
}

extern "C" int segk_optim_adamw(const segk_optim_rec* table, int n, int total_blocks, const segk_optim_group* groups, int ngroups,
                                void* state, int flags, int parity, segk_stream_t s) {
  hipStream_t st = (hipStream_t)s;
  const int known = SEGK_OPTIM_NORMED | SEGK_OPTIM_SKIP_NONFINITE | SEGK_OPTIM_EMA_WARMUP | SEGK_OPTIM_SWAP;
  SEGK_REQUIRE(table && n > 0 && total_blocks >= n, "optim_adamw: bad table n=%d blocks=%d", n, total_blocks);
  SEGK_REQUIRE((flags & ~known) == 0 && (parity == 0 || parity == 1), "optim_adamw: bad flags %d or parity %d", flags, parity);
  if (flags & SEGK_OPTIM_SWAP) {
    SEGK_REQUIRE(flags == SEGK_OPTIM_SWAP, "optim_adamw: the exchange takes no other flag (%d)", flags);
    hipLaunchKernelGGL(optim_swap_kernel, dim3(total_blocks), dim3(NT), 0, st, table, n);
    SEGK_CHECK_LAUNCH("optim_swap");
    return 0;
  }
  SEGK_REQUIRE(groups && state && ngroups > 0 && ngroups <= SEGK_OPTIM_MAX_GROUPS, "optim_adamw: bad groups (%d) or null state",
               ngroups);
  SEGK_REQUIRE(!(flags & SEGK_OPTIM_SKIP_NONFINITE) || (flags & SEGK_OPTIM_NORMED),
               "optim_adamw: the non-finite skip needs the norm pass");
  hipLaunchKernelGGL(optim_adamw_kernel, dim3(total_blocks), dim3(NT), 0, st, table, n, groups, ngroups, (char*)state, flags,
                     parity);
  SEGK_CHECK_LAUNCH("optim_adamw");
  return 0;
}
