// The integer building blocks of the object kernels: components.hip, lovasz.hip, vectors.hip and
// panoptic.hip count, scan and collapse with these.  Everything here is integer arithmetic whose result does not depend on
// who arrives first; a workgroup is 64 * NW threads in x, and every function that holds a barrier or a ballot is called by
// all of its threads together.
//   block_scan<NW>      exclusive prefix of one value per thread over the workgroup, and the total
//   wg_scan<T>          ONE workgroup of 256: exclusive prefix sums of an array in global memory, 1024 items per trip
//   run_length<T>       run heads of a wave's 64 consecutive keys
//   tab_slot / AddTable a small open LDS table that turns a workgroup's adds to one word into one global atomic
#pragma once
#include "common.hpp"

typedef unsigned long long u64;

__host__ __device__ inline long r4(long n) { return (n + 3) / 4 * 4; }

// a word that other workgroups move with atomics while this one reads it
__device__ __forceinline__ int dev_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 dev_load64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// flat index and grid stride of a launch of 256-thread workgroups
__device__ __forceinline__ long thread_of(void) { return (long)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ long stride_of(void) { return (long)gridDim.x * 256; }

// exclusive prefix of v over the 64 * NW threads of the workgroup, and the sum of all in `total`; s_w: NW words of LDS.  Calls
// may follow each other on the same s_w: the first barrier holds a call until the words of the one before have been read.
template <int NW, typename T>
__device__ __forceinline__ T block_scan(T v, T* s_w, T& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  __syncthreads();                     // the words of the call before have been read
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const T t = s_w[w];
    if (w < wv) base += t;
    total += t;
  }
  return base + inc - v;
}

// ONE workgroup of 256 threads: dst[0..n) = the exclusive prefix sums of src[0..n), returns the sum of all.  dst may be src:
// a trip reads its 1024 items (4 consecutive per thread, the workgroup's loads coalesced) before it writes any.
template <typename T>
__device__ __forceinline__ T wg_scan(const T* src, T* dst, long n) {
  __shared__ T s_w[4];
  T carry = 0;
  for (long i0 = 0; i0 < n; i0 += 1024) {
    const long i = i0 + 4 * threadIdx.x;
    T v[4], sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = i + k < n ? src[i + k] : (T)0;
      sum += v[k];
    }
    T total;
    T ex = carry + block_scan<4>(sum, s_w, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < n) dst[i + k] = ex;
      ex += v[k];
    }
    carry += total;
  }
  return carry;
}

// run heads of a wave's 64 keys: a lane starts a run where its key differs from the lane before; returns the run length for
// a head lane (0 otherwise)
template <typename T>
__device__ __forceinline__ int run_length(T key, int lane) {
  const T prev = __shfl_up(key, 1);
  const bool head = lane == 0 || prev != key;
  const u64 heads = __ballot(head);
  if (!head) return 0;
  const u64 upper = lane == 63 ? 0ull : heads >> (lane + 1);
  return upper ? __ffsll((long long)upper) : 64 - lane;
}

// A small open table in LDS keyed by an integer >= 0 (-1: empty): what a workgroup adds under one key leaves as ONE global
// atomic (a large component, or a segment that meets thousands of others, would otherwise take an atomic per item on the same
// address from every workgroup).  A key that finds its slot taken by another goes to global memory directly: the sums are
// integers, the route does not show.
template <int SLOTS>
__device__ __forceinline__ int tab_slot(int* keys, int key) {         // the key's slot, or -1
  static_assert(SLOTS >= 2 && (SLOTS & (SLOTS - 1)) == 0, "the hash keeps the top log2(SLOTS) bits");
  const int h = (int)(((unsigned)key * 2654435761u) >> (32 - __builtin_ctz(SLOTS)));
  const int old = atomicCAS(keys + h, -1, key);
  return (old == -1 || old == key) ? h : -1;
}

template <int SLOTS>
struct AddTable {                      // __shared__; a barrier after clear() and one before flush()
  int key[SLOTS], val[SLOTS];
  __device__ __forceinline__ void clear() {
    if (threadIdx.x < SLOTS) { key[threadIdx.x] = -1; val[threadIdx.x] = 0; }
  }
  // n more under key k; `word` is where k's sum lives in global memory
  __device__ __forceinline__ void add(int k, int n, int* word) {
    const int h = tab_slot<SLOTS>(key, k);
    if (h >= 0) atomicAdd(val + h, n);
    else atomicAdd(word, n);
  }
  // thread i sends slot i to word_of(its key)
  template <typename F>
  __device__ __forceinline__ void flush(F word_of) {
    if (threadIdx.x < SLOTS && key[threadIdx.x] >= 0) atomicAdd(word_of(key[threadIdx.x]), val[threadIdx.x]);
  }
};
