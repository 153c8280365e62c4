// Shared pieces (layout, walk, piece map, transform, swizzle, slot map, statistics rows and tile store): conv_tile.hpp.
#include "conv_tile.hpp"

namespace {

// Producer / consumer 3x3 kernel for the MFMA-bound bf16 layers (channel tiles of 128, K = 9*Cin long).
//
// Why it exists (s_memtime traces and ablation builds of the symmetric 8-wave kernels at 512->512 @ 32x32,
// B = 32): with two MFMA waves per SIMD the matrix pipe arbitrates oldest-first, so the two waves of a SIMD
// run one after the other, and each is an in-order stream in which every staging instruction (global load,
// ds_write_b128, address arithmetic) behind MFMA k delays MFMA k+1 -- ~2070-2900 cycles per step for 1536
// cycles of matrix work, whatever the placement of the staging instructions inside the stream.
//
// Structure here: the 8 waves of a workgroup split into
//   * 4 CONSUMER waves (one per SIMD, raised priority), each owning a 128-pixel x 64-channel tile of the
//     256 x 128 workgroup tile: their stream is nothing but MFMAs and ds_read_b128 fragment reads (one
//     sub-step ahead; the first fragments of the next step are read BEFORE the barrier that ends the
//     current one);
//   * 4 PRODUCER waves (the SIMDs' second waves) that do all staging: weight steps through a ring of three
//     LDS buffers, stored two steps ahead of their use from registers fetched two steps before that, and
//     the next chunk's patch (BatchNorm+ReLU prologue and halo zero-fill applied on the way), stored one
//     step ahead.  Their waits (vmcnt, LDS-store queueing) no longer sit in any MFMA stream.
// One s_barrier per step joins the two roles.  The weight ring keeps running across work units (the epilogue
// tile overlays only [P0 | P1 | W2], dead at that point).  LDS: [W0 | W1 | P0 | P1 | W2].
// The consumers multiply with v_mfma_f32_16x16x32_bf16 (the same LDS bytes and matrix cycles per FLOP as 32x32x16; on random
// data the chip holds a ~12 % higher clock on the 16x16 shape: tools/ubench/mfma_tiles.hip 1.79 vs 1.60 PFLOP/s at this wave
// tile; on the whole step 0.5 % faster, and its producers' stores lose 6 % of their LDS cycles to bank conflicts instead of
// 22 %).  A 16x16x32 operand is 16 rows x one whole 64-byte chunk, so the LDS image is: patch pixels at a 96-byte pitch
// (conflict-free for 16 consecutive pixels at any tap shift), weight rows unpadded with the 16-byte piece index XOR-ed by
// [0,3,2,1][(row >> 2) & 3] (conflict-free, rows never shift).
// Diagnostic build only (-DSEGK_PIPE_STAMPS, tools/stamp_build.sh): per-wave cycle sums of the loop's phases, written
// over the statistics buffer by lane 0 of every wave; the shipped library contains no stamp.
#ifdef SEGK_PIPE_STAMPS
#define PIPE_STAMP(i)                                                                     \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    unsigned long long t_;                                                                \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
    stamp_sum[i] += t_ - stamp_last;                                                      \
    stamp_last = t_;                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#define PIPE_STAMP_OUT()                                                                  \
  do {                                                                                    \
    if (a.stats != nullptr && lane == 0) {                                                \
      unsigned long long* o_ = (unsigned long long*)a.stats + ((size_t)blockIdx.x * 8 + wave) * 8; \
      for (int i_ = 0; i_ < 6; ++i_) o_[i_] = stamp_sum[i_];                              \
      o_[6] = stamp_last - stamp_t0;                                                      \
    }                                                                                     \
  } while (0)
#else
#define PIPE_STAMP(i) do {} while (0)
#define PIPE_STAMP_OUT() do {} while (0)
#endif

// DMA (round 4; 16x16x32 consumers, no prologue): the producers move NOTHING through registers.  Weights and patch arrive by
// LDS-DMA (global_load_lds, 1 KiB per wave-instruction, out-of-image halo pixels from a zero page), so a staged KiB costs the
// SIMD one issue instead of a global load plus a ds_write_b128 (tools/ubench/pipe_roles.hip: +38 instead of +154 cycles per
// 1536-cycle step beside the consumer), and the consumers' matrix stream is the only LDS writer-free critical path.  A DMA
// instruction writes 64 consecutive 16-byte slots, so both images are unpadded and conflict freedom comes from WHICH piece a
// lane fetches: weight rows keep the XOR image above (it never had padding); the patch becomes rows of 8-pixel blocks of
// 512 B with piece q of pixel x at (x >> 3) * 512 + (q >> 1) * 256 + ((6 x + q) & 15) * 16 -- the slot map of conv_rs.hip,
// conflict-free for a 16-pixel operand read at ANY x shift; a 16-pixel block starts at x = 0 or 16, so the consumers need
// one per-lane address per tap column (three registers instead of eight) plus immediates.
// The DMA form also has NO EPILOGUE TILE and no boundary barriers: its consumers multiply channels x pixels (A = weights, B =
// patch; the weight rows a lane reads are permuted so that accumulator rows 4 lq + j of a pair of 16-channel blocks are 8
// consecutive channels of one pixel) and store 16 bytes per pixel and block pair straight from the accumulators; BatchNorm
// sums are reduced over the 16 pixel lanes with DPP adds and written as one partial row per (unit, consumer pixel half).
// Producers and consumers then run through unit boundaries like through any other step: the next unit's first patch chunk
// and weight steps land under this unit's last steps, and the 128 two-byte LDS stores + three barriers + 512-thread store
// pass of the staged epilogue (8 k cycles per unit: 30 % of a Cin = 128 unit) become ~100 vector instructions of the
// consumers alone.
template <int TWL, bool PRO, int BN, bool DMA = false>
__global__ __launch_bounds__(512, 2) void conv3x3_pipe_kernel(const ConvArgs a) {
  using T = bf16_t;
  using E = ET<T>;
  static_assert(!DMA || !PRO, "the LDS-DMA form serves the layers without a prologue");
  // workgroup tile 256 px x 128 ch (consumers 2 x 2) or, for 64-channel layers, 512 px x 64 ch (consumers 4 x 1):
  // the same bytes per step and the same 128 x 64 consumer tile either way
  static_assert(BN == 128 || BN == 64, "channel tile is 128 or 64");
  using L = PipeLayout<TWL, BN, DMA>;              // patch pixels at PPIX, weight rows at WPIX bytes; NPT: producer threads
  constexpr int PPIX = L::PPIX, WPIX = L::WPIX, BM = L::BM, NTHR = L::NTHR, NPT = L::NPT;
  constexpr int WN = BN / 64, WM = 4 / WN;                   // consumer waves: WM x WN, 128 px x 64 ch each
  constexpr int TW = L::TW, TH = L::TH, PW = L::PW, PH = L::PH, RPX = L::RPX, ROWP = L::ROWP, PB = L::PB, WB = L::WB;
  constexpr int NP = L::NP, NPL = (NP + NPT - 1) / NPT;
  constexpr int NWL = 3 * BN * 4 / NPT;            // 16-byte weight pieces per producer thread and step
  constexpr int POFF = L::POFF, W2OFF = L::W2OFF, MAINB = L::MAINB;
  static_assert(3 * BN * 4 % NPT == 0, "weight pieces divide evenly");
  auto wring = [](int r) { return r < 2 ? r * WB : W2OFF; };

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W;

  // ---- work units: every XCD owns a contiguous range, walked by its workgroups with stride GW
  const int NT = a.Ntot / BN;
  const int tpi = a.tiles_x * a.tiles_y;
  const UnitWalk uw = unit_walk(a.B * tpi * NT);
  const int GW = uw.GW, u_end = uw.u_end;
  int u = uw.u;
  if (u >= u_end) return;
  const int nchA = a.CA / E::CH;
  const int nchunks = (a.CA + a.CB) / E::CH;       // >= 2 (checked by the launcher)
  const int nsteps = nchunks * 3;
  auto decode = [&](int uu, int& mt, int& b, int& y0, int& x0, int& n0) { decode_unit<TW, TH, BN>(a, NT, tpi, uu, mt, b, y0, x0, n0); };
  int ub, uy0, ux0, un0, umt;
  decode(u, umt, ub, uy0, ux0, un0);
#ifdef SEGK_PIPE_STAMPS
  unsigned long long stamp_sum[6] = {0, 0, 0, 0, 0, 0}, stamp_last;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_last)::"memory");
  const unsigned long long stamp_t0 = stamp_last;
#endif

  // ---- the part of the epilogue all 512 threads run: BN-statistics reduction over the consumer rows and
  // the 16-byte coalesced NHWC stores of the staged tile
  constexpr int OP = L::OP;
  constexpr int LDSEND = MAINB;                    // DMA: one trash KiB behind the ring (no epilogue tile), then the
  constexpr int STOFF = L::STOFF;                  // statistics exchange: [WM][WN][64 ch][2] floats + one flag per consumer wave
  char* const ot = smem + POFF;
  float* const red = (float*)(ot + L::RED);
  auto store_tile = [&](auto FULLc) {
#ifndef SEGK_PIPE_STAMPS
    reduce_stat_rows<WM, BN>(a, red, tid, umt, un0);
#endif
    store_staged_tile<T, TWL, BM, BN, NTHR, decltype(FULLc)::value, false>(a, ot, tid, ub, uy0, ux0, un0);
  };

  if constexpr (DMA) {
  if (wave >= 4) {
    // =========================================== PRODUCERS (LDS-DMA) ===========================================
    const int pw = wave - 4;                          // producer wave: pieces pw, pw + 4, ...
    constexpr int NPIECE = PH * RPX / 16;             // patch pieces (16 pixel slots = 1 KiB) per chunk
    static_assert(PH * RPX % 16 == 0, "whole pieces");
    constexpr int NPL = (NPIECE + 3) / 4;             // per wave (a wave without a last piece issues it into the trash KiB)
    constexpr int NPL0 = (NPL + 1) / 2;               // issued in the chunk's first step; the rest in its second
    constexpr int G16 = BN / 16;                      // 16-row weight groups per tap
    constexpr int NWL = 3 * G16 / 4;                  // weight pieces per wave and step (6 or 3)
    static_assert(3 * G16 % 4 == 0, "weight pieces divide evenly");
    // lane -> (pixel of the 16-slot piece, 16-byte piece q) by inverting the slot map; -> weight row / piece of a 16-row group
    int pq, p16;
    dma_slot_lane(lane, pq, p16);
    const unsigned wl_off = (unsigned)((lane >> 2) * 64 + (((lane & 3) ^ wswz(lane >> 2)) << 4));
    const char* const zp = (const char*)g_conv_zero_page + (lane & 15) * 16;
    int prel[NPL];                                    // (patch row << 8) | patch column of the lane's pixel; row 32767: never valid
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int j = pw + 4 * i;
      const int slot = 16 * j + p16;                  // pixel slot of the chunk's image: RPX per patch row
      const int py = slot / RPX, px = slot - py * RPX;
      prel[i] = (j < NPIECE && px < PW) ? ((py << 8) | px) : PREL_NEVER;
    }
    unsigned pvalid = 0;
    int plin[NPL];
    auto patch_unit = [&](int b, int y0, int x0) {
      pvalid = 0;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const int gy = y0 + (prel[i] >> 8) - 1, gx = x0 + (prel[i] & 255) - 1;
        const bool ok = (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W);
        plin[i] = ok ? (b * H + gy) * W + gx : 0;
        pvalid |= (ok ? 1u : 0u) << i;
      }
    };
    // pieces [I0, I1) of chunk kc into patch buffer `buf`
    auto issue_p = [&](int kc, int buf, auto I0c, auto I1c) {
      constexpr int I0 = decltype(I0c)::value, I1 = decltype(I1c)::value;
      const T* base;
      int C;
      if (kc < nchA) { base = (const T*)a.srcA + kc * E::CH; C = a.CA; }
      else { base = (const T*)a.srcB + (kc - nchA) * E::CH; C = a.CB; }
      const char* const cb = (const char*)(base + pq * E::VEC);
      const unsigned cbytes = (unsigned)C * 2u;
#pragma unroll
      for (int i = I0; i < I1; ++i) {
        const int j = pw + 4 * i;                       // wave-uniform
        char* const dst = smem + ((j < NPIECE) ? POFF + buf * PB + j * 1024 : LDSEND);
        const char* const src = ((pvalid >> i) & 1) ? cb + (size_t)((unsigned)plin[i] * cbytes) : zp;
        __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)dst, 16, 0, 0);
      }
    };
    // weight step `step` of the unit whose channel tile starts at n0 -> ring slot
    auto issue_w = [&](int n0, int step, int ring) {
      const char* const wb = (const char*)a.w + ((size_t)(step * 3) * a.Ntot + n0) * 64 + wl_off;
      char* const dst = smem + wring(ring);
#pragma unroll
      for (int i = 0; i < NWL; ++i) {
        const int j = pw + 4 * i, t = j / G16, g = j - t * G16;
        __builtin_amdgcn_global_load_lds((glb_vp)(wb + ((size_t)t * a.Ntot * 64 + g * 1024)), (lds_vp)(dst + j * 1024), 16, 0, 0);
      }
    };
    using I_0 = std::integral_constant<int, 0>;
    using I_H = std::integral_constant<int, NPL0>;
    using I_N = std::integral_constant<int, NPL>;

    issue_w(un0, 0, 0);
    issue_w(un0, 1, 1);
    patch_unit(ub, uy0, ux0);
    issue_p(0, 0, I_0{}, I_N{});
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                   // B0
    PIPE_STAMP(5);
    for (;;) {
      const int un = u + GW;
      const bool has_next = un < u_end;
      int nmt = 0, nb = 0, ny0 = 0, nx0 = 0, nn0 = 0;
      if (has_next) decode(un, nmt, nb, ny0, nx0, nn0);
      for (int kc = 0; kc < nchunks; ++kc) {
        const int s0 = 3 * kc;
        const bool last = (kc + 1 == nchunks);
        // ---- step TG0: weights of step s0 + 2 (slot 2); first half of the next chunk's patch (the next unit's chunk 0 into
        // P0 behind the last chunk: nchunks is even, so the last chunk lives in P1)
        issue_w(un0, s0 + 2, 2);
        if (!last) {
          issue_p(kc + 1, (kc + 1) & 1, I_0{}, I_H{});
          PIPE_STAMP(0);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPL0) : "memory");     // the weights (older) have landed
        } else if (has_next) {
          patch_unit(nb, ny0, nx0);
          issue_p(0, 0, I_0{}, I_H{});
          PIPE_STAMP(0);
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPL0) : "memory");
        } else {
          PIPE_STAMP(0);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PIPE_STAMP(2);
        // raw s_barrier: __syncthreads() carries a fence that hipcc lowers to s_waitcnt vmcnt(0) -- it would drain the patch
        // pieces this step leaves in flight.  The DMA data a barrier publishes is covered by the counted wait above it.
        __builtin_amdgcn_s_barrier();
        PIPE_STAMP(1);
        // ---- step TG1: weights of step s0 + 3 (slot 0: the next chunk's or the next unit's first step); rest of the patch
        if (!last) issue_w(un0, s0 + 3, 0);
        else if (has_next) issue_w(nn0, 0, 0);
        if (!last) issue_p(kc + 1, (kc + 1) & 1, I_H{}, I_N{});
        else if (has_next) issue_p(0, 0, I_H{}, I_N{});
        PIPE_STAMP(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PIPE_STAMP(2);
        __builtin_amdgcn_s_barrier();
        PIPE_STAMP(1);
        // ---- step TG2: weights of step s0 + 4 (slot 1)
        if (!last) issue_w(un0, s0 + 4, 1);
        else if (has_next) issue_w(nn0, 1, 1);
        PIPE_STAMP(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PIPE_STAMP(2);
        __builtin_amdgcn_s_barrier();
        PIPE_STAMP(1);
      }
      // no boundary: the consumers store their results from registers, and the ring slots the next unit's first steps write
      // were released by the step barriers above
      if (!has_next) break;
      u = un; umt = nmt; ub = nb; uy0 = ny0; ux0 = nx0; un0 = nn0;
    }
    PIPE_STAMP_OUT();
    return;
  }
  } else {
  if (wave >= 4) {
    // =========================================== PRODUCERS ===========================================
    // wave priorities stay at their default: raising the producers (s_setprio 3) or the consumers (2) was measured
    // 3-5 % slower than leaving the oldest-first arbitration alone (512->512: 132 / 132 / 128 us)
    const int ptid = tid - NPT;
    const int trash = MAINB + ptid * 16;
    const int pc = ptid & 3;        // 16-byte slot inside the 64-byte chunk (NPT % 4 == 0: same for every piece)
    int plds[NPL], prel[NPL];
    unsigned pint = 0;              // bit i: piece i is an interior (non-halo) pixel of the tile
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int q = ptid + i * NPT;
      int py, px;
      prel[i] = patch_piece<L>(q, py, px);
      plds[i] = (q < NP) ? POFF + py * ROWP + px * PPIX + pc * 16 : trash;
      pint |= (patch_interior<L>(q, py, px) ? 1u : 0u) << i;
    }
    unsigned wsrc[NWL];
    int wlds[NWL];
#pragma unroll
    for (int i = 0; i < NWL; ++i) {
      const int q = ptid + i * NPT;
      const int t = q / (BN * 4), r = q - t * (BN * 4);
      wsrc[i] = t * a.Ntot * 64 + r * 16;              // byte offset from the step's weight base
      const int wrow = r >> 2, wpc = (r & 3) ^ wswz(wrow);
      wlds[i] = t * (BN * WPIX) + wrow * WPIX + wpc * 16;
    }

    // ---- patch: per-unit pixel indices and validity, per-chunk source; one register set
    u32x4 preg[NPL];
    unsigned pvalid = 0;
    int plin[NPL];
    float psc[E::VEC], psh[E::VEC];
    int pl_aoff = -1;               // channel offset of the fetched chunk inside act_out (or -1)
    bool pl_first = false;          // the fetched patch belongs to a unit of channel tile 0 (writes act_out)
    auto patch_unit = [&](int b, int y0, int x0, int n0) {
      pl_first = (n0 == 0);
      pvalid = 0;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const PatchPixel px = patch_pixel<1>(prel[i], y0, x0, H, W);
        plin[i] = (b * H + px.cy) * W + px.cx;
        pvalid |= (px.ok ? 1u : 0u) << i;
      }
    };
    auto patch_load = [&](int kc) {
      const T* base;
      int C, coff;
      if (kc < nchA) { base = (const T*)a.srcA; C = a.CA; coff = kc * E::CH; }
      else { base = (const T*)a.srcB; C = a.CB; coff = (kc - nchA) * E::CH; }
      base += coff + pc * E::VEC;
      pl_aoff = (kc < nchA) ? coff + pc * E::VEC : -1;      // act_out mirrors srcA only
#pragma unroll
      for (int i = 0; i < NPL; ++i) preg[i] = *(const u32x4*)(base + (size_t)(unsigned)(plin[i] * C));
      if (PRO) {
#pragma unroll
        for (int j = 0; j < E::VEC; ++j) {
          psc[j] = a.scale[coff + pc * E::VEC + j];
          psh[j] = a.shift[coff + pc * E::VEC + j];
        }
      }
    };
    auto patch_store = [&](int pboff) {
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const bool ok = (pvalid >> i) & 1;
        const u32x4 v = patch_transform<T, PRO>(preg[i], psc, psh, ok);
        const int off = (plds[i] < MAINB) ? plds[i] + pboff : trash;
        *(u32x4*)(smem + off) = v;
        if (PRO) {   // side output: the transformed activation itself, interior pixels, once per pixel and chunk
          if (a.act_out && pl_first && pl_aoff >= 0 && ok && ((pint >> i) & 1))
            *(u32x4*)((T*)a.act_out + (size_t)(unsigned)(plin[i] * a.CA) + pl_aoff) = v;
        }
      }
    };

    // ---- weights: step x lives in register set x % 3 from its fetch (during step x-4) to its store
    // (during step x-2) and in ring slot x % 3 from then until step x has been computed
    u32x4 wreg[3][NWL];
    int cu_step = 0, cu_n0 = un0;   // fetch cursor: the next weight step to fetch, (unit, step) walking ahead
    bool cu_ok = true;              // false past the last unit
    int nn0 = 0;                    // channel origin of the next unit (set per unit below)
    bool has_next = false;
    auto fetch_w = [&](u32x4 (&R)[NWL]) {
      if (cu_ok) {
        const char* wb = (const char*)a.w + ((size_t)(cu_step * 3) * a.Ntot + cu_n0) * 64;
#pragma unroll
        for (int i = 0; i < NWL; ++i) R[i] = *(const u32x4*)(wb + wsrc[i]);
        if (++cu_step == nsteps) { cu_step = 0; cu_n0 = nn0; cu_ok = has_next; }
      }
    };
    auto store_w = [&](int ring, const u32x4 (&R)[NWL]) {
#pragma unroll
      for (int i = 0; i < NWL; ++i) *(u32x4*)(smem + wring(ring) + wlds[i]) = R[i];
    };

    // first unit: weight steps 0, 1 and patch chunk 0 into LDS; steps 2, 3 and patch chunk 1 in registers
    {
      const int un = u + GW;
      has_next = un < u_end;
      int t0, t1, t2, t3;
      if (has_next) decode(un, t0, t1, t2, t3, nn0);
    }
    patch_unit(ub, uy0, ux0, un0);
    patch_load(0);
    fetch_w(wreg[0]);
    fetch_w(wreg[1]);
    store_w(0, wreg[0]);
    store_w(1, wreg[1]);
    patch_store(0);
    fetch_w(wreg[2]);
    fetch_w(wreg[0]);
    patch_load(1);
    __syncthreads();                                   // B0
    PIPE_STAMP(5);
    for (;;) {
      const int un = u + GW;
      has_next = un < u_end;
      int nmt = 0, nb = 0, ny0 = 0, nx0 = 0;
      if (has_next) decode(un, nmt, nb, ny0, nx0, nn0);
      for (int kc = 0; kc < nchunks; ++kc) {
        // step TG0: ring slot 2 <- weights of step s+2; fetch step s+4
        store_w(2, wreg[2]);
        fetch_w(wreg[1]);
        PIPE_STAMP(0);
        __syncthreads();
        PIPE_STAMP(1);
        // step TG1: the next chunk's patch, ring slot 0
        if (kc + 1 < nchunks) patch_store(((kc + 1) & 1) * PB);
        store_w(0, wreg[0]);
        fetch_w(wreg[2]);
        PIPE_STAMP(0);
        __syncthreads();
        PIPE_STAMP(1);
        // step TG2: ring slot 1; fetch the patch two chunks ahead (the next unit's chunk 0 from the
        // second-to-last chunk; the last chunk fetches nothing: its registers are stored after the epilogue)
        store_w(1, wreg[1]);
        fetch_w(wreg[0]);
        if (kc + 2 < nchunks) patch_load(kc + 2);
        else if (kc + 2 == nchunks && has_next) { patch_unit(nb, ny0, nx0, nn0); patch_load(0); }
        PIPE_STAMP(0);
        __syncthreads();
        PIPE_STAMP(1);
      }
      __syncthreads();                                 // E1: the consumers have staged the output tile
      PIPE_STAMP(2);
      if ((uy0 + TH <= H) && (ux0 + TW <= W)) store_tile(std::true_type{});
      else store_tile(std::false_type{});
      PIPE_STAMP(3);
      if (!has_next) break;
      __syncthreads();                                 // E2: tile consumed, [P0 | P1 | W2] may be rewritten
      patch_store(0);                                  // next unit's chunk 0
      patch_load(1);                                   // and its chunk 1, stored during its step 1
      u = un; umt = nmt; ub = nb; uy0 = ny0; ux0 = nx0; un0 = nn0;
      __syncthreads();                                 // E3
      PIPE_STAMP(4);
    }
    PIPE_STAMP_OUT();
    return;
  }
  }

  // ============================================= CONSUMERS =============================================
  // the 128 x 64 wave tile is 8 x 4 blocks of 16 x 16; per tap (k = 32 = one whole chunk) 8 patch and 4 weight fragments
  // feed 32 MFMAs.  Sub-step = one tap x one half of the pixel blocks (4 A + 4 B -> 16 MFMAs, 256 matrix cycles); fragments
  // are read one sub-step ahead, the weight fragments of a tap once per two.
  const int wm = wave / WN, wn = wave - wm * WN;
  const int lc = lane & 15, lq = lane >> 4;
  constexpr int MB = 8, NB = 4;
  int laneA[DMA ? 3 : MB], laneB[NB];
  if constexpr (DMA) {
    // one address per tap column t: pixel x = (block start: 0 or 16) + t + lc of the wave's first tile row; pixel block mb
    // adds the immediate mboff(mb)
#pragma unroll
    for (int t = 0; t < 3; ++t)
      laneA[t] = POFF + ((wm * MB * 16) >> TWL) * ROWP + dma_slot(t + lc, lq);
  } else {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = (wm * MB + mb) * 16 + lc;
      laneA[mb] = POFF + (m >> TWL) * ROWP + (m & (TW - 1)) * PPIX + lq * 16;
    }
  }
  // byte address of the lane's 16 bytes of pixel block mb at tap column t, relative to the patch row base `prow`
  auto pa = [&](int prow, int mb, int t) -> const char* {
    if constexpr (DMA) return smem + prow + laneA[t] + (((mb * 16) >> TWL) * ROWP + (((mb * 16) & (TW - 1)) >> 3) * 512);
    else return smem + prow + laneA[mb] + t * PPIX;
  };
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    // DMA form: the lane's row of block nb is channel 8 (lc >> 2) + 4 (nb & 1) + (lc & 3) of the block pair's 32
    const int row = DMA ? (wn * NB + (nb & ~1)) * 16 + 8 * (lc >> 2) + 4 * (nb & 1) + (lc & 3) : (wn * NB + nb) * 16 + lc;
    laneB[nb] = row * WPIX + ((lq ^ wswz(row)) << 4);
  }

  f32x4 acc[MB][NB];
  auto zero_acc = [&]() {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  uint4 fa[2][4], fb[3][NB];    // patch halves ping-pong per sub-step; weight fragments per tap ([0] primed before a step)
  auto rdA = [&](int prow, int t, int hh, uint4 (&A)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) A[j] = *(const uint4*)pa(prow, 4 * hh + j, t);
  };
  auto rdB = [&](int wb, int t, uint4 (&Bf)[NB]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) Bf[nb] = *(const uint4*)(smem + wb + laneB[nb] + t * (BN * WPIX));
  };
  // staged form: pixels x channels (A = patch); DMA form: channels x pixels (A = weights), see the epilogue
  auto mma16 = [&](const uint4& pfrag, const uint4& wfrag, const f32x4& c) {
    if constexpr (DMA) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wfrag), __builtin_bit_cast(bf16x8, pfrag), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, pfrag), __builtin_bit_cast(bf16x8, wfrag), c, 0, 0, 0);
  };
  auto step = [&](auto TGc, int kc) {
    constexpr int TG = decltype(TGc)::value;
    const int prow = (kc & 1) * PB + TG * ROWP;
    const int prow_next = (TG < 2) ? prow + ROWP : ((kc + 1) & 1) * PB;
    constexpr int wb = TG < 2 ? TG * WB : W2OFF, wb_next = (TG + 1) % 3 < 2 ? ((TG + 1) % 3) * WB : W2OFF;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int t = i >> 1, hh = i & 1;
      // the next sub-step's fragments are read BETWEEN this sub-step's MFMAs, one ds_read_b128 behind every second MFMA
      // (weight fragments of a new tap first: the next sub-step's first MFMAs need all four).  A consumer is alone on its
      // SIMD's matrix pipe: while it issues a group of 4-8 reads back to back the pipe runs dry (tools/ubench/pipe_roles.hip:
      // 1968 -> 1652 cycles per 1536-cycle step in the bare loop, 2006 -> 1806 beside staging partners).
      const int ni = (i + 1) % 6, nt_ = ni >> 1, nh = ni & 1;
      const int rp = (i + 1 < 6) ? prow : prow_next;
      const int rw = (i + 1 < 6) ? wb : wb_next;
      const bool needB = (nh == 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          acc[4 * hh + j][nb] = mma16(fa[i & 1][j], fb[t][nb], acc[4 * hh + j][nb]);
          const int m = j * NB + nb;
          if (m & 1) {
            const int r = m >> 1;   // 0 .. 7
            if (needB) {
              if (r < 4) fb[nt_][r] = *(const uint4*)(smem + rw + laneB[r] + nt_ * (BN * WPIX));
              else fa[(i + 1) & 1][r - 4] = *(const uint4*)pa(rp, 4 * nh + r - 4, nt_);
            } else if (r < 4) {
              fa[(i + 1) & 1][r] = *(const uint4*)pa(rp, 4 * nh + r, nt_);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
    }
    // rdA / rdB are captured only to keep this closure's layout, which steers the register assignment of the instances as
    // measured; drop these two lines with the next change to the step.
    (void)rdA;
    (void)rdB;
  };
  auto stage_tile = [&](auto FULLc) {   // bias, BN partial sums from the fp32 accumulators, tile -> LDS
    constexpr bool full = decltype(FULLc)::value;      // compile time: a run-time test here is a branch per value
    const bool do_stats = (a.stats != nullptr);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n = (wn * NB + nb) * 16 + lc;
      const float bv = a.bias ? a.bias[un0 + n] : 0.f;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int m0 = (wm * MB + mb) * 16 + 4 * lq;        // the lane holds pixels m0 .. m0 + 3 of channel n
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = acc[mb][nb][j] + bv;
          if (!full) {   // rare: pixels past the image edge must not enter the statistics (they are never stored)
            const int m = m0 + j;
            v[j] = ((uy0 + (m >> TWL) < H) && (ux0 + (m & (TW - 1)) < W)) ? v[j] : 0.f;
          }
          s1 += v[j];
          s2 = fmaf(v[j], v[j], s2);
        }
        char* const ob = ot + m0 * OP + n * E::ES;
        uint32_t p01, p23;
        p01 = cvt_pk_bf16(v[0], v[1]);
        p23 = cvt_pk_bf16(v[2], v[3]);
        *(uint16_t*)(ob) = (uint16_t)(p01 & 0xffffu);
        *(uint16_t*)(ob + OP) = (uint16_t)(p01 >> 16);
        *(uint16_t*)(ob + 2 * OP) = (uint16_t)(p23 & 0xffffu);
        *(uint16_t*)(ob + 3 * OP) = (uint16_t)(p23 >> 16);
      }
      if (do_stats) {
        s1 += __shfl_xor(s1, 16);
        s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (lq == 0) {
          red[(wm * BN + n) * 2 + 0] = s1;
          red[(wm * BN + n) * 2 + 1] = s2;
        }
      }
    }
  };

  int stat_seq = 0;                                          // DMA form: units this wave has written statistics for
  if constexpr (DMA) {
    if (lane == 0) ((volatile int*)(smem + STOFF + WM * WN * 64 * 8))[wave] = 0;   // flags (consumer waves = wm * WN + wn), before B0
  }
  // DMA form: the unit's results straight from the accumulators.  acc[mb][2k][j] / acc[mb][2k + 1][j] are channels
  // 32 k + 8 lq + j / + 4 + j (of the wave's 64) of pixel 16 mb + lc (of the wave's 128): 8 consecutive channels = one 16-byte
  // store per pixel block and channel group, 64 contiguous bytes per pixel from the four lq lanes.  Both groups of a pixel block
  // are stored BACK TO BACK, so the two 64-byte halves of a pixel's 128-byte line reach L2 within one store pair: with the
  // groups eight stores apart (the first form) the HBM write traffic of these launches was 20-36 % above the output size
  // (half-written lines leaving L2 twice: 183 -> 138 MB at 128->128@128, profiles/r04_pmc_conv_layers.txt).  No bias here --
  // every conv in front of a BatchNorm and every data gradient; a biased conv takes the staged form (launch_pipe): sixteen bias
  // registers beside both groups' statistics spill.
  auto direct_out = [&](auto FULLc) {
    constexpr bool full = decltype(FULLc)::value;
    static_assert(!DMA || NB == 4, "two 32-channel groups per consumer wave");
    const bool do_stats = (a.stats != nullptr);
    const int m0 = wm * MB * 16 + lc;                        // the lane's pixel of block 0
    const int ty0 = m0 >> TWL, tx0 = m0 & (TW - 1);
    const size_t pix0 = ((size_t)(ub * H + uy0 + ty0)) * W + ux0 + tx0;
    T* dpx[2];
    int pstr[2];
    float s1[2][8], s2[2][8];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int nbase = un0 + wn * 64 + 32 * k;              // wave-uniform; a 32-channel group never straddles CO1
      T* dch;
      if (nbase < a.CO1) { dch = (T*)a.out + nbase + 8 * lq; pstr[k] = a.CO1; }
      else { dch = (T*)a.out2 + (nbase - a.CO1) + 8 * lq; pstr[k] = a.CO2; }
      dpx[k] = dch + pix0 * pstr[k];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[k][e] = 0.f; s2[k][e] = 0.f; }
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int dty = (mb * 16) >> TWL, dtx = (mb * 16) & (TW - 1);     // compile-time per mb
      // rare (!full): pixels past the image edge are neither stored nor counted
      const bool in = full || ((uy0 + ty0 + dty < H) && (ux0 + tx0 + dtx < W));
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = acc[mb][2 * k + (e >> 2)][e & 3];
          if (!full) v[e] = in ? v[e] : 0.f;
          s1[k][e] += v[e];
          s2[k][e] = fmaf(v[e], v[e], s2[k][e]);
        }
        const uint4 o = make_uint4(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7]));
        if (in) *(uint4*)(dpx[k] + (size_t)(dty * W + dtx) * pstr[k]) = o;
      }
    }
    if (do_stats) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[k][e] = row16_sum(s1[k][e]); s2[k][e] = row16_sum(s2[k][e]); }
        if (lc == 0) {   // the wave's sums over its 128 pixels -> its slot of the exchange area
          float4* const dst = (float4*)(smem + STOFF) + ((wm * WN + wn) * 64 + 32 * k + 8 * lq) / 2;
#pragma unroll
          for (int e = 0; e < 8; e += 2) dst[e / 2] = make_float4(s1[k][e], s2[k][e], s1[k][e + 1], s2[k][e + 1]);
        }
      }
    }
    if (do_stats) {
      // ONE statistics row per unit: the consumer waves of a channel half (same wn, WM pixel parts) meet in LDS -- parts 1 ..
      // WM - 1 publish (data, then a sequence flag), part 0 waits for their flags and adds the WM values per channel in part
      // order (bit-stable) -- 512 contiguous bytes per wave instead of WM rows for segk_bn_finalize to walk (a first form with
      // WM rows per unit made the BatchNorm finalize launches 0.17 -> 0.28 ms per step).  No wave waits on a wave that waits:
      // the publishers never wait, and every wave passes at least one workgroup barrier between two units, so a slot is
      // consumed long before it is rewritten.
      volatile int* const flags = (volatile int*)(smem + STOFF + WM * WN * 64 * 8);
      ++stat_seq;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // the slot is written
      if (wm > 0) {
        if (lane == 0) flags[wm * WN + wn] = stat_seq;
      } else {
#pragma unroll
        for (int w = 1; w < WM; ++w)
          while (flags[w * WN + wn] != stat_seq) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");                           // the slots are read after the flags, not before
        const float2* const src = (const float2*)(smem + STOFF) + wn * 64 + lane;
        float2 t = src[0];
#pragma unroll
        for (int w = 1; w < WM; ++w) {
          const float2 q = src[w * WN * 64];
          t.x += q.x;
          t.y += q.y;
        }
        ((float2*)a.stats)[(size_t)umt * a.Ntot + un0 + wn * 64 + lane] = t;
      }
    }
  };

  zero_acc();
  __syncthreads();                                     // B0
  PIPE_STAMP(5);
  rdA(0, 0, 0, fa[0]);
  rdB(0, 0, fb[0]);
  for (;;) {
    const int un = u + GW;
    const bool has_next = un < u_end;
    int nmt = 0, nb = 0, ny0 = 0, nx0 = 0, nn0 = 0;
    if (has_next) decode(un, nmt, nb, ny0, nx0, nn0);
    // step barriers: __syncthreads() drains the consumers' LDS reads (s_waitcnt lgkmcnt(0)) before the barrier, so the producers
    // may overwrite the slot it releases by DMA right after it.  A raw s_barrier would be valid only if every read of that slot
    // had already been consumed by an MFMA.
    for (int kc = 0; kc < nchunks; ++kc) {
      step(std::integral_constant<int, 0>{}, kc);
      PIPE_STAMP(0);
      __syncthreads();
      PIPE_STAMP(1);
      step(std::integral_constant<int, 1>{}, kc);
      PIPE_STAMP(0);
      __syncthreads();
      PIPE_STAMP(1);
      step(std::integral_constant<int, 2>{}, kc);
      PIPE_STAMP(0);
      __syncthreads();
      PIPE_STAMP(1);
    }
    const bool full = (uy0 + TH <= H) && (ux0 + TW <= W);
    if constexpr (DMA) {
      if (full) direct_out(std::true_type{});
      else direct_out(std::false_type{});
      PIPE_STAMP(2);
      if (!has_next) break;
      zero_acc();
      u = un; umt = nmt; ub = nb; uy0 = ny0; ux0 = nx0; un0 = nn0;
      rdA(0, 0, 0, fa[0]);                             // (P0 / W0 of the next unit landed under this unit's last steps)
      rdB(0, 0, fb[0]);
      PIPE_STAMP(4);
      continue;
    }
    if (full) stage_tile(std::true_type{});
    else stage_tile(std::false_type{});
    PIPE_STAMP(2);
    __syncthreads();                                   // E1
    if (full) store_tile(std::true_type{});
    else store_tile(std::false_type{});
    PIPE_STAMP(3);
    if (!has_next) break;
    zero_acc();
    __syncthreads();                                   // E2
    u = un; umt = nmt; ub = nb; uy0 = ny0; ux0 = nx0; un0 = nn0;
    __syncthreads();                                   // E3: the next unit's chunk 0 is in P0
    PIPE_STAMP(4);
    rdA(0, 0, 0, fa[0]);
    rdB(0, 0, fb[0]);
  }
  PIPE_STAMP_OUT();
}

template <int TWL, bool PRO, int BN, bool DMA>
int launch_pipe_m(ConvArgs a, const ConvPlan& p, hipStream_t st) {
  using L = PipeLayout<TWL, BN, DMA>;
  static_assert(L::LDS <= 160 * 1024, "conv3x3_pipe: LDS exceeds 160 KiB");
  SEGK_REQUIRE_PLAN_TILE("conv3x3_pipe", p, L::BM, TWL);
  const int gw = conv_unit_grid(conv_set_tiles<L>(a, TWL) * (a.Ntot / BN), 1);      // one 8-wave workgroup per CU
  return segk_launch_lds<conv3x3_pipe_kernel<TWL, PRO, BN, DMA>>("conv3x3_pipe", 160 * 1024, dim3(8 * gw), dim3(L::NTHR), L::LDS, st, a);
}

template <int TWL, bool PRO, int BN>
int launch_pipe(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
  if constexpr (!PRO) {
    // LDS-DMA producers (round 4): layers without a BatchNorm prologue and without a bias (the register epilogue carries none)
    // whose chunk count is even (the patch ring's parity across the unit boundary) and whose sources stay below 4 GiB (32-bit
    // byte offsets per DMA lane)
    const int nchunks = (a.CA + a.CB) / 32;
    const long long px = (long long)a.B * a.H * a.W;
    int cmax = a.CA > a.CB ? a.CA : a.CB;
    cmax = cmax > a.CO1 ? cmax : a.CO1;
    cmax = cmax > a.CO2 ? cmax : a.CO2;
    if (nchunks % 2 == 0 && px * cmax * 2 < 4294967296LL && a.bias == nullptr) return launch_pipe_m<TWL, PRO, BN, true>(a, p, st);
  }
  return launch_pipe_m<TWL, PRO, BN, false>(a, p, st);
}

}  // namespace

int segk_conv_pipe_launch(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
  auto by_bn = [&](auto TWLc, auto PROc) {
    constexpr int TWL = decltype(TWLc)::value;
    constexpr bool PRO = decltype(PROc)::value;
    return p.bn == 128 ? launch_pipe<TWL, PRO, 128>(a, p, st) : launch_pipe<TWL, PRO, 64>(a, p, st);
  };
  auto by_pro = [&](auto TWLc) { return a.scale ? by_bn(TWLc, std::true_type{}) : by_bn(TWLc, std::false_type{}); };
  return p.twl == 5 ? by_pro(std::integral_constant<int, 5>{}) : by_pro(std::integral_constant<int, 4>{});
}
