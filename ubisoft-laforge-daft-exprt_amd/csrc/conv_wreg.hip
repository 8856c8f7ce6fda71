// conv_wreg_kernel: the conv GEMM with the weights held in registers (K = taps * 128 <= 384), and its launcher.
#include "conv_args.h"

namespace {

#include "conv_common.h"

// ---- weight-stationary variant for short contractions (Cin = 128, Cout a multiple of 256: the FF block's 128 -> 1024
// conv and the data gradient of its 1024 -> 128 partner).  With K = taps * Cin <= 384 the tiled kernel (conv_gemm_kernel.h) spends a
// workgroup's life waiting: 4 K-chunks of 0.3 us of MFMA work, each behind a ~1.5 us global -> LDS round trip, plus a
// prologue and an epilogue (measured 26 % MFMA utilisation at 3 workgroups / CU).  Here a 512-thread workgroup owns 256
// output channels for its lifetime: wave w keeps the weights of channels [32w, 32w + 32) for the WHOLE contraction in
// registers as ready-made MFMA B fragments (taps * 8 k-steps * 4 VGPRs = 96), so the weights are read once per
// workgroup instead of once per position tile and never touch LDS.  128-position tiles of the input stream past:
// the A tile (130 x 128) is double-buffered in LDS, fetched into registers one tile ahead, and shared by the 8 waves;
// per k-step a wave reads 4 A fragments for 4 MFMAs (128 rows x 32 channels).  One barrier per tile.  The epilogue is
// wave-private and register-only: the MFMA operands are swapped (D[co][pos]) so that a lane ends up with 8 consecutive
// channels of one position after four v_permlane32_swap, bias / ReLU / gate are applied in that layout and the block
// leaves through 16-byte buffer stores (out-of-range rows dropped by the descriptor), issued in slices between the
// MFMAs of the next tile, so no wave waits for another between tiles.  The live position tiles of the batch
// (skip_lengths) are split evenly over the workgroups of a channel block; dead tiles are zero-filled in a second pass.
constexpr int WR_THREADS = 512, WR_BN = 256, WR_BM = 128;
// BITS (bf16 output only): the ReLU of the FF block's first conv also leaves ONE BIT per output element -- a 32-bit word per
// (position, 32-channel block of a wave), bit layout = the wave's own post-swap register order -- and the data gradient of the second
// conv gates with that word instead of re-reading the 2 KB activation row: 128 B instead of 2 KB per row of gate traffic.
template <typename TO, typename TG, int TAPS, bool RELU, bool GATE, bool BITS = false>
__global__ __launch_bounds__(WR_THREADS, 2) void conv_wreg_kernel(ConvArgs p, int ngrp) {
  typedef bf16_t TC;
  constexpr int BM = WR_BM, HALO = TAPS / 2, AROWS = BM + TAPS - 1, CIN = 128, LDK = CIN + Pad<TC>::value, KCH = CIN / 8;
  constexpr int KSTEPS = CIN / 16;
  constexpr int A_CH = AROWS * KCH, A_PT = (A_CH + WR_THREADS - 1) / WR_THREADS;
  constexpr int A_BYTES = AROWS * LDK * (int)sizeof(TC);
  typedef typename Vec8<TC>::type frag_t;
  __shared__ __attribute__((aligned(16))) char smem[2 * A_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, g = lane >> 5;
  const int ztiles = p.Cout / WR_BN, ptiles = dx_cdiv(p.N, BM);
  // workgroup -> (position group, channel slice), slice-major: the ztiles workgroups of one position group sit 64 indices apart = on
  // the SAME XCD (round-robin dispatch, ngrp % 8 == 0) and read their common activation tiles through one L2
  const bool zmajor = ngrp % 8 == 0;
  const int grp = zmajor ? (int)blockIdx.x % ngrp : (int)blockIdx.x / ztiles, zt = zmajor ? (int)blockIdx.x / ngrp : (int)blockIdx.x % ztiles;
  const int co0 = zt * WR_BN + wave * 32;
  const int N = p.N, Cout = p.Cout;
  const TC* W = reinterpret_cast<const TC*>(p.w);
  TO* Y = reinterpret_cast<TO*>(p.y);
  const TG* G = reinterpret_cast<const TG*>(p.gate);

  // ---- this wave's weights, once: B fragment of k-step (tap, ks) = W[tap][co0 + l31][16 ks + 8 g .. + 8]
  // Read straight from global memory a fragment load touches 32 rows x 2 x 16 bytes -- 64 sectors for 1 KB -- and the prologue
  // took 9.3 us of a 43 us launch (s_memrealtime stamps per workgroup, tools/wreg_timing.py): five dependent global round trips
  // (three taps of weights, bias, the first A tile) behind the kernel-argument load.  Now the workgroup's slice of each tap,
  // W[tap][256 channels][128] = 64 KB CONTIGUOUS, is requested with whole-row 16-byte loads at the very top, the bias, the tile
  // bookkeeping and the first A tile are requested behind it, and only then do the slices pass through the (still unused) A
  // buffers, one tap at a time, for the waves to pick up their fragments.
  frag_t wreg[TAPS][KSTEPS];
  static_assert(WR_BN * LDK * (int)sizeof(TC) <= 2 * A_BYTES, "a tap's weight slice must fit in the A buffers");
  static_assert((WR_BN * KCH) % WR_THREADS == 0, "weight slice must split evenly over the workgroup");
  constexpr int W_PT = WR_BN * KCH / WR_THREADS;
  bf16x8 wtmp[TAPS][W_PT];
  // With a fragment-order copy of the weights (dx_pack_frag_major: a fragment is one contiguous KiB, and it is exactly
  // wreg[tap][ks] of the wave that owns channel block co0 / 32) the wave loads its 8 x TAPS fragments straight into their
  // registers: one round trip, no pass through LDS, none of the 2 TAPS barriers below.
  const bool wfrag = TAPS == 3 && p.w_frag != nullptr;
  if (wfrag) {
    const TC* wf = reinterpret_cast<const TC*>(p.w_frag) + (size_t)(co0 >> 5) * 512 + lane * 8;
    const size_t fstride = (size_t)(Cout >> 5) * 512;            // fragments of one (chunk, tap, half): all channel blocks
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
        wreg[tap][ks] = *reinterpret_cast<const frag_t*>(wf + (size_t)((((ks >> 1) * TAPS + tap) << 1) + (ks & 1)) * fstride);
  } else {
    const int cblk = zt * WR_BN;
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const TC* src = W + ((size_t)tap * Cout + cblk) * CIN;
#pragma unroll
      for (int t = 0; t < W_PT; ++t) wtmp[tap][t] = *reinterpret_cast<const bf16x8*>(src + (size_t)(tid + t * WR_THREADS) * 8);
    }
  }
  // The MFMAs run with the operands swapped (weights as A, activations as B), so the accumulator tile is D[co][position]:
  // a lane holds ONE position (l31) and, per group of 4 registers, 4 CONSECUTIVE output channels (rows (r & 3) + 8 (r >> 2)
  // + 4 g) -- row-major output leaves the registers without an LDS transpose.
  // (the data-gradient instantiation has no bias: its 16 registers hold the prefetched gate values instead, see gpre)
  float bvr[GATE ? 1 : 16];
  if constexpr (!GATE) {
#pragma unroll
    for (int r = 0; r < 16; ++r) bvr[r] = p.bias ? p.bias[co0 + dx_acc_row(r, g)] : 0.f;
  }

  // ---- this workgroup's share of the live position tiles (flat list over the batch)
  // (cooperative count + prefix sums in LDS, dx_block_count_scan: the serial walks over the lengths -- count, locate the first live
  //  tile, locate the first dead tile -- were most of this kernel's 8 us prologue)
  __shared__ int s_live[DX_SCAN_MAXB + 1], s_cum[DX_SCAN_MAXB + 1], s_part[WR_THREADS / 64];
  const bool scan = p.B <= DX_SCAN_MAXB;
  auto live_g = [&](int b) { return p.skip_len ? min(ptiles, dx_cdiv(min(N, (int)p.skip_len[b] + 2), BM)) : ptiles; };
  auto live_of = [&](int b) { return scan ? s_live[b] : live_g(b); };
  int total = 0, b = 0, pt = 0, nlive = 0, i0, i1;
  if (scan) {
    dx_block_count_scan<WR_THREADS>(p.B, live_g, [](int v) { return v; }, s_live, s_cum, s_part);
    total = s_cum[p.B];
    i0 = (int)((long)total * grp / ngrp); i1 = (int)((long)total * (grp + 1) / ngrp);
    b = dx_locate_item(s_cum, p.B, i0);
    nlive = s_live[b];
    pt = i0 - s_cum[b];
  } else {
    for (int bb = 0; bb < p.B; ++bb) total += live_g(bb);
    i0 = (int)((long)total * grp / ngrp); i1 = (int)((long)total * (grp + 1) / ngrp);
    for (int cum = 0; b < p.B; ++b) {
      nlive = live_g(b);
      if (i0 < cum + nlive) { pt = i0 - cum; break; }
      cum += nlive;
    }
  }
  int left = i1 - i0;

  // All global accesses of the tile loop are BUFFER loads / stores on a per-utterance resource: rows outside [0, N) are
  // dropped / read as zero by the hardware bounds check, so the loop body has no divergent branches and hipcc can count
  // the outstanding memory operations exactly (with `if (n < N)` around the stores it fell back to `s_waitcnt vmcnt(0)`
  // in front of every epilogue block, which also drained the A-tile prefetch issued at the top of the tile).
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t xbytes = (uint32_t)((size_t)N * p.ldx * sizeof(TC)), ybytes = (uint32_t)((size_t)N * p.ldy * sizeof(TO));
  bf16x8 ra[A_PT];
  auto fetch = [&](int fb, int fpt) {
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<TC*>(reinterpret_cast<const TC*>(p.x)) + (size_t)fb * N * p.ldx, 0, xbytes, 0x00020000);
#pragma unroll
    for (int t = 0; t < A_PT; ++t) {
      const int c = tid + t * WR_THREADS;
      const int n = fpt * BM + (c >> 4) - HALO;                       // -1 (halo of the first tile) wraps to out-of-range
      const uint32_t voff = c < A_CH ? (uint32_t)(n * (int)p.ldx + (c & 15) * 8) * (uint32_t)sizeof(TC) : 0xffffff00u;
      ra[t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)voff, 0, 0));
    }
  };
  auto commit = [&](int buf) {
    TC* As = reinterpret_cast<TC*>(smem + buf * A_BYTES);
#pragma unroll
    for (int t = 0; t < A_PT; ++t) {
      const int c = tid + t * WR_THREADS;
      if (c < A_CH) *reinterpret_cast<bf16x8*>(&As[(c >> 4) * LDK + (c & 15) * 8]) = ra[t];
    }
  };

  // Software pipeline inside a wave: the matrix pipe runs asynchronously, so the epilogue of one 64-row half (VALU +
  // LDS + stores) is issued in slices BETWEEN the MFMAs of the other half:
  //   phase A(t): MFMAs of rows 0..63 of tile t    ||  epilogue of rows 64..127 of tile t-1
  //   phase B(t): MFMAs of rows 64..127 of tile t  ||  epilogue of rows 0..63 of tile t
  // (measured before: MFMA loop 22 us + epilogue 15 us back to back; the two waves of a SIMD ran them in lockstep)
  struct Epi { int cb, n0, len; };   // utterance, first row of the tile, mask length
  // Epilogue of one 32-position accumulator tile, straight from registers.  bf16 output: two v_permlane32_swap per
  // 8-channel group gather a lane's 8 consecutive channels (16-byte stores; lanes g = 0 / 1 of a position write
  // channels [0, 8) / [8, 16) and [16, 24) / [24, 32) of the wave's 32); fp32 output: one 16-byte store per register group.
  // gate words of ONE 32-position tile (two 16-byte loads per lane), requested by gate_fetch one or more k-steps before the
  // epilogue slice that consumes them: issued inside epi_tile they were consumed by the very next instruction, a full
  // memory round trip with the wave unable to issue MFMAs, four times per position tile (the GATE variant ran 62 us where
  // the same GEMM without a gate runs 42).
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t gpre[2][2];
  auto gate_fetch = [&](u32x4_t* dst, const Epi& e, int row0) {
    if constexpr (GATE && BITS) {
      const int n = e.n0 + row0 + l31;
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint32_t*>(p.gate_bits) + ((size_t)e.cb * (Cout >> 5) + (co0 >> 5)) * N, 0, (uint32_t)((size_t)N * 4), 0x00020000);
      dst[0][0] = __builtin_amdgcn_raw_buffer_load_b32(rb, n * 4, 0, 0);      // (rows outside [0, N): zero = gate closed; their stores are dropped)
    } else if constexpr (GATE && sizeof(TO) == 2) {
      const int n = e.n0 + row0 + l31;
      const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<TG*>(G) + (size_t)e.cb * N * p.ldy, 0, (uint32_t)((size_t)N * p.ldy * sizeof(TG)), 0x00020000);
      const uint32_t eoff = (uint32_t)n * (uint32_t)p.ldy + (uint32_t)co0;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) dst[h2] = __builtin_amdgcn_raw_buffer_load_b128(rg, (int)((eoff + 16 * h2 + 8 * g) * 2u), 0, 0);
    }
  };
  auto epi_tile = [&](const f32x16& ac, const Epi& e, int row0, const u32x4_t* gw2) {
    const int n = e.n0 + row0 + l31;
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(Y + (size_t)e.cb * N * p.ldy, 0, ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<TG*>(GATE ? G : reinterpret_cast<const TG*>(Y)) + (size_t)e.cb * N * p.ldy, 0, (uint32_t)((size_t)N * p.ldy * sizeof(TG)), 0x00020000);
    const uint32_t eoff = (uint32_t)n * (uint32_t)p.ldy + (uint32_t)co0;     // element offset inside the utterance
    const bool zero_row = n >= e.len;              // mask_lengths
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      v[r] = GATE ? ac[r] : ac[r] + bvr[GATE ? 0 : r];
      if (GATE && p.bias) v[r] += p.bias[co0 + dx_acc_row(r, g)];      // (no caller on the step path gates AND biases: loaded in place)
      if (RELU) v[r] = fmaxf(v[r], 0.f);
    }
    if constexpr (sizeof(TO) == 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t o = (eoff + 8 * q + 4 * g) * 4u;
        f32x4 w = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        if (GATE) {
          const f32x4 gv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, (int)o, 0, 0));
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = gv[j] > 0.f ? w[j] : 0.f;
        }
        if (zero_row) w = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), ry, (int)o, 0, 0);
      }
    } else {
      typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      uint32_t P[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bf16x2 pr = {(bf16_t)v[2 * k], (bf16_t)v[2 * k + 1]};
        P[k] = __builtin_bit_cast(uint32_t, pr);
      }
      // (P0,P1 | P2,P3) and (P4,P5 | P6,P7): hi half of the first pair <-> lo half of the second
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const u32x2 sw = __builtin_amdgcn_permlane32_swap(P[4 * h2 + k], P[4 * h2 + 2 + k], false, false);
          P[4 * h2 + k] = sw[0];
          P[4 * h2 + 2 + k] = sw[1];
        }
      // now (P0, P1, P2, P3) = channel pairs (0,1)(2,3)(4,5)(6,7) + 8 g and (P4 .. P7) the same + 16
      if constexpr (RELU && BITS) {   // bit k / 16 + k of a lane's word: low / high half of P[k] is non-zero (values are >= 0: + 0x7fff carries into bit 15)
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) m |= (((P[k] + 0x7fff7fffu) >> (15 - k)) & (0x00010001u << k));
        const uint32_t mp = (uint32_t)__shfl_xor((int)m, 32, 64);
        uint32_t word = g ? (mp | (m << 8)) : (m | (mp << 8));      // lane group 0 in bits 0-7 / 16-23, group 1 in 8-15 / 24-31
        if (zero_row) word = 0u;
        const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
            p.relu_bits + ((size_t)e.cb * (Cout >> 5) + (co0 >> 5)) * N, 0, (uint32_t)((size_t)N * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(word, rb, g ? (int)0xffffff00u : n * 4, 0, 0);   // one lane of the pair stores (the other one out of range)
      }
      uint32_t own = 0;
      if constexpr (GATE && BITS) own = g ? (gw2[0][0] >> 8) : gw2[0][0];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const uint32_t o = (eoff + 16 * h2 + 8 * g) * 2u;
        u32x4 w = {P[4 * h2], P[4 * h2 + 1], P[4 * h2 + 2], P[4 * h2 + 3]};
        if constexpr (GATE && BITS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int k = 4 * h2 + j;
            const uint32_t lo = (uint32_t)__builtin_amdgcn_sbfe((int)own, k, 1), hi = (uint32_t)__builtin_amdgcn_sbfe((int)own, 16 + k, 1);
            w[j] &= (lo & 0x0000ffffu) | (hi & 0xffff0000u);
          }
        } else if (GATE) {   // gate > 0 on the packed bf16 bits: sign clear and magnitude non-zero  <=>  bits - 1 < 0x7fff (unsigned)
          const u32x4 gw = gw2[h2];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t m = (((gw[j] & 0xffffu) - 1u) < 0x7fffu ? 0x0000ffffu : 0u) | (((gw[j] >> 16) - 1u) < 0x7fffu ? 0xffff0000u : 0u);
            w[j] &= m;
          }
        }
        if (zero_row) w = u32x4{0u, 0u, 0u, 0u};
        __builtin_amdgcn_raw_buffer_store_b128(w, ry, (int)o, 0, 0);
      }
    }
  };
  // slice kk (0 .. TAPS*KSTEPS-1) of the epilogue of accumulator pair ac[0], ac[1] (rows [64 h, 64 h + 64) of tile e)
  // `nx` / `nh`: the rows whose epilogue runs in the NEXT phase (the accumulators being filled now): their gate words are
  // requested right after this phase's second drain has freed gpre -- two thirds of a phase plus the head of the next one ahead
  auto epi_slice = [&](int kk, const f32x16* ac, const Epi& e, int h, const Epi& nx, int nh) {
    constexpr int NS = TAPS * KSTEPS;
    // early in the phase: the end-of-tile wait for the prefetched A tile (vmcnt) also covers these stores
    if (kk == 1) epi_tile(ac[0], e, h * 64, gpre[0]);
    else if (kk == NS / 3) epi_tile(ac[1], e, h * 64 + 32, gpre[1]);
    else if (kk == NS / 3 + 1) { gate_fetch(gpre[0], nx, nh * 64); gate_fetch(gpre[1], nx, nh * 64 + 32); }
  };

  int buf = 0;
  if (left > 0) fetch(b, pt);
  if (!wfrag) {   // weights: registers (whole rows) -> LDS -> registers (MFMA fragments), see the top of the kernel
    TC* Ws = reinterpret_cast<TC*>(smem);
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      if (tap) __syncthreads();   // the previous tap's fragments have been read
#pragma unroll
      for (int t = 0; t < W_PT; ++t) {
        const int c = tid + t * WR_THREADS;
        *reinterpret_cast<bf16x8*>(&Ws[(c >> 4) * LDK + (c & 15) * 8]) = wtmp[tap][t];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks)
        wreg[tap][ks] = *reinterpret_cast<const frag_t*>(&Ws[(wave * 32 + l31) * LDK + ks * 16 + g * 8]);
    }
    __syncthreads();   // the A tile of the first position tile goes into the same memory
  }
  if (left > 0) commit(0);
  __syncthreads();
  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  Epi prev{0, N, 0};   // n0 = N: every row out of range, nothing is stored before the first tile
  while (left > 0) {
    const Epi cur{b, pt * BM, p.mask_len ? (int)p.mask_len[b] : N};
    const TC* As = reinterpret_cast<const TC*>(smem + buf * A_BYTES);
    --left;
    if (left > 0) {
      if (++pt >= nlive) { ++b; pt = 0; nlive = live_of(b); }
      fetch(b, pt);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // epilogue partner: phase A drains acc[2..3] of the previous tile, phase B drains acc[0..1] of this tile
      const Epi& ep = h == 0 ? prev : cur;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[h * 2 + i][r] = 0.f;   // drained one phase ago
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          frag_t a[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const frag_t*>(&As[(h * 64 + i * 32 + l31 + tap) * LDK + ks * 16 + g * 8]);
#pragma unroll
          for (int i = 0; i < 2; ++i) dx_mma(acc[h * 2 + i], wreg[tap][ks], a[i]);
          epi_slice(tap * KSTEPS + ks, &acc[h == 0 ? 2 : 0], ep, h == 0 ? 1 : 0, cur, h);
        }
      }
    }
    prev = cur;
    if (left > 0) commit(buf ^ 1);
    buf ^= 1;
    __syncthreads();
  }
  {   // drain: rows 64..127 of the last tile
#pragma unroll
    for (int kk = 0; kk < TAPS * KSTEPS; ++kk) epi_slice(kk, &acc[2], prev, 1, Epi{0, N, 0}, 0);
  }

  // ---- dead tiles (start past length + conv halo): zeros, no reads; split evenly like the live ones
  if (p.skip_len) {
    const int cblk = zt * WR_BN;
    const int dead = ptiles * p.B - total;
    const int j0 = (int)((long)dead * grp / ngrp), j1 = (int)((long)dead * (grp + 1) / ngrp);
    int db = 0, dpt = 0, cum = 0;
    if (scan && j0 < j1) {   // dead tiles before utterance u: u * ptiles - s_cum[u] (monotone): the largest u with that <= j0
      int lo = 0, hi = p.B - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (mid * ptiles - s_cum[mid] <= j0) lo = mid; else hi = mid - 1; }
      db = lo;
      dpt = s_live[db] + (j0 - (db * ptiles - s_cum[db]));
    } else if (!scan) {
      for (; db < p.B; ++db) {
        const int nd = ptiles - live_of(db);
        if (j0 < cum + nd) { dpt = live_of(db) + (j0 - cum); break; }
        cum += nd;
      }
    }
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = j0; j < j1; ++j) {
      const int fend = db < p.B ? dx_fill_end((int)p.skip_len[db], N) : 0;   // dead tiles past the fill end stay unwritten (dx_common.h)
      for (int c = tid; c < BM * (WR_BN / 8) && dpt * BM < fend; c += WR_THREADS) {
        const int n = dpt * BM + (c >> 5), co = cblk + (c & 31) * 8;
        if (n < fend) store8<TO>(Y + ((size_t)db * N + n) * p.ldy + co, z);
      }
      if (++dpt >= ptiles) { ++db; while (db < p.B && live_of(db) >= ptiles) ++db; dpt = db < p.B ? live_of(db) : 0; }
    }
  }
}

// activations and weights are bf16; TO / TG: output and gate type.  false = shape not taken, nothing launched
template <typename TO, typename TG>
bool try_weight_stationary(const ConvArgs& a, int taps, hipStream_t s) {
  if (a.ln.enabled || !conv_wreg_takes(a.Cin, a.Cout, a.N, a.ldx, a.ldy, a.flags)) return false;
  const int ztiles = a.Cout / WR_BN;
  // about one workgroup per CU; more position groups than tiles only adds weight loads
  const long tiles = (long)dx_cdiv(a.N, WR_BM) * a.B;
  int ngrp = 256 / ztiles;
  if (ngrp > tiles) ngrp = (int)tiles;
  if (ngrp < 1) ngrp = 1;
  dim3 grid(ngrp * ztiles), block(WR_THREADS);
  const bool relu = a.flags & DX_CONV_RELU, gate = a.gate != nullptr;
  if (a.relu_bits || a.gate_bits) {   // dx_conv1d_relu_bits: one bit per element written by the ReLU / read as the gate
    if constexpr (sizeof(TO) == 2) {
      if (taps != 3 || gate || (a.relu_bits != nullptr) == (a.gate_bits != nullptr) || (a.relu_bits && !relu) || (a.gate_bits && relu)) return false;
      if (a.relu_bits) hipLaunchKernelGGL((conv_wreg_kernel<TO, TG, 3, true, false, true>), grid, block, 0, s, a, ngrp);
      else hipLaunchKernelGGL((conv_wreg_kernel<TO, TG, 3, false, true, true>), grid, block, 0, s, a, ngrp);
      return true;
    } else {
      return false;
    }
  }
#define DX_WREG_LAUNCH(T, R, GT) hipLaunchKernelGGL((conv_wreg_kernel<TO, TG, T, R, GT>), grid, block, 0, s, a, ngrp)
  if (taps == 3) {
    if (relu && gate) DX_WREG_LAUNCH(3, true, true); else if (relu) DX_WREG_LAUNCH(3, true, false);
    else if (gate) DX_WREG_LAUNCH(3, false, true); else DX_WREG_LAUNCH(3, false, false);
  } else {
    if (relu && gate) DX_WREG_LAUNCH(1, true, true); else if (relu) DX_WREG_LAUNCH(1, true, false);
    else if (gate) DX_WREG_LAUNCH(1, false, true); else DX_WREG_LAUNCH(1, false, false);
  }
#undef DX_WREG_LAUNCH
  return true;
}

}  // namespace

// the shapes and epilogue options conv_wreg_kernel takes (bf16 operands): a pure predicate, shared by the launcher above and
// dx_conv1d_plain_path
bool conv_wreg_takes(int Cin, int Cout, int N, long ldx, long ldy, int flags) {
  if (flags & (DX_CONV_TRANSPOSED_OUT | DX_CONV_ACCUMULATE)) return false;
  if (Cin != 128 || Cout <= 0 || Cout % WR_BN || ldy % 8 || ldx % 8) return false;
  return (size_t)N * ldy * 4 < (1ull << 32) && (size_t)N * ldx * 2 < (1ull << 32);   // 32-bit buffer offsets
}

bool conv_wreg_try(const ConvArgs& a, bool bf16_out, int taps, hipStream_t s) {
  return bf16_out ? try_weight_stationary<bf16_t, bf16_t>(a, taps, s) : try_weight_stationary<float, float>(a, taps, s);
}
