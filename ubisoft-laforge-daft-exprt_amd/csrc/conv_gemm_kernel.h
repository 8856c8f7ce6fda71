// conv_gemm_kernel: the tiled conv GEMM, and the launch ladder of its LayerNorm-fused instantiations.  Included INSIDE the anonymous
// namespace of the three units that instantiate it (conv_gemm_plain.hip: LNM 0, conv_gemm_ln.hip: LNM 1, conv_gemm_lnbwd.hip: LNM 2 / 3),
// behind conv_args.h and conv_common.h; its A/B macros are defined here so that every unit sees one definition.
//
// Tiling: one workgroup (4 MFMA waves) computes a 64 / 128 / 256-position x 128-channel tile of ONE utterance, so
// the conv halo is simply rows n0-1 .. n0+rows of that utterance (rows outside [0, N) are zero padding).
// The K loop walks Cin in chunks of 32; per chunk the haloed activation tile and the weight tile (taps x 128 x 32)
// are staged in LDS (bf16: unpadded XOR-swizzled rows, fp32: rows padded by 16 B -> conflict-free ds_read_b128
// fragment reads), and every tap reuses the same activation tile at a row offset -- no im2col is materialised.
// Each wave owns a (32 MI) x 64 sub-tile = MI x 2 MFMA 32x32 accumulators.
// Operand type TC: bf16 (v_mfma_f32_32x32x16_bf16) or fp32 (v_mfma_f32_32x32x2_f32, exact fp32 mode).
// RING: an LDS-DMA ring with loader waves instead of the register-staged pipeline, and on top of it the balanced variable-height
// tiles of dx_conv_tile_plan.
#pragma once

// Pipeline: the global loads of K-chunk k+1 are issued into registers (raw element type, converted only when they are
// written to LDS) BEFORE the MFMAs of chunk k, so HBM/L2 latency hides under the matrix work; one LDS buffer, two
// barriers per chunk.  Epilogue: accumulators are staged through LDS (reusing the operand buffers) 64 rows at a time
// and leave as whole 16-byte row segments (16 lanes cover a 128-channel row) -- the MFMA C layout would otherwise
// emit 64 two-byte stores per lane.
#ifndef DX_CONV_WPS
#define DX_CONV_WPS 2
#endif
// MI = 32-row MFMA tiles per wave along the position axis: 2 -> 128-row workgroup tile; 1 -> 64-row tile, used when
// Cout <= 128 (one channel tile): twice the workgroups for the GEMMs whose grid would otherwise under-fill 256 CUs.
// BK = channels per K chunk: 32, or 64 for the narrow-output kernels whose long serial K loop is latency-bound.
#ifndef DX_CONV_WPS_NARROW
#define DX_CONV_WPS_NARROW 4
#endif
// LNM: 0 none, 1 forward LayerNorm, 2 backward LayerNorm with FiLM gradients, 3 backward LayerNorm without FiLM
// LDS-DMA ring pipeline (conv_gemm_kernel<..., RING>): bf16 operands, long contractions.  OPT-IN (DX_CONV_RING=1):
// measured on MI355X it ties with the register-staged pipeline (1024 -> 1024 k3: 814 vs 818 TFLOP/s; 1024 -> 128 k3
// 55 vs 61 us plain, 78 vs 72 us with the LayerNorm epilogue; training step 9.35 vs 9.36 ms) because neither is bound by
// its pipeline: a CU fetches at most ~30 B/clk from L2 (tools/probes/lds_dma_rate_probe.hip: 16-17 TB/s chip-wide for
// global_load_lds_dwordx4, 14 TB/s for loads to registers, independent of row width and of the number of pieces in
// flight), a 128 x 128 x (3 x 32) chunk needs 36 KB for 768 MFMA cycles = 47 B/clk, and the ablations of this kernel
// give 306 us with the MFMA waves idle, 237 us with the loaders idle, 367 us together.  Past ~800 TFLOP/s the lever
// is bytes per FLOP per CU (taller position tiles when the batch has enough of them), not the pipeline.
#ifndef DX_PLAN_RING
#define DX_PLAN_RING 3   // stages of the balanced-tile (plan) kernels: 3 x 41 KB (2: main loop 39.5 vs 36.1 us)
#endif
// RING: 0 = register-staged single-buffer pipeline; S >= 2 = S-stage LDS ring filled by four loader waves (512 threads, bf16)
#ifndef CG_K1_BK
#define CG_K1_BK 32   // K chunk of the LayerNorm-fused k = 1 GEMMs (64: A/B build; the operand image stays below the epilogue stage)
#endif
#ifndef CG_K1_PF
#define CG_K1_PF 1   // chunks in flight of the register-staged k = 1 GEMMs (2: measured +-0, 29.8 vs 30.5 us / 20.2 vs 19.6 us: the chunk period is its barrier / LDS chain, not the global round trip)
#endif
template <typename TA, typename TC, typename TO, typename TG, int TAPS, int MI, int BK, int LNM = 0, int RING = 0>
// (fp32 activations feeding bf16 MFMAs at k = 3 -- instantiations off the bf16 step path, the LayerNorm kernels hand the GEMMs bf16 copies --
// prefetch their K chunk as raw fp32: one wave per SIMD less than the bf16-input form instead of 28-52 bytes of scratch)
__global__ __launch_bounds__(RING ? 2 * NTHREADS : NTHREADS, RING ? 2 : ((sizeof(TA) == 4 && sizeof(TC) == 2 && TAPS == 3) ? (MI == 1 ? DX_CONV_WPS_NARROW - 1 : 1) : (MI == 1 ? DX_CONV_WPS_NARROW : DX_CONV_WPS))) void conv_gemm_kernel(ConvArgs p) {
  constexpr int LN = LNM == 3 ? 2 : LNM;
  constexpr bool LNFILM = LNM == 2;
  constexpr int BM = 64 * MI, KC = BK / 8;   // KC = 8-element chunks per row of a K chunk
  constexpr int HALO = TAPS / 2;
  constexpr int AROWS = BM + TAPS - 1;
  // LDS image of the operand tiles.  bf16 (BK = 32: four 16-byte chunks per row): NO padding, chunk c of row r sits at
  // chunk position c ^ ((r >> 2) & 3) -- the 16 rows of a ds_read_b128 lane group then cover all 64 banks, and the
  // 8 lanes of a ds_write_b128 group (2 rows x 4 chunks) cover 32 distinct banks.  (The padded 80-byte rows read
  // conflict-free but staged with 2-way write conflicts: SQ_LDS_BANK_CONFLICT was 30 % of the LDS cycles of a kernel
  // whose LDS pipe -- ds_write_b128 of the weight tile above all -- is busier than its matrix pipe.)  fp32: padded rows.
  constexpr bool SWZ = sizeof(TC) == 2 && BK == 32;
  constexpr int LDS_K = SWZ ? BK : BK + Pad<TC>::value;
  auto lds_at = [](int row, int chunk) { return SWZ ? row * LDS_K + ((chunk ^ ((row >> 2) & 3)) << 3) : row * LDS_K + (chunk << 3); };
  constexpr int A_CH = AROWS * (BK / 8), A_PT = (A_CH + NTHREADS - 1) / NTHREADS;
  constexpr int W_PT = TAPS * BN * (BK / 8) / NTHREADS;
  constexpr int STG_LD = BN + 4;
  // ring image of one K chunk: activation rows rounded up to whole 16-row DMA pieces, then the taps x 128 weight rows
  constexpr int AR16 = (AROWS + 15) & ~15, STAGE_EL = (AR16 + TAPS * BN) * 32;
  constexpr int OPER_BYTES = RING ? RING * STAGE_EL * 2 : (AROWS + TAPS * BN) * LDS_K * (int)sizeof(TC), STG_BYTES = 64 * STG_LD * 4 * (RING > 0 && MI == 4 ? 2 : 1);
  typedef typename Vec8<TC>::type frag_t;
  typedef typename VecN<TA, 8>::type raw_t;
  __shared__ __attribute__((aligned(16))) char smem[OPER_BYTES > STG_BYTES ? OPER_BYTES : STG_BYTES];
  TC* As = reinterpret_cast<TC*>(smem);
  TC* Ws = As + AROWS * LDS_K;
  float* stage = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, g = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware, weight-stationary order.  Workgroup L runs on XCD L % 8 (observed dispatch order).  Every workgroup
  // streams the whole weight slice of its channel tile (taps x 128 x Cin, up to 786 KB) through LDS, so the slice must
  // stay in that XCD's 4 MB L2 across workgroups: each XCD walks ALL of its position tiles for channel tile 0, then
  // for channel tile 1, ...  (Measured: no difference vs the channel-tile-fastest order on MI355X -- the kernel is bound
  // by its LDS->MFMA issue pattern at ~800 TFLOP/s, the known ceiling of a 128x128-tile two-barrier structure -- but this
  // order keeps the weight working set of an XCD at one slice, which matters once the inner loop gets faster.)
  // PLAN (ring kernels with 256-row tiles, one channel tile): the position tiles come from a table that cuts every
  // utterance into equal pieces of <= 256 rows such that the whole batch is a multiple of 256 workgroups of (nearly) the
  // same height -- a workgroup costs one pass over the weights whatever its height.  The padding rows [length, N) of the
  // batch are zero-filled by the loader waves, an equal share per workgroup, while the first chunks are in flight.
  constexpr bool PLAN = RING > 0 && MI == 4 && LNM != 0;
  int n0, b, co0, h = BM;              // h = rows of this tile
  int fill_per = 0;                    // PLAN: padding rows (flattened over the batch) this workgroup zero-fills
  if constexpr (PLAN) {
    co0 = 0;
    const int4 e = reinterpret_cast<const int4*>(p.plan)[blockIdx.x];
    b = e.x; n0 = e.y; h = e.z; fill_per = e.w;
    if (h <= 0 && threadIdx.x < NTHREADS) return;       // an empty tile: only its loader waves work (padding fill)
  } else {
    const int ztiles = dx_cdiv(p.Cout, BN), ptiles = dx_cdiv(p.N, BM);
    const int Lid = blockIdx.x, jj = Lid >> 3;
    const int per_xcd = (ptiles * p.B + 7) >> 3;         // position tiles owned by one XCD
    const int pt = (Lid & 7) + 8 * (jj % per_xcd);
    if (pt >= ptiles * p.B) return;
    n0 = (pt % ptiles) * BM; b = pt / ptiles; co0 = (jj / per_xcd) * BN;
    (void)ztiles;
  }
  const int N = p.N, Cin = p.Cin, Cout = p.Cout;
  const TA* X = reinterpret_cast<const TA*>(p.x) + (size_t)b * N * p.ldx;
  const TC* W = reinterpret_cast<const TC*>(p.w);
  const bool relu = p.flags & DX_CONV_RELU, trans = p.flags & DX_CONV_TRANSPOSED_OUT, accum = p.flags & DX_CONV_ACCUMULATE;
  const int len = p.mask_len ? (int)p.mask_len[b] : N;
  TO* Y = reinterpret_cast<TO*>(p.y);
  const TG* G = reinterpret_cast<const TG*>(p.gate);
  const bool vec_out = !trans && (Cout % 8 == 0) && (p.ldy % 8 == 0);

  // padding early-out: a tile that starts past length + conv halo cannot reach a valid output -> zeros, no MFMA
  if (!PLAN && p.skip_len && n0 >= (int)p.skip_len[b] + 2) {
    if (RING && tid >= NTHREADS) return;             // loader waves
    if (!trans && n0 >= dx_fill_end((int)p.skip_len[b], N)) return;   // past the fill end: nobody reads these rows (dx_common.h); the
                                                                        // transposed (B, C, N) form is the user-visible mel: fully padded
    if (LN == 2) {   // incoming residual gradient rows are zero there and stay; the bf16 dx_pre rows must exist as zeros
      float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int c = tid; c < BM * (BN / 8); c += NTHREADS) {
        const int n = n0 + (c >> 4), cl = (c & 15) * 8;
        if (n >= N) continue;
        const size_t off = ((size_t)b * N + n) * BN + cl;
        store8<float>(p.ln.y + off, z);
        store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + off, z);
      }
      return;
    }
    if (accum) return;
    if (LN == 1) {
      float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int c = tid; c < BM * (BN / 8); c += NTHREADS) {
        const int n = n0 + (c >> 4), cl = (c & 15) * 8;
        if (n >= N) continue;
        const size_t off = ((size_t)b * N + n) * BN + cl;
        if (p.ln.y) store8<float>(p.ln.y + off, z);
        if (p.ln.y_lp) store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + off, z);
        if (p.ln.s_out) store8<float>(p.ln.s_out + off, z);
        if (p.ln.mean && cl == 0) { p.ln.mean[(size_t)b * N + n] = 0.f; p.ln.rstd[(size_t)b * N + n] = 0.f; }
      }
      return;
    }
    if (vec_out) {
      float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int c = tid; c < BM * (BN / 8); c += NTHREADS) {
        const int n = n0 + (c >> 4), co = co0 + (c & 15) * 8;
        if (n < N && co < Cout) store8<TO>(Y + ((size_t)b * N + n) * p.ldy + co, z);
      }
    } else {
      for (int c = tid; c < BM * BN; c += NTHREADS) {
        const int n = n0 + (trans ? c % BM : c / BN), co = co0 + (trans ? c / BM : c % BN);
        if (n < N && co < Cout) Y[trans ? ((size_t)b * Cout + co) * p.ldy + n : ((size_t)b * N + n) * p.ldy + co] = (TO)0.f;
      }
    }
    return;
  }

  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if constexpr (RING > 0) {
    // ---- LDS-DMA ring with dedicated loader waves (bf16 operands, Cin % 32 == 0; 512-thread workgroup).
    // Waves 0-3 run the MFMAs exactly as in the register-staged pipeline; waves 4-7 (one per SIMD, next to an MFMA
    // wave) only move data: measured with the MFMA waves issuing their own loads, a 1-wave-per-SIMD workgroup spends
    // more time ISSUING global -> LDS pieces (~100 cycles each, in order with its MFMAs) than the MFMAs take.
    // A K chunk's image is (AR16 + TAPS * 128) rows of 64 bytes in the swizzled layout of lds_at, written by
    // global_load_lds_dwordx4 pieces of 16 rows (1 KiB per wave instruction; LDS destination = piece base + 16 * lane,
    // so the swizzle is applied to each lane's SOURCE chunk).  Piece q belongs to loader q % 4; rows outside the
    // utterance / beyond Cout read a zero page.
    // Per chunk k, ONE workgroup barrier: a loader arrives after its pieces of chunk k have landed (counted vmcnt: the
    // RING - 2 younger chunks stay in flight), an MFMA wave after it has finished reading chunk k - 1.  Past the
    // barrier the MFMA waves read chunk k and the loaders refill the buffer chunk k - 1 just left with chunk k + RING - 1.
    static_assert(sizeof(TA) == 2 && sizeof(TC) == 2 && BK == 32, "ring pipeline: bf16 operands, 32-channel chunks");
    // pieces of a chunk: the first nA cover the h + TAPS - 1 activation rows of this tile, then TAPS * 8 weight pieces
    constexpr int W_INS = TAPS * BN / 16, MAXP = (AR16 / 16 + W_INS + 3) / 4, NSTEP = TAPS * 2;
    const int nA = (h + TAPS - 1 + 15) >> 4, nP = nA + W_INS;
    TC* ring = reinterpret_cast<TC*>(smem);
    const int nk = Cin >> 5;
    if (wave >= 4) {
      const int lw = __builtin_amdgcn_readfirstlane(wave) - 4;
      const int mine = (nP - lw + 3) >> 2;                       // pieces lw, lw + 4, ... of every chunk are this loader's
      const TC* src[MAXP];
      int dst[MAXP];
#pragma unroll
      for (int t = 0; t < MAXP; ++t) {
        const int q = lw + 4 * t;
        const bool isw = q >= nA;
        const int r = (isw ? q - nA : q) * 16 + (lane >> 2);     // row of the activation / weight image this lane fills
        const int c = (lane & 3) ^ ((r >> 2) & 3);                // source chunk that belongs at position lane & 3
        const TC* sp = reinterpret_cast<const TC*>(dx_zero_page) + c * 8;
        const int n = n0 + r - HALO, co = co0 + (r & (BN - 1));
        const TC* xa = reinterpret_cast<const TC*>(X) + (long)n * p.ldx + c * 8;
        const TC* wa = W + ((size_t)(r / BN) * Cout + co) * Cin + c * 8;
        sp = (!isw && r < h + TAPS - 1 && n >= 0 && n < N) ? xa : sp;
        sp = (isw && q < nP && co < Cout) ? wa : sp;
        src[t] = sp;
        dst[t] = __builtin_amdgcn_readfirstlane((isw ? AR16 / 16 + q - nA : q) * 512);
      }
      auto issue_chunk = [&](int kc, int buf) {
#pragma unroll
        for (int t = 0; t < MAXP; ++t)
          if (t < mine)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[t] + kc * 32),
                                             (__attribute__((address_space(3))) void*)(ring + buf * STAGE_EL + dst[t]), 16, 0, 0);
      };
      auto wait_landed = [&](int keep) {                         // s_waitcnt vmcnt(keep), keep wave-uniform
        switch (keep) {
#define DX_VMW(n) case n: asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); break;
          DX_VMW(1) DX_VMW(2) DX_VMW(3) DX_VMW(4) DX_VMW(5) DX_VMW(6) DX_VMW(7) DX_VMW(8) DX_VMW(9) DX_VMW(10) DX_VMW(11) DX_VMW(12)
          DX_VMW(13) DX_VMW(14) DX_VMW(15) DX_VMW(16) DX_VMW(17) DX_VMW(18) DX_VMW(19) DX_VMW(20) DX_VMW(21) DX_VMW(22) DX_VMW(23) DX_VMW(24)
          DX_VMW(25) DX_VMW(26) DX_VMW(27) DX_VMW(28) DX_VMW(29) DX_VMW(30) DX_VMW(31) DX_VMW(32) DX_VMW(33) DX_VMW(34) DX_VMW(35) DX_VMW(36)
#undef DX_VMW
          default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      };
      static_assert(MAXP * (RING - 2) <= 36, "vmcnt switch too short");
#pragma unroll
      for (int st = 0; st < RING - 1; ++st)
        if (st < nk && h > 0) issue_chunk(st, st);
      bool stores_in_flight = false;
      if constexpr (PLAN) {
        // padding fill: the batch's padding rows, flattened utterance by utterance, are split evenly over the workgroups;
        // this one owns [lo, hi).  Each loader wave finds the utterances its range touches with a wave scan over the
        // lengths, and the 256 loader threads share the 16-byte segments of those rows.
        const long lo = (long)blockIdx.x * fill_per, hi = lo + fill_per;
        const int ltid = lw * 64 + lane;
        long carry = 0;
        for (int base = 0; base < p.B && carry < hi; base += 64) {
          const int ub = base + lane;
          const int ulen = ub < p.B ? (int)p.skip_len[ub] : N;
          const int dead = ub < p.B ? N - (ulen < 0 ? 0 : (ulen > N ? N : ulen)) : 0;
          int incl = dead;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
          const long ustart = carry + incl - dead, uend = carry + incl;
          const long fs = ustart > lo ? ustart : lo, fe = uend < hi ? uend : hi;
          unsigned long long todo = __ballot(fs < fe);
          while (todo) {
            const int src_lane = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int fb = base + src_lane;
            const int first = __shfl(N - dead + (int)(fs - ustart), src_lane, 64);
            int cnt = __shfl((int)(fe - fs), src_lane, 64);
            cnt = min(cnt, dx_fill_end((int)p.skip_len[fb], N) - first);   // dead rows past the fill end stay unwritten (dx_common.h)
            float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int c = ltid; c < cnt * (BN / 8); c += NTHREADS) {
              const int n = first + (c >> 4), cl = (c & 15) * 8;
              const size_t off = ((size_t)fb * N + n) * BN + cl;
              if (LN == 2 || p.ln.y) store8<float>(p.ln.y + off, z);
              if (LN == 2 || p.ln.y_lp) store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + off, z);
              if (LN == 1) {
                if (p.ln.s_out) store8<float>(p.ln.s_out + off, z);
                if (p.ln.mean && cl == 0) { p.ln.mean[(size_t)fb * N + n] = 0.f; p.ln.rstd[(size_t)fb * N + n] = 0.f; }
              }
            }
            stores_in_flight = true;
          }
          carry += __shfl(incl, 63, 64);
        }
        if (h <= 0) return;
      }
      int nbuf = RING - 1, k = 0;                                // buffer that chunk k + RING - 1 goes to
      for (; k + RING - 1 < nk; ++k) {
        // (the fill's stores share the counter and may retire out of order with the loads: drain everything once)
        if (PLAN && k == 0 && stores_in_flight) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else wait_landed(mine * (RING - 2));
        __builtin_amdgcn_s_barrier();
        issue_chunk(k + RING - 1, nbuf);
        nbuf = nbuf + 1 == RING ? 0 : nbuf + 1;
      }
      for (; k < nk; ++k) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if (!PLAN) return;                                          // fixed tiles: the epilogue belongs to the MFMA waves
    }
    // MFMA waves.  PLAN: wave (wm, wn) owns the 32-row blocks wm, wm + 2, ... (interleaved, so a short tile still
    // spreads over both wave rows) and skips the blocks past the tile's height; the loader waves come back for the
    // epilogue as a second 256-thread team (one 64-row slab each per round).
    if (wave < 4) {
    auto row_of = [&](int i) { return PLAN ? (2 * i + wm) * 32 : wm * 32 * MI + i * 32; };
    const int nact = PLAN ? __builtin_amdgcn_readfirstlane((((h + 31) >> 5) - wm + 1) >> 1) : MI;
    auto mainloop = [&](auto na_tag) {
      constexpr int NA = decltype(na_tag)::value;
      int buf = 0;
      for (int k = 0; k < nk; ++k) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if constexpr (NA > 0) {
          const TC* Ar = ring + buf * STAGE_EL;
          const TC* Wr = Ar + AR16 * 32;
          frag_t a[2][NA], bf[2][2];
          auto load_frags = [&](int step, frag_t* af, frag_t* bfr) {
            const int tap = step >> 1, ks = step & 1;
#pragma unroll
            for (int i = 0; i < NA; ++i) af[i] = *reinterpret_cast<const frag_t*>(&Ar[lds_at(row_of(i) + l31 + tap, ks * 2 + g)]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bfr[j] = *reinterpret_cast<const frag_t*>(&Wr[lds_at(tap * BN + wn * 64 + j * 32 + l31, ks * 2 + g)]);
          };
          load_frags(0, a[0], bf[0]);
#pragma unroll
          for (int step = 0; step < NSTEP; ++step) {   // fragments of k-step s + 1 are read before the MFMAs of k-step s
            if (step + 1 < NSTEP) load_frags(step + 1, a[(step + 1) & 1], bf[(step + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < NA; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j) dx_mma(acc[i][j], a[step & 1][i], bf[step & 1][j]);
          }
        }
        buf = buf + 1 == RING ? 0 : buf + 1;
      }
    };
    if (nact >= MI) mainloop(std::integral_constant<int, MI>{});
    else if (MI > 3 && nact == 3) mainloop(std::integral_constant<int, (MI > 3 ? 3 : MI)>{});
    else if (MI > 2 && nact == 2) mainloop(std::integral_constant<int, (MI > 2 ? 2 : MI)>{});
    else if (MI > 1 && nact == 1) mainloop(std::integral_constant<int, 1>{});
    else mainloop(std::integral_constant<int, 0>{});
    }
    __syncthreads();                                 // every MFMA wave is done with the ring: the epilogue stages through it
  } else {
  // register-staged pipeline.  CG_K1_PF = 2 keeps TWO chunks of the k = 1 GEMMs in flight in two static register sets: no gain (see the
    // macro) -- their chunk loop (0.74 us per chunk, tools/cg_timing_k1.py: 8.9 us of an 18 us QKV data gradient, 3.6 us of a 14 us
    // out-projection + LayerNorm whose epilogue runs at 5 TB/s) is bound by its two barriers and the LDS round trip per chunk
    constexpr int PF = TAPS == 1 ? CG_K1_PF : 1;
    raw_t ra[PF][A_PT];
    frag_t rw[PF][W_PT];
    auto fetch = [&](auto slot, int k0) {
      constexpr int S = decltype(slot)::value;
#pragma unroll
      for (int t = 0; t < A_PT; ++t) {
        const int c = tid + t * NTHREADS;
        const int r = c / KC, kc = (c % KC) * 8;
        const int n = n0 + r - HALO, ci = k0 + kc;
#pragma unroll
        for (int e = 0; e < 8; ++e) ra[S][t][e] = (TA)0.f;
        if (c < A_CH && n >= 0 && n < N && ci < Cin) ra[S][t] = raw_load8<TA>(X + (size_t)n * p.ldx + ci);
      }
#pragma unroll
      for (int t = 0; t < W_PT; ++t) {
        const int c = tid + t * NTHREADS;
        const int tap = c / (BN * KC), rem = c - tap * (BN * KC);
        const int row = rem / KC, kc = (rem % KC) * 8;
        const int co = co0 + row, ci = k0 + kc;
        rw[S][t] = zero8<TC>();
        if (co < Cout && ci < Cin) rw[S][t] = *reinterpret_cast<const frag_t*>(W + ((size_t)tap * Cout + co) * Cin + ci);
      }
    };
    auto commit = [&](auto slot) {
      constexpr int S = decltype(slot)::value;
#pragma unroll
      for (int t = 0; t < A_PT; ++t) {
        const int c = tid + t * NTHREADS;
        if (c < A_CH) *reinterpret_cast<frag_t*>(&As[lds_at(c / KC, c % KC)]) = cvt8<TA, TC>(ra[S][t]);
      }
#pragma unroll
      for (int t = 0; t < W_PT; ++t) {
        const int c = tid + t * NTHREADS;
        const int tap = c / (BN * KC), rem = c - tap * (BN * KC);
        *reinterpret_cast<frag_t*>(&Ws[lds_at(tap * BN + rem / KC, rem % KC)]) = rw[S][t];
      }
    };
    auto compute = [&]() {
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
          frag_t a[MI], bf[2];
#pragma unroll
          for (int i = 0; i < MI; ++i)
            a[i] = *reinterpret_cast<const frag_t*>(&As[lds_at(wm * 32 * MI + i * 32 + l31 + tap, ks * 2 + g)]);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            bf[j] = *reinterpret_cast<const frag_t*>(&Ws[lds_at(tap * BN + wn * 64 + j * 32 + l31, ks * 2 + g)]);
#pragma unroll
          for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) dx_mma(acc[i][j], a[i], bf[j]);
        }
      }
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, PF - 1>;

    fetch(S0{}, 0);
    if constexpr (PF == 2) {
      if (BK < Cin) fetch(S1{}, BK);
      commit(S0{});
      __syncthreads();
      // chunk k0 is in LDS, chunk k0 + BK in the registers of the other set, chunk k0 + 2 BK is requested into the set just committed
      auto step = [&](auto cur, auto nxt, int k0) {
        if (k0 + 2 * BK < Cin) fetch(cur, k0 + 2 * BK);
        compute();
        __syncthreads();
        if (k0 + BK < Cin) {
          commit(nxt);
          __syncthreads();
        }
      };
      for (int k0 = 0; k0 < Cin; k0 += 2 * BK) {
        step(S0{}, S1{}, k0);
        if (k0 + BK < Cin) step(S1{}, S0{}, k0 + BK);
      }
    } else {
      commit(S0{});
      __syncthreads();
      for (int k0 = 0; k0 < Cin; k0 += BK) {
        const bool more = k0 + BK < Cin;
        if (more) fetch(S0{}, k0 + BK);
        compute();
        __syncthreads();
        if (more) {
          commit(S0{});
          __syncthreads();
        }
      }
    }
  }

  // ---- epilogue
  constexpr int NCS = LNM == 2 ? 4 : (LNM == 3 ? 2 : 1);
  float csum[NCS][8];   // LN backward: this thread's column sums (dgamma, dbeta [, dfilm_g, dfilm_b]) over its rows
#pragma unroll
  for (int q = 0; q < NCS; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) csum[q][e] = 0.f;
  // PLAN: two teams of 256 threads (MFMA waves / loader waves) take one 64-row slab each per round
  constexpr int ETEAMS = PLAN ? 2 : 1;
  const int team = PLAN ? tid >> 8 : 0, etid = PLAN ? tid & 255 : tid;
  float* const mystage = stage + team * (64 * STG_LD);
  if (vec_out) {
#pragma unroll
    for (int ip = 0; ip < MI / ETEAMS; ++ip) {
      if (PLAN && ip * 64 * ETEAMS >= h) break;                   // workgroup-uniform: the barriers below stay matched
      const int i = ip * ETEAMS + team;                           // this team's slab
      // phase 1: bias + ReLU in the MFMA layout, accumulators -> LDS stage (64 rows x 128 channels, fp32, one per team)
      if (!PLAN || tid < NTHREADS) {
#pragma unroll
        for (int sl = 0; sl < ETEAMS; ++sl) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int cl = wn * 64 + j * 32 + l31, co = co0 + cl;
            const float bv = (p.bias && co < Cout) ? p.bias[co] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              float v = acc[ip * ETEAMS + sl][j][r] + bv;
              if (relu) v = fmaxf(v, 0.f);
              stage[sl * (64 * STG_LD) + (wm * 32 + dx_acc_row(r, g)) * STG_LD + cl] = v;
            }
          }
        }
      }
      // LayerNorm epilogues: the global inputs of all four passes are requested BEFORE the barrier (one round trip per
      // 64-row slab; issued pass by pass they are four dependent trips, because the in-place stores of a pass may alias
      // the loads of the next one as far as the compiler knows -- they never do: every row belongs to one thread group)
      constexpr bool PFB = !(LNFILM && MI != 2);     // FiLM-gradient variants at the 128 / 256 register caps: loads stay in their pass
      f32x8 pf_a[4], pf_b[4];
      float pf_m[4], pf_r[4];
      // the per-channel operands of the row passes (gamma, beta, FiLM row of this utterance) depend on the thread's channel segment
      // only: requested once per slab in front of the barrier.  Inside the passes every one of them sat behind the stores of the
      // pass before -- y / s_out may alias them as far as the compiler knows -- one exposed L2 round trip per pass (conv_sk_kernel:
      // 8.9 -> 7.3 us of epilogue).  Not for the variants at their register caps (PFB).
      const int cl_h = (etid & 15) * 8;
      f32x8 gm_h, bt_h, fg_h, fb_h;
      if (LN != 0 && PFB) {
        gm_h = raw_load8<float>(p.ln.gamma + cl_h);
        if (LN == 1 || LNFILM) bt_h = raw_load8<float>(p.ln.beta + cl_h);
        if (p.ln.film && (LN == 1 || LNFILM)) fg_h = raw_load8<float>(p.ln.film + (size_t)b * p.ln.ldf + cl_h);
        if (p.ln.film && LN == 1) fb_h = raw_load8<float>(p.ln.film + (size_t)b * p.ln.ldf + BN + cl_h);
      }
      if (LN != 0 && PFB) {
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
          const int sr = (etid >> 4) + pass * 16;
          const int trow = PLAN ? i * 64 + sr : (sr >> 5) * 32 * MI + i * 32 + (sr & 31);
          const int n = n0 + trow, cl = (etid & 15) * 8;
          if (n < N && trow < h) {
            const size_t rowg = (size_t)b * N + n, offl = rowg * BN + cl;
            if (LN == 2) {
              pf_a[pass] = raw_load8<float>(p.ln.y + offl);
              pf_b[pass] = raw_load8<float>(p.ln.s_out + offl);
              pf_m[pass] = p.ln.mean[rowg];
              pf_r[pass] = p.ln.rstd[rowg];
            } else {
              pf_a[pass] = raw_load8<float>(p.ln.residual + offl);
            }
          }
        }
      }
      __syncthreads();
      // phase 2: whole 16-byte row segments: gate, mask, accumulate, store
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int sr = (etid >> 4) + pass * 16;                    // stage row 0..63
        const int trow = PLAN ? i * 64 + sr : (sr >> 5) * 32 * MI + i * 32 + (sr & 31);   // row inside the tile
        const int n = n0 + trow, cl = (etid & 15) * 8, co = co0 + cl;
        if (n < N && co < Cout && trow < h) {
          float v[8];
          const f32x4 lo = *reinterpret_cast<const f32x4*>(&mystage[sr * STG_LD + cl]);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(&mystage[sr * STG_LD + cl + 4]);
          v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
          if (LN == 2) {        // fused LayerNorm BACKWARD: v + residual gradient = dL/d(LN output) of this row
            const size_t rowg = (size_t)b * N + n, offl = rowg * BN + cl;
            {
              const f32x8 r = PFB ? pf_a[pass] : raw_load8<float>(p.ln.y + offl);
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = n < len ? v[e] + r[e] : 0.f;     // masked_fill rows carry no gradient
            }
            const f32x8 sv = PFB ? pf_b[pass] : raw_load8<float>(p.ln.s_out + offl);
            const float mean = PFB ? pf_m[pass] : p.ln.mean[rowg], rstd = PFB ? pf_r[pass] : p.ln.rstd[rowg];
            const f32x8 gm = PFB ? gm_h : raw_load8<float>(p.ln.gamma + cl);
            float xh[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) xh[e] = (sv[e] - mean) * rstd;
            if (LNFILM) {                                         // y = fg * LN + fb
              const f32x8 fg = PFB ? fg_h : raw_load8<float>(p.ln.film + (size_t)b * p.ln.ldf + cl), bt = PFB ? bt_h : raw_load8<float>(p.ln.beta + cl);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                csum[LNFILM ? 2 : 0][e] += v[e] * (xh[e] * gm[e] + bt[e]);
                csum[LNFILM ? 3 : 0][e] += v[e];
                v[e] *= fg[e];
              }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              csum[0][e] += v[e] * xh[e];
              csum[1][e] += v[e];
              v[e] *= gm[e];
              s1 += v[e];
              s2 += v[e] * xh[e];
            }
            s1 = dx_row16_sum(s1); s2 = dx_row16_sum(s2);
            s1 *= 1.f / BN; s2 *= 1.f / BN;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = rstd * (v[e] - s1 - xh[e] * s2);
            store8<float>(p.ln.y + offl, v);                      // ds, in place of the residual gradient
            if (p.ln.p_pre > 0.f) {
              const uint32_t th = dx_drop_th8(p.ln.p_pre), key = dx_key32(dx_seed_eff(p.ln.seed_pre, p.ln.step), 0);
              const float sc = dx_drop_inv_keep8(th);
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = dx_keep_elem(key, (uint32_t)rowg * BN + cl + e, th) ? v[e] * sc : 0.f;
            }
            store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + offl, v);
            continue;
          }
          if (LN == 1) {        // fused LayerNorm: 16 lanes hold one complete 128-channel row
            const size_t rowg = (size_t)b * N + n, offl = rowg * BN + cl;
            if (p.ln.p_pre > 0.f) {
              const uint32_t th = dx_drop_th8(p.ln.p_pre), key = dx_key32(dx_seed_eff(p.ln.seed_pre, p.ln.step), 0);
              const float sc = dx_drop_inv_keep8(th);
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = dx_keep_elem(key, (uint32_t)rowg * BN + cl + e, th) ? v[e] * sc : 0.f;
            }
            {
              const f32x8 r = pf_a[pass];
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] += r[e];
            }
            if (p.ln.s_out) store8<float>(p.ln.s_out + offl, v);
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += v[e];
            sum = dx_row16_sum(sum);
            const float mean = sum * (1.f / BN);
            float sq = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[e] - mean; sq += d * d; }
            sq = dx_row16_sum(sq);
            const float rstd = rsqrtf(sq * (1.f / BN) + 1e-5f);
            if (p.ln.mean && cl == 0) { p.ln.mean[rowg] = mean; p.ln.rstd[rowg] = rstd; }
            const f32x8 gm = gm_h, bt = bt_h;                      // (LN == 1: PFB is always true)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (v[e] - mean) * rstd * gm[e] + bt[e];
            if (p.ln.film) {
              const f32x8 fg = fg_h, fb = fb_h;
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = fg[e] * v[e] + fb[e];
            }
            if (n >= len) {
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
            if (p.ln.y) store8<float>(p.ln.y + offl, v);       // (NULL: the consumer of the fp32 stream re-derives it, LNEpi::res_mean)
            if (p.ln.y_lp) store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + offl, v);
            continue;
          }
          const size_t off = ((size_t)b * N + n) * p.ldy + co;
          if (G) {
            const typename VecN<TG, 8>::type gv = raw_load8<TG>(G + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = ((float)gv[e] > 0.f) ? v[e] : 0.f;
          }
          if (n >= len) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
          }
          if (accum) {
            const typename VecN<TO, 8>::type old = raw_load8<TO>(Y + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += (float)old[e];
          }
          store8<TO>(Y + off, v);
        }
      }
      __syncthreads();
    }
    if (LN == 2) {   // column sums: 16 row-threads per channel segment -> LDS -> one atomic per channel per workgroup
      constexpr int nq = NCS;
      constexpr int RG = 16 * ETEAMS;                               // row groups (16 threads each) that hold partial sums
      for (int q = 0; q < nq; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) stage[(q * RG + (tid >> 4)) * BN + (tid & 15) * 8 + e] = csum[q][e];
      __syncthreads();
      for (int idx = tid; idx < nq * BN; idx += NTHREADS * ETEAMS) {
        const int q = idx / BN, c = idx - q * BN;
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < RG; ++r) t += stage[(q * RG + r) * BN + c];
        if (q == 0) atomicAdd(p.ln.dgamma + c, t);
        else if (q == 1) atomicAdd(p.ln.dbeta + c, t);
        else atomicAdd(p.ln.dfilm + (size_t)b * p.ln.lddf + (q == 3 ? BN : 0) + c, t);
      }
    }
    return;
  }
  // scalar path: transposed output (mel projection) or channel counts that are not multiples of 8
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = co0 + wn * 64 + j * 32 + l31;
    if (co >= Cout) continue;
    const float bv = p.bias ? p.bias[co] : 0.f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wm * 32 * MI + i * 32 + dx_acc_row(r, g);
        if (n >= N) continue;
        float v = acc[i][j][r] + bv;
        if (relu) v = fmaxf(v, 0.f);
        const size_t off = trans ? ((size_t)b * Cout + co) * p.ldy + n : ((size_t)b * N + n) * p.ldy + co;
        if (G) v = ((float)G[off] > 0.f) ? v : 0.f;
        if (n >= len) v = 0.f;
        if (accum) v += (float)Y[off];
        Y[off] = (TO)v;
      }
    }
  }
}

// Launch ladder of the LayerNorm-fused instantiations (one channel tile, Cout = 128): LN = 1 forward (conv_gemm_ln.hip), LN = 2 backward
// (conv_gemm_lnbwd.hip).  `path` is what dx_conv1d_ln_path said; DX_LN_PATH_SPLITK is not a path of this kernel (conv_sk.hip).
template <typename TA, typename TC, int LN>
int launch_ln_taps(const ConvArgs& a, int path, int taps, hipStream_t s) {
  typedef float TO, TG;                              // the LayerNorm epilogues write fp32 rows (+ a bf16 copy) and take no gate
  constexpr int LNB = LN == 2 ? 3 : LN;             // backward without FiLM gradients: fewer registers
  constexpr bool BF16 = sizeof(TA) == 2 && sizeof(TC) == 2;   // the plan paths are bf16 kernels (the classifier never names them otherwise)
  const bool film = LN == 2 && a.ln.film != nullptr;
  const dim3 plan_grid((unsigned)a.plan_tiles), plan_block(2 * NTHREADS), block(NTHREADS);
  auto fixed_grid = [&](int rows) { return dim3((unsigned)((((long)dx_cdiv(a.N, rows) * a.B + 7) / 8) * 8)); };
#define DX_LN_LAUNCH(grid, block, ...)                                                               \
  do {                                                                                               \
    if (film) { constexpr int LNX = LN; hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, a); }   \
    else { constexpr int LNX = LNB; hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, a); }       \
  } while (0)
  switch (path) {
    case DX_LN_PATH_PLAN_K3:
      if constexpr (BF16) DX_LN_LAUNCH(plan_grid, plan_block, conv_gemm_kernel<TA, TC, TO, TG, 3, 4, 32, LNX, DX_PLAN_RING>);
      break;
    case DX_LN_PATH_PLAN_K1:
      if constexpr (BF16 && LN == 2) DX_LN_LAUNCH(plan_grid, plan_block, conv_gemm_kernel<TA, TC, TO, TG, 1, 4, 32, LNX, 3>);
      break;
    case DX_LN_PATH_ROWS128:
      DX_LN_LAUNCH(fixed_grid(128), block, conv_gemm_kernel<TA, TC, TO, TG, 3, 2, 32, LNX>);
      break;
    default:                  // DX_LN_PATH_ROWS64 (DX_LN_PATH_SPLITK never comes here)
      if (taps == 1) DX_LN_LAUNCH(fixed_grid(64), block, conv_gemm_kernel<TA, TC, TO, TG, 1, 1, CG_K1_BK, LNX>);
      else DX_LN_LAUNCH(fixed_grid(64), block, conv_gemm_kernel<TA, TC, TO, TG, 3, 1, 32, LNX>);
  }
#undef DX_LN_LAUNCH
  DX_LAUNCH_CHECK();
  return DX_OK;
}
