// conv_sk_kernel: the narrow-output k = 3 conv GEMM with LayerNorm epilogues, split-K inside the workgroup, and its launcher.
#include <type_traits>

#include "conv_args.h"

namespace {

#include "conv_common.h"

// ---- narrow-output k = 3 GEMM with the LayerNorm epilogues, split-K INSIDE the workgroup (conv_sk_kernel) ------------------------
// The balanced-tile ring kernel (conv_gemm_kernel.h, PLAN) gives every CU one pass over the 786 KB weight slice of a 1024 -> 128 k = 3 GEMM, but its
// main loop runs at a third of the matrix rate: weights (24 KB per K chunk) and activations (8 KB) share one LDS ring filled by
// LDS-DMA, whose issue -> landed latency is ~1 us under load, so the bytes a CU can have in flight (two ring stages) cap the
// stream at ~30 GB/s per CU; 4 x 2 register blocking needs 0.75 KB of LDS fragments per MFMA on top.  Here
//   * the workgroup is 4 waves, ONE per SIMD, with the full 512-register file each (accumulators in AGPRs), and the contraction
//     is split between the waves (the comment inside the kernel has the details): the register file is the weight ring -- the
//     weights are stored in fragment order (dx_pack_frag_major: a fragment is one contiguous KiB), come straight from L2 into
//     registers, every fragment read by exactly ONE wave of the workgroup: 786 KB per CU per launch -- and LDS holds activations only;
//   * the haloed activation slabs go through per-wave LDS-DMA rings issued by the waves themselves (inline asm: hipcc would drain
//     every counted load before the first LDS read that follows a DMA it knows of);
//   * after the last step the partial tiles of the K slices meet through LDS, which leaves wave w with the complete rows of channel
//     block w for the LayerNorm epilogues (forward LayerNorm: dx_conv1d_ln; backward: dx_conv1d_lnbwd), the row-wise code of
//     conv_gemm_kernel run by one 256-thread team.
// The padding rows of the batch (an equal share per workgroup, as in the ring kernel) are zero-filled after the epilogue.
// (Rounds 3-5 split the contraction two ways x two channel halves over ONE shared activation ring with a workgroup barrier per
//  32-channel chunk: 36 % matrix-pipe issue inside its compute phase, 620 cycles of hand-over per chunk; same-box A/B against the
//  loop below: 6.39 -> 6.27 ms per training step, DESIGN 5.  That loop, the main-loop ablation switches and an LDS-staged store of
//  the second GEMM's rows (53.9 vs 51.1 us) were deleted after their measurements.)
constexpr int SK_THREADS = 256;
constexpr int SK4_MAXNA = 6, SK4_S = 3, SK4_NPMAX = (SK4_MAXNA * 32 + 2 + 15) / 16, SK4_WAVE_EL = SK4_S * SK4_NPMAX * 512;
template <int N>
__device__ __forceinline__ void sk_wait_vmcnt_c() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <int LNM>
__global__ __launch_bounds__(SK_THREADS, 1) void conv_sk_kernel(ConvArgs p) {
  typedef bf16_t TC;
  typedef bf16x8 frag_t;
  constexpr int LN = LNM == 3 ? 2 : LNM;
  constexpr bool LNFILM = LNM == 2;
  constexpr int TAPS = 3, HALO = 1, STG_LD = BN + 4, STG_BYTES = 64 * STG_LD * 4;
  constexpr int MAXBLK = SK4_MAXNA;
  constexpr int RING_BYTES = 4 * SK4_WAVE_EL * 2, XCH_BYTES = 24 * 4096;
  constexpr int SMEM_BYTES = RING_BYTES > XCH_BYTES ? (RING_BYTES > STG_BYTES ? RING_BYTES : STG_BYTES) : (XCH_BYTES > STG_BYTES ? XCH_BYTES : STG_BYTES);
  __shared__ __attribute__((aligned(16))) char smem[SMEM_BYTES];
  TC* ring = reinterpret_cast<TC*>(smem);
  float* stage = reinterpret_cast<float*>(smem);
  float* xch = reinterpret_cast<float*>(smem);
  auto lds_at = [](int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 2) & 3)) << 3); };
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wk = wave & 1, wc = wave >> 1;
  const int4 e = reinterpret_cast<const int4*>(p.plan)[blockIdx.x];
  const int b = e.x, n0_tile = e.y, h_tile = e.z, fill_per = e.w;
  const int N = p.N, Cin = p.Cin;
  const int len = p.mask_len ? (int)p.mask_len[b] : N;
  // a tile taller than the accumulators of the main loop hold (SK4_MAXNA = 6 row blocks = 192 rows) is two workgroups' work:
  // blockIdx.y = 0 takes 128 rows, blockIdx.y = 1 the rows from 128 on (and exits at once for every other tile); the grid is
  // (tiles, 2) when N > 192
  const bool tall = h_tile > 32 * SK4_MAXNA;
  if (blockIdx.y && !tall) return;
  const int n0 = n0_tile + (int)blockIdx.y * 128, h = tall ? (blockIdx.y ? h_tile - 128 : 128) : h_tile;
  if (h > 0) {
    const TC* X = reinterpret_cast<const TC*>(p.x) + (size_t)b * N * p.ldx;
    const int nk = Cin >> 5;
    // ---- main loop (round 6).  The contraction (Cin x 3 taps) is split KS ways inside the workgroup, by the number NA of live 32-row
    // blocks of the tile (the dispatch below the lambda):
    //     NA 1..4 (<= 128 rows)    KS = 4: wave w takes the 32-channel chunks 4 s + w (s = "step") with all three taps, for ALL rows
    //                              and ALL 128 output channels: <= 4 x 4 MFMA tiles = 256 accumulator registers
    //     NA 5..6 (129..192 rows)  KS = 2: wave w takes the chunks 2 s + (w & 1) for all rows and the 64 channels of group w >> 1:
    //                              <= 6 x 2 MFMA tiles = 192 accumulator registers
    //     more than 192 rows       two workgroups (blockIdx.y, above), each with NA <= 4
    // Nothing is shared between the waves until the end:
    //   * the activation slab of a wave's chunk (<= 194 rows x 32 channels, 13 KiB) goes through the wave's OWN 3-stage LDS-DMA
    //     ring -- there is no workgroup barrier in the loop, only the wave's own vmcnt waits (hand-counted below);
    //   * the weight fragments (fragment order, dx_pack_frag_major: the four channel blocks of one (chunk, tap, k half) are 4 KiB
    //     contiguous) come from L2 straight into registers, every fragment read by exactly ONE wave: 786 KB per workgroup as before;
    //   * per (tap, k half) "sub-step" a wave reads NA activation fragments from LDS for KS NA MFMAs (KS = 4: 0.25 KB of LDS per
    //     MFMA; KS = 2 and the rounds 3-5 loop: 0.5), the fragments of the next sub-step are requested before the MFMAs of this one;
    //   * after the last step the KS partial tiles of every (row block, channel block) meet through LDS, two row blocks per pass;
    //     local channel block j of a wave is block j ^ (its K slice) of its channel group, so that local 0 is the one the wave keeps
    //     (static register indices) and the sum runs in the fixed order own + (w ^ 1) [+ (w ^ 2) + (w ^ 3)]: results stay run-to-run
    //     reproducible.
    // Why: one wave per SIMD in lock step with three others (the rounds 3-5 loop: a workgroup barrier per chunk) exposes every latency.
    // Tiles of 129..160 rows (the balanced plan of a B = 48 batch: H = 124..135) also ran that loop's 8-block code path: 48 MFMAs per chunk for 30.
    f32x16 fin[SK4_MAXNA];
    {
      const int nblk = __builtin_amdgcn_readfirstlane((h + 31) >> 5);     // live 32-row blocks, 1 .. 6
      const unsigned ring_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem) +
                                 (unsigned)(wave * SK4_WAVE_EL * 2);
      const TC* ringw = ring + wave * SK4_WAVE_EL;
      // LDS-DMA pieces: 16 rows x 64 B; lane -> row lane >> 2, slot lane & 3, which holds source chunk slot ^ ((row >> 2) & 3) (lds_at;
      // (row >> 2) & 3 == (lane >> 4) & 3 for every piece).  Rows outside the utterance or past the halo read the zero page.
      const int lr = lane >> 2, csrc = (lane & 3) ^ ((lane >> 4) & 3);
      const TC* zp = reinterpret_cast<const TC*>(dx_zero_page);
      asm volatile("" : "+s"(zp));                                        // (an SGPR pair, not a GOT load per piece)
      const int rowoff0 = (n0 - HALO + lr) * (int)p.ldx + csrc * 8, ld16 = 16 * (int)p.ldx;   // elements from X; < 2^31 (plan_check: B * N * ldx)
      const int rlo = n0 == 0 ? 1 : 0, rhi = min(h + TAPS - 1, N - n0 + HALO);
      const TC* wl = reinterpret_cast<const TC*>(p.w_frag) + lane * 8;
      auto mainloop = [&](auto na_tag, auto ks_tag) {
        // KS K slices x (4 / KS) channel groups: wave = wk + KS wc takes the chunks KS s + wk and the channel blocks NCB wc + (j ^ wk),
        // j = 0 .. NCB - 1 (NCB = KS): local block 0 is global block `wave`, the one the wave keeps after the exchange
        constexpr int NA = decltype(na_tag)::value, KS = decltype(ks_tag)::value, NCB = KS;
        constexpr int NP = (NA * 32 + TAPS - 1 + 15) / 16, STAGE_EL = NP * 512;
        constexpr int RQ = NA * NCB >= 10 ? 3 : 6;                         // weight-fragment ring, in sub-steps (6 per step)
        auto dist = [](int q) constexpr { return (NP + 5 - q) / 6; };      // pieces issued in sub-step q
        auto first = [](int q) constexpr { int f = 0; for (int i = 0; i < q; ++i) f += (NP + 5 - i) / 6; return f; };
        constexpr int QL = NP >= 6 ? 5 : NP - 1;                           // last sub-step that issues a piece
        constexpr int P5 = NP - NP / 6;                                    // pieces issued before sub-step 5
        static_assert(3 * STAGE_EL <= SK4_WAVE_EL, "ring stage");
        const int skw = wave % KS, scw = wave / KS;
        const int ns = nk / KS;                                             // steps (launcher: Cin % 128 == 0, Cin >= 256)
        // every workgroup walks the steps in its own rotation: workgroup L runs on XCD L % 8, and the 32 workgroups of an XCD start within a
        // microsecond of each other -- in the same order they would all ask the XCD's L2 for the same weight lines at the same time (one channel
        // serves them one after the other: measured 30 GB/s per CU of L2 hits, a quarter of what the L2 delivers to CUs that read different
        // lines).  The fp32 sums of different tiles then run in different step orders (each still fixed, so results stay reproducible)
        const int soff = (int)((blockIdx.x >> 3) % (unsigned)ns);
        auto kc_of = [&](int s) { int t = s + soff; if (t >= ns) t -= ns; return KS * t + skw; };
        const int jx = skw * 512, jb = scw * NCB * 512;
        f32x16 acc[NA][NCB];
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
          for (int j = 0; j < NCB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        frag_t bq[RQ][NCB], a[2][NA];
        auto piece = [&](int t, int kc, int stg) {
          // (laundered: as loop invariants hipcc keeps 2 NP hoisted pointers in registers -- and spills them; re-deriving one costs ~8 VALU)
          int lrv = lr, ro = rowoff0;
          asm volatile("" : "+v"(lrv), "+v"(ro));
          const int r = t * 16 + lrv;
          const bool ok = (unsigned)(r - rlo) < (unsigned)(rhi - rlo);
          const TC* sp = (ok ? X : zp) + ((ok ? ro + t * ld16 : csrc * 8) + kc * 32);
          sk_dma16(sp, __builtin_amdgcn_readfirstlane(ring_base + (unsigned)((stg * STAGE_EL + t * 512) * 2)));
        };
        auto load_b = [&](int kc, int q, frag_t* d) {
          const TC* wq = wl + (size_t)kc * 12288 + q * 2048 + jb;
#pragma unroll
          for (int j = 0; j < NCB; ++j) d[j] = *reinterpret_cast<const frag_t*>(wq + ((j * 512) ^ jx));
        };
        auto read_a = [&](const TC* Ar, int q, frag_t* d) {
          const int tap = q >> 1, half = q & 1;
#pragma unroll
          for (int i = 0; i < NA; ++i) d[i] = *reinterpret_cast<const frag_t*>(&Ar[lds_at(i * 32 + l31 + tap, half * 2 + g)]);
        };
        // prologue: the slabs of steps 0 and 1, the fragments of the first RQ sub-steps, then the first activation fragments
#pragma unroll
        for (int t = 0; t < NP; ++t) piece(t, kc_of(0), 0);
#pragma unroll
        for (int t = 0; t < NP; ++t) piece(t, kc_of(1), 1);
#pragma unroll
        for (int q = 0; q < RQ; ++q) load_b(kc_of(0), q, bq[q]);
        sk_wait_vmcnt_c<NP + NCB * RQ>();                                  // behind the slab of step 0: the slab of step 1, NCB RQ fragments
        read_a(ringw, 0, a[0]);
        int stg = 0;                                                        // ring stage of step s
        for (int s = 0; s < ns; ++s) {
          const int stg1 = stg + 1 == SK4_S ? 0 : stg + 1, stg2 = stg1 + 1 == SK4_S ? 0 : stg1 + 1;
          const bool dma = s + 2 < ns, more = s + 1 < ns;
          const int kc0 = kc_of(s), kc1 = kc_of(more ? s + 1 : s), kc2 = dma ? kc_of(s + 2) : 0;
          const TC* Ar = ringw + stg * STAGE_EL;
          const TC* An = ringw + stg1 * STAGE_EL;
          auto sub = [&](auto q_tag) {
            constexpr int Q = decltype(q_tag)::value, SL = Q % RQ;
            if (Q < 5) read_a(Ar, Q + 1, a[(Q + 1) & 1]);
            else if (more) {
              // the slab of step s + 1 must have landed.  Behind its last piece in this wave's queue: the fragment loads of the rest
              // of that step (s >= 1: NCB (6 - QL); s == 0: the prologue's NCB RQ), and of this step's sub-steps 0..4 (5 NCB) with
              // the pieces issued beside them (P5, when step s + 2 exists).  hipcc does not see the pieces: its own waits are early.
              if (s == 0) { if (dma) sk_wait_vmcnt_c<NCB * RQ + 5 * NCB + P5>(); else sk_wait_vmcnt_c<NCB * RQ + 5 * NCB>(); }
              else { if (dma) sk_wait_vmcnt_c<NCB * (6 - QL) + 5 * NCB + P5>(); else sk_wait_vmcnt_c<NCB * (6 - QL) + 5 * NCB>(); }
              read_a(An, 0, a[0]);
            }
            __builtin_amdgcn_sched_barrier(0);
            constexpr int HALF = NA / 2;
#pragma unroll
            for (int i = 0; i < HALF; ++i)
#pragma unroll
              for (int j = 0; j < NCB; ++j) dx_mma(acc[i][j], a[Q & 1][i], bq[SL][j]);
            __builtin_amdgcn_sched_barrier(0);
            if (dma) {
#pragma unroll
              for (int t = first(Q); t < first(Q) + dist(Q); ++t) piece(t, kc2, stg2);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = HALF; i < NA; ++i)
#pragma unroll
              for (int j = 0; j < NCB; ++j) dx_mma(acc[i][j], a[Q & 1][i], bq[SL][j]);
            __builtin_amdgcn_sched_barrier(0);
            // refill the slots just read with sub-step Q + RQ (UNCONDITIONAL: past the end it re-reads -- a load that may not execute
            // makes hipcc assume the worst at every use: with a condition around them it drained the whole queue, vmcnt(0), in front of the
            // first MFMA that follows)
            load_b(Q + RQ < 6 ? kc0 : kc1, (Q + RQ) % 6, bq[SL]);
          };
          sub(std::integral_constant<int, 0>{});
          sub(std::integral_constant<int, 1>{});
          sub(std::integral_constant<int, 2>{});
          sub(std::integral_constant<int, 3>{});
          sub(std::integral_constant<int, 4>{});
          sub(std::integral_constant<int, 5>{});
          stg = stg1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                 // every wave is done with its ring: the exchange buffer reuses it
        // ---- the K slices meet, two row blocks per pass: slot ((wave (KS - 1) + j - 1) * 2 + rbl) of 4 KiB = [register quad][lane][4];
        // fixed order own + (wk ^ 1) [+ (wk ^ 2) + (wk ^ 3)]: results stay run-to-run reproducible
#pragma unroll
        for (int pp = 0; pp < (NA + 1) / 2; ++pp) {
#pragma unroll
          for (int rbl = 0; rbl < 2; ++rbl)
            if (2 * pp + rbl < NA) {
#pragma unroll
              for (int j = 1; j < KS; ++j)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                  const f32x16& t = acc[2 * pp + rbl][j];
                  *reinterpret_cast<f32x4*>(xch + ((((wave * (KS - 1) + j - 1) * 2 + rbl) * 4 + r4) * 64 + lane) * 4) =
                      f32x4{t[4 * r4], t[4 * r4 + 1], t[4 * r4 + 2], t[4 * r4 + 3]};
                }
            }
          __syncthreads();
#pragma unroll
          for (int rbl = 0; rbl < 2; ++rbl)
            if (2 * pp + rbl < NA) {
              f32x16 t = acc[2 * pp + rbl][0];
#pragma unroll
              for (int d = 1; d < KS; ++d)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                  const f32x4 v = *reinterpret_cast<const f32x4*>(xch + (((((wave ^ d) * (KS - 1) + d - 1) * 2 + rbl) * 4 + r4) * 64 + lane) * 4);
#pragma unroll
                  for (int e2 = 0; e2 < 4; ++e2) t[4 * r4 + e2] += v[e2];
                }
              fin[2 * pp + rbl] = t;
            }
          __syncthreads();
        }
#pragma unroll
        for (int i = NA; i < SK4_MAXNA; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) fin[i][r] = 0.f;
      };
      constexpr std::integral_constant<int, 4> K4{};
      constexpr std::integral_constant<int, 2> K2{};
      if (nblk > 5) mainloop(std::integral_constant<int, 6>{}, K2);
      else if (nblk == 5) mainloop(std::integral_constant<int, 5>{}, K2);
      else if (nblk == 4) mainloop(std::integral_constant<int, 4>{}, K4);
      else if (nblk == 3) mainloop(std::integral_constant<int, 3>{}, K4);
      else if (nblk == 2) mainloop(std::integral_constant<int, 2>{}, K4);
      else mainloop(std::integral_constant<int, 1>{}, K4);
    }
#define DX_SK_FIN(i) fin[i]
    // ---- LayerNorm epilogue (the PLAN epilogue of conv_gemm_kernel with one 256-thread team)
    constexpr int NCS = LNM == 2 ? 4 : (LNM == 3 ? 2 : 1);
    float csum[NCS][8];
#pragma unroll
    for (int q = 0; q < NCS; ++q)
#pragma unroll
      for (int e2 = 0; e2 < 8; ++e2) csum[q][e2] = 0.f;
    const int cb = 2 * wc + wk;                        // == wave: the channel block whose complete rows this wave holds
    const float bv = p.bias ? p.bias[cb * 32 + l31] : 0.f;
    // second GEMM of the backward variant (LayerNorm backward -> output-projection data gradient, model.py:182-186): the rows this
    // epilogue writes as y_lp are the operand of a 128 -> 128 k = 1 GEMM that used to be the next launch (18 us for 3 us of work).
    // Weights as the A operand (wave = 32 output channels, its 8 fragments in registers), the 64 freshly written rows as B from an
    // LDS image beside the staging buffer: D[channel][row], a lane owns one row and 4 x 4 consecutive channels (8-byte stores).
    // The forward variant does the same with the NEXT block's QKV projection (128 -> 384, model.py:165-171): three channel blocks per
    // wave, bias added in the store.
    constexpr int A2_LD = BN + 8, A2_OFF = 64 * 1024, NC2 = LN == 2 ? 1 : 3;
    static_assert(A2_OFF >= STG_BYTES && A2_OFF + 64 * A2_LD * 2 <= SMEM_BYTES, "second-GEMM operand tile must fit beside the staging buffer");
    const bool gemm2 = p.ln.y2 != nullptr;
    const int n2 = p.ln.n2, ncb2 = __builtin_amdgcn_readfirstlane(n2 >> 7);      // channel blocks per wave (1 or 3)
    TC* a2 = reinterpret_cast<TC*>(smem + A2_OFF);
    frag_t w2f[NC2][8];
    if (gemm2) {
#pragma unroll
      for (int c = 0; c < NC2; ++c)
        if (c < ncb2) {
          const TC* w2 = reinterpret_cast<const TC*>(p.ln.w2) + (size_t)((c * 4 + wave) * 32 + l31) * BN + g * 8;
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) w2f[c][ks] = *reinterpret_cast<const frag_t*>(w2 + ks * 16);
        }
    }
    // the per-channel operands of the row passes depend on (b, channel segment) only: loaded ONCE here.  Inside the passes they sat
    // behind the stores of the pass before (the compiler cannot prove that y / s_out do not alias gamma / beta / film), one exposed
    // L2 round trip per pass and slab
    const int cl_h = (tid & 15) * 8;
    const f32x8 gm_h = raw_load8<float>(p.ln.gamma + cl_h);
    f32x8 bt_h = gm_h, fg_h = gm_h, fb_h = gm_h;
    if (LN == 1 || LNFILM) bt_h = raw_load8<float>(p.ln.beta + cl_h);
    if (p.ln.film && (LN == 1 || LNFILM)) fg_h = raw_load8<float>(p.ln.film + (size_t)b * p.ln.ldf + cl_h);
    if (p.ln.film && LN == 1) fb_h = raw_load8<float>(p.ln.film + (size_t)b * p.ln.ldf + BN + cl_h);
    const bool vres = LN == 1 && p.ln.res_mean != nullptr;
    f32x8 rg_h = gm_h, rb_h = gm_h;
    if (vres) { rg_h = raw_load8<float>(p.ln.res_gamma + cl_h); rb_h = raw_load8<float>(p.ln.res_beta + cl_h); }
#pragma unroll
    for (int i = 0; i < (MAXBLK + 1) / 2; ++i) {
      if (i * 64 >= h) break;                          // workgroup-uniform: the barriers below stay matched
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
        if (2 * i + rb < MAXBLK) {
#pragma unroll
          for (int r = 0; r < 16; ++r) stage[(rb * 32 + dx_acc_row(r, g)) * STG_LD + cb * 32 + l31] = DX_SK_FIN(2 * i + rb)[r] + bv;
        }
      f32x8 pf_a[4], pf_b[4];
      float pf_m[4], pf_r[4];
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {           // the global inputs of all four passes are requested before the barrier
        const int sr = (tid >> 4) + pass * 16, trow = i * 64 + sr;
        const int n = n0 + trow, cl = (tid & 15) * 8;
        if (n < N && trow < h) {
          const size_t rowg = (size_t)b * N + n, offl = rowg * BN + cl;
          if (LN == 2) {
            pf_a[pass] = raw_load8<float>(p.ln.y + offl);
            pf_b[pass] = raw_load8<float>(p.ln.s_out + offl);
            pf_m[pass] = p.ln.mean[rowg];
            pf_r[pass] = p.ln.rstd[rowg];
          } else {
            pf_a[pass] = raw_load8<float>(p.ln.residual + offl);
            if (vres) { pf_m[pass] = p.ln.res_mean[rowg]; pf_r[pass] = p.ln.res_rstd[rowg]; }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int sr = (tid >> 4) + pass * 16, trow = i * 64 + sr;
        const int n = n0 + trow, cl = (tid & 15) * 8;
        if (n < N && trow < h) {
          float v[8];
          const f32x4 lo = *reinterpret_cast<const f32x4*>(&stage[sr * STG_LD + cl]);
          const f32x4 hi = *reinterpret_cast<const f32x4*>(&stage[sr * STG_LD + cl + 4]);
          v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
          const size_t rowg = (size_t)b * N + n, offl = rowg * BN + cl;
          if (LN == 2) {        // fused LayerNorm BACKWARD: v + residual gradient = dL/d(LN output) of this row
            {
              const f32x8 r = pf_a[pass];
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] = n < len ? v[e2] + r[e2] : 0.f;     // masked_fill rows carry no gradient
            }
            const f32x8 sv = pf_b[pass];
            const float mean = pf_m[pass], rstd = pf_r[pass];
            const f32x8 gm = gm_h;
            float xh[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) xh[e2] = (sv[e2] - mean) * rstd;
            if (LNFILM) {                                         // y = fg * LN + fb
              const f32x8 fg = fg_h, bt = bt_h;
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) {
                csum[LNFILM ? 2 : 0][e2] += v[e2] * (xh[e2] * gm[e2] + bt[e2]);
                csum[LNFILM ? 3 : 0][e2] += v[e2];
                v[e2] *= fg[e2];
              }
            }
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) {
              csum[0][e2] += v[e2] * xh[e2];
              csum[NCS > 1 ? 1 : 0][e2] += v[e2];
              v[e2] *= gm[e2];
              s1 += v[e2];
              s2 += v[e2] * xh[e2];
            }
            s1 = dx_row16_sum(s1); s2 = dx_row16_sum(s2);
            s1 *= 1.f / BN; s2 *= 1.f / BN;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) v[e2] = rstd * (v[e2] - s1 - xh[e2] * s2);
            store8<float>(p.ln.y + offl, v);                      // ds, in place of the residual gradient
            if (p.ln.p_pre > 0.f) {
              const uint32_t th = dx_drop_th8(p.ln.p_pre), key = dx_key32(dx_seed_eff(p.ln.seed_pre, p.ln.step), 0);
              const float sc = dx_drop_inv_keep8(th);
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] = dx_keep_elem(key, (uint32_t)rowg * BN + cl + e2, th) ? v[e2] * sc : 0.f;
            }
            store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + offl, v);
            if (gemm2) store8<bf16_t>(a2 + sr * A2_LD + cl, v);
          } else {              // fused LayerNorm: 16 lanes hold one complete 128-channel row
            if (p.ln.p_pre > 0.f) {
              const uint32_t th = dx_drop_th8(p.ln.p_pre), key = dx_key32(dx_seed_eff(p.ln.seed_pre, p.ln.step), 0);
              const float sc = dx_drop_inv_keep8(th);
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] = dx_keep_elem(key, (uint32_t)rowg * BN + cl + e2, th) ? v[e2] * sc : 0.f;
            }
            {
              f32x8 r = pf_a[pass];
              if (vres) {   // the residual stream = mask(LayerNorm(s)) of the launch that produced s: same expression as its epilogue
                const float rm = pf_m[pass], rr = pf_r[pass];
#pragma unroll
                for (int e2 = 0; e2 < 8; ++e2) r[e2] = n < len ? (r[e2] - rm) * rr * rg_h[e2] + rb_h[e2] : 0.f;
              }
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] += r[e2];
            }
            if (p.ln.s_out) store8<float>(p.ln.s_out + offl, v);
            float sum = 0.f;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) sum += v[e2];
            sum = dx_row16_sum(sum);
            const float mean = sum * (1.f / BN);
            float sq = 0.f;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) { const float d = v[e2] - mean; sq += d * d; }
            sq = dx_row16_sum(sq);
            const float rstd = rsqrtf(sq * (1.f / BN) + 1e-5f);
            if (p.ln.mean && cl == 0) { p.ln.mean[rowg] = mean; p.ln.rstd[rowg] = rstd; }
            const f32x8 gm = gm_h, bt = bt_h;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) v[e2] = (v[e2] - mean) * rstd * gm[e2] + bt[e2];
            if (p.ln.film) {
              const f32x8 fg = fg_h, fb = fb_h;
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] = fg[e2] * v[e2] + fb[e2];
            }
            if (n >= len) {
#pragma unroll
              for (int e2 = 0; e2 < 8; ++e2) v[e2] = 0.f;
            }
            if (p.ln.y) store8<float>(p.ln.y + offl, v);
            if (p.ln.y_lp) store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + offl, v);
            if (gemm2) store8<bf16_t>(a2 + sr * A2_LD + cl, v);
          }
        } else if (gemm2) {                            // rows outside the tile / the tensor: zeros in the operand image
          const float z8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          store8<bf16_t>(a2 + sr * A2_LD + cl, z8);
        }
      }
      __syncthreads();
      if (gemm2) {   // (the next iteration writes the image only behind its own barrier, i.e. after every wave has read it)
        // all (channel block, row block) products of the slab at once: 2 NC2 independent accumulators, every operand fragment of the
        // slab read from LDS ONCE (round 5 ran them one after the other: 8 dependent MFMAs per tile, the fragments re-read per channel block)
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        f32x16 d2[NC2][2];
#pragma unroll
        for (int c = 0; c < NC2; ++c)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) d2[c][rb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          const frag_t x0 = *reinterpret_cast<const frag_t*>(a2 + l31 * A2_LD + ks * 16 + g * 8);
          const frag_t x1 = *reinterpret_cast<const frag_t*>(a2 + (32 + l31) * A2_LD + ks * 16 + g * 8);
#pragma unroll
          for (int c = 0; c < NC2; ++c)
            if (c < ncb2) {
              dx_mma(d2[c][0], w2f[c][ks], x0);
              dx_mma(d2[c][1], w2f[c][ks], x1);
            }
        }
#pragma unroll
        for (int c = 0; c < NC2; ++c) {
          if (c >= ncb2) break;
          const int cw = (c * 4 + wave) * 32;                     // this wave's 32 output channels of channel group c
          f32x4 bj4[4];                                           // bias of the lane's channels cw + 4 g + 8 j + 0..3 (MFMA layout)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            bj4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p.ln.b2) bj4[j] = *reinterpret_cast<const f32x4*>(p.ln.b2 + cw + 4 * g + 8 * j);
          }
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
            // bf16 pairs, then two v_permlane32_swap per 16 channels (conv_wreg_kernel's epilogue): the lane ends up with channels
            // cw + 8 g + 0..7 and cw + 16 + 8 g + 0..7 of its row -- two 16-byte stores instead of four 8-byte ones
            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            uint32_t P[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const bf16x2 pr = {(bf16_t)(d2[c][rb][2 * k] + bj4[k >> 1][(2 * k) & 3]), (bf16_t)(d2[c][rb][2 * k + 1] + bj4[k >> 1][(2 * k + 1) & 3])};
              P[k] = __builtin_bit_cast(uint32_t, pr);
            }
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
              for (int k = 0; k < 2; ++k) {
                const u32x2 sw = __builtin_amdgcn_permlane32_swap(P[4 * h2 + k], P[4 * h2 + 2 + k], false, false);
                P[4 * h2 + k] = sw[0];
                P[4 * h2 + 2 + k] = sw[1];
              }
            // (through an LDS image of the slab, whole rows per store instruction: measured 53.9 vs 51.1 us -- the 8 us the QKV rows cost are
            //  their 23 MB in a write-bound epilogue, not the shape of the store instructions)
            const int trow = i * 64 + rb * 32 + l31, n = n0 + trow;
            if (trow < h && n < N) {
              TC* yo = reinterpret_cast<TC*>(p.ln.y2) + ((size_t)b * N + n) * n2 + cw + 8 * g;
              *reinterpret_cast<u32x4*>(yo) = u32x4{P[0], P[1], P[2], P[3]};
              *reinterpret_cast<u32x4*>(yo + 16) = u32x4{P[4], P[5], P[6], P[7]};
            }
          }
        }
      }
    }
    if (LN == 2) {   // column sums: 16 row-threads per channel segment -> LDS -> one atomic per channel per workgroup
      for (int q = 0; q < NCS; ++q)
#pragma unroll
        for (int e2 = 0; e2 < 8; ++e2) stage[(q * 16 + (tid >> 4)) * BN + (tid & 15) * 8 + e2] = csum[q][e2];
      __syncthreads();
      for (int idx = tid; idx < NCS * BN; idx += SK_THREADS) {
        const int q = idx / BN, c = idx - q * BN;
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += stage[(q * 16 + r) * BN + c];
        if (q == 0) atomicAdd(p.ln.dgamma + c, t);
        else if (q == 1) atomicAdd(p.ln.dbeta + c, t);
        else atomicAdd(p.ln.dfilm + (size_t)b * p.ln.lddf + (q == 3 ? BN : 0) + c, t);
      }
    }
  }
#undef DX_SK_FIN
  // ---- padding fill: the batch's padding rows, flattened utterance by utterance, are split evenly over the workgroups; this one
  // owns [lo, hi).  Each wave finds the utterances its range touches with a wave scan over the lengths, and the 256 threads share
  // the 16-byte segments of those rows.
  if (blockIdx.y == 0) {
    const long lo = (long)blockIdx.x * fill_per, hi = lo + fill_per;
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
        int cntr = __shfl((int)(fe - fs), src_lane, 64);
        cntr = min(cntr, dx_fill_end((int)p.skip_len[fb], N) - first);   // dead rows past the fill end stay unwritten (dx_common.h)
        float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p.ln.y2) {                                   // rows of the second GEMM's output (n2 channels, bf16)
          const int segs = p.ln.n2 >> 3;
          for (int c = tid; c < cntr * segs; c += SK_THREADS) {
            const int n = first + c / segs, cl = (c % segs) * 8;
            store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y2) + ((size_t)fb * N + n) * p.ln.n2 + cl, z);
          }
        }
        for (int c = tid; c < cntr * (BN / 8); c += SK_THREADS) {
          const int n = first + (c >> 4), cl = (c & 15) * 8;
          const size_t off = ((size_t)fb * N + n) * BN + cl;
          if (LN == 2 || p.ln.y) store8<float>(p.ln.y + off, z);
          if (LN == 2 || p.ln.y_lp) store8<bf16_t>(reinterpret_cast<bf16_t*>(p.ln.y_lp) + off, z);
          if (LN == 1) {
            if (p.ln.s_out) store8<float>(p.ln.s_out + off, z);
            if (p.ln.mean && cl == 0) { p.ln.mean[(size_t)fb * N + n] = 0.f; p.ln.rstd[(size_t)fb * N + n] = 0.f; }
          }
        }
      }
      carry += __shfl(incl, 63, 64);
    }
  }
}

}  // namespace

int conv_sk_launch(const ConvArgs& a, hipStream_t s) {
  // tiles of more than 192 rows (possible when N > 192) are split between blockIdx.y = 0 and 1
  const dim3 grid((unsigned)a.plan_tiles, a.N > 32 * SK4_MAXNA ? 2u : 1u), block(SK_THREADS);
  if (a.ln.enabled == 1) hipLaunchKernelGGL(conv_sk_kernel<1>, grid, block, 0, s, a);
  else if (a.ln.film) hipLaunchKernelGGL(conv_sk_kernel<2>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(conv_sk_kernel<3>, grid, block, 0, s, a);   // backward without FiLM gradients: fewer registers
  DX_LAUNCH_CHECK();
  return DX_OK;
}
