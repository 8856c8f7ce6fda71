// conv_wide_kernel: the wide k = 3 conv GEMM on 256 x 256 tiles, and its launcher.
#include <type_traits>

#include "conv_args.h"

namespace {

#include "conv_common.h"

// ---- wide k = 3 GEMM (Cout a multiple of 256, long contraction: the pre-net's 1024 -> 1024 conv and its data gradient) on the
// full register file: 256 rows x 256 channels per 4-wave workgroup, ONE wave per SIMD, wave (wr, wc) = 128 rows x 128 channels =
// 4 x 4 MFMA tiles = 256 accumulator registers.  Same ingredients as conv_sk_kernel: the haloed activation tile (258 rows x 32
// channels per chunk) through a 3-stage LDS-DMA ring issued by the waves themselves, the weights in fragment order
// (dx_pack_frag_major) from L2 straight into registers -- a ring of 6 k-steps = one chunk (4 fragments each, 96 registers): the
// slot a k-step has just read is refilled with the same k-step of the next chunk -- and the per-workgroup rotation of the chunk order.  Per k-step a wave
// reads 4 activation fragments from LDS for 16 MFMAs (0.25 KB of LDS per MFMA; the 128-channel tiles of conv_gemm_kernel need 0.75).
// L2 -> CU traffic per launch = 2 bytes x M N K x (1 / 256 + 1 / 256): half of what 256 x 128 tiles fetch.
// Epilogue: bias, ReLU, rows past length + 2 zeroed; a wave stages one 32-row x 128-channel slab at a time through its own LDS
// region and stores whole 256-byte row segments in bf16.
constexpr int WD_THREADS = 256, WD_S = 3, WD_RING = 6, WD_MAXP = 5;
__device__ __forceinline__ void wd_wait_vmcnt(int n) {
  switch (n) {
#define DX_VMW(n) case n: asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); break;
    DX_VMW(48) DX_VMW(49) DX_VMW(50) DX_VMW(51) DX_VMW(52) DX_VMW(53)
#undef DX_VMW
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

__global__ __launch_bounds__(WD_THREADS, 1) void conv_wide_kernel(ConvArgs p) {
  typedef bf16_t TC;
  typedef bf16x8 frag_t;
  constexpr int TAPS = 3, HALO = 1, BMW = 256, AROWS = BMW + TAPS - 1, AR16 = (AROWS + 15) & ~15, STAGE_EL = AR16 * 32;
  constexpr int SLAB_LD = 128 + 4;
  constexpr int RING_BYTES = WD_S * STAGE_EL * 2, SLAB_BYTES = 4 * 32 * SLAB_LD * 4;
  __shared__ __attribute__((aligned(16))) char smem[RING_BYTES > SLAB_BYTES ? RING_BYTES : SLAB_BYTES];
  TC* ring = reinterpret_cast<TC*>(smem);
  auto lds_at = [](int row, int chunk) { return row * 32 + ((chunk ^ ((row >> 2) & 3)) << 3); };
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, g = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave >> 1, wc = wave & 1;
  const int N = p.N, Cin = p.Cin, Cout = p.Cout;
  // position tiles of the batch from dx_conv_tile_plan (rows < length + halo of every utterance, cut into equal pieces of <= 256 rows such
  // that the tile count is a multiple of 64 = 256 CUs / 4 channel tiles); channel tile slowest: consecutive workgroups (one per XCD in
  // turn) share a channel tile, so an XCD's L2 holds one 1.5 MB weight slice at a time
  const int pt = blockIdx.x % p.plan_tiles, ct = blockIdx.x / p.plan_tiles;
  const int4 e = reinterpret_cast<const int4*>(p.plan)[pt];
  const int b = e.x, n0 = e.y, h = e.z, fill_per = e.w;
  const int co_w = ct * 256 + wc * 128;                              // first channel of this wave
  TC* Y = reinterpret_cast<TC*>(p.y);
  if (h > 0) {
  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.f;
  const TC* X = reinterpret_cast<const TC*>(p.x) + (size_t)b * N * p.ldx;
  const int nk = Cin >> 5;
  const int nA = (h + TAPS - 1 + 15) >> 4;
  const int mine = __builtin_amdgcn_readfirstlane(nA > wave ? (nA - wave + 3) >> 2 : 0);
  const TC* src[WD_MAXP];
  unsigned dst[WD_MAXP];
#pragma unroll
  for (int t = 0; t < WD_MAXP; ++t) {
    const int q = wave + 4 * t;
    const int r = q * 16 + (lane >> 2);
    const int c = (lane & 3) ^ ((r >> 2) & 3);
    const int n = n0 + r - HALO;
    const TC* sp = reinterpret_cast<const TC*>(dx_zero_page) + c * 8;
    if (q < nA && r < h + TAPS - 1 && n >= 0 && n < N) sp = X + (long)n * p.ldx + c * 8;
    src[t] = sp;
    dst[t] = (unsigned)(q * 512 * 2);
  }
  const unsigned ring_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem);
  auto issue_dma = [&](int kc, int buf) {
#pragma unroll
    for (int t = 0; t < WD_MAXP; ++t)
      if (t < mine) sk_dma16(src[t] + kc * 32, __builtin_amdgcn_readfirstlane(ring_base + (unsigned)(buf * STAGE_EL * 2) + dst[t]));
  };
  // rotation of the chunk order (see conv_sk_kernel) by POSITION tile only: the channel tiles of one position tile run on the same
  // XCD (plan_tiles % 8 == 0) at the same time and read the same activation chunks -- in the same chunk order the first one
  // pulls a chunk into the XCD's L2 and the others hit it (with the rotation keyed on blockIdx they walked the chunks 8 apart and
  // each fetched the activation tile for itself: FETCH_SIZE 188 MB per launch for 61 MB of activations)
  const int koff = (int)((pt >> 3) % (unsigned)nk);
  auto kc_of = [&](int it) { const int k = it + koff; return k >= nk ? k - nk : k; };
  // fragment (k-step q = chunk * 6 + tap * 2 + half, channel block c) at q * (Cout / 32) * 512 + c * 512 elements
  const size_t qstride = (size_t)(Cout >> 5) * 512;
  const TC* wp = reinterpret_cast<const TC*>(p.w_frag) + (size_t)(co_w >> 5) * 512 + lane * 8;
  frag_t bq[WD_RING][4];
  auto load_b = [&](int it, int ks6, frag_t* d) {   // k-step ks6 of chunk `it` (in this workgroup's rotation; past the end: the last chunk again)
    const TC* base = wp + (size_t)(kc_of(it < nk ? it : nk - 1) * 6 + ks6) * qstride;
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = *reinterpret_cast<const frag_t*>(base + c * 512);
  };
  // 32-row blocks interleaved over the two wave rows (block 2 i + wr is wave row wr's i-th), so that a tile of any height splits evenly
  const int nblk = (h + 31) >> 5;
  const int nact = __builtin_amdgcn_readfirstlane((nblk - wr + 1) >> 1);
  const bool counted = nk >= 8;
#pragma unroll
  for (int st = 0; st < WD_S - 1; ++st)
    if (st < nk) issue_dma(kc_of(st), st);
#pragma unroll
  for (int s0 = 0; s0 < WD_RING; ++s0) load_b(0, s0, bq[s0]);
  // per chunk a wave issues [DMA pieces of chunk it + S - 1] [24 fragment loads]: when the pieces of chunk `it` must have landed,
  // 24 (S - 1) fragment loads + the pieces of the iteration in between may be in flight: 48 + mine * min(1, nk - 1 - it) (S = 3)
  auto chunk = [&](int it, auto na_tag) {
    constexpr int NA = decltype(na_tag)::value;
    const int behind = nk - 1 - it;
    if (counted) wd_wait_vmcnt(48 + mine * (behind > 1 ? 1 : behind));
    else wd_wait_vmcnt(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (it + WD_S - 1 < nk) issue_dma(kc_of(it + WD_S - 1), (it + WD_S - 1) % WD_S);
    const TC* Ar = ring + (it % WD_S) * STAGE_EL;
    frag_t a[2][NA > 0 ? NA : 1];
    if constexpr (NA > 0) {
#pragma unroll
      for (int i = 0; i < NA; ++i) a[0][i] = *reinterpret_cast<const frag_t*>(&Ar[lds_at((2 * i + wr) * 32 + l31, g)]);
    }
#pragma unroll
    for (int ks6 = 0; ks6 < 6; ++ks6) {
      if constexpr (NA > 0) {
        if (ks6 + 1 < 6) {                           // the next k-step's activation fragments are requested before this one's MFMAs
          const int tn = (ks6 + 1) >> 1, kn = (ks6 + 1) & 1;
#pragma unroll
          for (int i = 0; i < NA; ++i) a[(ks6 + 1) & 1][i] = *reinterpret_cast<const frag_t*>(&Ar[lds_at((2 * i + wr) * 32 + l31 + tn, kn * 2 + g)]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NA; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c) dx_mma(acc[i][c], a[ks6 & 1][i], bq[ks6][c]);
        __builtin_amdgcn_sched_barrier(0);
      }
      load_b(it + 1, ks6, bq[ks6]);                  // the same k-step of the next chunk
    }
  };
  auto mainloop = [&](auto na_tag) {
    for (int it = 0; it < nk; ++it) chunk(it, na_tag);
  };
  if (nact >= 4) mainloop(std::integral_constant<int, 4>{});
  else if (nact == 3) mainloop(std::integral_constant<int, 3>{});
  else if (nact == 2) mainloop(std::integral_constant<int, 2>{});
  else if (nact == 1) mainloop(std::integral_constant<int, 1>{});
  else mainloop(std::integral_constant<int, 0>{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                   // the ring is dead: every wave stages its slabs through its own region

  const bool relu = p.flags & DX_CONV_RELU;
  float* slab = reinterpret_cast<float*>(smem) + (size_t)wave * (32 * SLAB_LD);
  float bv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) bv[c] = p.bias ? p.bias[co_w + c * 32 + l31] : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r0 = (2 * i + wr) * 32;                // first tile row of this 32-row block
    if (r0 >= h) break;                              // wave-uniform; the staging region is wave-private: no workgroup barrier
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][c][r] + bv[c];
        if (relu) v = fmaxf(v, 0.f);
        slab[dx_acc_row(r, g) * SLAB_LD + c * 32 + l31] = v;
      }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {           // 16 lanes x 16 bytes = one 256-byte row segment per store instruction
      const int row = pass * 4 + (lane >> 4), cl = (lane & 15) * 8;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(&slab[row * SLAB_LD + cl]);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(&slab[row * SLAB_LD + cl + 4]);
      if (r0 + row < h) {
        const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        store8<bf16_t>(Y + ((size_t)b * N + n0 + r0 + row) * p.ldy + co_w + cl, v);
      }
    }
    asm volatile("" ::: "memory");
  }
  }
  // ---- padding fill (rows past length + halo of every utterance: zeros), an equal share of the flattened padding rows per position tile,
  // this channel tile's 256 columns of them (see conv_sk_kernel)
  {
    const long lo = (long)pt * fill_per, hi = lo + fill_per;
    const int halo = p.flags >> 8;
    long carry = 0;
    for (int base = 0; base < p.B && carry < hi; base += 64) {
      const int ub = base + lane;
      int ulen = ub < p.B ? (int)p.skip_len[ub] : N;
      ulen = (ulen < 0 ? 0 : ulen) + halo;
      const int dead = ub < p.B ? N - (ulen > N ? N : ulen) : 0;
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
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = tid; c < cntr * 32; c += WD_THREADS)
          store8<bf16_t>(Y + ((size_t)fb * N + first + (c >> 5)) * p.ldy + ct * 256 + (c & 31) * 8, z);
      }
      carry += __shfl(incl, 63, 64);
    }
  }
}

}  // namespace

int conv_wide_launch(const ConvArgs& a, hipStream_t s) {
  dim3 grid((unsigned)(a.plan_tiles * (a.Cout / 256)));
  hipLaunchKernelGGL(conv_wide_kernel, grid, dim3(WD_THREADS), 0, s, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
