// K32: the hot path of a speaker encoder that scores whose voice a synthesis has -- attentive statistics pooling over the live steps of
// an utterance, its backward, and the score histograms of all verification trials of a set.  The contract is the K32 comment of
// include/daft_exprt_hip.h.
//
// Pooling: a row is ~500 steps by 256 channels, read twice (the mean, then the variance ABOUT it: at a channel mean of 100 and a
// deviation of 0.1 the one-pass sum w h^2 - mu^2 has no correct digit in fp32); the second read comes from L2.  One workgroup of four
// waves per (row, 64-channel block), the lanes along C, the waves splitting t with four accumulators each and combining through LDS in
// the order of the waves: the association depends on n and on the wave and lane positions alone, never on the padded extents or the
// batch.  The softmax weights of the row are computed once into LDS by every workgroup of the row (4 096 floats at most).
// The backward's g_a needs q[t], a sum over ALL channels: every channel block writes its partial q -- one dx_wave_sum per step, four in
// flight -- to the workspace, and a second launch, one workgroup per row, adds the blocks in order and forms g_a.  No atomics.
//
// Trial counts: the one kernel here with real arithmetic, E E^T over the upper triangle in 128 x 128 tiles from the exact-fp32 dx_mma.
// Four waves, each a 64 x 64 quarter (2 x 2 accumulators of 32 x 32); both operand tiles go through LDS 16 columns at a time, the next 16
// fetched into registers while the MFMAs of the current run.  Every score is binned into one of two LDS histograms with a 32-bit LDS
// atomic; a workgroup loops over its tiles and flushes its nonzero bins once with 64-bit integer global atomics.
// No 32-bit LDS count can overflow: a tile adds at most 128 x 128 = 2^14 to a bin, and ALL the tiles of the largest admitted set, N =
// 65 536 -> 512 x 513 / 2 = 131 328 tiles, are fewer than the 2^18 it would take -- even a single workgroup taking every tile stays
// below 2^32.
#include "dx_common.h"

namespace {

constexpr int SP_MAX_C = 1024;         // dx_spk_pool_max_channels()
constexpr int SP_MAX_T = 4096;         // dx_spk_pool_max_steps(): the softmax weights (and the backward's q) of a row live in LDS
constexpr int SP_WAVES = 4;
constexpr int SP_THREADS = SP_WAVES * 64;
constexpr float SP_VAR_EPS = 1e-5f;
constexpr int TC_MAX_D = 1024;         // dx_trial_max_dim()
constexpr int TC_MAX_N = 65536;        // dx_trial_max_rows()
constexpr int TC_BINS = 4096;
constexpr int TC_TILE = 128;
constexpr int TC_KC = 16;              // columns of E per dx_mma step
constexpr int TC_LD = TC_KC + 4;       // LDS row stride of an operand tile: 80 B keeps the 16-B alignment and spreads the banks
constexpr int TC_THREADS = 256;
constexpr int TC_GROUPS = 512;         // persistent workgroups: two per compute unit

// the softmax weight of a live step, w[t] = exp(a[t] - m) / l with m and l as the forward stored them.  Forward and backward state it
// through this one expression, so they hold the same bits.
__device__ __forceinline__ float sp_weight(float a, float m, float l) { return expf(a - m) / l; }

// sum over the live steps of one 64-channel block: wave `wave` takes the steps wave, wave + 4, ..., four accumulators in turn; the
// waves are added in their order through s_part.  f(t) is the lane's term of step t.  Every thread must call it.
template <typename F>
__device__ __forceinline__ float sp_sum_steps(int n, int wave, int lane, float (*s_part)[64], F f) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int t = wave;
  for (; t + 3 * SP_WAVES < n; t += 4 * SP_WAVES) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += f(t + j * SP_WAVES);
  }
  for (int j = 0; t < n; t += SP_WAVES, ++j) acc[j] += f(t);
  s_part[wave][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  float s = s_part[0][lane];
#pragma unroll
  for (int w = 1; w < SP_WAVES; ++w) s += s_part[w][lane];
  __syncthreads();                                              // s_part is free again
  return s;
}

__global__ __launch_bounds__(SP_THREADS) void attn_stat_pool_fwd_kernel(const float* __restrict__ h, const float* __restrict__ a,
                                                                        const int64_t* __restrict__ n_steps, float* __restrict__ out,
                                                                        float* __restrict__ stat, int T, int C) {
  __shared__ float s_w[SP_MAX_T];
  __shared__ float s_part[SP_WAVES][64];
  __shared__ float s_red[SP_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
  const bool live = c < C;
  const int n = (int)dx_clamp_len(n_steps, b, T);
  const float* ar = a + (long)b * T;
  const float* hr = h + (long)b * T * C + (live ? c : 0);
  float* o = out + (long)b * 2 * C;
  if (n == 0) {                                                 // (uniform)
    if (live && wave == 0) { o[c] = 0.f; o[C + c] = 0.f; }
    if (blockIdx.x == 0 && tid == 0) { stat[2 * b] = 0.f; stat[2 * b + 1] = 0.f; }
    return;
  }
  float m = -__builtin_inff();
  for (int t = tid; t < n; t += SP_THREADS) m = fmaxf(m, ar[t]);
  m = dx_block_max<SP_WAVES>(m, s_red);
  float l = 0.f;
  for (int t = tid; t < n; t += SP_THREADS) l += expf(ar[t] - m);
  l = dx_block_sum<SP_WAVES>(l, s_red);
  for (int t = tid; t < n; t += SP_THREADS) s_w[t] = sp_weight(ar[t], m, l);
  __syncthreads();
  const float mu = sp_sum_steps(n, wave, lane, s_part, [&](int t) { return live ? s_w[t] * hr[(long)t * C] : 0.f; });
  const float var = sp_sum_steps(n, wave, lane, s_part, [&](int t) {
    const float d = live ? hr[(long)t * C] - mu : 0.f;
    return s_w[t] * d * d;
  });
  if (live && wave == 0) { o[c] = mu; o[C + c] = sqrtf(var + SP_VAR_EPS); }
  if (blockIdx.x == 0 && tid == 0) { stat[2 * b] = m; stat[2 * b + 1] = l; }
}

// g_h of one 64-channel block and that block's partial q[t] into ws (B, blocks, T)
__global__ __launch_bounds__(SP_THREADS) void attn_stat_pool_bwd_kernel(const float* __restrict__ h, const float* __restrict__ a,
                                                                        const int64_t* __restrict__ n_steps, const float* __restrict__ out,
                                                                        const float* __restrict__ stat, const float* __restrict__ g_out,
                                                                        float* __restrict__ g_h, float* __restrict__ ws, int T, int C) {
  __shared__ float s_w[SP_MAX_T];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
  const bool live = c < C;
  const int n = (int)dx_clamp_len(n_steps, b, T);
  const float* ar = a + (long)b * T;
  const float* hr = h + (long)b * T * C + (live ? c : 0);
  float* gr = g_h + (long)b * T * C + (live ? c : 0);
  float* q = ws + ((long)b * gridDim.x + blockIdx.x) * T;
  const float m = stat[2 * b], l = stat[2 * b + 1];
  for (int t = tid; t < n; t += SP_THREADS) s_w[t] = sp_weight(ar[t], m, l);
  __syncthreads();
  const float mu = live ? out[(long)b * 2 * C + c] : 0.f, sd = live ? out[(long)b * 2 * C + C + c] : 1.f;
  const float g_mu = live ? g_out[(long)b * 2 * C + c] : 0.f, g_sd = live ? g_out[(long)b * 2 * C + C + c] : 0.f;
  for (int t0 = 4 * wave; t0 < n; t0 += 4 * SP_WAVES) {         // the wave takes four consecutive steps, their butterflies in flight
    float qp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + j;
      const bool in = t < n && live;
      const float d = in ? hr[(long)t * C] - mu : 0.f;
      if (in) gr[(long)t * C] = s_w[t] * (g_mu + g_sd * d / sd);
      qp[j] = g_mu * d + g_sd * d * d / (2.f * sd);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[j] = dx_wave_sum(qp[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane == 0 && t0 + j < n) q[t0 + j] = qp[j];
  }
  if (live)
    for (int t = n + wave; t < T; t += SP_WAVES) gr[(long)t * C] = 0.f;
}

// g_a[t] = w[t] (q[t] - sum_s w[s] q[s]), q[t] the partials of the channel blocks added in their order
__global__ __launch_bounds__(SP_THREADS) void attn_stat_pool_ga_kernel(const float* __restrict__ a, const int64_t* __restrict__ n_steps,
                                                                       const float* __restrict__ stat, const float* __restrict__ ws,
                                                                       float* __restrict__ g_a, int T, int blocks) {
  __shared__ float s_w[SP_MAX_T], s_q[SP_MAX_T];
  __shared__ float s_red[SP_WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = (int)dx_clamp_len(n_steps, b, T);
  const float* ar = a + (long)b * T;
  const float* qb = ws + (long)b * blocks * T;
  const float m = stat[2 * b], l = stat[2 * b + 1];
  float part = 0.f;
  for (int t = tid; t < n; t += SP_THREADS) {
    float q = qb[t];
    for (int k = 1; k < blocks; ++k) q += qb[(long)k * T + t];
    const float w = sp_weight(ar[t], m, l);
    s_w[t] = w;
    s_q[t] = q;
    part += w * q;
  }
  const float mean = dx_block_sum<SP_WAVES, false>(part, s_red);
  for (int t = tid; t < T; t += SP_THREADS) g_a[(long)b * T + t] = t < n ? s_w[t] * (s_q[t] - mean) : 0.f;   // (a thread reads its own cells)
}

// ---- the score histograms ---------------------------------------------------------------------------------------------------------------

// 8 consecutive columns k .. k + 7 of row `row` of E, zeros past N rows / D columns
__device__ __forceinline__ f32x8 tc_fetch(const float* __restrict__ E, int N, int D, int row, int k, bool vec) {
  f32x8 r = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (row >= N) return r;
  const float* p = E + (long)row * D + k;
  if (vec) {                                                    // D % 4 == 0: a group of four is inside or outside as a whole
    if (k < D) { const f32x4 v = *reinterpret_cast<const f32x4*>(p); r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3]; }
    if (k + 4 < D) { const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4); r[4] = v[0]; r[5] = v[1]; r[6] = v[2]; r[7] = v[3]; }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) r[e] = p[e];
  }
  return r;
}

__device__ __forceinline__ void tc_store(float* tile, int row, int k, const f32x8& v) {
  float* p = tile + row * TC_LD + k;
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

__device__ __forceinline__ f32x8 tc_frag(const float* tile, int row, int k) {
  const float* p = tile + row * TC_LD + k;
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
  return f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__global__ __launch_bounds__(TC_THREADS) void trial_counts_kernel(const float* __restrict__ E, const int* __restrict__ spk,
                                                                  unsigned long long* __restrict__ counts, int N, int D, int tiles_per_side,
                                                                  int n_tiles) {
  __shared__ unsigned s_hist[2 * TC_BINS];
  __shared__ __attribute__((aligned(16))) float s_a[TC_TILE * TC_LD], s_b[TC_TILE * TC_LD];
  __shared__ int s_spk_i[TC_TILE], s_spk_j[TC_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;        // the wave's 64 x 64 quarter of the tile
  const int fr = lane & 31, fk = 8 * (lane >> 5);               // dx_mma: the lane's row / column and its 8 of the 16 columns of E
  const int lrow = tid >> 1, lk = 8 * (tid & 1);                // staging: thread -> (row of the tile, 8 columns)
  const bool vec = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0;
  for (int i = tid; i < 2 * TC_BINS; i += TC_THREADS) s_hist[i] = 0u;
  int ti = 0, base = 0;                                         // tile row and the index of its first tile (tiles: ti <= tj, row by row)
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    while (tile >= base + (tiles_per_side - ti)) { base += tiles_per_side - ti; ++ti; }
    const int tj = ti + (tile - base);
    const int i0 = ti * TC_TILE, j0 = tj * TC_TILE;
    __syncthreads();                                            // the previous tile's epilogue is done with s_spk (and the zeroing is visible)
    if (tid < TC_TILE) s_spk_i[tid] = i0 + tid < N ? spk[i0 + tid] : 0;
    else s_spk_j[tid - TC_TILE] = j0 + tid - TC_TILE < N ? spk[j0 + tid - TC_TILE] : 0;
    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
    f32x8 ga = tc_fetch(E, N, D, i0 + lrow, lk, vec), gb = tc_fetch(E, N, D, j0 + lrow, lk, vec);
    for (int k0 = 0; k0 < D; k0 += TC_KC) {
      __syncthreads();                                          // the MFMAs of the previous 16 columns have read their fragments
      tc_store(s_a, lrow, lk, ga);
      tc_store(s_b, lrow, lk, gb);
      __syncthreads();
      if (k0 + TC_KC < D) {                                     // (uniform) the next 16 columns, in flight under the MFMAs
        ga = tc_fetch(E, N, D, i0 + lrow, k0 + TC_KC + lk, vec);
        gb = tc_fetch(E, N, D, j0 + lrow, k0 + TC_KC + lk, vec);
      }
      f32x8 fa[2], fb[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) { fa[x] = tc_frag(s_a, wr + 32 * x + fr, fk); fb[x] = tc_frag(s_b, wc + 32 * x + fr, fk); }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) dx_mma(acc[x][y], fa[x], fb[y]);
    }
    // the scores of the tile into the histograms: register r of accumulator (x, y) is the pair (row dx_acc_row(r, lane >> 5), column
    // lane & 31) of its 32 x 32 block
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int cj = wc + 32 * y + fr, j = j0 + cj;
        const int sj = s_spk_j[cj];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ci = wr + 32 * x + dx_acc_row(r, lane >> 5), i = i0 + ci;
          if (i < j && j < N) {
            const float f = fminf(fmaxf(floorf((acc[x][y][r] + 1.f) * 2048.f), 0.f), (float)(TC_BINS - 1));   // (NaN -> 0)
            atomicAdd(&s_hist[(s_spk_i[ci] == sj ? 0 : TC_BINS) + (int)f], 1u);
          }
        }
      }
  }
  __syncthreads();
  for (int i = tid; i < 2 * TC_BINS; i += TC_THREADS) {
    const unsigned v = s_hist[i];
    if (v != 0u) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

}  // namespace

extern "C" long dx_spk_pool_max_channels(void) { return SP_MAX_C; }
extern "C" long dx_spk_pool_max_steps(void) { return SP_MAX_T; }
extern "C" long dx_trial_max_dim(void) { return TC_MAX_D; }
extern "C" long dx_trial_max_rows(void) { return TC_MAX_N; }

extern "C" int dx_attn_stat_pool_fwd(const float* h, const float* a, const int64_t* n_steps, float* out, float* stat, int B, int T, int C,
                                     void* stream) {
  DX_REQUIRE(h && a && n_steps && out && stat, DX_ERR_ARG, "dx_attn_stat_pool_fwd: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && C > 0, DX_ERR_SHAPE, "dx_attn_stat_pool_fwd: bad shape B=%d T=%d C=%d", B, T, C);
  DX_REQUIRE(C <= SP_MAX_C && T <= SP_MAX_T && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_attn_stat_pool_fwd: C=%d channels (at most %d), T=%d steps (at most %d) or B=%d > 65535", C, SP_MAX_C, T, SP_MAX_T, B);
  hipLaunchKernelGGL(attn_stat_pool_fwd_kernel, dim3(dx_cdiv(C, 64), B), dim3(SP_THREADS), 0, (hipStream_t)stream, h, a, n_steps, out, stat,
                     T, C);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_attn_stat_pool_bwd(const float* h, const float* a, const int64_t* n_steps, const float* out, const float* stat,
                                     const float* g_out, float* g_h, float* g_a, float* ws, int B, int T, int C, void* stream) {
  DX_REQUIRE(h && a && n_steps && out && stat && g_out && g_h && g_a && ws, DX_ERR_ARG, "dx_attn_stat_pool_bwd: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && C > 0, DX_ERR_SHAPE, "dx_attn_stat_pool_bwd: bad shape B=%d T=%d C=%d", B, T, C);
  DX_REQUIRE(C <= SP_MAX_C && T <= SP_MAX_T && B <= 65535, DX_ERR_UNSUPPORTED,
             "dx_attn_stat_pool_bwd: C=%d channels (at most %d), T=%d steps (at most %d) or B=%d > 65535", C, SP_MAX_C, T, SP_MAX_T, B);
  const int blocks = dx_cdiv(C, 64);
  hipLaunchKernelGGL(attn_stat_pool_bwd_kernel, dim3(blocks, B), dim3(SP_THREADS), 0, (hipStream_t)stream, h, a, n_steps, out, stat, g_out,
                     g_h, ws, T, C);
  DX_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn_stat_pool_ga_kernel, dim3(B), dim3(SP_THREADS), 0, (hipStream_t)stream, a, n_steps, stat, ws, g_a, T, blocks);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_trial_counts(const float* E, const int* spk, int64_t* counts, int N, int D, void* stream) {
  DX_REQUIRE(E && spk && counts, DX_ERR_ARG, "dx_trial_counts: null pointer");
  DX_REQUIRE(N > 0 && D > 0, DX_ERR_SHAPE, "dx_trial_counts: bad shape N=%d D=%d", N, D);
  DX_REQUIRE(N <= TC_MAX_N && D <= TC_MAX_D, DX_ERR_UNSUPPORTED, "dx_trial_counts: N=%d rows (at most %d) or D=%d columns (at most %d)", N,
             TC_MAX_N, D, TC_MAX_D);
  if (hipMemsetAsync(counts, 0, 2 * TC_BINS * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) {
    dx_set_error("dx_trial_counts: clearing the counts failed");
    return DX_ERR_LAUNCH;
  }
  const int side = dx_cdiv(N, TC_TILE);
  const int n_tiles = side * (side + 1) / 2;
  hipLaunchKernelGGL(trial_counts_kernel, dim3(n_tiles < TC_GROUPS ? n_tiles : TC_GROUPS), dim3(TC_THREADS), 0, (hipStream_t)stream, E, spk,
                     reinterpret_cast<unsigned long long*>(counts), N, D, side, n_tiles);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
