// K34 -- BigVGAN's anti-aliased periodic activation (Lee et al. 2023, `Activation1d` around `Snake` / `SnakeBeta`) as ONE pass over
// K24's time-major fp32 activations: 2x upsampling by a 12-tap filter, s = u + inv_beta sin^2(alpha u) per channel, 2x downsampling
// by a 12-tap filter.  Per utterance b (n = n_rows[b] live rows) and channel c:
//   u[t] = 2 sum_i f_up[t + 15 - 2 i] x[clamp(i - 5, 0, n - 1)]          t in [0, 2 n)
//   s[t] = u[t] + inv_beta[c] sin(alpha[c] u[t])^2
//   y[m] = sum_k f_down[k] s[clamp(2 m + k - 5, 0, 2 n - 1)]              m in [0, n)
// u and s never leave the registers.  A thread owns 4 consecutive channels (one 16-byte load and store per row) and walks a tile of
// SNAKE_R rows: step m loads x row m + 5, which completes the six rows m .. m + 5 that BOTH new samples s[2 m + 5] (taps 10, 8 .. 0)
// and s[2 m + 6] (taps 11, 9 .. 1) read, pushes the two into a 12-deep window and takes y[m] from the window -- every s is computed
// once per tile although six outputs read it.  Five steps before the tile fill the window (10 s values of halo; the 11th comes with
// the first output).  The loop is NOT unrolled: the accurate sinf inlines to ~170 instructions with its large-argument reduction, eight
// of them per step, and the ~90 register moves that shift the two windows are 5 % of a step; unrolled by six (windows indexed at
// compile time, nothing moved) the kernel took 256 VGPRs and 80 KB of code.  Sequence ends: x rows >= n are never read (the edge ROW is replicated, the first clamp); s past 2 n - 1 repeats the last
// VALUE (the second clamp), s before 0 the first; y rows >= n are written as zeros up to N.  No atomics, no LDS: an output is one
// chain of fmas in one lane whose order depends on the row alone, whatever the batch and N.
#include "dx_common.h"

namespace {

constexpr int SNAKE_R = 192;       // rows per thread (dx_vocoder_snake_tile_rows() tells the tests)

struct SnakeArgs {
  const float* x; const float* alpha; const float* inv_beta; float* y; const int64_t* n;
  long ldx, ldy, threads;
  int N, C4, tiles;
  float f_up[12], f_down[12];
};

__device__ __forceinline__ f32x4 snake_act(f32x4 u, f32x4 al, f32x4 ib) {
  f32x4 s;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = sinf(al[e] * u[e]);
    s[e] = fmaf(ib[e], t * t, u[e]);
  }
  return s;
}

// one thread per (utterance, tile of SNAKE_R rows, 4 channels), channels fastest; 1-D grid.  At step m slot i of xw holds x row m + i
// and slot j of sw holds s[2 m - 5 + j]; the windows shift by one row / two samples per step (the unrolling renames most of it away)
__global__ __launch_bounds__(256) void snake_kernel(SnakeArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.threads) return;
  const int cq = (int)(idx % a.C4);
  const long tl = idx / a.C4;
  const int tile = (int)(tl % a.tiles), b = (int)(tl / a.tiles);
  const int n = (int)dx_clamp_len(a.n, b, a.N);
  const int m0 = tile * SNAKE_R, row_end = min(m0 + SNAKE_R, a.N), live_end = min(row_end, n), last = 2 * n - 1;
  const float* xb = a.x + (long)b * a.N * a.ldx + 4 * cq;
  float* yb = a.y + (long)b * a.N * a.ldy + 4 * cq;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (m0 < n) {
    const f32x4 al = *reinterpret_cast<const f32x4*>(a.alpha + 4 * cq), ib = *reinterpret_cast<const f32x4*>(a.inv_beta + 4 * cq);
    f32x4 xw[6], sw[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) xw[i] = *reinterpret_cast<const f32x4*>(xb + (long)min(max(m0 - 6 + i, 0), n - 1) * a.ldx);
#pragma unroll
    for (int j = 0; j < 12; ++j) sw[j] = zero;
    f32x4 xnext = *reinterpret_cast<const f32x4*>(xb + (long)min(m0, n - 1) * a.ldx);   // row m + 5 of the coming step, a step ahead
#pragma unroll 1
    for (int m = m0 - 5; m < live_end; ++m) {                                 // five steps fill the window: 11 s values of halo
#pragma unroll
      for (int i = 0; i < 5; ++i) xw[i] = xw[i + 1];
      xw[5] = xnext;
      xnext = *reinterpret_cast<const f32x4*>(xb + (long)min(max(m + 6, 0), n - 1) * a.ldx);
      f32x4 uo = zero, ue = zero;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        uo += a.f_up[10 - 2 * i] * xw[i];                                     // s[2 m + 5]: rows m .. m + 5 under taps 10, 8 .. 0
        ue += a.f_up[11 - 2 * i] * xw[i];                                     // s[2 m + 6]: the same rows under taps 11, 9 .. 1
      }
      const f32x4 so = snake_act(2.f * uo, al, ib), se = snake_act(2.f * ue, al, ib);
#pragma unroll
      for (int j = 0; j < 10; ++j) sw[j] = sw[j + 2];
      sw[10] = 2 * m + 5 > last ? sw[9] : so;                                 // past the end: the last VALUE again
      sw[11] = 2 * m + 6 > last ? sw[10] : se;
      if (m == -3) {                                                          // se is s[0]: it stands for every s[t < 0]
#pragma unroll
        for (int j = 0; j < 11; ++j) sw[j] = se;
      }
      if (m >= m0) {
        f32x4 v = zero;
#pragma unroll
        for (int j = 0; j < 12; ++j) v += a.f_down[j] * sw[j];
        *reinterpret_cast<f32x4*>(yb + (long)m * a.ldy) = v;
      }
    }
  }
  for (int m = max(m0, live_end); m < row_end; ++m) *reinterpret_cast<f32x4*>(yb + (long)m * a.ldy) = zero;
}

bool snake_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int dx_vocoder_snake_tile_rows(void) { return SNAKE_R; }

extern "C" int dx_vocoder_snake(const float* x, long ldx, const float* alpha, const float* inv_beta, const float* filters, float* y,
                                long ldy, const int64_t* n_rows, int B, int N, int C, void* stream) {
  DX_REQUIRE(x && alpha && inv_beta && filters && y && n_rows, DX_ERR_ARG, "dx_vocoder_snake: null pointer");
  DX_REQUIRE(B > 0 && N > 0 && C > 0 && ldx >= C && ldy >= C, DX_ERR_SHAPE, "dx_vocoder_snake: bad shape B=%d N=%d C=%d ldx=%ld ldy=%ld",
             B, N, C, ldx, ldy);
  DX_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, DX_ERR_UNSUPPORTED,
             "dx_vocoder_snake: C=%d, ldx=%ld and ldy=%ld must be multiples of 4 (16-byte loads and stores)", C, ldx, ldy);
  DX_REQUIRE(snake_aligned16(x) && snake_aligned16(y) && snake_aligned16(alpha) && snake_aligned16(inv_beta), DX_ERR_ARG,
             "dx_vocoder_snake: x, y, alpha and inv_beta must be 16-byte aligned");
  DX_REQUIRE(y != x, DX_ERR_ARG, "dx_vocoder_snake: the output must not alias the input (other threads read its halo)");
  SnakeArgs a = {x, alpha, inv_beta, y, n_rows, ldx, ldy, 0, N, C / 4, (int)(((long)N + SNAKE_R - 1) / SNAKE_R), {}, {}};
  a.threads = (long)B * a.tiles * a.C4;
  const long blocks = (a.threads + 255) / 256;
  DX_REQUIRE(blocks <= 0x7fffffffL && (long)N + SNAKE_R <= 0x7fffffffL, DX_ERR_UNSUPPORTED,
             "dx_vocoder_snake: B=%d N=%d C=%d need %ld workgroups: more than grid.x, or more rows than a 32-bit row index, holds", B, N, C, blocks);
  for (int i = 0; i < 12; ++i) { a.f_up[i] = filters[i]; a.f_down[i] = filters[12 + i]; }
  hipLaunchKernelGGL(snake_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
