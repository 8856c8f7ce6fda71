// The in-LDS FFT of the audio kernels (mel front-end: frontend.hip, Griffin-Lim: griffin_lim.hip): the supported sizes,
// the twiddle / window table kernel and the radix-4 Stockham stage loop.
#pragma once
#include <type_traits>

#include "dx_common.h"

// The supported n_fft (powers of 4: radix-4 stages only) in one place: calls f(std::integral_constant<int, n_fft>) --
// a kernel launch with NFFT = decltype(N)::value and, for the FFT kernels, NFFT / 4 threads -- and returns false, without
// calling f, for any other size.
template <typename F>
static inline bool dx_nfft_dispatch(int n_fft, F&& f) {
  switch (n_fft) {
    case 256: f(std::integral_constant<int, 256>{}); return true;
    case 1024: f(std::integral_constant<int, 1024>{}); return true;
    case 4096: f(std::integral_constant<int, 4096>{}); return true;
  }
  return false;
}
static inline bool dx_nfft_ok(int n_fft) { return dx_nfft_dispatch(n_fft, [](auto) {}); }

enum DxHann { DX_HANN_PERIODIC, DX_HANN_SYMMETRIC };   // torch.hann_window (STFT) / np.hanning (Griffin-Lim)

// twiddle[t] = exp(-2 pi i t / n_fft) (cos, sin); window[n] = 0.5 - 0.5 cos(2 pi n / n_fft) (periodic) or
// 0.5 - 0.5 cos(2 pi n / (n_fft - 1)) (symmetric).  grid ceil(n_fft / 256), 256 threads.
template <DxHann HANN>
static __global__ void dx_fft_tables_kernel(float* __restrict__ twiddle, float* __restrict__ window, int n_fft) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_fft) return;
  double s, c;
  sincospi(2.0 * (double)n / (double)n_fft, &s, &c);
  twiddle[2 * n] = (float)c;
  twiddle[2 * n + 1] = (float)(-s);
  window[n] = (float)(0.5 - 0.5 * (HANN == DX_HANN_PERIODIC ? c : cospi(2.0 * (double)n / (double)(n_fft - 1))));
}

struct cplx { float re, im; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// Radix-4 Stockham FFT of NFFT complex points (forward, exp(-2 pi i k n / N)) in the ping-pong LDS buffers bufr / bufi:
// NFFT / 4 threads (j = threadIdx.x), one butterfly per thread per stage, one barrier per stage.  Input in buffer `cur`
// (written and synchronised by the caller); returns the buffer holding the output.
template <int NFFT>
__device__ __forceinline__ int dx_fft_lds(float (*bufr)[NFFT], float (*bufi)[NFFT], int cur, const float* twiddle, int j) {
  constexpr int NT = NFFT / 4;
#pragma unroll
  for (int Ns = 1; Ns < NFFT; Ns *= 4) {
    const int k = j & (Ns - 1);
    cplx v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = {bufr[cur][j + r * NT], bufi[cur][j + r * NT]};
    if (Ns > 1) {
      const int t = k * (NFFT / (4 * Ns));                        // angle = -2 pi k / (4 Ns)
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        const cplx w = {twiddle[2 * (r * t)], twiddle[2 * (r * t) + 1]};
        v[r] = cmul(v[r], w);
      }
    }
    const cplx s02 = {v[0].re + v[2].re, v[0].im + v[2].im}, d02 = {v[0].re - v[2].re, v[0].im - v[2].im};
    const cplx s13 = {v[1].re + v[3].re, v[1].im + v[3].im}, d13 = {v[1].re - v[3].re, v[1].im - v[3].im};
    const cplx y0 = {s02.re + s13.re, s02.im + s13.im}, y2 = {s02.re - s13.re, s02.im - s13.im};
    const cplx y1 = {d02.re + d13.im, d02.im - d13.re};           // d02 - i d13
    const cplx y3 = {d02.re - d13.im, d02.im + d13.re};           // d02 + i d13
    const int o = (j - k) * 4 + k;                                // (j / Ns) * 4 Ns + k
    bufr[cur ^ 1][o] = y0.re; bufi[cur ^ 1][o] = y0.im;
    bufr[cur ^ 1][o + Ns] = y1.re; bufi[cur ^ 1][o + Ns] = y1.im;
    bufr[cur ^ 1][o + 2 * Ns] = y2.re; bufi[cur ^ 1][o + 2 * Ns] = y2.im;
    bufr[cur ^ 1][o + 3 * Ns] = y3.re; bufi[cur ^ 1][o + 3 * Ns] = y3.im;
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// ---- every power of two from 256 to 4096 (K36, spectrogram.hip: the multi-resolution discriminator's 512 and 2048) ------------
// A dispatch of its own: dx_nfft_dispatch / dx_nfft_ok above state what the front end and Griffin-Lim accept, and stay as they are.
template <typename F>
static inline bool dx_nfft2_dispatch(int n_fft, F&& f) {
  switch (n_fft) {
    case 256: f(std::integral_constant<int, 256>{}); return true;
    case 512: f(std::integral_constant<int, 512>{}); return true;
    case 1024: f(std::integral_constant<int, 1024>{}); return true;
    case 2048: f(std::integral_constant<int, 2048>{}); return true;
    case 4096: f(std::integral_constant<int, 4096>{}); return true;
  }
  return false;
}
static inline bool dx_nfft2_ok(int n_fft) { return dx_nfft2_dispatch(n_fft, [](auto) {}); }

// dx_fft_lds for any power of two NFFT >= 4: the radix-4 Stockham stages while 4 Ns <= NFFT -- the same butterfly, so a power of 4
// gives dx_fft_lds's bits -- closed, where NFFT = 2 * 4^m, by ONE radix-2 stage (Ns = NFFT / 2: butterfly k reads k and k + NFFT / 2,
// twiddle k, writes k and k + NFFT / 2; two butterflies per thread).  NFFT / 4 threads, one barrier per stage; same buffers and return.
template <int NFFT>
__device__ __forceinline__ int dx_fft_lds2(float (*bufr)[NFFT], float (*bufi)[NFFT], int cur, const float* twiddle, int j) {
  constexpr int NT = NFFT / 4;
#pragma unroll
  for (int Ns = 1; Ns * 4 <= NFFT; Ns *= 4) {
    const int k = j & (Ns - 1);
    cplx v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = {bufr[cur][j + r * NT], bufi[cur][j + r * NT]};
    if (Ns > 1) {
      const int t = k * (NFFT / (4 * Ns));                        // angle = -2 pi k / (4 Ns)
#pragma unroll
      for (int r = 1; r < 4; ++r) {
        const cplx w = {twiddle[2 * (r * t)], twiddle[2 * (r * t) + 1]};
        v[r] = cmul(v[r], w);
      }
    }
    const cplx s02 = {v[0].re + v[2].re, v[0].im + v[2].im}, d02 = {v[0].re - v[2].re, v[0].im - v[2].im};
    const cplx s13 = {v[1].re + v[3].re, v[1].im + v[3].im}, d13 = {v[1].re - v[3].re, v[1].im - v[3].im};
    const cplx y0 = {s02.re + s13.re, s02.im + s13.im}, y2 = {s02.re - s13.re, s02.im - s13.im};
    const cplx y1 = {d02.re + d13.im, d02.im - d13.re};           // d02 - i d13
    const cplx y3 = {d02.re - d13.im, d02.im + d13.re};           // d02 + i d13
    const int o = (j - k) * 4 + k;                                // (j / Ns) * 4 Ns + k
    bufr[cur ^ 1][o] = y0.re; bufi[cur ^ 1][o] = y0.im;
    bufr[cur ^ 1][o + Ns] = y1.re; bufi[cur ^ 1][o + Ns] = y1.im;
    bufr[cur ^ 1][o + 2 * Ns] = y2.re; bufi[cur ^ 1][o + 2 * Ns] = y2.im;
    bufr[cur ^ 1][o + 3 * Ns] = y3.re; bufi[cur ^ 1][o + 3 * Ns] = y3.im;
    cur ^= 1;
    __syncthreads();
  }
  if constexpr (__builtin_ctz(NFFT) & 1) {                        // NFFT = 2 * 4^m: Ns = NFFT / 2
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = j + h * NT;
      const cplx a = {bufr[cur][k], bufi[cur][k]};
      const cplx w = {twiddle[2 * k], twiddle[2 * k + 1]};        // angle = -2 pi k / NFFT
      const cplx b = cmul(cplx{bufr[cur][k + NFFT / 2], bufi[cur][k + NFFT / 2]}, w);
      bufr[cur ^ 1][k] = a.re + b.re; bufi[cur ^ 1][k] = a.im + b.im;
      bufr[cur ^ 1][k + NFFT / 2] = a.re - b.re; bufi[cur ^ 1][k + NFFT / 2] = a.im - b.im;
    }
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}
