// K18 -- Griffin-Lim preview audio of the synthesis path (reference `griffin_lim.py:63-198` as called from
// `generate.py:130-137, 311-314`):
//   mel_to_linear:  per frame, min 1/2 ||A x - exp(mel)||^2 s.t. x >= 0 (A = the (n_mel, n_fft/2 + 1) Slaney filterbank).
//                   The reference starts L-BFGS-B from clip(pinv(A) b, 0) and stops it early; here the same start is
//                   followed by a fixed number of FISTA (accelerated projected gradient) steps of size 1 / ||A||_2^2.
//                   One wave per frame: x, its momentum copy y and b stay in registers / LDS for every iteration.  A is
//                   sparse (each filter a contiguous bin range, each bin in at most two filters): A y walks every filter's
//                   range in LDS, A^T r is two products per bin from per-bin (filter, weight) pairs held in registers.
//   griffin_lim:    per iteration, frames(x) -> window, rFFT, keep the phase, swap in the given magnitude, irFFT, window
//                   (one workgroup per PAIR of frames: the two real frames travel as the real / imaginary parts of one
//                   complex radix-4 Stockham FFT in LDS, forward and inverse), then a gather overlap-add in frame order
//                   (no atomics: bit-reproducible) divided by n_fft / hop / 2.  Two launches per iteration.
//   normalise:      x / max|x| per utterance; an utterance with no frame or all zeros gives zeros (the reference: 0 / 0).
#include "dx_fft.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// mel -> linear magnitude (NNLS)

struct NnlsArgs {
  const float* mel; const int64_t* lengths; const float* fb; const int* lo; const int* hi; const float* pinv_t;
  const int* bin_m; const float* bin_w; float* lin; long ld_lb, ld_lk, ld_lt;
  int T, n_mel, iters, input_is_log; float step;
};

constexpr int NNLS_MAX_MEL = 256;   // 4 filters per lane

// grid (T, B), one wave per frame.  Lane l owns bins l, l + 64, ... (PER of them).
template <int NFFT>
__global__ __launch_bounds__(64) void gl_nnls_kernel(NnlsArgs a) {
  constexpr int NB = NFFT / 2 + 1, PER = (NB + 63) / 64;
  __shared__ float4 bins[NB];                 // {y, w_a, w_b, (m_a + 1) | (m_b + 1) << 16}: one ds_read_b128 per filter tap
  __shared__ float bsh[NNLS_MAX_MEL], rsh[NNLS_MAX_MEL];
  const int l = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  float* lin = a.lin + (long)b * a.ld_lb + (long)f * a.ld_lt;
  if (f >= (int)a.lengths[b]) {                                    // frames past the utterance: zeros
    for (int k = l; k < NB; k += 64) lin[(long)k * a.ld_lk] = 0.f;
    return;
  }
  for (int m = l; m < a.n_mel; m += 64) {
    const float v = a.mel[((long)b * a.n_mel + m) * a.T + f];
    bsh[m] = a.input_is_log ? expf(v) : v;
  }
  float x[PER], y[PER], wa[PER], wb[PER];
  int ma[PER], mb[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = l + 64 * i;
    const bool ok = k < NB;
    ma[i] = ok ? a.bin_m[2 * k] : -1;
    mb[i] = ok ? a.bin_m[2 * k + 1] : -1;
    wa[i] = ok ? a.bin_w[2 * k] : 0.f;
    wb[i] = ok ? a.bin_w[2 * k + 1] : 0.f;
    if (ok) bins[k] = make_float4(0.f, wa[i], wb[i], __int_as_float((ma[i] + 1) | ((mb[i] + 1) << 16)));
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PER; ++i) {                                  // start: clip(pinv(A) b, 0) (griffin_lim.py:47-48)
    const int k = l + 64 * i;
    float s = 0.f;
    if (k < NB) {
#pragma unroll 8
      for (int m = 0; m < a.n_mel; ++m) s = fmaf(a.pinv_t[(long)m * NB + k], bsh[m], s);
    }
    x[i] = fmaxf(s, 0.f);
    y[i] = x[i];
  }
  constexpr int MPL = NNLS_MAX_MEL / 64;                          // filters per lane: m = l + 64 r
  int k0[MPL], k1[MPL];
  float bm[MPL];
#pragma unroll
  for (int r = 0; r < MPL; ++r) {                                  // loop invariants in registers (the barriers below would
    const int m = l + 64 * r;                                      // otherwise re-load them every iteration)
    const bool ok = m < a.n_mel;
    k0[r] = ok ? a.lo[m] : 0;
    k1[r] = ok ? a.hi[m] : 0;
    bm[r] = ok ? bsh[m] : 0.f;
  }
  float t = 1.f;
  for (int it = 0; it < a.iters; ++it) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = l + 64 * i;
      if (k < NB) bins[k].x = y[i];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MPL; ++r) {                                // r = A y - b
      const int m = l + 64 * r;
      if (m < a.n_mel) {
        float s = 0.f;
#pragma unroll 4
        for (int k = k0[r]; k < k1[r]; ++k) {                      // in order: the same sum whatever the unrolling
          const float4 v = bins[k];
          const int mm = __float_as_int(v.w);
          const float w = ((mm & 0xffff) == m + 1) ? v.y : ((mm >> 16) == m + 1 ? v.z : 0.f);
          s = fmaf(w, v.x, s);
        }
        rsh[m] = s - bm[r];
      }
    }
    __syncthreads();
    const float tn = 0.5f * (1.f + sqrtf(1.f + 4.f * t * t));
    const float mom = (t - 1.f) / tn;
#pragma unroll
    for (int i = 0; i < PER; ++i) {                                // x+ = max(y - step A^T r, 0); y = x+ + mom (x+ - x)
      const float g = (ma[i] >= 0 ? wa[i] * rsh[ma[i]] : 0.f) + (mb[i] >= 0 ? wb[i] * rsh[mb[i]] : 0.f);
      const float xn = fmaxf(y[i] - a.step * g, 0.f);
      y[i] = xn + mom * (xn - x[i]);
      x[i] = xn;
    }
    t = tn;
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int k = l + 64 * i;
    if (k < NB) lin[(long)k * a.ld_lk] = x[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Griffin-Lim

__device__ __forceinline__ int gl_nframes(int64_t len) { return len > 2 ? (int)(len - 2) : 0; }   // spec[:, :-2]

// S * R / |R|, R = 0 -> S (np.angle(0) = 0)
__device__ __forceinline__ cplx gl_swap_mag(float re, float im, float s) {
  const float m = hypotf(re, im);
  return m > 0.f ? cplx{s * (re / m), s * (im / m)} : cplx{s, 0.f};
}

struct FrameArgs {
  const float* x; long ldx; const float* mag; long ld_mb, ld_mk, ld_mt; const int64_t* lengths;
  const float* twiddle; const float* window; float* frames; int Fcap, hop;
};

// grid (ceil(Fcap / 2), B), NFFT / 4 threads: frames f0 = 2 p and f0 + 1 of utterance b, written windowed to
// frames[(b * Fcap + f) * NFFT + n] (the overlap-add divides).
template <int NFFT>
__global__ __launch_bounds__(NFFT / 4) void gl_frames_kernel(FrameArgs a) {
  constexpr int NT = NFFT / 4, H = NFFT / 2;
  __shared__ float bufr[2][NFFT], bufi[2][NFFT];
  const int j = threadIdx.x, b = blockIdx.y, f0 = 2 * blockIdx.x;
  const int F = gl_nframes(a.lengths[b]);
  if (f0 >= F) return;
  const bool has1 = f0 + 1 < F;
  const float* x = a.x + (long)b * a.ldx + (long)f0 * a.hop;
#pragma unroll
  for (int r = 0; r < 4; ++r) {                                    // z = w x_f0 + i w x_f1
    const int n = j + r * NT;
    const float w = a.window[n];
    bufr[0][n] = w * x[n];
    bufi[0][n] = has1 ? w * x[n + a.hop] : 0.f;
  }
  __syncthreads();
  int cur = dx_fft_lds<NFFT>(bufr, bufi, 0, a.twiddle, j);
  const float* S = a.mag + (long)b * a.ld_mb + (long)f0 * a.ld_mt;
  cplx y1v[(H + NT) / NT], y2v[(H + NT) / NT];
#pragma unroll
  for (int r = 0; r < (H + NT) / NT; ++r) {                        // bins 0..H: split Z into X1, X2, swap magnitudes
    const int k = j + r * NT;
    if (k > H) break;
    const int kn = (NFFT - k) & (NFFT - 1);
    const float zr = bufr[cur][k], zi = bufi[cur][k], nr = bufr[cur][kn], ni = bufi[cur][kn];
    // X1 = (Z[k] + conj Z[N-k]) / 2,  X2 = (Z[k] - conj Z[N-k]) / 2i
    cplx y1 = gl_swap_mag(0.5f * (zr + nr), 0.5f * (zi - ni), S[(long)k * a.ld_mk]);
    cplx y2 = has1 ? gl_swap_mag(0.5f * (zi + ni), -0.5f * (zr - nr), S[(long)k * a.ld_mk + a.ld_mt]) : cplx{0.f, 0.f};
    if (k == 0 || k == H) { y1.im = 0.f; y2.im = 0.f; }            // irfft ignores the imaginary parts there
    y1v[r] = y1; y2v[r] = y2;
  }
  const int nxt = cur ^ 1;
#pragma unroll
  for (int r = 0; r < (H + NT) / NT; ++r) {                        // conj(Y1 + i Y2) over the full circle (Hermitian halves)
    const int k = j + r * NT;
    if (k > H) break;
    const cplx y1 = y1v[r], y2 = y2v[r];
    bufr[nxt][k] = y1.re - y2.im;
    bufi[nxt][k] = -(y1.im + y2.re);
    if (k != 0 && k != H) {
      bufr[nxt][NFFT - k] = y1.re + y2.im;
      bufi[nxt][NFFT - k] = y1.im - y2.re;
    }
  }
  __syncthreads();
  cur = dx_fft_lds<NFFT>(bufr, bufi, nxt, a.twiddle, j);          // ifft(Z) = conj(fft(conj Z)) / N
  constexpr float inv_n = 1.f / NFFT;
  float* o0 = a.frames + ((long)b * a.Fcap + f0) * NFFT;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = j + r * NT;
    const float w = a.window[n];
    o0[n] = w * (bufr[cur][n] * inv_n);
    if (has1) o0[NFFT + n] = w * (-bufi[cur][n] * inv_n);
  }
}

// grid (ceil(S / 256), B): x[b, s] = (sum over the frames covering s, in frame order) / (n_fft / hop / 2); 0 past n_samples.
__global__ __launch_bounds__(256) void gl_ola_kernel(const float* __restrict__ frames, const int64_t* __restrict__ lengths,
                                                     float* __restrict__ x, long ldx, int64_t* __restrict__ n_samples,
                                                     long S, int Fcap, int n_fft, int hop, float scale) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const int F = gl_nframes(lengths[b]);
  const long Sb = (long)F * hop + n_fft;
  if (s == 0 && n_samples) n_samples[b] = Sb;
  if (s >= S) return;
  float acc = 0.f;
  if (s < Sb && F > 0) {
    const long fa = s >= n_fft ? (s - n_fft) / hop + 1 : 0;
    const long fb = min((long)F - 1, s / hop);
    const float* fr = frames + (long)b * Fcap * n_fft;
    for (long f = fa; f <= fb; ++f) acc += fr[f * n_fft + (s - f * hop)];
    acc = acc / scale;
  }
  x[(long)b * ldx + s] = acc;
}

// standard normal noise x[b, s] = Box-Muller of two counter hashes of (seed, b, s); 0 past n_samples
__global__ __launch_bounds__(256) void gl_noise_kernel(float* __restrict__ x, long ldx, const int64_t* __restrict__ lengths,
                                                       long S, int n_fft, int hop, uint64_t seed) {
  const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= S) return;
  const long Sb = (long)gl_nframes(lengths[b]) * hop + n_fft;
  float v = 0.f;
  if (s < Sb) {
    const uint32_t key = dx_key32(seed, (uint32_t)b);
    const uint32_t h1 = dx_mix32(key ^ dx_mix32(2u * (uint32_t)s + 0x68E31DA4u));
    const uint32_t h2 = dx_mix32(key ^ dx_mix32(2u * (uint32_t)s + 0x68E31DA5u));
    const float u1 = ((h1 >> 8) + 1u) * (1.f / 16777216.f);       // (0, 1]
    const float u2 = (h2 >> 8) * (1.f / 16777216.f);              // [0, 1)
    v = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
  }
  x[(long)b * ldx + s] = v;
}

// grid B, 256 threads: x / max|x| over n_samples; zeros when the utterance has no frame or is all zeros
__global__ __launch_bounds__(256) void gl_normalise_kernel(float* __restrict__ x, long ldx, const int64_t* __restrict__ lengths,
                                                           long S, int n_fft, int hop) {
  __shared__ float red[4];
  const int b = blockIdx.x, j = threadIdx.x;
  const int F = gl_nframes(lengths[b]);
  const long Sb = min((long)F * hop + n_fft, S);
  float* xb = x + (long)b * ldx;
  float m = 0.f;
  for (long s = j; s < Sb; s += 256) m = fmaxf(m, fabsf(xb[s]));
  m = dx_wave_max(m);
  if ((j & 63) == 0) red[j >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const bool zero = F == 0 || !(m > 0.f);
  for (long s = j; s < S; s += 256) xb[s] = (zero || s >= Sb) ? 0.f : xb[s] / m;
}

// What dx_griffin_lim, dx_gl_noise and dx_gl_normalise require of their shape: a T-frame batch makes S = max(T - 2, 0) * hop +
// n_fft samples per utterance, and the rows (`ld` floats apart) must hold them.  `fn`: the entry point, for the message.
int gl_check_shape(const char* fn, int B, int T, int n_fft, int hop, long ld, long* S) {
  DX_REQUIRE(B > 0 && T > 0 && hop > 0, DX_ERR_SHAPE, "%s: bad shape B=%d T=%d hop=%d", fn, B, T, hop);
  DX_REQUIRE(dx_nfft_ok(n_fft) && n_fft % hop == 0, DX_ERR_UNSUPPORTED,
             "%s: n_fft=%d hop=%d unsupported (n_fft 256, 1024 or 4096, a multiple of hop)", fn, n_fft, hop);
  *S = (long)(T > 2 ? T - 2 : 0) * hop + n_fft;
  DX_REQUIRE(ld >= *S, DX_ERR_SHAPE, "%s: rows hold %ld < %ld samples", fn, ld, *S);
  return DX_OK;
}

}  // namespace

extern "C" int dx_gl_tables(float* twiddle, float* window, int n_fft, void* stream) {
  DX_REQUIRE(twiddle && window, DX_ERR_ARG, "dx_gl_tables: null pointer");
  DX_REQUIRE(dx_nfft_ok(n_fft), DX_ERR_UNSUPPORTED, "dx_gl_tables: n_fft=%d unsupported (256, 1024 or 4096)", n_fft);
  hipLaunchKernelGGL(dx_fft_tables_kernel<DX_HANN_SYMMETRIC>, dim3(dx_cdiv(n_fft, 256)), dim3(256), 0, (hipStream_t)stream, twiddle,
                     window, n_fft);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_mel_to_linear(const float* mel, const int64_t* lengths, const float* fb, const int* fb_lo, const int* fb_hi,
                                const float* pinv_t, const int* bin_m, const float* bin_w, float* linear, long ld_lb, long ld_lk,
                                long ld_lt, int B, int T, int n_mel, int n_fft, int iters, float step, int input_is_log,
                                void* stream) {
  DX_REQUIRE(mel && lengths && fb && fb_lo && fb_hi && pinv_t && bin_m && bin_w && linear, DX_ERR_ARG,
             "dx_mel_to_linear: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && n_mel > 0 && n_mel <= NNLS_MAX_MEL && iters >= 0 && step > 0.f, DX_ERR_SHAPE,
             "dx_mel_to_linear: bad shape B=%d T=%d n_mel=%d (<= %d) iters=%d step=%g", B, T, n_mel, NNLS_MAX_MEL, iters,
             (double)step);
  NnlsArgs a{mel, lengths, fb, fb_lo, fb_hi, pinv_t, bin_m, bin_w, linear, ld_lb, ld_lk, ld_lt, T, n_mel, iters, input_is_log, step};
  const bool ok = dx_nfft_dispatch(n_fft, [&](auto N) {
    hipLaunchKernelGGL(gl_nnls_kernel<decltype(N)::value>, dim3(T, B), dim3(64), 0, (hipStream_t)stream, a);
  });
  DX_REQUIRE(ok, DX_ERR_UNSUPPORTED, "dx_mel_to_linear: n_fft=%d unsupported (256, 1024 or 4096)", n_fft);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" long dx_gl_ws_floats(int B, int T, int n_fft) {
  return (long)B * (T > 2 ? T - 2 : 0) * n_fft;
}

extern "C" int dx_griffin_lim(const float* mag, long ld_mb, long ld_mk, long ld_mt, const int64_t* lengths, const float* x0,
                              long ldx0, const float* twiddle, const float* window, float* wav, long ldw, int64_t* n_samples,
                              float* ws, int B, int T, int n_fft, int hop, int iters, uint64_t seed, void* stream) {
  DX_REQUIRE(mag && lengths && twiddle && window && wav && n_samples && (ws || T <= 2), DX_ERR_ARG, "dx_griffin_lim: null pointer");
  DX_REQUIRE(iters >= 1, DX_ERR_SHAPE, "dx_griffin_lim: bad shape iters=%d", iters);
  long S;
  if (const int rc = gl_check_shape("dx_griffin_lim", B, T, n_fft, hop, x0 && ldx0 < ldw ? ldx0 : ldw, &S)) return rc;
  const int Fcap = T > 2 ? T - 2 : 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 sgrid((unsigned)((S + 255) / 256), B);
  const float scale = (float)((double)n_fft / hop / 2.0);
  if (!x0) {
    hipLaunchKernelGGL(gl_noise_kernel, sgrid, dim3(256), 0, s, wav, ldw, lengths, S, n_fft, hop, seed);
    DX_LAUNCH_CHECK();
  }
  const float* src = x0 ? x0 : wav;
  long lds = x0 ? ldx0 : ldw;
  for (int it = 0; it < iters; ++it) {
    if (Fcap > 0) {
      FrameArgs a{src, lds, mag, ld_mb, ld_mk, ld_mt, lengths, twiddle, window, ws, Fcap, hop};
      dx_nfft_dispatch(n_fft, [&](auto N) {
        constexpr int NFFT = decltype(N)::value;
        hipLaunchKernelGGL(gl_frames_kernel<NFFT>, dim3(dx_cdiv(Fcap, 2), B), dim3(NFFT / 4), 0, s, a);
      });
      DX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gl_ola_kernel, sgrid, dim3(256), 0, s, ws, lengths, wav, ldw, n_samples, S, Fcap, n_fft, hop, scale);
    DX_LAUNCH_CHECK();
    src = wav;
    lds = ldw;
  }
  return DX_OK;
}

extern "C" int dx_gl_noise(float* x, long ldx, const int64_t* lengths, int B, int T, int n_fft, int hop, uint64_t seed,
                           void* stream) {
  DX_REQUIRE(x && lengths, DX_ERR_ARG, "dx_gl_noise: null pointer");
  long S;
  if (const int rc = gl_check_shape("dx_gl_noise", B, T, n_fft, hop, ldx, &S)) return rc;
  hipLaunchKernelGGL(gl_noise_kernel, dim3((unsigned)((S + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, x, ldx, lengths,
                     S, n_fft, hop, seed);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_gl_normalise(float* wav, long ldw, const int64_t* lengths, int B, int T, int n_fft, int hop, void* stream) {
  DX_REQUIRE(wav && lengths, DX_ERR_ARG, "dx_gl_normalise: null pointer");
  long S;
  if (const int rc = gl_check_shape("dx_gl_normalise", B, T, n_fft, hop, ldw, &S)) return rc;
  hipLaunchKernelGGL(gl_normalise_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, wav, ldw, lengths, S, n_fft, hop);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
