// K36 -- the magnitude spectrogram of a waveform and its gradient back to the waveform: the one operation BigVGAN's multi-resolution
// discriminator (Lee et al. 2023, section 3) adds to the discriminators of K33's fine-tuning.  Per utterance b (n = n_samples[b]) and
// resolution (n_fft, hop), with the caller's window table w[0 .. n_fft):
//   p = (n_fft - hop) div 2,   x~[s] = x[r(s - p)] (torch's 'reflect'),   F = 1 + (n + 2 p - n_fft) div hop
//   X[f, k] = sum_j w[j] x~[f hop + j] exp(-2 pi i j k / n_fft),  k in [0, n_fft / 2];   mag[b, k, f] = sqrt(re^2 + im^2)
// Forward: one workgroup per frame, as fe_fft_mel_kernel -- the hop-strided, reflect-indexed frame goes straight from wav into LDS
// (no padded copy), through dx_fft_lds2 (n_fft / 4 threads, ping-pong buffers: 16 n_fft bytes), and the magnitudes are written from LDS.
// Backward, nothing saved: launch 1 recomputes X per frame, forms G = dmag X / |X| (0 where |X| = 0) on the bins [0, n_fft / 2] and
// zeros above, and takes dy_f[j] = w[j] Re sum_k G[k] exp(+2 pi i j k / n_fft) as the real part of the SAME forward FFT over conj(G)
// (Re of a sum is Re of its conjugate); dy_f goes to the workspace.  Launch 2, one thread per sample, gathers
//   dx~[s] = sum_{f : 0 <= s - f hop < n_fft} dy_f[s - f hop]       (ascending f)
//   dx[i]  = dx~[i + p] + (1 <= i <= p ? dx~[p - i] : 0) + (n - 1 - p <= i <= n - 2 ? dx~[p + 2 (n - 1) - i] : 0)    (in this order)
// No atomics: every sum is one chain in one lane whose order the sample index and n alone set -- the same bits twice, alone, in any
// batch and at any T.  The kernels derive F from the device's n_samples under the launcher's own conditions (an utterance that fails
// them has no frame), so no index leaves wav, mag, dmag, the workspace or dwav whatever that tensor holds.
#include "dx_fft.h"

namespace {

struct SpecArgs {
  const float* wav; long ldw; const int64_t* n; const float* twiddle; const float* window;
  float* mag;            // forward: out (B, bins, T)
  const float* dmag;     // backward: in (B, bins, T)
  float* ws;             // backward: dy (B, T, n_fft)
  int S, T, hop;
};

// live samples and frames of utterance b; 0 frames where the padding is not defined (n <= p), no frame fits, or n exceeds the row
__device__ __forceinline__ int spec_frames(const SpecArgs& a, int b, int n_fft, long* n_out) {
  const long n = (long)a.n[b], p = (n_fft - a.hop) / 2;
  *n_out = n;
  if (n <= p || n + 2 * p < n_fft || n > a.S) return 0;
  const long F = 1 + (n + 2 * p - n_fft) / a.hop;
  return (int)(F < a.T ? F : a.T);
}

// the windowed frame f of utterance b into bufr[0] (bufi[0] = 0), then its FFT; returns the buffer that holds X
template <int NFFT>
__device__ __forceinline__ int spec_frame_fft(const SpecArgs& a, float (*bufr)[NFFT], float (*bufi)[NFFT], int b, int f, long n, int j) {
  constexpr int NT = NFFT / 4;
  const float* wav = a.wav + (long)b * a.ldw;
  const long start = (long)f * a.hop - (NFFT - a.hop) / 2;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * NT;
    long i = start + m;
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    bufr[0][m] = wav[i] * a.window[m];                            // 0 <= i < n: n > p, and f < F keeps start + m < n + p
    bufi[0][m] = 0.f;
  }
  __syncthreads();
  return dx_fft_lds2<NFFT>(bufr, bufi, 0, a.twiddle, j);
}

// grid (T, B); NFFT / 4 threads
template <int NFFT>
__global__ __launch_bounds__(NFFT / 4) void spec_fwd_kernel(SpecArgs a) {
  constexpr int NT = NFFT / 4, NB = NFFT / 2 + 1;
  __shared__ float bufr[2][NFFT], bufi[2][NFFT];
  const int j = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  long n;
  const int F = spec_frames(a, b, NFFT, &n);
  float* out = a.mag + (long)b * NB * a.T + f;
  if (f >= F) {                                                   // frames past the utterance: zeros
    for (int k = j; k < NB; k += NT) out[(long)k * a.T] = 0.f;
    return;
  }
  const int cur = spec_frame_fft<NFFT>(a, bufr, bufi, b, f, n, j);
  for (int k = j; k < NB; k += NT) {
    const float re = bufr[cur][k], im = bufi[cur][k];
    out[(long)k * a.T] = sqrtf(re * re + im * im);
  }
}

// grid (T, B); NFFT / 4 threads.  Frames at or past F write nothing: launch 2 never reads them
template <int NFFT>
__global__ __launch_bounds__(NFFT / 4) void spec_bwd_frames_kernel(SpecArgs a) {
  constexpr int NT = NFFT / 4, NB = NFFT / 2 + 1;
  __shared__ float bufr[2][NFFT], bufi[2][NFFT];
  const int j = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  long n;
  const int F = spec_frames(a, b, NFFT, &n);
  if (f >= F) return;
  const int cur = spec_frame_fft<NFFT>(a, bufr, bufi, b, f, n, j);
  const float* g = a.dmag + (long)b * NB * a.T + f;
  // conj(G) into the other buffer: bins [0, NFFT / 2] from X (thread j owns j, j + NT and, for j = 0, NFFT / 2), zeros above
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = j + r * NT;
    float gr = 0.f, gi = 0.f;
    if (k < NB) {
      const float re = bufr[cur][k], im = bufi[cur][k];
      const float m = sqrtf(re * re + im * im);
      if (m > 0.f) {
        const float s = g[(long)k * a.T] / m;
        gr = s * re;
        gi = -(s * im);
      }
    }
    bufr[cur ^ 1][k] = gr;
    bufi[cur ^ 1][k] = gi;
  }
  __syncthreads();
  const int res = dx_fft_lds2<NFFT>(bufr, bufi, cur ^ 1, a.twiddle, j);
  float* dy = a.ws + ((long)b * a.T + f) * NFFT;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * NT;
    dy[m] = a.window[m] * bufr[res][m];
  }
}

struct SpecGatherArgs {
  const float* ws; const int64_t* n; float* dwav; long lddw;
  int S, T, hop, n_fft;
};

// dx~[s] of an utterance with F frames, s in [0, n + 2 p): the frames that cover s, in ascending order
__device__ __forceinline__ float spec_overlap_add(const float* ws, int s, int F, int n_fft, int hop) {
  const int lo = s >= n_fft ? (s - n_fft) / hop + 1 : 0;         // the first f with s - f hop < n_fft
  const int hi = min(s / hop, F - 1);
  float acc = 0.f;
  for (int f = lo; f <= hi; ++f) acc += ws[(long)f * n_fft + (s - f * hop)];
  return acc;
}

// grid (ceil(S / 256), B); 256 threads, one sample each
__global__ __launch_bounds__(256) void spec_bwd_gather_kernel(SpecGatherArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= a.S) return;
  const long n = (long)a.n[b];
  const int p = (a.n_fft - a.hop) / 2;
  float* out = a.dwav + (long)b * a.lddw + i;
  if (n <= p || n + 2L * p < a.n_fft || n > a.S || i >= n) { *out = 0.f; return; }
  const long Fl = 1 + (n + 2 * p - a.n_fft) / a.hop;
  const int F = (int)(Fl < a.T ? Fl : a.T);
  const float* ws = a.ws + (long)b * a.T * a.n_fft;
  float v = spec_overlap_add(ws, i + p, F, a.n_fft, a.hop);
  if (i >= 1 && i <= p) v += spec_overlap_add(ws, p - i, F, a.n_fft, a.hop);
  if (i >= n - 1 - p && i <= n - 2) v += spec_overlap_add(ws, (int)(p + 2 * (n - 1) - i), F, a.n_fft, a.hop);
  *out = v;
}

__global__ void spec_twiddle_kernel(float* __restrict__ twiddle, int n_fft) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_fft) return;
  double s, c;
  sincospi(2.0 * (double)t / (double)n_fft, &s, &c);
  twiddle[2 * t] = (float)c;
  twiddle[2 * t + 1] = (float)(-s);
}

// what both directions check before any launch; n_host: the B values of n_samples on the host
int spec_check(const char* who, const int64_t* n_host, int B, int S, int T, int n_fft, int hop) {
  DX_REQUIRE(dx_nfft2_ok(n_fft), DX_ERR_UNSUPPORTED, "%s: n_fft=%d unsupported (256, 512, 1024, 2048, 4096)", who, n_fft);
  DX_REQUIRE(hop >= 1 && hop <= n_fft, DX_ERR_UNSUPPORTED, "%s: hop=%d outside [1, n_fft=%d]", who, hop, n_fft);
  DX_REQUIRE(B > 0 && S > 0 && T > 0 && B <= 65535, DX_ERR_SHAPE, "%s: bad shape B=%d S=%d T=%d", who, B, S, T);
  const long p = (n_fft - hop) / 2;
  for (int b = 0; b < B; ++b) {
    const long n = (long)n_host[b];
    DX_REQUIRE(n > p && n + 2 * p >= n_fft, DX_ERR_UNSUPPORTED,
               "%s: utterance %d has %ld samples; reflect padding of %ld per side needs more than %ld, and one frame n + 2 p >= %d",
               who, b, n, p, p, n_fft);
    DX_REQUIRE(n <= S, DX_ERR_SHAPE, "%s: utterance %d has %ld samples, the rows hold S=%d", who, b, n, S);
    DX_REQUIRE(1 + (n + 2 * p - n_fft) / hop <= T, DX_ERR_SHAPE, "%s: utterance %d has %ld frames, T=%d", who, b,
               1 + (n + 2 * p - n_fft) / hop, T);
  }
  return DX_OK;
}

}  // namespace

extern "C" int dx_spectrogram_tables(float* twiddle, int n_fft, void* stream) {
  DX_REQUIRE(twiddle, DX_ERR_ARG, "dx_spectrogram_tables: null pointer");
  DX_REQUIRE(dx_nfft2_ok(n_fft), DX_ERR_UNSUPPORTED, "dx_spectrogram_tables: n_fft=%d unsupported (256, 512, 1024, 2048, 4096)", n_fft);
  hipLaunchKernelGGL(spec_twiddle_kernel, dim3(dx_cdiv(n_fft, 256)), dim3(256), 0, (hipStream_t)stream, twiddle, n_fft);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_spectrogram(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                              const float* window, float* mag, int B, int S, int T, int n_fft, int hop, void* stream) {
  DX_REQUIRE(wav && n_samples && n_samples_host && twiddle && window && mag, DX_ERR_ARG, "dx_spectrogram: null pointer");
  const int rc = spec_check("dx_spectrogram", n_samples_host, B, S, T, n_fft, hop);
  if (rc != DX_OK) return rc;
  DX_REQUIRE(ldw >= S, DX_ERR_SHAPE, "dx_spectrogram: ldw=%ld < S=%d", ldw, S);
  SpecArgs a{wav, ldw, n_samples, twiddle, window, mag, nullptr, nullptr, S, T, hop};
  dx_nfft2_dispatch(n_fft, [&](auto N) {
    constexpr int NFFT = decltype(N)::value;
    hipLaunchKernelGGL(spec_fwd_kernel<NFFT>, dim3(T, B), dim3(NFFT / 4), 0, (hipStream_t)stream, a);
  });
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" long dx_spectrogram_bwd_workspace(int B, int T, int n_fft) {
  if (B <= 0 || T <= 0 || n_fft <= 0) return 0;
  return (long)B * T * n_fft * (long)sizeof(float);
}

extern "C" int dx_spectrogram_bwd(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host,
                                  const float* twiddle, const float* window, const float* dmag, float* dwav, long lddw, void* ws,
                                  int B, int S, int T, int n_fft, int hop, void* stream) {
  DX_REQUIRE(wav && n_samples && n_samples_host && twiddle && window && dmag && dwav && ws, DX_ERR_ARG, "dx_spectrogram_bwd: null pointer");
  const int rc = spec_check("dx_spectrogram_bwd", n_samples_host, B, S, T, n_fft, hop);
  if (rc != DX_OK) return rc;
  DX_REQUIRE(ldw >= S && lddw >= S, DX_ERR_SHAPE, "dx_spectrogram_bwd: ldw=%ld or lddw=%ld < S=%d", ldw, lddw, S);
  SpecArgs a{wav, ldw, n_samples, twiddle, window, nullptr, dmag, (float*)ws, S, T, hop};
  dx_nfft2_dispatch(n_fft, [&](auto N) {
    constexpr int NFFT = decltype(N)::value;
    hipLaunchKernelGGL(spec_bwd_frames_kernel<NFFT>, dim3(T, B), dim3(NFFT / 4), 0, (hipStream_t)stream, a);
  });
  DX_LAUNCH_CHECK();
  SpecGatherArgs g{(const float*)ws, n_samples, dwav, lddw, S, T, hop, n_fft};
  hipLaunchKernelGGL(spec_bwd_gather_kernel, dim3(dx_cdiv(S, 256), B), dim3(256), 0, (hipStream_t)stream, g);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
