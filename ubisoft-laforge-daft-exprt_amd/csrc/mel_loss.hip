// K37 -- one scale of BigVGAN-v2's multi-scale mel loss as a kernel pair: the log10-mel of a waveform, and the L1 between that log-mel
// and a target's WITH its gradient back to the waveform.  It replaces, per scale, what `vocoder_train.LossMel` does for the single
// HiFi-GAN mel: a dense (n_fft, 2 bins) DFT matmul, a filter-bank matmul, log / clamp / abs as torch ops and an autograd graph over
// all of them.  Per utterance b (n = n_samples[b]), scale (n_fft, hop, p = reflect padding per side), window table w, filter bank fb:
//   x~[s] = x[r(s - p)] (torch's 'reflect'),   F = 1 + (n + 2 p - n_fft) div hop
//   X[f, k] = sum_j w[j] x~[f hop + j] exp(-2 pi i j k / n_fft),   mag = |X|,   mel[f, m] = sum_k fb[m, k] mag[f, k]
//   L[f, m] = log10(max(mel[f, m], eps))
// One launch over the frames does everything that belongs to a frame.  A frame is NFFT / 4 threads on its own ping-pong pair of
// dx_fft_lds2; a workgroup holds 256 / (NFFT / 4) consecutive frames (32 at 32 points, 1 from 1024 up), so no workgroup is below a
// wave of useful threads, and every frame of a workgroup runs the same stage count under the workgroup-wide barriers (a frame past the
// utterance's last computes on zeros and stores nothing).  The magnitudes stay in LDS; thread j of the frame projects the filters
// j, j + NFFT / 4, ... over their run of bins [fb_lo, fb_hi).  The loss kernel then forms
//   g[f, m]   = -sign(Tg - L) (mel >= eps) / (mel ln 10)          (to the workspace: M is not bounded by the frame's LDS)
//   dmag[k]   = sum_{m in [bin_lo[k], bin_hi[k])} fb[m, k] g[m]   (the transpose, per bin, over the bin's run of filters)
//   G[k]      = dmag X / |X| (0 where |X| = 0),  dy_f[j] = w[j] Re FFT(conj G)[j]      (the forward FFT again, as K36)
// and leaves dy_f and the frame's loss term (a tree over the frame's threads) in the workspace.  A second launch, one thread per sample,
// gathers dwav as K36's gather does (ascending frames, then the two reflect folds, then the scale), and its first workgroup per
// utterance sums the frame terms in a fixed order.  No atomics: the same bits twice, alone, in any batch and at any T.
#include "dx_fft.h"

namespace {

template <typename F>
inline bool mel_nfft_dispatch(int n_fft, F&& f) {
  switch (n_fft) {
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
    case 256: f(std::integral_constant<int, 256>{}); return true;
    case 512: f(std::integral_constant<int, 512>{}); return true;
    case 1024: f(std::integral_constant<int, 1024>{}); return true;
    case 2048: f(std::integral_constant<int, 2048>{}); return true;
  }
  return false;
}
inline bool mel_nfft_ok(int n_fft) { return mel_nfft_dispatch(n_fft, [](auto) {}); }

constexpr int mel_fpw(int n_fft) { return n_fft / 4 >= 256 ? 1 : 256 / (n_fft / 4); }      // frames per workgroup
constexpr int mel_threads(int n_fft) { return mel_fpw(n_fft) * (n_fft / 4); }            // 256; 512 at 2048 points
constexpr float MEL_LN10 = 2.302585092994046f;

struct MelArgs {
  const float* wav; long ldw; const int64_t* n; const float* twiddle; const float* window;
  const float* fb; const int* fb_lo; const int* fb_hi; const int* bin_lo; const int* bin_hi;
  const float* target;   // loss: (B, T, M)
  float* log_mel;        // (B, T, M); the loss kernel: may be null
  float* ws_dy;          // loss: (B, T, n_fft)
  float* ws_g;           // loss: (B, T, M)
  float* ws_loss;        // loss: (B, T)
  int S, T, M, hop, pad;
  float eps, log_eps;    // log_eps: log10(eps) taken in double on the host and rounded once -- what L is wherever the clamp holds
};

// live samples and frames of utterance b; 0 frames where the padding is not defined (n <= p), no frame fits, or n exceeds the row
__device__ __forceinline__ int mel_frames(const int64_t* n_samples, int b, int n_fft, int hop, int pad, int S, int T, long* n_out) {
  const long n = (long)n_samples[b], p = pad;
  *n_out = n;
  if (n <= p || n + 2 * p < n_fft || n > S) return 0;
  const long F = 1 + (n + 2 * p - n_fft) / hop;
  return (int)(F < T ? F : T);
}

// grid (ceil(T / FPW), B); FPW * NFFT / 4 threads
template <int NFFT, bool LOSS>
__global__ __launch_bounds__(mel_threads(NFFT)) void mel_frames_kernel(MelArgs a) {
  constexpr int NT = NFFT / 4, NB = NFFT / 2 + 1, FPW = mel_fpw(NFFT);
  constexpr int PAD = NT < 32 ? NT : 0;                            // frames that share a half-wave start on different banks
  __shared__ float sr[FPW][2 * NFFT + PAD], si[FPW][2 * NFFT + PAD];
  const int g = threadIdx.x / NT, j = threadIdx.x % NT, b = blockIdx.y;
  const int f = blockIdx.x * FPW + g;
  long n;
  const int F = mel_frames(a.n, b, NFFT, a.hop, a.pad, a.S, a.T, &n);
  const long row = ((long)b * a.T + f) * a.M;
  if (blockIdx.x * FPW >= F) {                                      // every frame of the workgroup is past the utterance: zeros
    if (a.log_mel && f < a.T)
      for (int m = j; m < a.M; m += NT) a.log_mel[row + m] = 0.f;
    return;
  }
  const bool live = f < F;
  float (*bufr)[NFFT] = reinterpret_cast<float (*)[NFFT]>(sr[g]);
  float (*bufi)[NFFT] = reinterpret_cast<float (*)[NFFT]>(si[g]);
  const float* wav = a.wav + (long)b * a.ldw;
  const long start = (long)f * a.hop - a.pad;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * NT;
    float v = 0.f;
    if (live) {
      long i = start + m;
      if (i < 0) i = -i;
      if (i >= n) i = 2 * (n - 1) - i;
      v = wav[i] * a.window[m];                                    // 0 <= i < n: n > p, and f < F keeps start + m < n + p
    }
    bufr[0][m] = v;
    bufi[0][m] = 0.f;
  }
  __syncthreads();
  const int cur = dx_fft_lds2<NFFT>(bufr, bufi, 0, a.twiddle, j);
  float* mag = bufr[cur ^ 1];
  for (int k = j; k < NB; k += NT) {
    const float re = bufr[cur][k], im = bufi[cur][k];
    mag[k] = sqrtf(re * re + im * im);
  }
  __syncthreads();
  float part = 0.f;
  for (int m = j; m < a.M; m += NT) {
    const int lo = max(a.fb_lo[m], 0), hi = min(a.fb_hi[m], NB);
    const float* w = a.fb + (long)m * NB;
    float mel = 0.f;
    for (int k = lo; k < hi; ++k) mel += w[k] * mag[k];
    const float L = mel >= a.eps ? log10f(mel) : a.log_eps;        // log10(max(mel, eps))
    if (a.log_mel && f < a.T) a.log_mel[row + m] = live ? L : 0.f;
    if (LOSS && live) {
      const float d = a.target[row + m] - L;
      part += fabsf(d);
      const float s = d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f);      // -sign(Tg - L)
      a.ws_g[row + m] = mel >= a.eps ? s / (mel * MEL_LN10) : 0.f;
    }
  }
  if (!LOSS) return;
  // the frame's loss term: a tree over its NT threads (an order NT alone fixes).  The barriers also order g's stores before its reads
  float* red = bufi[cur ^ 1];
  red[j] = part;
  __syncthreads();
#pragma unroll
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (j < s) red[j] += red[j + s];
    __syncthreads();
  }
  if (live && j == 0) a.ws_loss[(long)b * a.T + f] = red[0];
  // conj(G) into the free pair: bins [0, NFFT / 2] from X (thread j owns j, j + NT and, for j = 0, NFFT / 2), zeros above
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = j + r * NT;
    float gr = 0.f, gi = 0.f;
    if (live && k < NB) {
      const float re = bufr[cur][k], im = bufi[cur][k];
      const float m2 = sqrtf(re * re + im * im);
      if (m2 > 0.f) {
        const int lo = max(a.bin_lo[k], 0), hi = min(a.bin_hi[k], a.M);
        float dm = 0.f;
        for (int m = lo; m < hi; ++m) dm += a.fb[(long)m * NB + k] * a.ws_g[row + m];
        const float s = dm / m2;
        gr = s * re;
        gi = -(s * im);
      }
    }
    bufr[cur ^ 1][k] = gr;
    bufi[cur ^ 1][k] = gi;
  }
  __syncthreads();
  const int res = dx_fft_lds2<NFFT>(bufr, bufi, cur ^ 1, a.twiddle, j);
  if (!live) return;
  float* dy = a.ws_dy + ((long)b * a.T + f) * NFFT;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = j + r * NT;
    dy[m] = a.window[m] * bufr[res][m];
  }
}

struct MelGatherArgs {
  const float* ws_dy; const float* ws_loss; const int64_t* n; float* dwav; long lddw; float* loss;
  float scale;
  int S, T, hop, n_fft, pad;
};

// dx~[s] of an utterance with F frames, s in [0, n + 2 p): the frames that cover s, in ascending order
__device__ __forceinline__ float mel_overlap_add(const float* ws, int s, int F, int n_fft, int hop) {
  const int lo = s >= n_fft ? (s - n_fft) / hop + 1 : 0;         // the first f with s - f hop < n_fft
  const int hi = min(s / hop, F - 1);
  float acc = 0.f;
  for (int f = lo; f <= hi; ++f) acc += ws[(long)f * n_fft + (s - f * hop)];
  return acc;
}

// grid (ceil(S / 256), B); 256 threads, one sample each; the first workgroup of an utterance also sums its frames' loss terms
__global__ __launch_bounds__(256) void mel_gather_kernel(MelGatherArgs a) {
  __shared__ float red[4];
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  long n;
  const int F = mel_frames(a.n, b, a.n_fft, a.hop, a.pad, a.S, a.T, &n);
  if (i < a.S) {
    float v = 0.f;
    if (F > 0 && i < n) {
      const int p = a.pad;
      const float* ws = a.ws_dy + (long)b * a.T * a.n_fft;
      v = mel_overlap_add(ws, i + p, F, a.n_fft, a.hop);
      if (i >= 1 && i <= p) v += mel_overlap_add(ws, p - i, F, a.n_fft, a.hop);
      if (i >= n - 1 - p && i <= n - 2) v += mel_overlap_add(ws, (int)(p + 2 * (n - 1) - i), F, a.n_fft, a.hop);
      v *= a.scale;
    }
    a.dwav[(long)b * a.lddw + i] = v;
  }
  if (blockIdx.x == 0) {                                           // thread t: frames t, t + 256, ...; then the workgroup's fixed order
    float s = 0.f;
    for (int f = threadIdx.x; f < F; f += 256) s += a.ws_loss[(long)b * a.T + f];
    s = dx_block_sum<4, false>(s, red);
    if (threadIdx.x == 0) a.loss[b] = s;
  }
}

__global__ void mel_twiddle_kernel(float* __restrict__ twiddle, int n_fft) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_fft) return;
  double s, c;
  sincospi(2.0 * (double)t / (double)n_fft, &s, &c);
  twiddle[2 * t] = (float)c;
  twiddle[2 * t + 1] = (float)(-s);
}

// what both entry points check before any launch; n_host: the B values of n_samples on the host
int mel_check(const char* who, const int64_t* n_host, int B, int S, int T, int M, int n_fft, int hop, int pad, float eps) {
  DX_REQUIRE(mel_nfft_ok(n_fft), DX_ERR_UNSUPPORTED, "%s: n_fft=%d unsupported (32, 64, 128, 256, 512, 1024, 2048)", who, n_fft);
  DX_REQUIRE(hop >= 1 && hop <= n_fft, DX_ERR_UNSUPPORTED, "%s: hop=%d outside [1, n_fft=%d]", who, hop, n_fft);
  DX_REQUIRE(M >= 1, DX_ERR_UNSUPPORTED, "%s: M=%d filters, at least one is needed", who, M);
  DX_REQUIRE(eps > 0.f, DX_ERR_UNSUPPORTED, "%s: eps=%g is not positive", who, (double)eps);
  DX_REQUIRE(pad >= 0, DX_ERR_ARG, "%s: pad=%d is negative", who, pad);
  DX_REQUIRE(B > 0 && S > 0 && T > 0 && B <= 65535, DX_ERR_SHAPE, "%s: bad shape B=%d S=%d T=%d", who, B, S, T);
  const long p = pad;
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

extern "C" int dx_mel_loss_tables(float* twiddle, int n_fft, void* stream) {
  DX_REQUIRE(twiddle, DX_ERR_ARG, "dx_mel_loss_tables: null pointer");
  DX_REQUIRE(mel_nfft_ok(n_fft), DX_ERR_UNSUPPORTED, "dx_mel_loss_tables: n_fft=%d unsupported (32, 64, 128, 256, 512, 1024, 2048)", n_fft);
  hipLaunchKernelGGL(mel_twiddle_kernel, dim3(dx_cdiv(n_fft, 256)), dim3(256), 0, (hipStream_t)stream, twiddle, n_fft);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_mel_loss_log_mel(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                                   const float* window, const float* fb, const int* fb_lo, const int* fb_hi, float* log_mel, int B, int S,
                                   int T, int M, int n_fft, int hop, int pad, float eps, void* stream) {
  DX_REQUIRE(wav && n_samples && n_samples_host && twiddle && window && fb && fb_lo && fb_hi && log_mel, DX_ERR_ARG,
             "dx_mel_loss_log_mel: null pointer");
  const int rc = mel_check("dx_mel_loss_log_mel", n_samples_host, B, S, T, M, n_fft, hop, pad, eps);
  if (rc != DX_OK) return rc;
  DX_REQUIRE(ldw >= S, DX_ERR_SHAPE, "dx_mel_loss_log_mel: ldw=%ld < S=%d", ldw, S);
  MelArgs a{wav, ldw, n_samples, twiddle, window, fb, fb_lo, fb_hi, nullptr, nullptr, nullptr, log_mel, nullptr, nullptr, nullptr,
            S, T, M, hop, pad, eps, (float)log10((double)eps)};
  mel_nfft_dispatch(n_fft, [&](auto N) {
    constexpr int NFFT = decltype(N)::value;
    hipLaunchKernelGGL((mel_frames_kernel<NFFT, false>), dim3(dx_cdiv(T, mel_fpw(NFFT)), B), dim3(mel_threads(NFFT)), 0,
                       (hipStream_t)stream, a);
  });
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" long dx_mel_loss_workspace(int B, int T, int M, int n_fft) {
  if (B <= 0 || T <= 0 || M <= 0 || n_fft <= 0) return 0;
  return (long)B * T * ((long)n_fft + M + 1) * (long)sizeof(float);
}

extern "C" int dx_mel_loss(const float* wav, long ldw, const int64_t* n_samples, const int64_t* n_samples_host, const float* twiddle,
                           const float* window, const float* fb, const int* fb_lo, const int* fb_hi, const int* bin_lo, const int* bin_hi,
                           const float* target, float scale, float* loss, float* dwav, long lddw, float* log_mel, void* ws, int B, int S,
                           int T, int M, int n_fft, int hop, int pad, float eps, void* stream) {
  DX_REQUIRE(wav && n_samples && n_samples_host && twiddle && window && fb && fb_lo && fb_hi && bin_lo && bin_hi && target && loss && dwav && ws,
             DX_ERR_ARG, "dx_mel_loss: null pointer");
  const int rc = mel_check("dx_mel_loss", n_samples_host, B, S, T, M, n_fft, hop, pad, eps);
  if (rc != DX_OK) return rc;
  DX_REQUIRE(ldw >= S && lddw >= S, DX_ERR_SHAPE, "dx_mel_loss: ldw=%ld or lddw=%ld < S=%d", ldw, lddw, S);
  float* dy = (float*)ws;
  float* g = dy + (long)B * T * n_fft;
  float* terms = g + (long)B * T * M;
  MelArgs a{wav, ldw, n_samples, twiddle, window, fb, fb_lo, fb_hi, bin_lo, bin_hi, target, log_mel, dy, g, terms, S, T, M, hop, pad, eps,
            (float)log10((double)eps)};
  mel_nfft_dispatch(n_fft, [&](auto N) {
    constexpr int NFFT = decltype(N)::value;
    hipLaunchKernelGGL((mel_frames_kernel<NFFT, true>), dim3(dx_cdiv(T, mel_fpw(NFFT)), B), dim3(mel_threads(NFFT)), 0,
                       (hipStream_t)stream, a);
  });
  DX_LAUNCH_CHECK();
  MelGatherArgs ga{dy, terms, n_samples, dwav, lddw, loss, scale, S, T, hop, n_fft, pad};
  hipLaunchKernelGGL(mel_gather_kernel, dim3(dx_cdiv(S, 256), B), dim3(256), 0, (hipStream_t)stream, ga);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
