// K20 -- pitch tracking, the stage the reference hands to a prebuilt REAPER binary (`extract_features.py:222-269`).  Not a port:
// the arithmetic is defined by tests/pitch_oracle.py (float64) and restated here; DESIGN 9d has the algorithm and its constants.
//   candidates: one workgroup per (analysis frame, utterance).  Frame a is centred on sample floor(a * step + 0.5), step =
//               sr * f0_interval.  The workgroup stages the span the frame reads (window + longest lag, zeros outside the
//               utterance) in LDS, lanes own lags: the cross term of every lag is summed in fp32 in tap order, the energies of the
//               lagged windows come from ONE running sum of squares over the span (kept in double: a difference of two fp32
//               prefixes would lose a quiet window that follows a loud one).  Local maxima of the normalised correlation are
//               interpolated through their neighbours and the K best kept in order of value.
//   viterbi:    one wave per utterance; lanes 0 .. K - 1 are the voiced candidates, lane K the unvoiced state.  The running
//               cost is re-based on its minimum at every frame (it stays of order one, so fp32 keeps its resolution over any
//               length).  Backpointers go to global scratch, lane 0 walks them back, then the wave gathers the analysis frames
//               to mel frames.
// Nothing depends on another utterance, and no sum is split by launch shape: a ragged batch gives each row bit for bit what
// the utterance gives alone.
#include "dx_common.h"

namespace {

constexpr int PT_K = 16;                       // candidates per frame (a steady 500 Hz tone has 12 period multiples in the default range)
constexpr int PT_THREADS = 256;
constexpr int PT_MAX_SPAN = 2048;              // staged samples per frame: window + longest lag + 1 (48 kHz, 40 Hz: 1921)
constexpr float PT_PEAK_MIN = 0.3f;
constexpr double PT_FLOOR_REL = 1e-2, PT_FLOOR_ABS = 1e-10;
constexpr float PT_LAG_WEIGHT = 0.3f;
constexpr float PT_UV_BASE = 0.5f;
constexpr float PT_FREQ_WEIGHT = 1.0f;
constexpr float PT_OCTAVE_COST = 0.35f;
constexpr float PT_VOICING_COST = 0.4f;
constexpr float PT_NO_STATE = 1e30f;
constexpr float PT_LN2 = 0.69314718055994530942f;

__device__ __forceinline__ int pt_n_analysis(long n, double step) { return 1 + (int)floor((double)n / step); }

// grid B: mean_sq[b] = mean of x^2 over the utterance, in double, summed in a fixed order (thread-strided, then a tree)
__global__ __launch_bounds__(PT_THREADS) void pt_mean_sq_kernel(const float* __restrict__ wav, long ldw, const int64_t* __restrict__ n_samples,
                                                                long S, double* __restrict__ mean_sq) {
  __shared__ double red[PT_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long n = dx_clamp_len(n_samples, b, S);
  const float* x = wav + (long)b * ldw;
  double s = 0.0;
  for (long i = tid; i < n; i += PT_THREADS) { const double v = x[i]; s += v * v; }
  red[tid] = s;
  __syncthreads();
  for (int off = PT_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) mean_sq[b] = n > 0 ? red[0] / (double)n : 0.0;
}

// grid (A, B); dynamic LDS: (span + 1) doubles, span + 3 * n_lags floats.  lag_lo = lag_min - 1, n_lags = lag_max - lag_min + 3,
// span = window + lag_max + 1.  cand_lag / cand_val (B, A, PT_K); frames past the utterance's last are written as zeros.
__global__ __launch_bounds__(PT_THREADS) void pt_candidates_kernel(const float* __restrict__ wav, long ldw, const int64_t* __restrict__ n_samples,
                                                                   const double* __restrict__ mean_sq, float* __restrict__ cand_lag,
                                                                   float* __restrict__ cand_val, long S, int A, double step, int window,
                                                                   int lag_min, int lag_max) {
  extern __shared__ double pt_lds[];
  const int n_lags = lag_max - lag_min + 3, lag_lo = lag_min - 1, span = window + lag_max + 1;
  double* pre = pt_lds;                                  // pre[i] = sum of xs[0 .. i)^2
  float* xs = reinterpret_cast<float*>(pre + span + 1);
  float* r = xs + span;
  float* pv = r + n_lags;                                // interpolated value of the peak at lag index j, -1 where none
  float* pl = pv + n_lags;                               // its interpolated lag
  __shared__ float out_lag[PT_K], out_val[PT_K];
  const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long n = dx_clamp_len(n_samples, b, S);
  float* ol = cand_lag + ((long)b * A + a) * PT_K;
  float* ov = cand_val + ((long)b * A + a) * PT_K;
  if (a >= pt_n_analysis(n, step)) {
    if (tid < PT_K) { ol[tid] = 0.f; ov[tid] = 0.f; }
    return;
  }
  const long s0 = (long)floor((double)a * step + 0.5) - window / 2;
  const float* x = wav + (long)b * ldw;
  for (int i = tid; i < span; i += PT_THREADS) {
    const long s = s0 + i;
    xs[i] = (s >= 0 && s < n) ? x[s] : 0.f;
  }
  if (tid < PT_K) { out_lag[tid] = 0.f; out_val[tid] = 0.f; }
  __syncthreads();
  if (tid < 64) {                                        // running sum of squares: 64 contiguous chunks, scanned across the wave
    const int chunk = (span + 63) / 64, i0 = min(tid * chunk, span), i1 = min(i0 + chunk, span);
    double s = 0.0;
    for (int i = i0; i < i1; ++i) { const double v = xs[i]; s += v * v; }
    const double incl = dx_wave_scan(s, tid);
    double run = incl - s;
    for (int i = i0; i < i1; ++i) { pre[i] = run; const double v = xs[i]; run += v * v; }
    if (tid == 63) pre[span] = incl;
  }
  __syncthreads();
  const float floor_e = (float)((double)window * (PT_FLOOR_REL * mean_sq[b] + PT_FLOOR_ABS));
  const float e0 = (float)(pre[window] - pre[0]);
  for (int j = tid; j < n_lags; j += PT_THREADS) {
    const int k = lag_lo + j;
    const float* xl = xs + k;
    float acc = 0.f;
    for (int i = 0; i < window; ++i) acc = fmaf(xs[i], xl[i], acc);
    const float ek = (float)(pre[k + window] - pre[k]);
    r[j] = acc / (sqrtf(e0 * ek) + floor_e);
  }
  __syncthreads();
  for (int j = tid; j < n_lags; j += PT_THREADS) {
    float val = -1.f, lag = 0.f;
    if (j >= 1 && j <= n_lags - 2) {
      const float rm = r[j - 1], rc = r[j], rp = r[j + 1];
      if (rc > rm && rc >= rp && rc > PT_PEAK_MIN) {
        const float d = 0.5f * (rm - rp) / (rm - 2.f * rc + rp);
        val = rc - 0.25f * (rm - rp) * d;
        lag = (float)(lag_lo + j) + d;
      }
    }
    pv[j] = val;
    pl[j] = lag;
  }
  __syncthreads();
  for (int j = tid; j < n_lags; j += PT_THREADS) {
    const float val = pv[j], lag = pl[j];
    if (val < 0.f) continue;
    int rank = 0;
    for (int q = 1; q <= n_lags - 2; ++q) {
      const float v = pv[q];
      rank += (v > val || (v == val && pl[q] < lag)) ? 1 : 0;
    }
    if (rank < PT_K) { out_lag[rank] = lag; out_val[rank] = val; }
  }
  __syncthreads();
  if (tid < PT_K) { ol[tid] = out_lag[tid]; ov[tid] = out_val[tid]; }
}

// grid B, one wave.  back (B, A, PT_K + 1) bytes and hz (B, A) floats are scratch and output; log_pitch (B, T).
__global__ __launch_bounds__(64) void pt_viterbi_kernel(const float* __restrict__ cand_lag, const float* __restrict__ cand_val,
                                                        const int64_t* __restrict__ n_samples, unsigned char* __restrict__ back,
                                                        float* __restrict__ hz, float* __restrict__ log_pitch, int64_t* __restrict__ n_frames,
                                                        long S, int A, int T, int sr, double step, int hop, int lag_max, float uv_cost) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long n = dx_clamp_len(n_samples, b, S);
  const int Ab = min(pt_n_analysis(n, step), A);
  const float* cl = cand_lag + (long)b * A * PT_K;
  const float* cv = cand_val + (long)b * A * PT_K;
  unsigned char* bk = back + (long)b * A * (PT_K + 1);
  float* hzb = hz + (long)b * A;
  const bool voiced = lane < PT_K, state = lane <= PT_K;
  float cost = PT_NO_STATE, loglag = 0.f;
  float lag_n = voiced ? cl[lane] : 0.f, val_n = voiced ? cv[lane] : 0.f;
  for (int a = 0; a < Ab; ++a) {
    const float lag = lag_n, val = val_n;
    if (a + 1 < Ab && voiced) { lag_n = cl[(long)(a + 1) * PT_K + lane]; val_n = cv[(long)(a + 1) * PT_K + lane]; }
    const bool live = lag > 0.f;
    float local = PT_NO_STATE;
    if (voiced && live) local = 1.f - val * (1.f - PT_LAG_WEIGHT * lag / (float)lag_max);
    if (lane == PT_K) local = uv_cost * PT_UV_BASE;
    const float ll = live ? logf(lag) : 0.f;
    float c = local;
    if (a > 0) {
      float best = 3e38f;
      int arg = 0;
#pragma unroll
      for (int p = 0; p <= PT_K; ++p) {
        const float cp = __shfl(cost, p, 64), lp = __shfl(loglag, p, 64);
        float t;
        if (voiced && p < PT_K) {
          const float d = fabsf(ll - lp);
          t = PT_FREQ_WEIGHT * fminf(d, PT_OCTAVE_COST + fabsf(d - PT_LN2));
        } else {
          t = (lane == PT_K && p == PT_K) ? 0.f : PT_VOICING_COST;
        }
        const float tot = cp + t;
        if (tot < best) { best = tot; arg = p; }       // first of equals: the lower state
      }
      c = local >= PT_NO_STATE ? PT_NO_STATE : best + local;
      if (state) bk[(long)a * (PT_K + 1) + lane] = (unsigned char)arg;
    }
    cost = c - dx_wave_min(c);
    loglag = ll;
  }
  float best = 3e38f;
  int st = 0;
#pragma unroll
  for (int p = 0; p <= PT_K; ++p) {
    const float cp = __shfl(cost, p, 64);
    if (cp < best) { best = cp; st = p; }
  }
  __threadfence_block();
  __syncthreads();
  if (lane == 0) {
    for (int a = Ab - 1; a >= 0; --a) {
      hzb[a] = st < PT_K ? (float)sr / cl[(long)a * PT_K + st] : 0.f;
      if (a > 0) st = bk[(long)a * (PT_K + 1) + st];
    }
  }
  for (int a = Ab + lane; a < A; a += 64) hzb[a] = 0.f;
  __threadfence_block();
  __syncthreads();
  const long nf = 1 + n / hop;
  if (lane == 0) n_frames[b] = nf;
  for (int t = lane; t < T; t += 64) {
    float v = 0.f;
    if (t < nf) {
      const int a = min((int)floor((double)((long)t * hop) / step + 0.5), Ab - 1);
      const float h = hzb[a];
      v = h > 0.f ? logf(h) : 0.f;
    }
    log_pitch[(long)b * T + t] = v;
  }
}

}  // namespace

extern "C" int dx_pitch_num_candidates(void) { return PT_K; }

extern "C" int dx_pitch_candidates(const float* wav, long ldw, const int64_t* n_samples, double* mean_sq, float* cand_lag,
                                   float* cand_val, int B, long S, int A, double step, int window, int lag_min, int lag_max,
                                   void* stream) {
  DX_REQUIRE(wav && n_samples && mean_sq && cand_lag && cand_val, DX_ERR_ARG, "dx_pitch_candidates: null pointer");
  DX_REQUIRE(B > 0 && S > 0 && ldw >= S && A > 0 && step >= 1.0 && window > 0 && lag_min >= 2 && lag_max > lag_min, DX_ERR_SHAPE,
             "dx_pitch_candidates: bad shape B=%d S=%ld ldw=%ld A=%d step=%g window=%d lags %d..%d", B, S, ldw, A, step, window, lag_min,
             lag_max);
  DX_REQUIRE((long)A >= 1 + (long)((double)S / step), DX_ERR_SHAPE, "dx_pitch_candidates: A=%d < 1 + floor(S / step) = %ld", A,
             1 + (long)((double)S / step));
  const int span = window + lag_max + 1, n_lags = lag_max - lag_min + 3;
  DX_REQUIRE(span <= PT_MAX_SPAN, DX_ERR_UNSUPPORTED, "dx_pitch_candidates: window %d + longest lag %d stages %d samples per frame (> %d)",
             window, lag_max, span, PT_MAX_SPAN);
  DX_REQUIRE(B <= 65535, DX_ERR_UNSUPPORTED, "dx_pitch_candidates: B=%d > 65535", B);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pt_mean_sq_kernel, dim3(B), dim3(PT_THREADS), 0, s, wav, ldw, n_samples, S, mean_sq);
  DX_LAUNCH_CHECK();
  const size_t lds = (size_t)(span + 1) * sizeof(double) + (size_t)(span + 3 * n_lags) * sizeof(float);
  hipLaunchKernelGGL(pt_candidates_kernel, dim3(A, B), dim3(PT_THREADS), lds, s, wav, ldw, n_samples, mean_sq, cand_lag, cand_val, S, A,
                     step, window, lag_min, lag_max);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_pitch_viterbi(const float* cand_lag, const float* cand_val, const int64_t* n_samples, unsigned char* back, float* hz,
                                float* log_pitch, int64_t* n_frames, int B, long S, int A, int T, int sr, double step, int hop,
                                int lag_max, float uv_cost, void* stream) {
  DX_REQUIRE(cand_lag && cand_val && n_samples && back && hz && log_pitch && n_frames, DX_ERR_ARG, "dx_pitch_viterbi: null pointer");
  DX_REQUIRE(B > 0 && S > 0 && A > 0 && T > 0 && sr > 0 && step >= 1.0 && hop > 0 && lag_max > 0, DX_ERR_SHAPE,
             "dx_pitch_viterbi: bad shape B=%d S=%ld A=%d T=%d sr=%d step=%g hop=%d lag_max=%d", B, S, A, T, sr, step, hop, lag_max);
  DX_REQUIRE((long)A >= 1 + (long)((double)S / step) && (long)T >= 1 + S / hop, DX_ERR_SHAPE,
             "dx_pitch_viterbi: A=%d, T=%d do not cover S=%ld samples (step %g, hop %d)", A, T, S, step, hop);
  hipLaunchKernelGGL(pt_viterbi_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cand_lag, cand_val, n_samples, back, hz, log_pitch,
                     n_frames, S, A, T, sr, step, hop, lag_max, uv_cost);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
