// K19 -- audio path of the vocoder fine-tuning data set (reference `fine_tune.py:91-115`):
//   resample:  what `librosa.load(wav, sr=hparams.sampling_rate)` does to a file of another rate (librosa 0.8.1 ->
//              resampy, res_type 'kaiser_best').  The phase of output sample t repeats every P = sr_out / gcd output
//              samples, so the host builds the (taps, P) polyphase bank of the windowed-sinc table once per rate pair and
//              the kernel is a gather FIR: one workgroup per (utterance, run of RS_TILE output samples) stages the input
//              span the run reads in LDS (zeros outside the utterance) and every output sums its taps in fp32 in tap order.
//              An output depends on its own utterance only, so a ragged batch gives each utterance's result bit for bit.
//   ft_pack:   crop every mel prediction to its length and every waveform to its marker span, convert the waveform to int16
//              (`(wav * 32768.0).astype('int16')`) and pack both back to back, so a batch leaves the device in one copy.
#include "dx_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 512;                  // output samples per workgroup
constexpr int RS_MAX_SPAN = 16384;            // staged input floats per workgroup (64 KiB of LDS)
constexpr long RS_MAX_WEIGHTS = 1L << 22;     // P * taps: 16 MiB of bank

__host__ __device__ inline long rs_gcd(long a, long b) {
  while (b) { const long t = a % b; a = b; b = t; }
  return a;
}

// grid (ceil(S_out / RS_TILE), B).  Output t < floor(n * P / Q) of utterance b:
//   y[t] = sum_j bank[j, t mod P] * x[floor(t Q / P) - (left - 1) + j],  x = 0 outside [0, n)
// outputs in [floor(n P / Q), S_out) are 0 (librosa's fix_length pads the ceiling sample).
__global__ __launch_bounds__(RS_THREADS) void rs_fir_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ n_in,
                                                           const float* __restrict__ bank, float* __restrict__ y, long ldy,
                                                           int64_t* __restrict__ n_out, long S_in, long S_out, long P, long Q,
                                                           int taps, int left) {
  extern __shared__ float xs[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * RS_TILE;
  const long t1 = min(t0 + RS_TILE, S_out);
  const long nb = dx_clamp_len(n_in, b, S_in);
  const long nf = nb * P / Q;
  if (blockIdx.x == 0 && tid == 0 && n_out) n_out[b] = (nb * P + Q - 1) / Q;
  float* yb = y + (long)b * ldy;
  if (t0 >= nf) {                                                  // past the utterance: zeros only
    for (long t = t0 + tid; t < t1; t += RS_THREADS) yb[t] = 0.f;
    return;
  }
  const long lo = t0 * Q / P - (left - 1);
  const long tl = min(t1, nf) - 1;
  const int span = (int)(tl * Q / P - (left - 1) + taps - lo);    // <= RS_MAX_SPAN (checked on the host side of the launch)
  const float* xb = x + (long)b * ldx;
  for (int i = tid; i < span; i += RS_THREADS) {
    const long s = lo + i;
    xs[i] = (s >= 0 && s < nb) ? xb[s] : 0.f;
  }
  __syncthreads();
  for (long t = t0 + tid; t < t1; t += RS_THREADS) {
    float acc = 0.f;
    if (t < nf) {
      const long n = t * Q / P;
      const float* xp = xs + (n - (left - 1) - lo);
      const float* w = bank + t % P;                                // tap-major bank: neighbouring lanes read neighbouring phases
      for (int j = 0; j < taps; ++j) acc = fmaf(w[(long)j * P], xp[j], acc);
    }
    yb[t] = acc;
  }
}

// equal rates: librosa returns the signal unchanged
__global__ __launch_bounds__(RS_THREADS) void rs_copy_kernel(const float* __restrict__ x, long ldx, const int64_t* __restrict__ n_in,
                                                            float* __restrict__ y, long ldy, int64_t* __restrict__ n_out, long S_in,
                                                            long S_out) {
  const int b = blockIdx.y;
  const long t = (long)blockIdx.x * RS_THREADS + threadIdx.x;
  const long nb = dx_clamp_len(n_in, b, S_in);
  if (t == 0 && n_out) n_out[b] = nb;
  if (t < S_out) y[(long)b * ldy + t] = t < nb ? x[(long)b * ldx + t] : 0.f;
}

// sum_{i < b} v(i) over the workgroup (every thread gets it); 256 threads
template <typename F>
__device__ __forceinline__ long ft_prefix(int b, F v, long* red) {
  long s = 0;
  for (int i = threadIdx.x; i < b; i += 256) s += v(i);
  return dx_block_sum<4, false>(s, red);                            // (one call per kernel: red is not used again)
}

__device__ __forceinline__ long ft_wav_len(const int64_t* crop, int i) { return max((long)crop[2 * i + 1], 0L); }

// grid (ceil(n_mel * T / 1024), B): mel_out[off_b + m * T_b + f] = mel[b, m, f], f < T_b = lengths[b]
__global__ __launch_bounds__(256) void ft_mel_kernel(const float* __restrict__ mel, long ld_mb, long ld_mk, const int64_t* __restrict__ len,
                                                     int n_mel, int T, float* __restrict__ out) {
  __shared__ long red[4];
  const int b = blockIdx.y;
  const long Tb = dx_clamp_len(len, b, T);
  const long off = (long)n_mel * ft_prefix(b, [&](int i) { return dx_clamp_len(len, i, T); }, red);
  const long n = (long)n_mel * Tb;
  for (long e = (long)blockIdx.x * 1024 + threadIdx.x; e < min(n, (long)(blockIdx.x + 1) * 1024); e += 256) {
    const long m = e / Tb, f = e - m * Tb;
    out[off + e] = mel[(long)b * ld_mb + m * ld_mk + f];
  }
}

// grid (ceil(S / 1024), B): wav_out[off_b + s] = sat16(trunc(wav[b, begin_b + s] * 32768)), s < len_b; 0 where begin_b + s
// falls outside [0, S)
__global__ __launch_bounds__(256) void ft_wav_kernel(const float* __restrict__ wav, long ldw, const int64_t* __restrict__ crop, long S,
                                                     int16_t* __restrict__ out) {
  __shared__ long red[4];
  const int b = blockIdx.y;
  const long n = ft_wav_len(crop, b), begin = crop[2 * b];
  const long off = ft_prefix(b, [&](int i) { return ft_wav_len(crop, i); }, red);
  for (long s = (long)blockIdx.x * 1024 + threadIdx.x; s < min(n, (long)(blockIdx.x + 1) * 1024); s += 256) {
    const long src = begin + s;
    const float v = (src >= 0 && src < S) ? wav[(long)b * ldw + src] * 32768.f : 0.f;
    int q;
    if (!(v == v)) q = 0;                                           // NaN
    else if (v >= 32767.f) q = 32767;
    else if (v <= -32768.f) q = -32768;
    else q = (int)v;                                                // truncation toward zero, as numpy's cast
    out[off + s] = (int16_t)q;
  }
}

}  // namespace

extern "C" long dx_resample_max_weights(void) { return RS_MAX_WEIGHTS; }

extern "C" int dx_resample(const float* x, long ldx, const int64_t* n_in, const float* bank, float* y, long ldy, int64_t* n_out,
                           int B, long S_in, long S_out, int sr_in, int sr_out, int taps, int left, void* stream) {
  DX_REQUIRE(x && n_in && y, DX_ERR_ARG, "dx_resample: null pointer");
  DX_REQUIRE(B > 0 && S_in > 0 && S_out > 0 && sr_in > 0 && sr_out > 0 && ldx >= S_in && ldy >= S_out, DX_ERR_SHAPE,
             "dx_resample: bad shape B=%d S_in=%ld S_out=%ld ldx=%ld ldy=%ld sr %d -> %d", B, S_in, S_out, ldx, ldy, sr_in, sr_out);
  const long g = rs_gcd(sr_in, sr_out), P = sr_out / g, Q = sr_in / g;
  DX_REQUIRE(S_out >= (S_in * P + Q - 1) / Q, DX_ERR_SHAPE, "dx_resample: S_out=%ld < ceil(S_in * %d / %d)", S_out, sr_out, sr_in);
  hipStream_t s = (hipStream_t)stream;
  if (P == Q) {
    hipLaunchKernelGGL(rs_copy_kernel, dim3((unsigned)((S_out + RS_THREADS - 1) / RS_THREADS), B), dim3(RS_THREADS), 0, s, x, ldx,
                       n_in, y, ldy, n_out, S_in, S_out);
    DX_LAUNCH_CHECK();
    return DX_OK;
  }
  DX_REQUIRE(bank, DX_ERR_ARG, "dx_resample: null bank");
  DX_REQUIRE(taps > 0 && left > 0 && left <= taps, DX_ERR_SHAPE, "dx_resample: bad taps=%d left=%d", taps, left);
  DX_REQUIRE(P * (long)taps <= RS_MAX_WEIGHTS, DX_ERR_UNSUPPORTED,
             "dx_resample: %d -> %d Hz needs a bank of %ld phases x %d taps > %ld weights", sr_in, sr_out, P, taps, RS_MAX_WEIGHTS);
  const long span = ((long)(RS_TILE - 1) * Q) / P + taps + 1;
  DX_REQUIRE(span <= RS_MAX_SPAN, DX_ERR_UNSUPPORTED, "dx_resample: %d -> %d Hz stages %ld input samples per workgroup (> %d)", sr_in,
             sr_out, span, RS_MAX_SPAN);
  hipLaunchKernelGGL(rs_fir_kernel, dim3((unsigned)((S_out + RS_TILE - 1) / RS_TILE), B), dim3(RS_THREADS), span * sizeof(float), s,
                     x, ldx, n_in, bank, y, ldy, n_out, S_in, S_out, P, Q, taps, left);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_ft_pack(const float* mel, long ld_mb, long ld_mk, const int64_t* lengths, int B, int n_mel, int T, const float* wav,
                          long ldw, const int64_t* crop, long S, float* mel_out, int16_t* wav_out, void* stream) {
  DX_REQUIRE(mel && lengths && wav && crop && mel_out && wav_out, DX_ERR_ARG, "dx_ft_pack: null pointer");
  DX_REQUIRE(B > 0 && n_mel > 0 && T > 0 && S > 0 && ldw >= S && ld_mk >= T && ld_mb >= (long)n_mel * ld_mk, DX_ERR_SHAPE,
             "dx_ft_pack: bad shape B=%d n_mel=%d T=%d S=%ld ldw=%ld ld_mb=%ld ld_mk=%ld", B, n_mel, T, S, ldw, ld_mb, ld_mk);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ft_mel_kernel, dim3((unsigned)(((long)n_mel * T + 1023) / 1024), B), dim3(256), 0, s, mel, ld_mb, ld_mk, lengths,
                     n_mel, T, mel_out);
  DX_LAUNCH_CHECK();
  hipLaunchKernelGGL(ft_wav_kernel, dim3((unsigned)((S + 1023) / 1024), B), dim3(256), 0, s, wav, ldw, crop, S, wav_out);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
