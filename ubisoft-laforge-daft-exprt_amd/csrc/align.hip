// K27: synthesis-based forced alignment -- the two steps between a DTW path (K25, csrc/dtw_eval.hip) and the phoneme boundaries
// of a recording.  dx_active_span finds the sounding stretch of a recording from its frame energies (what an aligner's silence
// trimming does); dx_dtw_transfer carries the frame counts the model gave each symbol of its synthesis over the path of a DTW
// against the recording: per sounding symbol the first recording frame matched to its first synthesis frame, repaired so that every
// sounding symbol keeps at least min_frames frames.
//
// Both are integer decisions on top of fp32 comparisons: a row / a pair gives the same bits alone, in any batch and with any padded
// extent.  The transfer keeps, per synthesis frame j, the smallest i the path pairs it with in LDS (an integer minimum: its result
// does not depend on the order the path entries arrive in), then walks the symbols a wave at a time with the wave scans of
// dx_common.h; only the repair of the starts is serial, over at most n_gen values in LDS.
#include "dx_common.h"

namespace {

constexpr int ALN_MAX_LEN = 4096;      // longest sequence of a pair: dx_dtw_max_len(); LDS: two arrays of 4096 ints = 32 KiB
constexpr int ALN_NONE = 0x7fffffff;   // a synthesis frame the path never visits
constexpr int SPAN_THREADS = 256;
constexpr int SPAN_WAVES = SPAN_THREADS / 64;

// ---- the sounding stretch of a row of frame energies -------------------------------------------------------------------------------
__global__ __launch_bounds__(SPAN_THREADS) void active_span_kernel(const float* __restrict__ energy, long ld,
                                                                   const int64_t* __restrict__ n_frames, float factor,
                                                                   int64_t* __restrict__ begin, int64_t* __restrict__ end, int T) {
  __shared__ float s_peak[SPAN_WAVES];
  __shared__ int s_idx[SPAN_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = (int)dx_clamp_len(n_frames, b, T);
  const float* e = energy + (long)b * ld;
  float peak = -__builtin_inff();
  for (int t = tid; t < n; t += SPAN_THREADS) peak = fmaxf(peak, e[t]);
  peak = dx_block_max<SPAN_WAVES>(peak, s_peak);
  int first = T, last = -1;
  if (peak > 0.f) {                                             // (uniform over the workgroup)
    const float thr = peak * factor;
    for (int t = tid; t < n; t += SPAN_THREADS)
      if (e[t] >= thr) { first = min(first, t); last = max(last, t); }
  }
  first = dx_block_min<SPAN_WAVES>(first, s_idx);
  last = dx_block_max<SPAN_WAVES>(last, s_idx);
  if (tid == 0) {
    begin[b] = last >= 0 ? first : 0;
    end[b] = last >= 0 ? last + 1 : 0;
  }
}

// ---- symbol durations over a DTW path ------------------------------------------------------------------------------------------------
// one chunk of 64 symbols: the lane's duration (0 behind n_symbols; clamped to [0, n_gen + 1], which keeps the sums small and
// changes neither the validity checks nor a valid row), its first synthesis frame and its rank among the sounding symbols
struct AlnSymbol { long d, g; int k, sounding; };
__device__ __forceinline__ AlnSymbol aln_symbol(const int64_t* __restrict__ dur, int s, int ns, int ng, long& sum, int& K, int lane) {
  const long raw = s < ns ? (long)dur[s] : 0;
  AlnSymbol y;
  y.d = min(max(raw, 0L), (long)ng + 1);
  y.sounding = y.d > 0 ? 1 : 0;
  y.g = sum + dx_wave_scan(y.d, lane) - y.d;
  y.k = K + dx_wave_scan(y.sounding, lane) - y.sounding;
  sum += dx_wave_sum(y.d);
  K += dx_wave_sum(y.sounding);
  return y;
}

__global__ __launch_bounds__(64) void dtw_transfer_kernel(const int* __restrict__ path, const int* __restrict__ path_len,
                                                          const int64_t* __restrict__ n_ref, const int64_t* __restrict__ n_gen,
                                                          const int64_t* __restrict__ gen_durations,
                                                          const int64_t* __restrict__ n_symbols, int64_t* __restrict__ rec_durations,
                                                          int* __restrict__ moved, int* __restrict__ status, int T_ref, int T_gen,
                                                          int L, int min_frames) {
  __shared__ int s_first[ALN_MAX_LEN];                          // per synthesis frame: the first recording frame on the path
  __shared__ int s_a[ALN_MAX_LEN];                              // per sounding symbol: its start in the recording
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nr = (int)dx_clamp_len(n_ref, b, T_ref), ng = (int)dx_clamp_len(n_gen, b, T_gen), ns = (int)dx_clamp_len(n_symbols, b, L);
  const int P = T_ref + T_gen - 1;
  const int len = min(max(path_len[b], 0), P);
  const int* pp = path + (long)b * P * 2;
  const int64_t* dur = gen_durations + (long)b * L;
  int64_t* out = rec_durations + (long)b * L;

  for (int j = lane; j < ng; j += 64) s_first[j] = ALN_NONE;
  __syncthreads();
  for (int p = lane; p < len; p += 64) {
    const int i = pp[2 * p], j = pp[2 * p + 1];
    if (i < 0 || i >= nr || j < 0 || j >= ng) continue;         // not a cell of this pair
    atomicMin(&s_first[j], i);
  }
  __syncthreads();

  // the symbols, a wave at a time: totals, validity and the raw starts
  long sum = 0;
  int K = 0, bad = 0;
  for (int s0 = 0; s0 < ns; s0 += 64) {
    const int s = s0 + lane;
    if (s < ns && dur[s] < 0) bad = 1;
    const AlnSymbol y = aln_symbol(dur, s, ns, ng, sum, K, lane);
    if (y.sounding) {
      const int a = y.g < ng ? s_first[y.g] : ALN_NONE;
      if (a != ALN_NONE && y.k < ALN_MAX_LEN) s_a[y.k] = a; else bad = 1;
    }
  }
  bad = dx_wave_sum(bad);
  const int st = (len == 0 || K == 0 || bad != 0 || sum != (long)ng) ? 2 : ((long)nr < (long)min_frames * K ? 1 : 0);
  __syncthreads();
  if (st == 0 && lane == 0) {                                   // status 0: K <= n_gen <= ALN_MAX_LEN and K * min_frames <= n_ref
    for (int k = 1; k < K; ++k) s_a[k] = max(s_a[k], s_a[k - 1] + min_frames);
    for (int k = 0; k < K; ++k) s_a[k] = min(s_a[k], nr - min_frames * (K - k));
  }
  __syncthreads();

  // every element of the row is written
  long sum2 = 0;
  int K2 = 0, mv = 0;
  for (int s0 = 0; s0 < L; s0 += 64) {
    const int s = s0 + lane;
    const AlnSymbol y = aln_symbol(dur, s, ns, ng, sum2, K2, lane);
    long r = 0;
    if (st == 0 && y.sounding) {
      const int a = s_a[y.k];
      r = (long)((y.k + 1 < K ? s_a[y.k + 1] : nr) - a);
      mv += a != s_first[y.g] ? 1 : 0;
    }
    if (s < L) out[s] = r;
  }
  mv = dx_wave_sum(mv);
  if (lane == 0) { moved[b] = mv; status[b] = st; }
}

}  // namespace

extern "C" int dx_active_span(const float* energy, long ld, const int64_t* n_frames, float rel_db, int64_t* begin, int64_t* end, int B,
                              int T, void* stream) {
  DX_REQUIRE(energy && n_frames && begin && end, DX_ERR_ARG, "dx_active_span: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && (B == 1 || ld >= T), DX_ERR_SHAPE, "dx_active_span: bad shape B=%d T=%d ld=%ld", B, T, ld);
  DX_REQUIRE(rel_db <= 0.f, DX_ERR_ARG, "dx_active_span: rel_db=%g (a level relative to the peak: <= 0)", (double)rel_db);
  const float factor = (float)pow(10.0, (double)rel_db / 20.0);
  hipLaunchKernelGGL(active_span_kernel, dim3(B), dim3(SPAN_THREADS), 0, (hipStream_t)stream, energy, ld, n_frames, factor, begin, end,
                     T);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_dtw_transfer(const int* path, const int* path_len, const int64_t* n_ref, const int64_t* n_gen,
                               const int64_t* gen_durations, const int64_t* n_symbols, int64_t* rec_durations, int* moved, int* status,
                               int B, int T_ref, int T_gen, int L, int min_frames, void* stream) {
  DX_REQUIRE(path && path_len && n_ref && n_gen && gen_durations && n_symbols && rec_durations && moved && status, DX_ERR_ARG,
             "dx_dtw_transfer: null pointer");
  DX_REQUIRE(B > 0 && T_ref > 0 && T_gen > 0 && L > 0, DX_ERR_SHAPE, "dx_dtw_transfer: bad shape B=%d T_ref=%d T_gen=%d L=%d", B, T_ref,
             T_gen, L);
  DX_REQUIRE(min_frames >= 1, DX_ERR_ARG, "dx_dtw_transfer: min_frames=%d (at least 1)", min_frames);
  DX_REQUIRE(T_ref <= ALN_MAX_LEN && T_gen <= ALN_MAX_LEN, DX_ERR_UNSUPPORTED,
             "dx_dtw_transfer: sequences of T_ref=%d, T_gen=%d frames (at most %d)", T_ref, T_gen, ALN_MAX_LEN);
  hipLaunchKernelGGL(dtw_transfer_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, path, path_len, n_ref, n_gen, gen_durations,
                     n_symbols, rec_durations, moved, status, T_ref, T_gen, L, min_frames);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
