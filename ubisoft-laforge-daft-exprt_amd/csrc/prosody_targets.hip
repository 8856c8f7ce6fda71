// K29: per-symbol prosody targets -- from the frames of a recording to targets in the model's domain (dx_clone_pool), and their
// imposition on the prosody predictor's outputs at synthesis time (dx_prosody_impose in front of K16, dx_prosody_impose_durations
// behind it).  The contract is stated in include/daft_exprt_hip.h; DESIGN 9m has the reasoning.
//
// All three are latency-sized: one wave per utterance, the symbols 64 at a time, reductions through dx_common.h, fp64 sums whose
// order is fixed by the row alone, no atomics.  A row gives the same bits alone, in any batch and with any padded extent.
#include <vector>

#include "dx_common.h"

namespace {

constexpr int PT_ST_OVERRUN = 1;       // dx_clone_pool: the row's frames are not all inside [0, T)
constexpr int PT_ST_EMPTY = 3;         // dx_prosody_impose_durations: a frame-exact row without a single frame (K16 owns 1 and 2)
constexpr int PT_ST_WEIGHT = 4;        // ... a row with a weight outside [0, 1]

// The statistics of one pooled quantity and its standardisation.  Every lane re-reads the values it wrote itself (l = lane,
// lane + 64, ...), so no fence is needed between the passes.  lsum / lcnt: the lane's sum and count of its non-zero pooled values.
// Returns 1 when the quantity is dropped (its outputs are then all 0).
__device__ __forceinline__ int pt_standardise(float* __restrict__ sym, int L, int lane, double lsum, long lcnt, const float* given_mean,
                                              const float* given_std, int b, float* __restrict__ stats2) {
  const double sum = dx_wave_sum(lsum);
  const long n = dx_wave_sum(lcnt);
  const double mean = n ? sum / (double)n : 0.0;
  double q = 0.0;
  for (int l = lane; l < L; l += 64) {
    const float v = sym[l];
    if (v != 0.f) { const double c = (double)v - mean; q += c * c; }
  }
  q = dx_wave_sum(q);
  const float self_mean = (float)mean, self_std = n ? (float)sqrt(q / (double)n) : 0.f;
  if (lane == 0) { stats2[0] = self_mean; stats2[1] = self_std; }
  float m, s;
  int drop;
  if (given_mean) { m = given_mean[b]; s = given_std[b]; drop = !(s > 0.f); }
  else { m = self_mean; s = self_std; drop = n < 2 || !(s > 0.f); }
  for (int l = lane; l < L; l += 64) {
    const float v = sym[l];
    sym[l] = (drop || v == 0.f) ? 0.f : (v - m) / s;                       // data_loader._standardise: zeros stay zeros
  }
  return drop;
}

// One wave per utterance.  The pooling is symbol_pool_kernel's (csrc/features.hip) on the curves shifted by begin[b]: a wave scan
// gives every row of a chunk its first frame, then the wave reduces the rows one after the other, lane j adding frames j, j + 64, ...
// of the row in double before the fixed butterfly.
__global__ __launch_bounds__(64) void clone_pool_kernel(const float* __restrict__ energy, const float* __restrict__ log_pitch, long ldt,
                                                        const int64_t* __restrict__ begin, const int64_t* __restrict__ durations,
                                                        const int64_t* __restrict__ n_rows, const float* __restrict__ mean_e,
                                                        const float* __restrict__ std_e, const float* __restrict__ mean_p,
                                                        const float* __restrict__ std_p, float* __restrict__ sym_energy,
                                                        float* __restrict__ sym_pitch, float* __restrict__ raw_energy,
                                                        float* __restrict__ raw_pitch, float* __restrict__ self_stats,
                                                        int* __restrict__ dropped, int* __restrict__ status, int T, int L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t* d = durations + (long)b * L;
  float* oe = sym_energy + (long)b * L;
  float* op = sym_pitch + (long)b * L;
  const long rows = dx_clamp_len(n_rows, b, L);
  const long b0 = (long)begin[b];
  // the row's frames must lie inside [0, T): decided before anything is read
  long total = 0;
  int bad = b0 < 0 || b0 > T;
  for (long l = lane; l < rows; l += 64) {
    const long dl = (long)d[l];
    bad |= dl < 0;
    total += min(max(dl, 0L), (long)T + 1);                              // (keeps the sum small; a clamped row overruns anyway)
  }
  total = dx_wave_sum(total);
  bad = __ballot(bad) != 0;
  if (bad || b0 + total > T) {
    for (int l = lane; l < L; l += 64) {
      oe[l] = 0.f; op[l] = 0.f;
      if (raw_energy) raw_energy[(long)b * L + l] = 0.f;
      if (raw_pitch) raw_pitch[(long)b * L + l] = 0.f;
    }
    if (lane < 4) self_stats[4 * b + lane] = 0.f;
    if (lane == 0) { dropped[b] = 0; status[b] = PT_ST_OVERRUN; }
    return;
  }
  const float* e = energy + (long)b * ldt + b0;
  const float* p = log_pitch + (long)b * ldt + b0;
  double sum_e = 0.0, sum_p = 0.0;                                       // of the lane's own non-zero pooled values
  long cnt_e = 0, cnt_p = 0;
  long first = 0;                                                        // first frame of the chunk's first row
  for (long l0 = 0; l0 < L; l0 += 64) {
    const long l = l0 + lane;
    const long dl = l < rows ? (long)d[l] : 0;
    const long x = dx_wave_scan(dl, lane);
    const long start = first + x - dl;
    first += __shfl(x, 63, 64);
    float out_e = 0.f, out_p = 0.f;
    const int live = (int)min(64L, rows - l0);                           // rows of this chunk that exist (<= 0: none)
    for (int r = 0; r < live; ++r) {
      const long dr = __shfl(dl, r, 64), sr = __shfl(start, r, 64);
      if (dr == 0) continue;                                             // (wave-uniform)
      double se = 0.0, spv = 0.0;
      long voiced = 0;
      for (long f = sr + lane; f < sr + dr; f += 64) {                   // (sr + dr <= total <= T - b0)
        se += (double)e[f];
        const float pv = p[f];
        if (pv > 0.f) { spv += (double)pv; ++voiced; }
      }
      se = dx_wave_sum(se);
      spv = dx_wave_sum(spv);
      voiced = dx_wave_sum(voiced);
      if (lane == r) {
        out_e = (float)(se / (double)dr);
        out_p = voiced ? (float)(spv / (double)voiced) : 0.f;
      }
    }
    if (l < L) {
      oe[l] = out_e; op[l] = out_p;
      if (raw_energy) raw_energy[(long)b * L + l] = out_e;
      if (raw_pitch) raw_pitch[(long)b * L + l] = out_p;
      if (out_e != 0.f) { sum_e += (double)out_e; ++cnt_e; }
      if (out_p != 0.f) { sum_p += (double)out_p; ++cnt_p; }
    }
  }
  const int drop_e = pt_standardise(oe, L, lane, sum_e, cnt_e, mean_e, std_e, b, self_stats + 4 * b);
  const int drop_p = pt_standardise(op, L, lane, sum_p, cnt_p, mean_p, std_p, b, self_stats + 4 * b + 2);
  if (lane == 0) { dropped[b] = drop_e | (drop_p << 1); status[b] = 0; }
}

__device__ __forceinline__ bool pt_bad_weight(float w) { return !(w >= 0.f && w <= 1.f); }       // (NaN is bad)
// x moved towards t by w: nothing at 0 and t itself at 1, bit for bit
__device__ __forceinline__ float pt_blend(float x, float t, float w) { return w == 0.f ? x : (w == 1.f ? t : fmaf(w, t - x, x)); }
// a zero energy / pitch target says "silent" / "unvoiced": it is taken over from w = 0.5 on and ignored below
__device__ __forceinline__ float pt_blend_level(float x, float t, float w) { return t == 0.f ? (w >= 0.5f ? 0.f : x) : pt_blend(x, t, w); }
__device__ __forceinline__ float pt_seconds(long frames, int hop, double sr) { return (float)((double)frames * (double)hop / sr); }

// One wave per utterance.  CHECK_ONLY: only exact[b] is written (the host reads it to report a bad weight).
template <bool CHECK_ONLY>
__global__ __launch_bounds__(64) void prosody_impose_kernel(float* __restrict__ dur, float* __restrict__ energy, float* __restrict__ pitch,
                                                            const int64_t* __restrict__ t_dur, const float* __restrict__ t_energy,
                                                            const float* __restrict__ t_pitch, const float* __restrict__ w_dur,
                                                            const float* __restrict__ w_energy, const float* __restrict__ w_pitch,
                                                            const int64_t* __restrict__ lengths, const float* __restrict__ dur_factors,
                                                            int* __restrict__ exact, int L, int hop, double sr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long n = dx_clamp_len(lengths, b, L), row = (long)b * L;
  int bad = 0, inexact = t_dur == nullptr;
  for (long l = lane; l < n; l += 64) {
    if (t_dur) {
      const float w = w_dur[row + l];
      bad |= pt_bad_weight(w);
      if (t_dur[row + l] < 0 || w != 1.f || (dur_factors && dur_factors[row + l] != 1.f)) inexact = 1;
    }
    if (t_energy) bad |= pt_bad_weight(w_energy[row + l]);
    if (t_pitch) bad |= pt_bad_weight(w_pitch[row + l]);
  }
  bad = __ballot(bad) != 0;
  inexact = __ballot(inexact) != 0;
  if (lane == 0) exact[b] = bad ? -1 : (inexact ? 0 : 1);
  if (CHECK_ONLY || bad) return;                                         // (wave-uniform)
  for (long l = lane; l < n; l += 64) {
    if (t_dur && t_dur[row + l] >= 0) dur[row + l] = pt_blend(dur[row + l], pt_seconds((long)t_dur[row + l], hop, sr), w_dur[row + l]);
    if (t_energy) energy[row + l] = pt_blend_level(energy[row + l], t_energy[row + l], w_energy[row + l]);
    if (t_pitch) pitch[row + l] = pt_blend_level(pitch[row + l], t_pitch[row + l], w_pitch[row + l]);
  }
}

__global__ __launch_bounds__(64) void prosody_impose_durations_kernel(const int* __restrict__ exact, const int64_t* __restrict__ t_dur,
                                                                      const int64_t* __restrict__ lengths, float* __restrict__ dur,
                                                                      int64_t* __restrict__ durations_int, int64_t* __restrict__ totals,
                                                                      int* __restrict__ status, int L, int hop, double sr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int ex = exact[b];
  if (ex == 0 || (ex > 0 && !t_dur)) return;                             // K16's result stands
  if (ex < 0) { if (lane == 0) status[b] = PT_ST_WEIGHT; return; }
  const long n = dx_clamp_len(lengths, b, L), row = (long)b * L;
  long sum = 0;
  for (long l = lane; l < L; l += 64) {
    const long v = l < n ? max((long)t_dur[row + l], 0L) : 0;
    durations_int[row + l] = v;
    if (l < n) dur[row + l] = pt_seconds(v, hop, sr);                    // K16 zeroed the symbols below its threshold
    sum += v;
  }
  sum = dx_wave_sum(sum);
  if (lane == 0) { totals[b] = sum; status[b] = sum > 0 ? 0 : PT_ST_EMPTY; }
}

}  // namespace

extern "C" int dx_clone_pool(const float* energy, const float* log_pitch, long ldt, const int64_t* begin, const int64_t* durations,
                             const int64_t* n_rows, const float* mean_e, const float* std_e, const float* mean_p, const float* std_p,
                             float* sym_energy, float* sym_pitch, float* raw_energy, float* raw_pitch, float* self_stats, int* dropped,
                             int* status, int B, int T, int L, void* stream) {
  DX_REQUIRE(energy && log_pitch && begin && durations && n_rows && sym_energy && sym_pitch && self_stats && dropped && status, DX_ERR_ARG,
             "dx_clone_pool: null pointer");
  DX_REQUIRE((mean_e == nullptr) == (std_e == nullptr) && (mean_p == nullptr) == (std_p == nullptr), DX_ERR_ARG,
             "dx_clone_pool: a mean without its std (each pair is given whole or not at all)");
  DX_REQUIRE(B > 0 && T > 0 && L > 0 && (B == 1 || ldt >= T), DX_ERR_SHAPE, "dx_clone_pool: bad shape B=%d T=%d L=%d ldt=%ld", B, T, L, ldt);
  hipLaunchKernelGGL(clone_pool_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, energy, log_pitch, ldt, begin, durations, n_rows, mean_e,
                     std_e, mean_p, std_p, sym_energy, sym_pitch, raw_energy, raw_pitch, self_stats, dropped, status, T, L);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_prosody_impose(float* dur, float* energy, float* pitch, const int64_t* t_dur_frames, const float* t_energy,
                                 const float* t_pitch, const float* w_dur, const float* w_energy, const float* w_pitch,
                                 const int64_t* lengths, const float* dur_factors, int* exact, int B, int L, int hop_length,
                                 double sampling_rate, int validate, void* stream) {
  DX_REQUIRE(dur && energy && pitch && lengths && exact, DX_ERR_ARG, "dx_prosody_impose: null pointer");
  DX_REQUIRE((!t_dur_frames || w_dur) && (!t_energy || w_energy) && (!t_pitch || w_pitch), DX_ERR_ARG,
             "dx_prosody_impose: a target without its weights");
  DX_REQUIRE(B > 0 && L > 0 && hop_length > 0 && sampling_rate > 0, DX_ERR_SHAPE, "dx_prosody_impose: bad shape B=%d L=%d hop_length=%d", B, L,
             hop_length);
  if (validate) {
    hipLaunchKernelGGL(prosody_impose_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, dur, energy, pitch, t_dur_frames, t_energy,
                       t_pitch, w_dur, w_energy, w_pitch, lengths, dur_factors, exact, L, hop_length, sampling_rate);
    DX_LAUNCH_CHECK();
    std::vector<int> flags((size_t)B);
    hipError_t err = hipMemcpyAsync(flags.data(), exact, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (err == hipSuccess) err = hipStreamSynchronize((hipStream_t)stream);
    DX_REQUIRE(err == hipSuccess, DX_ERR_LAUNCH, "dx_prosody_impose: reading the weight check back failed: %s", hipGetErrorString(err));
    for (int b = 0; b < B; ++b)
      DX_REQUIRE(flags[b] >= 0, DX_ERR_ARG, "dx_prosody_impose: row %d has a weight outside [0, 1]", b);
  }
  hipLaunchKernelGGL(prosody_impose_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, dur, energy, pitch, t_dur_frames, t_energy,
                     t_pitch, w_dur, w_energy, w_pitch, lengths, dur_factors, exact, L, hop_length, sampling_rate);
  DX_LAUNCH_CHECK();
  return DX_OK;
}

extern "C" int dx_prosody_impose_durations(const int* exact, const int64_t* t_dur_frames, const int64_t* lengths, float* dur,
                                           int64_t* durations_int, int64_t* totals, int* status, int B, int L, int hop_length,
                                           double sampling_rate, void* stream) {
  DX_REQUIRE(exact && lengths && dur && durations_int && totals && status, DX_ERR_ARG, "dx_prosody_impose_durations: null pointer");
  DX_REQUIRE(B > 0 && L > 0 && hop_length > 0 && sampling_rate > 0, DX_ERR_SHAPE, "dx_prosody_impose_durations: bad shape B=%d L=%d", B, L);
  // without duration targets no row can be frame-exact; the launch still turns a bad weight (exact < 0) into its status
  hipLaunchKernelGGL(prosody_impose_durations_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, exact, t_dur_frames, lengths, dur,
                     durations_int, totals, status, L, hop_length, sampling_rate);
  DX_LAUNCH_CHECK();
  return DX_OK;
}
